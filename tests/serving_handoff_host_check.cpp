// serving_handoff_host_check.cpp -- the host side of the serving threads, without a GPU: the completion hand-off, the
// callers-inside guard and the guarded loop body of the-algorithm_amd/csrc/handoff.h, and the micro-batching queue of
// request_queue.h with a fake runner in place of the GPU call.  Stand-alone (its own main, nothing of the library linked);
// tests/test_serving_handoff_cpu.py builds it three ways and runs each: under the thread sanitizer, under the address and
// undefined-behaviour sanitizers, and plain with -DALLOC_FAULTS, where a replaced operator new fails the k-th allocation of
// a submit.  At most 16 threads of its own at a time (plus a queue's dispatchers).
#if defined(__SANITIZE_THREAD__) && __has_include(<bits/c++config.h>)
// The thread sanitizer's runtime of GCC 11 does not know pthread_cond_clockwait, which is what libstdc++ makes of a timed wait
// on the steady clock (the dispatchers' deadline wait): it then believes the mutex still held and reports races that are not
// there.  Without this macro libstdc++ waits by pthread_cond_timedwait, which every runtime knows.  Before any other include.
#include <bits/c++config.h>
#undef _GLIBCXX_USE_PTHREAD_COND_CLOCKWAIT
#endif
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "handoff.h"
#include "request_queue.h"

using request_queue::Batch;
using request_queue::Queue;
using request_queue::Status;

namespace {

std::atomic<int> failures{0};
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (failures.fetch_add(1) < 20) {                    \
        std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
        std::printf(__VA_ARGS__);                          \
        std::printf("\n");                                 \
      }                                                    \
    }                                                      \
  } while (0)

// ends the program when a step that must finish does not (the dispatcher that spins forever on `pending`, a lost wake-up)
struct Watchdog {
  std::mutex m;
  std::condition_variable cv;
  bool done = false;
  std::thread th;
  Watchdog(const char *what, int seconds) {
    th = std::thread([this, what, seconds] {
      std::unique_lock<std::mutex> lk(m);
      if (!cv.wait_for(lk, std::chrono::seconds(seconds), [this] { return done; })) {
        std::printf("FAILED: watchdog: %s did not finish within %d s\n", what, seconds);
        std::fflush(stdout);
        std::_Exit(3);
      }
    });
  }
  ~Watchdog() {
    {
      std::lock_guard<std::mutex> lk(m);
      done = true;
      cv.notify_all();
    }
    th.join();
  }
};

// ---------------------------------------------------------------------------------------------------------------------------
// a request of the check, and the fake runner's answer to it

constexpr int kRows = 6;  // maxNumResults of every request here

struct Call {
  std::vector<int32_t> cids;
  std::vector<double> scores;
  int64_t ids[kRows + 1];
  double sc[kRows + 1];
  int32_t count = -1, msz = -1;
  int64_t ticket = 0;
  Call(int n_emb, int seed) : cids((size_t)n_emb), scores((size_t)n_emb) {
    for (int i = 0; i < n_emb; i++) {
      cids[(size_t)i] = seed * 31 + i;
      scores[(size_t)i] = 0.5 + seed + i * 0.25;
    }
    for (int i = 0; i <= kRows; i++) { ids[i] = -7; sc[i] = -7.0; }
  }
};

int64_t emb_sum(const int32_t *c, const double *s, int64_t n) {
  double t = 0;
  for (int64_t i = 0; i < n; i++) t += c[i] * s[i];
  return (int64_t)t;
}
// rows derived from the request's ticket and embedding, as the batch holds them
int64_t row_id(int64_t ticket, int64_t esum, int i) { return ticket * 1000003 + esum * 7 + i; }
double row_score(int64_t ticket, int64_t esum, int i) { return (double)esum - i * 0.5 + (double)(ticket % 97); }

struct FakeGpu {
  int fail_every = 0;        // every N-th batch fails with SANN_EDEVICE and a message that names the batch
  int throw_pattern = 0;     // 1: batch % 3 == 1 throws bad_alloc, batch % 3 == 2 throws runtime_error
  std::atomic<int64_t> n_batches{0}, n_requests{0};
  std::vector<std::atomic<int64_t>> batch_of;  // ticket -> 1-based batch number
  explicit FakeGpu(size_t max_ticket) : batch_of(max_ticket + 1) {
    for (auto &b : batch_of) b.store(0);
  }
  static std::string failure_text(int64_t bn) { return "fake device failure in batch " + std::to_string(bn); }
  void run(int, Batch &bt) {
    const int64_t bn = n_batches.fetch_add(1) + 1;
    const size_t nq = bt.reqs.size();
    n_requests.fetch_add((int64_t)nq);
    for (size_t q = 0; q < nq; q++) batch_of[(size_t)bt.reqs[q]->ticket].store(bn);
    std::this_thread::sleep_for(std::chrono::microseconds((bn * 37) % 201));
    if (throw_pattern == 1 && bn % 3 == 1) throw std::bad_alloc();
    if (throw_pattern == 1 && bn % 3 == 2) throw std::runtime_error("boom");
    const bool fail = fail_every > 0 && bn % fail_every == 0;
    CHECK(bt.emb_offsets.size() == nq + 1 && bt.src.size() == nq && bt.now.size() == nq && bt.cfgs.size() == nq && bt.has_src.size() == nq,
          "batch %lld: per-request vectors disagree", (long long)bn);
    for (size_t q = 0; q < nq; q++) {
      request_queue::Request &r = *bt.reqs[q];
      if (fail) {
        r.status = SANN_EDEVICE;
        r.message = failure_text(bn);
        continue;
      }
      const int64_t lo = bt.emb_offsets[q], hi = bt.emb_offsets[q + 1];
      const int64_t es = emb_sum(bt.emb.cids.get() + lo, bt.emb.scores.get() + lo, hi - lo);
      CHECK(bt.now[q] == es * 3 + 1 && bt.has_src[q] == (es & 1) && bt.src[q] == (bt.has_src[q] ? es + 5 : 0), "batch %lld: a request's now / source tweet is another's", (long long)bn);
      const int c = bt.cfgs[q].max_num_results;
      for (int i = 0; i < c; i++) {
        r.out_ids[i] = row_id(r.ticket, es, i);
        r.out_scores[i] = row_score(r.ticket, es, i);
      }
      *r.out_count = c;
      *r.out_map_size = (int32_t)(hi - lo);
      r.status = SANN_OK;
    }
  }
};

sann_config_t config_of() {
  sann_config_t c{};
  c.max_num_results = kRows;
  c.ann_algorithm = SANN_ALG_COSINE;
  return c;
}

// every request carries a Time.now and a source tweet derived from its own embedding: the fake checks that a batch kept them together
Status submit(Queue &q, Call &c) {
  const sann_config_t cfg = config_of();
  const int64_t es = emb_sum(c.cids.data(), c.scores.data(), (int64_t)c.cids.size());
  return q.submit(es * 3 + 1, (int32_t)c.cids.size(), c.cids.data(), c.scores.data(), es + 5, (int32_t)(es & 1), &cfg, kRows, c.ids, c.sc,
                  &c.count, &c.msz, &c.ticket);
}

// the answer of a collected request: exactly its own rows, or exactly its batch's status and message
void check_answer(const Call &c, const Status &s, const FakeGpu &gpu) {
  const int64_t bn = gpu.batch_of[(size_t)c.ticket].load();
  CHECK(bn > 0, "ticket %lld collected, but no batch ran it", (long long)c.ticket);
  const bool should_fail = gpu.fail_every > 0 && bn % gpu.fail_every == 0;
  if (should_fail) {
    CHECK(s.code == SANN_EDEVICE && s.message == FakeGpu::failure_text(bn), "ticket %lld of failed batch %lld: status %d \"%s\"",
          (long long)c.ticket, (long long)bn, s.code, s.message.c_str());
    CHECK(c.count == -1 && c.ids[0] == -7, "ticket %lld: rows written for a failed batch", (long long)c.ticket);
    return;
  }
  CHECK(s.code == SANN_OK, "ticket %lld: status %d \"%s\"", (long long)c.ticket, s.code, s.message.c_str());
  const int64_t es = emb_sum(c.cids.data(), c.scores.data(), (int64_t)c.cids.size());
  bool own = c.count == kRows && c.msz == (int32_t)c.cids.size() && c.ids[kRows] == -7 && c.sc[kRows] == -7.0;
  for (int i = 0; i < kRows && own; i++) own = c.ids[i] == row_id(c.ticket, es, i) && c.sc[i] == row_score(c.ticket, es, i);
  CHECK(own, "ticket %lld: not its own rows", (long long)c.ticket);
}

// ---------------------------------------------------------------------------------------------------------------------------
// 1. A completion in the waiter's own stack frame (the engine's job): publish, wait, leave the frame; the next round's frame
//    lies where this one lay.  A completer that touches the completion after a waiter could see `done` is a use after scope
//    (address sanitizer) and a race with the destructor (thread sanitizer).
constexpr int kStackRounds = 40000;

void stack_owned_completion() {
  std::atomic<handoff::Completion *> slot{nullptr};
  std::thread completer([&] {
    for (int i = 0; i < kStackRounds; i++) {
      handoff::Completion *c;
      while (!(c = slot.exchange(nullptr, std::memory_order_acquire))) std::this_thread::yield();
      c->complete(i, i % 5 == 0 ? std::string("the message of round ") + std::to_string(i) : std::string());
    }
  });
  std::thread waiter([&] {
    for (int i = 0; i < kStackRounds; i++) {
      handoff::Completion c;
      slot.store(&c, std::memory_order_release);
      if (i % 3 == 0) while (!c.poll()) std::this_thread::yield();
      else c.wait();
      CHECK(c.status() == i, "round %d: status %d", i, c.status());
      CHECK(c.message() == (i % 5 == 0 ? std::string("the message of round ") + std::to_string(i) : std::string()), "round %d: message", i);
    }
  });
  waiter.join();
  completer.join();
}

// 2. One completion behind a shared_ptr (the batcher's batch), sixteen threads waiting and polling on it.
void shared_completion_many_waiters() {
  for (int round = 0; round < 300; round++) {
    auto c = std::make_shared<handoff::Completion>();
    std::atomic<int> woken{0};
    std::vector<std::thread> ths;
    for (int t = 0; t < 16; t++)
      ths.emplace_back([c, t, round, &woken] {
        if (t % 2) while (!c->poll()) std::this_thread::yield();
        else c->wait();
        CHECK(c->status() == round && c->message() == "shared", "round %d thread %d", round, t);
        woken++;
      });
    c->complete(round, "shared");
    c.reset();  // (the waiters hold it now)
    for (auto &th : ths) th.join();
    CHECK(woken == 16, "round %d: %d of 16 woken", round, woken.load());
  }
}

// 3. The queue itself with the fake runner: sixteen callers, three call shapes.
void queue_under_load(int max_batch, int max_wait_us, int per_thread, bool one_large_embedding) {
  constexpr int kThreads = 16;
  const int total = kThreads * per_thread;
  FakeGpu gpu((size_t)total);
  gpu.fail_every = 5;
  Queue::Options o;
  o.max_batch = max_batch;
  o.max_wait_us = max_wait_us;
  o.n_dispatchers = 3;
  Queue q(o, [&gpu](int d, Batch &bt) { gpu.run(d, bt); });
  // shape 2 hands the submitted call to the next thread, which collects it after its own calls
  std::mutex box_mu[kThreads];
  std::vector<std::unique_ptr<Call>> box[kThreads];
  std::atomic<int> submitting{kThreads};
  auto collect_and_check = [&](Call &c, bool block) {
    Status s;
    if (block) s = q.collect(c.ticket, true, nullptr);
    else
      for (;;) {
        int32_t done = 0;
        s = q.collect(c.ticket, false, &done);
        if (done || s.code != SANN_OK) break;
        std::this_thread::yield();
      }
    check_answer(c, s, gpu);
    const Status again = q.collect(c.ticket, block, nullptr);
    CHECK(again.code == SANN_EINVAL, "ticket %lld collected twice: status %d", (long long)c.ticket, again.code);
  };
  std::vector<std::thread> ths;
  for (int t = 0; t < kThreads; t++)
    ths.emplace_back([&, t] {
      for (int i = 0; i < per_thread; i++) {
        // 30-entry embeddings (a 4-request batch's buffer of 256 closes by size, not by count); one of 700 outgrows the buffer
        const int n_emb = one_large_embedding && t == 3 && i == per_thread / 2 ? 700 : (t + i) % 11 == 0 ? 0 : 30;
        std::unique_ptr<Call> c(new Call(n_emb, t * 1000 + i));
        const Status s = submit(q, *c);
        CHECK(s.code == SANN_OK, "submit: %d \"%s\"", s.code, s.message.c_str());
        if (s.code != SANN_OK) continue;
        const int shape = (t + i) % 3;
        if (shape == 2) {
          std::lock_guard<std::mutex> lk(box_mu[(t + 1) % kThreads]);
          box[(t + 1) % kThreads].push_back(std::move(c));
        } else {
          collect_and_check(*c, shape == 0);
        }
      }
      submitting--;
      while (submitting.load() != 0) std::this_thread::yield();
      std::vector<std::unique_ptr<Call>> mine;
      {
        std::lock_guard<std::mutex> lk(box_mu[t]);
        mine.swap(box[t]);
      }
      for (size_t i = 0; i < mine.size(); i++) collect_and_check(*mine[i], i % 2 == 0);
    });
  for (auto &th : ths) th.join();
  const sann_batcher_stats_t st = q.stats();
  const Queue::Observed ob = q.observe();
  CHECK(st.n_requests == total && st.n_requests == gpu.n_requests.load(), "requests %lld, batches held %lld, submitted %d",
        (long long)st.n_requests, (long long)gpu.n_requests.load(), total);
  CHECK(st.n_batches == gpu.n_batches.load() && st.n_closed_full + st.n_closed_by_deadline == st.n_batches,
        "batches %lld run %lld, closed full %lld + by deadline %lld", (long long)st.n_batches, (long long)gpu.n_batches.load(),
        (long long)st.n_closed_full, (long long)st.n_closed_by_deadline);
  CHECK(st.max_batch <= max_batch && st.max_batch >= 1, "max batch %lld", (long long)st.max_batch);
  CHECK(ob.tickets == 0 && ob.open_pending == 0 && ob.ready == 0 && ob.inside == 0 && ob.in_lock_throws == 0,
        "left behind: %zu tickets, pending %d, %zu ready, %d inside", ob.tickets, ob.open_pending, ob.ready, ob.inside);
  std::printf("queue max_batch %d max_wait_us %d: %lld requests in %lld batches (%lld full, %lld by deadline, largest %lld)\n", max_batch,
              max_wait_us, (long long)st.n_requests, (long long)st.n_batches, (long long)st.n_closed_full,
              (long long)st.n_closed_by_deadline, (long long)st.max_batch);
}

// 4. Destroy with callers inside: eight threads blocked in a wait that only a deadline far away (or the destroy) ends; the
//    queue is deleted from a ninth.  Each gets its answer; the delete returns only when they have left the queue (touching
//    it later would be a use after free).
void destroy_with_callers_inside() {
  FakeGpu gpu(8);
  Queue::Options o;
  o.max_batch = 100;
  o.max_wait_us = 30 * 1000 * 1000;
  o.n_dispatchers = 2;
  Queue *q = new Queue(o, [&gpu](int d, Batch &bt) { gpu.run(d, bt); });
  Watchdog dog("destroy with callers inside", 10);
  std::atomic<int> answered{0};
  std::vector<std::thread> ths;
  for (int t = 0; t < 8; t++)
    ths.emplace_back([&, t] {
      Call c(30, t);
      const Status s = submit(*q, c);
      CHECK(s.code == SANN_OK, "submit: %d", s.code);
      const Status w = q->collect(c.ticket, true, nullptr);
      check_answer(c, w, gpu);
      answered++;
    });
  while (q->observe().inside != 8) std::this_thread::yield();
  std::thread ninth([&] { delete q; });
  ninth.join();
  for (auto &th : ths) th.join();
  CHECK(answered == 8 && gpu.n_requests == 8, "%d of 8 callers answered", answered.load());
}

// 5. A runner that throws: the batch's requests get the classified status, the dispatcher serves the next batch, and the
//    queue still shuts down.
void runner_that_throws() {
  constexpr int n = 24;
  FakeGpu gpu(n);
  gpu.throw_pattern = 1;
  Queue::Options o;
  o.max_batch = 2;
  o.max_wait_us = 200;
  o.n_dispatchers = 2;
  int seen[3] = {0, 0, 0};
  {
    Queue q(o, [&gpu](int d, Batch &bt) { gpu.run(d, bt); });
    Watchdog dog("a runner that throws", 10);
    std::vector<std::unique_ptr<Call>> calls;
    for (int i = 0; i < n; i++) {
      calls.emplace_back(new Call(30, i));
      CHECK(submit(q, *calls.back()).code == SANN_OK, "submit %d", i);
    }
    for (auto &c : calls) {
      const Status s = q.collect(c->ticket, true, nullptr);
      const int64_t bn = gpu.batch_of[(size_t)c->ticket].load();
      seen[bn % 3]++;
      if (bn % 3 == 1) CHECK(s.code == SANN_ENOMEM && s.message == "out of host memory", "batch %lld: %d \"%s\"", (long long)bn, s.code, s.message.c_str());
      else if (bn % 3 == 2) CHECK(s.code == SANN_EINTERNAL && s.message == "internal error: boom", "batch %lld: %d \"%s\"", (long long)bn, s.code, s.message.c_str());
      else check_answer(*c, s, gpu);
    }
    CHECK(q.observe().tickets == 0, "tickets left");
  }
  CHECK(seen[0] > 0 && seen[1] > 0 && seen[2] > 0, "batches answered / bad_alloc / runtime_error: %d %d %d", seen[0], seen[1], seen[2]);
}

// The guarded loop body on its own: the body's exception reaches the action classified; no exception, no action.
void guarded_classifies() {
  int st = 0;
  std::string msg;
  auto held = [&](int s, const char *m) { st = s; msg = m; };
  handoff::guarded(SANN_ENOMEM, SANN_EINTERNAL, [] {}, held);
  CHECK(st == 0 && msg.empty(), "action without an exception");
  handoff::guarded(SANN_ENOMEM, SANN_EINTERNAL, [] { throw std::bad_alloc(); }, held);
  CHECK(st == SANN_ENOMEM && msg == "out of host memory", "bad_alloc: %d \"%s\"", st, msg.c_str());
  handoff::guarded(SANN_ENOMEM, SANN_EINTERNAL, [] { throw std::length_error("too long"); }, held);
  CHECK(st == SANN_EINTERNAL && msg == "internal error: too long", "length_error: %d \"%s\"", st, msg.c_str());
  handoff::guarded(SANN_ENOMEM, SANN_EINTERNAL, [] { throw 5; }, held);
  CHECK(st == SANN_EINTERNAL && msg == "internal error", "int: %d \"%s\"", st, msg.c_str());
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
#ifdef ALLOC_FAULTS
// The k-th allocation from now on, on this thread, fails (once).
namespace {
thread_local long fault_countdown = -1;
thread_local bool fault_fired = false;
void arm(long k) { fault_fired = false; fault_countdown = k; }
bool disarm() { fault_countdown = -1; return fault_fired; }
void *allocate(std::size_t n) {
  if (fault_countdown == 0) {
    fault_countdown = -1;
    fault_fired = true;
    throw std::bad_alloc();
  }
  if (fault_countdown > 0) fault_countdown--;
  void *p = std::malloc(n ? n : 1);
  if (!p) throw std::bad_alloc();
  return p;
}
}  // namespace
void *operator new(std::size_t n) { return allocate(n); }
void *operator new[](std::size_t n) { return allocate(n); }
void operator delete(void *p) noexcept { std::free(p); }
void operator delete[](void *p) noexcept { std::free(p); }
void operator delete(void *p, std::size_t) noexcept { std::free(p); }
void operator delete[](void *p, std::size_t) noexcept { std::free(p); }

namespace {

// A submit whose k-th allocation fails, k = 0, 1, 2, ...: SANN_ENOMEM, and the queue as it was -- no ticket left in the table
// (the parent left it), nothing pending on the open batch (the parent left `pending` up, and the dispatcher spun on it for
// ever).  On a queue with room in its open batch, a submit allocates in front of the lock only -- the Request (k = 0), its
// node in the ticket table (k = 1) and, for the first ticket of a shard, the table's buckets (k = 2) -- so those are the sites
// that fail, and in_lock_throws stays 0.
void submit_sweep_open_batch_with_room() {
  FakeGpu gpu(64);
  Queue::Options o;
  o.max_batch = 64;
  o.max_wait_us = 1000;
  o.n_dispatchers = 2;
  Queue q(o, [&gpu](int d, Batch &bt) { gpu.run(d, bt); });
  int failed = 0;
  std::string sites;
  for (long k = 0;; k++) {
    CHECK(k < 32, "a submit still fails at its 32nd allocation");
    if (k >= 32) break;
    Call c(30, (int)k);
    const Queue::Observed before = q.observe();
    arm(k);
    const Status s = submit(q, c);
    const bool fired = disarm();
    const Queue::Observed after = q.observe();
    if (!fired) {
      CHECK(s.code == SANN_OK, "submit with no fault: %d \"%s\"", s.code, s.message.c_str());
      CHECK(q.collect(c.ticket, true, nullptr).code == SANN_OK, "the unfaulted submit's wait");
      break;
    }
    failed++;
    sites += " k=" + std::to_string(k);
    CHECK(s.code == SANN_ENOMEM, "allocation %ld failed: status %d \"%s\"", k, s.code, s.message.c_str());
    CHECK(after.tickets == before.tickets, "allocation %ld failed: %zu tickets, %zu before", k, after.tickets, before.tickets);
    CHECK(after.open_pending == 0, "allocation %ld failed: pending %d", k, after.open_pending);
    CHECK(after.in_lock_throws == 0, "allocation %ld failed inside the queue's lock", k);
  }
  CHECK(failed >= 1, "no allocation of a submit failed: the sweep checked nothing");
  std::printf("submit, open batch with room: failing allocation sites%s (Request, ticket node, ticket buckets), none under the lock\n", sites.c_str());
  // and the queue still serves (a `pending` left up would hang this wait)
  Watchdog dog("submit + wait after failed submits", 2);
  Call c(30, 99);
  Status s = submit(q, c);
  CHECK(s.code == SANN_OK, "submit after the sweep: %d", s.code);
  s = q.collect(c.ticket, true, nullptr);
  CHECK(s.code == SANN_OK && c.count == kRows, "wait after the sweep: %d", s.code);
}

// The same sweep over the submit that FILLS a batch (max_batch = 2, second request): closing it needs a new Batch and room in
// the ready queue, under the lock.  The request is in the batch by then, so the submit succeeds whatever fails there, and the
// batch leaves with the next submit or its deadline.  Either way: both requests are answered.
void submit_sweep_closing_submit() {
  int failed = 0, fired_but_ok = 0;
  for (long k = 0;; k++) {
    CHECK(k < 64, "a closing submit still meets a fault at its 64th allocation");
    if (k >= 64) break;
    FakeGpu gpu(8);
    Queue::Options o;
    o.max_batch = 2;
    o.max_wait_us = 20000;
    o.n_dispatchers = 1;
    Queue q(o, [&gpu](int d, Batch &bt) { gpu.run(d, bt); });
    Call a(30, 1), b(30, 2);
    CHECK(submit(q, a).code == SANN_OK, "first submit");
    arm(k);
    const Status s = submit(q, b);
    const bool fired = disarm();
    const Queue::Observed after = q.observe();
    Watchdog dog("waits after a faulted closing submit", 2);
    if (s.code != SANN_OK) {
      failed++;
      CHECK(fired && s.code == SANN_ENOMEM && after.tickets <= 1, "closing submit, allocation %ld: status %d, %zu tickets", k, s.code, after.tickets);
    } else {
      fired_but_ok += fired;
      CHECK(q.collect(b.ticket, true, nullptr).code == SANN_OK && b.count == kRows, "closing submit, allocation %ld: second request's wait", k);
    }
    CHECK(q.collect(a.ticket, true, nullptr).code == SANN_OK && a.count == kRows, "closing submit, allocation %ld: first request's wait", k);
    if (!fired) break;
  }
  CHECK(failed >= 1 && fired_but_ok >= 1, "closing submit: %d failed, %d succeeded over a failed close", failed, fired_but_ok);
  std::printf("submit that fills a batch: %d failed in front of the lock, %d succeeded although the close found no memory\n", failed, fired_but_ok);
}

}  // namespace
#endif

int main() {
#ifdef ALLOC_FAULTS
  submit_sweep_open_batch_with_room();
  submit_sweep_closing_submit();
#endif
  guarded_classifies();
  stack_owned_completion();
  shared_completion_many_waiters();
  queue_under_load(/* max_batch */ 4, /* max_wait_us */ 2000, /* per thread */ 60, /* one large embedding */ true);
  queue_under_load(256, 1, 120, false);
  queue_under_load(1000, 3000, 60, false);
  destroy_with_callers_inside();
  runner_that_throws();
  std::printf("%s: %d stack-owned rounds, 300 shared rounds, 3 queue loads, destroy with 8 inside, throwing runner, %d failures\n",
              failures ? "FAILED" : "ok", kStackRounds, failures.load());
  return failures ? 1 : 0;
}
