// request_queue.h -- the micro-batching queue of sann_batcher.hip without its GPU call (host code, no HIP include: it is
// compiled and hammered under the host sanitizers by tests/serving_handoff_host_check.cpp).
//
//   submit            copies the request (embedding, config, source tweet, Time.now) into the OPEN batch and returns a ticket
//   a batch closes    when it holds max_batch requests, or max_wait_us after its first request arrived
//   dispatcher d      takes a closed batch and calls run(d, batch): the ONE thing done on the GPU, "run this closed batch and
//                     give every request its status and rows" (sann_batcher.hip's runner; a fake in the host check)
//   collect           the caller's side of sann_wait / sann_poll
//
// Who owns what: the queue owns its batches (open, ready, spare, or in a dispatcher's hands); a Request is shared between its
// batch, the ticket table and a caller inside collect(); a batch's Completion is shared between the batch and its requests.
// shutdown() runs what was submitted, joins the dispatchers, and waits for the callers inside collect() to leave: only then
// may the queue be deleted.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/simclusters_ann.h"
#include "abi_guard.h"
#include "handoff.h"

namespace request_queue {

using Clock = std::chrono::steady_clock;

struct Status {
  int code = SANN_OK;
  std::string message;
};

struct Request {
  int64_t ticket = 0;
  std::shared_ptr<handoff::Completion> done;  // its batch's: the callers of a batch sleep there, not on a queue-wide condition
  int32_t out_cap = 0;
  int64_t *out_ids = nullptr;
  double *out_scores = nullptr;
  int32_t *out_count = nullptr, *out_map_size = nullptr;
  int status = SANN_OK;
  std::string message;
};

// The embeddings of a batch's requests, back to back.  Plain buffers, not std::vector: a submitter RESERVES its stretch under the
// queue's lock and copies into it after letting the lock go (`pending` counts the copies still running; the dispatcher waits
// for zero before it reads), so growing must never move the buffer under a writer -- a batch that would outgrow its buffer is
// closed instead, and only an EMPTY batch grows.
struct EmbBuf {
  std::unique_ptr<int32_t[]> cids;
  std::unique_ptr<double[]> scores;
  size_t size = 0, cap = 0;
  void reserve_empty(size_t n) {  // (size == 0: nobody holds a pointer into the old buffers)
    if (n <= cap) return;
    std::unique_ptr<int32_t[]> c(new int32_t[n]);
    scores.reset(new double[n]);
    cids = std::move(c);
    cap = n;
  }
};

struct Batch {
  std::shared_ptr<handoff::Completion> done;
  std::vector<int64_t> emb_offsets;
  EmbBuf emb;
  std::atomic<int> pending{0};
  std::vector<int64_t> src, now;
  std::vector<uint8_t> has_src;
  std::vector<sann_config_t> cfgs;
  std::vector<std::shared_ptr<Request>> reqs;
  Clock::time_point deadline;
  int kmax = 1;
  // Every per-request vector holds max_batch entries from the start: a submit, under the queue's lock, allocates nothing.
  explicit Batch(size_t max_batch) {
    emb_offsets.reserve(max_batch + 1);
    src.reserve(max_batch); now.reserve(max_batch); has_src.reserve(max_batch); cfgs.reserve(max_batch); reqs.reserve(max_batch);
    emb.reserve_empty(max_batch * 64);
    recycle();
  }
  void recycle() {  // (capacities stay)
    done = std::make_shared<handoff::Completion>();
    emb_offsets.assign(1, 0);
    emb.size = 0;
    src.clear(); now.clear(); has_src.clear(); cfgs.clear(); reqs.clear();
    kmax = 1;
  }
};

class Queue {
 public:
  struct Options {
    int32_t variant = 0, max_batch = 1024, max_wait_us = 500, n_dispatchers = 3;
  };
  // run(d, batch), on dispatcher thread d: sets status (and message, or the rows) of every request of the batch.  It may throw.
  using Runner = std::function<void(int, Batch &)>;
  // what a check program needs to see
  struct Observed {
    size_t tickets = 0;       // submitted, not yet collected
    int open_pending = 0;     // embedding copies into the open batch still running
    size_t ready = 0, spare = 0;
    int inside = 0;           // callers inside collect()
    int64_t in_lock_throws = 0;  // submits that failed by an exception while they held the queue's lock
  };

  Queue(const Options &o, Runner run) : opt_(o), run_(std::move(run)) {
    spare_.reserve(kSpare);
    open_.reset(new Batch((size_t)opt_.max_batch));
    try {
      for (int d = 0; d < opt_.n_dispatchers; d++) workers_.emplace_back([this, d] { dispatcher(d); });
    } catch (...) {
      shutdown();
      throw;
    }
  }
  ~Queue() { shutdown(); }
  Queue(const Queue &) = delete;
  Queue &operator=(const Queue &) = delete;

  // Runs whatever was submitted, stops the dispatchers, and returns when no caller is inside collect() any more: a caller that
  // was blocked there has its answer and has left.  Tickets nobody collected are dropped with the object.
  void shutdown() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      stop_ = true;
    }
    cv_work_.notify_all();
    for (auto &t : workers_)
      if (t.joinable()) t.join();
    inside_.wait_empty();
  }

  Status submit(int64_t now_ms, int32_t n_embedding, const int32_t *cluster_ids, const double *scores, int64_t source_tweet_id,
                int32_t has_source_tweet, const sann_config_t *config, int32_t out_capacity, int64_t *out_ids, double *out_scores,
                int32_t *out_count, int32_t *out_map_size, int64_t *ticket) noexcept {
    bool in_lock = false;
    try {
      if (!config || !ticket) return {SANN_EINVAL, "NULL argument"};
      if (n_embedding < 0 || (n_embedding > 0 && (!cluster_ids || !scores))) return {SANN_EINVAL, "bad embedding"};
      if (opt_.variant == SANN_VARIANT_LEGACY) {
        if (config->ann_algorithm != SANN_ALG_DOT_PRODUCT && config->ann_algorithm != SANN_ALG_COSINE && config->ann_algorithm != SANN_ALG_LOG_COSINE)
          return {SANN_EINVAL, "legacy variant: ann_algorithm must be dot product, cosine or log cosine"};
        if (config->max_num_results > 1000) return {SANN_ELIMIT, "legacy variant: max_num_results above 1000"};
      }
      const int k = config->max_num_results < 1000 ? (config->max_num_results < 0 ? 0 : config->max_num_results) : 1000;
      if (out_capacity < k || (k > 0 && (!out_ids || !out_scores))) return {SANN_EINVAL, "out_capacity must hold min(maxNumResults, 1000) results"};
      // everything that allocates comes first: the request, and its entry in the ticket table (taken out again on every failing exit)
      std::shared_ptr<Request> r = std::make_shared<Request>();
      r->ticket = next_ticket_.fetch_add(1, std::memory_order_relaxed);
      r->out_cap = out_capacity;
      r->out_ids = out_ids;
      r->out_scores = out_scores;
      r->out_count = out_count;
      r->out_map_size = out_map_size;
      TicketShard &sh = shard_of(r->ticket);
      {
        std::lock_guard<std::mutex> lk(sh.mu);
        sh.map.emplace(r->ticket, r);
      }
      struct Unwind {
        TicketShard &sh;
        int64_t ticket;
        bool keep = false;
        ~Unwind() {
          if (keep) return;
          std::lock_guard<std::mutex> lk(sh.mu);
          sh.map.erase(ticket);
        }
      } unwind{sh, r->ticket};
      Batch *copy_to = nullptr;
      size_t copy_at = 0;
      {
        std::lock_guard<std::mutex> lk(mu_);
        in_lock = true;
        if (stop_) {
          in_lock = false;
          return {SANN_EINVAL, "the batcher is shutting down"};
        }
        // no room for this request (its embedding would outgrow the buffer, or an earlier close failed and left the batch full):
        // close, and grow the (empty) next one.  Both may throw; nothing of this request is in a batch yet.
        if (open_->emb.size + (size_t)n_embedding > open_->emb.cap || (int)open_->reqs.size() >= opt_.max_batch) {
          if (close_open_locked()) n_full_++;
          open_->emb.reserve_empty(std::max((size_t)n_embedding * 2, (size_t)opt_.max_batch * 64));
        }
        // from here to the end of the lock nothing allocates (Batch reserved every vector), so nothing fails: `pending` goes up last
        Batch &bt = *open_;
        if (bt.reqs.empty()) bt.deadline = Clock::now() + std::chrono::microseconds(opt_.max_wait_us);
        copy_to = &bt;
        copy_at = bt.emb.size;
        bt.emb.size += (size_t)n_embedding;
        bt.emb_offsets.push_back((int64_t)bt.emb.size);
        bt.src.push_back(has_source_tweet ? source_tweet_id : 0);
        bt.has_src.push_back(has_source_tweet ? 1 : 0);
        bt.now.push_back(now_ms);
        bt.cfgs.push_back(*config);
        bt.kmax = std::max(bt.kmax, k);
        r->done = bt.done;
        bt.reqs.push_back(r);
        n_requests_++;
        bt.pending.fetch_add(1, std::memory_order_relaxed);
        const bool first = bt.reqs.size() == 1;
        if ((int)bt.reqs.size() >= opt_.max_batch) {
          // (a close that finds no memory leaves the batch open and full: the next submit or the deadline closes it)
          try { if (close_open_locked()) n_full_++; } catch (...) { if (first) cv_work_.notify_one(); }
        } else if (first) {
          cv_work_.notify_one();  // a dispatcher now has a deadline to sleep towards
        }
        in_lock = false;
      }
      unwind.keep = true;
      // the embedding itself travels outside the lock, into the stretch reserved above
      if (n_embedding > 0) {
        memcpy(copy_to->emb.cids.get() + copy_at, cluster_ids, (size_t)n_embedding * sizeof(int32_t));
        memcpy(copy_to->emb.scores.get() + copy_at, scores, (size_t)n_embedding * sizeof(double));
      }
      copy_to->pending.fetch_sub(1, std::memory_order_release);
      *ticket = r->ticket;
      return {};
    } catch (...) {
      if (in_lock) in_lock_throws_.fetch_add(1, std::memory_order_relaxed);
      return caught();
    }
  }

  // block: sann_wait; otherwise sann_poll (*done = 0 and SANN_OK while the request is still out)
  Status collect(int64_t ticket, bool block, int32_t *done) noexcept {
    handoff::Inside::Hold inside(inside_);  // first in, last out: shutdown() waits for it
    try {
      std::shared_ptr<Request> r;
      TicketShard &sh = shard_of(ticket);
      {
        std::lock_guard<std::mutex> lk(sh.mu);
        auto it = sh.map.find(ticket);
        if (it == sh.map.end()) return {SANN_EINVAL, "unknown ticket (already collected?)"};
        r = it->second;
      }
      if (block) r->done->wait();
      const bool is_done = block || r->done->poll();
      if (done) *done = is_done ? 1 : 0;
      if (!is_done) return {};
      {
        std::lock_guard<std::mutex> lk(sh.mu);
        if (sh.map.erase(ticket) == 0) return {SANN_EINVAL, "unknown ticket (already collected?)"};
      }
      if (r->status != SANN_OK) return {r->status, r->message};
      return {};
    } catch (...) {
      return caught();
    }
  }

  sann_batcher_stats_t stats() const {
    std::lock_guard<std::mutex> lk(mu_);
    sann_batcher_stats_t s{};
    s.n_requests = n_requests_;
    s.n_batches = n_batches_;
    s.n_closed_full = n_full_;
    s.n_closed_by_deadline = n_timeout_;
    s.max_batch = max_batch_seen_;
    return s;
  }

  Observed observe() const {
    Observed o;
    o.inside = inside_.count();
    for (const TicketShard &sh : tk_) {
      std::lock_guard<std::mutex> lk(sh.mu);
      o.tickets += sh.map.size();
    }
    std::lock_guard<std::mutex> lk(mu_);
    o.open_pending = open_->pending.load(std::memory_order_acquire);
    o.ready = ready_.size();
    o.spare = spare_.size();
    o.in_lock_throws = in_lock_throws_.load(std::memory_order_relaxed);
    return o;
  }

 private:
  static constexpr size_t kSpare = 8;
  // the ticket table has locks of its own (collecting answers does not hold up submissions), sixteen of them: a ticket's
  // shard is its low bits, so callers that submit and collect at a million requests a second rarely meet
  static constexpr int TK_SHARDS = 16;
  struct TicketShard {
    mutable std::mutex mu;
    std::unordered_map<int64_t, std::shared_ptr<Request>> map;
  };
  TicketShard &shard_of(int64_t ticket) { return tk_[(size_t)ticket & (TK_SHARDS - 1)]; }

  static Status caught() noexcept {  // (inside a catch block) the exception as the entry points' ABI_CATCH classifies it
    Status s;
    s.code = abi_guard::caught([&s](int code, const std::string &msg) { s.message = msg; return code; }, SANN_ENOMEM, SANN_EINTERNAL);
    return s;
  }

  // open -> ready (mu_ held); false: the open batch is empty and stays.  All or nothing: when it throws, nothing has changed.
  bool close_open_locked() {
    if (open_->reqs.empty()) return false;
    std::unique_ptr<Batch> next;
    if (!spare_.empty()) { next = std::move(spare_.back()); spare_.pop_back(); }
    else next.reset(new Batch((size_t)opt_.max_batch));
    try {
      ready_.push_back(std::move(open_));  // (strong guarantee: open_ is moved from only when the deque has room)
    } catch (...) {
      spare_.push_back(std::move(next));  // (reserved)
      throw;
    }
    open_ = std::move(next);
    cv_work_.notify_one();
    return true;
  }

  void dispatcher(int d) {
    std::unique_lock<std::mutex> lk(mu_);
    bool finished = false;
    while (!finished) {
      std::unique_ptr<Batch> bt;  // the batch in this thread's hands
      bool answered = false;      // its requests have their answers and its completion is complete
      handoff::guarded(SANN_ENOMEM, SANN_EINTERNAL, [&] {
        // a closed batch, or the open batch's deadline, or the end
        while (!stop_ && ready_.empty()) {
          if (!open_->reqs.empty()) {
            if (Clock::now() >= open_->deadline) {
              if (close_open_locked()) n_timeout_++;
              break;
            }
            cv_work_.wait_until(lk, open_->deadline);
          } else {
            cv_work_.wait(lk);
          }
        }
        if (ready_.empty()) {
          if (stop_) {
            if (open_->reqs.empty()) { finished = true; return; }
            close_open_locked();  // drain what was submitted before the stop
          }
          if (ready_.empty()) return;
        }
        bt = std::move(ready_.front());
        ready_.pop_front();
        n_batches_++;
        max_batch_seen_ = std::max<int64_t>(max_batch_seen_, (int64_t)bt->reqs.size());
        lk.unlock();
        while (bt->pending.load(std::memory_order_acquire) != 0) std::this_thread::yield();  // (submitters still copying their embeddings in)
        run_(d, *bt);
        bt->done->complete();
        answered = true;
        bt->recycle();
        lk.lock();
        if (spare_.size() < kSpare) spare_.push_back(std::move(bt));
      }, [&](int status, const char *msg) {
        // the batch's requests fail with the classified status (unless they already have their answers); the batch is dropped
        if (bt && !answered) {
          for (auto &r : bt->reqs) {
            r->status = status;
            r->message = handoff::text(msg);
          }
          bt->done->complete();
        }
        bt.reset();
        if (!lk.owns_lock()) lk.lock();
      });
    }
  }

  const Options opt_;
  const Runner run_;
  mutable std::mutex mu_;
  std::condition_variable cv_work_;
  std::unique_ptr<Batch> open_;                 // accepting requests (never null)
  std::deque<std::unique_ptr<Batch>> ready_;    // closed, waiting for a dispatcher
  std::vector<std::unique_ptr<Batch>> spare_;   // recycled
  TicketShard tk_[TK_SHARDS];
  std::vector<std::thread> workers_;
  std::atomic<int64_t> next_ticket_{1};
  bool stop_ = false;
  handoff::Inside inside_;
  // statistics
  int64_t n_requests_ = 0, n_batches_ = 0, n_full_ = 0, n_timeout_ = 0, max_batch_seen_ = 0;
  std::atomic<int64_t> in_lock_throws_{0};
};

}  // namespace request_queue
