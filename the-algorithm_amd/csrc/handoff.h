// handoff.h -- the three things the serving threads (the submission engine of sann_api.hip, the micro-batching queue of
// request_queue.h) say to each other, each written once.  Host code, standard library only: it compiles and runs under the
// host sanitizers on a machine with no GPU (tests/serving_handoff_host_check.cpp).
//
//   Completion      a caller sleeps until a worker thread has finished its job or batch
//   Inside          counts the callers currently inside an object, so that whoever deletes it can wait for them to leave
//   guarded         one iteration of a worker thread's loop: an exception fails what the thread was holding, not the process
//
// No work queue and no thread pool: the engine's loop and the queue's deadline loop have different shapes and stay their own.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <exception>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <utility>

namespace handoff {

// A message as a std::string without an exception: empty when there is no memory for it (the status still travels).
inline std::string text(const char *s) noexcept {
  try { return std::string(s); } catch (...) { return std::string(); }
}

// The completion of one job (one waiter: the engine's caller, who also reads status and message) or one batch (many waiters:
// the callers of its requests).  complete() sets the fields and notifies WHILE IT HOLDS THE MUTEX, and touches nothing
// afterwards: a waiter gets past wait() / a true poll() only through that mutex, hence only after the completer's last access,
// and may then destroy the object.  So it is sound both as a member of the waiter's stack frame and behind a shared_ptr.
class Completion {
 public:
  Completion() = default;
  Completion(const Completion &) = delete;
  Completion &operator=(const Completion &) = delete;

  void complete(int status = 0, std::string &&message = std::string()) noexcept {
    std::lock_guard<std::mutex> lk(m_);
    status_ = status;
    message_ = std::move(message);
    done_ = true;
    cv_.notify_all();
  }
  void wait() {
    std::unique_lock<std::mutex> lk(m_);
    cv_.wait(lk, [this] { return done_; });
  }
  bool poll() {
    std::lock_guard<std::mutex> lk(m_);
    return done_;
  }
  // (the waiter's, after wait() or a true poll())
  int status() const { return status_; }
  const std::string &message() const { return message_; }

 private:
  std::mutex m_;
  std::condition_variable cv_;
  bool done_ = false;
  int status_ = 0;
  std::string message_;
};

// Callers currently inside an object.  A caller holds an Inside::Hold for as long as it touches the object (declared first, so
// released last); the thread that deletes the object makes sure nobody new can get in and what they sleep on has been completed,
// then wait_empty(), then delete.  Leaving is the caller's last access to the object.
class Inside {
 public:
  class Hold {
   public:
    explicit Hold(Inside &in) : in_(in) { in_.n_.fetch_add(1, std::memory_order_acquire); }
    ~Hold() { in_.n_.fetch_sub(1, std::memory_order_release); }
    Hold(const Hold &) = delete;
    Hold &operator=(const Hold &) = delete;

   private:
    Inside &in_;
  };
  void wait_empty() const {  // (short: the callers inside have been woken and are on their way out)
    while (n_.load(std::memory_order_acquire) != 0) std::this_thread::yield();
  }
  int count() const { return n_.load(std::memory_order_acquire); }

 private:
  alignas(64) std::atomic<int> n_{0};
};

// One iteration of a worker thread's loop.  body() runs; if it throws, the exception is classified as abi_guard::caught
// classifies it at an entry point (bad_alloc -> enomem, anything else -> einternal) and handed to fail_held(status, message),
// which fails whatever the thread was holding, completes it, and leaves the loop's state fit for the next iteration.
// fail_held must not throw (the message is a plain character array for that reason: handoff::text turns it into a string).
template <class Body, class FailHeld>
void guarded(int enomem, int einternal, Body &&body, FailHeld &&fail_held) noexcept {
  int status = einternal;
  char msg[200];
  try {
    body();
    return;
  } catch (const std::bad_alloc &) {
    status = enomem;
    snprintf(msg, sizeof msg, "out of host memory");
  } catch (const std::exception &e) {
    snprintf(msg, sizeof msg, "internal error: %s", e.what());
  } catch (...) {
    snprintf(msg, sizeof msg, "internal error");
  }
  fail_held(status, (const char *)msg);
}

}  // namespace handoff
