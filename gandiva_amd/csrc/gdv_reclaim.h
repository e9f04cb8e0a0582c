// The two mechanisms behind the runtime's pools and deferred frees, free of HIP so that they run under ThreadSanitizer as a
// plain program (tests/cxx/reclaim_test.cc): a bounded list of idle handles, and a queue of work that waits for a token
// (the product's token is a hipEvent_t).  Neither calls anything it was given while it holds its mutex — except the
// queue's is_ready, which must be a non-blocking query.
#pragma once
#include <cstddef>
#include <functional>
#include <mutex>
#include <utility>
#include <vector>

namespace gdv {

// Idle handles kept for reuse, last in first out, at most `cap` of them: one more is handed to `destroy`, outside the lock.
template <typename T>
class FreeList {
 public:
  FreeList(size_t cap, std::function<void(T)> destroy) : cap_(cap), destroy_(std::move(destroy)) {}
  bool Take(T* out) {
    std::lock_guard<std::mutex> g(mu_);
    if (idle_.empty()) return false;
    *out = idle_.back();
    idle_.pop_back();
    return true;
  }
  void Give(T v) {
    {
      std::lock_guard<std::mutex> g(mu_);
      if (idle_.size() < cap_) {
        idle_.push_back(v);
        return;
      }
    }
    destroy_(v);
  }

 private:
  std::mutex mu_;
  std::vector<T> idle_;
  const size_t cap_;
  const std::function<void(T)> destroy_;
};

// Entries {token, tag, done} in push order.  The rule this type exists for: an entry is REMOVED from the queue, under the
// lock, before anyone waits on its token, releases its token or runs its `done` — whoever removed it is its only owner, so
// no second thread can recycle or destroy a token that the first is still waiting on.
template <typename Token>
class DeferredQueue {
 public:
  struct Entry {
    Token token;
    size_t tag;
    std::function<void()> done;
  };
  void Push(Token token, size_t tag, std::function<void()> done) {
    std::lock_guard<std::mutex> g(mu_);
    entries_.push_back(Entry{std::move(token), tag, std::move(done)});
  }
  // every entry whose token `is_ready` accepts (called under the lock: a query, never a wait); the others stay, in order
  template <typename IsReady>
  std::vector<Entry> TakeReady(IsReady is_ready) {
    std::vector<Entry> taken;
    std::lock_guard<std::mutex> g(mu_);
    size_t keep = 0;
    for (size_t i = 0; i < entries_.size(); i++) {
      if (is_ready(entries_[i].token)) {
        taken.push_back(std::move(entries_[i]));
      } else {
        if (keep != i) entries_[keep] = std::move(entries_[i]);
        keep++;
      }
    }
    entries_.erase(entries_.begin() + static_cast<std::ptrdiff_t>(keep), entries_.end());
    return taken;
  }
  std::vector<Entry> TakeAll() {
    std::vector<Entry> taken;
    std::lock_guard<std::mutex> g(mu_);
    taken.swap(entries_);
    return taken;
  }
  // the oldest entry tagged `tag`, when at least `at_least` entries carry that tag; false (and `out` untouched) otherwise
  bool TakeOldestIf(size_t tag, size_t at_least, Entry* out) {
    std::lock_guard<std::mutex> g(mu_);
    size_t count = 0, oldest = 0;
    for (size_t i = 0; i < entries_.size(); i++)
      if (entries_[i].tag == tag && count++ == 0) oldest = i;
    if (count == 0 || count < at_least) return false;
    *out = std::move(entries_[oldest]);
    entries_.erase(entries_.begin() + static_cast<std::ptrdiff_t>(oldest));
    return true;
  }

 private:
  std::mutex mu_;
  std::vector<Entry> entries_;
};

}  // namespace gdv
