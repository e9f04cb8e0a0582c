// What a context hands out and takes back: the device block pool with deferred frees, the pinned-block pools, the stream
// pool and the event pool (declared in gdv_runtime.h; the mechanisms are gdv_reclaim.h's).
#include <cstdlib>

#include "gdv_runtime.h"

namespace gdv {

static size_t RoundSize(size_t b) {
  if (b < 256) return 256;
  if (b < (1u << 20)) {
    size_t p = 256;
    while (p < b) p <<= 1;
    return p;
  }
  const size_t g = 2u << 20;
  return (b + g - 1) / g * g;
}

void Runtime::Defer(hipStream_t stream, size_t tag, std::function<void()> fn) {
  hipEvent_t e = nullptr;
  if (!AcquireEvent(&e).ok() || hipEventRecord(e, stream) != hipSuccess) {
    // no event to wait on: fall back to waiting for the stream itself
    (void)hipGetLastError();
    ReleaseEvent(e);
    (void)hipStreamSynchronize(stream);
    fn();
    return;
  }
  deferred_.Push(e, tag, std::move(fn));
}

void Runtime::Defer(hipStream_t stream, std::function<void()> fn) { Defer(stream, 0, std::move(fn)); }

void Runtime::FreeAfter(void* ptr, hipStream_t stream) {
  if (!ptr) return;
  size_t sz = 0;  // (a block that is not this pool's: Free will ignore it, and it counts towards no size)
  {
    std::lock_guard<std::mutex> g(mu_);
    auto it = live_blocks_.find(ptr);
    if (it != live_blocks_.end()) sz = it->second;
  }
  Defer(stream, sz, [this, ptr] { Free(ptr); });
}

void Runtime::Complete(Deferred::Entry& d, bool wait) {
  if (wait && hipEventSynchronize(d.token) != hipSuccess) (void)hipGetLastError();
  ReleaseEvent(d.token);
  d.done();
}

void Runtime::Reap(bool wait) {
  auto taken = wait ? deferred_.TakeAll() : deferred_.TakeReady([](hipEvent_t e) {
    hipError_t q = hipEventQuery(e);
    if (q != hipSuccess && q != hipErrorNotReady) (void)hipGetLastError();
    return q == hipSuccess;
  });
  for (auto& d : taken) Complete(d, wait);
}

bool Runtime::TakeFree(size_t sz, void** ptr) {
  std::lock_guard<std::mutex> g(mu_);
  auto it = free_blocks_.find(sz);
  if (it == free_blocks_.end()) return false;
  *ptr = it->second;
  free_blocks_.erase(it);
  cached_bytes_ -= sz;
  live_blocks_[*ptr] = sz;
  return true;
}

Status Runtime::Alloc(size_t bytes, void** ptr) {
  GDV_RETURN_NOT_OK(EnsureDevice());
  Reap(false);
  size_t sz = RoundSize(bytes);
  if (TakeFree(sz, ptr)) return Status::OK();
  // Bounded run-ahead (round 6).  An asynchronous caller enqueues faster than the GPU completes: every call would find the
  // blocks of the calls before it still in flight and take NEW ones from the driver — unbounded memory, and a hipMalloc that
  // has to map fresh memory stalls the kernels that are running (C5's asynchronous Evaluate as the fourth workload of one
  // process: a 3-5 ms gap every 13-14 calls, profiles/r06_bench_step_outliers.txt).  With kMaxDeferredPerSize blocks of this
  // size already waiting for their streams, wait for the oldest of them instead and take that one.
  constexpr int kMaxDeferredPerSize = 8;
  Deferred::Entry oldest;
  if (deferred_.TakeOldestIf(sz, kMaxDeferredPerSize, &oldest)) {
    Complete(oldest, true);  // (out of the queue: no other thread's Reap can release the event under this wait)
    Reap(false);             // what else completed during the wait
    if (TakeFree(sz, ptr)) return Status::OK();
  }
  hipError_t e = hipMalloc(ptr, sz);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    Reap(true);
    TrimPool();
    e = hipMalloc(ptr, sz);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return Status::OutOfMemory("hipMalloc of " + std::to_string(sz) + " bytes failed");
  }
  std::lock_guard<std::mutex> g(mu_);
  live_blocks_[*ptr] = sz;
  return Status::OK();
}

void Runtime::Free(void* ptr) {
  if (!ptr) return;
  std::lock_guard<std::mutex> g(mu_);
  auto it = live_blocks_.find(ptr);
  if (it == live_blocks_.end()) return;
  size_t sz = it->second;
  live_blocks_.erase(it);
  // keep at most kPoolCapBytes of idle blocks (staging buffers of the host path can be tens
  // of GB); beyond that, blocks go straight back to the driver
  static const size_t cap = [] {
    const char* e = std::getenv("GDV_POOL_CAP_MB");
    return (e ? static_cast<size_t>(atoll(e)) : static_cast<size_t>(16384)) << 20;
  }();
  if (cached_bytes_ + sz > cap) {
    (void)hipFree(ptr);
    return;
  }
  free_blocks_.emplace(sz, ptr);
  cached_bytes_ += sz;
}

void Runtime::TrimPool() {
  std::multimap<size_t, void*> blocks;
  {
    std::lock_guard<std::mutex> g(mu_);
    blocks.swap(free_blocks_);
    cached_bytes_ = 0;
  }
  for (auto& b : blocks) (void)hipFree(b.second);
}

Status Runtime::AcquirePinnedOf(FreeList<char*>& pool, size_t bytes, const char* what, char** p) {
  GDV_RETURN_NOT_OK(EnsureDevice());
  Reap(false);
  if (pool.Take(p)) return Status::OK();
  void* q = nullptr;
  if (hipHostMalloc(&q, bytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    return Status::OutOfMemory(std::string("hipHostMalloc of ") + what + " failed");
  }
  *p = static_cast<char*>(q);
  return Status::OK();
}

Status Runtime::AcquirePinned(char** p) { return AcquirePinnedOf(pinned_, kPinnedBlock, "the pinned staging block", p); }
void Runtime::ReleasePinned(char* p) {
  if (p != nullptr) pinned_.Give(p);
}

Status Runtime::AcquirePinnedSmall(char** p) {
  return AcquirePinnedOf(pinned_small_, kPinnedSmall, "a pinned argument-table block", p);
}
void Runtime::ReleasePinnedSmall(char* p) {
  if (p != nullptr) pinned_small_.Give(p);
}

Status Runtime::AcquireStream(hipStream_t* out) {
  GDV_RETURN_NOT_OK(EnsureDevice());
  if (streams_.Take(out)) return Status::OK();
  GDV_HIP_RETURN_NOT_OK(hipStreamCreateWithFlags(out, hipStreamNonBlocking));
  return Status::OK();
}
void Runtime::ReleaseStream(hipStream_t s) {
  if (s != nullptr) streams_.Give(s);
}

Status Runtime::AcquireEvent(hipEvent_t* out) {
  GDV_RETURN_NOT_OK(EnsureDevice());
  if (events_.Take(out)) return Status::OK();
  GDV_HIP_RETURN_NOT_OK(hipEventCreateWithFlags(out, hipEventDisableTiming));
  return Status::OK();
}
void Runtime::ReleaseEvent(hipEvent_t e) {
  if (e != nullptr) events_.Give(e);
}

}  // namespace gdv
