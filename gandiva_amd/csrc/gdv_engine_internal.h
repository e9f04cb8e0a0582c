// What the engine's units (gdv_engine.cc, gdv_projector.cc, gdv_varlen_launch.cc, gdv_filter.cc,
// gdv_filter_project.cc) share: the argument block, host staging, the debug switches, and the launch
// helpers more than one operator uses.  Included by those units only.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <list>
#include <optional>
#include <unordered_map>

#include "gdv_engine.h"
#include "gdv_engine_policy.h"
#include "gdv_kernels.h"

namespace gdv::engine {

// ------------------------------------------------------------------ LRU cache of built modules
// (the reference keeps a process-wide, mutex-guarded LRU of compiled modules keyed on
// schema + expressions + configuration: SURVEY.md §2 row 12)
template <typename T>
class LruCache {
 public:
  explicit LruCache(size_t cap) : cap_(cap) {}
  std::shared_ptr<T> Get(const std::string& key) {
    std::lock_guard<std::mutex> g(mu_);
    auto it = map_.find(key);
    if (it == map_.end()) return nullptr;
    order_.splice(order_.begin(), order_, it->second.second);
    return it->second.first;
  }
  void Put(const std::string& key, std::shared_ptr<T> v) {
    std::lock_guard<std::mutex> g(mu_);
    if (map_.count(key)) return;
    order_.push_front(key);
    map_[key] = {std::move(v), order_.begin()};
    if (map_.size() > cap_) {
      map_.erase(order_.back());
      order_.pop_back();
    }
  }

 private:
  size_t cap_;
  std::mutex mu_;
  std::list<std::string> order_;
  std::unordered_map<std::string,
                     std::pair<std::shared_ptr<T>, std::list<std::string>::iterator>>
      map_;
};

std::string SchemaKey(const Schema& s);

// ------------------------------------------------------------------ argument block

struct HostBitmap {
  const uint64_t* p = nullptr;
  int32_t shift = 0;
  int32_t pad = 0;
  int64_t nwords = 0;
};
static_assert(sizeof(HostBitmap) == 24, "must match struct gdv_bitmap in gdv_device_lib.hpp");

class ArgBlock {
 public:
  explicit ArgBlock(const ArgLayout& l) : layout_(l), buf_(l.total(), 0) {}
  void Set64(int off, uint64_t v) { std::memcpy(&buf_[off], &v, 8); }
  uint64_t Get64(int off) const { uint64_t v; std::memcpy(&v, &buf_[off], 8); return v; }
  void SetPtr(int off, const void* p) { Set64(off, reinterpret_cast<uint64_t>(p)); }
  void SetInData(int k, const void* p) { SetPtr(layout_.in_base() + k * ArgLayout::kInStride, p); }
  void SetInValid(int k, const HostBitmap& b) {
    std::memcpy(&buf_[layout_.in_base() + k * ArgLayout::kInStride + 8], &b, 24);
  }
  void SetInBits(int k, const HostBitmap& b) {
    std::memcpy(&buf_[layout_.in_base() + k * ArgLayout::kInStride + 32], &b, 24);
  }
  void SetInOffsets(int k, const void* p) {
    SetPtr(layout_.in_base() + k * ArgLayout::kInStride + 56, p);
  }
  void SetOutData(int e, void* p) { SetPtr(layout_.out_base() + e * ArgLayout::kOutStride, p); }
  void SetOutValid(int e, void* p) {
    SetPtr(layout_.out_base() + e * ArgLayout::kOutStride + 8, p);
  }
  void SetOutOffsets(int e, void* p) {
    SetPtr(layout_.out_base() + e * ArgLayout::kOutStride + 16, p);
  }
  void* GetOutOffsets(int e) const {
    return reinterpret_cast<void*>(Get64(layout_.out_base() + e * ArgLayout::kOutStride + 16));
  }
  void SetLit(int i, uint64_t v) { Set64(layout_.lit_base() + i * 8, v); }
  // input slot k := slot `src_k` of another block (same column, already bound / staged there)
  void CopyInSlot(int k, const ArgBlock& src, int src_k) {
    std::memcpy(&buf_[layout_.in_base() + k * ArgLayout::kInStride],
                &src.buf_[src.layout_.in_base() + src_k * ArgLayout::kInStride], ArgLayout::kInStride);
  }
  void SetOutCap(int e, int64_t bytes) {
    Set64(layout_.out_base() + e * ArgLayout::kOutStride + 24, static_cast<uint64_t>(bytes));
  }
  // input slot k moved forward by `rows` rows (a multiple of 64).  width > 0: fixed-width values;
  // 0: bool values (a bitmap); -1: var-len (offsets move, the byte buffer stays)
  void AdvanceInSlot(int k, int64_t rows, int width) {
    const int base = layout_.in_base() + k * ArgLayout::kInStride;
    auto bump_ptr = [&](int off, int64_t bytes) {
      uint64_t p;
      std::memcpy(&p, &buf_[off], 8);
      if (p != 0) p += static_cast<uint64_t>(bytes);
      std::memcpy(&buf_[off], &p, 8);
    };
    auto bump_bitmap = [&](int off) {
      HostBitmap b;
      std::memcpy(&b, &buf_[off], 24);
      if (b.p != nullptr && b.nwords > 1) {  // (nwords == 1: the all-ones word, index clamped)
        b.p += rows / 64;
        b.nwords = std::max<int64_t>(b.nwords - rows / 64, 1);
      }
      std::memcpy(&buf_[off], &b, 24);
    };
    if (width > 0) bump_ptr(base, rows * width);
    bump_bitmap(base + 8);
    if (width == 0) bump_bitmap(base + 32);
    if (width < 0) bump_ptr(base + 56, rows * 4);
  }
  const void* data() const { return buf_.data(); }
  size_t size() const { return buf_.size(); }

 private:
  ArgLayout layout_;
  std::vector<char> buf_;
};

HostBitmap FoldBitmap(const void* ptr, int64_t size, int64_t bit_offset);

inline int64_t BytesForBits(int64_t bits) { return (bits + 7) / 8; }

// Error paths must not hand staging blocks back to the pool while copies or kernels that
// use them are still queued: declared AFTER the Staging object, this drains the stream first.
struct StreamDrain {
  hipStream_t stream;
  bool armed;
  ~StreamDrain() {
    if (armed) (void)hipStreamSynchronize(stream);
  }
};

// Debug switches of the evaluation path, read from the environment ONCE per process (first use): no
// getenv is reachable from Evaluate (round-3 verdict: a getenv per call on a path that takes 0.6-7 us
// per batch, and not safe against a concurrent setenv).  Code-generation switches are read at Make
// (CodegenOptions::FromEnv).
struct EngineKnobs {
  bool trace = false;              // GDV_TRACE: one line per Evaluate on stderr
  bool no_optflat = false;         // GDV_NO_OPTFLAT: var-len plans go straight to the general kernel
  bool no_evaluate_many = false;   // GDV_NO_EVALUATE_MANY: multi-batch calls run batch by batch
  bool no_small_filter = false;    // GDV_NO_SMALL_FILTER: default of Filter "small_filter" tuning (read at Make)
  int filter_chunks = 1;           // GDV_FILTER_CHUNKS: default of Filter "chunks" tuning (read at Make)
  int grid_mult = 0;               // GDV_GRID_MULT: workgroups per CU of the grid-stride launch (0: default)
  bool fp_window_only = false;     // GDV_FP_WINDOW_ONLY: fused filter-project never moves to its direct kernel (tests, sweeps)
  bool fp_force_stall = false;     // GDV_FP_FORCE_STALL: treat every fused launch as stalled (exercises the chain re-run)
  bool no_tier0 = false;           // GDV_NO_TIER0: Make waits for the specialised kernel as before round 6
  bool force_tier0 = false;        // GDV_FORCE_TIER0: every plan that has a tier-0 program runs on it, always (tests)
  static const EngineKnobs& Get() {
    static const EngineKnobs k = [] {
      EngineKnobs x;
      x.trace = std::getenv("GDV_TRACE") != nullptr;
      x.no_optflat = std::getenv("GDV_NO_OPTFLAT") != nullptr;
      x.no_evaluate_many = std::getenv("GDV_NO_EVALUATE_MANY") != nullptr;
      x.no_small_filter = std::getenv("GDV_NO_SMALL_FILTER") != nullptr;
      x.fp_window_only = std::getenv("GDV_FP_WINDOW_ONLY") != nullptr;
      x.fp_force_stall = std::getenv("GDV_FP_FORCE_STALL") != nullptr;
      x.no_tier0 = std::getenv("GDV_NO_TIER0") != nullptr;
      x.force_tier0 = std::getenv("GDV_FORCE_TIER0") != nullptr;
      if (const char* s = std::getenv("GDV_GRID_MULT")) x.grid_mult = std::max(1, atoi(s));
      if (const char* s = std::getenv("GDV_FILTER_CHUNKS")) x.filter_chunks = std::max(1, std::min(64, atoi(s)));
      return x;
    }();
    return k;
  }
};

// GDV_TRACE=1: one line per Evaluate on stderr (kind, kernel, rows, device time between two
// HIP events on the launch stream, rows/s).  The reference has no tracing of its own
// (SURVEY.md §5); this is the hook its micro-benchmarks' std::chrono timers stood in for.
// Tracing synchronises the stream, so it also serialises asynchronous evaluations.
class EvalTrace {
 public:
  EvalTrace(const char* kind, const std::string& kernel, int64_t rows, hipStream_t stream)
      : kind_(kind), kernel_(kernel), rows_(rows), stream_(stream) {
    on_ = EngineKnobs::Get().trace;
    if (on_ && hipEventCreate(&t0_) == hipSuccess && hipEventCreate(&t1_) == hipSuccess) {
      (void)hipEventRecord(t0_, stream_);
    } else {
      on_ = false;
    }
  }
  ~EvalTrace() {
    if (!on_) return;
    (void)hipEventRecord(t1_, stream_);
    (void)hipEventSynchronize(t1_);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, t0_, t1_);
    fprintf(stderr, "[gdv] %s %s rows=%lld device_ms=%.4f Mrows/s=%.1f\n", kind_, kernel_.c_str(),
            static_cast<long long>(rows_), ms, ms > 0 ? rows_ / (ms * 1e3) : 0.0);
    (void)hipEventDestroy(t0_);
    (void)hipEventDestroy(t1_);
  }

 private:
  const char* kind_;
  std::string kernel_;
  int64_t rows_;
  hipStream_t stream_;
  bool on_ = false;
  hipEvent_t t0_ = nullptr, t1_ = nullptr;
};

// Host-buffer path.  Large batches: one device buffer and one copy per Arrow buffer (the
// copies are PCIe-bound anyway).  Small batches (<= kPackRows rows, while they fit the
// block): every staged input and every fixed-size output shares ONE device block mirrored by
// ONE pinned host block — one H2D before the launches, one D2H after them — because a
// pageable hipMemcpyAsync costs 10-25 us however small it is and a ten-expression projection
// would issue ~30 of them (C2 at 1024 rows: 397 -> 74 us per Evaluate).
struct Staging {
  static constexpr int64_t kPackRows = 131072;
  std::deque<DeviceBuffer> buffers;  // deque: references stay valid across Add()
  DeviceBuffer& Add() {
    buffers.emplace_back();
    return buffers.back();
  }
  ~Staging() {
    if (pin_ != nullptr) Runtime::Get().ReleasePinned(pin_);
  }

  Status EnablePacked() {
    GDV_RETURN_NOT_OK(Runtime::Get().AcquirePinned(&pin_));
    GDV_RETURN_NOT_OK(block_.Allocate(Runtime::kPinnedBlock));
    packed_ = true;
    return Status::OK();
  }

  // device copy of n host bytes, readable (zero-filled) up to `alloc` bytes
  Status In(const void* src, size_t n, size_t alloc, hipStream_t stream, void** dev) {
    if (alloc < n) alloc = n;
    HostRegistry::StagedBytes().fetch_add(static_cast<int64_t>(n), std::memory_order_relaxed);
    size_t off = 0;
    if (packed_ && !flushed_ && Reserve(alloc, &off)) {
      if (n > 0) std::memcpy(pin_ + off, src, n);
      if (alloc > n) std::memset(pin_ + off + n, 0, alloc - n);
      *dev = block_.as<char>() + off;
      in_end_ = used_;
      return Status::OK();
    }
    DeviceBuffer& d = Add();
    GDV_RETURN_NOT_OK(d.Allocate(std::max<size_t>(alloc, 8)));
    if (alloc > n) GDV_HIP_RETURN_NOT_OK(hipMemsetAsync(d.get(), 0, alloc, stream));
    if (n > 0) GDV_HIP_RETURN_NOT_OK(hipMemcpyAsync(d.get(), src, n, hipMemcpyHostToDevice, stream));
    *dev = d.get();
    return Status::OK();
  }
  // all In() regions -> device with one copy; call once, before the first launch
  Status FlushIn(hipStream_t stream) {
    flushed_ = true;
    if (packed_ && in_end_ > 0)
      GDV_HIP_RETURN_NOT_OK(hipMemcpyAsync(block_.get(), pin_, in_end_, hipMemcpyHostToDevice, stream));
    return Status::OK();
  }
  // device region of `alloc` bytes whose first `copy` bytes FetchOut/Deliver bring to `user`
  Status Out(size_t alloc, size_t copy, void* user, void** dev) {
    size_t off = 0;
    OutCopy oc{user, nullptr, 0, copy, false};
    HostRegistry::StagedBytes().fetch_add(static_cast<int64_t>(copy), std::memory_order_relaxed);
    if (packed_ && Reserve(alloc, &off)) {
      oc.off = off;
      oc.packed = true;
      *dev = block_.as<char>() + off;
    } else {
      DeviceBuffer& d = Add();
      GDV_RETURN_NOT_OK(d.Allocate(std::max<size_t>(alloc, 8)));
      oc.dev = d.get();
      *dev = d.get();
    }
    outs_.push_back(oc);
    return Status::OK();
  }
  Status FetchOut(hipStream_t stream) {
    size_t lo = used_, hi = 0;
    for (auto& o : outs_) {
      if (o.n == 0) continue;
      if (o.packed) {
        lo = std::min(lo, o.off);
        hi = std::max(hi, o.off + o.n);
      } else {
        GDV_HIP_RETURN_NOT_OK(hipMemcpyAsync(o.user, o.dev, o.n, hipMemcpyDeviceToHost, stream));
      }
    }
    if (hi > lo)
      GDV_HIP_RETURN_NOT_OK(hipMemcpyAsync(pin_ + lo, block_.as<char>() + lo, hi - lo,
                                           hipMemcpyDeviceToHost, stream));
    return Status::OK();
  }
  void Deliver() {  // after the stream is drained
    for (auto& o : outs_)
      if (o.packed && o.n > 0) std::memcpy(o.user, pin_ + o.off, o.n);
  }

 private:
  struct OutCopy {
    void* user;
    void* dev;
    size_t off, n;
    bool packed;
  };
  bool Reserve(size_t bytes, size_t* off) {
    const size_t at = (used_ + 255) & ~size_t{255};
    if (at + bytes > Runtime::kPinnedBlock) return false;
    *off = at;
    used_ = at + bytes;
    return true;
  }
  bool packed_ = false, flushed_ = false;
  DeviceBuffer block_;
  char* pin_ = nullptr;
  size_t used_ = 0, in_end_ = 0;
  std::vector<OutCopy> outs_;
};

Status StageBitmap(const void* host, int64_t off, int64_t rows, hipStream_t stream,
                   Staging* st, HostBitmap* out);

Status BindInputs(const KernelPlan& plan, const Schema& schema, const ColumnBuffers* cols,
                  int num_cols, int64_t batch_rows, MemKind mem, hipStream_t stream,
                  ArgBlock* args, Staging* st, int64_t compact_rows = -1);

int64_t GridFor(const KernelPlan& plan, int64_t rows);

constexpr uint32_t kErrStall = 8u;  // GDV_ERR_STALL (gdv_device_lib.hpp): a look-back / scanner hand-off gave up

std::string ErrorMessage(uint32_t bits);
Status UploadConstBlock(const KernelPlan& plan, DeviceBuffer* out);
void BindLiterals(const KernelPlan& plan, const DeviceBuffer& consts, ArgBlock* args);

struct ScratchPart {  // a piece of a scratch block, spelled like a DeviceBuffer
  char* p;
  template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};


// ------------------------------------------------------------------ first-stage temporaries
// (StageCapacity, the other half of the sizing, is in gdv_engine_policy.h)

// First guess for the byte buffers: as many bytes as the var-len inputs hold plus 32 per row.
inline int64_t StageGuess(const ColumnBuffers* cols, int num_cols, int64_t rows) {
  int64_t guess = 32 * rows;
  for (int k = 0; k < num_cols; k++)
    if (cols[k].offsets != nullptr) guess += cols[k].data_size;
  return std::min<int64_t>(guess, kStageGuessMax);
}

// a first-stage output as the second stage's input column, `data_size` readable bytes
inline ColumnBuffers AsColumn(const OutputBuffers& o, int64_t data_size) {
  ColumnBuffers c;
  c.validity = o.validity;
  c.validity_size = o.validity_size;
  c.offsets = o.offsets;
  c.offsets_size = o.offsets_size;
  c.data = o.data;
  c.data_size = data_size;
  return c;
}

// ------------------------------------------------------------------ tier 0

// Tier 0 (round 6): a plan the ahead-of-time interpreter takes, whose specialised kernel is not at hand yet, does not
// wait for hipRTC (0.25-0.9 s): the compilation is queued, Make returns, and Evaluate runs the plan's post-fix program
// until the code object is there.  GDV_NO_TIER0=1: as before.  GDV_FORCE_TIER0=1 (tests): tier 0 always.
// Leaves *tier0 null when the plan stays on the blocking path.
void ArmTier0(const Schema& schema, const std::vector<ExpressionPtr>& exprs, bool is_filter, const KernelPlan& plan,
              std::unique_ptr<tier0::Args>* tier0, std::atomic<bool>* pending);
// one launch of the interpreter kernel over `args`
Status RunTier0(const tier0::Args& prog, const ArgBlock& args, int64_t rows, Runtime& rt, hipStream_t stream);

// ------------------------------------------------------------------ the pinned block of a multi-batch call

// One of the runtime's pinned host blocks (the small kind when `bytes` fit it), given back by the destructor or,
// for an asynchronous exit, once `stream` has passed the copy that reads it.
class PinnedLease {
 public:
  explicit PinnedLease(Runtime& rt) : rt_(rt) {}
  PinnedLease(const PinnedLease&) = delete;
  PinnedLease& operator=(const PinnedLease&) = delete;
  ~PinnedLease() {
    if (pin_ != nullptr) { if (small_) rt_.ReleasePinnedSmall(pin_); else rt_.ReleasePinned(pin_); }
  }
  Status Acquire(size_t bytes) {
    small_ = bytes <= Runtime::kPinnedSmall;
    return small_ ? rt_.AcquirePinnedSmall(&pin_) : rt_.AcquirePinned(&pin_);
  }
  char* get() const { return pin_; }
  void ReleaseAfter(hipStream_t stream) {
    if (pin_ == nullptr) return;
    char* p = pin_;
    pin_ = nullptr;
    Runtime* owner = &rt_;
    const bool small = small_;
    rt_.Defer(stream, [owner, p, small] { if (small) owner->ReleasePinnedSmall(p); else owner->ReleasePinned(p); });
  }

 private:
  Runtime& rt_;
  char* pin_ = nullptr;
  bool small_ = false;
};

// ------------------------------------------------------------------ the var-len launch

// The kernels of ONE var-len evaluation on `stream`, for the synchronous and the asynchronous entry alike: the
// geometry of both shapes, their pooled scratch, and the two enqueue sequences.  Nothing here waits or reads
// back: the callers fetch the error word and the totals their own way, from the addresses below.
//   Wave shape (plans whose output lengths follow from the offsets): pre-pass -> offsets scan -> main kernel of
//   independent wave tiles.  Head block: [error word | grand totals (2 * ng) | totals of the scanned segments].
//   Scanner shape: one launch; workgroup 0 scans the tile totals, workers post one granule and poll one.
//   State block: [error word | grand totals (2 * ng) | granules (2 * ng per tile)].
// The scratch blocks are pooled: declare a VarlenLaunch BEFORE the call's StreamDrain.
class VarlenLaunch {
 public:
  VarlenLaunch(const KernelPlan& plan, const PlanDeviceState* dev, Runtime& rt, int64_t out_rows, hipStream_t stream);

  // the exact variant (main + pre-pass) / the general variant of a plan, compiled the first time a batch needs them
  static Status EnsureExact(const KernelPlan& plan, const PlanDeviceState* dev, Runtime& rt);
  static Status EnsureGeneral(const KernelPlan& plan, const PlanDeviceState* dev, Runtime& rt);
  Status EnsureExact() { return EnsureExact(plan_, dev_, rt_); }
  Status EnsureGeneral() { return EnsureGeneral(plan_, dev_, rt_); }

  // Wave shape, the optimistic pair or (exact) its exact variant.  `args` is the main kernel's block with inputs,
  // outputs, selection and rows word bound; the pre-pass block is derived from it once.  zero_counts: the
  // pre-pass may walk fewer rows than the launch is sized for (a row count in device memory), so the per-tile
  // counts the scan reads must start at zero.
  Status EnqueueWave(ArgBlock* args, bool exact, bool zero_counts);
  // Scanner shape: `kernel` over `grid` workgroups (scanner_grid(), or 2 for the serial-safe re-run).
  Status EnqueueScanner(ArgBlock* args, const CompiledKernel& kernel, int64_t grid);
  int64_t scanner_grid() const { return std::max<int64_t>(1, ntiles) + 1; }  // one workgroup per tile + the scanner

  // where the results of the last launch live: the head / state block starts with the error word
  const PlanDeviceState* dev() const { return dev_; }
  const char* wave_head() const { return head_.as<char>(); }
  size_t wave_total_word(int v) const {  // index, in 8-byte words from the head, of var-len output v's byte total
    return plan_.wave_segments[v] >= 0 ? 1 + 2 * ng + plan_.wave_segments[v] : 1 + v;
  }
  const char* wave_total(int v) const { return wave_head() + 8 * wave_total_word(v); }
  const char* scanner_state() const { return state_.as<char>(); }
  const char* scanner_total(int v) const { return scanner_state() + 8 + 8 * v; }

  // asynchronous exit: the scratch goes back to the pool when the stream has passed this point
  void ReleaseAfter(hipStream_t stream);

  // geometry (all zero for a plan without var-len outputs)
  int ng = 0;                // pairs of var-len outputs
  int nseg = 0;              // wave shape: scanned segments
  size_t totals_bytes = 0, head_bytes = 0, state_bytes = 0;
  int64_t nwt = 0;           // wave tiles
  int64_t seg_stride = 0;    // counts per segment (the scan kernels read the totals 16 bytes at a time)
  int sc_u = 0, sc_w = 0;    // tile of the scanner-shaped kernel: a wave plan's fallback has its own
  int64_t ntiles = 0;        // workgroup tiles of the scanner-shaped kernel
  std::vector<int> vl;       // the var-len outputs

 private:
  const KernelPlan& plan_;
  const PlanDeviceState* dev_;
  Runtime& rt_;
  const int64_t out_rows_;
  const hipStream_t stream_;
  DeviceBuffer head_, counts_, bases_, chunks_, state_;
  std::optional<ArgBlock> pargs_;  // the pre-pass block
};

}  // namespace gdv::engine
