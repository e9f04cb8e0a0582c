#include "gdv_engine_internal.h"

namespace gdv {

using namespace engine;

// ------------------------------------------------------------------ fused filter -> project

Status FilterProject::Make(const Schema& schema, const ExpressionPtr& condition, const std::vector<ExpressionPtr>& exprs,
                           SelectionMode index_mode, const Configuration& config, std::shared_ptr<FilterProject>* out) {
  (void)config;
  if (out == nullptr) return Status::Invalid("FilterProject::Make: null output pointer");
  if (!condition) return Status::Invalid("Condition cannot be null");
  if (exprs.empty()) return Status::Invalid("Expressions cannot be empty");
  // materialised values (concat / castVARCHAR ...) need a first stage: the chain handles them
  StagedExpressions staged;
  std::vector<ExpressionPtr> all = exprs;
  all.push_back(condition);
  StageMaterialisedValues(schema, all, &staged, CodegenOptions::FromEnv());
  if (!staged.pre.empty()) return Status::CodeGenError("fused filter-project: two-stage plans take the filter + projector chain");
  auto fp = std::make_shared<FilterProject>();
  fp->schema_ = schema;
  fp->condition_ = condition;
  fp->exprs_ = exprs;
  GDV_RETURN_NOT_OK(PlanFilterProject(schema, condition, exprs, index_mode, CodegenOptions::FromEnv(), &fp->plan_));
  fp->raises_ = fp->plan_.exprs_raise;
  const PlanDeviceState* st = nullptr;
  GDV_RETURN_NOT_OK(fp->states_.Get(fp->plan_, &st));
  *out = fp;
  return Status::OK();
}

Status FilterProject::SetTuning(const std::string& key, int64_t value) {
  if (key == "kernel" && value >= -1 && value <= 1) pinned_kernel_.store(static_cast<int>(value));
  else if (key == "small" && value >= 0 && value <= 1) small_.store(value != 0);
  else if (key == "small_rows" && value >= 0 && value <= (int64_t{1} << 17)) small_rows_.store(value);
  else return Status::Invalid("FilterProject tuning: unknown key or value out of range: " + key);
  return Status::OK();
}

FilterProject::~FilterProject() {
  if (int64_t* p = pinned_count_.load()) (void)hipHostFree(p);
}

int FilterProject::which_kernel() const {
  if (plan_.fp_window_rows <= 0 || plan_.exact == nullptr) return -1;
  if (pinned_kernel_.load(std::memory_order_relaxed) >= 0) return pinned_kernel_.load(std::memory_order_relaxed);
  // the window holds fp_window_rows of a wave tile's 64 x subtiles rows; beyond ~85 % of that on average, wave
  // tiles start to overflow into the re-read path and the direct kernel is the better one
  const int limit = plan_.fp_window_rows * 1024 / (64 * plan_.opts.subtiles * std::max(1, plan_.fp_rounds)) * 85 / 100;
  return selected_per_1024_.load(std::memory_order_relaxed) > limit ? 1 : 0;
}

Status FilterProject::Evaluate(int64_t num_rows, const ColumnBuffers* cols, int num_cols, OutputBuffers* outs,
                               int num_outs, void* out_indices, int64_t max_slots, int64_t* num_selected, MemKind mem,
                               hipStream_t stream, uint32_t flags, void* count_out) const {
  bool stalled = false;
  GDV_RETURN_NOT_OK(EvaluateFused(num_rows, cols, num_cols, outs, num_outs, out_indices, max_slots, num_selected, mem, stream,
                                  flags, count_out, &stalled));
  if (!stalled) return Status::OK();
  // The look-back waited 5 s for an earlier workgroup tile (a device time-sliced away, or workgroups not dispatched
  // in index order): the launch is over, its outputs are not complete.  Round 4 returned ExecutionError here; the
  // reference's own chain gives the same results without any cross-workgroup wait.
  return EvaluateChain(num_rows, cols, num_cols, outs, num_outs, out_indices, max_slots, num_selected, mem, stream, count_out);
}

// ------------------------------------------------------------------ many small batches, one launch

// 2^15 rows of a two-int64 predicate: the bytes ONE workgroup is given for one batch.  MEASURED, MI355X,
// profiles/filter_project_small_batches.txt (tools/small_batch_bench fp, 256 batches per round, ~12 % selected): one
// batch per call through the by-value entry beats the one-batch call (memsets + look-back kernel + publish-count kernel)
// up to ~43K rows of the K2F plan (28 bytes per row: 1.2 MB) and ~10K rows of the five-expression threshold plan (62 bytes
// per row: 0.63 MB); 512 KiB is below both.  (The filter's own rule — 2^17 rows x 16 bytes = 2 MiB — is four times that:
// a fused plan does more per byte than a predicate.)
static constexpr int64_t kSmallBatchBytes = int64_t{1} << 19;

int64_t FilterProject::SmallBatchRows(int nb) const {
  if (plan_.small == nullptr || nb < 1) return 0;
  if (const int64_t pinned = small_rows_.load(std::memory_order_relaxed)) return pinned;  // (measurements: "small_rows")
  // Filter::SmallBatchRows' rule — no more rows than one workgroup gets through in about the time the multi-launch
  // path needs to start, never above 2^17 — scaled by the bytes a row moves: one CU has ~1/256 of the chip's
  // bandwidth, and a fused plan reads and writes wider rows than a predicate does.
  int row_bytes = IndexWidth(plan_.mode);
  for (size_t k = 0; k < plan_.input_fields.size(); k++)
    if (plan_.input_needs_values[k]) row_bytes += std::max(1, schema_[plan_.input_fields[k]].type.byte_width());
  for (const DataType& t : plan_.output_types) row_bytes += t.id == kBool ? 1 : t.byte_width();
  // A list of nb batches: the workgroups run side by side (two per CU), so the launch takes about as long as its
  // biggest batch, while the batch-by-batch path takes nb times its start-up: nb times the rows still win.  (Same run:
  // 256 batches of 65536 rows, 1.7-2.6 us per batch in one launch against 75-105 batch by batch.)
  return std::min<int64_t>(kSmallBatchBytes / std::max(16, row_bytes) * nb, int64_t{1} << 17);
}

Status FilterProject::CheckBatch(const BatchView& v, int b) const {
  const std::string where = "batch " + std::to_string(b) + ": ";
  if (v.num_rows < 0) return Status::Invalid(where + "negative row count");
  if (v.num_outs != num_outputs() || (v.num_outs > 0 && v.outs == nullptr))
    return Status::Invalid(where + "number of output buffers does not match the number of expressions");
  const int w = IndexWidth(plan_.mode);
  if (w != 0) {
    if (v.out_indices == nullptr && v.num_rows > 0) return Status::Invalid(where + "Selection vector cannot be null");
    if (v.max_slots < v.num_rows)
      return Status::Invalid(where + "Selection vector too small: max slots " + std::to_string(v.max_slots) + " < rows " +
                             std::to_string(v.num_rows));
    if (w == 2 && v.num_rows > 65536) return Status::Invalid(where + "uint16 selection vector cannot address " + std::to_string(v.num_rows) + " rows");
    if (w == 4 && v.num_rows > (int64_t(1) << 32)) return Status::Invalid(where + "uint32 selection vector cannot address " + std::to_string(v.num_rows) + " rows");
  }
  if (v.num_rows == 0) return Status::OK();  // (none of its buffers is touched)
  for (int e = 0; e < v.num_outs; e++) {
    const int64_t vbytes = Projector::ValidityBytes(v.num_rows), dbytes = Projector::DataBytes(plan_.output_types[e], v.num_rows);
    if (v.outs[e].validity == nullptr || v.outs[e].data == nullptr || v.outs[e].validity_size < vbytes || v.outs[e].data_size < dbytes)
      return Status::Invalid(where + "output buffer " + std::to_string(e) + " too small (device buffers need 8-byte word granularity: " +
                             std::to_string(vbytes) + " validity bytes, " + std::to_string(dbytes) + " data bytes)");
  }
  return Status::OK();
}

static Status EnsureSmall(const KernelPlan& plan, const PlanDeviceState* dev, Runtime& rt) {
  PlanDeviceState* d = const_cast<PlanDeviceState*>(dev);
  if (d->kernel_small.load() == nullptr) {
    const CompiledKernel* k = nullptr;
    GDV_RETURN_NOT_OK(rt.GetKernel(plan.small->source, plan.small->kernel_name, &k));
    if (k->function_small == nullptr || k->function_small1 == nullptr)
      return Status::ExecutionError("internal: the small fused kernel has no multi-batch entry points");
    d->kernel_small.store(k);
  }
  return Status::OK();
}

Status FilterProject::EvaluateMany(const BatchView* batches, int nb, int64_t* counts_host, void* counts_device,
                                   hipStream_t stream, uint32_t flags) const {
  if (nb <= 0) return Status::OK();
  if (batches == nullptr) return Status::Invalid("null batch list");
  if (counts_host == nullptr && counts_device == nullptr) return Status::Invalid("no place for the selected-row counts");
  for (int b = 0; b < nb; b++) GDV_RETURN_NOT_OK(CheckBatch(batches[b], b));
  Runtime& rt = Runtime::Get();
  GDV_RETURN_NOT_OK(rt.EnsureDevice());
  const PlanDeviceState* dev = nullptr;
  GDV_RETURN_NOT_OK(states_.Get(plan_, &dev));
  const int64_t cap_rows = SmallBatchRows(nb);
  const size_t stride = static_cast<size_t>(plan_.layout.total());
  bool fused = cap_rows > 0 && nb <= 65535 && stride * static_cast<size_t>(nb) <= Runtime::kPinnedBlock / 2 &&
               small_.load(std::memory_order_relaxed);
  for (int b = 0; fused && b < nb; b++) fused = batches[b].num_rows <= cap_rows;
  if (!fused) {
    for (int b = 0; b < nb; b++) {
      const BatchView& v = batches[b];
      int64_t count = 0;
      GDV_RETURN_NOT_OK(Evaluate(v.num_rows, v.cols, v.num_cols, v.outs, v.num_outs, v.out_indices, v.max_slots, &count,
                                 MemKind::kDevice, stream, flags,
                                 counts_device != nullptr ? static_cast<char*>(counts_device) + 8 * b : nullptr));
      if (counts_host != nullptr) counts_host[b] = count;
    }
    return Status::OK();
  }
  GDV_RETURN_NOT_OK(EnsureSmall(plan_, dev, rt));
  const CompiledKernel& kernel = *dev->kernel_small.load();
  // scratch: [argument table | error word | counts (int64 per batch)] — no look-back granules, no ticket: one
  // workgroup owns a batch; no memset of the output bitmaps: the workgroup zeroes them itself
  size_t scratch = (stride * nb + 255) & ~size_t{255};
  const size_t err_off = scratch;
  scratch += 256;
  const size_t cnt_off = scratch;
  scratch += (static_cast<size_t>(nb) * 8 + 255) & ~size_t{255};
  DeviceBuffer block;
  GDV_RETURN_NOT_OK(block.Allocate(scratch));
  char* const base = block.as<char>();
  // one batch: its argument block goes by value; several: a table, staged through a pinned block
  const bool by_value = nb == 1;
  std::vector<char> one(by_value ? stride : 0);
  PinnedLease lease(rt);
  if (!by_value) GDV_RETURN_NOT_OK(lease.Acquire(stride * static_cast<size_t>(nb)));
  char* const pin = by_value ? one.data() : lease.get();
  StreamDrain drain{stream, false};  // armed once something is enqueued: error returns wait before the blocks go back
  Staging st;
  for (int b = 0; b < nb; b++) {
    const BatchView& v = batches[b];
    ArgBlock args(plan_.layout);
    if (v.num_rows > 0) {  // (a 0-row batch: its workgroup stores the count 0 and touches nothing else)
      GDV_RETURN_NOT_OK(BindInputs(plan_, schema_, v.cols, v.num_cols, v.num_rows, MemKind::kDevice, stream, &args, &st));
      if (!st.buffers.empty()) return Status::Invalid("internal: staged input in a multi-batch evaluation");
      for (int e = 0; e < v.num_outs; e++) {
        args.SetOutData(e, v.outs[e].data);
        args.SetOutValid(e, v.outs[e].validity);
      }
      args.SetPtr(ArgLayout::kOffSel, v.out_indices);
    }
    BindLiterals(plan_, dev->consts, &args);
    args.Set64(ArgLayout::kOffN, static_cast<uint64_t>(v.num_rows));
    args.SetPtr(ArgLayout::kOffErr, base + err_off);
    args.SetPtr(ArgLayout::kOffAux2, base + cnt_off + 8 * b);
    std::memcpy(pin + stride * b, args.data(), stride);
  }
  EvalTrace trace("filter-project-small", plan_.small->kernel_name + (by_value ? "_small1" : "_small"), nb, stream);
  drain.armed = true;
  if (raises_) GDV_HIP_RETURN_NOT_OK(hipMemsetAsync(base + err_off, 0, 8, stream));
  if (by_value) {
    GDV_RETURN_NOT_OK(rt.Launch(kernel, 1, plan_.opts.waves * 64, pin, stride, stream, kernel.function_small1));
  } else {
    GDV_HIP_RETURN_NOT_OK(hipMemcpyAsync(base, pin, stride * nb, hipMemcpyHostToDevice, stream));
    GDV_RETURN_NOT_OK(rt.LaunchMany(kernel, 1, nb, plan_.opts.waves * 64, base, stream, /*small=*/true));
  }
  if (counts_device != nullptr)
    GDV_HIP_RETURN_NOT_OK(hipMemcpyAsync(counts_device, base + cnt_off, 8 * static_cast<size_t>(nb), hipMemcpyDefault, stream));
  const bool async = (flags & kEvalAsync) != 0 && !raises_ && counts_device != nullptr;
  if (async) {
    if (counts_host != nullptr)
      for (int b = 0; b < nb; b++) counts_host[b] = -1;
    block.release_after(stream);
    lease.ReleaseAfter(stream);  // (nothing to give back when the block went by value)
    drain.armed = false;
    return Status::OK();
  }
  std::vector<int64_t> counts(nb, 0);
  uint32_t err_bits = 0;
  GDV_HIP_RETURN_NOT_OK(hipMemcpyAsync(counts.data(), base + cnt_off, 8 * static_cast<size_t>(nb), hipMemcpyDeviceToHost, stream));
  if (raises_) GDV_HIP_RETURN_NOT_OK(hipMemcpyAsync(&err_bits, base + err_off, 4, hipMemcpyDeviceToHost, stream));
  GDV_HIP_RETURN_NOT_OK(hipStreamSynchronize(stream));
  drain.armed = false;
  if (err_bits != 0) return Status::ExecutionError(ErrorMessage(err_bits));
  if (counts_host != nullptr)
    for (int b = 0; b < nb; b++) counts_host[b] = counts[b];
  return Status::OK();
}

Status FilterProject::EvaluateChain(int64_t num_rows, const ColumnBuffers* cols, int num_cols, OutputBuffers* outs, int num_outs,
                                    void* out_indices, int64_t max_slots, int64_t* num_selected, MemKind mem,
                                    hipStream_t stream, void* count_out) const {
  // index width of the chain: the plan's own, or the narrowest that addresses the batch when it emits none
  const SelectionMode mode = plan_.mode != SelectionMode::kNone ? plan_.mode
                             : (num_rows <= (int64_t{1} << 32) ? SelectionMode::kUInt32 : SelectionMode::kUInt64);
  const int w = IndexWidth(mode);
  // (the two operators are held through locals: a concurrent call that needs the other index width replaces
  // chain_projector_ under the lock, and must not free the one this call is still evaluating)
  std::shared_ptr<Filter> chain_filter;
  std::shared_ptr<Projector> chain_projector;
  {
    std::lock_guard<std::mutex> lock(chain_mu_);
    if (chain_filter_ == nullptr) GDV_RETURN_NOT_OK(Filter::Make(schema_, condition_, Configuration{}, &chain_filter_));
    if (chain_projector_ == nullptr || chain_projector_->plan().mode != mode)
      GDV_RETURN_NOT_OK(Projector::Make(schema_, exprs_, mode, Configuration{}, &chain_projector_));
    chain_filter = chain_filter_;
    chain_projector = chain_projector_;
  }
  std::vector<char> host_idx;
  DeviceBuffer dev_idx;
  void* idx = out_indices;
  if (plan_.mode == SelectionMode::kNone) {
    if (mem == MemKind::kHost) {
      host_idx.resize(static_cast<size_t>(num_rows) * w);
      idx = host_idx.data();
    } else {
      GDV_RETURN_NOT_OK(dev_idx.Allocate(static_cast<size_t>(num_rows) * w));
      idx = dev_idx.get();
    }
    max_slots = num_rows;
  }
  int64_t count = 0;
  GDV_RETURN_NOT_OK(chain_filter->Evaluate(num_rows, cols, num_cols, mode, idx, max_slots, &count, mem, stream, 0, count_out));
  if (count > 0) {
    SelectionView sel;
    sel.mode = mode;
    sel.indices = idx;
    sel.num_slots = count;
    // the projector sizes its checks for `count` rows; the caller's buffers hold num_rows
    GDV_RETURN_NOT_OK(chain_projector->Evaluate(num_rows, cols, num_cols, &sel, outs, num_outs, mem, stream, 0));
  }
  if (num_selected != nullptr) *num_selected = count;
  return Status::OK();
}

Status FilterProject::EvaluateFused(int64_t num_rows, const ColumnBuffers* cols, int num_cols, OutputBuffers* outs,
                                    int num_outs, void* out_indices, int64_t max_slots, int64_t* num_selected, MemKind mem,
                                    hipStream_t stream, uint32_t flags, void* count_out, bool* stalled) const {
  *stalled = false;
  if (num_rows < 0) return Status::Invalid("negative row count");
  if (num_outs != num_outputs() || (num_outs > 0 && outs == nullptr))
    return Status::Invalid("number of output buffers does not match the number of expressions");
  const SelectionMode mode = plan_.mode;
  const int w = IndexWidth(mode);
  if (w != 0) {
    if (out_indices == nullptr && num_rows > 0) return Status::Invalid("Selection vector cannot be null");
    if (max_slots < num_rows)
      return Status::Invalid("Selection vector too small: max slots " + std::to_string(max_slots) + " < rows " +
                             std::to_string(num_rows));
    if (w == 2 && num_rows > 65536) return Status::Invalid("uint16 selection vector cannot address " + std::to_string(num_rows) + " rows");
    if (w == 4 && num_rows > (int64_t(1) << 32)) return Status::Invalid("uint32 selection vector cannot address " + std::to_string(num_rows) + " rows");
  }
  Runtime& rt = Runtime::Get();
  GDV_RETURN_NOT_OK(rt.EnsureDevice());
  const PlanDeviceState* dev = nullptr;
  GDV_RETURN_NOT_OK(states_.Get(plan_, &dev));
  bool async = (flags & kEvalAsync) != 0 && mem == MemKind::kDevice && !raises_ && count_out != nullptr;

  ArgBlock args(plan_.layout);
  Staging st;
  DeviceBuffer scratch;                      // look-back granules | count | error word | tile ticket
  std::vector<DeviceBuffer> staged(mem == MemKind::kHost ? 2 * num_outs + 1 : 0);  // host path: results are produced in HBM first
  StreamDrain drain{stream, !async};         // declared last: drains before any pooled block is freed
  if (num_rows == 0) {
    if (num_selected != nullptr) *num_selected = 0;
    if (count_out != nullptr) GDV_HIP_RETURN_NOT_OK(hipMemsetAsync(count_out, 0, 8, stream));
    return Status::OK();
  }
  GDV_RETURN_NOT_OK(BindInputs(plan_, schema_, cols, num_cols, num_rows, mem, stream, &args, &st));
  BindLiterals(plan_, dev->consts, &args);
  if (!st.buffers.empty()) { async = false; drain.armed = true; }
  args.Set64(ArgLayout::kOffN, static_cast<uint64_t>(num_rows));

  if (int64_t* seen = pinned_count_.load(std::memory_order_relaxed)) {  // what an earlier asynchronous call selected
    const int64_t share = *reinterpret_cast<volatile int64_t*>(seen);  // rows selected per 1024, written by one launch
    if (share >= 0 && share <= 1024) selected_per_1024_.store(static_cast<int>(share), std::memory_order_relaxed);
  }
  // which shape: the windowed kernel unless recent batches selected more rows than its LDS window holds (the
  // direct kernel takes the same argument block: PlanFilterProject checks that its literals and constants are a
  // prefix of the windowed plan's)
  const CompiledKernel* kernel = dev->kernel.load();
  const KernelPlan* running = &plan_;
  if (which_kernel() == 1 && !EngineKnobs::Get().fp_window_only) {
    GDV_RETURN_NOT_OK(VarlenLaunch::EnsureExact(plan_, dev, rt));
    kernel = dev->kernel_exact.load();
    running = plan_.exact.get();
  }
  // one workgroup tile: waves x rounds x sub-tiles x 64 rows (the windowed kernel walks GDV_FP_K rounds per look-back)
  const int64_t rows_per_wg = 64 * static_cast<int64_t>(plan_.opts.subtiles) * plan_.opts.waves * std::max(1, running->fp_rounds);
  const int64_t grid = (num_rows + rows_per_wg - 1) / rows_per_wg;
  if (grid > 0x7fffffff) return Status::Invalid("batch too large for the fused filter-project launch");
  auto up = [](size_t v) { return (v + 255) & ~size_t{255}; };
  const size_t state_b = up(static_cast<size_t>(grid) * 8);
  GDV_RETURN_NOT_OK(scratch.Allocate(state_b + 256));
  char* const base = scratch.as<char>();
  // granules, count (+0), error word (+64) and the tile ticket (+128, round 6) start at zero (one memset)
  GDV_HIP_RETURN_NOT_OK(hipMemsetAsync(base, 0, state_b + 256, stream));
  drain.armed = true;  // from here on an error return must wait for what was enqueued (re-disarmed on the async exit)
  args.SetPtr(ArgLayout::kOffMask, base);
  args.SetPtr(ArgLayout::kOffCounts, base + state_b);
  args.SetPtr(ArgLayout::kOffErr, base + state_b + 64);

  // outputs: the validity (and bool value) bitmaps are OR-ed into at tile boundaries -> pre-zeroed
  std::vector<void*> dev_data(num_outs), dev_valid(num_outs);
  for (int e = 0; e < num_outs; e++) {
    const DataType& t = plan_.output_types[e];
    const int64_t vbytes = Projector::ValidityBytes(num_rows), dbytes = Projector::DataBytes(t, num_rows);
    if (mem == MemKind::kHost) {
      const int64_t host_v = BytesForBits(num_rows), host_d = t.id == kBool ? BytesForBits(num_rows) : dbytes;
      if (outs[e].validity == nullptr || outs[e].data == nullptr || outs[e].validity_size < host_v || outs[e].data_size < host_d)
        return Status::Invalid("output buffer " + std::to_string(e) + " too small");
      GDV_RETURN_NOT_OK(staged[2 * e].Allocate(std::max<int64_t>(vbytes, 8)));
      GDV_RETURN_NOT_OK(staged[2 * e + 1].Allocate(std::max<int64_t>(dbytes, 8)));
      dev_valid[e] = staged[2 * e].get();
      dev_data[e] = staged[2 * e + 1].get();
    } else {
      if (outs[e].validity == nullptr || outs[e].data == nullptr || outs[e].validity_size < vbytes || outs[e].data_size < dbytes)
        return Status::Invalid("output buffer " + std::to_string(e) + " too small (device buffers need 8-byte word granularity: " +
                               std::to_string(vbytes) + " validity bytes, " + std::to_string(dbytes) + " data bytes)");
      dev_valid[e] = outs[e].validity;
      dev_data[e] = outs[e].data;
    }
    GDV_HIP_RETURN_NOT_OK(hipMemsetAsync(dev_valid[e], 0, vbytes, stream));
    if (t.id == kBool) GDV_HIP_RETURN_NOT_OK(hipMemsetAsync(dev_data[e], 0, dbytes, stream));
    args.SetOutData(e, dev_data[e]);
    args.SetOutValid(e, dev_valid[e]);
  }
  void* dev_idx = out_indices;
  if (w != 0 && mem == MemKind::kHost) {
    GDV_RETURN_NOT_OK(staged[2 * num_outs].Allocate(num_rows * w));
    dev_idx = staged[2 * num_outs].get();
  }
  args.SetPtr(ArgLayout::kOffSel, dev_idx);
  GDV_RETURN_NOT_OK(st.FlushIn(stream));

  EvalTrace trace("filter-project", running->kernel_name, num_rows, stream);
  GDV_RETURN_NOT_OK(rt.Launch(*kernel, grid, plan_.opts.waves * 64, args.data(), args.size(), stream));
  const char* count_dev = base + state_b;
  // the count leaves through a one-thread kernel: -1 when the look-back gave up (GDV_ERR_STALL in the error word) —
  // round 4 copied the word as it was and an asynchronous caller never learnt that the outputs were not complete
  int64_t* telemetry = nullptr;
  if (async && plan_.exact != nullptr) {  // (two shapes to choose between: let the next call learn this one's count)
    telemetry = pinned_count_.load(std::memory_order_relaxed);
    if (telemetry == nullptr) {
      int64_t* fresh = nullptr;
      if (hipHostMalloc(reinterpret_cast<void**>(&fresh), 64, hipHostMallocDefault) == hipSuccess && fresh != nullptr) {
        fresh[0] = -1;
        int64_t* expected = nullptr;
        if (pinned_count_.compare_exchange_strong(expected, fresh)) telemetry = fresh;
        else { (void)hipHostFree(fresh); telemetry = expected; }
      } else {
        (void)hipGetLastError();
      }
    }
  }
  if (count_out != nullptr || telemetry != nullptr)
    GDV_HIP_RETURN_NOT_OK(LaunchPublishCount(static_cast<int64_t*>(count_out), reinterpret_cast<const int64_t*>(count_dev),
                                             reinterpret_cast<const uint32_t*>(base + state_b + 64), kErrStall, stream, telemetry, num_rows));
  if (async) {
    if (num_selected != nullptr) *num_selected = -1;
    scratch.release_after(stream);
    drain.armed = false;
    return Status::OK();
  }
  int64_t count = 0;
  uint32_t err_bits = 0;
  GDV_HIP_RETURN_NOT_OK(hipMemcpyAsync(&count, count_dev, 8, hipMemcpyDeviceToHost, stream));
  GDV_HIP_RETURN_NOT_OK(hipMemcpyAsync(&err_bits, base + state_b + 64, 4, hipMemcpyDeviceToHost, stream));
  GDV_HIP_RETURN_NOT_OK(hipStreamSynchronize(stream));
  if ((err_bits & kErrStall) != 0 || EngineKnobs::Get().fp_force_stall) {
    drain.armed = false;
    *stalled = true;
    return Status::OK();
  }
  if (err_bits != 0) return Status::ExecutionError(ErrorMessage(err_bits));
  selected_per_1024_.store(static_cast<int>(count * 1024 / num_rows), std::memory_order_relaxed);
  if (mem == MemKind::kHost && count > 0) {
    for (int e = 0; e < num_outs; e++) {
      const DataType& t = plan_.output_types[e];
      GDV_HIP_RETURN_NOT_OK(hipMemcpyAsync(outs[e].validity, dev_valid[e], BytesForBits(count), hipMemcpyDeviceToHost, stream));
      GDV_HIP_RETURN_NOT_OK(hipMemcpyAsync(outs[e].data, dev_data[e], t.id == kBool ? BytesForBits(count) : count * t.byte_width(),
                                           hipMemcpyDeviceToHost, stream));
    }
    if (w != 0) GDV_HIP_RETURN_NOT_OK(hipMemcpyAsync(out_indices, dev_idx, count * w, hipMemcpyDeviceToHost, stream));
    GDV_HIP_RETURN_NOT_OK(hipStreamSynchronize(stream));
  }
  drain.armed = false;
  if (num_selected != nullptr) *num_selected = count;
  return Status::OK();
}

}  // namespace gdv
