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
