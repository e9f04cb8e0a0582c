// The var-len launch (VarlenLaunch, gdv_engine_internal.h): what Projector::Evaluate and
// Projector::EvaluateAsyncStage enqueue for a plan with var-len outputs.
#include "gdv_engine_internal.h"

namespace gdv::engine {

VarlenLaunch::VarlenLaunch(const KernelPlan& plan, const PlanDeviceState* dev, Runtime& rt, int64_t out_rows,
                           hipStream_t stream)
    : plan_(plan), dev_(dev), rt_(rt), out_rows_(out_rows), stream_(stream) {
  const int nv = plan.num_varlen_outputs;
  if (nv == 0) return;
  ng = (nv + 1) / 2;
  // (tile of the scanner-shaped kernel: a wave plan's fallback has its own)
  sc_u = plan.general_subtiles > 0 ? plan.general_subtiles : plan.opts.subtiles;
  sc_w = plan.general_waves > 0 ? plan.general_waves : plan.opts.waves;
  const int64_t rows_wg = 64 * static_cast<int64_t>(sc_u) * sc_w;
  ntiles = (out_rows + rows_wg - 1) / rows_wg;
  // head of the state block, one memset and one read-back per launch:
  // [error word | grand totals (2 * ng) | wave shape: totals of the scanned segments]
  for (int sgm : plan.wave_segments) nseg = std::max(nseg, sgm + 1);
  totals_bytes = static_cast<size_t>(2 * ng) * 8;
  head_bytes = 8 + totals_bytes + static_cast<size_t>(nseg) * 8;
  state_bytes = 8 + totals_bytes + static_cast<size_t>(2 * ng * ntiles) * 8;
  for (int e = 0; e < static_cast<int>(plan.output_types.size()); e++)
    if (plan.output_types[e].is_varlen()) vl.push_back(e);
  // wave shape
  const int64_t rows_wt = 64 * static_cast<int64_t>(plan.opts.subtiles);
  nwt = (out_rows + rows_wt - 1) / rows_wt;
  seg_stride = (nwt + 3) & ~int64_t{3};  // the scan kernels read the totals 16 bytes at a time
}

Status VarlenLaunch::EnsureExact(const KernelPlan& plan, const PlanDeviceState* dev, Runtime& rt) {
  PlanDeviceState* d = const_cast<PlanDeviceState*>(dev);
  if (d->kernel_exact.load() == nullptr) {
    const CompiledKernel* k = nullptr;
    GDV_RETURN_NOT_OK(rt.GetKernel(plan.exact->source, plan.exact->kernel_name, &k));
    if (plan.exact->prepass) {
      const CompiledKernel* kp = nullptr;
      GDV_RETURN_NOT_OK(rt.GetKernel(plan.exact->prepass->source, plan.exact->prepass->kernel_name, &kp));
      d->kernel_pre_exact.store(kp);
    }
    d->kernel_exact.store(k);
  }
  return Status::OK();
}

Status VarlenLaunch::EnsureGeneral(const KernelPlan& plan, const PlanDeviceState* dev, Runtime& rt) {
  if (dev->kernel_general.load() == nullptr) {
    const CompiledKernel* k = nullptr;
    GDV_RETURN_NOT_OK(rt.GetKernel(plan.source_general, plan.kernel_name_general, &k));
    const_cast<PlanDeviceState*>(dev)->kernel_general.store(k);
  }
  return Status::OK();
}

Status VarlenLaunch::EnqueueWave(ArgBlock* args, bool exact, bool zero_counts) {
  const CompiledKernel* k_main = dev_->kernel.load();
  const CompiledKernel* k_pre = dev_->kernel_pre;
  if (exact) {
    GDV_RETURN_NOT_OK(EnsureExact());
    k_main = dev_->kernel_exact.load();
    k_pre = dev_->kernel_pre_exact.load();
  }
  if (nseg > 0 && (plan_.prepass == nullptr || k_pre == nullptr))
    return Status::ExecutionError("internal: wave plan without a pre-pass");
  hipStream_t stream = stream_;
  if (head_.get() == nullptr) {
    GDV_RETURN_NOT_OK(head_.Allocate(head_bytes));
    if (nseg > 0) {
      GDV_RETURN_NOT_OK(counts_.Allocate(static_cast<size_t>(nseg * seg_stride) * 4 + 64));
      GDV_RETURN_NOT_OK(bases_.Allocate(static_cast<size_t>(nseg * seg_stride) * 8));
      GDV_RETURN_NOT_OK(chunks_.Allocate(static_cast<size_t>(nseg * ScanChunks(nwt)) * 8));
      // the pre-pass reads columns the main kernel has bound (and, on the host path, staged) already
      const KernelPlan& pp = *plan_.prepass;
      pargs_.emplace(pp.layout);
      for (size_t kp = 0; kp < pp.input_fields.size(); kp++) {
        int k = -1;
        for (size_t j = 0; j < plan_.input_fields.size(); j++)
          if (plan_.input_fields[j] == pp.input_fields[kp]) k = static_cast<int>(j);
        if (k < 0 || (pp.input_needs_values[kp] && !plan_.input_needs_values[k]) ||
            (pp.input_needs_validity[kp] && !plan_.input_needs_validity[k]))
          return Status::ExecutionError("internal: pre-pass input not bound by the main kernel");
        pargs_->CopyInSlot(static_cast<int>(kp), *args, k);
      }
      BindLiterals(pp, dev_->consts_pre, &*pargs_);
      pargs_->Set64(ArgLayout::kOffN, static_cast<uint64_t>(out_rows_));
      pargs_->SetPtr(ArgLayout::kOffErr, head_.get());
      pargs_->SetPtr(ArgLayout::kOffCounts, counts_.get());
      pargs_->Set64(ArgLayout::kOffAux1, static_cast<uint64_t>(seg_stride));
      // selection mode (round 5): the pre-pass walks the same slots — the (staged) selection vector, the rows word
      pargs_->Set64(ArgLayout::kOffSel, args->Get64(ArgLayout::kOffSel));
      pargs_->Set64(ArgLayout::kOffAux2, args->Get64(ArgLayout::kOffAux2));
    }
  }
  char* const head = head_.as<char>();
  args->SetPtr(ArgLayout::kOffErr, head);
  args->SetPtr(ArgLayout::kOffCounts, head + 8);
  args->SetPtr(ArgLayout::kOffMask, bases_.get());  // (null without scanned segments)
  args->Set64(ArgLayout::kOffAux1, static_cast<uint64_t>(seg_stride));
  GDV_HIP_RETURN_NOT_OK(hipMemsetAsync(head, 0, head_bytes, stream));
  const int64_t grid = GridFor(plan_, out_rows_);
  if (nseg > 0) {
    // a second stage whose gate is closed walks 0 rows: its pre-pass writes no count, the scan must still see zeros
    // (the same for a selection whose slot count sits in device memory: wave tiles past it write no count)
    if (zero_counts)
      GDV_HIP_RETURN_NOT_OK(hipMemsetAsync(counts_.get(), 0, static_cast<size_t>(nseg * seg_stride) * 4 + 64, stream));
    GDV_RETURN_NOT_OK(rt_.Launch(*k_pre, std::min<int64_t>(grid, static_cast<int64_t>(rt_.num_cus()) * 16),
                                 plan_.opts.waves * 64, pargs_->data(), pargs_->size(), stream));
    // the scan also writes each output's closing offset: offsets[out_rows] of the buffer bound in `args`
    int32_t* closing[kMaxScanSegments] = {};
    for (size_t v = 0; v < vl.size(); v++)
      if (plan_.wave_segments[v] >= 0)
        closing[plan_.wave_segments[v]] = static_cast<int32_t*>(args->GetOutOffsets(vl[v])) + out_rows_;
    GDV_HIP_RETURN_NOT_OK(LaunchSegmentedOffsetsScan(counts_.as<uint32_t>(), nwt, seg_stride, nseg,
                                                     chunks_.as<uint64_t>(), bases_.as<uint64_t>(),
                                                     reinterpret_cast<uint64_t*>(head + 8 + totals_bytes), closing, stream));
  }
  return rt_.Launch(*k_main, grid, plan_.opts.waves * 64, args->data(), args->size(), stream);
}

Status VarlenLaunch::EnqueueScanner(ArgBlock* args, const CompiledKernel& kernel, int64_t grid) {
  hipStream_t stream = stream_;
  if (state_.get() == nullptr) GDV_RETURN_NOT_OK(state_.Allocate(state_bytes));
  char* const state = state_.as<char>();
  args->SetPtr(ArgLayout::kOffErr, state);
  args->SetPtr(ArgLayout::kOffCounts, state + 8);
  args->SetPtr(ArgLayout::kOffMask, state + 8 + totals_bytes);
  GDV_HIP_RETURN_NOT_OK(hipMemsetAsync(state, 0, state_bytes, stream));
  return rt_.Launch(kernel, grid, sc_w * 64, args->data(), args->size(), stream);
}

void VarlenLaunch::ReleaseAfter(hipStream_t stream) {
  state_.release_after(stream);
  head_.release_after(stream);
  counts_.release_after(stream);
  bases_.release_after(stream);
  chunks_.release_after(stream);
}

}  // namespace gdv::engine
