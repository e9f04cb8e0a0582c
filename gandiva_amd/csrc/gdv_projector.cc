#include "gdv_engine_internal.h"

namespace gdv {

using namespace engine;

namespace {

LruCache<Projector>& ProjectorCache() {
  static LruCache<Projector> c(500);
  return c;
}

// an "invalid argument" of a plan whose upper / lower map through utf8proc's table names them: they are what raises on text
// that is not UTF-8
std::string RaiseMessage(const KernelPlan& plan, uint32_t bits) {
  std::string m = ErrorMessage(bits);
  if ((bits & 4u) && !plan.utf8_case_fns.empty())
    m += " (" + plan.utf8_case_fns + " under GDV_UTF8_CASE=1: text that is not UTF-8 raises)";
  return m;
}

}  // namespace

// ------------------------------------------------------------------ Projector

int64_t Projector::VarlenBytesHint(int i, int64_t rows) const {
  if (i < 0 || static_cast<size_t>(i) >= out_bytes_x16_.size() || rows <= 0) return 0;
  const int64_t x16 = out_bytes_x16_[i].load(std::memory_order_relaxed);
  if (x16 <= 0) return 0;
  // (an eighth of head room: batches of one column rarely differ by more)
  const __int128 bytes = static_cast<__int128>(x16) * rows / 16 * 9 / 8 + 256;
  return static_cast<int64_t>(std::min<__int128>(bytes, (int64_t{1} << 31) - 64));
}

Status Projector::Make(const Schema& schema, const std::vector<ExpressionPtr>& exprs,
                       SelectionMode mode, const Configuration& config,
                       std::shared_ptr<Projector>* out) {
  if (out == nullptr) return Status::Invalid("Projector::Make: null output pointer");
  if (exprs.empty()) return Status::Invalid("Expressions cannot be empty");
  CodegenOptions opts = CodegenOptions::FromEnv();
  std::string key = "P|" + SchemaKey(schema) + "|";
  for (auto& e : exprs) {
    if (!e) return Status::Invalid("Expression cannot be null");
    key += e->CacheKey() + ";";
  }
  key += "|m" + std::to_string(static_cast<int>(mode)) + "|" + opts.Key() +
         (config.optimize ? "|O" : "|o");
  if (auto hit = ProjectorCache().Get(key)) {
    *out = hit;
    return Status::OK();
  }
  auto p = std::make_shared<Projector>();
  p->schema_ = schema;
  p->plan_schema_ = schema;
  const std::vector<ExpressionPtr>* planned = &exprs;
  StagedExpressions staged;
  // (round 3: in every selection mode — the first stage is built in the SAME mode, so it evaluates,
  // and can raise, only on the selected rows, and writes one temporary row per slot)
  StageMaterialisedValues(schema, exprs, &staged, opts);
  if (!staged.pre.empty()) {
    for (auto& e : exprs) GDV_RETURN_NOT_OK(ValidateExpression(schema, *e));  // errors name the caller's trees
    GDV_RETURN_NOT_OK(Projector::Make(schema, staged.pre, mode, config, &p->pre_));
    p->plan_schema_ = staged.schema;
    planned = &staged.main;
    p->stage_hints_ = std::vector<std::atomic<int64_t>>(staged.pre.size());
  }
  if (p->pre_) opts.rows_word = true;  // (second stage: GDV_ROWS reads the gate's word of an asynchronous evaluation)
  GDV_RETURN_NOT_OK(PlanProjector(p->plan_schema_, *planned, mode, opts, &p->plan_,
                                  mode == SelectionMode::kNone ? 0x7fffffff : static_cast<int>(schema.size())));
  p->out_bytes_x16_ = std::vector<std::atomic<int64_t>>(exprs.size());
  const PlanDeviceState* st = nullptr;
  GDV_RETURN_NOT_OK(Runtime::Get().EnsureDevice());
  if (p->pre_ == nullptr)
    ArmTier0(schema, exprs, /*is_filter=*/false, p->plan_, &p->tier0_, &p->tier0_pending_);
  if (!p->tier0_) GDV_RETURN_NOT_OK(p->states_.Get(p->plan_, &st));  // compiles + loads on the calling thread's device
  ProjectorCache().Put(key, p);
  *out = p;
  return Status::OK();
}

// Checks the caller's output buffers and binds them: in place (device buffers, registered host memory) or through
// the staging block.  dev_* receive what the kernel writes to, per output.
Status Projector::BindOutputs(int64_t out_rows, OutputBuffers* outs, int num_outs, MemKind mem, hipStream_t stream,
                              ArgBlock& args, Staging& st, std::vector<void*>& dev_data, std::vector<void*>& dev_valid,
                              std::vector<void*>& dev_offs) const {
  for (int e = 0; e < num_outs; e++) {
    const DataType& t = plan_.output_types[e];
    const int64_t need_valid_dev = ValidityBytes(out_rows);
    const int64_t need_data_dev = t.is_varlen() ? 0 : DataBytes(t, out_rows);
    const int64_t need_offs = t.is_varlen() ? (out_rows + 1) * 4 : 0;
    if (t.is_varlen() && (outs[e].offsets == nullptr || outs[e].offsets_size < need_offs))
      return Status::Invalid("output buffer " + std::to_string(e) + ": offsets buffer too small (" +
                             std::to_string(need_offs) + " bytes needed)");
    if (mem == MemKind::kHost) {
      const int64_t need_data_host = t.id == kBool ? BytesForBits(out_rows) : need_data_dev;
      if (outs[e].validity_size < BytesForBits(out_rows) || outs[e].data_size < need_data_host ||
          (out_rows > 0 && (outs[e].validity == nullptr || (outs[e].data == nullptr && !t.is_varlen()))))
        return Status::Invalid("output buffer " + std::to_string(e) + " too small");
      const int64_t vbytes = out_rows > 0 ? BytesForBits(out_rows) : 0;
      // Buffers inside a registered host range (gdv_host_register / gdv_host_alloc) that hold whole
      // 8-byte words are written in place by the kernel; the others come back through the staging block.
      const bool fixed = !t.is_varlen();
      dev_valid[e] = fixed && outs[e].validity_size >= need_valid_dev && (reinterpret_cast<uintptr_t>(outs[e].validity) & 7) == 0
                         ? HostRegistry::Get().View(outs[e].validity, need_valid_dev) : nullptr;
      if (dev_valid[e] == nullptr)
        GDV_RETURN_NOT_OK(st.Out(std::max<int64_t>(need_valid_dev, 8), vbytes, outs[e].validity, &dev_valid[e]));
      if (t.is_varlen()) {
        GDV_RETURN_NOT_OK(st.Out(need_offs, out_rows > 0 ? need_offs : 0, outs[e].offsets, &dev_offs[e]));
      } else {
        const int64_t dbytes = out_rows == 0 ? 0 : (t.id == kBool ? vbytes : need_data_dev);
        dev_data[e] = fixed && outs[e].data_size >= need_data_dev && (reinterpret_cast<uintptr_t>(outs[e].data) & 15) == 0
                          ? HostRegistry::Get().View(outs[e].data, need_data_dev) : nullptr;
        if (dev_data[e] == nullptr)
          GDV_RETURN_NOT_OK(st.Out(std::max<int64_t>(need_data_dev, 8), dbytes, outs[e].data, &dev_data[e]));
      }
    } else {
      if (outs[e].validity_size < need_valid_dev || outs[e].data_size < need_data_dev)
        return Status::Invalid("output buffer " + std::to_string(e) +
                               " too small (device buffers need 8-byte word granularity: " +
                               std::to_string(need_valid_dev) + " validity bytes, " +
                               std::to_string(need_data_dev) + " data bytes)");
      dev_valid[e] = outs[e].validity;
      dev_data[e] = outs[e].data;
      dev_offs[e] = outs[e].offsets;
    }
    args.SetOutData(e, dev_data[e]);
    args.SetOutValid(e, dev_valid[e]);
    args.SetOutOffsets(e, dev_offs[e]);
    // offsets[0] = 0 is written by the byte pass with every other offset; an empty selection
    // launches nothing (the closing offset comes from the scan launcher)
    if (t.is_varlen() && out_rows == 0) GDV_HIP_RETURN_NOT_OK(hipMemsetAsync(dev_offs[e], 0, 4, stream));
  }
  return Status::OK();
}

// The kernels of one synchronous var-len evaluation, a wait after each launch: err_bits and seg (bytes per
// var-len output) are what the last one left.
Status Projector::LaunchVarlen(VarlenLaunch& vlaunch, ArgBlock& args, std::vector<uint64_t>& back, std::vector<uint64_t>& seg,
                               uint32_t& err_bits, hipStream_t stream) const {
  const PlanDeviceState* dev = vlaunch.dev();
  const int nv = plan_.num_varlen_outputs;
  const int ng = vlaunch.ng;
  const CompiledKernel* active = dev->kernel.load();
  auto run = [&](int64_t grid) -> Status {  // scanner shape
    GDV_RETURN_NOT_OK(vlaunch.EnqueueScanner(&args, *active, grid));
    GDV_HIP_RETURN_NOT_OK(hipMemcpyAsync(back.data(), vlaunch.scanner_state(), 8 + vlaunch.totals_bytes, hipMemcpyDeviceToHost, stream));
    GDV_HIP_RETURN_NOT_OK(hipStreamSynchronize(stream));
    err_bits = static_cast<uint32_t>(back[0]);
    for (int i = 0; i < 2 * ng; i++) seg[i] = back[1 + i];
    return Status::OK();
  };
  auto run_wave = [&](bool exact) -> Status {
    GDV_RETURN_NOT_OK(vlaunch.EnqueueWave(&args, exact, /*zero_counts=*/false));
    GDV_HIP_RETURN_NOT_OK(hipMemcpyAsync(back.data(), vlaunch.wave_head(), vlaunch.head_bytes, hipMemcpyDeviceToHost, stream));
    GDV_HIP_RETURN_NOT_OK(hipStreamSynchronize(stream));
    err_bits = static_cast<uint32_t>(back[0]);
    for (int v = 0; v < nv; v++) seg[v] = back[vlaunch.wave_total_word(v)];
    return Status::OK();
  };
  const bool has_exact = plan_.wave_tiles && plan_.exact != nullptr;
  const int64_t scanner_grid = vlaunch.scanner_grid();
  // Outputs that are an input column's (mapped) bytes — a column passed through, upper(col),
  // lower(col) — are first evaluated OPTIMISTICALLY: bytes copied by the byte sweep as they
  // are read, offsets = input offsets rebased, no scan.  That holds unless a NULL row carries
  // bytes (Arrow allows it, producers rarely do it); the kernel then raises NOTFLAT and the
  // batch is re-run with those outputs on the general path.  The wave shape adds the ASCII
  // assumption of its pre-pass (NOTASCII).
  // Round 4 — which kernels a batch runs on is decided PER BATCH (it used to be sticky for good:
  // one byte >= 0x80 sent every later batch of the Projector to the scanner kernel, 0.27 of the
  // roofline):  NOTASCII -> the wave shape's EXACT variant (flags from the sweep: same structure,
  // the pre-pass reads the bytes once more), which also tells whether the batch really held such
  // bytes — if not, the next batch starts on the optimistic kernels again;  NOTFLAT -> the
  // scanner-shaped general kernel, and the optimistic kernels get another try every 16th batch.
  const bool has_optimistic = plan_.wave_tiles || plan_.has_flat_output;
  if (!has_optimistic) {
    active = dev->kernel.load();
    GDV_RETURN_NOT_OK(run(scanner_grid));
  } else {
    const bool no_optflat = EngineKnobs::Get().no_optflat;
    const int hint = path_hint_.load(std::memory_order_relaxed);
    // (the counter advances for the batches that would start on the general kernel only)
    int path = VarlenStartPath(hint, has_optimistic, has_exact, no_optflat, 0);
    if (path == 2 && !no_optflat)
      path = VarlenStartPath(hint, has_optimistic, has_exact, no_optflat, general_batches_.fetch_add(1, std::memory_order_relaxed));
    if (path == 0) {
      if (plan_.wave_tiles) {
        GDV_RETURN_NOT_OK(run_wave(false));
      } else {
        active = dev->kernel.load();
        GDV_RETURN_NOT_OK(run(scanner_grid));
      }
      path = VarlenNextPath(0, err_bits, has_exact);
      if (path == 0) path_hint_.store(0, std::memory_order_relaxed);
    }
    if (EngineKnobs::Get().trace)
      fprintf(stderr, "[gdv] var-len path after the optimistic attempt: %d (error bits 0x%x)\n", path, err_bits);
    if (path == 1) {
      GDV_RETURN_NOT_OK(run_wave(true));
      if (EngineKnobs::Get().trace) fprintf(stderr, "[gdv] exact wave variant ran (error bits 0x%x)\n", err_bits);
      path = VarlenNextPath(1, err_bits, has_exact);
      if (path == 1) path_hint_.store((err_bits & kSawUtf8) ? 1 : 0, std::memory_order_relaxed);
    }
    if (path == 2) {
      GDV_RETURN_NOT_OK(vlaunch.EnsureGeneral());
      active = dev->kernel_general.load();
      GDV_RETURN_NOT_OK(run(scanner_grid));
      path_hint_.store(2, std::memory_order_relaxed);
    }
  }
  err_bits &= ~(kNotFlat | kNotAscii | kSawUtf8);
  if (err_bits & 8u) {
    // The scan made no progress for a very long time: some workgroup of the grid was not
    // scheduled while later ones waited for it.  Never observed (workgroups start in index
    // order); the serial-safe configuration — scanner + ONE worker workgroup walking all
    // tiles in order — cannot wait on anything unscheduled.
    GDV_RETURN_NOT_OK(run(2));
    if (err_bits & 8u) return Status::ExecutionError("var-len projection: device scan stalled");
  }
  return Status::OK();
}

// Var-len outputs of a synchronous evaluation: the launches, then capacities, totals and the size hints; host
// buffers take a second round of launches into byte buffers sized by the first.
Status Projector::EvaluateVarlen(VarlenLaunch& vlaunch, ArgBlock& args, Staging& st, OutputBuffers* outs, MemKind mem,
                                 int64_t out_rows, std::vector<void*>& dev_data, std::vector<uint64_t>& totals,
                                 uint32_t& err_bits, hipStream_t stream) const {
  const int nv = plan_.num_varlen_outputs;
  const std::vector<int>& vl = vlaunch.vl;
  std::vector<uint64_t> back(vlaunch.head_bytes / 8, 0);
  std::vector<uint64_t> seg(2 * vlaunch.ng, 0);
  for (int v = 0; v < nv; v++) args.SetOutCap(vl[v], mem == MemKind::kHost ? 0 : outs[vl[v]].data_size);
  GDV_RETURN_NOT_OK(LaunchVarlen(vlaunch, args, back, seg, err_bits, stream));
  Status capacity = Status::OK();
  for (int v = 0; v < nv; v++) {
    const int e = vl[v];
    totals[e] = seg[v];
    // (totals saturate at 2^31 - 1, so a total of exactly that many bytes cannot be told from an
    // overflow: rejected too — one byte short of what int32 offsets could address)
    if (totals[e] >= 0x7fffffffull)
      return Status::Invalid("var-len output " + std::to_string(e) + " exceeds 2 GiB");
    const int64_t have = outs[e].data_size;
    outs[e].data_size = static_cast<int64_t>(totals[e]);  // bytes needed / produced
    if (static_cast<size_t>(e) < out_bytes_x16_.size() && out_rows > 0) {
      const int64_t seen = static_cast<int64_t>(totals[e]) * 16 / out_rows + 1;
      // a DECAYING maximum: a batch that produces more raises the hint at once, one that produces
      // less lets it sink by an eighth towards what it produced — one outlier batch no longer makes
      // every later call allocate for its ratio for good (round-3 advisor)
      int64_t cur = out_bytes_x16_[e].load(std::memory_order_relaxed);
      for (;;) {
        const int64_t next = seen >= cur ? seen : std::max(seen, cur - (cur >> 3) - 1);
        if (next == cur || out_bytes_x16_[e].compare_exchange_weak(cur, next, std::memory_order_relaxed)) break;
      }
    }
    if (have < static_cast<int64_t>(totals[e]) || (totals[e] > 0 && outs[e].data == nullptr))
      capacity = Status::Invalid("output buffer " + std::to_string(e) + ": data capacity " +
                                 std::to_string(have) + " < " + std::to_string(totals[e]) +
                                 " bytes needed (data_size updated; retry with a larger buffer)");
  }
  if (err_bits != 0) return Status::ExecutionError(RaiseMessage(plan_, err_bits));
  GDV_RETURN_NOT_OK(capacity);
  if (mem == MemKind::kHost) {
    bool any = false;
    for (int v = 0; v < nv; v++) {
      const int e = vl[v];
      DeviceBuffer& dd = st.Add();
      GDV_RETURN_NOT_OK(dd.Allocate(std::max<uint64_t>(totals[e], 8)));
      dev_data[e] = dd.get();
      args.SetOutData(e, dev_data[e]);
      args.SetOutCap(e, static_cast<int64_t>(totals[e]));
      any |= totals[e] > 0;
    }
    if (any) GDV_RETURN_NOT_OK(LaunchVarlen(vlaunch, args, back, seg, err_bits, stream));
  }
  return Status::OK();
}

Status Projector::Evaluate(int64_t num_rows, const ColumnBuffers* cols, int num_cols,
                           const SelectionView* sel, OutputBuffers* outs, int num_outs,
                           MemKind mem, hipStream_t stream, uint32_t flags, const void* rows_word, void* err_word) const {
  if (num_rows <= 0) return Status::Invalid("RecordBatch must be non-empty.");
  const bool two_stage = pre_ != nullptr && !(flags & kEvalStaged);  // (kEvalStaged: the caller ran the first stage)
  if (outs == nullptr) return Status::Invalid("Output array vector cannot be null");
  if (num_outs != num_outputs())
    return Status::Invalid("number of output buffers (" + std::to_string(num_outs) +
                           ") does not match the number of expressions (" +
                           std::to_string(num_outputs()) + ")");
  const bool has_sel = sel != nullptr && sel->mode != SelectionMode::kNone;
  if (has_sel != (plan_.mode != SelectionMode::kNone) || (has_sel && sel->mode != plan_.mode))
    return Status::Invalid("selection vector type does not match the mode the projector was built for");
  const int64_t out_rows = has_sel ? sel->num_slots : num_rows;
  if (has_sel) {
    // what the selection vector's index type can address bounds its slot count
    const int64_t cap = sel->mode == SelectionMode::kUInt16 ? 65536
                        : sel->mode == SelectionMode::kUInt32 ? (int64_t{1} << 32)
                                                              : INT64_MAX;
    if (sel->num_slots < 0 || sel->num_slots > cap)
      return Status::Invalid("selection vector: invalid slot count " + std::to_string(sel->num_slots));
  }
  if (has_sel && sel->num_slots_device != nullptr &&
      (mem != MemKind::kDevice || plan_.num_varlen_outputs > 0 || two_stage))
    return Status::Invalid("a device-resident slot count needs device buffers and fixed-width outputs "
                           "(read the count back and pass it as num_slots instead)");
  Runtime& rt = Runtime::Get();
  GDV_RETURN_NOT_OK(rt.EnsureDevice());
  const PlanDeviceState* dev = nullptr;
  // tier 0: while the specialised kernel is still compiling this evaluation interprets the plan's program instead
  // (row mode and selection mode alike; the asynchronous and gated paths — rows_word, err_word — stay on the specialised kernel)
  const bool tier0 = UseTier0() && rows_word == nullptr && err_word == nullptr;
  GDV_RETURN_NOT_OK(states_.Get(plan_, &dev, /*need_kernel=*/!tier0));

  ArgBlock args(plan_.layout);
  Staging st;
  DeviceBuffer err;
  VarlenLaunch vlaunch(plan_, dev, rt, out_rows, stream);  // var-len outputs: geometry + pooled scratch of their launches
  StageColumns stage;  // two-stage plans: the first stage's temporary columns (outlive the drain below)
  // declared last: drains first (the byte pass of a var-len plan reads pooled scratch)
  StreamDrain drain{stream, mem == MemKind::kHost || plan_.has_varlen_output || two_stage};
  if (two_stage) {
    if (num_cols != static_cast<int>(schema_.size()))
      return Status::Invalid("number of columns in batch (" + std::to_string(num_cols) +
                             ") does not match the schema (" + std::to_string(schema_.size()) + ")");
    GDV_RETURN_NOT_OK(stage.Run(*pre_, num_rows, cols, num_cols, mem, stream, has_sel ? sel : nullptr, &stage_hints_));
    cols = stage.cols.data();
    num_cols = static_cast<int>(stage.cols.size());
  }
  if (mem == MemKind::kHost && num_rows <= Staging::kPackRows) GDV_RETURN_NOT_OK(st.EnablePacked());
  GDV_RETURN_NOT_OK(BindInputs(plan_, plan_schema_, cols, num_cols, num_rows, mem, stream, &args, &st,
                               has_sel ? out_rows : -1));
  BindLiterals(plan_, dev->consts, &args);
  // pooled staging blocks (e.g. the zero-padded copy of a tiny var-len buffer) go back to the
  // pool when this call returns: an asynchronous evaluation must not outlive them
  drain.armed = drain.armed || !st.buffers.empty();
  args.Set64(ArgLayout::kOffN, static_cast<uint64_t>(out_rows));

  if (has_sel) {
    const int w = IndexWidth(plan_.mode);
    if (out_rows > 0 && sel->indices == nullptr) return Status::Invalid("selection vector has no buffer");
    if (mem == MemKind::kHost) {
      void* d = nullptr;
      GDV_RETURN_NOT_OK(st.In(sel->indices, out_rows * w, std::max<int64_t>(out_rows, 1) * w, stream, &d));
      args.SetPtr(ArgLayout::kOffSel, d);
    } else {
      args.SetPtr(ArgLayout::kOffSel, sel->indices);
      args.SetPtr(ArgLayout::kOffAux2, sel->num_slots_device);  // null: the count is kOffN
    }
  }
  if (rows_word != nullptr) args.SetPtr(ArgLayout::kOffAux2, rows_word);

  // outputs
  std::vector<void*> dev_data(num_outs, nullptr), dev_valid(num_outs), dev_offs(num_outs, nullptr);
  GDV_RETURN_NOT_OK(BindOutputs(out_rows, outs, num_outs, mem, stream, args, st, dev_data, dev_valid, dev_offs));

  const int nv = plan_.num_varlen_outputs;
  const bool has_err = plan_.can_raise && nv == 0;  // var-len plans keep the error word in their scan-state block
  const bool own_err = has_err && err_word == nullptr;
  if (own_err) {
    GDV_RETURN_NOT_OK(err.Allocate(8));
    GDV_HIP_RETURN_NOT_OK(hipMemsetAsync(err.get(), 0, 8, stream));
    args.SetPtr(ArgLayout::kOffErr, err.get());
  } else if (has_err) {
    args.SetPtr(ArgLayout::kOffErr, err_word);  // the caller's word: raised into, never read here
  }

  GDV_RETURN_NOT_OK(st.FlushIn(stream));
  EvalTrace trace(tier0 ? "project (tier 0: interpreted)" : "project", plan_.kernel_name, out_rows, stream);
  std::vector<uint64_t> totals(num_outs, 0);
  uint32_t err_bits = 0;
  if (nv == 0) {
    if (out_rows > 0 && tier0) {
      GDV_RETURN_NOT_OK(RunTier0(*tier0_, args, out_rows, rt, stream));
    } else if (out_rows > 0) {
      GDV_RETURN_NOT_OK(rt.Launch(*dev->kernel.load(), GridFor(plan_, out_rows), plan_.opts.waves * 64, args.data(),
                                  args.size(), stream));
    }
  } else if (out_rows > 0) {
    // Scanner shape — single launch: workgroup 0 scans the tile totals (granules: tile_starts;
    // grand totals: tile_counts), workers post one granule and poll one.  Wave shape (plans whose
    // output lengths follow from the offsets, gdv_planner.cc): pre-pass -> offsets scan -> main
    // kernel of independent wave tiles; a batch that breaks its ASCII / flat assumption is re-run
    // on the scanner-shaped general kernel.  Device buffers: the caller's capacities are honoured
    // inside the kernels (tiles that do not fit skip their bytes) and the totals say what was
    // needed.  Host buffers: a first launch with capacity 0 sizes the device byte buffers, a
    // second one fills them (the path is PCIe-bound anyway).
    GDV_RETURN_NOT_OK(EvaluateVarlen(vlaunch, args, st, outs, mem, out_rows, dev_data, totals, err_bits, stream));
  } else {
    for (int e = 0; e < num_outs; e++)
      if (plan_.output_types[e].is_varlen()) outs[e].data_size = 0;
  }

  if (own_err)
    GDV_HIP_RETURN_NOT_OK(hipMemcpyAsync(&err_bits, err.get(), 4, hipMemcpyDeviceToHost, stream));
  if (mem == MemKind::kHost) {
    GDV_RETURN_NOT_OK(st.FetchOut(stream));  // validity, fixed-width values, offsets
    for (int e = 0; e < num_outs; e++)       // var-len bytes: sized after the length pass
      if (plan_.output_types[e].is_varlen() && out_rows > 0 && totals[e] > 0)
        GDV_HIP_RETURN_NOT_OK(hipMemcpyAsync(outs[e].data, dev_data[e], totals[e],
                                             hipMemcpyDeviceToHost, stream));
  }
  const bool must_sync = mem == MemKind::kHost || (plan_.can_raise && err_word == nullptr) || !(flags & kEvalAsync) || two_stage;
  if (must_sync) GDV_HIP_RETURN_NOT_OK(hipStreamSynchronize(stream));
  if (err_bits != 0) return Status::ExecutionError(RaiseMessage(plan_, err_bits));
  if (mem == MemKind::kHost) st.Deliver();
  return Status::OK();
}

Status Projector::EvaluateMany(const BatchView* batches, int nb, hipStream_t stream, uint32_t flags) const {
  if (nb <= 0) return Status::OK();
  if (batches == nullptr) return Status::Invalid("null batch list");
  Runtime& rt = Runtime::Get();
  GDV_RETURN_NOT_OK(rt.EnsureDevice());
  const PlanDeviceState* dev = nullptr;
  GDV_RETURN_NOT_OK(states_.Get(plan_, &dev));
  const size_t stride = static_cast<size_t>(plan_.layout.total());
  const bool one_launch = plan_.has_many_entry && dev->kernel.load()->function_many != nullptr && pre_ == nullptr &&
                          plan_.num_varlen_outputs == 0 && !plan_.string_skeleton &&
                          stride * static_cast<size_t>(nb) <= Runtime::kPinnedBlock && nb <= 65535 &&
                          !EngineKnobs::Get().no_evaluate_many;
  if (!one_launch) {
    // batch by batch, all enqueued on `stream`; one wait at the end unless the caller asked for none
    for (int b = 0; b < nb; b++)
      GDV_RETURN_NOT_OK(Evaluate(batches[b].num_rows, batches[b].cols, batches[b].num_cols, nullptr, batches[b].outs,
                                 batches[b].num_outs, MemKind::kDevice, stream, kEvalAsync));
    if (!(flags & kEvalAsync)) GDV_HIP_RETURN_NOT_OK(hipStreamSynchronize(stream));
    return Status::OK();
  }
  PinnedLease lease(rt);
  GDV_RETURN_NOT_OK(lease.Acquire(stride * static_cast<size_t>(nb)));
  char* const pin = lease.get();
  DeviceBuffer table, err;
  StreamDrain drain{stream, false};  // declared after the pooled blocks: an error return waits for what was enqueued
  GDV_RETURN_NOT_OK(table.Allocate(stride * nb));
  if (plan_.can_raise) GDV_RETURN_NOT_OK(err.Allocate(8));
  Staging st;  // (device buffers bind in place: nothing is staged)
  int64_t grid = 1;
  // every batch is validated and its argument block written (host memory only) BEFORE anything is
  // enqueued: an Invalid return frees `table` / `err` with nothing pending on them
  for (int b = 0; b < nb; b++) {
    const BatchView& v = batches[b];
    if (v.num_rows <= 0) return Status::Invalid("RecordBatch must be non-empty.");
    if (v.outs == nullptr || v.num_outs != num_outputs())
      return Status::Invalid("batch " + std::to_string(b) + ": number of output buffers does not match the number of expressions");
    ArgBlock args(plan_.layout);
    GDV_RETURN_NOT_OK(BindInputs(plan_, plan_schema_, v.cols, v.num_cols, v.num_rows, MemKind::kDevice, stream, &args, &st));
    if (!st.buffers.empty()) return Status::Invalid("internal: staged input in a multi-batch evaluation");
    BindLiterals(plan_, dev->consts, &args);
    args.Set64(ArgLayout::kOffN, static_cast<uint64_t>(v.num_rows));
    if (plan_.can_raise) args.SetPtr(ArgLayout::kOffErr, err.get());
    for (int e = 0; e < v.num_outs; e++) {
      const DataType& t = plan_.output_types[e];
      if (v.outs[e].validity == nullptr || v.outs[e].data == nullptr || v.outs[e].validity_size < ValidityBytes(v.num_rows) ||
          v.outs[e].data_size < DataBytes(t, v.num_rows))
        return Status::Invalid("batch " + std::to_string(b) + ", output buffer " + std::to_string(e) + " too small");
      args.SetOutData(e, v.outs[e].data);
      args.SetOutValid(e, v.outs[e].validity);
    }
    std::memcpy(pin + stride * b, args.data(), stride);
    grid = std::max(grid, GridFor(plan_, v.num_rows));
  }
  EvalTrace trace("project-many", plan_.kernel_name, nb, stream);
  drain.armed = true;
  if (plan_.can_raise) GDV_HIP_RETURN_NOT_OK(hipMemsetAsync(err.get(), 0, 8, stream));
  GDV_HIP_RETURN_NOT_OK(hipMemcpyAsync(table.get(), pin, stride * nb, hipMemcpyHostToDevice, stream));
  GDV_RETURN_NOT_OK(rt.LaunchMany(*dev->kernel.load(), grid, nb, plan_.opts.waves * 64, table.get(), stream));
  uint32_t err_bits = 0;
  if (plan_.can_raise)
    GDV_HIP_RETURN_NOT_OK(hipMemcpyAsync(&err_bits, err.get(), 4, hipMemcpyDeviceToHost, stream));
  if ((flags & kEvalAsync) && !plan_.can_raise) {
    // the table and the pinned block go back once the stream has passed this point
    table.release_after(stream);
    lease.ReleaseAfter(stream);
    drain.armed = false;
    return Status::OK();
  }
  GDV_HIP_RETURN_NOT_OK(hipStreamSynchronize(stream));
  drain.armed = false;
  if (err_bits != 0) return Status::ExecutionError(RaiseMessage(plan_, err_bits));
  return Status::OK();
}

// ------------------------------------------------------------------ var-len plans, asynchronously

Status Projector::EvaluateAsync(int64_t num_rows, const ColumnBuffers* cols, int num_cols, const SelectionView* sel,
                                OutputBuffers* outs, int num_outs, hipStream_t stream, void* result) const {
  if (pre_ != nullptr) return EvaluateAsyncTwoStage(num_rows, cols, num_cols, sel, outs, num_outs, stream, result);
  return EvaluateAsyncStage(num_rows, cols, num_cols, sel, outs, num_outs, stream, result, nullptr);
}

// The stages of a staged plan on the stream, a gate kernel between each two (gdv_kernels.h: StageGate).
Status Projector::EvaluateAsyncTwoStage(int64_t num_rows, const ColumnBuffers* cols, int num_cols, const SelectionView* sel,
                                        OutputBuffers* outs, int num_outs, hipStream_t stream, void* result) const {
  if (num_rows <= 0) return Status::Invalid("RecordBatch must be non-empty.");
  if (outs == nullptr || result == nullptr) return Status::Invalid("Output array vector and result block cannot be null");
  if (num_outs != num_outputs()) return Status::Invalid("number of output buffers does not match the number of expressions");
  if (num_cols != static_cast<int>(schema_.size()))
    return Status::Invalid("number of columns in batch (" + std::to_string(num_cols) +
                           ") does not match the schema (" + std::to_string(schema_.size()) + ")");
  const int np = pre_->num_outputs();
  if (np > kMaxStageOutputs) return Status::Invalid("too many temporaries for an asynchronous two-stage evaluation");
  const bool has_sel = sel != nullptr && sel->mode != SelectionMode::kNone;
  const int64_t stage_rows = has_sel ? sel->num_slots : num_rows;   // (with a device-resident count: the capacity)
  if (stage_rows <= 0) return EvaluateAsyncStage(num_rows, cols, num_cols, sel, outs, num_outs, stream, result, nullptr);
  Runtime& rt = Runtime::Get();
  GDV_RETURN_NOT_OK(rt.EnsureDevice());
  // temporaries: validity | offsets | bytes per first-stage output, sized as StageColumns::Run sizes them
  const int64_t guess = StageGuess(cols, num_cols, stage_rows);
  StageCaps caps{};
  std::vector<DeviceBuffer> blocks(3 * static_cast<size_t>(np) + 1);
  std::vector<OutputBuffers> po(np);
  std::vector<ColumnBuffers> all(cols, cols + num_cols);
  StreamDrain drain{stream, false};  // declared after the blocks: an error return after the first enqueue waits
  const int64_t vbytes = ValidityBytes(stage_rows);
  for (int e = 0; e < np; e++) {
    if (!pre_->output_type(e).is_varlen()) return Status::Invalid("two-stage plan: first stage must produce utf8 / binary");
    const int64_t per_row_x16 = e < static_cast<int>(stage_hints_.size()) ? stage_hints_[e].load(std::memory_order_relaxed) : 0;
    const int64_t cap = std::max<int64_t>(StageCapacity(guess, per_row_x16, stage_rows), 8);
    GDV_RETURN_NOT_OK(blocks[3 * e].Allocate(static_cast<size_t>(std::max<int64_t>(vbytes, 8))));
    GDV_RETURN_NOT_OK(blocks[3 * e + 1].Allocate(static_cast<size_t>((stage_rows + 1) * 4)));
    GDV_RETURN_NOT_OK(blocks[3 * e + 2].Allocate(static_cast<size_t>(cap) + 16));  // (+16: zeroed by the gate)
    po[e].validity = blocks[3 * e].get();
    po[e].validity_size = std::max<int64_t>(vbytes, 8);
    po[e].offsets = blocks[3 * e + 1].get();
    po[e].offsets_size = (stage_rows + 1) * 4;
    po[e].data = blocks[3 * e + 2].get();
    po[e].data_size = cap;
    caps.cap[e] = cap;
    caps.data[e] = po[e].data;
    all.push_back(AsColumn(po[e], cap + 16));
  }
  // gate block: first stage's result (1 + np words) | rows word | status word
  DeviceBuffer& gate = blocks[3 * static_cast<size_t>(np)];
  GDV_RETURN_NOT_OK(gate.Allocate(256));
  uint64_t* const stage_result = gate.as<uint64_t>();
  int64_t* const rows_word = reinterpret_cast<int64_t*>(gate.as<char>() + 128);
  uint64_t* const status_word = reinterpret_cast<uint64_t*>(gate.as<char>() + 136);
  drain.armed = true;
  // (a first stage that is itself staged — upper(reverse(replace(..))) — goes through this function again: its result block,
  // status and byte totals, is what the gate reads either way; round 5: three and more stages were synchronous only)
  if (pre_->pre_ != nullptr)
    GDV_RETURN_NOT_OK(pre_->EvaluateAsyncTwoStage(num_rows, cols, num_cols, sel, po.data(), np, stream, stage_result));
  else
    GDV_RETURN_NOT_OK(pre_->EvaluateAsyncStage(num_rows, cols, num_cols, sel, po.data(), np, stream, stage_result, nullptr));
  GDV_HIP_RETURN_NOT_OK(LaunchStageGate(stage_result, np, caps, has_sel ? static_cast<const int64_t*>(sel->num_slots_device) : nullptr,
                                        stage_rows, rows_word, status_word, stream));
  if (plan_.num_varlen_outputs > 0) {
    GDV_RETURN_NOT_OK(EvaluateAsyncStage(num_rows, all.data(), static_cast<int>(all.size()), sel, outs, num_outs, stream, result,
                                         rows_word));
  } else {  // fixed-width outputs only: the ordinary asynchronous launch over the staged columns, rows from the gate
    // (a second stage that can raise — divide, castINT of the staged text ... — raises into result[0] itself: round 4
    // sent such plans to the synchronous call)
    GDV_HIP_RETURN_NOT_OK(hipMemsetAsync(result, 0, 8 * (1 + static_cast<size_t>(num_outs)), stream));
    GDV_RETURN_NOT_OK(Evaluate(num_rows, all.data(), static_cast<int>(all.size()), sel, outs, num_outs, MemKind::kDevice, stream,
                               kEvalAsync | kEvalStaged, rows_word, plan_.can_raise ? result : nullptr));
  }
  GDV_HIP_RETURN_NOT_OK(LaunchOrStatus(static_cast<uint64_t*>(result), status_word, stream));
  for (auto& b : blocks) b.release_after(stream);
  drain.armed = false;
  return Status::OK();
}

Status Projector::EvaluateAsyncStage(int64_t num_rows, const ColumnBuffers* cols, int num_cols, const SelectionView* sel,
                                     OutputBuffers* outs, int num_outs, hipStream_t stream, void* result,
                                     const void* rows_word) const {
  if (num_rows <= 0) return Status::Invalid("RecordBatch must be non-empty.");
  if (outs == nullptr || result == nullptr) return Status::Invalid("Output array vector and result block cannot be null");
  if (num_outs != num_outputs()) return Status::Invalid("number of output buffers does not match the number of expressions");
  const bool has_sel = sel != nullptr && sel->mode != SelectionMode::kNone;
  if (has_sel != (plan_.mode != SelectionMode::kNone) || (has_sel && sel->mode != plan_.mode))
    return Status::Invalid("selection vector type does not match the mode the projector was built for");
  const int64_t out_rows = has_sel ? sel->num_slots : num_rows;   // (with a device-resident count: the capacity)
  if (has_sel && (sel->num_slots < 0 || (out_rows > 0 && sel->indices == nullptr)))
    return Status::Invalid("selection vector: invalid slot count or no buffer");
  const int nv = plan_.num_varlen_outputs;
  uint64_t* const res = static_cast<uint64_t*>(result);
  if (nv == 0) {  // fixed-width plans: the ordinary asynchronous launch; no byte totals; a plan that can raise raises into result[0]
    GDV_HIP_RETURN_NOT_OK(hipMemsetAsync(result, 0, 8 * (1 + static_cast<size_t>(num_outs)), stream));
    return Evaluate(num_rows, cols, num_cols, sel, outs, num_outs, MemKind::kDevice, stream, kEvalAsync, nullptr,
                    plan_.can_raise ? result : nullptr);
  }
  if (out_rows == 0) {
    GDV_HIP_RETURN_NOT_OK(hipMemsetAsync(result, 0, 8 * (1 + static_cast<size_t>(num_outs)), stream));
    for (int e = 0; e < num_outs; e++)
      if (plan_.output_types[e].is_varlen() && outs[e].offsets != nullptr)
        GDV_HIP_RETURN_NOT_OK(hipMemsetAsync(outs[e].offsets, 0, 4, stream));
    return Status::OK();
  }
  Runtime& rt = Runtime::Get();
  GDV_RETURN_NOT_OK(rt.EnsureDevice());
  const PlanDeviceState* dev = nullptr;
  GDV_RETURN_NOT_OK(states_.Get(plan_, &dev));

  ArgBlock args(plan_.layout);
  Staging st;
  VarlenLaunch vlaunch(plan_, dev, rt, out_rows, stream);
  StreamDrain drain{stream, false};  // declared last: an error return after the first enqueue waits before the blocks go back
  GDV_RETURN_NOT_OK(BindInputs(plan_, plan_schema_, cols, num_cols, num_rows, MemKind::kDevice, stream, &args, &st,
                               has_sel ? out_rows : -1));
  BindLiterals(plan_, dev->consts, &args);
  drain.armed = !st.buffers.empty();   // (a tiny var-len buffer was copied into a padded pool block)
  args.Set64(ArgLayout::kOffN, static_cast<uint64_t>(out_rows));
  if (has_sel) {
    args.SetPtr(ArgLayout::kOffSel, sel->indices);
    args.SetPtr(ArgLayout::kOffAux2, sel->num_slots_device);  // null: the count is kOffN
  }
  if (rows_word != nullptr) args.SetPtr(ArgLayout::kOffAux2, rows_word);  // second stage: the gate's word (it folds the slot count in)
  const std::vector<int>& vl = vlaunch.vl;
  for (int e = 0; e < num_outs; e++) {
    const DataType& t = plan_.output_types[e];
    const int64_t need_valid = ValidityBytes(out_rows), need_data = t.is_varlen() ? 0 : DataBytes(t, out_rows);
    if (outs[e].validity == nullptr || outs[e].validity_size < need_valid || outs[e].data_size < need_data ||
        (outs[e].data == nullptr && (need_data > 0 || outs[e].data_size > 0)))
      return Status::Invalid("output buffer " + std::to_string(e) + " too small");
    if (t.is_varlen() && (outs[e].offsets == nullptr || outs[e].offsets_size < (out_rows + 1) * 4))
      return Status::Invalid("output buffer " + std::to_string(e) + ": offsets buffer too small");
    args.SetOutData(e, outs[e].data);
    args.SetOutValid(e, outs[e].validity);
    args.SetOutOffsets(e, outs[e].offsets);
    if (t.is_varlen()) args.SetOutCap(e, outs[e].data_size);
  }
  GDV_RETURN_NOT_OK(st.FlushIn(stream));
  GDV_HIP_RETURN_NOT_OK(hipMemsetAsync(result, 0, 8 * (1 + static_cast<size_t>(num_outs)), stream));
  drain.armed = true;

  // The path this Projector is currently on; an asynchronous call cannot read the error word, so it neither re-runs
  // the batch nor moves the Projector (the synchronous call does both).
  const bool has_optimistic = plan_.wave_tiles || plan_.has_flat_output;
  const int path = VarlenStartPath(path_hint_.load(std::memory_order_relaxed), has_optimistic,
                                   plan_.wave_tiles && plan_.exact != nullptr, EngineKnobs::Get().no_optflat, 0);
  EvalTrace trace("project-async", plan_.kernel_name, out_rows, stream);
  if (path != 2 && plan_.wave_tiles) {
    // ---- wave shape: pre-pass -> offsets scan -> main kernel (the optimistic pair or its exact variant)
    // a second stage whose gate is closed walks 0 rows, and so do the wave tiles past a slot count that sits in
    // device memory: their pre-pass writes no count
    const bool zero_counts = rows_word != nullptr || (has_sel && sel->num_slots_device != nullptr);
    GDV_RETURN_NOT_OK(vlaunch.EnqueueWave(&args, /*exact=*/path == 1, zero_counts));
    // the error word, minus the exact kernels' note that the batch did hold bytes >= 0x80 (64: not an error —
    // round 4 published it, and every asynchronous call on non-ASCII text looked failed to its caller)
    GDV_HIP_RETURN_NOT_OK(LaunchPublishStatus(res, reinterpret_cast<const uint32_t*>(vlaunch.wave_head()), kSawUtf8, stream));
    for (int v = 0; v < nv; v++)
      GDV_HIP_RETURN_NOT_OK(hipMemcpyAsync(res + 1 + vl[v], vlaunch.wave_total(v), 8, hipMemcpyDefault, stream));
  } else {
    // ---- scanner shape: one launch (selection-mode plans; plans without a wave shape; path 2: the general kernel)
    const CompiledKernel* active = dev->kernel.load();
    if (has_optimistic && path == 2) {
      GDV_RETURN_NOT_OK(vlaunch.EnsureGeneral());
      active = dev->kernel_general.load();
    }
    GDV_RETURN_NOT_OK(vlaunch.EnqueueScanner(&args, *active, vlaunch.scanner_grid()));
    GDV_HIP_RETURN_NOT_OK(hipMemcpyAsync(res, vlaunch.scanner_state(), 4, hipMemcpyDefault, stream));
    for (int v = 0; v < nv; v++)
      GDV_HIP_RETURN_NOT_OK(hipMemcpyAsync(res + 1 + vl[v], vlaunch.scanner_total(v), 8, hipMemcpyDefault, stream));
  }
  // scratch goes back to the pool when the stream has passed this point
  vlaunch.ReleaseAfter(stream);
  for (auto& b : st.buffers) b.release_after(stream);
  drain.armed = false;
  return Status::OK();
}

}  // namespace gdv
