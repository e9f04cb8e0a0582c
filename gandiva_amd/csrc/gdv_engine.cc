#include "gdv_engine_internal.h"

namespace gdv {

namespace engine {

std::string SchemaKey(const Schema& s) {
  std::string k;
  for (auto& f : s) k += std::to_string(f.name.size()) + ":" + f.name + ":" + f.type.ToString() + ";";
  return k;
}

// Folds buffer misalignment and the Arrow array offset into (8-byte aligned word pointer,
// shift < 64, readable words).  The buffer must be readable up to the next 8-byte boundary
// (Arrow pads buffers to 64 bytes: pyarrow/include/arrow/type_fwd.h:759).
HostBitmap FoldBitmap(const void* ptr, int64_t size, int64_t bit_offset) {
  HostBitmap b;
  if (ptr == nullptr) return b;
  uintptr_t a = reinterpret_cast<uintptr_t>(ptr);
  uintptr_t aligned = a & ~uintptr_t(7);
  int64_t lead = static_cast<int64_t>(a & 7) * 8 + bit_offset;
  uintptr_t p = aligned + static_cast<uintptr_t>(lead >> 6) * 8;
  b.p = reinterpret_cast<const uint64_t*>(p);
  b.shift = static_cast<int32_t>(lead & 63);
  int64_t bytes = static_cast<int64_t>(a + size - p);
  b.nwords = bytes > 0 ? (bytes + 7) / 8 : 0;
  return b;
}

// host bitmap bytes covering bits [off, off+rows) -> zero-padded device words
Status StageBitmap(const void* host, int64_t off, int64_t rows, hipStream_t stream,
                   Staging* st, HostBitmap* out) {
  const int64_t first = off / 8;
  const int64_t len = BytesForBits(off + rows) - first;
  const int64_t words = (len + 7) / 8 + 1;
  void* dev = nullptr;
  GDV_RETURN_NOT_OK(st->In(static_cast<const char*>(host) + first, len, words * 8, stream, &dev));
  out->p = static_cast<const uint64_t*>(dev);
  out->shift = static_cast<int32_t>(off % 8);
  out->nwords = words;
  return Status::OK();
}

Status BindInputs(const KernelPlan& plan, const Schema& schema, const ColumnBuffers* cols,
                  int num_cols, int64_t batch_rows, MemKind mem, hipStream_t stream,
                  ArgBlock* args, Staging* st, int64_t compact_rows) {
  if (num_cols != static_cast<int>(schema.size()))
    return Status::Invalid("number of columns in batch (" + std::to_string(num_cols) +
                           ") does not match the schema (" + std::to_string(schema.size()) + ")");
  for (size_t k = 0; k < plan.input_fields.size(); k++) {
    const int idx = plan.input_fields[k];
    // (temporaries of a selection-mode first stage hold one row per slot, not per batch row)
    const int64_t num_rows = (idx >= plan.compact_from && compact_rows >= 0) ? compact_rows : batch_rows;
    const ColumnBuffers& c = cols[idx];
    const DataType& t = schema[idx].type;
    const std::string& name = schema[idx].name;
    if (plan.input_needs_values[k]) {
      if (c.data == nullptr && num_rows > 0 && !t.is_varlen())
        return Status::Invalid("column '" + name + "' has no data buffer");
      if (t.is_varlen()) {
        // int32 offsets (rows + 1 of them, from the array offset) + the whole byte buffer
        const int64_t need = (c.offset + num_rows + 1) * 4;
        if (c.offsets == nullptr || c.offsets_size < need)
          return Status::Invalid("column '" + name + "': offsets buffer too small");
        const char* osrc = static_cast<const char*>(c.offsets) + c.offset * 4;
        if (mem == MemKind::kHost) {
          // Round 5: offsets and bytes that lie in REGISTERED host memory (gdv_host_register / gdv_host_alloc) are
          // read in place over the fabric, like fixed-width columns since round 4.  The bytes need their 16-byte
          // granule behind the last byte inside the registered range as well (the sweep reads whole pieces: Arrow's
          // zeroed 64-byte padding covers it; a buffer that ends flush with its range is staged as before).
          void* dof = (reinterpret_cast<uintptr_t>(osrc) & 3) == 0 ? HostRegistry::Get().View(osrc, (num_rows + 1) * 4) : nullptr;
          void* dd = c.data_size >= 8 ? HostRegistry::Get().View(c.data, c.data_size + 16) : nullptr;
          if (dd != nullptr) {
            // (round 6: the sweep reads the last piece up to its 16-byte boundary; the staged copy zeroes what lies behind
            // the last byte, a caller's own registered buffer need not — a stale byte >= 0x80 there would send an ASCII
            // batch to the exact string kernels for nothing.  Host memory: look, and stage when the tail is not clean.)
            const unsigned char* end = static_cast<const unsigned char*>(c.data) + c.data_size;
            const unsigned char* stop = reinterpret_cast<const unsigned char*>((reinterpret_cast<uintptr_t>(end) + 15) & ~uintptr_t{15});
            for (const unsigned char* q = end; q < stop; q++)
              if (*q & 0x80) { dd = nullptr; break; }
          }
          if (dof == nullptr) GDV_RETURN_NOT_OK(st->In(osrc, (num_rows + 1) * 4, (num_rows + 1) * 4, stream, &dof));
          // (16 zero bytes behind the last byte: the byte sweep reads whole 16-byte pieces, and whatever
          // the block held before must not look like a byte >= 0x80 — it would send an ASCII batch to
          // the exact variant of the string kernels for nothing)
          if (dd == nullptr) GDV_RETURN_NOT_OK(st->In(c.data, c.data_size, c.data_size + 16, stream, &dd));
          args->SetInOffsets(static_cast<int>(k), dof);
          args->SetInData(static_cast<int>(k), dd);
        } else if (c.data_size < 8) {
          // the kernels' 8-byte loads need 8 readable bytes ending at the limit: a tiny
          // buffer is copied into a zero-padded one
          DeviceBuffer& dd = st->Add();
          GDV_RETURN_NOT_OK(dd.Allocate(8));
          GDV_HIP_RETURN_NOT_OK(hipMemsetAsync(dd.get(), 0, 8, stream));
          if (c.data_size > 0)
            GDV_HIP_RETURN_NOT_OK(hipMemcpyAsync(dd.get(), c.data, c.data_size,
                                                 hipMemcpyDeviceToDevice, stream));
          args->SetInOffsets(static_cast<int>(k), osrc);
          args->SetInData(static_cast<int>(k), dd.get());
        } else {
          args->SetInOffsets(static_cast<int>(k), osrc);
          args->SetInData(static_cast<int>(k), c.data);
        }
        // readable extent of the byte buffer (the kernels' 8-byte loads stop at this limit)
        HostBitmap extent;
        extent.nwords = std::max<int64_t>(c.data_size, 8);
        args->SetInBits(static_cast<int>(k), extent);
      } else if (t.id == kBool) {
        if (c.data_size < BytesForBits(c.offset + num_rows))
          return Status::Invalid("column '" + name + "': data buffer too small");
        HostBitmap b;
        if (mem == MemKind::kHost) {
          // (a buffer inside a registered host range is read in place: gdv_host_register)
          if (const void* v = HostRegistry::Get().View(c.data, c.data_size)) b = FoldBitmap(v, c.data_size, c.offset);
          else GDV_RETURN_NOT_OK(StageBitmap(c.data, c.offset, num_rows, stream, st, &b));
        } else {
          b = FoldBitmap(c.data, c.data_size, c.offset);
        }
        args->SetInBits(static_cast<int>(k), b);
      } else {
        const int w = t.byte_width();
        if (c.data_size < (c.offset + num_rows) * w)
          return Status::Invalid("column '" + name + "': data buffer too small (" +
                                 std::to_string(c.data_size) + " bytes for " +
                                 std::to_string(c.offset + num_rows) + " rows)");
        const char* src = static_cast<const char*>(c.data) + c.offset * w;
        if (mem == MemKind::kHost) {
          void* d = HostRegistry::Get().View(src, num_rows * w);
          if (d == nullptr) GDV_RETURN_NOT_OK(st->In(src, num_rows * w, num_rows * w, stream, &d));
          args->SetInData(static_cast<int>(k), d);
        } else {
          args->SetInData(static_cast<int>(k), src);
        }
      }
    }
    if (plan.input_needs_validity[k]) {
      HostBitmap b;
      if (c.validity == nullptr) {
        // no validity buffer = no nulls: bind the one-word all-ones bitmap (index clamped)
        GDV_RETURN_NOT_OK(Runtime::Get().AllOnesWord(&b.p));
        b.shift = 0;
        b.nwords = 1;
      } else {
        if (c.validity_size < BytesForBits(c.offset + num_rows))
          return Status::Invalid("column '" + name + "': validity buffer too small");
        if (mem == MemKind::kHost) {
          if (const void* v = HostRegistry::Get().View(c.validity, c.validity_size)) b = FoldBitmap(v, c.validity_size, c.offset);
          else GDV_RETURN_NOT_OK(StageBitmap(c.validity, c.offset, num_rows, stream, st, &b));
        } else {
          b = FoldBitmap(c.validity, c.validity_size, c.offset);
        }
      }
      args->SetInValid(static_cast<int>(k), b);
    }
  }
  return Status::OK();
}

int64_t GridFor(const KernelPlan& plan, int64_t rows) {
  if (plan.wave_tiles) {
    // wave shape: one WAVE per tile, no scanner workgroup
    const int64_t nwt = (rows + plan.rows_per_tile() - 1) / plan.rows_per_tile();
    return std::max<int64_t>(1, (nwt + plan.opts.waves - 1) / plan.opts.waves);
  }
  if (plan.string_skeleton) {
    // one workgroup per tile (+ the scanner workgroup when there are var-len outputs)
    const int64_t ntiles = (rows + plan.rows_per_tile() - 1) / plan.rows_per_tile();
    return std::max<int64_t>(1, ntiles) + (plan.num_varlen_outputs > 0 ? 1 : 0);
  }
  const int64_t nwords = (rows + 63) / 64;
  const int64_t per_tile = static_cast<int64_t>(plan.opts.subtiles) * plan.opts.waves;
  int64_t ntiles = (nwords + per_tile - 1) / per_tile;
  int blocks_per_cu = std::max(1, 32 / plan.opts.waves);
  // String work per tile varies with the data (lengths, divergent per-row loops): four times
  // as many, smaller shares of the grid-stride loop even out the tail (C5: 2.26 -> 2.01 ms;
  // fixed-width plans measured best at the base value)
  if (plan.has_varlen_input || plan.has_varlen_output) blocks_per_cu *= 4;
  // (read-dominated 16-sub-tile plans, PlanProjectorShape / PlanFilter: fewer resident workgroups stream better — once every
  // workgroup has a long loop to run; a batch of a few tiles per CU is over sooner with all of them in flight)
  else if (plan.grid_blocks_per_cu > 0 && ntiles >= 64LL * Runtime::Get().num_cus()) blocks_per_cu = plan.grid_blocks_per_cu;
  if (EngineKnobs::Get().grid_mult > 0) blocks_per_cu = EngineKnobs::Get().grid_mult;
  int64_t cap = static_cast<int64_t>(Runtime::Get().num_cus()) * blocks_per_cu;
  return std::max<int64_t>(1, std::min(ntiles, cap));
}

std::string ErrorMessage(uint32_t bits) {
  std::string m;
  if (bits & 1u) m += "divide by zero error";
  if (bits & 2u) m += (m.empty() ? "" : "; ") + std::string("overflow");
  if (bits & 4u) m += (m.empty() ? "" : "; ") + std::string("invalid argument");
  if (bits & 8u) m += (m.empty() ? "" : "; ") + std::string("device scan stalled");
  if (bits & 48u) m += (m.empty() ? "" : "; ") + std::string("internal: optimistic var-len kernel was not re-run");
  if (bits & 128u) m += (m.empty() ? "" : "; ") + std::string("asynchronous two-stage evaluation: a temporary was too small");
  return m.empty() ? "execution error" : m;
}

// String literals, LIKE patterns and IN tables of a plan live in one small device block that the
// kernel reaches through gdv_args::aux0 (uploaded once, at Make).
Status UploadConstBlock(const KernelPlan& plan, DeviceBuffer* out) {
  if (plan.const_block.empty()) return Status::OK();
  GDV_RETURN_NOT_OK(out->Allocate(plan.const_block.size() + 16));
  GDV_HIP_RETURN_NOT_OK(hipMemcpy(out->get(), plan.const_block.data(), plan.const_block.size(), hipMemcpyHostToDevice));
  return Status::OK();
}

void BindLiterals(const KernelPlan& plan, const DeviceBuffer& consts, ArgBlock* args) {
  for (size_t i = 0; i < plan.literals.size(); i++) args->SetLit(static_cast<int>(i), plan.literals[i]);
  args->SetPtr(ArgLayout::kOffAux0, consts.get());
}

void ArmTier0(const Schema& schema, const std::vector<ExpressionPtr>& exprs, bool is_filter, const KernelPlan& plan,
              std::unique_ptr<tier0::Args>* tier0, std::atomic<bool>* pending) {
  if (EngineKnobs::Get().no_tier0) return;
  std::unique_ptr<tier0::Args> prog(new tier0::Args);
  if (BuildTier0Program(schema, exprs, is_filter, plan, prog.get(), nullptr)) {
    const int state = EngineKnobs::Get().force_tier0 ? 0 : Runtime::Get().CodeObjectState(plan.kernel_name);
    if (state == 0 || EngineKnobs::Get().force_tier0) {
      if (EngineKnobs::Get().force_tier0 || Runtime::Get().CompileInBackground(plan.source, plan.kernel_name)) {
        *tier0 = std::move(prog);
        pending->store(true);
      }  // (else: the background compiler was shut down — Make waits for the compilation, as before round 6)
    }
  }
}

Status RunTier0(const tier0::Args& prog, const ArgBlock& args, int64_t rows, Runtime& rt, hipStream_t stream) {
  tier0::Args t0 = prog;
  std::memcpy(t0.block, args.data(), args.size());
  GDV_HIP_RETURN_NOT_OK(LaunchTier0(t0, rows, rt.num_cus(), stream));
  CountTier0Launch();
  return Status::OK();
}

}  // namespace engine

using namespace engine;

Status PlanDeviceStates::Get(const KernelPlan& plan, const PlanDeviceState** out, bool need_kernel) const {
  Runtime& rt = Runtime::Get();
  const int id = rt.id();
  PlanDeviceState* have = slots_[id].load(std::memory_order_acquire);
  if (have != nullptr && (!need_kernel || have->kernel.load(std::memory_order_acquire) != nullptr)) {
    *out = have;
    return Status::OK();
  }
  std::lock_guard<std::mutex> g(mu_);
  have = slots_[id].load(std::memory_order_acquire);
  if (have == nullptr) {
    std::unique_ptr<PlanDeviceState> st(new PlanDeviceState);
    GDV_RETURN_NOT_OK(UploadConstBlock(plan, &st->consts));
    if (plan.prepass) GDV_RETURN_NOT_OK(UploadConstBlock(*plan.prepass, &st->consts_pre));
    have = st.release();
    slots_[id].store(have, std::memory_order_release);
  }
  if (need_kernel && have->kernel.load(std::memory_order_acquire) == nullptr) {
    if (plan.prepass) GDV_RETURN_NOT_OK(rt.GetKernel(plan.prepass->source, plan.prepass->kernel_name, &have->kernel_pre));
    const CompiledKernel* k = nullptr;
    GDV_RETURN_NOT_OK(rt.GetKernel(plan.source, plan.kernel_name, &k));
    have->kernel.store(k, std::memory_order_release);
  }
  *out = have;
  return Status::OK();
}

// ------------------------------------------------------------------ two-stage plans

Status StageColumns::Run(const Projector& pre, int64_t batch_rows, const ColumnBuffers* in, int num_cols,
                         MemKind mem, hipStream_t stream, const SelectionView* sel,
                         std::vector<std::atomic<int64_t>>* hints) {
  const int np = pre.num_outputs();
  // under a selection vector the first stage evaluates the SELECTED rows only (it may raise only
  // where the caller's projector may) and its temporaries hold one row per slot
  const int64_t num_rows = sel != nullptr ? sel->num_slots : batch_rows;
  cols.assign(in, in + num_cols);
  auto alloc = [&](int64_t bytes, void** p) -> Status {
    bytes = std::max<int64_t>(bytes, 8);
    if (mem == MemKind::kHost) {
      host.emplace_back(new std::vector<uint8_t>(static_cast<size_t>(bytes)));
      *p = host.back()->data();
      return Status::OK();
    }
    dev.emplace_back(new DeviceBuffer());
    GDV_RETURN_NOT_OK(dev.back()->Allocate(static_cast<size_t>(bytes)));
    *p = dev.back()->get();
    return Status::OK();
  };
  // first guess for the byte buffers: as many bytes as the var-len inputs hold plus 32 per row
  // (device memory; the host path starts from nothing, it sizes its buffers by a length pass
  // anyway).  The evaluation reports what it needs, so a short buffer costs one retry.
  const int64_t guess = mem == MemKind::kDevice ? StageGuess(in, num_cols, num_rows) : 0;
  std::vector<OutputBuffers> po(np);
  std::vector<int64_t> cap(np, guess);
  // (round-2 advisor: the blanket guess grabbed gigabytes of HBM scratch per call however small the
  // temporaries were) — what the previous batch of this plan produced, per row, + 25 % is a far
  // better first guess; a short buffer still costs one retry
  if (hints != nullptr && mem == MemKind::kDevice)
    for (int e = 0; e < np && e < static_cast<int>(hints->size()); e++)
      cap[e] = StageCapacity(guess, (*hints)[e].load(std::memory_order_relaxed), num_rows);
  const int64_t vbytes = mem == MemKind::kHost ? BytesForBits(num_rows) : Projector::ValidityBytes(num_rows);
  for (int e = 0; e < np; e++) {
    if (!pre.output_type(e).is_varlen()) return Status::Invalid("two-stage plan: first stage must produce utf8 / binary");
    GDV_RETURN_NOT_OK(alloc(vbytes, &po[e].validity));
    po[e].validity_size = std::max<int64_t>(vbytes, 8);
    GDV_RETURN_NOT_OK(alloc((num_rows + 1) * 4, &po[e].offsets));
    po[e].offsets_size = (num_rows + 1) * 4;
    GDV_RETURN_NOT_OK(alloc(cap[e] + 16, &po[e].data));  // (+16: zeroed behind the bytes produced, below)
    po[e].data_size = cap[e];
  }
  Status s = pre.Evaluate(batch_rows, in, num_cols, sel, po.data(), np, mem, stream, 0);
  if (!s.ok()) {
    bool grew = false;
    for (int e = 0; e < np; e++) {
      if (po[e].data_size > cap[e]) {
        cap[e] = po[e].data_size;
        GDV_RETURN_NOT_OK(alloc(cap[e] + 16, &po[e].data));
        grew = true;
      }
      po[e].data_size = cap[e];
    }
    if (!grew) return s;
    GDV_RETURN_NOT_OK(pre.Evaluate(batch_rows, in, num_cols, sel, po.data(), np, mem, stream, 0));
  }
  if (hints != nullptr)
    for (int e = 0; e < np && e < static_cast<int>(hints->size()); e++)
      (*hints)[e].store(std::max<int64_t>(1, po[e].data_size * 16 / std::max<int64_t>(num_rows, 1) + 1),
                        std::memory_order_relaxed);
  for (int e = 0; e < np; e++) {
    ColumnBuffers c = AsColumn(po[e], po[e].data_size);
    // The second stage's byte sweep reads whole 16-byte pieces: the 16 bytes behind the text are zeroed and
    // readable, so that pool garbage is never taken for bytes >= 0x80 (round 4: every synchronous two-stage
    // batch went optimistic kernel -> NOTASCII -> exact variant because of it).
    if (mem == MemKind::kDevice) {
      GDV_HIP_RETURN_NOT_OK(hipMemsetAsync(static_cast<char*>(po[e].data) + po[e].data_size, 0, 16, stream));
      c.data_size = po[e].data_size + 16;
    }
    cols.push_back(c);
  }
  return Status::OK();
}

// Tier 0 is on while the plan has a program and its specialised code object has not arrived (or always, under
// GDV_FORCE_TIER0).  A background compilation that failed turns it off: the blocking path then reports the error.
static bool Tier0Active(const tier0::Args* prog, std::atomic<bool>* pending, const std::string& kernel_name) {
  if (prog == nullptr) return false;
  if (EngineKnobs::Get().force_tier0) return true;
  if (!pending->load(std::memory_order_relaxed)) return false;
  if (Runtime::Get().CodeObjectState(kernel_name, /*memory_only=*/true) != 0) {
    pending->store(false, std::memory_order_relaxed);
    return false;
  }
  return true;
}
bool Projector::UseTier0() const { return Tier0Active(tier0_.get(), &tier0_pending_, plan_.kernel_name); }
bool Filter::UseTier0() const { return Tier0Active(tier0_.get(), &tier0_pending_, plan_.kernel_name); }

// ------------------------------------------------------------------ tier 0: the program of a plan as text (no device)

Status Tier0Describe(const Schema& schema, const std::vector<ExpressionPtr>& exprs, bool is_condition, std::string* text,
                     SelectionMode mode) {
  KernelPlan plan;
  StagedExpressions staged;
  StageMaterialisedValues(schema, exprs, &staged, CodegenOptions::FromEnv());
  if (!staged.pre.empty()) return Status::NotImplemented("no tier 0: the plan materialises values in a first stage");
  if (is_condition) {
    if (exprs.size() != 1) return Status::Invalid("one condition expected");
    if (mode != SelectionMode::kNone) return Status::Invalid("a filter has no selection mode");
    GDV_RETURN_NOT_OK(PlanFilter(schema, exprs[0], CodegenOptions::FromEnv(), &plan));
  } else {
    GDV_RETURN_NOT_OK(PlanProjector(schema, exprs, mode, CodegenOptions::FromEnv(), &plan,
                                    mode == SelectionMode::kNone ? 0x7fffffff : static_cast<int>(schema.size())));
  }
  std::unique_ptr<tier0::Args> prog(new tier0::Args);
  std::string why;
  if (!BuildTier0Program(schema, exprs, is_condition, plan, prog.get(), &why)) return Status::NotImplemented("no tier 0: " + why);
  *text = DescribeTier0Program(*prog);
  return Status::OK();
}

// ------------------------------------------------------------------ precompile (no device)

Status PrecompileProjector(const Schema& schema, const std::vector<ExpressionPtr>& exprs,
                           SelectionMode mode) {
  KernelPlan plan;
  StagedExpressions staged;
  StageMaterialisedValues(schema, exprs, &staged, CodegenOptions::FromEnv());
  if (!staged.pre.empty()) {
    for (auto& e : exprs) GDV_RETURN_NOT_OK(ValidateExpression(schema, *e));
    GDV_RETURN_NOT_OK(PrecompileProjector(schema, staged.pre, mode));
    CodegenOptions second = CodegenOptions::FromEnv();
    second.rows_word = true;
    GDV_RETURN_NOT_OK(PlanProjector(staged.schema, staged.main, mode, second, &plan,
                                    mode == SelectionMode::kNone ? 0x7fffffff : static_cast<int>(schema.size())));
  } else {
    GDV_RETURN_NOT_OK(PlanProjector(schema, exprs, mode, CodegenOptions::FromEnv(), &plan));
  }
  std::vector<char> code;
  GDV_RETURN_NOT_OK(Runtime::Get().CompileToCodeObject(plan.source, plan.kernel_name, &code));
  // the variant without the optimistic flat path is otherwise compiled only when a batch needs it
  // (offline tool path, not reachable from Evaluate)
  if (!plan.source_general.empty() && std::getenv("GDV_PRECOMPILE_SKIP_GENERAL") == nullptr)
    GDV_RETURN_NOT_OK(Runtime::Get().CompileToCodeObject(plan.source_general, plan.kernel_name_general, &code));
  if (plan.prepass)
    GDV_RETURN_NOT_OK(Runtime::Get().CompileToCodeObject(plan.prepass->source, plan.prepass->kernel_name, &code));
  if (plan.exact && std::getenv("GDV_PRECOMPILE_SKIP_GENERAL") == nullptr) {  // (as the general variant: on demand at run time)
    GDV_RETURN_NOT_OK(Runtime::Get().CompileToCodeObject(plan.exact->source, plan.exact->kernel_name, &code));
    if (plan.exact->prepass)
      GDV_RETURN_NOT_OK(Runtime::Get().CompileToCodeObject(plan.exact->prepass->source, plan.exact->prepass->kernel_name, &code));
  }
  return Status::OK();
}

Status PrecompileFilter(const Schema& schema, const ExpressionPtr& condition) {
  KernelPlan plan;
  StagedExpressions staged;
  StageMaterialisedValues(schema, {condition}, &staged, CodegenOptions::FromEnv());
  if (!staged.pre.empty()) {
    GDV_RETURN_NOT_OK(ValidateExpression(schema, *condition));
    GDV_RETURN_NOT_OK(PrecompileProjector(schema, staged.pre, SelectionMode::kNone));
    GDV_RETURN_NOT_OK(PlanFilter(staged.schema, staged.main[0], CodegenOptions::FromEnv(), &plan));
  } else {
    GDV_RETURN_NOT_OK(PlanFilter(schema, condition, CodegenOptions::FromEnv(), &plan));
  }
  std::vector<char> code;
  return Runtime::Get().CompileToCodeObject(plan.source, plan.kernel_name, &code);
}

Status PrecompileFilterProject(const Schema& schema, const ExpressionPtr& condition,
                               const std::vector<ExpressionPtr>& exprs, SelectionMode index_mode) {
  KernelPlan plan;
  GDV_RETURN_NOT_OK(PlanFilterProject(schema, condition, exprs, index_mode, CodegenOptions::FromEnv(), &plan));
  std::vector<char> code;
  GDV_RETURN_NOT_OK(Runtime::Get().CompileToCodeObject(plan.source, plan.kernel_name, &code));
  if (plan.exact)  // round 5: the direct kernel behind the windowed one
    GDV_RETURN_NOT_OK(Runtime::Get().CompileToCodeObject(plan.exact->source, plan.exact->kernel_name, &code));
  return Status::OK();
}

Status FilterProjectPlanText(const Schema& schema, const ExpressionPtr& condition, const std::vector<ExpressionPtr>& exprs,
                             SelectionMode index_mode, int shape, bool with_small, bool compile, std::string* text) {
  KernelPlan plan;
  GDV_RETURN_NOT_OK(PlanFilterProject(schema, condition, exprs, index_mode, CodegenOptions::FromEnv(), &plan, with_small));
  const KernelPlan* which = shape == 0 ? &plan : shape == 1 ? plan.exact.get() : shape == 2 ? plan.small.get() : nullptr;
  if (shape < 0 || shape > 2) return Status::Invalid("fused filter-project: shapes are 0 (main), 1 (direct), 2 (small)");
  if (which == nullptr)
    return Status::CodeGenError(shape == 2 ? "fused filter-project: the plan has no small shape" : "fused filter-project: the plan has one shape only");
  if (compile) {
    std::vector<char> code;
    GDV_RETURN_NOT_OK(Runtime::Get().CompileToCodeObject(which->source, which->kernel_name, &code));
  }
  *text = which->source;
  return Status::OK();
}

}  // namespace gdv
