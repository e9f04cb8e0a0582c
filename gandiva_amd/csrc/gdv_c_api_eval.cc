// C ABI, the three operators: make (also from protobuf bytes), accessors, every Evaluate variant, tuning, dump, free.
#include "gdv_c_api_internal.h"

using namespace gdv;
using namespace gdv::capi;

namespace gdv {
namespace capi {
int ProjectorEvaluate(const gdv_projector_t* p, int64_t num_rows, const gdv_column_t* cols,
                      int num_cols, const gdv_selection_t* sel, const void* num_slots_device,
                      gdv_out_column_t* outs, int num_outs, int mem_kind, void* stream, uint32_t flags) {
  return Guarded([&]() -> int {
  if (!p) return Fail(Status::Invalid("null projector"));
  if (num_cols > 0 && !cols) return Fail(Status::Invalid("null column array"));
  if (!outs) return Fail(Status::Invalid("Output array vector cannot be null"));
  std::vector<ColumnBuffers> c = ToColumns(cols, num_cols);
  std::vector<OutputBuffers> o = ToOutputs(outs, num_outs);
  SelectionView sv;
  if (!ToSelection(sel, num_slots_device, &sv)) return Fail(Status::Invalid("bad selection mode"));
  Status st = p->p->Evaluate(num_rows, c.data(), num_cols, sel ? &sv : nullptr, o.data(), num_outs,
                             ToMemKind(mem_kind), static_cast<hipStream_t>(stream), flags);
  WriteBackDataSizes(outs, o, num_outs);
  return Check(st);
  });
}
}  // namespace capi
}  // namespace gdv

extern "C" {

// ---------------------------------------------------------------- projector
int gdv_projector_make(const gdv_schema_t* schema, gdv_expression_t* const* exprs, int num_exprs,
                       int selection_mode, const gdv_config_t* config, gdv_projector_t** out) {
  return Guarded([&]() -> int {
  if (!schema || !out) return Fail(Status::Invalid("null schema or output pointer"));
  std::vector<ExpressionPtr> ex;
  if (!CollectExprs(exprs, num_exprs, &ex)) return Fail(Status::Invalid("null expression"));
  SelectionMode mode;
  if (!ToSelectionMode(selection_mode, &mode)) return Fail(Status::Invalid("bad selection mode"));
  const Configuration cfg = ToConfig(config);
  std::shared_ptr<Projector> p;
  Status s = Projector::Make(schema->fields, ex, mode, cfg, &p);
  if (!s.ok()) return Fail(s);
  std::vector<std::string> names;
  for (auto& e : ex) names.push_back(e->result().name);
  *out = new gdv_projector{p, std::move(names)};
  return GDV_OK;
  });
}
int gdv_projector_num_outputs(const gdv_projector_t* p) { return p ? p->p->num_outputs() : 0; }
int gdv_projector_path_hint(const gdv_projector_t* p) { return p ? p->p->path_hint() : -1; }
gdv_type_t gdv_projector_output_type(const gdv_projector_t* p, int i) {
  if (!p || i < 0 || i >= p->p->num_outputs()) return gdv_type_t{0, 0, 0};
  return FromType(p->p->output_type(i));
}
int gdv_projector_output_sizes(const gdv_projector_t* p, int i, int64_t rows, int mem_kind,
                               int64_t* validity_bytes, int64_t* data_bytes) {
  if (!p || i < 0 || i >= p->p->num_outputs() || rows < 0) return Fail(Status::Invalid("bad argument"));
  const DataType& t = p->p->output_type(i);
  const bool dev = mem_kind == GDV_MEM_DEVICE;
  if (validity_bytes) *validity_bytes = dev ? Projector::ValidityBytes(rows) : (rows + 7) / 8;
  if (data_bytes && t.is_varlen()) {
    *data_bytes = p->p->VarlenBytesHint(i, rows);  // 0 until a batch has been evaluated
    return GDV_OK;
  }
  if (data_bytes)
    *data_bytes = t.id == kBool ? (dev ? Projector::ValidityBytes(rows) : (rows + 7) / 8)
                                : Projector::DataBytes(t, rows);
  return GDV_OK;
}

int gdv_projector_evaluate(const gdv_projector_t* p, int64_t num_rows, const gdv_column_t* cols,
                           int num_cols, const gdv_selection_t* sel, gdv_out_column_t* outs,
                           int num_outs, int mem_kind, void* stream, uint32_t flags) {
  return ProjectorEvaluate(p, num_rows, cols, num_cols, sel, nullptr, outs, num_outs, mem_kind, stream, flags);
}
int gdv_projector_evaluate_selected(const gdv_projector_t* p, int64_t num_rows, const gdv_column_t* cols,
                                    int num_cols, const gdv_selection_t* sel, const void* num_slots_device,
                                    gdv_out_column_t* outs, int num_outs, void* stream, uint32_t flags) {
  if (!sel || !num_slots_device) return Fail(Status::Invalid("selection vector and device slot count are required"));
  return ProjectorEvaluate(p, num_rows, cols, num_cols, sel, num_slots_device, outs, num_outs, GDV_MEM_DEVICE, stream,
                           flags);
}
int gdv_projector_evaluate_async(const gdv_projector_t* p, int64_t num_rows, const gdv_column_t* cols, int num_cols,
                                 const gdv_selection_t* sel, const void* num_slots_device, gdv_out_column_t* outs,
                                 int num_outs, void* stream, void* result) {
  return Guarded([&]() -> int {
  if (!p) return Fail(Status::Invalid("null projector"));
  if (num_cols > 0 && !cols) return Fail(Status::Invalid("null column array"));
  if (!outs || !result) return Fail(Status::Invalid("Output array vector and result block cannot be null"));
  std::vector<ColumnBuffers> c = ToColumns(cols, num_cols);
  std::vector<OutputBuffers> o = ToOutputs(outs, num_outs);
  SelectionView sv;
  if (!ToSelection(sel, num_slots_device, &sv)) return Fail(Status::Invalid("bad selection mode"));
  return Check(p->p->EvaluateAsync(num_rows, c.data(), num_cols, sel ? &sv : nullptr, o.data(), num_outs,
                                   static_cast<hipStream_t>(stream), result));
  });
}
int gdv_projector_evaluate_many(const gdv_projector_t* p, const gdv_batch_t* batches, int num_batches, void* stream,
                                uint32_t flags) {
  return Guarded([&]() -> int {
  if (!p) return Fail(Status::Invalid("null projector"));
  if (num_batches < 0 || (num_batches > 0 && !batches)) return Fail(Status::Invalid("null batch list"));
  std::vector<std::vector<ColumnBuffers>> cols(num_batches);
  std::vector<std::vector<OutputBuffers>> outs(num_batches);
  std::vector<Projector::BatchView> views(num_batches);
  for (int b = 0; b < num_batches; b++) {
    const gdv_batch_t& g = batches[b];
    if ((g.num_cols > 0 && !g.cols) || (g.num_outs > 0 && !g.outs)) return Fail(Status::Invalid("null column array"));
    cols[b] = ToColumns(g.cols, g.num_cols);
    outs[b] = ToOutputs(g.outs, g.num_outs);
    views[b].num_rows = g.num_rows;
    views[b].cols = cols[b].data();
    views[b].num_cols = g.num_cols;
    views[b].outs = outs[b].data();
    views[b].num_outs = g.num_outs;
  }
  Status st = p->p->EvaluateMany(views.data(), num_batches, static_cast<hipStream_t>(stream), flags);
  for (int b = 0; b < num_batches; b++) WriteBackDataSizes(batches[b].outs, outs[b], batches[b].num_outs);
  return Check(st);
  });
}
char* gdv_projector_dump_ir(const gdv_projector_t* p) { return p ? DupString(p->p->DumpIR()) : nullptr; }
void gdv_projector_free(gdv_projector_t* p) { delete p; }

// ---------------------------------------------------------------- filter
int gdv_filter_make(const gdv_schema_t* schema, gdv_expression_t* condition,
                    const gdv_config_t* config, gdv_filter_t** out) {
  return Guarded([&]() -> int {
  if (!schema || !out) return Fail(Status::Invalid("null schema or output pointer"));
  if (!condition || !condition->expr) return Fail(Status::Invalid("Condition cannot be null"));
  const Configuration cfg = ToConfig(config);
  std::shared_ptr<Filter> f;
  Status s = Filter::Make(schema->fields, condition->expr, cfg, &f);
  if (!s.ok()) return Fail(s);
  *out = new gdv_filter{f};
  return GDV_OK;
  });
}
int gdv_filter_evaluate(const gdv_filter_t* f, int64_t num_rows, const gdv_column_t* cols,
                        int num_cols, int selection_mode, void* out_indices, int64_t max_slots,
                        int64_t* num_selected, int mem_kind, void* stream) {
  return Guarded([&]() -> int {
  if (!f) return Fail(Status::Invalid("null filter"));
  if (num_cols > 0 && !cols) return Fail(Status::Invalid("null column array"));
  SelectionMode mode;
  if (!ToSelectionMode(selection_mode, &mode)) return Fail(Status::Invalid("bad selection mode"));
  std::vector<ColumnBuffers> c = ToColumns(cols, num_cols);
  return Check(f->f->Evaluate(num_rows, c.data(), num_cols, mode, out_indices, max_slots,
                              num_selected, ToMemKind(mem_kind),
                              static_cast<hipStream_t>(stream)));
  });
}
int gdv_filter_evaluate_async(const gdv_filter_t* f, int64_t num_rows, const gdv_column_t* cols, int num_cols,
                              int selection_mode, void* out_indices, int64_t max_slots, void* num_selected_device,
                              void* stream) {
  return Guarded([&]() -> int {
  if (!f) return Fail(Status::Invalid("null filter"));
  if (num_cols > 0 && !cols) return Fail(Status::Invalid("null column array"));
  if (!num_selected_device) return Fail(Status::Invalid("null count pointer"));
  SelectionMode mode;
  if (!ToSelectionMode(selection_mode, &mode)) return Fail(Status::Invalid("bad selection mode"));
  std::vector<ColumnBuffers> c = ToColumns(cols, num_cols);
  int64_t unused = 0;
  return Check(f->f->Evaluate(num_rows, c.data(), num_cols, mode, out_indices, max_slots, &unused, MemKind::kDevice,
                              static_cast<hipStream_t>(stream), kEvalAsync, num_selected_device));
  });
}
int gdv_filter_evaluate_many(const gdv_filter_t* f, const gdv_filter_batch_t* batches, int num_batches,
                             int selection_mode, int64_t* num_selected, void* num_selected_device, void* stream,
                             uint32_t flags) {
  return Guarded([&]() -> int {
  if (!f) return Fail(Status::Invalid("null filter"));
  if (num_batches < 0 || (num_batches > 0 && !batches)) return Fail(Status::Invalid("null batch list"));
  SelectionMode mode;
  if (!ToSelectionMode(selection_mode, &mode)) return Fail(Status::Invalid("bad selection mode"));
  std::vector<std::vector<ColumnBuffers>> cols(num_batches);
  std::vector<Filter::BatchView> views(num_batches);
  for (int b = 0; b < num_batches; b++) {
    if (batches[b].num_cols > 0 && !batches[b].cols) return Fail(Status::Invalid("null column array"));
    cols[b] = ToColumns(batches[b].cols, batches[b].num_cols);
    views[b].num_rows = batches[b].num_rows;
    views[b].cols = cols[b].data();
    views[b].num_cols = batches[b].num_cols;
    views[b].out_indices = batches[b].out_indices;
    views[b].max_slots = batches[b].max_slots;
  }
  return Check(f->f->EvaluateMany(views.data(), num_batches, mode, num_selected, num_selected_device,
                                  static_cast<hipStream_t>(stream), flags));
  });
}

// ---------------------------------------------------------------- build from protobuf bytes (JNI)
int gdv_projector_make_from_proto(const void* schema_bytes, int64_t schema_len, const void* exprs_bytes,
                                  int64_t exprs_len, int selection_mode, const gdv_config_t* config,
                                  gdv_projector_t** out) {
  return Guarded([&]() -> int {
  if (!out || schema_len < 0 || exprs_len < 0) return Fail(Status::Invalid("bad argument"));
  Schema schema;
  std::vector<ExpressionPtr> ex;
  Status s = DecodePlan({schema_bytes, schema_len}, {}, {exprs_bytes, exprs_len}, &schema, nullptr, &ex);
  if (!s.ok()) return Fail(s);
  SelectionMode mode;
  if (!ToSelectionMode(selection_mode, &mode)) return Fail(Status::Invalid("bad selection mode"));
  const Configuration cfg = ToConfig(config);
  std::shared_ptr<Projector> p;
  s = Projector::Make(schema, ex, mode, cfg, &p);
  if (!s.ok()) return Fail(s);
  std::vector<std::string> names;
  for (auto& e : ex) names.push_back(e->result().name);
  *out = new gdv_projector{p, std::move(names)};
  return GDV_OK;
  });
}
int gdv_filter_make_from_proto(const void* schema_bytes, int64_t schema_len, const void* condition_bytes,
                               int64_t condition_len, const gdv_config_t* config, gdv_filter_t** out) {
  return Guarded([&]() -> int {
  if (!out || schema_len < 0 || condition_len < 0) return Fail(Status::Invalid("bad argument"));
  Schema schema;
  ExpressionPtr cond;
  Status s = DecodePlan({schema_bytes, schema_len}, {condition_bytes, condition_len}, {}, &schema, &cond, nullptr);
  if (!s.ok()) return Fail(s);
  const Configuration cfg = ToConfig(config);
  std::shared_ptr<Filter> f;
  s = Filter::Make(schema, cond, cfg, &f);
  if (!s.ok()) return Fail(s);
  *out = new gdv_filter{f};
  return GDV_OK;
  });
}
int gdv_filter_project_make_from_proto(const void* schema_bytes, int64_t schema_len, const void* condition_bytes,
                                       int64_t condition_len, const void* exprs_bytes, int64_t exprs_len, int index_mode,
                                       const gdv_config_t* config, gdv_filter_project_t** out) {
  return Guarded([&]() -> int {
  if (!out || schema_len < 0 || condition_len < 0 || exprs_len < 0) return Fail(Status::Invalid("bad argument"));
  SelectionMode mode;
  if (!ToSelectionMode(index_mode, &mode)) return Fail(Status::Invalid("bad selection mode"));
  Schema schema;
  ExpressionPtr cond;
  std::vector<ExpressionPtr> exprs;
  Status s = DecodePlan({schema_bytes, schema_len}, {condition_bytes, condition_len}, {exprs_bytes, exprs_len}, &schema, &cond,
                        &exprs);
  if (!s.ok()) return Fail(s);
  const Configuration cfg = ToConfig(config);
  std::shared_ptr<FilterProject> fp;
  s = FilterProject::Make(schema, cond, exprs, mode, cfg, &fp);
  if (!s.ok()) return Fail(s);
  *out = new gdv_filter_project{fp};
  return GDV_OK;
  });
}
// the decoded trees, rendered (what a test — or a maintainer diffing against the Java side — reads)
char* gdv_proto_describe(const void* schema_bytes, int64_t schema_len, const void* exprs_bytes, int64_t exprs_len,
                         int is_condition) {
  return GuardedPtr([&]() -> char* {
  if (schema_len < 0 || exprs_len < 0 || (schema_len > 0 && schema_bytes == nullptr) ||
      (exprs_len > 0 && exprs_bytes == nullptr)) {
    Fail(Status::Invalid("gdv_proto_describe: negative length or null message"));
    return nullptr;
  }
  Schema schema;
  ExpressionPtr cond;
  std::vector<ExpressionPtr> ex;
  // (exprs_bytes holds the one message or the other)
  Status s = DecodePlan({schema_bytes, schema_len}, {exprs_bytes, exprs_len}, {exprs_bytes, exprs_len}, &schema,
                        is_condition ? &cond : nullptr, is_condition ? nullptr : &ex);
  if (!s.ok()) { Fail(s); return nullptr; }
  std::string text;
  for (auto& f : schema) text += "field " + f.name + ": " + f.type.ToString() + (f.nullable ? "" : " not null") + "\n";
  if (is_condition) text += "condition " + cond->ToString() + "\n";
  for (auto& e : ex) text += "expr " + e->result().name + ": " + e->result().type.ToString() + " = " + e->ToString() + "\n";
  return DupString(text);
  });
}
char* gdv_filter_dump_ir(const gdv_filter_t* f) { return f ? DupString(f->f->DumpIR()) : nullptr; }
void gdv_filter_free(gdv_filter_t* f) { delete f; }
int gdv_filter_set_tuning(gdv_filter_t* f, const char* key, int64_t value) {
  return Guarded([&]() -> int {
    if (f == nullptr || key == nullptr) return Fail(Status::Invalid("gdv_filter_set_tuning: null argument"));
    Status st = f->f->SetTuning(key, value);
    return st.ok() ? GDV_OK : Fail(st);
  });
}

// ---------------------------------------------------------------- fused filter -> project
int gdv_filter_project_make(const gdv_schema_t* schema, gdv_expression_t* condition, gdv_expression_t* const* exprs,
                            int num_exprs, int index_mode, const gdv_config_t* config, gdv_filter_project_t** out) {
  return Guarded([&]() -> int {
  if (!schema || !out) return Fail(Status::Invalid("null schema or output pointer"));
  if (!condition || !condition->expr) return Fail(Status::Invalid("Condition cannot be null"));
  if (num_exprs <= 0 || !exprs) return Fail(Status::Invalid("Expressions cannot be empty"));
  SelectionMode mode;
  if (!ToSelectionMode(index_mode, &mode)) return Fail(Status::Invalid("bad selection mode"));
  std::vector<ExpressionPtr> ex;
  if (!CollectExprs(exprs, num_exprs, &ex)) return Fail(Status::Invalid("Expression cannot be null"));
  const Configuration cfg = ToConfig(config);
  std::shared_ptr<FilterProject> fp;
  Status s = FilterProject::Make(schema->fields, condition->expr, ex, mode, cfg, &fp);
  if (!s.ok()) return Fail(s);
  *out = new gdv_filter_project{fp};
  return GDV_OK;
  });
}
int gdv_filter_project_num_outputs(const gdv_filter_project_t* fp) { return fp ? fp->fp->num_outputs() : 0; }
gdv_type_t gdv_filter_project_output_type(const gdv_filter_project_t* fp, int i) {
  if (!fp || i < 0 || i >= fp->fp->num_outputs()) return gdv_type_t{0, 0, 0};
  return FromType(fp->fp->output_type(i));
}
int gdv_filter_project_evaluate(const gdv_filter_project_t* fp, int64_t num_rows, const gdv_column_t* cols, int num_cols,
                                gdv_out_column_t* outs, int num_outs, void* out_indices, int64_t max_slots,
                                int64_t* num_selected, void* num_selected_device, int mem_kind, void* stream,
                                uint32_t flags) {
  return Guarded([&]() -> int {
  if (!fp) return Fail(Status::Invalid("null filter-project"));
  if ((num_cols > 0 && !cols) || (num_outs > 0 && !outs)) return Fail(Status::Invalid("null column array"));
  std::vector<ColumnBuffers> c = ToColumns(cols, num_cols);
  std::vector<OutputBuffers> o = ToOutputs(outs, num_outs);
  for (auto& b : o) { b.offsets = nullptr; b.offsets_size = 0; }  // fixed-width outputs only: the offsets fields are not passed on
  return Check(fp->fp->Evaluate(num_rows, c.data(), num_cols, o.data(), num_outs, out_indices, max_slots, num_selected,
                                ToMemKind(mem_kind),
                                static_cast<hipStream_t>(stream), flags, num_selected_device));
  });
}
int gdv_filter_project_evaluate_many(const gdv_filter_project_t* fp, const gdv_filter_project_batch_t* batches,
                                     int num_batches, int64_t* num_selected, void* num_selected_device, void* stream,
                                     uint32_t flags) {
  return Guarded([&]() -> int {
  if (!fp) return Fail(Status::Invalid("null filter-project"));
  if (num_batches < 0 || (num_batches > 0 && !batches)) return Fail(Status::Invalid("null batch list"));
  std::vector<std::vector<ColumnBuffers>> cols(num_batches);
  std::vector<std::vector<OutputBuffers>> outs(num_batches);
  std::vector<FilterProject::BatchView> views(num_batches);
  for (int b = 0; b < num_batches; b++) {
    const gdv_filter_project_batch_t& g = batches[b];
    if ((g.num_cols > 0 && !g.cols) || (g.num_outs > 0 && !g.outs))
      return Fail(Status::Invalid("batch " + std::to_string(b) + ": null column array"));
    cols[b] = ToColumns(g.cols, g.num_cols);
    outs[b] = ToOutputs(g.outs, g.num_outs);
    for (auto& o : outs[b]) { o.offsets = nullptr; o.offsets_size = 0; }  // fixed-width outputs only, as the one-batch call
    views[b].num_rows = g.num_rows;
    views[b].cols = cols[b].data();
    views[b].num_cols = g.num_cols;
    views[b].outs = outs[b].data();
    views[b].num_outs = g.num_outs;
    views[b].out_indices = g.out_indices;
    views[b].max_slots = g.max_slots;
  }
  return Check(fp->fp->EvaluateMany(views.data(), num_batches, num_selected, num_selected_device,
                                    static_cast<hipStream_t>(stream), flags));
  });
}
int64_t gdv_filter_project_small_batch_rows(const gdv_filter_project_t* fp) { return fp ? fp->fp->SmallBatchRows() : 0; }
char* gdv_filter_project_dump_ir(const gdv_filter_project_t* fp) { return fp ? DupString(fp->fp->DumpIR()) : nullptr; }
int gdv_filter_project_kernel_shape(const gdv_filter_project_t* fp) { return fp ? fp->fp->which_kernel() : -1; }
int gdv_filter_project_set_tuning(gdv_filter_project_t* fp, const char* key, int64_t value) {
  return Guarded([&]() -> int {
    if (fp == nullptr || key == nullptr) return Fail(Status::Invalid("gdv_filter_project_set_tuning: null argument"));
    Status st = fp->fp->SetTuning(key, value);
    return st.ok() ? GDV_OK : Fail(st);
  });
}
void gdv_filter_project_free(gdv_filter_project_t* fp) { delete fp; }

// ---------------------------------------------------------------- JNI-shaped flat entry points
namespace {
// validity, [offsets,] data per field, in schema order
Status UnflattenInputs(const Schema& schema, const int64_t* addrs, const int64_t* sizes, int num_bufs,
                       std::vector<ColumnBuffers>* cols) {
  int want = 0;
  for (auto& f : schema) want += f.type.is_varlen() ? 3 : 2;
  if (num_bufs != want || (want > 0 && (addrs == nullptr || sizes == nullptr)))
    return Status::Invalid("expected " + std::to_string(want) + " input buffers (validity, [offsets,] data per field), got " +
                           std::to_string(num_bufs));
  cols->assign(schema.size(), ColumnBuffers());
  int b = 0;
  for (size_t i = 0; i < schema.size(); i++) {
    ColumnBuffers& c = (*cols)[i];
    c.validity = reinterpret_cast<const void*>(addrs[b]);
    c.validity_size = c.validity ? sizes[b] : 0;
    b++;
    if (schema[i].type.is_varlen()) {
      c.offsets = reinterpret_cast<const void*>(addrs[b]);
      c.offsets_size = sizes[b];
      b++;
    }
    c.data = reinterpret_cast<const void*>(addrs[b]);
    c.data_size = sizes[b];
    b++;
  }
  return Status::OK();
}
}  // namespace

int gdv_projector_evaluate_flat(const gdv_projector_t* p, int64_t num_rows, const int64_t* buf_addrs,
                                const int64_t* buf_sizes, int num_bufs, int sel_mode,
                                int64_t sel_addr, int64_t sel_slots, const int64_t* out_addrs,
                                int64_t* out_sizes, int num_out_bufs, int mem_kind) {
  return Guarded([&]() -> int {
  if (!p) return Fail(Status::Invalid("null projector"));
  std::vector<ColumnBuffers> cols;
  Status st = UnflattenInputs(p->p->schema(), buf_addrs, buf_sizes, num_bufs, &cols);
  if (!st.ok()) return Fail(st);
  const int n_out = p->p->num_outputs();
  int want = 0;
  for (int e = 0; e < n_out; e++) want += p->p->output_type(e).is_varlen() ? 3 : 2;
  if (num_out_bufs != want || out_addrs == nullptr || out_sizes == nullptr)
    return Fail(Status::Invalid("expected " + std::to_string(want) + " output buffers, got " +
                                std::to_string(num_out_bufs)));
  std::vector<OutputBuffers> o(n_out);
  std::vector<int> data_slot(n_out);
  int b = 0;
  for (int e = 0; e < n_out; e++) {
    o[e].validity = reinterpret_cast<void*>(out_addrs[b]);
    o[e].validity_size = out_sizes[b];
    b++;
    if (p->p->output_type(e).is_varlen()) {
      o[e].offsets = reinterpret_cast<void*>(out_addrs[b]);
      o[e].offsets_size = out_sizes[b];
      b++;
    }
    o[e].data = reinterpret_cast<void*>(out_addrs[b]);
    o[e].data_size = out_sizes[b];
    data_slot[e] = b++;
  }
  SelectionView sv;
  if (!ToSelectionMode(sel_mode, &sv.mode)) return Fail(Status::Invalid("bad selection mode"));
  sv.indices = reinterpret_cast<const void*>(sel_addr);
  sv.num_slots = sel_slots;
  const bool has_sel = sv.mode != SelectionMode::kNone;
  st = p->p->Evaluate(num_rows, cols.data(), static_cast<int>(cols.size()), has_sel ? &sv : nullptr,
                      o.data(), n_out, ToMemKind(mem_kind),
                      nullptr, 0);
  for (int e = 0; e < n_out; e++)
    if (p->p->output_type(e).is_varlen()) out_sizes[data_slot[e]] = o[e].data_size;
  return Check(st);
  });
}

int gdv_filter_evaluate_flat(const gdv_filter_t* f, int64_t num_rows, const int64_t* buf_addrs,
                             const int64_t* buf_sizes, int num_bufs, int sel_mode, int64_t out_addr,
                             int64_t out_size_bytes, int64_t* num_selected, int mem_kind) {
  return Guarded([&]() -> int {
  if (!f) return Fail(Status::Invalid("null filter"));
  SelectionMode mode;
  if (!ToSelectionMode(sel_mode, &mode) || mode == SelectionMode::kNone)
    return Fail(Status::Invalid("bad selection mode"));
  std::vector<ColumnBuffers> cols;
  Status st = UnflattenInputs(f->f->schema(), buf_addrs, buf_sizes, num_bufs, &cols);
  if (!st.ok()) return Fail(st);
  const int w = IndexWidth(mode);
  return Check(f->f->Evaluate(num_rows, cols.data(), static_cast<int>(cols.size()), mode,
                              reinterpret_cast<void*>(out_addr), out_size_bytes / w, num_selected,
                              ToMemKind(mem_kind), nullptr));
  });
}

}  // extern "C"
