// C ABI, the Arrow C device data interface: batches imported as struct arrays, results exported the same way.
#include "gdv_c_api_internal.h"

using namespace gdv;
using namespace gdv::capi;

extern "C" {

// ---------------------------------------------------------------- C device data interface
namespace {

// struct array (one child per field) -> gdv_column_t[]; sizes are derived from
// offset + length and the field type because the C data interface carries no buffer sizes
Status ImportBatch(const Schema& schema, const ArrowDeviceArray* batch, hipStream_t stream,
                   std::vector<ColumnBuffers>* cols, MemKind* mem, int64_t* num_rows) {
  if (batch == nullptr) return Status::Invalid("null ArrowDeviceArray");
  const ArrowArray& a = batch->array;
  if (a.release == nullptr) return Status::Invalid("ArrowDeviceArray was already released");
  if (a.n_children != static_cast<int64_t>(schema.size()))
    return Status::Invalid("ArrowDeviceArray has " + std::to_string(a.n_children) +
                           " children, the schema has " + std::to_string(schema.size()) + " fields");
  if (a.offset != 0) return Status::Invalid("struct-level offset is not supported");
  switch (batch->device_type) {
    case ARROW_DEVICE_ROCM: *mem = MemKind::kDevice; break;
    case ARROW_DEVICE_CPU: case ARROW_DEVICE_ROCM_HOST: *mem = MemKind::kHost; break;
    default: return Status::Invalid("unsupported ArrowDeviceType " + std::to_string(batch->device_type));
  }
  if (batch->sync_event != nullptr && *mem == MemKind::kDevice)
    GDV_HIP_RETURN_NOT_OK(hipStreamWaitEvent(stream, *static_cast<hipEvent_t*>(batch->sync_event), 0));
  *num_rows = a.length;
  cols->assign(schema.size(), ColumnBuffers());
  for (size_t i = 0; i < schema.size(); i++) {
    const ArrowArray* c = a.children[i];
    if (c == nullptr) return Status::Invalid("null child array");
    if (c->length != a.length) return Status::Invalid("child length differs from the batch length");
    const DataType& t = schema[i].type;
    ColumnBuffers& col = (*cols)[i];
    const int64_t rows = c->offset + c->length;
    col.offset = c->offset;
    const int64_t want = t.is_varlen() ? 3 : 2;
    if (c->n_buffers < want) continue;  // e.g. a null-type child: fails later only if referenced
    col.validity = c->buffers[0];
    col.validity_size = col.validity ? (rows + 7) / 8 : 0;
    if (t.is_varlen()) {
      col.offsets = c->buffers[1];
      col.offsets_size = (rows + 1) * 4;
      col.data = c->buffers[2];
      int32_t last = 0;  // byte extent = the last offset
      if (col.offsets != nullptr && rows >= 0) {
        const char* src = static_cast<const char*>(col.offsets) + rows * 4;
        if (*mem == MemKind::kDevice) {
          GDV_HIP_RETURN_NOT_OK(hipMemcpyAsync(&last, src, 4, hipMemcpyDeviceToHost, stream));
          GDV_HIP_RETURN_NOT_OK(hipStreamSynchronize(stream));
        } else {
          std::memcpy(&last, src, 4);
        }
      }
      col.data_size = last;
    } else {
      col.data = c->buffers[1];
      col.data_size = t.id == kBool ? (rows + 7) / 8 : rows * t.byte_width();
    }
  }
  return Status::OK();
}

}  // namespace

int gdv_projector_evaluate_device_array(const gdv_projector_t* p, const ArrowDeviceArray* batch,
                                        const gdv_selection_t* sel, gdv_out_column_t* outs,
                                        int num_outs, void* stream, uint32_t flags) {
  return Guarded([&]() -> int {
  if (!p) return Fail(Status::Invalid("null projector"));
  if (!outs) return Fail(Status::Invalid("Output array vector cannot be null"));
  std::vector<ColumnBuffers> cols;
  MemKind mem;
  int64_t rows = 0;
  Status st = ImportBatch(p->p->schema(), batch, static_cast<hipStream_t>(stream), &cols, &mem, &rows);
  if (!st.ok()) return Fail(st);
  std::vector<OutputBuffers> o = ToOutputs(outs, num_outs);
  SelectionView sv;
  if (!ToSelection(sel, nullptr, &sv)) return Fail(Status::Invalid("bad selection mode"));
  st = p->p->Evaluate(rows, cols.data(), static_cast<int>(cols.size()), sel ? &sv : nullptr, o.data(),
                      num_outs, mem, static_cast<hipStream_t>(stream), flags);
  WriteBackDataSizes(outs, o, num_outs);
  return Check(st);
  });
}

int gdv_filter_evaluate_device_array(const gdv_filter_t* f, const ArrowDeviceArray* batch,
                                     int selection_mode, void* out_indices, int64_t max_slots,
                                     int64_t* num_selected, void* stream) {
  return Guarded([&]() -> int {
  if (!f) return Fail(Status::Invalid("null filter"));
  SelectionMode mode;
  if (!ToSelectionMode(selection_mode, &mode)) return Fail(Status::Invalid("bad selection mode"));
  std::vector<ColumnBuffers> cols;
  MemKind mem;
  int64_t rows = 0;
  Status st = ImportBatch(f->f->schema(), batch, static_cast<hipStream_t>(stream), &cols, &mem, &rows);
  if (!st.ok()) return Fail(st);
  return Check(f->f->Evaluate(rows, cols.data(), static_cast<int>(cols.size()), mode, out_indices,
                              max_slots, num_selected, mem, static_cast<hipStream_t>(stream)));
  });
}

// ---------------------------------------------------------------- C device data export
namespace {

// Buffers of one exported batch: owned jointly by the parent array and every child (a
// consumer may move children out and release them on their own).
struct ExportBlock {
  MemKind mem = MemKind::kHost;
  std::vector<void*> bufs;
  hipEvent_t event = nullptr;
  ~ExportBlock() {
    for (void* b : bufs) {
      if (mem == MemKind::kDevice) Runtime::Get().Free(b); else std::free(b);
    }
    if (event != nullptr) (void)hipEventDestroy(event);
  }
  Status Allocate(int64_t bytes, void** out) {
    const size_t padded = static_cast<size_t>((std::max<int64_t>(bytes, 1) + 63) / 64 * 64);
    if (mem == MemKind::kDevice) {
      GDV_RETURN_NOT_OK(Runtime::Get().Alloc(padded, out));
    } else {
      *out = std::aligned_alloc(64, padded);
      if (*out == nullptr) return Status::OutOfMemory("host allocation of " + std::to_string(padded) + " bytes failed");
    }
    bufs.push_back(*out);
    return Status::OK();
  }
  void Drop(void* b) {  // give one buffer back early (var-len data regrown)
    for (auto it = bufs.begin(); it != bufs.end(); ++it)
      if (*it == b) { bufs.erase(it); break; }
    if (mem == MemKind::kDevice) Runtime::Get().Free(b); else std::free(b);
  }
};

struct ExportNode {  // private_data of an exported ArrowArray
  std::shared_ptr<ExportBlock> block;
  const void* buffers[3] = {nullptr, nullptr, nullptr};
  std::vector<ArrowArray*> children;
};

void ReleaseExportedArray(ArrowArray* a) {
  if (a == nullptr || a->release == nullptr) return;
  auto* node = static_cast<ExportNode*>(a->private_data);
  for (ArrowArray* c : node->children) {
    if (c->release != nullptr) c->release(c);
    delete c;
  }
  delete node;
  a->release = nullptr;
}

struct SchemaNode {  // private_data of an exported ArrowSchema
  std::string format, name;
  std::vector<ArrowSchema*> children;
};

void ReleaseExportedSchema(ArrowSchema* s) {
  if (s == nullptr || s->release == nullptr) return;
  auto* node = static_cast<SchemaNode*>(s->private_data);
  for (ArrowSchema* c : node->children) {
    if (c->release != nullptr) c->release(c);
    delete c;
  }
  delete node;
  s->release = nullptr;
}

// Arrow C data interface format string (pyarrow/include/arrow/c/abi.h; format spec §"Data
// type description")
std::string FormatOf(const DataType& t) {
  static const char* const units = "smun";
  switch (t.id) {
    case kBool: return "b";
    case kInt8: return "c";
    case kUInt8: return "C";
    case kInt16: return "s";
    case kUInt16: return "S";
    case kInt32: return "i";
    case kUInt32: return "I";
    case kInt64: return "l";
    case kUInt64: return "L";
    case kFloat: return "f";
    case kDouble: return "g";
    case kString: return "u";
    case kBinary: return "z";
    case kDate32: return "tdD";
    case kDate64: return "tdm";
    case kTimestamp: return std::string("ts") + units[t.precision & 3] + ":";
    case kTime32: return std::string("tt") + units[t.precision & 3];
    case kTime64: return std::string("tt") + units[t.precision & 3];
    case kDecimal128: return "d:" + std::to_string(t.precision) + "," + std::to_string(t.scale);
    default: return "n";
  }
}

void FillSchema(ArrowSchema* s, const std::string& format, const std::string& name, int64_t flags) {
  auto* node = new SchemaNode{format, name, {}};
  std::memset(s, 0, sizeof(*s));
  s->format = node->format.c_str();
  s->name = node->name.c_str();
  s->flags = flags;
  s->private_data = node;
  s->release = ReleaseExportedSchema;
}

}  // namespace

int gdv_projector_evaluate_export(const gdv_projector_t* p, const ArrowDeviceArray* batch,
                                  const gdv_selection_t* sel, void* stream_ptr,
                                  ArrowDeviceArray* out, ArrowSchema* out_schema) {
  return Guarded([&]() -> int {
  if (!p) return Fail(Status::Invalid("null projector"));
  if (!out) return Fail(Status::Invalid("null output ArrowDeviceArray"));
  hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
  std::vector<ColumnBuffers> cols;
  MemKind mem;
  int64_t rows = 0;
  Status st = ImportBatch(p->p->schema(), batch, stream, &cols, &mem, &rows);
  if (!st.ok()) return Fail(st);
  SelectionView sv;
  if (!ToSelection(sel, nullptr, &sv)) return Fail(Status::Invalid("bad selection mode"));
  const int64_t out_rows = sel ? sel->num_slots : rows;
  const int n_out = p->p->num_outputs();
  const bool dev = mem == MemKind::kDevice;
  auto block = std::make_shared<ExportBlock>();
  block->mem = mem;
  std::vector<OutputBuffers> o(n_out);
  int64_t varlen_guess = 64;
  for (auto& c : cols) if (c.offsets != nullptr) varlen_guess += c.data_size;
  for (int e = 0; e < n_out; e++) {
    const DataType& t = p->p->output_type(e);
    o[e].validity_size = dev ? Projector::ValidityBytes(out_rows) : (out_rows + 7) / 8;
    if (t.is_varlen()) {
      o[e].offsets_size = (out_rows + 1) * 4;
      const int64_t hint = p->p->VarlenBytesHint(e, out_rows);  // what earlier batches produced per row
      o[e].data_size = hint > 0 ? hint : varlen_guess;
      st = block->Allocate(o[e].offsets_size, &o[e].offsets);
      if (!st.ok()) return Fail(st);
    } else {
      o[e].data_size = t.id == kBool ? o[e].validity_size : Projector::DataBytes(t, out_rows);
    }
    st = block->Allocate(o[e].validity_size, &o[e].validity);
    if (st.ok()) st = block->Allocate(o[e].data_size, &o[e].data);
    if (!st.ok()) return Fail(st);
  }
  for (int attempt = 0; attempt < 2; attempt++) {
    std::vector<int64_t> caps(n_out);
    for (int e = 0; e < n_out; e++) caps[e] = o[e].data_size;
    st = p->p->Evaluate(rows, cols.data(), static_cast<int>(cols.size()), sel ? &sv : nullptr, o.data(),
                        n_out, mem, stream, 0);
    if (st.ok() || attempt == 1) break;
    bool grown = false;  // a var-len output needed more bytes than guessed: regrow once
    for (int e = 0; e < n_out; e++) {
      if (!p->p->output_type(e).is_varlen()) continue;
      if (o[e].data_size > caps[e]) {
        block->Drop(o[e].data);
        Status a = block->Allocate(o[e].data_size, &o[e].data);
        if (!a.ok()) return Fail(a);
        grown = true;
      } else {
        o[e].data_size = caps[e];
      }
    }
    if (!grown) break;
  }
  if (!st.ok()) return Fail(st);
  if (dev) {
    hipError_t he = hipEventCreateWithFlags(&block->event, hipEventDisableTiming);
    if (he == hipSuccess) he = hipEventRecord(block->event, stream);
    if (he != hipSuccess) return Fail(Status::ExecutionError(hipGetErrorString(he)));
  }
  // ---- assemble the struct array
  auto* parent = new ExportNode();
  parent->block = block;
  for (int e = 0; e < n_out; e++) {
    const DataType& t = p->p->output_type(e);
    auto* node = new ExportNode();
    node->block = block;
    auto* child = new ArrowArray();
    std::memset(child, 0, sizeof(*child));
    child->length = out_rows;
    child->null_count = -1;  // not computed
    node->buffers[0] = o[e].validity;
    if (t.is_varlen()) {
      node->buffers[1] = o[e].offsets;
      node->buffers[2] = o[e].data;
      child->n_buffers = 3;
    } else {
      node->buffers[1] = o[e].data;
      child->n_buffers = 2;
    }
    child->buffers = node->buffers;
    child->private_data = node;
    child->release = ReleaseExportedArray;
    parent->children.push_back(child);
  }
  std::memset(out, 0, sizeof(*out));
  out->array.length = out_rows;
  out->array.null_count = 0;
  out->array.n_buffers = 1;
  out->array.buffers = parent->buffers;  // {NULL}: a struct array without a validity bitmap
  out->array.n_children = n_out;
  out->array.children = parent->children.data();
  out->array.private_data = parent;
  out->array.release = ReleaseExportedArray;
  int device_id = 0;
  if (dev) (void)hipGetDevice(&device_id);
  out->device_id = dev ? device_id : -1;
  out->device_type = dev ? ARROW_DEVICE_ROCM : ARROW_DEVICE_CPU;
  out->sync_event = dev ? static_cast<void*>(&block->event) : nullptr;
  if (out_schema != nullptr) {
    FillSchema(out_schema, "+s", "", 0);
    auto* sn = static_cast<SchemaNode*>(out_schema->private_data);
    for (int e = 0; e < n_out; e++) {
      auto* cs = new ArrowSchema();
      FillSchema(cs, FormatOf(p->p->output_type(e)), p->output_names[e], /*ARROW_FLAG_NULLABLE*/ 2);
      sn->children.push_back(cs);
    }
    out_schema->n_children = n_out;
    out_schema->children = sn->children.data();
  }
  return GDV_OK;
  });
}

}  // extern "C"
