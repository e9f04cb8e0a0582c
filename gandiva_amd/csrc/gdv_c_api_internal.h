// Shared by the C ABI units (gdv_c_api*.cc): the handle structs, the error plumbing and the C struct -> core converters.
#pragma once
#include "../../include/gandiva_amd.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "gdv_engine.h"
#include "gdv_pool.h"
#include "gdv_proto.h"

struct gdv_schema { gdv::Schema fields; };
struct gdv_node { gdv::NodePtr node; };
struct gdv_expression { gdv::ExpressionPtr expr; };
struct gdv_projector {
  std::shared_ptr<gdv::Projector> p;
  std::vector<std::string> output_names;  // result field names, for the C data export
};
struct gdv_filter { std::shared_ptr<gdv::Filter> f; };
struct gdv_filter_project { std::shared_ptr<gdv::FilterProject> fp; };
struct gdv_device_pool { gdv::DevicePool pool; };

namespace gdv {
namespace capi {

// what gdv_last_error() returns on this thread (the one thread_local string lives in gdv_c_api.cc)
void SetLastError(std::string msg);

inline int Fail(const Status& s) {
  SetLastError(s.ToString());
  return static_cast<int>(s.code);
}
inline int Check(const Status& s) {
  if (s.ok()) return GDV_OK;
  return Fail(s);
}
template <typename T>
T* FailPtr(const std::string& msg) {
  SetLastError("Invalid: " + msg);
  return nullptr;
}

// No C++ exception may cross the C boundary (std::bad_alloc from a vector, a std::string
// length_error …): entry points that allocate run through this guard.
template <typename F>
int Guarded(F&& body) {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    return Fail(Status::OutOfMemory("host allocation failed"));
  } catch (const std::exception& e) {
    return Fail(Status::ExecutionError(std::string("internal error: ") + e.what()));
  } catch (...) {
    return Fail(Status::ExecutionError("internal error: unknown exception"));
  }
}

template <typename F>
auto GuardedPtr(F&& body) -> decltype(body()) {
  try {
    return body();
  } catch (const std::exception& e) {
    SetLastError(std::string("ExecutionError: internal error: ") + e.what());
  } catch (...) {
    SetLastError("ExecutionError: internal error: unknown exception");
  }
  return nullptr;
}

// ------------------------------------------------------------------ converters
inline bool ToType(gdv_type_t t, DataType* out) {
  switch (t.id) {
    case kBool: case kUInt8: case kInt8: case kUInt16: case kInt16: case kUInt32: case kInt32:
    case kUInt64: case kInt64: case kFloat: case kDouble: case kString: case kBinary:
    case kDate32: case kDate64: case kTimestamp: case kTime32: case kTime64: case kDecimal128:
      *out = DataType(static_cast<TypeId>(t.id), t.precision, t.scale);
      return true;
    default:
      return false;
  }
}
inline gdv_type_t FromType(const DataType& t) { return gdv_type_t{t.id, t.precision, t.scale}; }

inline char* DupString(const std::string& s) {
  char* p = static_cast<char*>(malloc(s.size() + 1));
  if (p) std::memcpy(p, s.c_str(), s.size() + 1);
  return p;
}

inline bool CollectChildren(gdv_node_t* const* children, int n, NodeVector* out) {
  if (n < 0 || (n > 0 && children == nullptr)) return false;
  for (int i = 0; i < n; i++) {
    if (children[i] == nullptr || !children[i]->node) return false;
    out->push_back(children[i]->node);
  }
  return true;
}

// require_tree = false: a handle without a tree passes (the tier-0 descriptions refuse only a null handle)
inline bool CollectExprs(gdv_expression_t* const* exprs, int n, std::vector<ExpressionPtr>* out, bool require_tree = true) {
  if (n < 0 || (n > 0 && !exprs)) return false;
  for (int i = 0; i < n; i++) {
    if (!exprs[i] || (require_tree && !exprs[i]->expr)) return false;
    out->push_back(exprs[i]->expr);
  }
  return true;
}

inline std::vector<ColumnBuffers> ToColumns(const gdv_column_t* cols, int n) {
  std::vector<ColumnBuffers> v(n > 0 ? n : 0);
  for (int i = 0; i < n; i++) {
    v[i].validity = cols[i].validity;
    v[i].validity_size = cols[i].validity_size;
    v[i].data = cols[i].data;
    v[i].data_size = cols[i].data_size;
    v[i].offsets = cols[i].offsets;
    v[i].offsets_size = cols[i].offsets_size;
    v[i].offset = cols[i].offset;
  }
  return v;
}

inline std::vector<OutputBuffers> ToOutputs(const gdv_out_column_t* outs, int n) {
  std::vector<OutputBuffers> o(n > 0 ? n : 0);
  for (int i = 0; i < n; i++) {
    o[i].validity = outs[i].validity; o[i].validity_size = outs[i].validity_size;
    o[i].data = outs[i].data; o[i].data_size = outs[i].data_size;
    o[i].offsets = outs[i].offsets; o[i].offsets_size = outs[i].offsets_size;
  }
  return o;
}
// var-len: bytes produced / needed, whether the evaluation succeeded or not
inline void WriteBackDataSizes(gdv_out_column_t* outs, const std::vector<OutputBuffers>& o, int n) {
  for (int i = 0; i < n; i++) outs[i].data_size = o[i].data_size;
}

inline bool ToSelectionMode(int m, SelectionMode* out) {
  if (m < 0 || m > 3) return false;
  *out = static_cast<SelectionMode>(m);
  return true;
}
// sel may be null (*sv is then left as it is); false: bad mode
inline bool ToSelection(const gdv_selection_t* sel, const void* num_slots_device, SelectionView* sv) {
  if (!sel) return true;
  if (!ToSelectionMode(sel->mode, &sv->mode)) return false;
  sv->indices = sel->indices;
  sv->num_slots = sel->num_slots;
  sv->num_slots_device = num_slots_device;
  return true;
}

inline Configuration ToConfig(const gdv_config_t* config) {
  Configuration cfg;
  if (config) { cfg.optimize = config->optimize != 0; cfg.dump_ir = config->dump_ir != 0; }
  return cfg;
}

inline MemKind ToMemKind(int mem_kind) { return mem_kind == GDV_MEM_DEVICE ? MemKind::kDevice : MemKind::kHost; }

// One protobuf message of a *_make_from_proto call.
struct ProtoBytes {
  const void* bytes;
  int64_t len;
};
// The schema, then the condition and the expression list where the caller has a place for them; the first failure ends it.
inline Status DecodePlan(ProtoBytes schema_msg, ProtoBytes cond_msg, ProtoBytes exprs_msg, Schema* schema, ExpressionPtr* cond,
                         std::vector<ExpressionPtr>* exprs) {
  auto u8 = [](const void* p) { return static_cast<const uint8_t*>(p); };
  Status s = DecodeSchema(u8(schema_msg.bytes), static_cast<size_t>(schema_msg.len), schema);
  if (s.ok() && cond) s = DecodeCondition(u8(cond_msg.bytes), static_cast<size_t>(cond_msg.len), cond);
  if (s.ok() && exprs) s = DecodeExpressionList(u8(exprs_msg.bytes), static_cast<size_t>(exprs_msg.len), exprs);
  return s;
}

// The shared tail of the two stream-ceiling probes: `e` is what MeasureStreamCeiling returned.
inline int StreamCeilingResult(hipError_t e, int wg, int nt, int* workgroups_per_cu, int* nontemporal) {
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipErrorInvalidValue) return Fail(Status::Invalid("no ceiling kernel for this (reads, writes) shape"));
  if (workgroups_per_cu) *workgroups_per_cu = wg;
  if (nontemporal) *nontemporal = nt;
  return e == hipSuccess ? GDV_OK : Fail(Status::ExecutionError(hipGetErrorString(e)));
}

// Remembers the calling thread's selected device and selects it again on scope exit.
class DeviceScope {
 public:
  DeviceScope() : before_(Runtime::SelectedDevice()) {}
  ~DeviceScope() {
    if (restore_ && before_ >= 0) (void)Runtime::SelectDevice(before_);
  }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
  // (a refused selection returns to the caller without a second one: nothing is put back then)
  Status Select(int device) {
    Status st = Runtime::SelectDevice(device);
    if (!st.ok()) restore_ = false;
    return st;
  }

 private:
  const int before_;
  bool restore_ = true;
};

// gdv_projector_evaluate / _evaluate_selected and the single-device branch of _evaluate_host_sharded (gdv_c_api_eval.cc)
int ProjectorEvaluate(const gdv_projector_t* p, int64_t num_rows, const gdv_column_t* cols, int num_cols,
                      const gdv_selection_t* sel, const void* num_slots_device, gdv_out_column_t* outs, int num_outs,
                      int mem_kind, void* stream, uint32_t flags);

}  // namespace capi
}  // namespace gdv
