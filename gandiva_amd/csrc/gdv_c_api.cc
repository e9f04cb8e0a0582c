// extern "C" boundary (include/gandiva_amd.h) over the C++ core: last error, builders, registry, build support.
#include "gdv_c_api_internal.h"

#include "gdv_libtag.h"
#include "gdv_regex.h"

using namespace gdv;
using namespace gdv::capi;

namespace {
thread_local std::string g_last_error;
}  // namespace
void gdv::capi::SetLastError(std::string msg) { g_last_error = std::move(msg); }

extern "C" {

const char* gdv_last_error(void) { return g_last_error.c_str(); }
const char* gdv_version(void) { return "gandiva_amd 0.1.0 (gfx950)"; }
void gdv_free_string(char* s) { free(s); }

// ---------------------------------------------------------------- schema
gdv_schema_t* gdv_schema_new(void) { return new gdv_schema(); }
int gdv_schema_add_field(gdv_schema_t* schema, const char* name, gdv_type_t type, int nullable) {
  return Guarded([&]() -> int {
  DataType t;
  if (!schema || !name) return Fail(Status::Invalid("null schema or field name"));
  if (!ToType(type, &t)) return Fail(Status::Invalid("unsupported type id " + std::to_string(type.id)));
  schema->fields.push_back(Field{name, t, nullable != 0});
  return GDV_OK;
  });
}
int gdv_schema_num_fields(const gdv_schema_t* schema) {
  return schema ? static_cast<int>(schema->fields.size()) : 0;
}
void gdv_schema_free(gdv_schema_t* schema) { delete schema; }

// ---------------------------------------------------------------- nodes
gdv_node_t* gdv_node_field(const char* name, gdv_type_t type) {
  return GuardedPtr([&]() -> gdv_node_t* {
  DataType t;
  if (!name) return FailPtr<gdv_node_t>("field name is null");
  if (!ToType(type, &t)) return FailPtr<gdv_node_t>("unsupported type id");
  return new gdv_node{std::make_shared<FieldNode>(Field{name, t, true})};
  });
}

gdv_node_t* gdv_node_literal(gdv_type_t type, const void* value, int is_null) {
  return GuardedPtr([&]() -> gdv_node_t* {
  DataType t;
  if (!ToType(type, &t)) return FailPtr<gdv_node_t>("unsupported type id");
  if (t.is_varlen()) return FailPtr<gdv_node_t>("use gdv_node_literal_bytes for var-len types");
  Literal lit;
  lit.is_null = is_null != 0;
  if (!lit.is_null) {
    if (!value) return FailPtr<gdv_node_t>("literal value is null");
    int w = t.id == kBool ? 1 : t.byte_width();
    unsigned char raw[16] = {0};
    std::memcpy(raw, value, w);
    std::memcpy(&lit.lo, raw, 8);
    std::memcpy(&lit.hi, raw + 8, 8);
    if (t.id == kBool) lit.lo = raw[0] ? 1 : 0;
    // sign-extend narrow signed integers so the payload is the value's int64 image
    if (t.id == kInt8) lit.lo = static_cast<uint64_t>(static_cast<int64_t>(static_cast<int8_t>(raw[0])));
    if (t.id == kInt16) { int16_t v; std::memcpy(&v, raw, 2); lit.lo = static_cast<uint64_t>(static_cast<int64_t>(v)); }
    if (t.id == kInt32 || t.id == kDate32 || t.id == kTime32) {
      int32_t v; std::memcpy(&v, raw, 4); lit.lo = static_cast<uint64_t>(static_cast<int64_t>(v));
    }
  }
  return new gdv_node{std::make_shared<LiteralNode>(t, lit)};
  });
}

gdv_node_t* gdv_node_literal_bytes(gdv_type_t type, const char* data, int64_t len, int is_null) {
  return GuardedPtr([&]() -> gdv_node_t* {
  DataType t;
  if (!ToType(type, &t) || !t.is_varlen()) return FailPtr<gdv_node_t>("type must be string or binary");
  Literal lit;
  lit.is_null = is_null != 0;
  if (!lit.is_null) {
    if (len < 0 || (len > 0 && !data)) return FailPtr<gdv_node_t>("bad literal bytes");
    lit.bytes.assign(data ? data : "", static_cast<size_t>(len));
  }
  return new gdv_node{std::make_shared<LiteralNode>(t, lit)};
  });
}

gdv_node_t* gdv_node_function(const char* name, gdv_node_t* const* children, int num_children,
                              gdv_type_t return_type) {
  return GuardedPtr([&]() -> gdv_node_t* {
  DataType t;
  NodeVector kids;
  if (!name) return FailPtr<gdv_node_t>("function name is null");
  if (!ToType(return_type, &t)) return FailPtr<gdv_node_t>("unsupported return type id");
  if (!CollectChildren(children, num_children, &kids)) return FailPtr<gdv_node_t>("null child node");
  return new gdv_node{MakeFunctionNode(name, std::move(kids), t)};
  });
}

gdv_node_t* gdv_node_if(gdv_node_t* c, gdv_node_t* t, gdv_node_t* e, gdv_type_t return_type) {
  return GuardedPtr([&]() -> gdv_node_t* {
  DataType rt;
  if (!c || !t || !e || !c->node || !t->node || !e->node) return FailPtr<gdv_node_t>("null child node");
  if (!ToType(return_type, &rt)) return FailPtr<gdv_node_t>("unsupported return type id");
  return new gdv_node{std::make_shared<IfNode>(c->node, t->node, e->node, rt)};
  });
}

gdv_node_t* gdv_node_and(gdv_node_t* const* children, int n) {
  return GuardedPtr([&]() -> gdv_node_t* {
  NodeVector kids;
  if (!CollectChildren(children, n, &kids)) return FailPtr<gdv_node_t>("null child node");
  return new gdv_node{std::make_shared<BooleanNode>(BooleanNode::kAnd, std::move(kids))};
  });
}

gdv_node_t* gdv_node_or(gdv_node_t* const* children, int n) {
  return GuardedPtr([&]() -> gdv_node_t* {
  NodeVector kids;
  if (!CollectChildren(children, n, &kids)) return FailPtr<gdv_node_t>("null child node");
  return new gdv_node{std::make_shared<BooleanNode>(BooleanNode::kOr, std::move(kids))};
  });
}

gdv_node_t* gdv_node_in(gdv_node_t* node, gdv_type_t value_type, const void* values, int n) {
  return GuardedPtr([&]() -> gdv_node_t* {
  DataType t;
  if (!node || !node->node) return FailPtr<gdv_node_t>("null child node");
  if (!ToType(value_type, &t) || t.is_varlen()) return FailPtr<gdv_node_t>("bad IN value type");
  if (n < 0 || (n > 0 && !values)) return FailPtr<gdv_node_t>("bad IN values");
  const int w = t.byte_width();
  if (w == 0) return FailPtr<gdv_node_t>("IN over this type is not supported");
  std::vector<Literal> lits(n);
  const char* p = static_cast<const char*>(values);
  for (int i = 0; i < n; i++) {
    unsigned char raw[16] = {0};
    std::memcpy(raw, p + static_cast<size_t>(i) * w, w);
    std::memcpy(&lits[i].lo, raw, 8);
    std::memcpy(&lits[i].hi, raw + 8, 8);
  }
  return new gdv_node{std::make_shared<InNode>(node->node, t, std::move(lits))};
  });
}

gdv_node_t* gdv_node_in_bytes(gdv_node_t* node, gdv_type_t value_type, const char* const* values,
                              const int64_t* lengths, int n) {
  return GuardedPtr([&]() -> gdv_node_t* {
  DataType t;
  if (!node || !node->node) return FailPtr<gdv_node_t>("null child node");
  if (!ToType(value_type, &t) || !t.is_varlen()) return FailPtr<gdv_node_t>("bad IN value type");
  if (n < 0 || (n > 0 && (!values || !lengths))) return FailPtr<gdv_node_t>("bad IN values");
  std::vector<Literal> lits(n);
  for (int i = 0; i < n; i++) lits[i].bytes.assign(values[i] ? values[i] : "", static_cast<size_t>(lengths[i]));
  return new gdv_node{std::make_shared<InNode>(node->node, t, std::move(lits))};
  });
}

char* gdv_node_to_string(const gdv_node_t* node) {
  return GuardedPtr([&]() -> char* {
  return node && node->node ? DupString(node->node->ToString()) : nullptr;
  });
}
gdv_type_t gdv_node_return_type(const gdv_node_t* node) {
  return node && node->node ? FromType(node->node->return_type()) : gdv_type_t{0, 0, 0};
}
void gdv_node_free(gdv_node_t* node) { delete node; }

gdv_expression_t* gdv_expression_new(gdv_node_t* root, const char* result_name, gdv_type_t rt) {
  return GuardedPtr([&]() -> gdv_expression_t* {
  DataType t;
  if (!root || !root->node) return FailPtr<gdv_expression_t>("root node is null");
  if (!result_name) return FailPtr<gdv_expression_t>("result field is null");
  if (!ToType(rt, &t)) return FailPtr<gdv_expression_t>("unsupported result type id");
  return new gdv_expression{std::make_shared<Expression>(root->node, Field{result_name, t, true})};
  });
}
gdv_expression_t* gdv_condition_new(gdv_node_t* root) {
  return GuardedPtr([&]() -> gdv_expression_t* {
  if (!root || !root->node) return FailPtr<gdv_expression_t>("root node is null");
  return new gdv_expression{std::make_shared<Expression>(root->node, Field{"cond", boolean(), true})};
  });
}
char* gdv_expression_to_string(const gdv_expression_t* e) {
  return GuardedPtr([&]() -> char* {
  return e && e->expr ? DupString(e->expr->ToString()) : nullptr;
  });
}
gdv_type_t gdv_expression_result_type(const gdv_expression_t* e) {
  return e && e->expr ? FromType(e->expr->result().type) : gdv_type_t{0, 0, 0};
}
void gdv_expression_free(gdv_expression_t* e) { delete e; }

// ---------------------------------------------------------------- registry
int gdv_registry_size(void) { return static_cast<int>(FunctionRegistry::Get().all().size()); }
int gdv_registry_get(int index, const char** name, gdv_type_t* return_type, gdv_type_t* params,
                     int max_params, int* num_params) {
  return Guarded([&]() -> int {
  auto& all = FunctionRegistry::Get().all();
  if (index < 0 || index >= static_cast<int>(all.size())) return Fail(Status::Invalid("index out of range"));
  const FunctionDef& d = all[index];
  if (name) *name = d.name.c_str();
  if (return_type) *return_type = FromType(d.ret);
  if (num_params) *num_params = static_cast<int>(d.params.size());
  for (int i = 0; params && i < max_params && i < static_cast<int>(d.params.size()); i++)
    params[i] = FromType(d.params[i]);
  return GDV_OK;
  });
}

// ---------------------------------------------------------------- build support
char* gdv_tier0_program(const gdv_schema_t* schema, gdv_expression_t* const* exprs, int num_exprs, int is_condition) {
  return GuardedPtr([&]() -> char* {
    if (!schema || !exprs || num_exprs < 1) return FailPtr<char>("schema and expressions are required");
    std::vector<ExpressionPtr> v;
    if (!CollectExprs(exprs, num_exprs, &v, /*require_tree=*/false)) return FailPtr<char>("null expression");
    std::string text;
    Status st = Tier0Describe(schema->fields, v, is_condition != 0, &text);
    if (!st.ok()) {
      Fail(st);
      return nullptr;
    }
    return DupString(text);
  });
}
char* gdv_tier0_program_selection(const gdv_schema_t* schema, gdv_expression_t* const* exprs, int num_exprs, int selection_mode) {
  return GuardedPtr([&]() -> char* {
    if (!schema || !exprs || num_exprs < 1) return FailPtr<char>("schema and expressions are required");
    if (selection_mode < 0 || selection_mode > 3) return FailPtr<char>("selection mode must be 0 (none), 1 (uint16), 2 (uint32) or 3 (uint64)");
    std::vector<ExpressionPtr> v;
    if (!CollectExprs(exprs, num_exprs, &v, /*require_tree=*/false)) return FailPtr<char>("null expression");
    std::string text;
    Status st = Tier0Describe(schema->fields, v, /*is_condition=*/false, &text, static_cast<SelectionMode>(selection_mode));
    if (!st.ok()) {
      Fail(st);
      return nullptr;
    }
    return DupString(text);
  });
}
int64_t gdv_tier0_launches(void) { return Tier0Launches(); }
void gdv_shutdown(void) { Runtime::ShutdownBackgroundCompiler(); }

int gdv_precompile_projector(const gdv_schema_t* schema, gdv_expression_t* const* exprs,
                             int num_exprs, int selection_mode) {
  return Guarded([&]() -> int {
  if (!schema) return Fail(Status::Invalid("null schema"));
  std::vector<ExpressionPtr> ex;
  if (!CollectExprs(exprs, num_exprs, &ex)) return Fail(Status::Invalid("null expression"));
  SelectionMode mode;
  if (!ToSelectionMode(selection_mode, &mode)) return Fail(Status::Invalid("bad selection mode"));
  return Check(PrecompileProjector(schema->fields, ex, mode));
  });
}
int gdv_precompile_filter_project(const gdv_schema_t* schema, gdv_expression_t* condition, gdv_expression_t* const* exprs,
                                  int num_exprs, int index_mode) {
  return Guarded([&]() -> int {
  if (!schema || !condition || !condition->expr || !exprs || num_exprs <= 0) return Fail(Status::Invalid("null argument"));
  SelectionMode mode;
  if (!ToSelectionMode(index_mode, &mode)) return Fail(Status::Invalid("bad selection mode"));
  std::vector<ExpressionPtr> ex;
  if (!CollectExprs(exprs, num_exprs, &ex)) return Fail(Status::Invalid("Expression cannot be null"));
  return Check(PrecompileFilterProject(schema->fields, condition->expr, ex, mode));
  });
}
char* gdv_filter_project_plan_text(const gdv_schema_t* schema, gdv_expression_t* condition, gdv_expression_t* const* exprs,
                                   int num_exprs, int index_mode, int shape, int request_small, int compile) {
  char* out = nullptr;
  (void)Guarded([&]() -> int {
  if (!schema || !condition || !condition->expr || !exprs || num_exprs <= 0) return Fail(Status::Invalid("null argument"));
  SelectionMode mode;
  if (!ToSelectionMode(index_mode, &mode)) return Fail(Status::Invalid("bad selection mode"));
  std::vector<ExpressionPtr> ex;
  if (!CollectExprs(exprs, num_exprs, &ex)) return Fail(Status::Invalid("Expression cannot be null"));
  std::string text;
  Status st = FilterProjectPlanText(schema->fields, condition->expr, ex, mode, shape, request_small != 0, compile != 0, &text);
  if (!st.ok()) return Fail(st);
  out = DupString(text);
  return GDV_OK;
  });
  return out;
}
int gdv_precompile_filter(const gdv_schema_t* schema, gdv_expression_t* condition) {
  return Guarded([&]() -> int {
  if (!schema || !condition || !condition->expr) return Fail(Status::Invalid("null argument"));
  return Check(PrecompileFilter(schema->fields, condition->expr));
  });
}

int gdv_compile_regex(const char* pattern, int64_t pattern_len, uint8_t* table) {
  return Guarded([&]() -> int {
  if (!pattern || pattern_len < 0 || !table) return Fail(Status::Invalid("null argument"));
  std::string bytes;
  Status st = CompileRegex(std::string(pattern, static_cast<size_t>(pattern_len)), &bytes);
  if (!st.ok()) return Fail(st);
  std::memcpy(table, bytes.data(), bytes.size());
  return 0;
  });
}

int gdv_compile_regex_extract(const char* pattern, int64_t pattern_len, int32_t group, uint8_t* table, int64_t cap, int64_t* n) {
  return Guarded([&]() -> int {
  if (!pattern || pattern_len < 0 || !table || !n) return Fail(Status::Invalid("null argument"));
  std::string bytes;
  Status st = CompileRegexExtract(std::string(pattern, static_cast<size_t>(pattern_len)), group, &bytes);
  if (!st.ok()) return Fail(st);
  if (static_cast<int64_t>(bytes.size()) > cap) return Fail(Status::Invalid("table buffer too small"));
  std::memcpy(table, bytes.data(), bytes.size());
  *n = static_cast<int64_t>(bytes.size());
  return 0;
  });
}

int gdv_compile_date_format(const char* pattern, int64_t pattern_len, uint8_t* ops, int64_t cap, int64_t* n) {
  return Guarded([&]() -> int {
  if (!pattern || pattern_len < 0 || !ops || !n) return Fail(Status::Invalid("null argument"));
  std::string bytes;
  Status st = CompileDateFormat(std::string(pattern, static_cast<size_t>(pattern_len)), &bytes);
  if (!st.ok()) return Fail(st);
  if (static_cast<int64_t>(bytes.size()) > cap) return Fail(Status::Invalid("ops buffer too small"));
  std::memcpy(ops, bytes.data(), bytes.size());
  *n = static_cast<int64_t>(bytes.size());
  return 0;
  });
}

// The part of a kernel's name that comes from the device function library: the hash of the library
// items `kernel_text` reaches (gdv_libtag.h).  library_source NULL = the embedded library.
char* gdv_kernel_library_tag(const char* library_source, const char* kernel_text) {
  if (kernel_text == nullptr) return nullptr;
  std::string tag;
  if (library_source == nullptr) {
    tag = LibraryIndex::Embedded().TagFor(kernel_text);
  } else {
    tag = LibraryIndex(library_source).TagFor(kernel_text);
  }
  return DupString(tag);
}
char* gdv_kernel_library_items(const char* library_source, const char* kernel_text) {
  if (kernel_text == nullptr) return nullptr;
  std::vector<std::string> names = library_source == nullptr
                                       ? LibraryIndex::Embedded().ReachedFrom(kernel_text)
                                       : LibraryIndex(library_source).ReachedFrom(kernel_text);
  std::string out;
  for (auto& n : names) out += n + "\n";
  return DupString(out);
}
const char* gdv_device_library_source(void) { return gdv_device_lib_src; }

}  // extern "C"
