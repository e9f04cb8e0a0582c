// Tier 0 (round 6): expression trees -> the post-fix program gdv_tier0.hip interprets.  See gdv_tier0.h.
#include "gdv_tier0.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <map>

#include "gdv_registry.h"

namespace gdv {
namespace {

using namespace tier0;

static_assert(kBlockN == ArgLayout::kOffN && kBlockSel == ArgLayout::kOffSel && kBlockMask == ArgLayout::kOffMask &&
                  kBlockCounts == ArgLayout::kOffCounts && kBlockAux2 == ArgLayout::kOffAux2 && kBlockHeader == ArgLayout::kHeaderBytes &&
                  kBlockInStride == ArgLayout::kInStride && kBlockOutStride == ArgLayout::kOutStride,
              "the interpreter kernel reads the generated kernels' argument block at these offsets");

int KindOf(const DataType& t) {
  switch (t.id) {
    case gdv::kBool: return kTBool;
    case kInt8: return kTI8;
    case kUInt8: return kTU8;
    case kInt16: return kTI16;
    case kUInt16: return kTU16;
    case kInt32: case kDate32: case kTime32: return kTI32;
    case kUInt32: return kTU32;
    case kInt64: case kDate64: case kTimestamp: case kTime64: return kTI64;
    case kUInt64: return kTU64;
    case kFloat: return kTF32;
    case kDouble: return kTF64;
    default: return -1;
  }
}

// gdv_tier0_fns.inc as a table: symbol -> function id and operand count
struct FnEntry {
  const char* symbol;
  int args;
};
const FnEntry kFns[] = {
#define GDV_T0_F1(sym, R, A) {#sym, 1},
#define GDV_T0_F2(sym, R, A, B) {#sym, 2},
#include "gdv_tier0_fns.inc"
#undef GDV_T0_F1
#undef GDV_T0_F2
};
static_assert(sizeof(kFns) / sizeof(kFns[0]) == kNumFns, "one table entry per function id");

const char* const kGen1Names[] = {"negative", "abs", "bitwise_not"};
const char* const kGen2Names[] = {"greatest", "least", "bitwise_and", "bitwise_or", "bitwise_xor"};
const char* const kBoolTestNames[] = {"istrue", "isfalse", "isnottrue", "isnotfalse"};

int IndexOf(const char* const* names, int n, const std::string& name) {
  for (int i = 0; i < n; i++)
    if (name == names[i]) return i;
  return -1;
}

struct Builder {
  const Schema& schema;
  const KernelPlan& plan;
  Args* out;
  std::string why;
  int depth = 0, max_depth = 0, nlits = 0;

  bool Fail(const std::string& w) {
    if (why.empty()) why = w;
    return false;
  }
  bool Emit(int op, int a = 0, int b = 0, int c = 0) {
    if (out->ncode >= kMaxCode) return Fail("program longer than " + std::to_string(kMaxCode) + " instructions");
    if (op > kFilterOut) out->extended = 1;
    out->code[out->ncode++] = static_cast<uint32_t>(op) | (static_cast<uint32_t>(a) << 8) | (static_cast<uint32_t>(b) << 16) |
                              (static_cast<uint32_t>(c) << 24);
    return true;
  }
  bool Push() {
    if (++depth > kMaxDepth) return Fail("operand stack deeper than " + std::to_string(kMaxDepth));
    max_depth = std::max(max_depth, depth);
    return true;
  }
  bool Node(const gdv::Node& n) {
    const int tk = KindOf(n.return_type());
    if (tk < 0) return Fail("type " + n.return_type().ToString());
    switch (n.kind()) {
      case NodeKind::kField: {
        auto& f = static_cast<const FieldNode&>(n);
        int idx = -1;
        for (size_t i = 0; i < schema.size(); i++)
          if (schema[i].name == f.field().name) idx = static_cast<int>(i);
        int slot = -1;
        for (size_t k = 0; k < plan.input_fields.size(); k++)
          if (plan.input_fields[k] == idx) slot = static_cast<int>(k);
        if (idx < 0 || slot < 0 || slot > 255) return Fail("field " + f.field().name + " has no input slot");
        const int flags = (plan.input_needs_values[slot] ? 1 : 0) | (plan.input_needs_validity[slot] ? 2 : 0);
        return Push() && Emit(kLoad, slot, tk, flags);
      }
      case NodeKind::kLiteral: {
        auto& l = static_cast<const LiteralNode&>(n);
        if (nlits >= kMaxLits) return Fail("more than " + std::to_string(kMaxLits) + " literals");
        uint64_t v = l.value().lo;
        switch (tk) {  // the interpreter's canonical 64-bit slot
          case kTBool: v &= 1; break;
          case kTI8: v = static_cast<uint64_t>(static_cast<int64_t>(static_cast<int8_t>(v))); break;
          case kTU8: v &= 0xff; break;
          case kTI16: v = static_cast<uint64_t>(static_cast<int64_t>(static_cast<int16_t>(v))); break;
          case kTU16: v &= 0xffff; break;
          case kTI32: v = static_cast<uint64_t>(static_cast<int64_t>(static_cast<int32_t>(v))); break;
          case kTU32: case kTF32: v &= 0xffffffffull; break;
          default: break;
        }
        out->lits[nlits] = l.is_null() ? 0 : v;
        return Push() && Emit(kLit, nlits++, l.is_null() ? 1 : 0);
      }
      case NodeKind::kFunction: {
        auto& fn = static_cast<const FunctionNode&>(n);
        const std::string& name = fn.name();
        const size_t nargs = fn.children().size();
        std::vector<int> at(nargs);
        std::vector<DataType> params(nargs);
        for (size_t i = 0; i < nargs; i++) {
          params[i] = fn.children()[i]->return_type();
          at[i] = KindOf(params[i]);
          if (at[i] < 0) return Fail("type " + params[i].ToString());
        }
        auto args = [&]() {
          for (auto& c : fn.children())
            if (!Node(*c)) return false;
          return true;
        };
        // Resolved through the registry: the SYMBOL decides the instruction, so an alias (eq, modulo, pow, weekofyear,
        // isnumeric ...) and its target give the same one.
        const FunctionDef* def = FunctionRegistry::Get().Lookup(name, params);
        if (def == nullptr || KindOf(def->ret) != tk) return Fail("function " + name + ": no such signature");
        if (def->flags & kNeedsContext) return Fail("function " + name + " can raise");
        const std::string& symbol = def->symbol;
        if (symbol.compare(0, 4, "hash") == 0) return Fail("function " + name + " is a hash");
        std::string base = symbol;  // the symbol without its _<type> suffixes
        {
          std::string suffix;
          for (auto& p : def->params) suffix += "_" + p.Suffix();
          if (base.size() > suffix.size() && base.compare(base.size() - suffix.size(), suffix.size(), suffix) == 0)
            base.resize(base.size() - suffix.size());
        }
        const bool same2 = nargs == 2 && at[0] == at[1] && params[0].id == params[1].id;
        if ((base == "add" || base == "subtract" || base == "multiply") && same2 && at[0] == tk && tk != kTBool) {
          if (!args()) return false;
          depth--;
          return Emit(base == "add" ? kAdd : base == "subtract" ? kSub : kMul, 0, tk);
        }
        static const std::map<std::string, int> cmps = {{"equal", kEq}, {"not_equal", kNe}, {"less_than", kLt},
                                                        {"less_than_or_equal_to", kLe}, {"greater_than", kGt},
                                                        {"greater_than_or_equal_to", kGe}};
        auto cmp = cmps.find(base);
        if (cmp != cmps.end() && same2 && tk == kTBool) {
          if (!args()) return false;
          depth--;
          return Emit(kCmp, cmp->second, at[0]);
        }
        if (base == "not" && nargs == 1 && at[0] == kTBool && tk == kTBool) return args() && Emit(kNot);
        if ((symbol == "gdv_isnull" || symbol == "gdv_isnotnull") && nargs == 1 && tk == kTBool)
          return args() && Emit(symbol == "gdv_isnull" ? kIsNull : kIsNotNull);
        if ((symbol == "gdv_is_distinct_from" || symbol == "gdv_is_not_distinct_from") && same2 && tk == kTBool) {
          if (!args()) return false;
          depth--;
          return Emit(kDistinct, symbol == "gdv_is_not_distinct_from" ? 1 : 0, at[0]);
        }
        if (symbol == "gdv_nvl" && same2 && at[0] == tk) {
          if (!args()) return false;
          depth--;
          return Emit(kNvl, 0, tk);
        }
        const int bt = IndexOf(kBoolTestNames, 4, base);
        if (bt >= 0 && nargs == 1 && at[0] == kTBool && tk == kTBool) return args() && Emit(kBoolTest, bt);
        const bool i32_64 = tk == kTI32 || tk == kTI64, f32_64 = tk == kTF32 || tk == kTF64, u32_64 = tk == kTU32 || tk == kTU64;
        const int g1 = IndexOf(kGen1Names, 3, base);
        if (g1 >= 0 && nargs == 1 && at[0] == tk && !def->ret.is_decimal() &&
            (g1 == kBitNot ? (i32_64 || u32_64) : (i32_64 || f32_64)))
          return args() && Emit(kGen1, g1, tk);
        const int g2 = IndexOf(kGen2Names, 5, base);
        if (g2 >= 0 && same2 && at[0] == tk && (g2 >= kBitAnd ? (i32_64 || u32_64) : (i32_64 || f32_64))) {
          if (!args()) return false;
          depth--;
          return Emit(kGen2, g2, tk);
        }
        // numeric casts the registry holds (gdv_device_lib.hpp: castINT_int64, castBIGINT_int32 / _float32 / _float64,
        // castINT_float32 / _float64, castFLOAT4_int32 / _int64 / _float64, castFLOAT8_int32 / _int64 / _float32)
        if (nargs == 1) {
          const TypeId from = params[0].id, to = n.return_type().id;
          const bool ok = (base == "castBIGINT" && to == kInt64 && (from == kInt32 || from == kFloat || from == kDouble)) ||
                          (base == "castINT" && to == kInt32 && (from == kInt64 || from == kFloat || from == kDouble)) ||
                          (base == "castFLOAT4" && to == kFloat && (from == kInt32 || from == kInt64 || from == kDouble)) ||
                          (base == "castFLOAT8" && to == kDouble && (from == kInt32 || from == kInt64 || from == kFloat));
          if (ok) return args() && Emit(kCast, at[0], tk);
        }
        // everything else: a device-library function called by id
        for (int id = 0; id < kNumFns; id++) {
          if (symbol != kFns[id].symbol) continue;
          if (static_cast<size_t>(kFns[id].args) != nargs) break;
          if (!args()) return false;
          if (nargs == 2) depth--;
          return Emit(nargs == 1 ? kCall1 : kCall2, id & 0xff, id >> 8);
        }
        return Fail("function " + name);
      }
      case NodeKind::kIf: {
        auto& f = static_cast<const IfNode&>(n);
        if (KindOf(f.condition()->return_type()) != kTBool || KindOf(f.then_node()->return_type()) != tk ||
            KindOf(f.else_node()->return_type()) != tk)
          return Fail("if / else over mixed types");
        if (!Node(*f.condition()) || !Node(*f.then_node()) || !Node(*f.else_node())) return false;
        depth -= 2;
        return Emit(kIf);
      }
      case NodeKind::kBoolean: {
        auto& b = static_cast<const BooleanNode&>(n);
        if (b.children().empty()) return Fail("empty AND / OR");
        for (size_t i = 0; i < b.children().size(); i++) {
          if (KindOf(b.children()[i]->return_type()) != kTBool) return Fail("AND / OR over a non-boolean");
          if (!Node(*b.children()[i])) return false;
          if (i > 0) {
            depth--;
            if (!Emit(b.op() == BooleanNode::kAnd ? kAnd2 : kOr2)) return false;
          }
        }
        return true;
      }
      case NodeKind::kIn: {
        auto& in = static_cast<const InNode&>(n);
        const DataType& vt = in.value_type();
        const int vk = KindOf(vt);
        if (vk < 0 || vk != KindOf(in.eval()->return_type())) return Fail("IN over type " + vt.ToString());
        // the same sorted bit images the generated kernel compares on
        const std::vector<uint64_t> vals = InListBitImages(vt, in.values());
        if (!Node(*in.eval())) return false;
        // (checked after the evaluated child, which may have taken literal slots of its own)
        if (nlits + vals.size() > static_cast<size_t>(kMaxLits))
          return Fail("IN list of " + std::to_string(vals.size()) + " values does not fit the literal table (" +
                      std::to_string(kMaxLits) + " slots, " + std::to_string(nlits) + " taken)");
        const int first = nlits;
        for (uint64_t v : vals) out->lits[nlits++] = v;
        return Emit(kIn, vals.empty() ? 0 : first, static_cast<int>(vals.size()), vk);
      }
      default:
        return Fail("unknown node kind");
    }
  }
};

}  // namespace

bool BuildTier0Program(const Schema& schema, const std::vector<ExpressionPtr>& exprs, bool filter, const KernelPlan& plan,
                       tier0::Args* out, std::string* why) {
  std::memset(out, 0, sizeof(*out));
  Builder b{schema, plan, out, {}};
  auto fail = [&](const std::string& w) {
    if (why) *why = w.empty() ? b.why : w;
    return false;
  };
  if (plan.layout.total() > kMaxBlock) return fail("argument block of " + std::to_string(plan.layout.total()) + " bytes");
  if (plan.mode != SelectionMode::kNone && filter) return fail("selection-mode filter");
  if (plan.has_varlen_input || plan.has_varlen_output || plan.string_skeleton || plan.wave_tiles) return fail("var-len plan");
  if (plan.opts.rows_word) return fail("plan option rows_word (the second stage of a two-stage plan)");
  if (plan.opts.cast_x86_indefinite) return fail("plan option cast_x86_indefinite (GDV_CAST_X86_INDEFINITE)");
  if (filter ? exprs.size() != 1 : exprs.size() != plan.output_types.size()) return fail("expression count");
  out->n_in = plan.layout.n_in;
  out->filter = filter ? 1 : 0;
  out->subtiles = plan.opts.subtiles;
  out->selw = IndexWidth(plan.mode);
  for (size_t e = 0; e < exprs.size(); e++) {
    const Node& root = *exprs[e]->root();
    if (!b.Node(root)) return fail("");
    if (filter) {
      if (KindOf(root.return_type()) != kTBool) return fail("condition is not boolean");
      if (!b.Emit(kFilterOut)) return fail("");
    } else {
      const int tk = KindOf(exprs[e]->result().type);
      if (tk < 0 || tk != KindOf(root.return_type()) || e > 255) return fail("output type " + exprs[e]->result().type.ToString());
      if (!b.Emit(kOut, static_cast<int>(e), tk)) return fail("");
    }
    b.depth--;
  }
  return true;
}


std::string DescribeTier0Program(const tier0::Args& prog) {
  static const char* kinds[] = {"bool", "int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64", "float32", "float64"};
  static const char* cmps[] = {"eq", "ne", "lt", "le", "gt", "ge"};
  std::string out;
  if (prog.selw != 0) out += "select uint" + std::to_string(prog.selw * 8) + "\n";
  for (int pc = 0; pc < prog.ncode; pc++) {
    const uint32_t ins = prog.code[pc];
    const int op = ins & 0xff, a = (ins >> 8) & 0xff, b = (ins >> 16) & 0xff, c = (ins >> 24) & 0xff;
    auto kind = [&](int k) { return std::string(k >= 0 && k <= tier0::kTF64 ? kinds[k] : "?"); };
    switch (op) {
      case tier0::kLoad: out += "load in" + std::to_string(a) + " " + kind(b) + ((c & 1) ? "" : " (values unused)") + ((c & 2) ? "" : " (no validity)"); break;
      case tier0::kLit: out += "lit #" + std::to_string(a) + (b ? " null" : " = 0x" + [&] { char t[24]; snprintf(t, sizeof t, "%llx", static_cast<unsigned long long>(prog.lits[a])); return std::string(t); }()); break;
      case tier0::kAdd: out += "add " + kind(b); break;
      case tier0::kSub: out += "subtract " + kind(b); break;
      case tier0::kMul: out += "multiply " + kind(b); break;
      case tier0::kCmp: out += std::string("compare ") + (a <= tier0::kGe ? cmps[a] : "?") + " " + kind(b); break;
      case tier0::kCast: out += "cast " + kind(a) + " -> " + kind(b); break;
      case tier0::kNot: out += "not"; break;
      case tier0::kIsNull: out += "isnull"; break;
      case tier0::kIsNotNull: out += "isnotnull"; break;
      case tier0::kAnd2: out += "and"; break;
      case tier0::kOr2: out += "or"; break;
      case tier0::kIf: out += "if"; break;
      case tier0::kOut: out += "out" + std::to_string(a) + " " + kind(b); break;
      case tier0::kFilterOut: out += "filter"; break;
      case tier0::kCall1: case tier0::kCall2: {
        const int id = a | (b << 8);
        out += std::string("call ") + (id < tier0::kNumFns ? kFns[id].symbol : "?");
        break;
      }
      case tier0::kGen1: out += std::string(a < 3 ? kGen1Names[a] : "?") + " " + kind(b); break;
      case tier0::kGen2: out += std::string(a < 5 ? kGen2Names[a] : "?") + " " + kind(b); break;
      case tier0::kBoolTest: out += a < 4 ? kBoolTestNames[a] : "?"; break;
      case tier0::kDistinct: out += std::string(a ? "is_not_distinct_from " : "is_distinct_from ") + kind(b); break;
      case tier0::kNvl: out += "nvl " + kind(b); break;
      case tier0::kIn:
        out += "in " + kind(c) + (b == 0 ? std::string(" (no values)") : " #" + std::to_string(a) + "..#" + std::to_string(a + b - 1));
        break;
      default: out += "?"; break;
    }
    out += "\n";
  }
  return out;
}

static std::atomic<int64_t> g_tier0_launches{0};
int64_t Tier0Launches() { return g_tier0_launches.load(std::memory_order_relaxed); }
void CountTier0Launch() { g_tier0_launches.fetch_add(1, std::memory_order_relaxed); }

}  // namespace gdv
