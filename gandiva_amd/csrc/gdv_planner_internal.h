// What the units of the planner share (gdv_planner.h is the public interface; nothing outside the planner includes this).
// DESIGN.md's module map says which unit holds what.
#pragma once
#include "gdv_planner.h"

#include <cstdio>
#include <sstream>

namespace gdv::planner {

// Ablation branches (GDV_ABL masks, set through GDV_RTC_OPT=-DGDV_ABL=<mask>) are experiment
// scaffolding: they are emitted only into kernels planned with GDV_ABLATION=1 in the environment of
// Make.  A product kernel's text does not contain them (round-3 verdict: 27 sites in every kernel).
extern thread_local bool tl_ablation;  // (defined in gdv_planner.cc)
struct AblationScope {
  bool prev;
  explicit AblationScope(bool on) : prev(tl_ablation) { tl_ablation = on; }
  ~AblationScope() { tl_ablation = prev; }
};
inline std::string AblNot(int bit) { return tl_ablation ? "!(GDV_ABL & " + std::to_string(bit) + ") && " : ""; }
inline std::string AblAnd(int bit) { return tl_ablation ? " && !(GDV_ABL & " + std::to_string(bit) + ")" : ""; }
inline std::string AblIf(int bit) { return tl_ablation ? "if (!(GDV_ABL & " + std::to_string(bit) + ")) " : ""; }
inline std::string AblSel(int bit, const std::string& on, const std::string& off) {
  return tl_ablation ? "((GDV_ABL & " + std::to_string(bit) + ") ? " + on + " : " + off + ")" : off;
}
inline std::string AblDefine() {
  return tl_ablation ? "#ifndef GDV_ABL\n#define GDV_ABL 0  // ablation mask for experiments; 0 = the product\n#endif\n" : "";
}

bool ResolveFunction(const FunctionNode& n, const FunctionDef** def, DataType* ret);  // gdv_plan_validate.cc

inline std::string Hex64(uint64_t v) {
  char buf[32];
  snprintf(buf, sizeof(buf), "0x%llxull", static_cast<unsigned long long>(v));
  return buf;
}

// A value inside the generated row body: a C++ expression plus its validity, split the way
// the reference's ValueValidityPair splits it — the set of input columns whose validity
// words intersect, and an optional per-lane predicate for value-dependent validity
// (if/else, SQL three-valued AND/OR, functions that produce nulls themselves).
struct Val {
  std::string v;
  DataType type;
  std::set<int> vcols;
  std::string vlane;
  // concat results are not a view: they are the list of their argument views, written one
  // after the other by the output copy (piece expression, per-lane "piece present"
  // predicate or "" for always).  Only an output expression or another concat can take one.
  std::vector<std::pair<std::string, std::string>> pieces;
  // A string value that IS the row of input slot `col_slot` (whole, unsliced), read through the
  // static byte map `col_map` (0 none, 1 upper, 2 lower): candidates for the byte-parallel
  // paths (sweep-answered '%needle%', flat output copy).  -1: anything else.
  int col_slot = -1;
  int col_map = 0;
  // reverse(), replace() and castVARCHAR(integer) results are not readable views (GDV_MAP_REVERSE /
  // GDV_MAP_REPLACE / GDV_MAP_DIGITS): like concat results, only the output copy or a concat can
  // take them (anything else gets them through a first stage, StageMaterialisedValues)
  bool opaque = false;
  bool never_null() const { return vcols.empty() && vlane.empty(); }
};

// '%needle%' predicate answered by the byte sweep of input slot `slot` (bytes read through `map`)
struct ContainsHook {
  int slot;
  int map;
  std::string needle;
};

// One var-len output of a projector: its row value as 1+ pieces (views written back to back),
// each with the name of the per-sub-tile register array holding it.
struct VarlenOut {
  int e = 0;                      // output index
  int flat_slot = -1;             // >= 0: the row is input slot flat_slot's whole row ...
  int flat_map = 0;               // ... read through this byte map
  int window = -1;                // >= 0: LDS staging window of this output (non-flat outputs)
  int segment = -1;               // wave shape: index of this output's array of wave-tile totals / bases
  bool reads_views = false;       // staged output whose copies read readable views (candidates for the LDS mirror)
};

class CodeGen {
 public:
  CodeGen(const Schema& schema, SelectionMode mode, const CodegenOptions& opts)
      : schema_(schema), sel_mode_(mode), opts_(opts) {}

  bool selection() const { return sel_mode_ != SelectionMode::kNone; }

  Status Gen(const Node& node, const std::string& active, Val* out);
  // specially planned functions, one emitter each (gdv_codegen_functions.cc); GenCall: everything else (the registry's symbol)
  using FnArgs = std::vector<Val>;
  Status GenRegexpLike(const FunctionNode& fn, FnArgs& args, const std::string& active, Val* out);
  Status GenRegexpExtract(const FunctionNode& fn, FnArgs& args, const std::string& active, Val* out);
  Status GenReplace(const FunctionNode& fn, FnArgs& args, const std::string& active, Val* out);
  Status GenTranslate(const FunctionNode& fn, FnArgs& args, const std::string& active, Val* out);
  Status GenUtf8Case(const FunctionNode& fn, FnArgs& args, const std::string& active, Val* out);
  Status GenMask(const FunctionNode& fn, FnArgs& args, const std::string& active, Val* out);
  Status GenPad(const FunctionNode& fn, FnArgs& args, const std::string& active, Val* out);
  Status GenConcat(const FunctionNode& fn, FnArgs& args, const std::string& active, Val* out);
  Status GenToDate(const FunctionNode& fn, FnArgs& args, const std::string& active, Val* out);
  Status GenLike(const FunctionNode& fn, FnArgs& args, const std::string& active, Val* out);
  Status GenCall(const FunctionNode& fn, const FunctionDef& def, FnArgs& args, const std::string& active, Val* out);

  // ---- emission helpers
  std::string Tmp(const std::string& ctype, const std::string& rhs) {
    std::string key = ctype + "|" + rhs;
    auto it = cse_.find(key);
    if (it != cse_.end()) return it->second;
    std::string name = "t" + std::to_string(next_tmp_++);
    body_ << "      const " << ctype << " " << name << " = " << rhs << ";\n";
    cse_[key] = name;
    return name;
  }
  void Stmt(const std::string& s) { body_ << "      " << s << "\n"; }

  // conjunction of per-lane predicates; "" stands for "always true"
  static std::string AndExpr(const std::string& a, const std::string& b) {
    if (a.empty() || a == "true") return (b == "true") ? "" : b;
    if (b.empty() || b == "true") return a;
    return "(" + a + " && " + b + ")";
  }

  // same, spelled out: never the empty string (for use as a full expression)
  static std::string AndFull(const std::string& a, const std::string& b) {
    std::string r = AndExpr(a, b);
    return r.empty() ? "true" : r;
  }

  // per-lane validity of a value ("true" when it can never be null)
  std::string LaneValid(const Val& val);

  // wave-uniform AND of the validity words of a set of input columns (row mode only)
  std::string WordExpr(const std::set<int>& cols);

  // ---- literals are kernel ARGUMENTS, not source text (round 2): `a > 499` and `a > 500`, or
  // like '%spark%' and like '%flink%', share one compiled kernel; only the shape (types, list
  // sizes, pattern form and needle length) is compiled in.
  // Fixed-width literal -> 8-byte slot of gdv_args::lit (decimal128: two slots, low word first)
  // (slots are never shared by VALUE — the code must not depend on which constants happen to be
  // equal — only by node identity: a literal node used in several places is one slot, so common
  // sub-expressions built from shared nodes still merge)
  int LitSlot(uint64_t v) {
    lits_.push_back(v);
    return static_cast<int>(lits_.size()) - 1;
  }
  std::string LiteralExpr(const DataType& t, const Literal& v, const void* node) {
    auto it = lit_of_node_.find(node);
    if (it != lit_of_node_.end()) return it->second;
    std::string e = LiteralExprNew(t, v);
    lit_of_node_[node] = e;
    return e;
  }
  static std::string InlineLiteral(const DataType& t, const Literal& v);
  std::string LiteralExprNew(const DataType& t, const Literal& v);
  // bytes -> the plan's constant block (device memory, bound through gdv_args::aux0); returns a
  // pointer expression.  Every table starts 16-byte aligned and is readable 8 bytes past its end.
  std::string ByteTable(const std::string& bytes, const char* ctype = "gdv_uint8");
  std::string StringConstant(const std::string& bytes);
  // SQL LIKE pattern -> (literal bytes, token kinds); `escape` < 0 means no escape character
  static Status CompileLike(const std::string& pat, int escape, std::string* bytes, std::string* kinds);

  // input slots of every var-len field below `node`
  std::set<int> StringSlotsOf(const Node& node);

  int SlotFor(const FieldNode& f, bool values, bool validity);

  const Schema& schema_;
  SelectionMode sel_mode_;
  CodegenOptions opts_;
  int compact_from_ = 0x7fffffff;  // schema fields from this index on are compact temporaries (selection mode)
  bool no_hooks_ = false;          // pre-pass kernels have no byte sweep: '%needle%' takes the per-row search
  // Wave kernels, round 4: false = the OPTIMISTIC variant (views of swept columns carry GDV_STR_ASCII as
  // a compile-time fact; a byte >= 0x80 raises NOTASCII); true = the EXACT variant the host re-runs such
  // a batch on: the flag is what the byte sweep of the (sub-)tile found, in the pre-pass and in the main
  // kernel alike, and a tile that did hold a byte >= 0x80 reports GDV_ERR_SAWUTF8 (so the host knows
  // when a later batch may go back to the optimistic kernels).
  bool exact_ascii_ = false;
  // selection-mode wave main kernel (round 5): the pre-pass took its lengths from the offsets under the ASCII
  // assumption; the rows, which read their bytes here anyway, verify it (NOTASCII -> the general kernel)
  bool sel_ascii_check_ = false;
  std::set<int> row_ascii_slots_;  // exact variant: inputs whose views take a PER-ROW flag (gdv_with_lead)
  bool bake_needles_ = false;      // wave kernels: '%needle%' bytes are immediates of the kernel text (NeedleConstants)
  bool unroll_rows_ = false;       // the row loop of this kernel is unrolled (small bodies that index registers by u)
  // ... and their lead-byte mask from the sweep's continuation bitmap: LDS bitmap index (behind the hooks' bitmaps)
  int CbIndex(int slot) {
    int j = 0;
    for (int k : ascii_slots_) { if (k == slot) return static_cast<int>(contains_hooks_.size()) + j; j++; }
    return -1;
  }
  int mirror_slot_ = -1;           // wave kernels: the var-len input whose sub-tile spans are swept one at a time
                                   // (main kernel: and mirrored in LDS)
  bool replace_hits_ = false;      // wave kernels: replace() over a whole column row may be answered by the sweep
  int replace_hook_ = -1;          // ... the hook (match bitmap) that does
  bool translate_ = false;         // a translate() value is copied: the plan's copies take the *_ext entry points
  bool datetime_ = false;          // a castVARCHAR of a date / time is copied: ... the *_dt entry points
  bool encode_ = false;            // a hex / unhex / base64 / unbase64 value is copied: ... the *_enc entry points
  // the output copy of a var-len value (the *_ext entry: translate values, *_dt: dates and times, *_enc: hex / base64 and
  // their inverses; only plans that hold one use it)
  // (a plan that holds an upper / lower value of GDV_UTF8_CASE=1 wraps whichever entry it is: GDV_STR_COPY / GDV_STAGE_COPY
  // are macros of the kernel's own text then, defined by the skeleton through WrapCopy)
  bool utf8_case_ = false;
  std::map<int, std::string> case_tables_;  // direction (1 upper, 2 lower) -> its table in the constant block
  // (a plan that holds a mask / mask_*_n value wraps the entry the same way, with GDV_COPY_MASK; a plan that holds both nests them)
  bool mask_ = false;
  std::string CopyFn() const { return utf8_case_ || mask_ ? "GDV_STR_COPY" : StageCopyFn("gdv_str_copy"); }
  std::string WrapCopy(const std::string& call) const {
    const std::string inner = utf8_case_ ? "GDV_COPY_UTF8CASE(dst, v, " + call + ")" : call;
    return mask_ ? "GDV_COPY_MASK(dst, v, " + inner + ")" : inner;
  }
  std::string StrCopyDefine() const {
    return utf8_case_ || mask_ ? "#define GDV_STR_COPY(dst, v) " + WrapCopy(StageCopyFn("gdv_str_copy") + "(dst, v)") + "\n" : "";
  }
  std::string StageCopyFn(const std::string& base) const {
    return base + (translate_ ? "_ext" : "") + (datetime_ ? "_dt" : "") + (encode_ ? "_enc" : "");
  }
  std::ostringstream body_;
  std::map<std::string, std::string> cse_;
  int next_tmp_ = 0;
  std::map<int, int> slot_of_field_;
  std::vector<int> input_fields_;
  std::vector<bool> needs_values_, needs_validity_;
  bool can_raise_ = false;
  std::vector<uint64_t> lits_;        // gdv_args::lit
  std::map<const void*, std::string> lit_of_node_;
  std::string blob_;                  // constant block: string literals, patterns, IN tables
  // string plans
  std::vector<ContainsHook> contains_hooks_;
  std::vector<std::string> hook_tables_;  // needle bytes in the constant block
  std::set<int> ascii_slots_;     // input slots whose tile-wide ASCII flag some function consults
  std::vector<VarlenOut> varlen_outs_;
  int HookFor(int slot, int map, const std::string& needle);
};

// what the planner knows about a function beyond its registry entry (the table: gdv_codegen_functions.cc)
enum FnTrait : unsigned {
  kFnOpaque = 1,     // the value is not a readable view: only the output copy or a concat can take it
  kFnDigest = 2,     // sha / md5: opaque too (hash*: only the var-len ones, by their return type)
  kFnAsciiHint = 4,  // its fast path is "the string is pure ASCII" (character index == byte index)
  kFnEncode = 8,     // hex / base64 and their inverses: opaque, of the kind GDV_MAP_ENCODE
};
unsigned FnTraits(const std::string& name);
bool IsNullLiteral(const Node& n);
std::vector<std::string> Utf8Chars(const std::string& text);  // runs that start at a byte that is not 10xxxxxx

// Selection mode: the row of input slot k that output slot `row` reads.  Columns of the caller's
// batch are gathered through the selection vector; the temporaries of a two-stage plan (schema
// index >= compact_from_) were produced BY a selection-mode first stage and are compact already.
inline std::string RowOf(const CodeGen& cg, int k) {
  return cg.input_fields_[k] >= cg.compact_from_ ? "(live ? row : 0)" : "srow[u]";
}

// Assembles the translation unit around the generated row body.
struct Assembler {
  CodeGen& cg;
  KernelPlan* plan;
  std::ostringstream src;
  int sweep_group_ = 1;  // > 1: wave-shaped main kernel whose byte sweep takes this many sub-tiles' spans at a time

  void Header(const std::vector<std::string>& expr_strings);
};
// names the kernel after its text (and the library functions it reaches) and substitutes GDV_KERNEL_NAME: every occurrence,
// or the first one only (string kernels have a single entry point)
// `tag`: appended to the name (plans that hold a value of a Make-time option carry the option's Key() tag: "uc")
void FinishKernel(std::string text, bool all_occurrences, std::string* name, std::string* source, const std::string& tag = std::string());
std::string SelCType(SelectionMode m);
void BindInputs(CodeGen& cg, KernelPlan* plan);  // what a plan records of its generation: the input slots, can_raise, the argument layout
// selection mode, inside the load loop: the slot's row (srow[u]) and every input gathered through it
void EmitSelectionLoads(std::ostream& s, CodeGen& cg, KernelPlan* plan);
// pointers of a tile function to the fixed-width inputs it reads and to its fixed-width outputs (inK / outE)
void EmitFixedPointers(std::ostream& s, CodeGen& cg, KernelPlan* plan);
// row mode, inside the row loop: sub-tile u's word of every bitmap the wave tile loaded (dK / vK from dw<suffix>K / vw<suffix>K)
void EmitTileWords(std::ostream& s, CodeGen& cg, KernelPlan* plan, const std::string& suffix = std::string());
extern const char* const kTilePreamble;          // first lines of every tile function: ctx, the constant block, the row count

// Output bitmap words are accumulated per wave tile: word u is deposited into lane u of an
// accumulator register, so the tile's GDV_U words leave with one coalesced store.  Outputs
// whose word expressions are textually identical share one accumulator.
struct WordAccumulators {
  std::map<std::string, std::string> by_expr;  // word expression -> accumulator name
  std::vector<std::string> names;
  std::string Get(CodeGen& cg, const std::string& word_expr) {
    auto it = by_expr.find(word_expr);
    if (it != by_expr.end()) return it->second;
    std::string name = "acc" + std::to_string(names.size());
    names.push_back(name);
    by_expr[word_expr] = name;
    cg.Stmt(name + " = gdv_deposit_word(" + name + ", u, " + word_expr + ", lane);");
    return name;
  }
};

std::string WordStore(const std::string& acc, const std::string& dst, bool nontemporal = false);

// the skeletons: each assembles the translation unit around cg's row body
Status Assemble(CodeGen& cg, KernelPlan* plan, const std::vector<std::string>& expr_strings, const WordAccumulators& accs,
                const std::string& decls_before_loop, const std::string& epilogue_after_loop);
Status AssembleStrings(CodeGen& cg, KernelPlan* plan, const std::vector<std::string>& expr_strings, const WordAccumulators& accs,
                       const std::string& decls_before_loop, const std::string& epilogue_after_loop);
enum class WaveKind { kMain, kPrepass };
Status AssembleStringsWave(CodeGen& cg, KernelPlan* plan, const std::vector<std::string>& expr_strings,
                           const WordAccumulators& accs, const std::string& decls_before_loop,
                           const std::string& decls_in_pass, const std::string& after_row_loop,
                           const std::string& epilogue_after_loop, WaveKind kind, bool has_direct_pass);
enum class FpShape { kDirect, kWindow, kSmall };  // kSmall: the windowed body, one workgroup per batch (many small batches)
Status PlanFilterProjectShape(const Schema& schema, const ExpressionPtr& condition, const std::vector<ExpressionPtr>& exprs,
                              SelectionMode index_mode, const CodegenOptions& opts, FpShape shape, KernelPlan* plan);

}  // namespace gdv::planner
