#include "gdv_planner_internal.h"

#include "gdv_regex.h"

#include <cstring>

namespace gdv::planner {

namespace {
#include "gdv_utf8_case_table.inc"  // gdv_utf8_upper_table / gdv_utf8_lower_table (tools/gen_utf8_case_table.py)
// what one direction may take of a plan's constant block
constexpr size_t kUtf8CaseTableMaxBytes = 16384;
static_assert(sizeof(gdv_utf8_upper_table) <= kUtf8CaseTableMaxBytes && sizeof(gdv_utf8_lower_table) <= kUtf8CaseTableMaxBytes,
              "utf8 case table beyond its bound");
}  // namespace

// One row per function the planner treats differently from a plain registry call.  (hash*: digests exactly when they return
// text, and castVARCHAR(non-string) is opaque: both by type, in CodeGen::Gen.)
unsigned FnTraits(const std::string& name) {
  static const std::map<std::string, unsigned> k = {
      {"reverse", kFnOpaque | kFnAsciiHint}, {"replace", kFnOpaque}, {"initcap", kFnOpaque}, {"repeat", kFnOpaque},
      {"space", kFnOpaque}, {"translate", kFnOpaque},
      {"mask", kFnOpaque}, {"mask_first_n", kFnOpaque}, {"mask_last_n", kFnOpaque}, {"mask_show_first_n", kFnOpaque},
      {"mask_show_last_n", kFnOpaque},
      {"sha256", kFnDigest}, {"sha1", kFnDigest}, {"sha", kFnDigest}, {"md5", kFnDigest},
      {"hex", kFnEncode}, {"to_hex", kFnEncode}, {"unhex", kFnEncode}, {"from_hex", kFnEncode}, {"base64", kFnEncode}, {"unbase64", kFnEncode},
      {"substr", kFnAsciiHint}, {"substring", kFnAsciiHint}, {"left", kFnAsciiHint}, {"right", kFnAsciiHint},
      {"char_length", kFnAsciiHint}, {"length", kFnAsciiHint}, {"lengthUtf8", kFnAsciiHint}, {"castVARCHAR", kFnAsciiHint},
      {"locate", kFnAsciiHint}, {"position", kFnAsciiHint}, {"strpos", kFnAsciiHint}, {"like", kFnAsciiHint},
      {"lpad", kFnAsciiHint}, {"rpad", kFnAsciiHint}};
  auto it = k.find(name);
  return it == k.end() ? 0u : it->second;
}

std::vector<std::string> Utf8Chars(const std::string& text) {
  std::vector<std::string> out;
  for (unsigned char c : text) {
    if (out.empty() || (c & 0xC0) != 0x80) out.emplace_back();
    out.back().push_back(static_cast<char>(c));
  }
  return out;
}

namespace {

// validity of a value that is null when any argument is: the union of the arguments' column sets goes to out->vcols, the
// conjunction of their per-lane predicates is returned
std::string MergeArgValidity(const CodeGen::FnArgs& args, Val* out) {
  std::string lanes;
  for (auto& a : args) {
    out->vcols.insert(a.vcols.begin(), a.vcols.end());
    lanes = CodeGen::AndExpr(lanes, a.vlane);
  }
  return lanes;
}

// a null literal among the arguments: the value is null on every row, and nothing has to be materialised for it
Status NullString(Val* out) {
  out->opaque = false;
  out->vlane = "false";
  out->v = "gdv_empty_str()";
  return Status::OK();
}

// lpad: the fill, then the text; rpad: the other way round
void PushPadPieces(bool left, const std::string& pad, const std::string& text, Val* out) {
  out->pieces.emplace_back(left ? pad : text, "");
  out->pieces.emplace_back(left ? text : pad, "");
}

// the constant-block table of translate(text, from, to) (layout: gdv_device_lib.hpp, GDV_MAP_TRANSLATE).  Characters of
// from / to are runs that start at a byte that is not 10xxxxxx; the first occurrence of a character in `from` wins.
void TranslateTable(const std::string& from, const std::string& to, std::string* tab) {
  const std::vector<std::string> fc = Utf8Chars(from), tc = Utf8Chars(to);
  bool ascii = true;
  for (unsigned char c : from + to) ascii = ascii && c < 0x80;
  auto put32 = [](std::string* t, uint32_t v) { t->append(reinterpret_cast<const char*>(&v), 4); };
  tab->clear();
  if (ascii) {
    put32(tab, 0);
    put32(tab, 0);
    tab->append(8, '\0');
    std::string m(256, '\0');
    std::vector<bool> seen(128, false);
    for (int c = 0; c < 256; c++) m[c] = static_cast<char>(c);
    for (size_t i = 0; i < fc.size(); i++) {
      const unsigned char c = static_cast<unsigned char>(fc[i][0]);
      if (seen[c]) continue;
      seen[c] = true;
      m[c] = i < tc.size() ? tc[i][0] : static_cast<char>(0xFF);  // GDV_TR_DELETE
    }
    *tab += m;
    return;
  }
  // kind 1: entries (key, replacement length, replacement offset, unused), then the replacement bytes.  A run of more than
  // four bytes is no well-formed character: it matches nothing (but keeps its position)
  std::vector<std::pair<uint32_t, std::string>> entries;
  std::set<uint32_t> seen;
  for (size_t i = 0; i < fc.size(); i++) {
    if (fc[i].size() > 4) continue;
    uint32_t key = 0;
    for (size_t j = 0; j < fc[i].size(); j++) key |= static_cast<uint32_t>(static_cast<unsigned char>(fc[i][j])) << (8 * j);
    if (!seen.insert(key).second) continue;
    entries.emplace_back(key, i < tc.size() ? tc[i] : std::string());
  }
  put32(tab, 1);
  put32(tab, static_cast<uint32_t>(entries.size()));
  tab->append(8, '\0');
  uint32_t at = 16 + 16 * static_cast<uint32_t>(entries.size());
  std::string bytes;
  for (auto& e : entries) {
    put32(tab, e.first);
    put32(tab, static_cast<uint32_t>(e.second.size()));
    put32(tab, at + static_cast<uint32_t>(bytes.size()));
    put32(tab, 0);
    bytes += e.second;
  }
  *tab += bytes;
}

}  // namespace

// SQL LIKE pattern -> (literal bytes, token kinds); `escape` < 0 means no escape character
Status CodeGen::CompileLike(const std::string& pat, int escape, std::string* bytes, std::string* kinds) {
  for (size_t i = 0; i < pat.size(); i++) {
    unsigned char c = static_cast<unsigned char>(pat[i]);
    if (escape >= 0 && c == static_cast<unsigned char>(escape)) {
      if (i + 1 >= pat.size())
        return Status::Invalid("like pattern must not end with the escape character");
      unsigned char nx = static_cast<unsigned char>(pat[i + 1]);
      if (nx != '%' && nx != '_' && nx != static_cast<unsigned char>(escape))
        return Status::Invalid("invalid escape sequence in like pattern");
      bytes->push_back(static_cast<char>(nx));
      kinds->push_back(0);
      i++;
    } else if (c == '%') {
      if (kinds->empty() || kinds->back() != 2) {  // collapse runs of %
        bytes->push_back(0);
        kinds->push_back(2);
      }
    } else if (c == '_') {
      bytes->push_back(0);
      kinds->push_back(1);
    } else {
      bytes->push_back(static_cast<char>(c));
      kinds->push_back(0);
    }
  }
  return Status::OK();
}

Status CodeGen::GenRegexpLike(const FunctionNode& fn, FnArgs& args, const std::string& active, Val* out) {
  // (patterns that are a plain literal became `like` when the tree was built: gdv_node.cc MakeFunctionNode)  Round 5, late:
  // the pattern is compiled to a position automaton here, at Make time; the row walks it with one 64-bit state set
  auto& pat = static_cast<const LiteralNode&>(*fn.children()[1]);
  out->vcols = args[0].vcols;
  out->vlane = args[0].vlane;
  if (pat.is_null()) {
    out->v = "false";
    out->vlane = "false";
    return Status::OK();
  }
  if (!args[0].pieces.empty() || args[0].opaque)
    return Status::CodeGenError("Function " + fn.ToString() + " not supported yet: a concat / lpad / rpad / reverse / replace / "
                                "castVARCHAR(number) result can only be an output expression or an argument of concat in the HIP backend. ");
  std::string table;
  GDV_RETURN_NOT_OK(CompileRegex(pat.value().bytes, &table));
  out->v = Tmp("bool", "gdv_regex_search(" + args[0].v + ", " + ByteTable(table) + ")");
  return Status::OK();
}

Status CodeGen::GenRegexpExtract(const FunctionNode& fn, FnArgs& args, const std::string& active, Val* out) {
  // regexp_extract(text, 'pattern', index) with a LITERAL pattern and index: the ordered lists for that one group are built
  // here, once per expression, into the constant block; the row's value is a narrower view of its text (as split_part's is)
  if (fn.children()[1]->kind() != NodeKind::kLiteral || fn.children()[2]->kind() != NodeKind::kLiteral)
    return Status::CodeGenError("Function " + fn.ToString() + " not supported yet: the HIP backend takes regexp_extract "
                                "with a literal pattern and a literal group index only (the pattern is compiled for that "
                                "group when the expression is compiled). ");
  auto& pat = static_cast<const LiteralNode&>(*fn.children()[1]);
  auto& idx = static_cast<const LiteralNode&>(*fn.children()[2]);
  out->vcols = args[0].vcols;
  if (pat.is_null() || idx.is_null()) return NullString(out);
  if (!args[0].pieces.empty() || args[0].opaque)
    return Status::CodeGenError("Function " + fn.ToString() + " not supported yet: a concat / lpad / rpad / reverse / replace / "
                                "castVARCHAR(number) result can only be an output expression or an argument of concat in the HIP backend. ");
  std::string table;
  GDV_RETURN_NOT_OK(CompileRegexExtract(pat.value().bytes, static_cast<int32_t>(idx.value().lo), &table));
  out->vlane = args[0].vlane;
  out->v = Tmp("gdv_str", "gdv_regex_extract(" + args[0].v + ", " + ByteTable(table) + ")");
  return Status::OK();
}

Status CodeGen::GenReplace(const FunctionNode& fn, FnArgs& args, const std::string& active, Val* out) {
  // replace(text, from, to) with LITERAL from / to: a table in the constant block; the result
  // is materialised by the output copy (GDV_MAP_REPLACE)
  if (fn.children()[1]->kind() != NodeKind::kLiteral || fn.children()[2]->kind() != NodeKind::kLiteral) {
    // round 5: from / to that are not both literals — the same rule with the arguments read through their own views,
    // per row (byte loops: a registry-tail path; literal arguments keep the table and the sweep's match bits)
    out->vlane = MergeArgValidity(args, out);
    can_raise_ = true;
    const std::string guard = AndExpr(AndExpr("live", active), LaneValid(*out));
    out->v = Tmp("gdv_str", guard + " ? gdv_replace_row(ctx, " + args[0].v + ", " + args[1].v + ", " + args[2].v + ") : gdv_empty_str()");
    return Status::OK();
  }
  auto& lf = static_cast<const LiteralNode&>(*fn.children()[1]);
  auto& lt = static_cast<const LiteralNode&>(*fn.children()[2]);
  out->vcols = args[0].vcols;
  if (lf.is_null() || lt.is_null()) return NullString(out);
  const std::string& from = lf.value().bytes;
  const std::string& to = lt.value().bytes;
  std::string tab(16, '\0');
  const int32_t fl = static_cast<int32_t>(from.size()), tl = static_cast<int32_t>(to.size());
  std::memcpy(&tab[0], &fl, 4);
  std::memcpy(&tab[4], &tl, 4);
  tab += from;
  tab.append((16 - from.size() % 16) % 16, '\0');
  tab += to;
  out->vlane = args[0].vlane;
  can_raise_ = true;
  const std::string guard = AndExpr(AndExpr("live", active), LaneValid(*out));
  // A 'from' that cannot overlap itself (no proper prefix is a suffix), over a whole column
  // row: the byte sweep marks the match positions of the sub-tile's span (the '%needle%'
  // machinery); the row counts its own bits, the copy walks them.  One such needle per
  // kernel; spans too long for the bitmap (wave-uniform) search per row as before.
  bool self_overlap = false;
  for (size_t k = 1; k < from.size(); k++) self_overlap |= from.compare(0, from.size() - k, from, k, from.size() - k) == 0;
  if (replace_hits_ && !selection() && args[0].col_slot >= 0 && from.size() >= 2 && from.size() <= 8 && !self_overlap) {
    int h = -1;
    for (size_t i = 0; i < contains_hooks_.size(); i++)
      if (contains_hooks_[i].slot == args[0].col_slot && contains_hooks_[i].map == args[0].col_map && contains_hooks_[i].needle == from)
        h = static_cast<int>(i);
    if (replace_hook_ < 0 || replace_hook_ == h) {
      const std::string K = std::to_string(args[0].col_slot), table = ByteTable(tab);
      if (h < 0) {
        // (the needle's bytes are in the replace table itself, 16 bytes in: no table of its own,
        // so the scanner-shaped fallback — which has no such hook — lays out the same constants)
        contains_hooks_.push_back({args[0].col_slot, args[0].col_map, from});
        hook_tables_.push_back("(" + table + " + 16)");
        h = static_cast<int>(contains_hooks_.size()) - 1;
      }
      replace_hook_ = h;
      out->v = Tmp("gdv_str", guard + " ? (hm_ok" + K + " ? gdv_replace_hits(ctx, " + args[0].v + ", " + table + ", hit" +
                                  std::to_string(h) + ", oa" + K + "[u] - sb" + K + ") : gdv_replace(ctx, " + args[0].v + ", " +
                                  table + ")) : gdv_empty_str()");
      return Status::OK();
    }
  }
  out->v = Tmp("gdv_str", guard + " ? gdv_replace(ctx, " + args[0].v + ", " + ByteTable(tab) + ") : gdv_empty_str()");
  return Status::OK();
}

Status CodeGen::GenTranslate(const FunctionNode& fn, FnArgs& args, const std::string& active, Val* out) {
  // translate(text, from, to) with LITERAL from / to: the character table is built here, once per expression, into the
  // constant block (gdv_device_lib.hpp lays it out); the row computes the length, the output copy writes
  if (fn.children()[1]->kind() != NodeKind::kLiteral || fn.children()[2]->kind() != NodeKind::kLiteral)
    return Status::CodeGenError("Function " + fn.ToString() + " not supported yet: the HIP backend takes translate "
                                "with literal from and to strings only (its character table is built when the "
                                "expression is compiled). ");
  auto& lf = static_cast<const LiteralNode&>(*fn.children()[1]);
  auto& lt = static_cast<const LiteralNode&>(*fn.children()[2]);
  out->vcols = args[0].vcols;
  if (lf.is_null() || lt.is_null()) return NullString(out);
  if (lf.value().bytes.empty()) {  // nothing to translate: the text itself
    *out = args[0];
    out->type = fn.return_type();
    return Status::OK();
  }
  std::string tab;
  TranslateTable(lf.value().bytes, lt.value().bytes, &tab);
  out->vlane = args[0].vlane;
  can_raise_ = true;
  translate_ = true;
  const std::string guard = AndExpr(AndExpr("live", active), LaneValid(*out));
  out->v = Tmp("gdv_str", guard + " ? gdv_translate(ctx, " + args[0].v + ", " + ByteTable(tab) + ") : gdv_empty_str()");
  return Status::OK();
}

Status CodeGen::GenUtf8Case(const FunctionNode& fn, FnArgs& args, const std::string& active, Val* out) {
  // upper / lower(text) under GDV_UTF8_CASE=1: utf8proc's simple case map, one table per direction and plan in the constant
  // block (gdv_device_lib.hpp lays it out); the row computes the length and validates, the output copy writes
  const int dir = fn.name() == "upper" ? 1 : 2;
  auto it = case_tables_.find(dir);
  if (it == case_tables_.end()) {
    const std::string tab = dir == 1 ? std::string(reinterpret_cast<const char*>(gdv_utf8_upper_table), sizeof(gdv_utf8_upper_table))
                                     : std::string(reinterpret_cast<const char*>(gdv_utf8_lower_table), sizeof(gdv_utf8_lower_table));
    it = case_tables_.emplace(dir, ByteTable(tab)).first;
  }
  out->vcols = args[0].vcols;
  out->vlane = args[0].vlane;
  can_raise_ = true;
  utf8_case_ = true;
  const std::string guard = AndExpr(AndExpr("live", active), LaneValid(*out));
  out->v = Tmp("gdv_str", guard + " ? gdv_utf8_case(ctx, " + args[0].v + ", " + it->second + ") : gdv_empty_str()");
  return Status::OK();
}

Status CodeGen::GenMask(const FunctionNode& fn, FnArgs& args, const std::string& active, Val* out) {
  // mask(text[, upper[, lower[, digit]]]) with LITERAL one-byte replacements below 0x80 (defaults 'X', 'x', 'n') and
  // mask_first_n / mask_last_n / mask_show_first_n / mask_show_last_n(text, n) with a literal or per-row n: the row packs the
  // parameters into the value and reads no byte, the output copy classifies and writes (gdv_device_lib.hpp, GDV_MAP_MASK)
  (void)active;
  const std::string& name = fn.name();
  int mode = 0;  // GDV_MASK_ALL ...
  unsigned reps = 'X' | ('x' << 8) | ('n' << 16);
  std::string n = "0";
  if (name == "mask") {
    bool null_literal = false;
    for (size_t i = 1; i < args.size(); i++) {
      const Node& c = *fn.children()[i];
      const bool literal = c.kind() == NodeKind::kLiteral;
      const std::string* bytes = literal ? &static_cast<const LiteralNode&>(c).value().bytes : nullptr;
      if (literal && static_cast<const LiteralNode&>(c).is_null()) {
        null_literal = true;
        continue;
      }
      if (!literal || bytes->size() != 1 || static_cast<unsigned char>((*bytes)[0]) >= 0x80)
        return Status::CodeGenError("Function " + fn.ToString() + " not supported yet: the HIP backend takes mask with "
                                    "literal replacement characters of exactly one byte below 0x80 only (argument " +
                                    std::to_string(i + 1) + " is " + (!literal ? "not a literal" : bytes->empty() ? "empty" :
                                    bytes->size() > 1 ? "longer than one byte" : "a byte >= 0x80") + "). ");
      reps = (reps & ~(0xFFu << (8 * (i - 1)))) | (static_cast<unsigned>(static_cast<unsigned char>((*bytes)[0])) << (8 * (i - 1)));
    }
    out->vcols = args[0].vcols;
    if (null_literal) return NullString(out);
    out->vlane = args[0].vlane;
  } else {
    mode = name == "mask_first_n" ? 1 : name == "mask_last_n" ? 2 : name == "mask_show_first_n" ? 3 : 4;
    n = args[1].v;
    out->vlane = MergeArgValidity(args, out);
  }
  mask_ = true;
  out->v = Tmp("gdv_str", "gdv_mask(" + args[0].v + ", " + std::to_string(mode) + ", (gdv_int32)(" + n + "), " + std::to_string(reps) + "u)");
  return Status::OK();
}

Status CodeGen::GenPad(const FunctionNode& fn, FnArgs& args, const std::string& active, Val* out) {
  // lpad / rpad(text, n[, fill]) with LITERAL n and fill: two pieces (device library), the
  // fill repeated to n characters laid out once in the constant block
  const Node& nn = *fn.children()[1];
  const Node* fl = fn.children().size() == 3 ? fn.children()[2].get() : nullptr;
  if (nn.kind() != NodeKind::kLiteral || (fl != nullptr && fl->kind() != NodeKind::kLiteral)) {
    // round 5: a length or a fill that is not a literal — the fill is read cyclically through its own view, per row
    const std::string lanes = MergeArgValidity(args, out);
    can_raise_ = true;
    const std::string fillv = fl != nullptr ? args[2].v : Tmp("gdv_str", StringConstant(" "));
    const std::string guard = AndExpr(AndExpr("live", active), AndExpr(lanes, LaneValid(args[0])));
    const std::string want = Tmp("gdv_int32", guard + " ? (gdv_int32)" + args[1].v + " : 0");
    const std::string text = Tmp("gdv_str", "gdv_pad_text(" + args[0].v + ", " + want + ")");
    const std::string pad = Tmp("gdv_str", "gdv_pad_fill_row(ctx, " + args[0].v + ", " + want + ", " + fillv + ")");
    PushPadPieces(fn.name() == "lpad", pad, text, out);
    out->vlane = lanes;
    out->v = "gdv_empty_str()";  // never read: consumers use the pieces
    return Status::OK();
  }
  auto& nl = static_cast<const LiteralNode&>(nn);
  const bool null_lit = nl.is_null() || (fl != nullptr && static_cast<const LiteralNode*>(fl)->is_null());
  const int32_t n = null_lit ? 0 : static_cast<int32_t>(nl.value().lo);
  if (n > (1 << 16))
    return Status::CodeGenError("Function " + fn.ToString() +
                                " not supported yet: pad lengths above 65536 characters. ");
  const std::string fill = fl != nullptr ? static_cast<const LiteralNode*>(fl)->value().bytes : " ";
  const std::vector<std::string> chars = Utf8Chars(fill);
  std::string tab;
  bool ascii = true;
  for (int32_t k = 0; k < n && !chars.empty(); k++) tab += chars[k % chars.size()];
  for (unsigned char c : tab) ascii = ascii && c < 0x80;
  const std::string N = std::to_string(n);
  const std::string text = Tmp("gdv_str", "gdv_pad_text(" + args[0].v + ", " + N + ")");
  const std::string pad = Tmp("gdv_str", "gdv_pad_fill(" + args[0].v + ", " + N + ", " + ByteTable(tab) + ", " +
                                             std::to_string(tab.size()) + ", " + (ascii ? "true" : "false") + ")");
  PushPadPieces(fn.name() == "lpad", pad, text, out);
  out->vcols = args[0].vcols;
  out->vlane = null_lit ? "false" : args[0].vlane;
  out->v = "gdv_empty_str()";  // never read: consumers use the pieces
  return Status::OK();
}

Status CodeGen::GenConcat(const FunctionNode& fn, FnArgs& args, const std::string& active, Val* out) {
  // concat: a null argument is the empty string, the result is never null;
  // concatOperator (||): null if any argument is null
  const bool never_null = fn.name() == "concat";
  for (auto& a : args) {
    const std::string present = never_null ? LaneValid(a) : "";
    if (a.pieces.empty()) {
      out->pieces.emplace_back(a.v, present == "true" ? "" : present);
    } else {
      for (auto& pc : a.pieces) {
        std::string pv = AndExpr(pc.second, present);
        out->pieces.emplace_back(pc.first, pv);
      }
    }
  }
  if (!never_null) out->vlane = MergeArgValidity(args, out);
  out->v = "gdv_empty_str()";  // never read: consumers use the pieces
  return Status::OK();
}

Status CodeGen::GenToDate(const FunctionNode& fn, FnArgs& args, const std::string& active, Val* out) {
  // to_date(s, 'pattern'[, suppress_errors]): the pattern becomes one byte per strptime directive here, at Make
  // time, the way the reference's ToDateHolder converts it once per expression; the row interprets it
  auto& pat = static_cast<const LiteralNode&>(*fn.children()[1]);
  if (pat.is_null()) return Status::Invalid("Invalid date format: null");
  int suppress = 0;
  if (fn.children().size() == 3) {
    auto& sl = static_cast<const LiteralNode&>(*fn.children()[2]);
    suppress = !sl.is_null() && static_cast<int32_t>(sl.value().lo) == 1 ? 1 : 0;
  }
  std::string ops;
  GDV_RETURN_NOT_OK(CompileDateFormat(pat.value().bytes, &ops));
  can_raise_ = true;
  const std::string ov = "ov" + std::to_string(next_tmp_++);
  Stmt("bool " + ov + " = false;");
  const std::string guard = AndExpr(AndExpr("live", active), LaneValid(args[0]));
  out->v = Tmp("gdv_int64", guard + " ? gdv_parse_date(ctx, " + args[0].v + ", " + ByteTable(ops) + ", " + std::to_string(ops.size()) + ", " +
                                std::to_string(suppress) + ", true, &" + ov + ") : (gdv_int64)0");
  out->vlane = ov;
  return Status::OK();
}

Status CodeGen::GenLike(const FunctionNode& fn, FnArgs& args, const std::string& active, Val* out) {
  // like(s, 'pattern'[, 'escape']): the pattern is compiled here, at Make time, the way
  // the reference's LikeHolder compiles it to a regex once per expression
  auto& pat = static_cast<const LiteralNode&>(*fn.children()[1]);
  int escape = -1;
  if (fn.children().size() == 3) {
    if (fn.children()[2]->kind() != NodeKind::kLiteral)
      return Status::ValidationError("'like' function requires a literal as the escape character");
    auto& esc = static_cast<const LiteralNode&>(*fn.children()[2]);
    if (esc.value().bytes.size() != 1)
      return Status::Invalid("The length of escape char in like function must be 1");
    escape = static_cast<unsigned char>(esc.value().bytes[0]);
  }
  if (pat.is_null()) {
    out->v = "false";
    out->vlane = "false";
    return Status::OK();
  }
  std::string pattern = pat.value().bytes;
  if (fn.name() == "ilike") {
    // case-insensitive: the pattern's ASCII letters are lowered here, the string is read through the
    // lower-case byte map (a whole-column argument stays a whole-column view: the sweep still answers '%needle%')
    for (auto& ch : pattern)
      if (ch >= 'A' && ch <= 'Z') ch = static_cast<char>(ch + 32);
    args[0].v = Tmp("gdv_str", "lower_utf8(" + args[0].v + ")");
    if (args[0].col_slot >= 0) args[0].col_map = 2;
  }
  std::string bytes, kinds;
  GDV_RETURN_NOT_OK(CompileLike(pattern, escape, &bytes, &kinds));
  out->vcols = args[0].vcols;
  out->vlane = args[0].vlane;
  // common shapes skip the general matcher: literal | literal% | %literal | %literal%
  const size_t nk = kinds.size();
  const bool lead = nk > 0 && kinds.front() == 2, trail = nk > 0 && kinds.back() == 2;
  const size_t lo = lead ? 1 : 0, hi = nk - ((trail && nk > lo) ? 1 : 0);
  bool plain = true;
  for (size_t i = lo; i < hi; i++) plain = plain && kinds[i] == 0;
  if (plain && !(nk == 1 && lead)) {
    const std::string lit = bytes.substr(lo, hi - lo);
    const char* fnname = lead && trail ? "gdv_like_contains" : lead ? "gdv_like_suffix"
                         : trail ? "gdv_like_prefix" : "gdv_like_equal";
    const std::string per_row = std::string(fnname) + "(" + args[0].v + ", " + ByteTable(lit) + ", " +
                                std::to_string(lit.size()) + ")";
    if (lead && trail && lit.size() >= 2 && lit.size() <= 8 && args[0].col_slot >= 0 && !selection() && !no_hooks_) {
      // '%needle%' over a whole input row: the byte sweep has marked every match position
      // of the tile's span in an LDS bitmap; the row tests its own byte range.  Spans too
      // long for the bitmap (wave-uniform) take the per-row search.
      const int h = HookFor(args[0].col_slot, args[0].col_map, lit);
      const std::string k = std::to_string(args[0].col_slot);
      out->v = Tmp("bool", AblSel(2, "(ob" + k + "[u] - oa" + k + "[u] > 19)",
                                      "(hm_ok" + k + " ? gdv_range_any(hit" + std::to_string(h) + ", oa" + k + "[u] - sb" + k +
                                          ", ob" + k + "[u] - sb" + k + " - " + std::to_string(lit.size() - 1) + ") : " +
                                          per_row + ")"));
      return Status::OK();
    }
    out->v = Tmp("bool", per_row);
    return Status::OK();
  }
  std::string pb = ByteTable(bytes), pk = ByteTable(kinds);
  out->v = Tmp("bool", "gdv_like(" + args[0].v + ", " + pb + ", " + pk + ", " +
                           std::to_string(kinds.size()) + ")");
  return Status::OK();
}

Status CodeGen::GenCall(const FunctionNode& fn, const FunctionDef& def, FnArgs& args, const std::string& active, Val* out) {
  const std::string ctype = out->type.CType();
  std::string call = def.symbol + "(";
  bool first = true;
  auto push = [&](const std::string& a) {
    if (!first) call += ", ";
    call += a;
    first = false;
  };
  if (def.flags & kNeedsContext) {
    push("ctx");
    can_raise_ = true;
  }
  // functions that see validity: value, (precision, scale) of a decimal, validity; the result's pair when it is a decimal
  auto push_with_validity = [&](const Val& a) {
    push(a.v);
    if ((def.flags & kDecimalArgs) && a.type.is_decimal()) {
      push(std::to_string(a.type.precision));
      push(std::to_string(a.type.scale));
    }
    push(LaneValid(a));
  };
  auto push_decimal_result = [&]() {
    if ((def.flags & kDecimalArgs) && out->type.is_decimal()) {
      push(std::to_string(out->type.precision));
      push(std::to_string(out->type.scale));
    }
  };
  if (def.policy == NullPolicy::kNullIfNull) {
    for (auto& a : args) {
      push(a.v);
      if ((def.flags & kDecimalArgs) && a.type.is_decimal()) {
        push(std::to_string(a.type.precision));
        push(std::to_string(a.type.scale));
      }
    }
    if (def.flags & kDecimalArgs) {
      push(std::to_string(out->type.precision));
      push(std::to_string(out->type.scale));
    }
    out->vlane = MergeArgValidity(args, out);
    call += ")";
    if (def.flags & kNeedsContext) {
      // Functions that can raise run only on rows where every argument is valid and
      // the enclosing if/else / short-circuit path is live — otherwise a guarded
      // `if (b != 0) a / b` would raise on the rows it guards against.
      std::string guard = AndExpr(AndExpr("live", active), LaneValid(*out));
      const std::string idle = out->type.is_varlen() ? "gdv_empty_str()" : "(" + ctype + ")0";
      out->v = Tmp(ctype, guard + " ? " + call + " : " + idle);
    } else {
      out->v = Tmp(ctype, call);
    }
  } else if (def.policy == NullPolicy::kNullNever) {
    for (auto& a : args) push_with_validity(a);
    push_decimal_result();
    call += ")";
    out->v = Tmp(ctype, call);
  } else {
    for (auto& a : args) push_with_validity(a);
    push_decimal_result();
    std::string ov = "ov" + std::to_string(next_tmp_++);
    Stmt("bool " + ov + " = false;");
    push("&" + ov);
    call += ")";
    out->v = Tmp(ctype, call);
    out->vlane = ov;
  }
  return Status::OK();
}

}  // namespace gdv::planner
