#include "gdv_planner_internal.h"

#include <algorithm>
#include <functional>

namespace gdv::planner {

std::string CodeGen::LaneValid(const Val& val) {
  std::string cols;
  if (!val.vcols.empty()) {
    if (selection()) {
      for (int k : val.vcols) cols = AndExpr(cols, "b" + std::to_string(k) + "[u]");
    } else {
      cols = Tmp("bool", "gdv_lane_bit(" + WordExpr(val.vcols) + ", lane)");
    }
  }
  std::string r = AndExpr(cols, val.vlane);
  return r.empty() ? "true" : r;
}

std::string CodeGen::WordExpr(const std::set<int>& cols) {
  if (cols.empty()) return "~0ull";
  std::string s;
  for (int k : cols) {
    if (!s.empty()) s += " & ";
    s += "v" + std::to_string(k);
  }
  if (cols.size() > 1) s = Tmp("gdv_uint64", s);
  return s;
}

std::string CodeGen::InlineLiteral(const DataType& t, const Literal& v) {
  switch (t.id) {
    case kBool: return v.lo ? "true" : "false";
    case kFloat: return "__uint_as_float(" + Hex64(v.lo & 0xffffffffull) + ")";
    case kDouble: return "__longlong_as_double((long long)" + Hex64(v.lo) + ")";
    case kDecimal128: return "gdv_make_int128(" + Hex64(v.hi) + ", " + Hex64(v.lo) + ")";
    default: {
      uint64_t mask = t.byte_width() >= 8 ? ~0ull : ((1ull << (8 * t.byte_width())) - 1);
      return "((" + t.CType() + ")" + Hex64(v.lo & mask) + ")";
    }
  }
}

std::string CodeGen::LiteralExprNew(const DataType& t, const Literal& v) {
  auto slot = [&](uint64_t x) { return "A.lit[" + std::to_string(LitSlot(x)) + "]"; };
  switch (t.id) {
    case kBool: return v.lo ? "true" : "false";
    case kFloat: return "__uint_as_float((gdv_uint32)" + slot(v.lo & 0xffffffffull) + ")";
    case kDouble: return "__longlong_as_double((long long)" + slot(v.lo) + ")";
    case kDecimal128: {
      // two consecutive slots that are never shared with single-word literals
      lits_.push_back(v.lo);
      lits_.push_back(v.hi);
      const std::string i = std::to_string(lits_.size() - 2), j = std::to_string(lits_.size() - 1);
      return "gdv_make_int128(A.lit[" + j + "], A.lit[" + i + "])";
    }
    default: {
      uint64_t mask = t.byte_width() >= 8 ? ~0ull : ((1ull << (8 * t.byte_width())) - 1);
      return "((" + t.CType() + ")" + slot(v.lo & mask) + ")";
    }
  }
}

std::string CodeGen::ByteTable(const std::string& bytes, const char* ctype) {
  while (blob_.size() % 16 != 0) blob_.push_back('\0');
  const size_t off = blob_.size();
  blob_ += bytes;
  blob_.append(8, '\0');  // 8-byte loads may run past the table's end
  return "((const " + std::string(ctype) + "*)(gdv_cst + " + std::to_string(off) + "))";
}

std::string CodeGen::StringConstant(const std::string& bytes) {
  std::string t = ByteTable(bytes);
  bool ascii = true;
  for (unsigned char c : bytes) ascii = ascii && c < 0x80;
  return "gdv_make_str(" + t + ", 0, " + std::to_string(bytes.size()) + ", " + t + " + " +
         std::to_string(bytes.size() + 8) + (ascii ? ", GDV_STR_ASCII | GDV_STR_INBUF)" : ", GDV_STR_INBUF)");
}

std::set<int> CodeGen::StringSlotsOf(const Node& node) {
  std::set<int> r;
  std::function<void(const Node&)> walk = [&](const Node& n) {
    switch (n.kind()) {
      case NodeKind::kField: {
        auto& f = static_cast<const FieldNode&>(n);
        if (f.return_type().is_varlen()) r.insert(SlotFor(f, true, true));
        break;
      }
      case NodeKind::kFunction:
        for (auto& c : static_cast<const FunctionNode&>(n).children()) walk(*c);
        break;
      case NodeKind::kIf: {
        auto& i = static_cast<const IfNode&>(n);
        walk(*i.condition()); walk(*i.then_node()); walk(*i.else_node());
        break;
      }
      case NodeKind::kBoolean:
        for (auto& c : static_cast<const BooleanNode&>(n).children()) walk(*c);
        break;
      case NodeKind::kIn: walk(*static_cast<const InNode&>(n).eval()); break;
      default: break;
    }
  };
  walk(node);
  return r;
}

int CodeGen::SlotFor(const FieldNode& f, bool values, bool validity) {
  int idx = -1;
  for (size_t i = 0; i < schema_.size(); i++)
    if (schema_[i].name == f.field().name) idx = static_cast<int>(i);
  int slot;
  auto it = slot_of_field_.find(idx);
  if (it == slot_of_field_.end()) {
    slot = static_cast<int>(input_fields_.size());
    slot_of_field_[idx] = slot;
    input_fields_.push_back(idx);
    needs_values_.push_back(false);
    needs_validity_.push_back(false);
  } else {
    slot = it->second;
  }
  if (values) needs_values_[slot] = true;
  if (validity) needs_validity_[slot] = true;
  return slot;
}

int CodeGen::HookFor(int slot, int map, const std::string& needle) {
  for (size_t h = 0; h < contains_hooks_.size(); h++)
    if (contains_hooks_[h].slot == slot && contains_hooks_[h].map == map && contains_hooks_[h].needle == needle)
      return static_cast<int>(h);
  contains_hooks_.push_back({slot, map, needle});
  hook_tables_.push_back(ByteTable(needle));
  return static_cast<int>(contains_hooks_.size()) - 1;
}

bool IsNullLiteral(const Node& n) {
  return n.kind() == NodeKind::kLiteral && static_cast<const LiteralNode&>(n).is_null();
}

Status CodeGen::Gen(const Node& node, const std::string& active, Val* out) {
  switch (node.kind()) {
    case NodeKind::kField: {
      auto& f = static_cast<const FieldNode&>(node);
      int slot = SlotFor(f, true, true);
      out->type = f.return_type();
      std::string k = std::to_string(slot);
      if (f.return_type().is_varlen()) {
        out->v = "s" + k;  // per-iteration view built from the two offsets (row phase prologue)
        out->col_slot = slot;
        out->col_map = 0;
      } else if (f.return_type().id == kBool) {
        out->v = selection() ? "x" + k + "[u]" : Tmp("bool", "gdv_lane_bit(d" + k + ", lane)");
      } else {
        out->v = "c" + k + "[u]";
      }
      out->vcols = {slot};
      out->vlane.clear();
      return Status::OK();
    }
    case NodeKind::kLiteral: {
      auto& l = static_cast<const LiteralNode&>(node);
      out->type = l.return_type();
      out->col_slot = -1;
      out->v = l.return_type().is_varlen() ? StringConstant(l.value().bytes) : LiteralExpr(l.return_type(), l.value(), &node);
      out->vcols.clear();
      out->vlane = l.is_null() ? "false" : "";
      return Status::OK();
    }
    case NodeKind::kFunction: {
      auto& fn = static_cast<const FunctionNode&>(node);
      const FunctionDef* def = nullptr;
      DataType ret;
      if (!ResolveFunction(fn, &def, &ret))
        return Status::CodeGenError("Function " + fn.ToString() + " not supported yet. ");
      // Integer literals handed to a function over strings (substr positions, left / right
      // counts, castVARCHAR lengths ...) are part of the query's SHAPE: compiled in, so the
      // position arithmetic folds (C5: +0.2 ms when they were kernel arguments).  Everything
      // else — comparison constants, arithmetic operands, IN lists, LIKE needles — is an argument.
      bool over_strings = false;
      for (auto& c : fn.children()) over_strings |= c->return_type().is_varlen();
      std::vector<Val> args(fn.children().size());
      for (size_t i = 0; i < args.size(); i++) {
        const Node& child = *fn.children()[i];
        if (over_strings && child.kind() == NodeKind::kLiteral && !child.return_type().is_varlen() &&
            !opts_.no_inline_string_args) {
          auto& l = static_cast<const LiteralNode&>(child);
          args[i].type = l.return_type();
          args[i].v = InlineLiteral(l.return_type(), l.value());
          args[i].vlane = l.is_null() ? "false" : "";
          continue;
        }
        GDV_RETURN_NOT_OK(Gen(child, active, &args[i]));
      }
      *out = Val();  // a value of its own: nothing of what `out` held before
      out->type = fn.return_type();
      const std::string& name = fn.name();
      if (name == "regexp_like" || name == "regexp_matches") return GenRegexpLike(fn, args, active, out);
      if (name == "regexp_extract") return GenRegexpExtract(fn, args, active, out);
      if (name.compare(0, 7, "regexp_") == 0)
        return Status::CodeGenError("Function " + fn.ToString() + " not supported yet: the HIP backend takes regexp_replace "
                                    "with a literal pattern and a replacement without backslashes only (no metacharacters, "
                                    "no '%' or '_'). ");
      const unsigned traits = FnTraits(name);
      const bool digest = name.compare(0, 4, "hash") == 0 ? fn.return_type().is_varlen() : (traits & kFnDigest) != 0;
      out->opaque = (traits & (kFnOpaque | kFnEncode)) != 0 || digest || (name == "castVARCHAR" && !args[0].type.is_varlen());
      if (traits & kFnEncode) encode_ = true;  // (planned as an ordinary call; its value is a GDV_MAP_ENCODE)
      if (name == "castVARCHAR" && (args[0].type.id == kDate32 || args[0].type.id == kDate64 ||
                                    args[0].type.id == kTimestamp || args[0].type.id == kTime32))
        datetime_ = true;  // (planned as an ordinary call; its value is a GDV_MAP_DATETIME)
      // (GDV_UTF8_CASE=1 at Make: a value of its own, whose length follows from the bytes — no byte map over the column's offsets)
      const bool utf8_case = opts_.utf8_case && (name == "upper" || name == "lower") && args.size() == 1;
      if (utf8_case) out->opaque = true;
      if (!utf8_case && (name == "upper" || name == "lower") && args.size() == 1 && args[0].col_slot >= 0) {
        out->col_slot = args[0].col_slot;
        out->col_map = name == "upper" ? 1 : 2;
      }
      if (traits & kFnAsciiHint)
        for (size_t i = 0; i < args.size(); i++)
          if (args[i].type.is_varlen())
            for (int k : StringSlotsOf(*fn.children()[i])) ascii_slots_.insert(k);
      const bool is_concat = name == "concat" || name == "concatOperator";
      for (auto& a : args)
        if ((!a.pieces.empty() || a.opaque) && !is_concat)
          return Status::CodeGenError("Function " + fn.ToString() +
                                      " not supported yet: a concat / lpad / rpad / reverse / replace / castVARCHAR(number) "
                                      "result can only be an output expression or an argument of concat in the "
                                      "HIP backend. ");
      if (name == "replace") return GenReplace(fn, args, active, out);
      if (name == "translate") return GenTranslate(fn, args, active, out);
      if (utf8_case) return GenUtf8Case(fn, args, active, out);
      if (name.compare(0, 4, "mask") == 0) return GenMask(fn, args, active, out);
      if (name == "lpad" || name == "rpad") return GenPad(fn, args, active, out);
      if (is_concat) return GenConcat(fn, args, active, out);
      if (def->flags & kDateFormatArg) return GenToDate(fn, args, active, out);
      if (def->flags & kPatternArg) return GenLike(fn, args, active, out);
      return GenCall(fn, *def, args, active, out);
    }
    case NodeKind::kIf: {
      auto& n = static_cast<const IfNode&>(node);
      Val c, t, e;
      GDV_RETURN_NOT_OK(Gen(*n.condition(), active, &c));
      // a null condition selects the else branch
      std::string take = Tmp("bool", AndFull(LaneValid(c), c.v));
      GDV_RETURN_NOT_OK(Gen(*n.then_node(), AndExpr(active, take), &t));
      GDV_RETURN_NOT_OK(Gen(*n.else_node(), AndExpr(active, "!" + take), &e));
      // `if (c) <materialised value> else NULL` (and its mirror): the value is the branch's, valid only
      // where the branch is taken — what a guarded first-stage expression of a two-stage plan looks
      // like (StageMaterialisedValues), and fine wherever a materialised value is (output, concat)
      {
        const bool t_mat = !t.pieces.empty() || t.opaque, e_mat = !e.pieces.empty() || e.opaque;
        if (t_mat != e_mat && IsNullLiteral(t_mat ? *n.else_node() : *n.then_node())) {
          const Val& m = t_mat ? t : e;
          const std::string taken = t_mat ? take : "!" + take;
          *out = m;
          out->type = n.return_type();
          if (!m.vcols.empty()) {  // fold the column validity into the lane predicate next to the guard
            out->vlane = AndExpr(LaneValid(m), taken);
            out->vcols.clear();
          } else {
            out->vlane = AndExpr(m.vlane, taken);
          }
          for (auto& pc : out->pieces) pc.second = AndExpr(pc.second, taken);
          out->col_slot = -1;
          return Status::OK();
        }
      }
      if (!t.pieces.empty() || !e.pieces.empty() || t.opaque || e.opaque)
        return Status::CodeGenError(
            "if/else over a concat / lpad / rpad / reverse / replace / castVARCHAR(number) result is not supported by the HIP "
            "backend yet");
      out->type = n.return_type();
      const std::string ctype = out->type.CType();
      out->pieces.clear();
      out->col_slot = -1;
      out->opaque = false;
      out->v = Tmp(ctype, take + " ? " + t.v + " : " + e.v);
      out->vcols.clear();
      if (t.never_null() && e.never_null()) {
        out->vlane.clear();
      } else {
        out->vlane = Tmp("bool", take + " ? " + LaneValid(t) + " : " + LaneValid(e));
      }
      return Status::OK();
    }
    case NodeKind::kBoolean: {
      // SQL three-valued logic with left-to-right short circuit:
      //   AND: false if any child is (valid, false); else null if any child is null; else true
      //   OR : true  if any child is (valid, true);  else null if any child is null; else false
      auto& n = static_cast<const BooleanNode&>(node);
      const bool is_and = n.op() == BooleanNode::kAnd;
      std::string decided;    // some earlier child already fixed the result
      std::string all_valid;  // every child so far valid
      std::string live_path = active;
      for (auto& child : n.children()) {
        Val c;
        GDV_RETURN_NOT_OK(Gen(*child, live_path, &c));
        std::string cvalid = LaneValid(c);
        std::string hit = AndFull(cvalid, is_and ? "!" + c.v : c.v);
        hit = Tmp("bool", hit);
        decided = decided.empty() ? hit : Tmp("bool", "(" + decided + " || " + hit + ")");
        all_valid = AndExpr(all_valid, cvalid);
        live_path = AndExpr(active, "!" + decided);
      }
      out->type = boolean();
      out->vcols.clear();
      out->col_slot = -1;
      if (all_valid.empty() || all_valid == "true") {
        out->vlane.clear();
        out->v = Tmp("bool", is_and ? "!" + decided : decided);
      } else {
        std::string av = Tmp("bool", all_valid);
        out->vlane = Tmp("bool", "(" + decided + " || " + av + ")");
        // value bit under a null result is defined as false
        out->v = Tmp("bool", is_and ? "(!" + decided + " && " + av + ")" : decided);
      }
      return Status::OK();
    }
    case NodeKind::kIn: {
      auto& n = static_cast<const InNode&>(node);
      Val x;
      GDV_RETURN_NOT_OK(Gen(*n.eval(), active, &x));
      if (!x.pieces.empty() || x.opaque)
        return Status::CodeGenError(
            "IN over a concat / lpad / rpad / reverse / replace / castVARCHAR(number) result is not supported by the HIP backend yet");
      out->pieces.clear();
      out->col_slot = -1;
      out->type = boolean();
      out->vcols = x.vcols;
      out->vlane = x.vlane;
      if (n.value_type().is_varlen()) {
        std::string bytes, offs;
        auto put32 = [&](uint32_t v) { offs.append(reinterpret_cast<const char*>(&v), 4); };
        put32(0);
        for (auto& l : n.values()) {
          bytes += l.bytes;
          put32(static_cast<uint32_t>(bytes.size()));
        }
        const std::string tab = ByteTable(offs, "gdv_int32");
        out->v = Tmp("bool", "gdv_in_strings(" + x.v + ", " + ByteTable(bytes) + ", " + tab + ", " +
                                 std::to_string(n.values().size()) + ")");
        return Status::OK();
      }
      const DataType& vt = n.value_type();
      if (vt.is_decimal()) {
        // 16-byte values: equality against two argument slots each (lists are short in practice)
        if (n.values().size() > 64)
          return Status::CodeGenError("IN over decimal128 with more than 64 values is not supported by the HIP backend yet");
        std::string e;
        for (auto& l : n.values()) {
          lits_.push_back(l.lo);
          lits_.push_back(l.hi);
          const std::string i = std::to_string(lits_.size() - 2), j = std::to_string(lits_.size() - 1);
          if (!e.empty()) e += " || ";
          e += "(" + x.v + " == gdv_make_int128(A.lit[" + j + "], A.lit[" + i + "]))";
        }
        out->v = e.empty() ? std::string("false") : Tmp("bool", e);
        return Status::OK();
      }
      // value equality, as a hash set of floats gives it: -0.0 and +0.0 are one value, a NaN equals nothing (the probe adds
      // +0.0, which maps -0.0 to +0.0 and keeps NaNs NaN)
      const std::vector<uint64_t> vals = InListBitImages(vt, n.values());
      const bool is_fp = vt.id == kFloat || vt.id == kDouble;
      const std::string probe = is_fp ? "gdv_bits64(" + x.v + " + (" + vt.CType() + ")0)" : "gdv_bits64(" + x.v + ")";
      if (vals.empty()) {
        out->v = "false";
      } else if (vals.size() <= 8) {
        const std::string xb = Tmp("gdv_uint64", probe);
        std::string e;
        for (auto v : vals) {
          if (!e.empty()) e += " || ";
          e += "(" + xb + " == A.lit[" + std::to_string(LitSlot(v)) + "])";
        }
        out->v = Tmp("bool", e);
      } else {
        // sorted table in the constant block + branch-free binary search on the value's bit image
        std::string tab(reinterpret_cast<const char*>(vals.data()), vals.size() * 8);
        out->v = Tmp("bool", "gdv_in_sorted(" + probe + ", " + ByteTable(tab, "gdv_uint64") + ", " +
                                 std::to_string(vals.size()) + ")");
      }
      return Status::OK();
    }
  }
  return Status::CodeGenError("unknown node kind");
}

}  // namespace gdv::planner
