#include "gdv_planner_internal.h"

namespace gdv {

namespace {

bool MaterialisesBytes(const Node& n, bool utf8_case) {
  if (n.kind() != NodeKind::kFunction) return false;
  auto& fn = static_cast<const FunctionNode&>(n);
  const std::string& f = fn.name();
  if (utf8_case && (f == "upper" || f == "lower")) return true;  // GDV_UTF8_CASE=1: values of their own kind
  if (f == "concat" || f == "concatOperator" || f == "lpad" || f == "rpad" || f == "reverse" || f == "replace" || f == "initcap" ||
      f == "hashSHA256" || f == "sha256" || f == "hashSHA1" || f == "sha1" || f == "sha" || f == "hashMD5" || f == "md5" ||
      f == "repeat" || f == "space" || f == "translate" || f == "mask" || f == "mask_first_n" || f == "mask_last_n" ||
      f == "mask_show_first_n" || f == "mask_show_last_n" || (planner::FnTraits(f) & planner::kFnEncode) != 0)
    return true;
  return f == "castVARCHAR" && !fn.children().empty() && !fn.children()[0]->return_type().is_varlen();
}

struct Stager {
  const Schema& schema;
  StagedExpressions* out;
  bool utf8_case;  // CodegenOptions::utf8_case of this Make
  std::map<std::string, NodePtr> field_of;  // hoisted sub-tree (cache key) -> its temporary field

  // `guard` (may be null): the condition under which the caller's tree evaluates `n` at all — the
  // enclosing if/else branches and short-circuit AND / OR children.  The first stage evaluates
  // every row, so a guarded sub-tree is hoisted as `if (guard) n else NULL`: functions that can
  // raise (castVARCHAR(a / b, n), replace ...) then run only where the caller's tree would have
  // run them (round-2 advisor: `if (b != 0) upper(castVARCHAR(a / b, 10)) else 'x'` raised).
  NodePtr Hoist(const NodePtr& sub, const NodePtr& guard) {
    NodePtr n = sub;
    if (guard) {
      Literal null_value;
      null_value.is_null = true;
      n = std::make_shared<IfNode>(guard, sub, std::make_shared<LiteralNode>(sub->return_type(), null_value),
                                   sub->return_type());
    }
    std::string key;
    n->AppendKey(&key);
    auto it = field_of.find(key);
    if (it != field_of.end()) return it->second;
    Field f;
    f.name = "__gdv_stage" + std::to_string(out->pre.size());
    for (bool clash = true; clash;) {  // fields are bound by name: stay clear of the caller's
      clash = false;
      for (auto& g : out->schema) clash = clash || g.name == f.name;
      if (clash) f.name += "_";
    }
    f.type = n->return_type();
    f.nullable = true;
    out->pre.push_back(std::make_shared<Expression>(n, f));
    out->schema.push_back(f);
    NodePtr field = std::make_shared<FieldNode>(f);
    field_of[key] = field;
    return field;
  }
  static NodePtr AndGuard(const NodePtr& a, const NodePtr& b) {
    if (!a) return b;
    if (!b) return a;
    return std::make_shared<BooleanNode>(BooleanNode::kAnd, NodeVector{a, b});
  }
  static NodePtr Test(const char* fn, const NodePtr& x) {  // istrue / isnottrue / isnotfalse: never null
    return std::make_shared<FunctionNode>(fn, NodeVector{x}, boolean());
  }
  // `takes_bytes`: the parent is an output root or a concat — it can take a materialising child as it is
  NodePtr Rewrite(const NodePtr& n, bool takes_bytes, const NodePtr& guard) {
    if (MaterialisesBytes(*n, utf8_case) && !takes_bytes) return Hoist(n, guard);  // (its own sub-tree is the first stage's business)
    switch (n->kind()) {
      case NodeKind::kFunction: {
        auto& fn = static_cast<const FunctionNode&>(*n);
        const bool is_concat = fn.name() == "concat" || fn.name() == "concatOperator";
        NodeVector kids;
        bool changed = false;
        for (auto& c : fn.children()) {
          kids.push_back(Rewrite(c, is_concat, guard));
          changed |= kids.back() != c;
        }
        return changed ? std::make_shared<FunctionNode>(fn.name(), kids, fn.return_type()) : n;
      }
      case NodeKind::kIf: {
        // guards are built from the caller's ORIGINAL condition: it must be evaluable by the first
        // stage, which knows nothing of the temporaries of this one
        auto& i = static_cast<const IfNode&>(*n);
        // (`if (c) <materialised> else NULL` is something the kernel takes as it is wherever it takes
        // a materialised value — CodeGen::Gen, kIf — which is also what a guarded hoist looks like:
        // its branch inherits `takes_bytes`, or the first stage would hoist it again, for ever)
        NodePtr c = Rewrite(i.condition(), false, guard);
        NodePtr t = Rewrite(i.then_node(), takes_bytes && planner::IsNullLiteral(*i.else_node()),
                            AndGuard(guard, Test("istrue", i.condition())));
        NodePtr e = Rewrite(i.else_node(), takes_bytes && planner::IsNullLiteral(*i.then_node()),
                            AndGuard(guard, Test("isnottrue", i.condition())));
        if (c == i.condition() && t == i.then_node() && e == i.else_node()) return n;
        return std::make_shared<IfNode>(c, t, e, i.return_type());
      }
      case NodeKind::kBoolean: {
        // left-to-right short circuit: child k of an AND runs while no earlier child was (valid,
        // false); of an OR, while none was (valid, true)
        auto& b = static_cast<const BooleanNode&>(*n);
        const char* still = b.op() == BooleanNode::kAnd ? "isnotfalse" : "isnottrue";
        NodeVector kids;
        bool changed = false;
        NodePtr g = guard;
        for (auto& c : b.children()) {
          kids.push_back(Rewrite(c, false, g));
          changed |= kids.back() != c;
          g = AndGuard(g, Test(still, c));
        }
        return changed ? std::make_shared<BooleanNode>(b.op(), kids) : n;
      }
      case NodeKind::kIn: {
        auto& in = static_cast<const InNode&>(*n);
        NodePtr e = Rewrite(in.eval(), false, guard);
        return e == in.eval() ? n : std::make_shared<InNode>(e, in.value_type(), in.values());
      }
      default:
        return n;
    }
  }
};

}  // namespace

void StageMaterialisedValues(const Schema& schema, const std::vector<ExpressionPtr>& exprs,
                             StagedExpressions* out, const CodegenOptions& opts) {
  out->pre.clear();
  out->main.clear();
  out->schema = schema;
  Stager st{schema, out, opts.utf8_case, {}};
  for (auto& e : exprs) {
    if (!e || !e->root()) {
      out->main.push_back(e);
      continue;
    }
    NodePtr root = st.Rewrite(e->root(), true, nullptr);
    out->main.push_back(root == e->root() ? e : std::make_shared<Expression>(root, e->result()));
  }
}

}  // namespace gdv
