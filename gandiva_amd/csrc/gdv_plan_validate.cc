#include "gdv_planner_internal.h"

namespace gdv {

bool planner::ResolveFunction(const FunctionNode& n, const FunctionDef** def, DataType* ret) {
  std::vector<DataType> params;
  for (auto& c : n.children()) params.push_back(c->return_type());
  const FunctionDef* d = FunctionRegistry::Get().Lookup(n.name(), params);
  if (d == nullptr) return false;
  *def = d;
  *ret = d->ret;
  if (d->flags & kDecimalResult) {
    DecimalOp op = DecimalOp::kAdd;
    if (n.name() == "subtract") op = DecimalOp::kSubtract;
    else if (n.name() == "multiply") op = DecimalOp::kMultiply;
    else if (n.name() == "divide") op = DecimalOp::kDivide;
    else if (n.name() == "mod") op = DecimalOp::kMod;
    *ret = DecimalResultType(op, params[0], params[1]);
  }
  return true;
}

using planner::ResolveFunction;

namespace {

Status ValidateNode(const Schema& schema, const Node& node);

Status ValidateField(const Schema& schema, const FieldNode& n) {
  for (auto& f : schema) {
    if (f.name == n.field().name) {
      if (f.type != n.field().type) {
        return Status::ValidationError("Field definition in schema " + f.name + ": " +
                                       f.type.ToString() + " different from field in expression " +
                                       n.field().name + ": " + n.field().type.ToString());
      }
      return Status::OK();
    }
  }
  return Status::ValidationError("Field " + n.field().name + " not in schema.");
}

Status ValidateFunction(const Schema& schema, const FunctionNode& n) {
  for (auto& c : n.children()) GDV_RETURN_NOT_OK(ValidateNode(schema, *c));
  const FunctionDef* def = nullptr;
  DataType ret;
  if (!ResolveFunction(n, &def, &ret)) {
    // next_day(t, text) / date_trunc(text, t) that was no literal name when the node was built
    const std::string refusal = CalendarNameRefusal(n);
    if (!refusal.empty()) return Status::CodeGenError(refusal);
    return Status::ValidationError("Function " + n.ToString() + " not supported yet. ");
  }
  if (ret != n.return_type()) {
    // decimal results declared by the caller win when only precision/scale differ
    if (!(ret.id == kDecimal128 && n.return_type().id == kDecimal128 &&
          !(def->flags & kDecimalResult))) {
      return Status::ValidationError("Function " + n.name() + " returns " + ret.ToString() +
                                     " but the expression declares " +
                                     n.return_type().ToString());
    }
  }
  if (def->flags & kSameDecimalType) {  // nvl / greatest / least over decimals: the value is one of the arguments, as it is
    for (auto& c : n.children()) {
      if (c->return_type() != n.return_type())
        return Status::ValidationError("Function " + n.name() + " takes decimal arguments of the result's precision and scale: " +
                                       c->return_type().ToString() + " given, " + n.return_type().ToString() + " declared");
    }
  }
  if (def->flags & kPatternArg) {
    if (n.children().size() < 2 || n.children()[1]->kind() != NodeKind::kLiteral) {
      return Status::ValidationError("'" + n.name() + "' function requires a literal as the last parameter");
    }
  }
  if (def->flags & kDateFormatArg) {  // [to_date_holder.cc ToDateHolder::Make's two messages, as recalled]
    if (n.children()[1]->kind() != NodeKind::kLiteral)
      return Status::ValidationError("'" + n.name() + "' function requires a literal as the second parameter");
    if (n.children().size() == 3 && n.children()[2]->kind() != NodeKind::kLiteral)
      return Status::ValidationError("'" + n.name() + "' function requires a int literal as the third parameter");
  }
  return Status::OK();
}

Status ValidateNode(const Schema& schema, const Node& node) {
  switch (node.kind()) {
    case NodeKind::kField:
      return ValidateField(schema, static_cast<const FieldNode&>(node));
    case NodeKind::kLiteral:
      return Status::OK();
    case NodeKind::kFunction:
      return ValidateFunction(schema, static_cast<const FunctionNode&>(node));
    case NodeKind::kIf: {
      auto& n = static_cast<const IfNode&>(node);
      GDV_RETURN_NOT_OK(ValidateNode(schema, *n.condition()));
      GDV_RETURN_NOT_OK(ValidateNode(schema, *n.then_node()));
      GDV_RETURN_NOT_OK(ValidateNode(schema, *n.else_node()));
      if (n.condition()->return_type().id != kBool)
        return Status::ValidationError("condition must be of boolean type, found type " +
                                       n.condition()->return_type().ToString());
      if (n.then_node()->return_type() != n.return_type())
        return Status::ValidationError("return type of if " + n.return_type().ToString() +
                                       " and then " + n.then_node()->return_type().ToString() +
                                       " not matching.");
      if (n.else_node()->return_type() != n.return_type())
        return Status::ValidationError("return type of if " + n.return_type().ToString() +
                                       " and else " + n.else_node()->return_type().ToString() +
                                       " not matching.");
      return Status::OK();
    }
    case NodeKind::kBoolean: {
      auto& n = static_cast<const BooleanNode&>(node);
      if (n.children().size() < 2)
        return Status::ValidationError("Boolean expression has " +
                                       std::to_string(n.children().size()) +
                                       " children, expected atleast two");
      for (auto& c : n.children()) {
        GDV_RETURN_NOT_OK(ValidateNode(schema, *c));
        if (c->return_type().id != kBool)
          return Status::ValidationError("Boolean expression has a child with return type " +
                                         c->return_type().ToString() + ", expected return type boolean");
      }
      return Status::OK();
    }
    case NodeKind::kIn: {
      auto& n = static_cast<const InNode&>(node);
      GDV_RETURN_NOT_OK(ValidateNode(schema, *n.eval()));
      if (n.eval()->return_type() != n.value_type())
        // message fragment pinned by test_gandiva.py:160-161
        return Status::ValidationError("Evaluation expression for IN clause returns " +
                                       n.eval()->return_type().ToString() +
                                       " values are of type" + n.value_type().ToString());
      return Status::OK();
    }
  }
  return Status::OK();
}

}  // namespace

Status ValidateExpression(const Schema& schema, const Expression& expr) {
  if (!expr.root()) return Status::ValidationError("Root node cannot be null");
  GDV_RETURN_NOT_OK(ValidateNode(schema, *expr.root()));
  if (expr.root()->return_type() != expr.result().type) {
    return Status::ValidationError("Return type of root node " +
                                   expr.root()->return_type().ToString() +
                                   " does not match that of expression " +
                                   expr.result().type.ToString());
  }
  return Status::OK();
}

}  // namespace gdv
