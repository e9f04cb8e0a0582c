// C++ acceptance test of the numeric tail through the drop-in gandiva:: API: round(x, 2) (literal scale), atan2(y, x) and
// pmod(a, n) (n from an int32 column).  `--host-only`: the trees build and the registry lists the functions (no GPU).  Without
// the flag the projector is evaluated on the GPU and compared with known answers, null rows included.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "arrow/api.h"
#include "gandiva/expression_registry.h"
#include "gandiva/projector.h"
#include "gandiva/tree_expr_builder.h"

using namespace gandiva;

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); failures++; } \
  } while (0)
#define CHECK_OK(expr)                                                     \
  do {                                                                     \
    arrow::Status _s = (expr);                                             \
    if (!_s.ok()) { std::printf("FAIL %s:%d  %s -> %s\n", __FILE__, __LINE__, #expr, _s.ToString().c_str()); failures++; } \
  } while (0)

int main(int argc, char** argv) {
  const bool host_only = argc > 1 && !std::strcmp(argv[1], "--host-only");
  auto fx = arrow::field("x", arrow::float64());
  auto fy = arrow::field("y", arrow::float64());
  auto fa = arrow::field("a", arrow::int32());
  auto fn_ = arrow::field("n", arrow::int32());
  auto schema = arrow::schema({fx, fy, fa, fn_});
  auto x = TreeExprBuilder::MakeField(fx), y = TreeExprBuilder::MakeField(fy);
  auto a = TreeExprBuilder::MakeField(fa), n = TreeExprBuilder::MakeField(fn_);
  auto f64 = arrow::float64();
  auto i32 = arrow::int32();
  ExpressionVector exprs = {
      TreeExprBuilder::MakeExpression(TreeExprBuilder::MakeFunction("round", {x, TreeExprBuilder::MakeLiteral((int32_t)2)}, f64), arrow::field("r", f64)),
      TreeExprBuilder::MakeExpression(TreeExprBuilder::MakeFunction("atan2", {y, x}, f64), arrow::field("t", f64)),
      TreeExprBuilder::MakeExpression(TreeExprBuilder::MakeFunction("pmod", {a, n}, i32), arrow::field("p", i32))};
  for (auto& e : exprs) CHECK(e != nullptr);
  // the registry lists the family
  const std::set<std::string> names = {"sin", "cos", "tan", "asin", "acos", "atan", "sinh", "cosh", "tanh", "cot", "degrees", "radians", "atan2",
                                       "sign", "pmod", "shift_left", "shift_right", "shift_right_unsigned", "gcd", "lcm"};
  int listed = 0, round_with_scale = 0;
  ExpressionRegistry registry;
  for (auto it = registry.function_signature_begin(); it != registry.function_signature_end(); ++it) {
    if (names.count((*it).base_name())) listed++;
    if ((*it).base_name() == "round" && (*it).param_types().size() == 2 && (*it).param_types()[0]->id() != arrow::Type::DECIMAL128) round_with_scale++;
  }
  CHECK(listed == 12 * 4 + 1 + 4 + 2 + 6 + 2);
  CHECK(round_with_scale == 4);
  if (host_only) {
    std::printf(failures ? "FAILED\n" : "OK (host-only)\n");
    return failures ? 1 : 0;
  }

  auto pool = arrow::default_memory_pool();
  arrow::DoubleBuilder xb, yb;
  arrow::Int32Builder ab, nb;
  (void)xb.AppendValues({2.5, -0.125, 1e308, 1.0, -1.0, 0.0});
  (void)xb.AppendNull();
  (void)yb.AppendValues({0.0, 1.0, 0.0, 1.0, -0.0, -0.0});
  (void)yb.AppendNull();
  (void)ab.AppendValues({-7, 7, 5, -2147483647 - 1, 0, 6});
  (void)ab.AppendNull();
  (void)nb.AppendValues({3, -3, 0, -1, 5, 3, 3});
  auto batch = arrow::RecordBatch::Make(schema, 7, {xb.Finish().ValueOrDie(), yb.Finish().ValueOrDie(), ab.Finish().ValueOrDie(), nb.Finish().ValueOrDie()});
  const double pi = 3.14159265358979323846;
  const std::vector<double> want_r = {2.5, -0.13, 1e308, 1.0, -1.0, 0.0};
  const std::vector<double> want_t = {0.0, 1.695151321341658, 0.0, pi / 4, -pi, -0.0};   // row 1: atan2(1, -0.125)
  const std::vector<int32_t> want_p = {2, -2, 5, 0, 0, 0};

  std::shared_ptr<Projector> projector;
  CHECK_OK(Projector::Make(schema, exprs, &projector));
  arrow::ArrayVector got;
  if (projector) CHECK_OK(projector->Evaluate(*batch, pool, &got));
  CHECK(got.size() == 3);
  if (got.size() == 3) {
    auto r = std::static_pointer_cast<arrow::DoubleArray>(got[0]);
    auto t = std::static_pointer_cast<arrow::DoubleArray>(got[1]);
    auto p = std::static_pointer_cast<arrow::Int32Array>(got[2]);
    for (int i = 0; i < 6; i++) {
      CHECK(!r->IsNull(i) && !t->IsNull(i) && !p->IsNull(i));
      if (r->Value(i) != want_r[i] || std::signbit(r->Value(i)) != std::signbit(want_r[i])) {
        std::printf("FAIL round row %d: %.17g, want %.17g\n", i, r->Value(i), want_r[i]);
        failures++;
      }
      const double tol = std::fabs(want_t[i]) * 4.5e-16;   // 2 ulp: the library's atan2
      if (std::fabs(t->Value(i) - want_t[i]) > tol || std::signbit(t->Value(i)) != std::signbit(want_t[i])) {
        std::printf("FAIL atan2 row %d: %.17g, want %.17g\n", i, t->Value(i), want_t[i]);
        failures++;
      }
      if (p->Value(i) != want_p[i]) {
        std::printf("FAIL pmod row %d: %d, want %d\n", i, p->Value(i), want_p[i]);
        failures++;
      }
    }
    CHECK(r->IsNull(6) && t->IsNull(6) && p->IsNull(6));
  }
  std::printf(failures ? "FAILED\n" : "OK\n");
  return failures ? 1 : 0;
}
