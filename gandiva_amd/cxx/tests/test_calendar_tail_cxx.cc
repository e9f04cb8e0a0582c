// C++ acceptance test of the calendar tail through the drop-in gandiva:: API: months_between(e, s), next_day(e, 'tue')
// (a literal day name), add_months(s, n) (n from an int32 column), date_trunc('MoNtH', e) and year(e).  `--host-only`:
// the trees build, the registry lists the functions and Make refuses a per-row day name (no GPU).  Without the flag the
// projector is evaluated on the GPU and compared with known answers, null rows included.
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

static const int64_t MS = 86400000LL;
// days since 1970-01-01 of the dates the test uses
static const int64_t D_1996_10_30 = 9799, D_1997_02_28 = 9920, D_1997_02_01 = 9893, D_1997_03_04 = 9924, D_2015_01_14 = 16449,
                     D_2015_01_20 = 16455, D_2015_01_01 = 16436, D_2015_01_31 = 16466, D_2015_02_28 = 16494, D_2016_01_14 = 16814;

int main(int argc, char** argv) {
  const bool host_only = argc > 1 && !std::strcmp(argv[1], "--host-only");
  auto ts = arrow::timestamp(arrow::TimeUnit::MILLI);
  auto f64 = arrow::float64(), i32 = arrow::int32(), i64 = arrow::int64(), d64 = arrow::date64();
  auto fe = arrow::field("e", ts), fs = arrow::field("s", ts), fn_ = arrow::field("n", i32), fw = arrow::field("w", arrow::utf8());
  auto schema = arrow::schema({fe, fs, fn_, fw});
  auto e = TreeExprBuilder::MakeField(fe), s = TreeExprBuilder::MakeField(fs), n = TreeExprBuilder::MakeField(fn_);
  ExpressionVector exprs = {
      TreeExprBuilder::MakeExpression(TreeExprBuilder::MakeFunction("months_between", {e, s}, f64), arrow::field("m", f64)),
      TreeExprBuilder::MakeExpression(TreeExprBuilder::MakeFunction("next_day", {e, TreeExprBuilder::MakeStringLiteral("tue")}, d64), arrow::field("d", d64)),
      TreeExprBuilder::MakeExpression(TreeExprBuilder::MakeFunction("add_months", {s, n}, ts), arrow::field("a", ts)),
      TreeExprBuilder::MakeExpression(TreeExprBuilder::MakeFunction("date_trunc", {TreeExprBuilder::MakeStringLiteral("MoNtH"), e}, ts), arrow::field("t", ts)),
      TreeExprBuilder::MakeExpression(TreeExprBuilder::MakeFunction("year", {e}, i64), arrow::field("y", i64))};
  for (auto& x : exprs) CHECK(x != nullptr);
  // the registry lists the family
  const std::set<std::string> names = {"months_between", "next_day", "add_months", "year", "month", "day", "dayofmonth", "dayofyear", "dayofweek",
                                       "quarter", "hour", "minute", "second"};
  int listed = 0;
  ExpressionRegistry registry;
  for (auto it = registry.function_signature_begin(); it != registry.function_signature_end(); ++it)
    if (names.count((*it).base_name())) listed++;
  CHECK(listed == 2 + 2 + 4 + 7 * 3 + 3 * 4);
  // a per-row day name is refused when the projector is made, and the message says what is taken
  {
    auto per_row = TreeExprBuilder::MakeExpression(TreeExprBuilder::MakeFunction("next_day", {e, TreeExprBuilder::MakeField(fw)}, d64), arrow::field("d", d64));
    std::shared_ptr<Projector> refused;
    arrow::Status st = Projector::Make(schema, {per_row}, &refused);
    CHECK(!st.ok() && st.ToString().find("next_day") != std::string::npos && st.ToString().find("SUN MON TUE") != std::string::npos);
  }
  if (host_only) {
    std::printf(failures ? "FAILED\n" : "OK (host-only)\n");
    return failures ? 1 : 0;
  }

  auto pool = arrow::default_memory_pool();
  arrow::TimestampBuilder eb(ts, pool), sb(ts, pool);
  arrow::Int32Builder nb;
  arrow::StringBuilder wb;
  const int64_t half_past_ten = 37800000LL;
  (void)eb.AppendValues({D_1997_02_28 * MS + half_past_ten, D_2015_01_14 * MS, D_2015_02_28 * MS + 5, D_2015_01_20 * MS + MS - 1});
  (void)eb.AppendNull();
  (void)sb.AppendValues({D_1996_10_30 * MS, D_2015_01_14 * MS + 77, D_2015_01_31 * MS + 9, D_2015_01_31 * MS + 9});
  (void)sb.AppendNull();
  (void)nb.AppendValues({0, 12, 1, -2147483647 - 1, 3});
  (void)wb.AppendValues({"tue", "tue", "tue", "tue", "tue"});
  auto batch = arrow::RecordBatch::Make(schema, 5, {eb.Finish().ValueOrDie(), sb.Finish().ValueOrDie(), nb.Finish().ValueOrDie(), wb.Finish().ValueOrDie()});
  const std::vector<double> want_m = {4.0 + (-2.0 + 0.4375) / 31.0, 0.0, 1.0, 0.0 + (-11.0 + (double)(MS - 1 - 9) / 86400000.0) / 31.0};
  const std::vector<int64_t> want_d = {D_1997_03_04 * MS, D_2015_01_20 * MS, (D_2015_02_28 + 3) * MS, (D_2015_01_20 + 7) * MS};
  const std::vector<int64_t> want_t = {D_1997_02_01 * MS, D_2015_01_01 * MS, (D_2015_02_28 - 27) * MS, D_2015_01_01 * MS};
  const std::vector<int64_t> want_y = {1997, 2015, 2015, 2015};

  std::shared_ptr<Projector> projector;
  CHECK_OK(Projector::Make(schema, exprs, &projector));
  arrow::ArrayVector got;
  if (projector) CHECK_OK(projector->Evaluate(*batch, pool, &got));
  CHECK(got.size() == 5);
  if (got.size() == 5) {
    auto m = std::static_pointer_cast<arrow::DoubleArray>(got[0]);
    auto d = std::static_pointer_cast<arrow::Date64Array>(got[1]);
    auto a = std::static_pointer_cast<arrow::TimestampArray>(got[2]);
    auto t = std::static_pointer_cast<arrow::TimestampArray>(got[3]);
    auto y = std::static_pointer_cast<arrow::Int64Array>(got[4]);
    for (int i = 0; i < 4; i++) {
      CHECK(!m->IsNull(i) && !d->IsNull(i) && !a->IsNull(i) && !t->IsNull(i) && !y->IsNull(i));
      if (m->Value(i) != want_m[i]) {
        std::printf("FAIL months_between row %d: %.17g, want %.17g\n", i, m->Value(i), want_m[i]);
        failures++;
      }
      if (d->Value(i) != want_d[i] || t->Value(i) != want_t[i] || y->Value(i) != want_y[i]) {
        std::printf("FAIL row %d: next_day %lld (want %lld), date_trunc %lld (want %lld), year %lld (want %lld)\n", i, (long long)d->Value(i),
                    (long long)want_d[i], (long long)t->Value(i), (long long)want_t[i], (long long)y->Value(i), (long long)want_y[i]);
        failures++;
      }
    }
    // add_months: unchanged, a year on, Jan 31 -> Feb 28 (clamped); row 3 (INT32_MIN months) only has to be there
    CHECK(a->Value(0) == D_1996_10_30 * MS && a->Value(1) == D_2016_01_14 * MS + 77 && a->Value(2) == D_2015_02_28 * MS + 9);
    CHECK(m->IsNull(4) && d->IsNull(4) && a->IsNull(4) && t->IsNull(4) && y->IsNull(4));
  }
  std::printf(failures ? "FAILED\n" : "OK\n");
  return failures ? 1 : 0;
}
