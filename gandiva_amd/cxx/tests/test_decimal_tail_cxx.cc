// C++ acceptance test of the decimal tail through the drop-in gandiva:: API: castDECIMAL of float64 / float32 / text,
// castDECIMALNullOnOverflow, nvl / greatest / least, is_distinct_from / is_not_distinct_from and the hash family over
// decimal128.  `--host-only`: the registry lists the fourteen signatures and the trees build (no GPU).  Without the flag
// the trees are evaluated on the GPU and compared with known answers; a text that is no number is an execution error, and
// nvl over two decimal types fails at Make.
#include <cstdio>
#include <cstring>
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
  auto d152 = arrow::decimal128(15, 2), d205 = arrow::decimal128(20, 5), d41 = arrow::decimal128(4, 1);
  auto fs = arrow::field("s", arrow::utf8()), fx = arrow::field("x", arrow::float64()), fd = arrow::field("d", d152),
       fe = arrow::field("e", d152), fg = arrow::field("g", d205);
  auto schema = arrow::schema({fs, fx, fd, fe, fg});
  auto s = TreeExprBuilder::MakeField(fs), x = TreeExprBuilder::MakeField(fx), d = TreeExprBuilder::MakeField(fd),
       e = TreeExprBuilder::MakeField(fe), g = TreeExprBuilder::MakeField(fg);

  int found = 0;
  ExpressionRegistry registry;
  for (auto it = registry.function_signature_begin(); it != registry.function_signature_end(); ++it) {
    const std::string name = (*it).base_name();
    const auto& params = (*it).param_types();
    const bool dec0 = !params.empty() && params[0]->id() == arrow::Type::DECIMAL128;
    const bool ret_dec = (*it).ret_type()->id() == arrow::Type::DECIMAL128;
    if (name == "castDECIMAL" && params.size() == 1 && ret_dec &&
        (params[0]->Equals(arrow::float64()) || params[0]->Equals(arrow::float32()) || params[0]->Equals(arrow::utf8())))
      found++;
    if (name == "castDECIMALNullOnOverflow" && dec0 && ret_dec) found++;
    if ((name == "nvl" || name == "greatest" || name == "least") && dec0 && params.size() == 2 && ret_dec) found++;
    if ((name == "is_distinct_from" || name == "is_not_distinct_from") && dec0 && params.size() == 2) found++;
    if ((name == "hash" || name == "hash32" || name == "hash64") && dec0) found++;
    CHECK(!(dec0 && (name == "hash32AsDouble" || name == "hash64AsDouble")));
  }
  CHECK(found == 14);

  auto fn = [](const char* name, NodeVector args, std::shared_ptr<arrow::DataType> t) { return TreeExprBuilder::MakeFunction(name, args, t); };
  auto cast_s = fn("castDECIMAL", {s}, d152);
  CHECK(cast_s->return_type()->Equals(d152));
  ExpressionVector exprs = {
      TreeExprBuilder::MakeExpression(cast_s, arrow::field("o0", d152)),
      TreeExprBuilder::MakeExpression(fn("castDECIMAL", {x}, d152), arrow::field("o1", d152)),
      TreeExprBuilder::MakeExpression(fn("castDECIMALNullOnOverflow", {g}, d41), arrow::field("o2", d41)),
      TreeExprBuilder::MakeExpression(fn("nvl", {d, e}, d152), arrow::field("o3", d152)),
      TreeExprBuilder::MakeExpression(fn("greatest", {d, e}, d152), arrow::field("o4", d152)),
      TreeExprBuilder::MakeExpression(fn("least", {d, e}, d152), arrow::field("o5", d152)),
      TreeExprBuilder::MakeExpression(fn("is_distinct_from", {d, g}, arrow::boolean()), arrow::field("o6", arrow::boolean())),
      TreeExprBuilder::MakeExpression(fn("is_not_distinct_from", {d, g}, arrow::boolean()), arrow::field("o7", arrow::boolean())),
      TreeExprBuilder::MakeExpression(fn("hash64", {d}, arrow::int64()), arrow::field("o8", arrow::int64())),
      TreeExprBuilder::MakeExpression(fn("hash32", {d, TreeExprBuilder::MakeLiteral((int32_t)7)}, arrow::int32()), arrow::field("o9", arrow::int32()))};
  // nvl over two decimal types: refused when the projector is made, before anything is compiled
  {
    std::shared_ptr<Projector> bad;
    auto st = Projector::Make(schema, {TreeExprBuilder::MakeExpression(fn("nvl", {d, g}, d152), arrow::field("z", d152))}, &bad);
    CHECK(!st.ok() && st.ToString().find("precision and scale") != std::string::npos);
  }
  if (host_only) {
    std::printf(failures ? "FAILED\n" : "OK (host-only)\n");
    return failures ? 1 : 0;
  }

  auto pool = arrow::default_memory_pool();
  auto dec_array = [](std::shared_ptr<arrow::DataType> t, const std::vector<int64_t>& v, const std::vector<bool>& valid) {
    arrow::Decimal128Builder b(t);
    for (size_t i = 0; i < v.size(); i++) {
      if (valid[i]) (void)b.Append(arrow::Decimal128(v[i]));
      else (void)b.AppendNull();
    }
    return b.Finish().ValueOrDie();
  };
  arrow::StringBuilder sb;
  for (const char* t : {"1.005", "-.5e1", "12e3", "0.004"}) (void)sb.Append(std::string(t));
  arrow::DoubleBuilder xb;
  for (double v : {1.25, -2.5, 1e300, 0.125}) (void)xb.Append(v);
  const std::vector<bool> all = {true, true, true, true};
  auto batch = arrow::RecordBatch::Make(
      schema, 4,
      {sb.Finish().ValueOrDie(), xb.Finish().ValueOrDie(), dec_array(d152, {100, -250, 0, 7}, {true, false, true, false}),
       dec_array(d152, {99, 300, 5, 8}, {true, true, false, false}), dec_array(d205, {100000, 1, 99950000, -99949999}, all)});
  std::shared_ptr<Projector> p;
  CHECK_OK(Projector::Make(schema, exprs, &p));
  arrow::ArrayVector out;
  if (p) CHECK_OK(p->Evaluate(*batch, pool, &out));
  CHECK(out.size() == 10);
  if (out.size() == 10) {
    auto dec = [&](int k, int i) { return arrow::Decimal128(std::static_pointer_cast<arrow::Decimal128Array>(out[k])->GetValue(i)); };
    const int64_t from_text[4] = {101, -500, 1200000, 0}, from_double[4] = {125, -250, 0, 13};
    for (int i = 0; i < 4; i++) {
      CHECK(!out[0]->IsNull(i) && dec(0, i) == arrow::Decimal128(from_text[i]));
      CHECK(!out[1]->IsNull(i) && dec(1, i) == arrow::Decimal128(from_double[i]));
    }
    // g at scale 5 -> decimal(4, 1): 1.00000 -> 1.0; 0.00001 -> 0.0; 999.50000 -> 999.5; -999.49999 -> -999.5
    CHECK(dec(2, 0) == arrow::Decimal128(10) && dec(2, 1) == arrow::Decimal128(0) && dec(2, 2) == arrow::Decimal128(9995) &&
          dec(2, 3) == arrow::Decimal128(-9995) && out[2]->null_count() == 0);
    CHECK(dec(3, 0) == arrow::Decimal128(100) && dec(3, 1) == arrow::Decimal128(300) && dec(3, 2) == arrow::Decimal128(0) && out[3]->IsNull(3));
    CHECK(dec(4, 0) == arrow::Decimal128(100) && out[4]->IsNull(1) && out[4]->IsNull(2) && out[4]->IsNull(3));
    CHECK(dec(5, 0) == arrow::Decimal128(99) && out[5]->null_count() == 3);
    auto o6 = std::static_pointer_cast<arrow::BooleanArray>(out[6]), o7 = std::static_pointer_cast<arrow::BooleanArray>(out[7]);
    // d: 1.00, NULL, 0.00, NULL against g: 1.00000, 0.00001, 999.5, -999.49999
    const bool distinct[4] = {false, true, true, true};
    for (int i = 0; i < 4; i++) CHECK(!o6->IsNull(i) && !o7->IsNull(i) && o6->Value(i) == distinct[i] && o7->Value(i) == !distinct[i]);
    auto o8 = std::static_pointer_cast<arrow::Int64Array>(out[8]);
    auto o9 = std::static_pointer_cast<arrow::Int32Array>(out[9]);
    CHECK(out[8]->null_count() == 0 && out[9]->null_count() == 0);
    CHECK(o8->Value(1) == 0 && o8->Value(3) == 0 && o9->Value(1) == 7 && o9->Value(3) == 7);   // NULL hashes to the seed
    CHECK(o8->Value(0) != 0 && o8->Value(0) != o8->Value(2));
  }
  // a text that is no number: an execution error, returned as a status
  arrow::StringBuilder sb2;
  for (const char* t : {"1.0", "1,5", "2", "3"}) (void)sb2.Append(std::string(t));
  auto bad = arrow::RecordBatch::Make(schema, 4, {sb2.Finish().ValueOrDie(), batch->column(1), batch->column(2), batch->column(3), batch->column(4)});
  arrow::ArrayVector out2;
  if (p) CHECK(!p->Evaluate(*bad, pool, &out2).ok());
  std::printf(failures ? "FAILED\n" : "OK\n");
  return failures ? 1 : 0;
}
