// C++ acceptance test of binary RESULTS through the drop-in gandiva:: API: unhex / unbase64 return an
// arrow::BinaryArray, hex / base64 take one, crc32 is an int64.  `--host-only`: the registry lists the signatures and the
// trees build (no GPU).  Without the flag the trees are evaluated on the GPU and compared with known answers
// (RFC 4648 §10's vectors, zlib's crc32("spark")), nulls included; a row that is not hex text is an execution error.
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

template <typename B>
std::shared_ptr<arrow::Array> MakeArr(const std::vector<const char*>& v) {  // nullptr: a null row
  B b;
  for (auto x : v) {
    if (x == nullptr) (void)b.AppendNull();
    else (void)b.Append(std::string(x));
  }
  return b.Finish().ValueOrDie();
}

int main(int argc, char** argv) {
  const bool host_only = argc > 1 && !std::strcmp(argv[1], "--host-only");
  auto fs = arrow::field("s", arrow::utf8()), fh = arrow::field("h", arrow::utf8()), fb = arrow::field("b", arrow::binary()),
       f64 = arrow::field("e", arrow::utf8());
  auto schema = arrow::schema({fs, fh, fb, f64});
  auto s = TreeExprBuilder::MakeField(fs), h = TreeExprBuilder::MakeField(fh), b = TreeExprBuilder::MakeField(fb),
       e = TreeExprBuilder::MakeField(f64);

  int found = 0;
  ExpressionRegistry registry;
  for (auto it = registry.function_signature_begin(); it != registry.function_signature_end(); ++it) {
    const std::string name = (*it).base_name();
    if ((name == "unhex" || name == "from_hex" || name == "unbase64") && (*it).ret_type()->Equals(arrow::binary())) found++;
    if ((name == "hex" || name == "base64") && (*it).param_types().size() == 1 && (*it).param_types()[0]->Equals(arrow::binary()) &&
        (*it).ret_type()->Equals(arrow::utf8()))
      found++;
  }
  CHECK(found == 5);

  auto unhex = TreeExprBuilder::MakeFunction("unhex", {h}, arrow::binary());
  CHECK(unhex->return_type()->Equals(arrow::binary()));
  ExpressionVector exprs = {
      TreeExprBuilder::MakeExpression(unhex, arrow::field("o0", arrow::binary())),
      TreeExprBuilder::MakeExpression(TreeExprBuilder::MakeFunction("unbase64", {e}, arrow::binary()), arrow::field("o1", arrow::binary())),
      TreeExprBuilder::MakeExpression(TreeExprBuilder::MakeFunction("hex", {b}, arrow::utf8()), arrow::field("o2", arrow::utf8())),
      TreeExprBuilder::MakeExpression(TreeExprBuilder::MakeFunction("base64", {s}, arrow::utf8()), arrow::field("o3", arrow::utf8())),
      TreeExprBuilder::MakeExpression(TreeExprBuilder::MakeFunction("crc32", {s}, arrow::int64()), arrow::field("o4", arrow::int64()))};
  if (host_only) {
    std::printf(failures ? "FAILED\n" : "OK (host-only)\n");
    return failures ? 1 : 0;
  }

  auto pool = arrow::default_memory_pool();
  auto batch = arrow::RecordBatch::Make(
      schema, 6,
      {MakeArr<arrow::StringBuilder>({"", "f", "fo", "foobar", nullptr, "spark"}),
       MakeArr<arrow::StringBuilder>({"", "66", "666F", "666f6F626172", nullptr, "00ff"}),
       MakeArr<arrow::BinaryBuilder>({"", "f", "fo", "foobar", nullptr, "\xff\x01"}),
       MakeArr<arrow::StringBuilder>({"", "Zg==", "Zm8=", "Zm9vYmFy", nullptr, "Zm9v"})});
  std::shared_ptr<Projector> p;
  CHECK_OK(Projector::Make(schema, exprs, &p));
  arrow::ArrayVector out;
  CHECK_OK(p->Evaluate(*batch, pool, &out));
  CHECK(out.size() == 5);
  if (out.size() == 5) {
    CHECK(out[0]->type_id() == arrow::Type::BINARY && out[1]->type_id() == arrow::Type::BINARY);
    CHECK(out[2]->type_id() == arrow::Type::STRING && out[3]->type_id() == arrow::Type::STRING);
    auto o0 = std::static_pointer_cast<arrow::BinaryArray>(out[0]), o1 = std::static_pointer_cast<arrow::BinaryArray>(out[1]);
    auto o2 = std::static_pointer_cast<arrow::StringArray>(out[2]), o3 = std::static_pointer_cast<arrow::StringArray>(out[3]);
    auto o4 = std::static_pointer_cast<arrow::Int64Array>(out[4]);
    const std::vector<std::string> plain = {"", "f", "fo", "foobar", "", std::string("\x00\xff", 2)};
    const std::vector<std::string> plain64 = {"", "f", "fo", "foobar", "", "foo"};
    const std::vector<std::string> hexes = {"", "66", "666F", "666F6F626172", "", "FF01"};
    const std::vector<std::string> b64 = {"", "Zg==", "Zm8=", "Zm9vYmFy", "", "c3Bhcms="};
    for (int i = 0; i < 6; i++) {
      const bool null = i == 4;
      CHECK(o0->IsNull(i) == null && o1->IsNull(i) == null && o2->IsNull(i) == null && o3->IsNull(i) == null && o4->IsNull(i) == null);
      if (null) continue;
      CHECK(o0->GetString(i) == plain[i]);
      CHECK(o1->GetString(i) == plain64[i]);
      CHECK(o2->GetString(i) == hexes[i]);
      CHECK(o3->GetString(i) == b64[i]);
    }
    CHECK(o4->Value(0) == 0 && o4->Value(5) == 2635321133ll);
  }
  // one row that is not hex text: an execution error, returned as a status
  auto bad = arrow::RecordBatch::Make(
      schema, 2,
      {MakeArr<arrow::StringBuilder>({"a", "b"}), MakeArr<arrow::StringBuilder>({"66", "6G"}), MakeArr<arrow::BinaryBuilder>({"a", "b"}),
       MakeArr<arrow::StringBuilder>({"Zg==", "Zg=="})});
  arrow::ArrayVector out2;
  CHECK(!p->Evaluate(*bad, pool, &out2).ok());
  std::printf(failures ? "FAILED\n" : "OK\n");
  return failures ? 1 : 0;
}
