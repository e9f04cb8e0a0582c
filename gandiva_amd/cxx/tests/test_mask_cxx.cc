// C++ acceptance test of the data-masking family through the drop-in gandiva:: API: mask (default and literal replacement
// characters), mask_first_n / mask_last_n (literal n), mask_show_first_n / mask_show_last_n (n from an int32 column), and a
// replacement that is not one ASCII byte refused by Projector::Make.  `--host-only`: the trees build and the registry lists the
// functions (no GPU).  Without the flag the projector is evaluated on the GPU and compared with known answers, null rows included.
#include <cstdio>
#include <cstdlib>
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

static std::shared_ptr<arrow::Array> Strings(const std::vector<const char*>& v) {  // nullptr: a null row
  arrow::StringBuilder b;
  for (auto x : v) {
    if (x == nullptr) (void)b.AppendNull();
    else (void)b.Append(std::string(x));
  }
  return b.Finish().ValueOrDie();
}

int main(int argc, char** argv) {
  const bool host_only = argc > 1 && !std::strcmp(argv[1], "--host-only");
  auto fs = arrow::field("s", arrow::utf8());
  auto fk = arrow::field("k", arrow::int32());
  auto schema = arrow::schema({fs, fk});
  auto s = TreeExprBuilder::MakeField(fs);
  auto k = TreeExprBuilder::MakeField(fk);
  auto str = [](const char* v) { return TreeExprBuilder::MakeStringLiteral(v); };
  auto i32 = [](int32_t v) { return TreeExprBuilder::MakeLiteral(v); };
  auto out = [](NodePtr n, const char* name) { return TreeExprBuilder::MakeExpression(n, arrow::field(name, arrow::utf8())); };
  auto fn = [](const char* name, NodeVector args) { return TreeExprBuilder::MakeFunction(name, args, arrow::utf8()); };
  ExpressionVector exprs = {out(fn("mask", {s}), "m"),
                            out(fn("mask", {s, str("U"), str("l"), str("#")}), "m4"),
                            out(fn("mask_first_n", {s, i32(4)}), "f"),
                            out(fn("mask_last_n", {s, i32(4)}), "l"),
                            out(fn("mask_show_first_n", {s, k}), "sf"),
                            out(fn("mask_show_last_n", {s, k}), "sl")};
  for (auto& e : exprs) CHECK(e != nullptr);
  // the registry lists the family
  int listed = 0;
  ExpressionRegistry registry;
  for (auto it = registry.function_signature_begin(); it != registry.function_signature_end(); ++it)
    if ((*it).base_name().compare(0, 4, "mask") == 0) listed++;
  CHECK(listed == 8);
  if (host_only) {
    std::printf(failures ? "FAILED\n" : "OK (host-only)\n");
    return failures ? 1 : 0;
  }

  auto pool = arrow::default_memory_pool();
  arrow::Int32Builder kb;
  (void)kb.AppendValues({2, 2, 1, 0, 2, 0});
  (void)kb.AppendNull();
  // Hello-123 | H é l l o   4 2 | é A | "" | null | a card number (n = 0) | a null n
  auto batch = arrow::RecordBatch::Make(schema, 7, {Strings({"Hello-123", "H\xc3\xa9llo 42", "\xc3\xa9" "A", "", nullptr, "Card 4556-7375-8689-9", "Ab1"}),
                                                     kb.Finish().ValueOrDie()});
  const std::vector<std::vector<std::string>> want = {
      {"Xxxxx-nnn", "X\xc3\xa9xxx nn", "\xc3\xa9" "X", "", "", "Xxxx nnnn-nnnn-nnnn-n", "Xxn"},
      {"Ullll-###", "U\xc3\xa9lll ##", "\xc3\xa9" "U", "", "", "Ulll ####-####-####-#", "Ul#"},
      {"Xxxxo-123", "X\xc3\xa9xxo 42", "\xc3\xa9" "X", "", "", "Xxxx 4556-7375-8689-9", "Xxn"},
      {"Hello-nnn", "H\xc3\xa9ll" "x nn", "\xc3\xa9" "X", "", "", "Card 4556-7375-86nn-n", "Xxn"},
      {"Hexxx-nnn", "H\xc3\xa9xxx nn", "\xc3\xa9" "X", "", "", "Xxxx nnnn-nnnn-nnnn-n", ""},
      {"Xxxxx-n23", "X\xc3\xa9xxx 42", "\xc3\xa9" "A", "", "", "Xxxx nnnn-nnnn-nnnn-n", ""}};

  std::shared_ptr<Projector> projector;
  CHECK_OK(Projector::Make(schema, exprs, &projector));
  arrow::ArrayVector got;
  if (projector) CHECK_OK(projector->Evaluate(*batch, pool, &got));
  CHECK(got.size() == want.size());
  if (got.size() == want.size()) {
    for (size_t e = 0; e < want.size(); e++) {
      auto col = std::static_pointer_cast<arrow::StringArray>(got[e]);
      for (int i = 0; i < 7; i++) {
        const bool null = i == 4 || (i == 6 && e >= 4);
        CHECK(col->IsNull(i) == null);
        if (!null && col->GetString(i) != want[e][i]) {
          std::printf("FAIL expression %zu row %d: '%s', want '%s'\n", e, i, col->GetString(i).c_str(), want[e][i].c_str());
          failures++;
        }
      }
    }
  }
  // a replacement of two bytes is refused when the projector is made, and the message names mask
  std::shared_ptr<Projector> refused;
  arrow::Status st = Projector::Make(schema, {out(fn("mask", {s, str("\xc3\xa9")}), "bad")}, &refused);
  CHECK(!st.ok() && st.ToString().find("mask") != std::string::npos);
  std::printf(failures ? "FAILED\n" : "OK\n");
  return failures ? 1 : 0;
}
