// C++ acceptance test of GDV_UTF8_CASE=1 through the drop-in gandiva:: API: the variable is read at Projector::Make, so a
// projector made with it set maps upper / lower through utf8proc's simple case map and one made without it keeps the ASCII
// map, in the same process.  `--host-only`: the trees build (no GPU).  Without the flag both projectors are evaluated on the
// GPU and compared with known answers, a null row included; a row that is not UTF-8 is an execution error only with the option.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "arrow/api.h"
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
  auto schema = arrow::schema({fs});
  auto s = TreeExprBuilder::MakeField(fs);
  ExpressionVector exprs = {
      TreeExprBuilder::MakeExpression(TreeExprBuilder::MakeFunction("upper", {s}, arrow::utf8()), arrow::field("up", arrow::utf8())),
      TreeExprBuilder::MakeExpression(TreeExprBuilder::MakeFunction("lower", {s}, arrow::utf8()), arrow::field("lo", arrow::utf8()))};
  CHECK(exprs[0] != nullptr && exprs[1] != nullptr);
  if (host_only) {
    std::printf(failures ? "FAILED\n" : "OK (host-only)\n");
    return failures ? 1 : 0;
  }

  auto pool = arrow::default_memory_pool();
  // h é l l o | ß | dotless i, long s | U+0250 | Kelvin sign | U+10428 | null | ""
  auto batch = arrow::RecordBatch::Make(schema, 8, {Strings({"h\xc3\xa9llo W\xc3\x96RLD", "\xc3\x9f", "\xc4\xb1\xc5\xbf", "\xc9\x90", "\xe2\x84\xaa",
                                                             "\xf0\x90\x90\xa8", nullptr, ""})});
  const std::vector<std::string> up = {"H\xc3\x89LLO W\xc3\x96RLD", "\xe1\xba\x9e", "IS", "\xe2\xb1\xaf", "\xe2\x84\xaa", "\xf0\x90\x90\x80", "", ""};
  const std::vector<std::string> lo = {"h\xc3\xa9llo w\xc3\xb6rld", "\xc3\x9f", "\xc4\xb1\xc5\xbf", "\xc9\x90", "k", "\xf0\x90\x90\xa8", "", ""};
  const std::vector<std::string> ascii_up = {"H\xc3\xa9LLO W\xc3\x96RLD", "\xc3\x9f", "\xc4\xb1\xc5\xbf", "\xc9\x90", "\xe2\x84\xaa", "\xf0\x90\x90\xa8", "", ""};

  setenv("GDV_UTF8_CASE", "1", 1);
  std::shared_ptr<Projector> with_option;
  CHECK_OK(Projector::Make(schema, exprs, &with_option));
  unsetenv("GDV_UTF8_CASE");
  std::shared_ptr<Projector> without;
  CHECK_OK(Projector::Make(schema, exprs, &without));
  CHECK(with_option != without);

  arrow::ArrayVector out, plain;
  CHECK_OK(with_option->Evaluate(*batch, pool, &out));
  CHECK_OK(without->Evaluate(*batch, pool, &plain));
  CHECK(out.size() == 2 && plain.size() == 2);
  if (out.size() == 2 && plain.size() == 2) {
    auto o0 = std::static_pointer_cast<arrow::StringArray>(out[0]), o1 = std::static_pointer_cast<arrow::StringArray>(out[1]);
    auto p0 = std::static_pointer_cast<arrow::StringArray>(plain[0]);
    for (int i = 0; i < 8; i++) {
      const bool null = i == 6;
      CHECK(o0->IsNull(i) == null && o1->IsNull(i) == null && p0->IsNull(i) == null);
      if (null) continue;
      CHECK(o0->GetString(i) == up[i]);
      CHECK(o1->GetString(i) == lo[i]);
      CHECK(p0->GetString(i) == ascii_up[i]);
    }
  }
  // a character cut by the end of the text: an execution error with the option, bytes like any other without it
  auto bad = arrow::RecordBatch::Make(schema, 2, {Strings({"fine", "cut \xe2\x82"})});
  arrow::ArrayVector out2, plain2;
  arrow::Status st = with_option->Evaluate(*bad, pool, &out2);
  CHECK(!st.ok() && st.ToString().find("upper / lower") != std::string::npos);
  CHECK_OK(without->Evaluate(*bad, pool, &plain2));
  std::printf(failures ? "FAILED\n" : "OK\n");
  return failures ? 1 : 0;
}
