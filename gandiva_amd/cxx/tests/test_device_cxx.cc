// Device-resident Arrow batches through the gandiva:: C++ API (gandiva/device_memory.h).
// `--host-only`: what HipDevice / HipMemoryManager promise without an allocation (no GPU needed).
// Without the flag, on the GPU, in this one process: the reference lineage's KATs, host-resident against
// device-resident evaluation of the same trees, slices, caller-allocated outputs, filters and selection vectors of
// every mode, the fused filter-project, the pool's retention, two devices and the restoring of the caller's device.
// Every result is asserted to be !is_cpu() and compared after CopyTo(default_cpu_memory_manager()).
// A Status that should be OK and is not ends the program at once: nothing further is started on the GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

#include "arrow/api.h"
#include "arrow/device.h"
#include "gandiva/device_memory.h"
#include "gandiva/filter.h"
#include "gandiva/filter_project.h"
#include "gandiva/projector.h"
#include "gandiva/sharded.h"
#include "gandiva/tree_expr_builder.h"
#include "gandiva_amd.h"  // gdv_set_virtual_devices / gdv_set_device / gdv_get_device

using namespace gandiva;

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); failures++; } \
  } while (0)
// fatal: after an unexpected error (a HIP error above all) nothing else runs
#define CHECK_OK(expr)                                                     \
  do {                                                                     \
    arrow::Status _s = (expr);                                             \
    if (!_s.ok()) {                                                        \
      std::printf("FATAL %s:%d  %s -> %s\n", __FILE__, __LINE__, #expr, _s.ToString().c_str()); \
      std::fflush(stdout);                                                 \
      std::_Exit(2);                                                       \
    }                                                                      \
  } while (0)
template <typename T>
T Must(arrow::Result<T> r, const char* what, int line) {
  if (!r.ok()) {
    std::printf("FATAL %s:%d  %s -> %s\n", __FILE__, line, what, r.status().ToString().c_str());
    std::fflush(stdout);
    std::_Exit(2);
  }
  return std::move(r).ValueUnsafe();
}
#define MUST(expr) Must((expr), #expr, __LINE__)

template <typename B, typename T>
ArrayPtr MakeArr(const std::vector<T>& v, const std::vector<bool>& valid = {}) {
  B b;
  for (size_t i = 0; i < v.size(); i++) {
    if (!valid.empty() && !valid[i]) (void)b.AppendNull();
    else (void)b.Append(v[i]);
  }
  return b.Finish().ValueOrDie();
}

static const std::shared_ptr<arrow::MemoryManager>& Cpu() {
  static auto mm = arrow::default_cpu_memory_manager();
  return mm;
}
static bool OnDevice(const arrow::ArrayData& d) {
  bool any = false;
  for (auto& b : d.buffers)
    if (b) {
      if (b->is_cpu()) return false;
      any = true;
    }
  return any;
}
static ArrayPtr ToHost(const ArrayPtr& a) { return MUST(a->CopyTo(Cpu())); }

// deterministic inputs
struct Rng {
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
  uint64_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
  int64_t below(int64_t n) { return static_cast<int64_t>(next() % static_cast<uint64_t>(n)); }
  double unit() { return static_cast<double>(next() >> 11) * (1.0 / 9007199254740992.0); }
};
// 10 % nulls, or no validity buffer at all
static std::vector<bool> Validity(int64_t n, bool nulls, Rng& r) {
  std::vector<bool> v;
  if (nulls) for (int64_t i = 0; i < n; i++) v.push_back(r.below(10) != 0);
  return v;
}
static ArrayPtr DropValidity(const ArrayPtr& a) {
  auto d = a->data()->Copy();
  d->buffers[0] = nullptr;
  d->null_count = 0;
  return arrow::MakeArray(d);
}
template <typename B, typename T>
static ArrayPtr Column(const std::vector<T>& v, const std::vector<bool>& valid) {
  auto a = MakeArr<B, T>(v, valid);
  return valid.empty() ? DropValidity(a) : a;
}

static NodePtr Fn(const std::string& name, const NodeVector& args, DataTypePtr t) { return TreeExprBuilder::MakeFunction(name, args, t); }

// ---- the trees of the host-against-device comparison
struct Workload {
  SchemaPtr schema;
  ExpressionVector exprs;
  ConditionPtr cond;
};
static Workload C1() {
  auto fa = arrow::field("a", arrow::int32()), fb = arrow::field("b", arrow::int32()), fc = arrow::field("c", arrow::int32());
  auto a = TreeExprBuilder::MakeField(fa), b = TreeExprBuilder::MakeField(fb), c = TreeExprBuilder::MakeField(fc);
  auto root = Fn("add", {a, Fn("multiply", {b, c}, arrow::int32())}, arrow::int32());
  return {arrow::schema({fa, fb, fc}), {TreeExprBuilder::MakeExpression(root, arrow::field("r", arrow::int32()))}, nullptr};
}
static std::shared_ptr<arrow::RecordBatch> C1Batch(int64_t n, bool nulls) {
  Rng r(11);
  std::vector<ArrayPtr> cols;
  for (int k = 0; k < 3; k++) {
    std::vector<int32_t> v(n);
    for (auto& x : v) x = static_cast<int32_t>(r.below(65536) - 32768);
    cols.push_back(Column<arrow::Int32Builder, int32_t>(v, Validity(n, nulls, r)));
  }
  return arrow::RecordBatch::Make(C1().schema, n, cols);
}
static Workload C2() {
  auto f64 = arrow::float64();
  FieldVector fs;
  NodeVector x;
  for (const char* name : {"a", "b", "c", "d"}) {
    fs.push_back(arrow::field(name, f64));
    x.push_back(TreeExprBuilder::MakeField(fs.back()));
  }
  auto add = [&](NodePtr l, NodePtr r) { return Fn("add", {l, r}, f64); };
  auto sub = [&](NodePtr l, NodePtr r) { return Fn("subtract", {l, r}, f64); };
  auto mul = [&](NodePtr l, NodePtr r) { return Fn("multiply", {l, r}, f64); };
  NodePtr a = x[0], b = x[1], c = x[2], d = x[3];
  NodeVector roots = {add(a, b), sub(a, b), mul(a, b), add(c, d), mul(c, d), mul(add(a, b), c), mul(sub(a, b), d),
                      add(mul(a, b), mul(c, d)), mul(add(a, b), sub(c, d)), mul(mul(mul(a, b), c), d)};
  Workload w{arrow::schema(fs), {}, nullptr};
  for (size_t i = 0; i < roots.size(); i++)
    w.exprs.push_back(TreeExprBuilder::MakeExpression(roots[i], arrow::field("e" + std::to_string(i), f64)));
  return w;
}
static std::shared_ptr<arrow::RecordBatch> C2Batch(int64_t n, bool nulls) {
  Rng r(42);
  std::vector<ArrayPtr> cols;
  for (int k = 0; k < 4; k++) {
    std::vector<double> v(n);
    for (auto& x : v) x = r.unit() * 8.0 - 4.0;
    cols.push_back(Column<arrow::DoubleBuilder, double>(v, Validity(n, nulls, r)));
  }
  return arrow::RecordBatch::Make(C2().schema, n, cols);
}
static Workload C3() {
  auto fa = arrow::field("a", arrow::int64()), fb = arrow::field("b", arrow::int64());
  auto a = TreeExprBuilder::MakeField(fa), b = TreeExprBuilder::MakeField(fb);
  auto gt = Fn("greater_than", {a, TreeExprBuilder::MakeLiteral(int64_t{499})}, arrow::boolean());
  auto lt = Fn("less_than", {b, TreeExprBuilder::MakeLiteral(int64_t{250})}, arrow::boolean());
  Workload w{arrow::schema({fa, fb}), {}, TreeExprBuilder::MakeCondition(TreeExprBuilder::MakeAnd({gt, lt}))};
  w.exprs.push_back(TreeExprBuilder::MakeExpression(Fn("add", {a, b}, arrow::int64()), arrow::field("s", arrow::int64())));
  return w;
}
static std::shared_ptr<arrow::RecordBatch> C3Batch(int64_t n, bool nulls) {
  Rng r(7);
  std::vector<ArrayPtr> cols;
  for (int k = 0; k < 2; k++) {
    std::vector<int64_t> v(n);
    for (auto& x : v) x = r.below(1000);
    cols.push_back(Column<arrow::Int64Builder, int64_t>(v, Validity(n, nulls, r)));
  }
  return arrow::RecordBatch::Make(C3().schema, n, cols);
}
static Workload C5() {
  auto fs = arrow::field("s", arrow::utf8());
  auto s = TreeExprBuilder::MakeField(fs);
  auto like = Fn("like", {s, TreeExprBuilder::MakeStringLiteral("%spark%")}, arrow::boolean());
  auto sub = Fn("substr", {s, TreeExprBuilder::MakeLiteral(int64_t{2}), TreeExprBuilder::MakeLiteral(int64_t{5})}, arrow::utf8());
  auto up = Fn("upper", {s}, arrow::utf8());
  return {arrow::schema({fs}),
          {TreeExprBuilder::MakeExpression(like, arrow::field("is_spark", arrow::boolean())),
           TreeExprBuilder::MakeExpression(sub, arrow::field("sub", arrow::utf8())),
           TreeExprBuilder::MakeExpression(up, arrow::field("up", arrow::utf8()))},
          nullptr};
}
static std::shared_ptr<arrow::RecordBatch> C5Batch(int64_t n, bool nulls) {
  Rng r(21);
  static const char letters[] = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ";
  std::vector<std::string> v(n);
  for (auto& s : v) {
    const int64_t len = 4 + r.below(17);
    for (int64_t i = 0; i < len; i++) s.push_back(letters[r.below(52)]);
    if (len >= 5 && r.below(20) == 0) s.replace(static_cast<size_t>(r.below(len - 4)), 5, "spark");
  }
  return arrow::RecordBatch::Make(C5().schema, n, {Column<arrow::StringBuilder, std::string>(v, Validity(n, nulls, r))});
}
static Workload Divide() {
  auto fa = arrow::field("a", arrow::int32()), fb = arrow::field("b", arrow::int32());
  auto root = Fn("divide", {TreeExprBuilder::MakeField(fa), TreeExprBuilder::MakeField(fb)}, arrow::int32());
  return {arrow::schema({fa, fb}), {TreeExprBuilder::MakeExpression(root, arrow::field("q", arrow::int32()))}, nullptr};
}
// row n / 2 divides by zero, and is valid
static std::shared_ptr<arrow::RecordBatch> DivideBatch(int64_t n, bool nulls) {
  Rng r(5);
  std::vector<int32_t> a(n), b(n);
  for (int64_t i = 0; i < n; i++) { a[i] = static_cast<int32_t>(r.below(100000)); b[i] = static_cast<int32_t>(1 + r.below(9)); }
  b[n / 2] = 0;
  auto va = Validity(n, nulls, r), vb = Validity(n, nulls, r);
  if (nulls) va[n / 2] = vb[n / 2] = true;
  return arrow::RecordBatch::Make(Divide().schema, n, {Column<arrow::Int32Builder, int32_t>(a, va), Column<arrow::Int32Builder, int32_t>(b, vb)});
}

// values and validity through Equals; utf8 / binary also offset for offset and byte for byte
static bool SameArray(const ArrayPtr& host, const ArrayPtr& from_device) {
  if (!host->Equals(from_device)) return false;
  if (host->type_id() != arrow::Type::STRING && host->type_id() != arrow::Type::BINARY) return true;
  auto h = std::static_pointer_cast<arrow::BinaryArray>(host), d = std::static_pointer_cast<arrow::BinaryArray>(from_device);
  const int64_t n = h->length();
  if (h->offset() != 0 || d->offset() != 0) return false;
  if (std::memcmp(h->value_offsets()->data(), d->value_offsets()->data(), static_cast<size_t>(n + 1) * 4) != 0) return false;
  const int64_t total = h->value_offset(n);
  return total == 0 || std::memcmp(h->value_data()->data(), d->value_data()->data(), static_cast<size_t>(total)) == 0;
}

// the device result of a projection, checked to be on the device, copied back
static ArrayVector ProjectOnDevice(const Projector& p, const arrow::RecordBatch& dbatch, const SelectionVector* sel = nullptr) {
  ArrayVector out, host;
  if (sel) CHECK_OK(p.Evaluate(dbatch, sel, nullptr, &out));
  else CHECK_OK(p.Evaluate(dbatch, nullptr, &out));
  for (auto& a : out) {
    CHECK(OnDevice(*a->data()));
    host.push_back(ToHost(a));
  }
  return host;
}
static void SameProjection(const char* what, const Projector& p, const arrow::RecordBatch& host, const arrow::RecordBatch& dbatch) {
  ArrayVector want;
  CHECK_OK(p.Evaluate(host, arrow::default_memory_pool(), &want));
  ArrayVector got = ProjectOnDevice(p, dbatch);
  bool same = got.size() == want.size();
  for (size_t e = 0; same && e < want.size(); e++) same = SameArray(want[e], got[e]);
  if (!same) { std::printf("FAIL %s: %lld rows, device result differs from the host result\n", what, static_cast<long long>(host.num_rows())); failures++; }
}
static ArrayPtr FilterOnDevice(Filter& f, const arrow::RecordBatch& dbatch, SelectionVector::Mode mode,
                               const std::shared_ptr<HipMemoryManager>& mm, std::shared_ptr<SelectionVector>* keep = nullptr) {
  auto sel = MUST(MakeDeviceSelectionVector(mode, dbatch.num_rows(), mm));
  CHECK(!sel->GetBuffer().is_cpu());
  CHECK_OK(f.Evaluate(dbatch, sel));
  if (keep) *keep = sel;
  auto arr = sel->ToArray();
  CHECK(OnDevice(*arr->data()));
  return ToHost(arr);
}
static ArrayPtr FilterOnHost(Filter& f, const arrow::RecordBatch& batch, SelectionVector::Mode mode,
                             std::shared_ptr<SelectionVector>* keep = nullptr) {
  std::shared_ptr<SelectionVector> sel;
  auto pool = arrow::default_memory_pool();
  if (mode == SelectionVector::MODE_UINT16) CHECK_OK(SelectionVector::MakeInt16(batch.num_rows(), pool, &sel));
  else if (mode == SelectionVector::MODE_UINT32) CHECK_OK(SelectionVector::MakeInt32(batch.num_rows(), pool, &sel));
  else CHECK_OK(SelectionVector::MakeInt64(batch.num_rows(), pool, &sel));
  CHECK_OK(f.Evaluate(batch, sel));
  if (keep) *keep = sel;
  return sel->ToArray();
}

static int HostOnly() {
  auto d0 = MUST(HipDevice::Make(0)), again = MUST(HipDevice::Make(0)), d1 = MUST(HipDevice::Make(1));
  CHECK(d0->Equals(*again) && again->Equals(*d0));
  CHECK(!d0->Equals(*d1));
  CHECK(!d0->Equals(*arrow::CPUDevice::Instance()));
  CHECK(d0->device_type() == arrow::DeviceAllocationType::kROCM);
  CHECK(!d0->is_cpu());
  CHECK(d0->device_id() == 0 && d1->device_id() == 1);
  CHECK(d0->ToString().find("0") != std::string::npos && d1->ToString().find("1") != std::string::npos);
  CHECK(d0->ToString() != d1->ToString());
  CHECK(std::string(d0->type_name()) == "gandiva::HipDevice");
  auto mm = d0->default_memory_manager();
  CHECK(mm != nullptr && mm == d0->default_memory_manager() && mm == again->default_memory_manager());
  CHECK(mm->device().get() == d0.get() && mm->device()->Equals(*d0));
  CHECK(!mm->is_cpu());
  CHECK(d0->hip_memory_manager() == mm && d0->hip_memory_manager()->device_id() == 0);
  CHECK(d1->default_memory_manager() != mm);
  CHECK(!HipDevice::Make(-1).ok());
  CHECK(d0->hip_memory_manager()->bytes_allocated() == 0);  // no pool before the first allocation
  CHECK(MakeDeviceSelectionVector(SelectionVector::MODE_UINT16, 65537, d0->hip_memory_manager()).status().IsInvalid());
  std::printf(failures ? "FAILED\n" : "OK (host-only)\n");
  return failures ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "--host-only")) return HostOnly();
  if (gdv_set_virtual_devices(2) != GDV_OK) { std::printf("FATAL gdv_set_virtual_devices\n"); return 2; }
  auto mm = MUST(HipDevice::Make(0))->hip_memory_manager();
  auto pool = arrow::default_memory_pool();

  {  // the manager itself: buffers, copies in both directions
    auto b = MUST(mm->AllocateBuffer(100));
    CHECK(!b->is_cpu() && b->is_mutable() && b->size() == 100 && b->capacity() == 128 && b->address() != 0);
    CHECK(b->device_type() == arrow::DeviceAllocationType::kROCM && b->memory_manager() == mm);
    auto z = MUST(mm->AllocateBuffer(0));
    CHECK(z->size() == 0 && z->capacity() % 64 == 0 && !z->is_cpu());
    CHECK(mm->GetBufferReader(std::shared_ptr<arrow::Buffer>(std::move(z))).status().IsNotImplemented());
    auto batch = C5Batch(1000, true);
    auto there = MUST(CopyBatchTo(*batch, mm));
    CHECK(OnDevice(*there->column_data(0)));
    auto back = MUST(CopyBatchTo(*there, Cpu()));
    CHECK(back->Equals(*batch));
    // device to device: the C ABI has no such copy, Arrow goes through the host
    auto mm1 = MUST(HipDevice::Make(1))->hip_memory_manager();
    auto moved = MUST(CopyBatchTo(*there, mm1));
    CHECK(moved->column_data(0)->buffers[1]->device()->device_id() == 1);
    CHECK(MUST(CopyBatchTo(*moved, Cpu()))->Equals(*batch));
  }

  // ---- the reference lineage's nine data-bearing KATs (pyarrow/tests/test_gandiva.py), literal expected values
  {
    auto i32 = arrow::int32();
    auto fa = arrow::field("a", i32), fb = arrow::field("b", i32), fc = arrow::field("c", i32);
    auto na = TreeExprBuilder::MakeField(fa), nb = TreeExprBuilder::MakeField(fb), nc = TreeExprBuilder::MakeField(fc);
    auto gt = Fn("greater_than", {na, nb}, arrow::boolean());
    {  // test_tree_exp_builder
      auto schema = arrow::schema({fa, fb});
      auto e = TreeExprBuilder::MakeExpression(TreeExprBuilder::MakeIf(gt, na, nb, i32), arrow::field("res", i32));
      std::shared_ptr<Projector> p;
      CHECK_OK(Projector::Make(schema, {e}, &p));
      auto batch = arrow::RecordBatch::Make(schema, 4, {MakeArr<arrow::Int32Builder, int32_t>({10, 12, -20, 5}),
                                                        MakeArr<arrow::Int32Builder, int32_t>({5, 15, 15, 17})});
      auto got = ProjectOnDevice(*p, *MUST(CopyBatchTo(*batch, mm)));
      CHECK(got.size() == 1 && got[0]->Equals(MakeArr<arrow::Int32Builder, int32_t>({10, 15, 15, 17})));
    }
    {  // test_table
      auto f64 = arrow::float64();
      auto xa = arrow::field("a", f64), xb = arrow::field("b", f64);
      auto schema = arrow::schema({xa, xb});
      auto e = TreeExprBuilder::MakeExpression(Fn("add", {TreeExprBuilder::MakeField(xa), TreeExprBuilder::MakeField(xb)}, f64), arrow::field("c", f64));
      std::shared_ptr<Projector> p;
      CHECK_OK(Projector::Make(schema, {e}, &p));
      auto batch = arrow::RecordBatch::Make(schema, 2, {MakeArr<arrow::DoubleBuilder, double>({1.0, 2.0}), MakeArr<arrow::DoubleBuilder, double>({3.0, 4.0})});
      auto got = ProjectOnDevice(*p, *MUST(CopyBatchTo(*batch, mm)));
      CHECK(got.size() == 1 && got[0]->Equals(MakeArr<arrow::DoubleBuilder, double>({4.0, 6.0})));
    }
    {  // test_filter
      auto xa = arrow::field("a", arrow::float64());
      auto schema = arrow::schema({xa});
      std::vector<double> v(10000);
      std::vector<uint32_t> want(1000);
      for (int i = 0; i < 10000; i++) v[i] = 1.0 * i;
      for (int i = 0; i < 1000; i++) want[i] = static_cast<uint32_t>(i);
      auto cond = TreeExprBuilder::MakeCondition(Fn("less_than", {TreeExprBuilder::MakeField(xa), TreeExprBuilder::MakeLiteral(1000.0)}, arrow::boolean()));
      std::shared_ptr<Filter> f;
      CHECK_OK(Filter::Make(schema, cond, &f));
      auto batch = arrow::RecordBatch::Make(schema, 10000, {MakeArr<arrow::DoubleBuilder, double>(v)});
      auto got = FilterOnDevice(*f, *MUST(CopyBatchTo(*batch, mm)), SelectionVector::MODE_UINT32, mm);
      CHECK(got->Equals(MakeArr<arrow::UInt32Builder, uint32_t>(want)));
    }
    {  // test_in_expr: utf8
      auto xa = arrow::field("a", arrow::utf8());
      auto schema = arrow::schema({xa});
      auto cond = TreeExprBuilder::MakeCondition(TreeExprBuilder::MakeInExpressionString(TreeExprBuilder::MakeField(xa), {"an", "nd"}));
      std::shared_ptr<Filter> f;
      CHECK_OK(Filter::Make(schema, cond, &f));
      auto batch = arrow::RecordBatch::Make(schema, 6, {MakeArr<arrow::StringBuilder, std::string>({"ga", "an", "nd", "di", "iv", "va"})});
      auto got = FilterOnDevice(*f, *MUST(CopyBatchTo(*batch, mm)), SelectionVector::MODE_UINT32, mm);
      CHECK(got->Equals(MakeArr<arrow::UInt32Builder, uint32_t>({1, 2})));
    }
    {  // test_in_expr: int32 and int64
      auto x32 = arrow::field("a", i32), x64 = arrow::field("a", arrow::int64());
      std::shared_ptr<Filter> f32, f64;
      CHECK_OK(Filter::Make(arrow::schema({x32}), TreeExprBuilder::MakeCondition(TreeExprBuilder::MakeInExpressionInt32(TreeExprBuilder::MakeField(x32), {1, 5})), &f32));
      CHECK_OK(Filter::Make(arrow::schema({x64}), TreeExprBuilder::MakeCondition(TreeExprBuilder::MakeInExpressionInt64(TreeExprBuilder::MakeField(x64), {1, 5})), &f64));
      auto b32 = arrow::RecordBatch::Make(arrow::schema({x32}), 10, {MakeArr<arrow::Int32Builder, int32_t>({3, 1, 4, 1, 5, 9, 2, 6, 5, 4})});
      auto b64 = arrow::RecordBatch::Make(arrow::schema({x64}), 10, {MakeArr<arrow::Int64Builder, int64_t>({3, 1, 4, 1, 5, 9, 2, 6, 5, 4})});
      auto want = MakeArr<arrow::UInt32Builder, uint32_t>({1, 3, 4, 8});
      CHECK(FilterOnDevice(*f32, *MUST(CopyBatchTo(*b32, mm)), SelectionVector::MODE_UINT32, mm)->Equals(want));
      CHECK(FilterOnDevice(*f64, *MUST(CopyBatchTo(*b64, mm)), SelectionVector::MODE_UINT32, mm)->Equals(want));
    }
    {  // test_boolean
      auto f64 = arrow::float64();
      auto xa = arrow::field("a", f64), xb = arrow::field("b", f64);
      auto schema = arrow::schema({xa, xb});
      auto a = TreeExprBuilder::MakeField(xa), b = TreeExprBuilder::MakeField(xb);
      auto c1 = Fn("less_than", {a, TreeExprBuilder::MakeLiteral(50.0)}, arrow::boolean());
      auto c2 = Fn("greater_than", {a, b}, arrow::boolean());
      auto c3 = Fn("less_than", {b, TreeExprBuilder::MakeLiteral(11.0)}, arrow::boolean());
      auto cond = TreeExprBuilder::MakeCondition(TreeExprBuilder::MakeOr({TreeExprBuilder::MakeAnd({c1, c2}), c3}));
      std::shared_ptr<Filter> f;
      CHECK_OK(Filter::Make(schema, cond, &f));
      auto batch = arrow::RecordBatch::Make(schema, 7, {MakeArr<arrow::DoubleBuilder, double>({1., 31., 46., 3., 57., 44., 22.}),
                                                        MakeArr<arrow::DoubleBuilder, double>({5., 45., 36., 73., 83., 23., 76.})});
      auto got = FilterOnDevice(*f, *MUST(CopyBatchTo(*batch, mm)), SelectionVector::MODE_UINT32, mm);
      CHECK(got->Equals(MakeArr<arrow::UInt32Builder, uint32_t>({0, 2, 5})));
    }
    {  // test_regex
      auto xa = arrow::field("a", arrow::utf8());
      auto schema = arrow::schema({xa});
      auto e = TreeExprBuilder::MakeExpression(Fn("like", {TreeExprBuilder::MakeField(xa), TreeExprBuilder::MakeStringLiteral("%spark%")}, arrow::boolean()),
                                               arrow::field("b", arrow::boolean()));
      std::shared_ptr<Projector> p;
      CHECK_OK(Projector::Make(schema, {e}, &p));
      auto batch = arrow::RecordBatch::Make(schema, 4, {MakeArr<arrow::StringBuilder, std::string>({"park", "sparkle", "bright spark and fire", "spark"})});
      auto got = ProjectOnDevice(*p, *MUST(CopyBatchTo(*batch, mm)));
      CHECK(got.size() == 1 && got[0]->Equals(MakeArr<arrow::BooleanBuilder, bool>({false, true, true, true})));
    }
    {  // test_filter_project: the chain, the fused operator, and the chain behind the fused interface (var-len output)
      auto schema = arrow::schema({fa, fb, fc});
      auto batch = arrow::RecordBatch::Make(
          schema, 6,
          {MakeArr<arrow::Int32Builder, int32_t>({10, 12, -20, 5, 21, 29}), MakeArr<arrow::Int32Builder, int32_t>({5, 15, 15, 17, 12, 3}),
           MakeArr<arrow::Int32Builder, int32_t>({1, 25, 11, 30, -21, 0}, {true, true, true, true, true, false})});
      auto dbatch = MUST(CopyBatchTo(*batch, mm));
      auto fcond = TreeExprBuilder::MakeCondition(gt);
      auto e = TreeExprBuilder::MakeExpression(TreeExprBuilder::MakeIf(Fn("less_than", {nb, nc}, arrow::boolean()), nb, nc, i32), arrow::field("res", i32));
      auto want = MakeArr<arrow::Int32Builder, int32_t>({1, -21, 0}, {true, true, false});
      std::shared_ptr<Filter> f;
      std::shared_ptr<Projector> p;
      CHECK_OK(Filter::Make(schema, fcond, &f));
      CHECK_OK(Projector::Make(schema, {e}, SelectionVector::MODE_UINT32, ConfigurationBuilder::DefaultConfiguration(), &p));
      std::shared_ptr<SelectionVector> sel;
      CHECK(FilterOnDevice(*f, *dbatch, SelectionVector::MODE_UINT32, mm, &sel)->Equals(MakeArr<arrow::UInt32Builder, uint32_t>({0, 4, 5})));
      auto got = ProjectOnDevice(*p, *dbatch, sel.get());
      CHECK(got.size() == 1 && got[0]->Equals(want));
      std::shared_ptr<FilterProject> fp;
      CHECK_OK(FilterProject::Make(schema, fcond, {e}, SelectionVector::MODE_UINT32, ConfigurationBuilder::DefaultConfiguration(), &fp));
      CHECK(fp->fused());
      auto fsel = MUST(MakeDeviceSelectionVector(SelectionVector::MODE_UINT32, 6, mm));
      ArrayVector out;
      CHECK_OK(fp->Evaluate(*dbatch, nullptr, &out, fsel));
      CHECK(fsel->GetNumSlots() == 3 && ToHost(fsel->ToArray())->Equals(MakeArr<arrow::UInt32Builder, uint32_t>({0, 4, 5})));
      CHECK(out.size() == 1 && OnDevice(*out[0]->data()) && ToHost(out[0])->Equals(want));
      std::shared_ptr<FilterProject> fp0;  // MODE_NONE: the temporary vector of the chain lives where the batch does
      auto cs = TreeExprBuilder::MakeExpression(Fn("castVARCHAR", {na, TreeExprBuilder::MakeLiteral(int64_t{10})}, arrow::utf8()), arrow::field("t", arrow::utf8()));
      CHECK_OK(FilterProject::Make(schema, fcond, {cs}, SelectionVector::MODE_NONE, ConfigurationBuilder::DefaultConfiguration(), &fp0));
      CHECK(!fp0->fused());
      ArrayVector outc;
      CHECK_OK(fp0->Evaluate(*dbatch, nullptr, &outc));
      CHECK(outc.size() == 1 && OnDevice(*outc[0]->data()) && ToHost(outc[0])->Equals(MakeArr<arrow::StringBuilder, std::string>({"10", "21", "29"})));
      // a CPU selection vector with a device-resident batch (what pyarrow's Filter.evaluate allocates): staged by the shim
      std::shared_ptr<SelectionVector> hsel;
      CHECK_OK(SelectionVector::MakeInt32(6, pool, &hsel));
      CHECK_OK(f->Evaluate(*dbatch, hsel));
      CHECK(hsel->ToArray()->Equals(MakeArr<arrow::UInt32Builder, uint32_t>({0, 4, 5})));
      auto goth = ProjectOnDevice(*p, *dbatch, hsel.get());
      CHECK(goth.size() == 1 && goth[0]->Equals(want));
      // the other way round is refused
      ArrayVector refused;
      CHECK(p->Evaluate(*batch, sel.get(), pool, &refused).IsInvalid());
      CHECK(f->Evaluate(*batch, sel).IsInvalid());
    }
  }

  // ---- the same tree, host-resident against device-resident
  const int64_t row_counts[] = {1, 64, 65, 1023, 1025, 4097, 70001};
  {
    Workload c1 = C1(), c2 = C2(), c3 = C3(), c5 = C5(), dv = Divide();
    std::shared_ptr<Projector> p1, p2, p5, pd;
    std::shared_ptr<Filter> f3;
    CHECK_OK(Projector::Make(c1.schema, c1.exprs, &p1));
    CHECK_OK(Projector::Make(c2.schema, c2.exprs, &p2));
    CHECK_OK(Projector::Make(c5.schema, c5.exprs, &p5));
    CHECK_OK(Projector::Make(dv.schema, dv.exprs, &pd));
    CHECK_OK(Filter::Make(c3.schema, c3.cond, &f3));
    for (int64_t n : row_counts) {
      for (bool nulls : {true, false}) {
        auto b1 = C1Batch(n, nulls), b2 = C2Batch(n, nulls), b3 = C3Batch(n, nulls), b5 = C5Batch(n, nulls), bd = DivideBatch(n, nulls);
        if (!nulls) CHECK(b2->column_data(0)->buffers[0] == nullptr && b5->column_data(0)->buffers[0] == nullptr);
        else if (n >= 1023) CHECK(b2->column_data(0)->buffers[0] != nullptr && b2->column(0)->null_count() > 0);
        SameProjection("C1", *p1, *b1, *MUST(CopyBatchTo(*b1, mm)));
        SameProjection("C2", *p2, *b2, *MUST(CopyBatchTo(*b2, mm)));
        SameProjection("C5", *p5, *b5, *MUST(CopyBatchTo(*b5, mm)));
        auto want3 = FilterOnHost(*f3, *b3, SelectionVector::MODE_UINT32);
        auto got3 = FilterOnDevice(*f3, *MUST(CopyBatchTo(*b3, mm)), SelectionVector::MODE_UINT32, mm);
        if (!want3->Equals(got3)) { std::printf("FAIL C3: %lld rows, device indices differ\n", static_cast<long long>(n)); failures++; }
        // a raising function: the same error Status from both paths, no result
        ArrayVector oh, od;
        arrow::Status sh = pd->Evaluate(*bd, pool, &oh), sd = pd->Evaluate(*MUST(CopyBatchTo(*bd, mm)), nullptr, &od);
        CHECK(!sh.ok() && !sd.ok() && sh.code() == sd.code() && sh.message() == sd.message());
        CHECK(sd.message().find("divide by zero") != std::string::npos);
      }
    }

    // ---- slices of a device-resident batch: array offset != 0, bitmaps start inside a byte
    auto s2 = C2Batch(5000, true), s5 = C5Batch(5000, true), s3 = C3Batch(5000, true);
    auto d2 = MUST(CopyBatchTo(*s2, mm)), d5 = MUST(CopyBatchTo(*s5, mm)), d3 = MUST(CopyBatchTo(*s3, mm));
    const std::vector<std::pair<int64_t, int64_t>> slices = {{3, 4000}, {67, 1000}};
    for (auto [lo, len] : slices) {
      CHECK(d2->Slice(lo, len)->column_data(0)->offset == lo);
      SameProjection("C2 slice", *p2, *s2->Slice(lo, len), *d2->Slice(lo, len));
      SameProjection("C5 slice", *p5, *s5->Slice(lo, len), *d5->Slice(lo, len));
      CHECK(FilterOnHost(*f3, *s3->Slice(lo, len), SelectionVector::MODE_UINT32)->Equals(
          FilterOnDevice(*f3, *d3->Slice(lo, len), SelectionVector::MODE_UINT32, mm)));
    }

    // ---- caller-allocated outputs from ReserveSet: ten float64 columns, then a utf8 one
    {
      const int64_t n = 4097;
      auto b2 = C2Batch(n, true);
      auto dbatch = MUST(CopyBatchTo(*b2, mm));
      auto set = MUST(mm->ReserveSet(20, n * 8));
      CHECK(set.size() == 20 && !set[0]->is_cpu() && set[0]->is_mutable() && set[0]->size() == n * 8 && set[0]->capacity() % 64 == 0);
      ArrayDataVector outs;
      for (int e = 0; e < 10; e++) outs.push_back(arrow::ArrayData::Make(arrow::float64(), n, {set[e], set[10 + e]}));
      CHECK_OK(p2->Evaluate(*dbatch, outs));
      ArrayVector want;
      CHECK_OK(p2->Evaluate(*b2, pool, &want));
      for (int e = 0; e < 10; e++) {
        CHECK(outs[e]->null_count == arrow::kUnknownNullCount);
        CHECK(SameArray(want[e], ToHost(arrow::MakeArray(outs[e]))));
      }
      // a CPU output under a device batch is refused before anything is launched
      auto hv = std::shared_ptr<arrow::Buffer>(MUST(arrow::AllocateBuffer(n * 8)));
      ArrayDataVector mixed = outs;
      mixed[0] = arrow::ArrayData::Make(arrow::float64(), n, {hv, hv});
      CHECK(p2->Evaluate(*dbatch, mixed).IsInvalid());

      auto fs = arrow::field("s", arrow::utf8());
      auto up = TreeExprBuilder::MakeExpression(Fn("upper", {TreeExprBuilder::MakeField(fs)}, arrow::utf8()), arrow::field("u", arrow::utf8()));
      std::shared_ptr<Projector> pu;
      CHECK_OK(Projector::Make(arrow::schema({fs}), {up}, &pu));
      auto b5 = C5Batch(n, true);
      auto d5s = MUST(CopyBatchTo(*b5, mm));
      auto sset = MUST(mm->ReserveSet(3, 32 * n));  // >= (n + 1) * 4 offsets and >= 20 bytes per row
      auto sdata = arrow::ArrayData::Make(arrow::utf8(), n, {sset[0], sset[1], sset[2]});
      CHECK_OK(pu->Evaluate(*d5s, ArrayDataVector{sdata}));
      ArrayVector wantu;
      CHECK_OK(pu->Evaluate(*b5, pool, &wantu));
      CHECK(SameArray(wantu[0], ToHost(arrow::MakeArray(sdata))));
      auto tiny = MUST(mm->ReserveSet(1, 64));
      arrow::Status small = pu->Evaluate(*d5s, ArrayDataVector{arrow::ArrayData::Make(arrow::utf8(), n, {sset[0], sset[1], tiny[0]})});
      CHECK(small.IsInvalid() && small.ToString().find("needed") != std::string::npos);
    }

    // ---- selection vectors of every mode; uint16 ends at 65536 rows
    {
      auto b16 = C3Batch(65536, true);
      auto d16 = MUST(CopyBatchTo(*b16, mm));
      CHECK(FilterOnHost(*f3, *b16, SelectionVector::MODE_UINT16)->Equals(FilterOnDevice(*f3, *d16, SelectionVector::MODE_UINT16, mm)));
      auto too_many = MakeDeviceSelectionVector(SelectionVector::MODE_UINT16, 65537, mm);
      CHECK(too_many.status().IsInvalid() && too_many.status().message().find("65536") != std::string::npos);
      {  // and a 65537-row batch into a 65536-slot vector is the filter's own bounds error
        auto b17 = C3Batch(65537, false);
        auto s16 = MUST(MakeDeviceSelectionVector(SelectionVector::MODE_UINT16, 65536, mm));
        CHECK(f3->Evaluate(*MUST(CopyBatchTo(*b17, mm)), s16).IsInvalid());
      }
      auto big = C3Batch(70001, true);
      auto dbig = MUST(CopyBatchTo(*big, mm));
      std::shared_ptr<SelectionVector> hsel, dsel;
      CHECK(FilterOnHost(*f3, *big, SelectionVector::MODE_UINT64)->Equals(FilterOnDevice(*f3, *dbig, SelectionVector::MODE_UINT64, mm)));
      CHECK(FilterOnHost(*f3, *big, SelectionVector::MODE_UINT32, &hsel)->Equals(FilterOnDevice(*f3, *dbig, SelectionVector::MODE_UINT32, mm, &dsel)));
      CHECK(hsel->GetNumSlots() > 1000 && hsel->GetNumSlots() == dsel->GetNumSlots());
      // selection-mode projector and the fused filter-project over the device batch and the device vector
      std::shared_ptr<Projector> ps;
      CHECK_OK(Projector::Make(c3.schema, c3.exprs, SelectionVector::MODE_UINT32, ConfigurationBuilder::DefaultConfiguration(), &ps));
      ArrayVector want;
      CHECK_OK(ps->Evaluate(*big, hsel.get(), pool, &want));
      auto got = ProjectOnDevice(*ps, *dbig, dsel.get());
      CHECK(got.size() == 1 && got[0]->length() == hsel->GetNumSlots() && SameArray(want[0], got[0]));
      std::shared_ptr<FilterProject> fp;
      CHECK_OK(FilterProject::Make(c3.schema, c3.cond, c3.exprs, SelectionVector::MODE_UINT32, ConfigurationBuilder::DefaultConfiguration(), &fp));
      CHECK(fp->fused());
      auto fsel = MUST(MakeDeviceSelectionVector(SelectionVector::MODE_UINT32, 70001, mm));
      ArrayVector fout;
      CHECK_OK(fp->Evaluate(*dbig, nullptr, &fout, fsel));
      CHECK(fsel->GetNumSlots() == hsel->GetNumSlots() && ToHost(fsel->ToArray())->Equals(hsel->ToArray()));
      CHECK(fout.size() == 1 && OnDevice(*fout[0]->data()) && SameArray(want[0], ToHost(fout[0])));
    }

    // ---- two devices (two contexts on the one GPU of a test box): one shard per device, each copied with its manager
    {
      auto mm1 = MUST(HipDevice::Make(1))->hip_memory_manager();
      std::shared_ptr<HipMemoryManager> mms[2] = {mm, mm1};
      const int64_t n = 10000;
      auto big = C1Batch(n, true);
      auto big3 = C3Batch(n, true);
      std::vector<std::shared_ptr<arrow::RecordBatch>> shards, shards3;
      std::vector<std::shared_ptr<SelectionVector>> sels;
      for (int s = 0; s < 2; s++) {
        int64_t lo = 0, hi = 0;
        ShardBounds(n, 2, s, &lo, &hi);
        shards.push_back(MUST(CopyBatchTo(*big->Slice(lo, hi - lo), mms[s])));
        shards3.push_back(MUST(CopyBatchTo(*big3->Slice(lo, hi - lo), mms[s])));
        sels.push_back(MUST(MakeDeviceSelectionVector(SelectionVector::MODE_UINT32, hi - lo, mms[s])));
      }
      std::shared_ptr<ShardedProjector> sp;
      CHECK_OK(ShardedProjector::Make(c1.schema, c1.exprs, {0, 1}, ConfigurationBuilder::DefaultConfiguration(), &sp));
      std::vector<ArrayVector> outs;
      CHECK_OK(sp->Evaluate(shards, &outs));
      ArrayVector want, parts;
      CHECK_OK(p1->Evaluate(*big, pool, &want));
      CHECK(outs.size() == 2);
      for (int s = 0; s < 2; s++) {
        CHECK(outs[s].size() == 1 && OnDevice(*outs[s][0]->data()));
        CHECK(outs[s][0]->data()->buffers[1]->device()->device_id() == s);
        parts.push_back(ToHost(outs[s][0]));
      }
      CHECK(MUST(arrow::Concatenate(parts))->Equals(want[0]));
      // shards handed over in the wrong order are refused, not evaluated on the wrong device
      std::vector<ArrayVector> wrong;
      CHECK(sp->Evaluate({shards[1], shards[0]}, &wrong).IsInvalid());

      std::shared_ptr<ShardedFilter> sf;
      CHECK_OK(ShardedFilter::Make(c3.schema, c3.cond, {0, 1}, ConfigurationBuilder::DefaultConfiguration(), &sf));
      int64_t total = -1;
      CHECK_OK(sf->Evaluate(shards3, sels, &total));
      ArrayVector iparts;
      for (int s = 0; s < 2; s++) {
        CHECK(sels[s]->GetBuffer().device()->device_id() == s);
        iparts.push_back(ToHost(sels[s]->ToArray()));
      }
      auto want3 = FilterOnHost(*f3, *big3, SelectionVector::MODE_UINT32);
      CHECK(total == want3->length() && MUST(arrow::Concatenate(iparts))->Equals(want3));
      CHECK(sf->Evaluate(shards3, {sels[1], sels[0]}, &total).IsInvalid());  // a vector on the other device than its shard

      // ---- the caller's device is the caller's: unchanged after an Evaluate on the other one
      CHECK(gdv_set_device(0) == GDV_OK);
      auto on1 = MUST(CopyBatchTo(*big, mm1));
      CHECK(gdv_get_device() == 0);
      auto got1 = ProjectOnDevice(*p1, *on1);
      CHECK(gdv_get_device() == 0);
      CHECK(got1[0]->Equals(want[0]));
      CHECK(FilterOnDevice(*f3, *MUST(CopyBatchTo(*big3, mm1)), SelectionVector::MODE_UINT32, mm1)->Equals(want3));
      CHECK(gdv_get_device() == 0);
      CHECK(gdv_set_device(1) == GDV_OK);
      auto got0 = ProjectOnDevice(*p1, *MUST(CopyBatchTo(*big, mm)));
      CHECK(gdv_get_device() == 1);
      CHECK(got0[0]->Equals(want[0]));
      CHECK(gdv_set_device(0) == GDV_OK);
    }
  }

  // ---- the pool: a dropped buffer is handed out again, nothing grows, Trim gives the retained bytes back
  {
    int64_t in_use = -1;
    auto first = MUST(mm->AllocateBuffer(123456));
    const uintptr_t at = first->address();
    const int64_t held = mm->bytes_allocated(&in_use);
    CHECK(held >= 123456 && in_use >= 123456);
    first.reset();
    CHECK(mm->bytes_allocated(&in_use) == held);  // retained
    auto second = MUST(mm->AllocateBuffer(123456));
    CHECK(second->address() == at);
    CHECK(mm->bytes_allocated() == held);
    second.reset();
    CHECK_OK(mm->Trim());
    const int64_t after = mm->bytes_allocated(&in_use);
    CHECK(after - in_use == 0);  // nothing retained
    CHECK(after == 0);           // and every buffer of this program has been dropped by now
  }
  std::printf(failures ? "FAILED\n" : "OK\n");
  return failures ? 1 : 0;
}
