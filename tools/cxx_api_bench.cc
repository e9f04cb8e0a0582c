// What the gandiva:: C++ API costs over the C ABI on device-resident batches (no Python in the loop).
// C2's ten float64 expressions over four HBM-resident columns with 10 % nulls, made by gandiva::HipMemoryManager
// (gandiva/device_memory.h), at 2^28 rows (the headline shape) and at 16 384 rows (what a query engine feeds):
//   c_abi     gdv_projector_evaluate on the raw addresses of those buffers                         — the yardstick
//   cxx_set   Projector::Evaluate(batch, ArrayDataVector), outputs from ReserveSet, reused across steps
//   cxx_pool  Projector::Evaluate(batch, pool, &out): twenty output buffers allocated and dropped per call
// Every call waits for its kernel, so a step is timed with the host clock around the call.  The three variants run
// in turn, `--rounds` times; each line is one round of one variant: the median, the fastest and the slowest of its
// `steps` timed calls (after `warmup` untimed ones).  The closing lines give, per size, the median over the rounds,
// the spread of c_abi's round medians, and the two differences cxx_set - c_abi and cxx_pool - cxx_set.
// Built by gandiva_amd/cxx/Makefile (target `tools`).
//   cxx_api_bench [--rows N]... [--steps K] [--warmup W] [--rounds R]      (K, W: for every size; default by size)
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "arrow/api.h"
#include "gandiva/device_memory.h"
#include "gandiva/projector.h"
#include "gandiva/tree_expr_builder.h"
#include "gandiva_amd.h"

using namespace gandiva;

#define OK(expr)                                                                                            \
  do {                                                                                                      \
    arrow::Status _s = (expr);                                                                              \
    if (!_s.ok()) { std::fprintf(stderr, "FAILED %s:%d %s -> %s\n", __FILE__, __LINE__, #expr, _s.ToString().c_str()); std::_Exit(1); } \
  } while (0)
#define C_OK(expr)                                                                                          \
  do {                                                                                                      \
    if ((expr) != GDV_OK) { std::fprintf(stderr, "FAILED %s:%d %s [%s]\n", __FILE__, __LINE__, #expr, gdv_last_error()); std::_Exit(1); } \
  } while (0)
template <typename T>
static T Get(arrow::Result<T> r, const char* what) {
  if (!r.ok()) { std::fprintf(stderr, "FAILED %s -> %s\n", what, r.status().ToString().c_str()); std::_Exit(1); }
  return std::move(r).ValueUnsafe();
}
#define GET(expr) Get((expr), #expr)

static double NowMs() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static double Median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v.empty() ? 0 : (v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]));
}

// one float64 column with 10 % nulls, generated on the host and copied into `mm`'s memory
static std::shared_ptr<arrow::Array> DeviceColumn(int64_t n, uint64_t seed, const std::shared_ptr<arrow::MemoryManager>& mm,
                                                  std::vector<double>* head, std::vector<bool>* head_valid) {
  auto data = GET(arrow::AllocateBuffer(n * 8));
  auto valid = GET(arrow::AllocateBuffer((n + 7) / 8));
  std::memset(valid->mutable_data(), 0, static_cast<size_t>(valid->size()));
  double* v = reinterpret_cast<double*>(data->mutable_data());
  uint8_t* bits = valid->mutable_data();
  uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
  for (int64_t i = 0; i < n; i++) {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    v[i] = static_cast<double>(s >> 11) * (8.0 / 9007199254740992.0) - 4.0;
    if ((s & 0xff) >= 26) bits[i >> 3] |= static_cast<uint8_t>(1u << (i & 7));  // ~10 % nulls
  }
  for (int64_t i = 0; i < std::min<int64_t>(n, 4096); i++) {
    head->push_back(v[i]);
    head_valid->push_back((bits[i >> 3] >> (i & 7)) & 1);
  }
  auto dd = GET(arrow::MemoryManager::CopyBuffer(std::shared_ptr<arrow::Buffer>(std::move(data)), mm));
  auto dv = GET(arrow::MemoryManager::CopyBuffer(std::shared_ptr<arrow::Buffer>(std::move(valid)), mm));
  return arrow::MakeArray(arrow::ArrayData::Make(arrow::float64(), n, {dv, dd}));
}

// e0 = a + b over the first rows, against the host's own sum
static void CheckHead(const char* what, const std::shared_ptr<arrow::ArrayData>& e0, const std::vector<double>& a, const std::vector<bool>& va,
                      const std::vector<double>& b, const std::vector<bool>& vb) {
  const int64_t m = static_cast<int64_t>(a.size());
  auto cpu = arrow::default_cpu_memory_manager();
  auto hv = GET(arrow::MemoryManager::CopyBuffer(arrow::SliceBuffer(e0->buffers[0], 0, (m + 7) / 8), cpu));
  auto hd = GET(arrow::MemoryManager::CopyBuffer(arrow::SliceBuffer(e0->buffers[1], 0, m * 8), cpu));
  auto host = std::static_pointer_cast<arrow::DoubleArray>(arrow::MakeArray(arrow::ArrayData::Make(arrow::float64(), m, {hv, hd})));
  for (int64_t i = 0; i < m; i++) {
    const bool valid = va[i] && vb[i];
    if (host->IsValid(i) != valid || (valid && host->Value(i) != a[i] + b[i])) {
      std::fprintf(stderr, "FAILED %s: row %lld of e0 is wrong\n", what, static_cast<long long>(i));
      std::_Exit(1);
    }
  }
}

int main(int argc, char** argv) {
  std::vector<int64_t> sizes;
  int steps_arg = 0, warmup_arg = 0, rounds = 5;
  for (int i = 1; i + 1 < argc; i += 2) {
    if (!std::strcmp(argv[i], "--rows")) sizes.push_back(std::atoll(argv[i + 1]));
    else if (!std::strcmp(argv[i], "--steps")) steps_arg = std::atoi(argv[i + 1]);
    else if (!std::strcmp(argv[i], "--warmup")) warmup_arg = std::atoi(argv[i + 1]);
    else if (!std::strcmp(argv[i], "--rounds")) rounds = std::max(1, std::atoi(argv[i + 1]));
    else { std::fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
  }
  if (sizes.empty()) sizes = {int64_t{1} << 28, 16384};

  // the same ten trees twice: through gandiva::TreeExprBuilder and through the C ABI
  auto f64 = arrow::float64();
  const char* names[4] = {"a", "b", "c", "d"};
  FieldVector fields;
  NodeVector x;
  const gdv_type_t g64 = {GDV_TYPE_DOUBLE, 0, 0};
  gdv_schema_t* cschema = gdv_schema_new();
  gdv_node_t* cx[4];
  for (int k = 0; k < 4; k++) {
    fields.push_back(arrow::field(names[k], f64));
    x.push_back(TreeExprBuilder::MakeField(fields.back()));
    C_OK(gdv_schema_add_field(cschema, names[k], g64, 1));
    cx[k] = gdv_node_field(names[k], g64);
  }
  auto fn = [&](const char* name, NodePtr l, NodePtr r) { return TreeExprBuilder::MakeFunction(name, {l, r}, f64); };
  auto cfn = [&](const char* name, gdv_node_t* l, gdv_node_t* r) {
    gdv_node_t* args[2] = {l, r};
    return gdv_node_function(name, args, 2, g64);
  };
  NodePtr a = x[0], b = x[1], c = x[2], d = x[3];
  NodeVector roots = {fn("add", a, b), fn("subtract", a, b), fn("multiply", a, b), fn("add", c, d), fn("multiply", c, d),
                      fn("multiply", fn("add", a, b), c), fn("multiply", fn("subtract", a, b), d),
                      fn("add", fn("multiply", a, b), fn("multiply", c, d)), fn("multiply", fn("add", a, b), fn("subtract", c, d)),
                      fn("multiply", fn("multiply", fn("multiply", a, b), c), d)};
  gdv_node_t *ca = cx[0], *cb = cx[1], *cc = cx[2], *cd = cx[3];
  gdv_node_t* croots[10] = {cfn("add", ca, cb), cfn("subtract", ca, cb), cfn("multiply", ca, cb), cfn("add", cc, cd), cfn("multiply", cc, cd),
                            cfn("multiply", cfn("add", ca, cb), cc), cfn("multiply", cfn("subtract", ca, cb), cd),
                            cfn("add", cfn("multiply", ca, cb), cfn("multiply", cc, cd)),
                            cfn("multiply", cfn("add", ca, cb), cfn("subtract", cc, cd)),
                            cfn("multiply", cfn("multiply", cfn("multiply", ca, cb), cc), cd)};
  ExpressionVector exprs;
  gdv_expression_t* cexprs[10];
  for (int e = 0; e < 10; e++) {
    const std::string name = "e" + std::to_string(e);
    exprs.push_back(TreeExprBuilder::MakeExpression(roots[e], arrow::field(name, f64)));
    cexprs[e] = gdv_expression_new(croots[e], name.c_str(), g64);
  }
  auto schema = arrow::schema(fields);
  std::shared_ptr<Projector> proj;
  OK(Projector::Make(schema, exprs, &proj));
  gdv_projector_t* cproj = nullptr;
  C_OK(gdv_projector_make(cschema, cexprs, 10, GDV_SEL_NONE, nullptr, &cproj));

  auto mm = GET(HipDevice::Make(0))->hip_memory_manager();
  for (int64_t n : sizes) {
    const int steps = steps_arg > 0 ? steps_arg : (n >= (1 << 24) ? 40 : 2000);
    const int warmup = warmup_arg > 0 ? warmup_arg : (n >= (1 << 24) ? 5 : 200);
    std::vector<std::vector<double>> head(4);
    std::vector<std::vector<bool>> head_valid(4);
    std::vector<std::shared_ptr<arrow::Array>> cols;
    for (int k = 0; k < 4; k++) cols.push_back(DeviceColumn(n, 42 + k, mm, &head[k], &head_valid[k]));
    auto batch = arrow::RecordBatch::Make(schema, n, cols);

    // the reused outputs: ten value columns placed together by ReserveSet, ten bitmaps
    const int64_t vbytes = (n + 63) / 64 * 8;
    auto dset = GET(mm->ReserveSet(10, n * 8));
    auto vset = GET(mm->ReserveSet(10, vbytes));
    ArrayDataVector outs;
    std::vector<gdv_column_t> ccols(4);
    std::vector<gdv_out_column_t> couts(10);
    for (int e = 0; e < 10; e++) {
      outs.push_back(arrow::ArrayData::Make(f64, n, {vset[e], dset[e]}));
      std::memset(&couts[e], 0, sizeof(couts[e]));
      couts[e].validity = reinterpret_cast<void*>(vset[e]->address());
      couts[e].validity_size = vset[e]->capacity();
      couts[e].data = reinterpret_cast<void*>(dset[e]->address());
      couts[e].data_size = dset[e]->capacity();
    }
    for (int k = 0; k < 4; k++) {
      std::memset(&ccols[k], 0, sizeof(ccols[k]));
      ccols[k].validity = reinterpret_cast<const void*>(cols[k]->data()->buffers[0]->address());
      ccols[k].validity_size = cols[k]->data()->buffers[0]->size();
      ccols[k].data = reinterpret_cast<const void*>(cols[k]->data()->buffers[1]->address());
      ccols[k].data_size = cols[k]->data()->buffers[1]->size();
    }
    auto c_abi = [&] { C_OK(gdv_projector_evaluate(cproj, n, ccols.data(), 4, nullptr, couts.data(), 10, GDV_MEM_DEVICE, nullptr, 0)); };
    auto cxx_set = [&] { OK(proj->Evaluate(*batch, outs)); };
    ArrayVector pooled;
    auto cxx_pool = [&] {
      pooled.clear();  // (the previous call's buffers go back to the pool first, as a caller that consumed them would do)
      OK(proj->Evaluate(*batch, nullptr, &pooled));
    };
    struct Variant { const char* name; std::function<void()> run; std::vector<double> medians; };
    std::vector<Variant> variants = {{"c_abi", c_abi, {}}, {"cxx_set", cxx_set, {}}, {"cxx_pool", cxx_pool, {}}};

    c_abi();
    CheckHead("c_abi", outs[0], head[0], head_valid[0], head[1], head_valid[1]);
    cxx_set();
    CheckHead("cxx_set", outs[0], head[0], head_valid[0], head[1], head_valid[1]);
    cxx_pool();
    CheckHead("cxx_pool", pooled[0]->data(), head[0], head_valid[0], head[1], head_valid[1]);

    for (int r = 0; r < rounds; r++) {
      for (auto& v : variants) {
        for (int i = 0; i < warmup; i++) v.run();
        std::vector<double> t(steps);
        for (int i = 0; i < steps; i++) {
          const double t0 = NowMs();
          v.run();
          t[i] = NowMs() - t0;
        }
        const double med = Median(t);
        v.medians.push_back(med);
        std::printf("rows=%lld variant=%-8s round=%d steps=%d warmup=%d ms_per_step=%.5f min=%.5f max=%.5f\n", static_cast<long long>(n),
                    v.name, r, steps, warmup, med, *std::min_element(t.begin(), t.end()), *std::max_element(t.begin(), t.end()));
        std::fflush(stdout);
      }
    }
    const double ma = Median(variants[0].medians), mb = Median(variants[1].medians), mc = Median(variants[2].medians);
    const double spread = *std::max_element(variants[0].medians.begin(), variants[0].medians.end()) -
                          *std::min_element(variants[0].medians.begin(), variants[0].medians.end());
    std::printf("rows=%lld summary steps=%d rounds=%d c_abi_ms=%.5f cxx_set_ms=%.5f cxx_pool_ms=%.5f c_abi_round_spread_ms=%.5f "
                "cxx_set_minus_c_abi_us=%.2f cxx_pool_minus_cxx_set_us=%.2f\n",
                static_cast<long long>(n), steps, rounds, ma, mb, mc, spread, (mb - ma) * 1e3, (mc - mb) * 1e3);
    std::fflush(stdout);
    pooled.clear();
    outs.clear();
    dset.clear();
    vset.clear();
    cols.clear();
    batch.reset();
    OK(mm->Trim());  // the next size starts from an empty pool
  }
  gdv_projector_free(cproj);
  return 0;
}
