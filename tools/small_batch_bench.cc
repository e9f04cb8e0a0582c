// Small-batch latency of the C ABI itself (no Python in the loop): the reference is fed 4K-64K-row
// batches by its query engine, where per-call overhead, not HBM, sets the rate.
// HBM-resident C2-shaped batches (4 float64 columns with validity, 10 expressions):
//   sync      gdv_projector_evaluate, one batch per call, the call waits
//   async     gdv_projector_evaluate + GDV_EVAL_ASYNC on one stream, one wait per 64 batches
//   many      gdv_projector_evaluate_many, 64 batches per call (ONE launch), the call waits
// and the filter (a > k1 AND b < k2 over int64): sync vs gdv_filter_evaluate_async.
// Prints microseconds per batch.   g++ -O2 -std=c++17 tools/small_batch_bench.cc -Iinclude
//   -Lgandiva_amd -lgandiva_amd -Wl,-rpath,$PWD/gandiva_amd -o tools/small_batch_bench
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gandiva_amd.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d %s [%s]\n", __FILE__, __LINE__, #c, gdv_last_error()); exit(1); } } while (0)

static double Now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static void FilterProjectSection();

int main(int argc, char** argv) {
  if (argc > 1 && strcmp(argv[1], "fp") == 0) {  // the fused filter-project section alone
    FilterProjectSection();
    return 0;
  }
  const gdv_type_t f64 = {GDV_TYPE_DOUBLE, 0, 0}, i64 = {GDV_TYPE_INT64, 0, 0}, boolean = {GDV_TYPE_BOOL, 0, 0};
  gdv_schema_t* schema = gdv_schema_new();
  const char* names[4] = {"a", "b", "c", "d"};
  gdv_node_t* f[4];
  for (int k = 0; k < 4; k++) {
    CHECK(gdv_schema_add_field(schema, names[k], f64, 1) == GDV_OK);
    f[k] = gdv_node_field(names[k], f64);
  }
  auto fn = [&](const char* name, gdv_node_t* x, gdv_node_t* y) {
    gdv_node_t* args[2] = {x, y};
    return gdv_node_function(name, args, 2, f64);
  };
  gdv_node_t *a = f[0], *b = f[1], *c = f[2], *d = f[3];
  gdv_node_t* roots[10] = {fn("add", a, b), fn("subtract", a, b), fn("multiply", a, b), fn("add", c, d), fn("multiply", c, d),
                           fn("multiply", fn("add", a, b), c), fn("multiply", fn("subtract", a, b), d),
                           fn("add", fn("multiply", a, b), fn("multiply", c, d)),
                           fn("multiply", fn("add", a, b), fn("subtract", c, d)),
                           fn("multiply", fn("multiply", fn("multiply", a, b), c), d)};
  gdv_expression_t* exprs[10];
  for (int e = 0; e < 10; e++) {
    char nm[8];
    snprintf(nm, sizeof(nm), "e%d", e);
    exprs[e] = gdv_expression_new(roots[e], nm, f64);
  }
  gdv_projector_t* proj = nullptr;
  CHECK(gdv_projector_make(schema, exprs, 10, GDV_SEL_NONE, nullptr, &proj) == GDV_OK);

  gdv_schema_t* fschema = gdv_schema_new();
  CHECK(gdv_schema_add_field(fschema, "a", i64, 1) == GDV_OK);
  CHECK(gdv_schema_add_field(fschema, "b", i64, 1) == GDV_OK);
  const int64_t k1 = 499, k2 = 250;
  gdv_node_t* ga[2] = {gdv_node_field("a", i64), gdv_node_literal(i64, &k1, 0)};
  gdv_node_t* gb[2] = {gdv_node_field("b", i64), gdv_node_literal(i64, &k2, 0)};
  gdv_node_t* conj[2] = {gdv_node_function("greater_than", ga, 2, boolean), gdv_node_function("less_than", gb, 2, boolean)};
  gdv_filter_t* flt = nullptr;
  CHECK(gdv_filter_make(fschema, gdv_condition_new(gdv_node_and(conj, 2)), nullptr, &flt) == GDV_OK);

  const int NB = 64;
  printf("%8s %10s %10s %10s   %12s %12s %12s   %10s %10s   (microseconds per batch, %d batches per round; host+reg = host buffers in registered memory)\n", "rows", "proj sync",
         "proj async", "proj many", "filter sync", "filter async", "filter many", "proj host", "host+reg", NB);
  for (int64_t rows : {1024, 4096, 16384, 65536, 262144}) {
    const int64_t vbytes = ((rows + 63) / 64) * 8;
    // NB independent batches: inputs + outputs in HBM
    std::vector<std::vector<gdv_column_t>> cols(NB, std::vector<gdv_column_t>(4));
    std::vector<std::vector<gdv_out_column_t>> outs(NB, std::vector<gdv_out_column_t>(10));
    std::vector<gdv_batch_t> batches(NB);
    std::vector<double> host(rows);
    for (int64_t i = 0; i < rows; i++) host[i] = (double)(i % 1000) * 0.25 - 100.0;
    std::vector<uint8_t> bits(vbytes, 0xEF);
    for (int bch = 0; bch < NB; bch++) {
      for (int k = 0; k < 4; k++) {
        memset(&cols[bch][k], 0, sizeof(gdv_column_t));
        void *dv, *dd;
        CHECK(gdv_device_alloc(vbytes, &dv) == GDV_OK);
        CHECK(gdv_device_alloc(rows * 8, &dd) == GDV_OK);
        CHECK(gdv_memcpy_h2d(dv, bits.data(), vbytes) == GDV_OK);
        CHECK(gdv_memcpy_h2d(dd, host.data(), rows * 8) == GDV_OK);
        cols[bch][k].validity = dv; cols[bch][k].validity_size = vbytes;
        cols[bch][k].data = dd; cols[bch][k].data_size = rows * 8;
      }
      for (int e = 0; e < 10; e++) {
        memset(&outs[bch][e], 0, sizeof(gdv_out_column_t));
        void *dv, *dd;
        CHECK(gdv_device_alloc(vbytes, &dv) == GDV_OK);
        CHECK(gdv_device_alloc(rows * 8, &dd) == GDV_OK);
        outs[bch][e].validity = dv; outs[bch][e].validity_size = vbytes;
        outs[bch][e].data = dd; outs[bch][e].data_size = rows * 8;
      }
      batches[bch] = gdv_batch_t{rows, cols[bch].data(), 4, outs[bch].data(), 10};
    }
    auto time_rounds = [&](auto&& round) {
      round();  // warm-up
      CHECK(gdv_device_synchronize() == GDV_OK);
      double best = 1e9;
      for (int rep = 0; rep < 5; rep++) {
        const double t0 = Now();
        round();
        CHECK(gdv_device_synchronize() == GDV_OK);
        best = std::min(best, Now() - t0);
      }
      return best / NB * 1e6;
    };
    const double p_sync = time_rounds([&] {
      for (int bch = 0; bch < NB; bch++)
        CHECK(gdv_projector_evaluate(proj, rows, cols[bch].data(), 4, nullptr, outs[bch].data(), 10, GDV_MEM_DEVICE, nullptr, 0) == GDV_OK);
    });
    const double p_async = time_rounds([&] {
      for (int bch = 0; bch < NB; bch++)
        CHECK(gdv_projector_evaluate(proj, rows, cols[bch].data(), 4, nullptr, outs[bch].data(), 10, GDV_MEM_DEVICE, nullptr, GDV_EVAL_ASYNC) == GDV_OK);
    });
    const double p_many = time_rounds([&] { CHECK(gdv_projector_evaluate_many(proj, batches.data(), NB, nullptr, 0) == GDV_OK); });
    // filter over the first two columns reinterpreted as int64 (the bit patterns do not matter for timing)
    void* idx;
    CHECK(gdv_device_alloc(rows * 4 + 64, &idx) == GDV_OK);
    void* cnt;
    CHECK(gdv_device_alloc(64, &cnt) == GDV_OK);
    const double f_sync = time_rounds([&] {
      int64_t count = 0;
      for (int bch = 0; bch < NB; bch++)
        CHECK(gdv_filter_evaluate(flt, rows, cols[bch].data(), 2, GDV_SEL_UINT32, idx, rows, &count, GDV_MEM_DEVICE, nullptr) == GDV_OK);
    });
    const double f_async = time_rounds([&] {
      for (int bch = 0; bch < NB; bch++)
        CHECK(gdv_filter_evaluate_async(flt, rows, cols[bch].data(), 2, GDV_SEL_UINT32, idx, rows, cnt, nullptr) == GDV_OK);
    });
    // host buffers in and out (what pyarrow / JNI callers pass): staged through HBM by the library
    std::vector<std::vector<double>> hout(10, std::vector<double>(rows));
    std::vector<std::vector<uint8_t>> hval(10, std::vector<uint8_t>((rows + 7) / 8 + 8));
    gdv_column_t hc[4];
    gdv_out_column_t ho[10];
    for (int k = 0; k < 4; k++) {
      memset(&hc[k], 0, sizeof(hc[k]));
      hc[k].validity = bits.data(); hc[k].validity_size = (rows + 7) / 8;
      hc[k].data = host.data(); hc[k].data_size = rows * 8;
    }
    for (int e = 0; e < 10; e++) {
      memset(&ho[e], 0, sizeof(ho[e]));
      ho[e].validity = hval[e].data(); ho[e].validity_size = (rows + 7) / 8;
      ho[e].data = hout[e].data(); ho[e].data_size = rows * 8;
    }
    const double p_host = time_rounds([&] {
      for (int bch = 0; bch < NB; bch++)
        CHECK(gdv_projector_evaluate(proj, rows, hc, 4, nullptr, ho, 10, GDV_MEM_HOST, nullptr, 0) == GDV_OK);
    });
    // the same call with every buffer in page-locked memory of the library (gdv_host_alloc): the kernel reads and
    // writes the host buffers in place, nothing is staged
    double p_reg = 0;
    {
      const int64_t vb = ((rows + 63) / 64) * 8 + 64, db = rows * 8 + 64;
      void* block = nullptr;
      CHECK(gdv_host_alloc(4 * (vb + db) + 10 * (vb + db), &block) == GDV_OK);
      char* at = (char*)block;
      gdv_column_t rc[4];
      gdv_out_column_t ro[10];
      for (int k = 0; k < 4; k++) {
        memset(&rc[k], 0, sizeof(rc[k]));
        memcpy(at, bits.data(), (rows + 7) / 8); rc[k].validity = at; rc[k].validity_size = vb - 64; at += vb;
        memcpy(at, host.data(), rows * 8); rc[k].data = at; rc[k].data_size = rows * 8; at += db;
      }
      for (int e = 0; e < 10; e++) {
        memset(&ro[e], 0, sizeof(ro[e]));
        ro[e].validity = at; ro[e].validity_size = vb - 64; at += vb;
        ro[e].data = at; ro[e].data_size = rows * 8; at += db;
      }
      const long long staged0 = gdv_host_staged_bytes();
      p_reg = time_rounds([&] {
        for (int bch = 0; bch < NB; bch++)
          CHECK(gdv_projector_evaluate(proj, rows, rc, 4, nullptr, ro, 10, GDV_MEM_HOST, nullptr, 0) == GDV_OK);
      });
      if (gdv_host_staged_bytes() != staged0) { fprintf(stderr, "registered buffers were staged\n"); return 1; }
      if (memcmp(ro[3].data, hout[3].data(), rows * 8) != 0) { fprintf(stderr, "registered path: output differs\n"); return 1; }
      CHECK(gdv_host_free(block) == GDV_OK);
    }
    std::vector<void*> idxs(NB);
    std::vector<gdv_filter_batch_t> fb(NB);
    for (int bch = 0; bch < NB; bch++) {
      CHECK(gdv_device_alloc(rows * 4 + 64, &idxs[bch]) == GDV_OK);
      fb[bch] = gdv_filter_batch_t{rows, cols[bch].data(), 2, idxs[bch], rows};
    }
    std::vector<int64_t> counts(NB);
    const double f_many = time_rounds([&] {
      CHECK(gdv_filter_evaluate_many(flt, fb.data(), NB, GDV_SEL_UINT32, counts.data(), nullptr, nullptr, 0) == GDV_OK);
    });
    for (int bch = 0; bch < NB; bch++) gdv_device_free(idxs[bch]);
    printf("%8lld %10.1f %10.1f %10.1f   %12.1f %12.1f %12.1f   %10.1f %10.1f\n", (long long)rows, p_sync, p_async, p_many, f_sync, f_async, f_many, p_host, p_reg);
    fflush(stdout);
    for (int bch = 0; bch < NB; bch++) {
      for (int k = 0; k < 4; k++) { gdv_device_free((void*)cols[bch][k].validity); gdv_device_free((void*)cols[bch][k].data); }
      for (int e = 0; e < 10; e++) { gdv_device_free(outs[bch][e].validity); gdv_device_free(outs[bch][e].data); }
    }
    gdv_device_free(idx); gdv_device_free(cnt);
  }
  FilterProjectSection();
  return 0;
}

// ---------------------------------------------------------------- fused filter -> project over small batches
// 256 HBM-resident batches per round, every batch with inputs and outputs of its own; microseconds per batch, the MEDIAN
// of five rounds behind a warm-up round.  Two plans at ~12 % and ~100 % selected:
//   k2f        a > k1 AND b < k2, a + b projected, uint32 indices (the K2F workload's plan)
//   threshold  a > t; a + b, x * x, (a < b) OR f, if (b != 0) a / b else -1, k + 7; uint32 indices (tests/test_filter_project.py)
//   (a) sync   gdv_filter_project_evaluate, one batch per call, the call waits
//   (b) async  the same with GDV_EVAL_ASYNC and a device count word, one wait per round (a plan that can raise waits anyway)
//   (c) many   gdv_filter_project_evaluate_many over the 256 batches (one launch up to the plan's row cap)
//   (d) many1  gdv_filter_project_evaluate_many with one batch per call (the by-value entry)
//   (d*) / (c*)  (d) and (c) with the row cap lifted to 2^17 ("small_rows"): what one workgroup costs beyond the cap
//   filter     gdv_filter_evaluate_many on the predicate alone over the 256 batches (the neighbour figure)
namespace {

struct FpPlan {
  const char* name;
  gdv_schema_t* schema;
  int num_cols;
  gdv_filter_project_t* fp[2];  // ~12 %, ~100 %
  gdv_filter_t* flt[2];
  int num_outs;
  int out_width[5];             // bytes per row; 0 = a bitmap
};

template <typename F>
double MedianRound(int nb, F&& round) {
  round();
  CHECK(gdv_device_synchronize() == GDV_OK);
  std::vector<double> t;
  for (int rep = 0; rep < 5; rep++) {
    const double t0 = Now();
    round();
    CHECK(gdv_device_synchronize() == GDV_OK);
    t.push_back(Now() - t0);
  }
  std::sort(t.begin(), t.end());
  return t[2] / nb * 1e6;
}

}  // namespace

static void FilterProjectSection() {
  const gdv_type_t i64 = {GDV_TYPE_INT64, 0, 0}, f64 = {GDV_TYPE_DOUBLE, 0, 0}, i32 = {GDV_TYPE_INT32, 0, 0}, boolean = {GDV_TYPE_BOOL, 0, 0};
  auto fn2 = [](const char* name, gdv_node_t* x, gdv_node_t* y, gdv_type_t t) {
    gdv_node_t* args[2] = {x, y};
    return gdv_node_function(name, args, 2, t);
  };
  auto lit64 = [&](int64_t v) { return gdv_node_literal(i64, &v, 0); };
  FpPlan plans[2];
  {  // k2f
    FpPlan& p = plans[0];
    p = FpPlan{"k2f", gdv_schema_new(), 2, {nullptr, nullptr}, {nullptr, nullptr}, 1, {8, 0, 0, 0, 0}};
    CHECK(gdv_schema_add_field(p.schema, "a", i64, 1) == GDV_OK);
    CHECK(gdv_schema_add_field(p.schema, "b", i64, 1) == GDV_OK);
    const int64_t k1[2] = {499, -1}, k2[2] = {250, 1000000};
    for (int s = 0; s < 2; s++) {
      auto cond = [&] {
        gdv_node_t* conj[2] = {fn2("greater_than", gdv_node_field("a", i64), lit64(k1[s]), boolean),
                               fn2("less_than", gdv_node_field("b", i64), lit64(k2[s]), boolean)};
        return gdv_condition_new(gdv_node_and(conj, 2));
      };
      gdv_expression_t* ex[1] = {gdv_expression_new(fn2("add", gdv_node_field("a", i64), gdv_node_field("b", i64), i64), "s", i64)};
      CHECK(gdv_filter_project_make(p.schema, cond(), ex, 1, GDV_SEL_UINT32, nullptr, &p.fp[s]) == GDV_OK);
      CHECK(gdv_filter_make(p.schema, cond(), nullptr, &p.flt[s]) == GDV_OK);
    }
  }
  {  // threshold
    FpPlan& p = plans[1];
    p = FpPlan{"threshold", gdv_schema_new(), 5, {nullptr, nullptr}, {nullptr, nullptr}, 5, {8, 8, 0, 8, 4}};
    CHECK(gdv_schema_add_field(p.schema, "a", i64, 1) == GDV_OK);
    CHECK(gdv_schema_add_field(p.schema, "b", i64, 1) == GDV_OK);
    CHECK(gdv_schema_add_field(p.schema, "x", f64, 1) == GDV_OK);
    CHECK(gdv_schema_add_field(p.schema, "k", i32, 1) == GDV_OK);
    CHECK(gdv_schema_add_field(p.schema, "f", boolean, 1) == GDV_OK);
    const int64_t thr[2] = {879, -1};
    for (int s = 0; s < 2; s++) {
      auto A = [&] { return gdv_node_field("a", i64); };
      auto B = [&] { return gdv_node_field("b", i64); };
      auto cond = [&] { return gdv_condition_new(fn2("greater_than", A(), lit64(thr[s]), boolean)); };
      gdv_node_t* either[2] = {fn2("less_than", A(), B(), boolean), gdv_node_field("f", boolean)};
      const int32_t seven = 7;
      gdv_expression_t* ex[5] = {
          gdv_expression_new(fn2("add", A(), B(), i64), "s", i64),
          gdv_expression_new(fn2("multiply", gdv_node_field("x", f64), gdv_node_field("x", f64), f64), "xx", f64),
          gdv_expression_new(gdv_node_or(either, 2), "lt_or_f", boolean),
          gdv_expression_new(gdv_node_if(fn2("not_equal", B(), lit64(0), boolean), fn2("divide", A(), B(), i64), lit64(-1), i64), "q", i64),
          gdv_expression_new(fn2("add", gdv_node_field("k", i32), gdv_node_literal(i32, &seven, 0), i32), "k7", i32)};
      CHECK(gdv_filter_project_make(p.schema, cond(), ex, 5, GDV_SEL_UINT32, nullptr, &p.fp[s]) == GDV_OK);
      CHECK(gdv_filter_make(p.schema, cond(), nullptr, &p.flt[s]) == GDV_OK);
    }
  }
  const int NB = 256;
  printf("\nfused filter-project, %d batches per round, microseconds per batch (median of 5 rounds); cap = rows per batch of the one-launch path\n", NB);
  printf("%10s %5s %8s %8s %9s %9s %9s %9s %9s %9s %9s\n", "plan", "sel", "rows", "cap", "(a) sync", "(b) async", "(c) many", "(d) many1",
         "(d*)", "(c*)", "filter");
  for (int64_t rows : {1024, 4096, 16384, 65536}) {
    const int64_t vbytes = ((rows + 63) / 64) * 8;
    std::vector<int64_t> ha(rows), hb_k2f(rows), hb_thr(rows);
    std::vector<double> hx(rows);
    std::vector<int32_t> hk(rows);
    std::vector<uint8_t> ones(vbytes, 0xFF), hf(vbytes);
    uint64_t state = 88172645463325252ull;
    auto next = [&] { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
    for (int64_t i = 0; i < rows; i++) {
      ha[i] = (int64_t)(next() % 1000); hb_k2f[i] = (int64_t)(next() % 1000); hb_thr[i] = (int64_t)(next() % 8);
      hx[i] = (double)(next() % 4096) * 0.5; hk[i] = (int32_t)(next() % 100000);
    }
    for (auto& byte : hf) byte = (uint8_t)next();
    for (FpPlan& p : plans) {
      // NB batches with inputs, outputs, indices of their own
      std::vector<void*> owned;
      auto dev = [&](int64_t bytes, const void* src) {
        void* d = nullptr;
        CHECK(gdv_device_alloc(bytes, &d) == GDV_OK);
        if (src != nullptr) CHECK(gdv_memcpy_h2d(d, src, bytes) == GDV_OK);
        owned.push_back(d);
        return d;
      };
      std::vector<std::vector<gdv_column_t>> cols(NB, std::vector<gdv_column_t>(p.num_cols));
      std::vector<std::vector<gdv_out_column_t>> outs(NB, std::vector<gdv_out_column_t>(p.num_outs));
      std::vector<gdv_filter_project_batch_t> fpb(NB);
      std::vector<gdv_filter_batch_t> fb(NB);
      void* counts_dev = dev(8 * NB, nullptr);
      for (int b = 0; b < NB; b++) {
        const void* src[5] = {ha.data(), p.num_cols == 2 ? (const void*)hb_k2f.data() : (const void*)hb_thr.data(), hx.data(), hk.data(), hf.data()};
        const int64_t bytes[5] = {rows * 8, rows * 8, rows * 8, rows * 4, vbytes};
        for (int k = 0; k < p.num_cols; k++) {
          memset(&cols[b][k], 0, sizeof(gdv_column_t));
          cols[b][k].validity = dev(vbytes, ones.data()); cols[b][k].validity_size = vbytes;
          cols[b][k].data = dev(bytes[k], src[k]); cols[b][k].data_size = bytes[k];
        }
        for (int e = 0; e < p.num_outs; e++) {
          memset(&outs[b][e], 0, sizeof(gdv_out_column_t));
          const int64_t dbytes = p.out_width[e] == 0 ? vbytes : rows * p.out_width[e];
          outs[b][e].validity = dev(vbytes, nullptr); outs[b][e].validity_size = vbytes;
          outs[b][e].data = dev(dbytes, nullptr); outs[b][e].data_size = dbytes;
        }
        void* idx = dev(rows * 4, nullptr);
        fpb[b] = gdv_filter_project_batch_t{rows, cols[b].data(), p.num_cols, outs[b].data(), p.num_outs, idx, rows};
        fb[b] = gdv_filter_batch_t{rows, cols[b].data(), p.num_cols, idx, rows};
      }
      std::vector<int64_t> counts(NB);
      for (int s = 0; s < 2; s++) {
        gdv_filter_project_t* fp = p.fp[s];
        const double t_sync = MedianRound(NB, [&] {
          for (int b = 0; b < NB; b++)
            CHECK(gdv_filter_project_evaluate(fp, rows, fpb[b].cols, p.num_cols, fpb[b].outs, p.num_outs, fpb[b].out_indices, rows, &counts[b],
                                              nullptr, GDV_MEM_DEVICE, nullptr, 0) == GDV_OK);
        });
        const int64_t want0 = counts[0];
        const double t_async = MedianRound(NB, [&] {
          for (int b = 0; b < NB; b++)
            CHECK(gdv_filter_project_evaluate(fp, rows, fpb[b].cols, p.num_cols, fpb[b].outs, p.num_outs, fpb[b].out_indices, rows, &counts[b],
                                              (char*)counts_dev + 8 * b, GDV_MEM_DEVICE, nullptr, GDV_EVAL_ASYNC) == GDV_OK);
        });
        auto many = [&] { CHECK(gdv_filter_project_evaluate_many(fp, fpb.data(), NB, counts.data(), nullptr, nullptr, 0) == GDV_OK); };
        auto many1 = [&] {
          for (int b = 0; b < NB; b++) CHECK(gdv_filter_project_evaluate_many(fp, &fpb[b], 1, &counts[b], nullptr, nullptr, 0) == GDV_OK);
        };
        const long long cap = (long long)gdv_filter_project_small_batch_rows(fp);
        const double t_many = MedianRound(NB, many);
        if (counts[0] != want0 || counts[NB - 1] != want0) { fprintf(stderr, "evaluate_many: count %lld, one batch %lld\n", (long long)counts[0], (long long)want0); exit(1); }
        const double t_many1 = MedianRound(NB, many1);
        CHECK(gdv_filter_project_set_tuning(fp, "small_rows", 131072) == GDV_OK);
        const double t_many1_lifted = MedianRound(NB, many1);
        const double t_many_lifted = MedianRound(NB, many);
        if (counts[0] != want0 || counts[NB - 1] != want0) { fprintf(stderr, "evaluate_many (cap lifted): count %lld, one batch %lld\n", (long long)counts[0], (long long)want0); exit(1); }
        CHECK(gdv_filter_project_set_tuning(fp, "small_rows", 0) == GDV_OK);
        const double t_filter = MedianRound(NB, [&] {
          CHECK(gdv_filter_evaluate_many(p.flt[s], fb.data(), NB, GDV_SEL_UINT32, counts.data(), nullptr, nullptr, 0) == GDV_OK);
        });
        printf("%10s %4.0f%% %8lld %8lld %9.1f %9.1f %9.1f %9.1f %9.1f %9.1f %9.1f\n", p.name, 100.0 * (double)want0 / (double)rows, (long long)rows,
               cap, t_sync, t_async, t_many, t_many1, t_many1_lifted, t_many_lifted, t_filter);
        fflush(stdout);
      }
      for (void* d : owned) gdv_device_free(d);
    }
  }
}
