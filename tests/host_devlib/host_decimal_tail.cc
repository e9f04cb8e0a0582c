// Test-only HOST build of the decimal tail of the device library: castDECIMAL of float32 / float64 / text,
// castDECIMALNullOnOverflow, nvl / greatest / least, the null-safe comparisons and the hash family over decimal128.  Built
// and driven by tests/test_decimal_tail_cpu.py the way test_encode_cpu.py drives host_encode.cc.  A decimal128 crosses the
// boundary as two uint64 (low, high).
#include <cmath>
#include <cstdint>
#include <cstring>

#define GDV_HOST_BUILD 1
#define __device__
#define __forceinline__ inline
static inline unsigned atomicOr(unsigned* p, unsigned v) { unsigned o = *p; *p |= v; return o; }
#define __builtin_nontemporal_load(p) (*(p))
#define __builtin_nontemporal_store(v, p) (*(p) = (v))
#define __builtin_amdgcn_readlane(v, l) (v)
#define __builtin_amdgcn_readfirstlane(v) (v)
#define __builtin_amdgcn_update_dpp(old, src, ctrl, rm, bm, bc) (old)
#define __builtin_amdgcn_wave_barrier() ((void)0)
static inline unsigned long long __ballot(bool x) { return x ? 1ull : 0ull; }
static inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
static inline long long __double_as_longlong(double d) { long long r; std::memcpy(&r, &d, 8); return r; }
static inline double __longlong_as_double(long long v) { double r; std::memcpy(&r, &v, 8); return r; }
static inline unsigned __float_as_uint(float f) { unsigned r; std::memcpy(&r, &f, 4); return r; }
static inline float __uint_as_float(unsigned v) { float r; std::memcpy(&r, &v, 4); return r; }

#include "../../gandiva_amd/csrc/gdv_device_lib.hpp"

namespace {
gdv_int128 get128(const unsigned long long* p, long i) { return gdv_make_int128(p[2 * i + 1], p[2 * i]); }
void put128(unsigned long long* p, long i, gdv_int128 v) {
  p[2 * i] = (unsigned long long)v;
  p[2 * i + 1] = (unsigned long long)((gdv_uint128)v >> 64);
}
}  // namespace

extern "C" {

// castDECIMAL(text) over the rows of (off, data); the buffer ends exactly at `size` (views claim nothing beyond it);
// valid[i] == 0: a null row, the function is not called (as in a plan).  text_map: read through upper (1) / lower (2).
// err_rows[i] = the row's error bits.
void host_cast_text(const int* off, const unsigned char* data, long size, const unsigned char* valid, long n, int text_map,
                    int op, int os, unsigned long long* out, unsigned char* err_rows) {
  for (long i = 0; i < n; i++) {
    unsigned err = 0;
    gdv_ctx ctx{&err};
    gdv_int128 r = 0;
    if (valid[i]) {
      gdv_str s = gdv_make_str(data, off[i], off[i + 1], data + size, 0);
      if (text_map == 1) s = upper_utf8(s);
      if (text_map == 2) s = lower_utf8(s);
      r = castDECIMAL_utf8(ctx, s, op, os);
    }
    put128(out, i, r);
    err_rows[i] = (unsigned char)err;
  }
}

void host_cast_f64(const double* v, long n, int op, int os, unsigned long long* out) {
  for (long i = 0; i < n; i++) put128(out, i, castDECIMAL_float64(v[i], op, os));
}
void host_cast_f32(const float* v, long n, int op, int os, unsigned long long* out) {
  for (long i = 0; i < n; i++) put128(out, i, castDECIMAL_float32(v[i], op, os));
}

void host_cast_null_on_overflow(const unsigned long long* x, const unsigned char* valid, long n, int xp, int xs, int op, int os,
                                unsigned long long* out, unsigned char* out_valid) {
  for (long i = 0; i < n; i++) {
    bool ov = true;
    put128(out, i, castDECIMALNullOnOverflow_decimal128(get128(x, i), xp, xs, valid[i] != 0, op, os, &ov));
    out_valid[i] = ov ? 1 : 0;
  }
}

// fn: 0 nvl, 1 greatest, 2 least over one (p, s); out_valid: nvl's own, the conjunction for the other two
void host_pick(int fn, const unsigned long long* a, const unsigned char* av, const unsigned long long* b, const unsigned char* bv,
               long n, int p, int s, unsigned long long* out, unsigned char* out_valid) {
  for (long i = 0; i < n; i++) {
    bool ov = av[i] && bv[i];
    gdv_int128 r = 0;
    if (fn == 0) r = nvl_decimal128_decimal128(get128(a, i), p, s, av[i] != 0, get128(b, i), p, s, bv[i] != 0, p, s, &ov);
    else if (ov) r = fn == 1 ? greatest_decimal128_decimal128(get128(a, i), p, s, get128(b, i), p, s, p, s)
                             : least_decimal128_decimal128(get128(a, i), p, s, get128(b, i), p, s, p, s);
    put128(out, i, r);
    out_valid[i] = ov ? 1 : 0;
  }
}

void host_distinct(const unsigned long long* a, const unsigned char* av, int ap, int as_, const unsigned long long* b,
                   const unsigned char* bv, int bp, int bs, long n, unsigned char* distinct, unsigned char* not_distinct) {
  for (long i = 0; i < n; i++) {
    distinct[i] = is_distinct_from_decimal128_decimal128(get128(a, i), ap, as_, av[i] != 0, get128(b, i), bp, bs, bv[i] != 0);
    not_distinct[i] = is_not_distinct_from_decimal128_decimal128(get128(a, i), ap, as_, av[i] != 0, get128(b, i), bp, bs, bv[i] != 0);
  }
}

void host_hash(const unsigned long long* x, const unsigned char* valid, const int* seed32, const long long* seed64,
               const unsigned char* seed_valid, long n, int* h32, int* h32s, long long* h64, long long* h64s) {
  for (long i = 0; i < n; i++) {
    const gdv_int128 v = get128(x, i);
    h32[i] = hash32_decimal128(v, 38, 0, valid[i] != 0);
    h32s[i] = hash32_decimal128_int32(v, 38, 0, valid[i] != 0, seed32[i], seed_valid[i] != 0);
    h64[i] = hash64_decimal128(v, 38, 0, valid[i] != 0);
    h64s[i] = hash64_decimal128_int64(v, 38, 0, valid[i] != 0, seed64[i], seed_valid[i] != 0);
  }
}

}  // extern "C"
