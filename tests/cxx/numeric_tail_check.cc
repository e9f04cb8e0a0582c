// Stand-alone program over the HOST build of the numeric tail's integer functions (gdv_device_lib.hpp: pmod, round / truncate
// to a scale, shifts, gcd / lcm, sign) and the float round to a scale, meant to be built with -fsanitize=address,undefined and
// run as a child process (tests/test_numeric_tail_cpu.py).  Every function runs over the cross product of the edge rows —
// INT_MIN, -1, 0, counts 31 / 32 / 63 / 64 / -1, scales -9 / -10 / -18 / -19 and INT32_MIN — where a signed overflow, a shift
// by the width or a division of INT_MIN by -1 would be reported as a runtime error; results are compared with a restatement
// in 128-bit integers.  Prints "numeric_tail_check: ok".
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

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

#include "gdv_device_lib.hpp"

typedef __int128 wide;
static int failures = 0;
static long rows = 0;

static void expect(const char* what, long long a, long long b, long long got, wide want, int width) {
  rows++;
  const long long w = width == 32 ? (long long)(int32_t)(uint32_t)(unsigned __int128)want : (long long)(uint64_t)(unsigned __int128)want;
  if (got != w && failures++ < 20) std::printf("FAIL %s(%lld, %lld) = %lld, want %lld\n", what, a, b, got, w);
}

static wide floor_mod(wide a, wide n) {
  if (n == 0) return a;
  wide r = a % n;
  if (r != 0 && ((r < 0) != (n < 0))) r += n;
  return r;
}
static wide to_scale(wide a, long long s, int max_scale, bool half) {
  if (s >= 0) return a;
  if (s < -(long long)max_scale) return 0;
  wide p = 1;
  for (long long i = 0; i < -s; i++) p *= 10;
  const wide mag = a < 0 ? -a : a;
  wide q = mag / p * p;
  if (half && 2 * (mag - q) >= p) q += p;
  return a < 0 ? -q : q;
}
static wide gcd_wide(wide a, wide b) {
  a = a < 0 ? -a : a;
  b = b < 0 ? -b : b;
  while (b != 0) { const wide t = a % b; a = b; b = t; }
  return a;
}

int main() {
  const std::vector<long long> v64 = {LLONG_MIN, LLONG_MIN + 1, -1000000000000000000LL, -4294967296LL, -2147483649LL, -2147483648LL, -125, -7, -5,
                                      -1, 0, 1, 3, 4, 5, 6, 7, 125, 2147483647LL, 2147483648LL, 4294967295LL, 499999999999999999LL,
                                      500000000000000000LL, 4611686018427387904LL, LLONG_MAX - 1, LLONG_MAX};
  const std::vector<int> v32 = {INT_MIN, INT_MIN + 1, -1000000000, -65536, -125, -7, -5, -1, 0, 1, 3, 4, 5, 6, 7, 125, 65535, 499999999, 500000000,
                                1073741824, 1500000000, INT_MAX - 1, INT_MAX};
  const std::vector<int> counts = {INT_MIN, -309, -308, -65, -64, -63, -33, -32, -31, -19, -18, -17, -10, -9, -8, -2, -1, 0, 1, 2, 8, 9, 10, 18, 19,
                                   31, 32, 33, 63, 64, 65, 308, 309, INT_MAX};
  for (int a : v32) {
    expect("sign_int32", a, 0, sign_int32(a), (a > 0) - (a < 0), 32);
    expect("round_int32", a, 0, round_int32(a), a, 32);
    for (int b : v32) expect("pmod_int32", a, b, pmod_int32_int32(a, b), floor_mod(a, b), 32);
    for (int c : counts) {
      expect("round_int32_int32", a, c, round_int32_int32(a, c), to_scale(a, c, 9, true), 32);
      expect("truncate_int32_int32", a, c, truncate_int32_int32(a, c), to_scale(a, c, 9, false), 32);
      const int k = (int)((unsigned)c & 31u);
      expect("shift_left_int32", a, c, shift_left_int32_int32(a, c), (wide)a * ((wide)1 << k), 32);
      expect("shift_right_int32", a, c, shift_right_int32_int32(a, c), (wide)a >> k, 32);
      expect("shift_right_unsigned_int32", a, c, shift_right_unsigned_int32_int32(a, c), (wide)((uint32_t)a >> k), 32);
    }
  }
  for (long long a : v64) {
    expect("sign_int64", a, 0, sign_int64(a), (a > 0) - (a < 0), 64);
    expect("round_int64", a, 0, round_int64(a), a, 64);
    for (long long b : v64) {
      expect("pmod_int64", a, b, pmod_int64_int64(a, b), floor_mod(a, b), 64);
      const wide g = gcd_wide(a, b);
      expect("gcd_int64", a, b, gcd_int64_int64(a, b), g, 64);
      const wide ma = a < 0 ? -(wide)a : (wide)a, mb = b < 0 ? -(wide)b : (wide)b;
      expect("lcm_int64", a, b, lcm_int64_int64(a, b), g == 0 ? 0 : ma / g * mb, 64);
    }
    for (int c : counts) {
      expect("round_int64_int32", a, c, round_int64_int32(a, c), to_scale(a, c, 18, true), 64);
      expect("truncate_int64_int32", a, c, truncate_int64_int32(a, c), to_scale(a, c, 18, false), 64);
      const int k = (int)((unsigned)c & 63u);
      expect("shift_left_int64", a, c, shift_left_int64_int32(a, c), (wide)((unsigned __int128)(uint64_t)a << k), 64);
      expect("shift_right_int64", a, c, shift_right_int64_int32(a, c), (wide)a >> k, 64);
      expect("shift_right_unsigned_int64", a, c, shift_right_unsigned_int64_int32(a, c), (wide)((uint64_t)a >> k), 64);
    }
  }
  // the float forms: every scale of the table and the ones past its ends (an index outside the table would be reported)
  const double xs[] = {0.0, -0.0, 2.5, -0.125, 1e308, -1e308, 5e-324, 1234.5678, INFINITY, -INFINITY, NAN};
  for (double x : xs)
    for (int s = -320; s <= 320; s++) {
      const double r = round_float64_int32(x, s);
      const float rf = round_float32_int32((float)x, s);
      rows += 2;
      if (std::isnan(x) != std::isnan(r) || std::isnan((float)x) != std::isnan(rf)) failures++;
    }
  for (int s : {INT_MIN, INT_MAX}) rows += round_float64_int32(2.5, s) == (s > 0 ? 2.5 : 0.0);
  if (round_float64_int32(2.5, 0) != 3.0 || round_float64_int32(-0.125, 2) != -0.13 || round_float64_int32(1e308, 10) != 1e308) failures++;
  if (failures) {
    std::printf("numeric_tail_check: %d failures over %ld rows\n", failures, rows);
    return 1;
  }
  std::printf("numeric_tail_check: ok (%ld rows)\n", rows);
  return 0;
}
