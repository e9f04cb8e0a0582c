// Stand-alone program over the HOST build of the decimal128 core (gdv_device_lib.hpp: add subtract multiply divide mod, the
// compare, castDECIMAL, castBIGINT, castFLOAT8, castVARCHAR, abs, negative, round truncate ceil floor), meant to be built with
// -fsanitize=address,undefined and run as a child process (tests/test_full_range_decimal_cpu.py).  It reads rows
//   xp xs yp ys  (op os) x 5  x y        (result types of add subtract multiply divide mod; x, y: unscaled values in decimal text)
// from the file named first — the anchor cross product of every type pair: the extremes +-(10^p - 1), zero, +-1 and the limb
// boundaries, where a signed overflow in gdv_dec_rescale_up, in r * gdv_pow10_128(..) of gdv_dec_round_to or in -x would be
// reported as a runtime error — and writes, per row, the results of the five operators (a zero divisor replaced by 1) and the
// three-way compare to the file named second; the test holds them to its reference.  The unary functions run on x with every
// k of the edge list, for the sanitizers alone.  Prints "decimal_core_check: ok".
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

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

static gdv_int128 parse(const char* s) {
  const bool neg = *s == '-';
  if (neg) s++;
  unsigned __int128 m = 0;
  for (; *s >= '0' && *s <= '9'; s++) m = m * 10 + (unsigned)(*s - '0');
  return neg ? -(gdv_int128)m : (gdv_int128)m;
}
static std::string text(gdv_int128 v) {
  unsigned __int128 m = v < 0 ? (unsigned __int128)0 - (unsigned __int128)v : (unsigned __int128)v;
  char buf[48];
  int at = 47;
  buf[at] = 0;
  do { buf[--at] = (char)('0' + (int)(m % 10)); m /= 10; } while (m != 0);
  if (v < 0) buf[--at] = '-';
  return std::string(buf + at);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "r");
  FILE* out = std::fopen(argv[2], "w");
  if (!in || !out) return 2;
  const int ks[] = {0, 1, 4, 37, 38, 39, -1, -37, -38, -39, INT_MIN, INT_MAX};
  const int targets[][2] = {{38, 1}, {20, 4}, {5, 0}, {38, 38}, {38, 0}};
  int xp, xs, yp, ys, rt[5][2];
  char xt[64], yt[64];
  long rows = 0;
  double sink = 0;
  unsigned err = 0;
  gdv_ctx ctx{&err};
  unsigned char buf[64];
  while (std::fscanf(in, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %63s %63s", &xp, &xs, &yp, &ys, &rt[0][0], &rt[0][1], &rt[1][0], &rt[1][1],
                     &rt[2][0], &rt[2][1], &rt[3][0], &rt[3][1], &rt[4][0], &rt[4][1], xt, yt) == 16) {
    const gdv_int128 x = parse(xt), y = parse(yt), d = y == 0 ? 1 : y;
    const gdv_int128 r[5] = {add_decimal128_decimal128(x, xp, xs, y, yp, ys, rt[0][0], rt[0][1]),
                             subtract_decimal128_decimal128(x, xp, xs, y, yp, ys, rt[1][0], rt[1][1]),
                             multiply_decimal128_decimal128(x, xp, xs, y, yp, ys, rt[2][0], rt[2][1]),
                             divide_decimal128_decimal128(ctx, x, xp, xs, d, yp, ys, rt[3][0], rt[3][1]),
                             mod_decimal128_decimal128(ctx, x, xp, xs, d, yp, ys, rt[4][0], rt[4][1])};
    std::fprintf(out, "%s %s %s %s %s %d\n", text(r[0]).c_str(), text(r[1]).c_str(), text(r[2]).c_str(), text(r[3]).c_str(), text(r[4]).c_str(),
                 gdv_dec_compare(x, xp, xs, y, yp, ys));
    // the unary functions: only that they run clean (their values are held to the reference through the host library)
    gdv_int128 acc = negative_decimal128(x, xp, xs, xp, xs) ^ abs_decimal128(x, xp, xs, xp, xs);
    for (const auto& t : targets) acc ^= castDECIMAL_decimal128(x, xp, xs, t[0], t[1]);
    for (int k : ks)
      for (const auto& t : targets)
        acc ^= round_decimal128_int32(x, xp, xs, k, t[0], t[1]) ^ truncate_decimal128_int32(x, xp, xs, k, t[0], t[1]);
    acc ^= round_decimal128(x, xp, xs, 38, 0) ^ truncate_decimal128(x, xp, xs, 38, 0) ^ ceil_decimal128(x, xp, xs, 38, 0) ^ floor_decimal128(x, xp, xs, 38, 0);
    acc ^= castBIGINT_decimal128(x, xp, xs, 0, 0);
    sink += castFLOAT8_decimal128(x, xp, xs, 0, 0) + (double)(long long)acc;
    for (long long n : {0LL, 1LL, 39LL, 40LL, 41LL}) {
      const gdv_str s = castVARCHAR_decimal128_int64(ctx, x, xp, xs, n, 0, 0);
      gdv_str_copy(buf, s);
      sink += s.len;
    }
    rows++;
  }
  std::fclose(in);
  std::fclose(out);
  if (err != 0 || rows == 0) {
    std::printf("decimal_core_check: error bits %u over %ld rows\n", err, rows);
    return 1;
  }
  std::printf("decimal_core_check: ok (%ld rows, %g)\n", rows, sink);
  return 0;
}
