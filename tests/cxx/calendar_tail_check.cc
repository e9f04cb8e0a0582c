// Stand-alone program over the HOST build of the calendar tail (gdv_device_lib.hpp: months_between, next_day, add_months),
// meant to be built with -fsanitize=address,undefined and run as a child process (tests/test_calendar_tail_cpu.py).  Every
// function runs over the cross product of the edge rows — INT64_MIN, INT64_MAX, 0, +-1, a day +-1 ms, month ends and leap
// days, weekday numbers 0, 8, negative ones and INT32_MIN, counts up to +-2^31 — where a signed overflow would be reported as
// a runtime error.  add_months only on rows whose exact result stays inside int64 (timestampaddMonth's own rule: its
// arithmetic is signed).  Results are held to properties restated in 128-bit integers.  Prints "calendar_tail_check: ok".
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
static const long long MS = 86400000LL;
static int failures = 0;
static long rows = 0;

static void check(bool ok, const char* what, long long a, long long b) {
  rows++;
  if (!ok && failures++ < 20) std::printf("FAIL %s(%lld, %lld)\n", what, a, b);
}
static wide floor_div(wide a, wide n) {
  const wide q = a / n;
  return (a % n != 0 && ((a < 0) != (n < 0))) ? q - 1 : q;
}
static wide floor_mod(wide a, wide n) { return a - floor_div(a, n) * n; }

int main() {
  std::vector<long long> v = {LLONG_MIN, LLONG_MIN + 1, LLONG_MAX, LLONG_MAX - 1, LLONG_MAX - 7 * MS, LLONG_MAX - 8 * MS, 0, 1, -1, MS, MS + 1, MS - 1,
                              -MS, -MS + 1, -MS - 1, 4611686018427387904LL, -4611686018427387904LL};
  const int dates[][3] = {{0, 2, 29}, {0, 3, 1}, {1, 1, 1}, {-1, 12, 31}, {1900, 2, 28}, {1996, 10, 30}, {1997, 2, 28}, {2000, 2, 29}, {2015, 1, 14},
                          {2023, 1, 31}, {2023, 3, 31}, {2024, 2, 29}, {2100, 2, 28}, {9999, 12, 31}};
  for (auto& d : dates) {
    const long long day = gdv_days_from_civil(d[0], d[1], d[2]);
    v.push_back(day * MS);
    v.push_back(day * MS + MS - 1);
    v.push_back(day * MS + 37800000LL);  // 10:30:00
  }
  const std::vector<int> dows = {INT_MIN, INT_MIN + 1, -14, -8, -7, -6, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 14, 15, INT_MAX - 1, INT_MAX};
  const std::vector<long long> counts = {0, 1, -1, 11, 12, -12, -13, 1200, -1200, 2147483647LL, -2147483648LL, 4294967296LL, LLONG_MAX, LLONG_MIN};

  for (long long a : v) {
    for (long long b : v) {
      const double m = months_between_timestamp_timestamp(a, b), r = months_between_date64_date64(b, a);
      check(m == -r && std::isfinite(m), "months_between is antisymmetric", a, b);
      check(std::fabs(m) < 8.6e9, "months_between stays below 2^33", a, b);
    }
    check(months_between_timestamp_timestamp(a, a) == 0.0, "months_between of an instant and itself", a, a);
    const wide day = floor_div(a, MS);
    for (int dow : dows) {
      const long long got = next_day_timestamp_int32(a, dow);
      const wide want_dow = floor_mod((wide)dow - 1, 7) + 1;
      // the exact result, found by walking: the first of the next seven days with the weekday (day 0 was a Thursday = 5)
      wide exact = 0;
      for (int k = 1; k <= 7; k++)
        if (floor_mod(day + k + 4, 7) + 1 == want_dow) exact = (day + k) * MS;
      check(got == (long long)(uint64_t)(unsigned __int128)exact, "next_day", a, dow);
      check(next_day_date64_int32(a, dow) == got, "next_day over date64", a, dow);
    }
    for (long long n : counts) {
      const wide mag_v = a < 0 ? -(wide)a : (wide)a, mag_n = n < 0 ? -(wide)n : (wide)n;
      if (mag_v + (mag_n + 2) * 31 * MS >= (wide)LLONG_MAX) continue;  // the exact result may leave int64: left out
      const long long got = add_months_timestamp_int64(a, n);
      check(got == timestampaddMonth_int64_timestamp(n, a) && got == add_months_date64_int64(a, n), "add_months(t, int64)", a, n);
      if (n >= INT_MIN && n <= INT_MAX)
        check(add_months_timestamp_int32(a, (int)n) == got && add_months_date64_int32(a, (int)n) == got, "add_months(t, int32)", a, n);
      const gdv_ymd from = gdv_civil_from_days(gdv_floor_div(a, MS)), to = gdv_civil_from_days(gdv_floor_div(got, MS));
      const wide months = (wide)from.y * 12 + (from.m - 1) + n;
      const int last = gdv_last_day_of_month(to.y, to.m);
      check((wide)to.y * 12 + (to.m - 1) == months && to.d == (from.d < last ? from.d : last) &&
                gdv_floor_mod(got, MS) == gdv_floor_mod(a, MS), "add_months: month, clamped day, time of day", a, n);
    }
  }
  // the hand vectors: Hive's documentation, and a Wednesday's next Tuesday
  const long long e = gdv_days_from_civil(1997, 2, 28) * MS + 37800000LL, s = gdv_days_from_civil(1996, 10, 30) * MS;
  check(months_between_timestamp_timestamp(e, s) == 4.0 + (-2.0 + 0.4375) / 31.0, "months_between hand vector", e, s);
  check(next_day_date64_int32(gdv_days_from_civil(2015, 1, 14) * MS, 3) == gdv_days_from_civil(2015, 1, 20) * MS, "next_day hand vector", 0, 3);
  if (failures) {
    std::printf("calendar_tail_check: %d failures over %ld rows\n", failures, rows);
    return 1;
  }
  std::printf("calendar_tail_check: ok (%ld rows)\n", rows);
  return 0;
}
