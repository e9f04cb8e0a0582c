// Stand-alone program over the HOST build of the text-to-decimal parser (gdv_device_lib.hpp, castDECIMAL_utf8), meant to be
// built with -fsanitize=address,undefined and run as a child process (tests/test_decimal_tail_cpu.py).  Every text is copied
// into a heap block of exactly its length, so a read one byte past the text is a heap-buffer-overflow; every prefix of a few
// long texts is parsed, and a handful of known answers is checked.  Prints "decimal_parse_check: ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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

static int failures = 0;

// the text in a block of exactly its size (length 0: a one-byte block the view must not touch, handed over past its end)
static bool parse(const std::string& text, int op, int os, int map, gdv_int128* out) {
  const size_t n = text.size();
  unsigned char* block = static_cast<unsigned char*>(std::malloc(n ? n : 1));
  if (n) std::memcpy(block, text.data(), n);
  const unsigned char* base = n ? block : block + 1;
  gdv_str s = gdv_make_str(base, 0, static_cast<gdv_int32>(n), base + n, 0);
  s.map = map;
  unsigned err = 0;
  gdv_ctx ctx{&err};
  *out = castDECIMAL_utf8(ctx, s, op, os);
  std::free(block);
  if (err != 0 && err != GDV_ERR_BAD_ARG) { std::printf("FAIL: error bits %u for '%s'\n", err, text.c_str()); failures++; }
  return err == 0;
}

static void expect(const std::string& text, int op, int os, bool ok, long long want) {
  gdv_int128 v = 0;
  const bool got = parse(text, op, os, 0, &v);
  if (got != ok || (ok && v != (gdv_int128)want)) {
    std::printf("FAIL: '%s' at (%d, %d): taken %d value %lld, want taken %d value %lld\n", text.c_str(), op, os, (int)got, (long long)v,
                (int)ok, want);
    failures++;
  }
}

int main() {
  for (const char* t : {"5.", ".5", "+.5", "-.5e1", "1.e1", "1e05", "1e-0"}) { gdv_int128 v; if (!parse(t, 38, 2, 0, &v)) { std::printf("FAIL: '%s' refused\n", t); failures++; } }
  for (const char* t : {"", " ", ".", "+", "1e", "1e+", ".e5", "1..", "1e 5", "1e5 ", " 1.2", "1,5", "1e+-5", "1e1234567890", "\xd9\xa1"}) expect(t, 38, 2, false, 0);
  expect("5.", 38, 2, true, 500);
  expect("-.5e1", 38, 2, true, -500);
  expect("1.005", 38, 2, true, 101);
  expect("-1.005", 38, 2, true, -101);
  expect("1.00499999999999999999999999999999999999999999999", 38, 2, true, 100);
  expect("0.5", 5, 0, true, 1);
  expect("0.49", 5, 0, true, 0);
  expect("5e-1", 5, 0, true, 1);
  expect("5e-2", 5, 0, true, 0);
  expect("12e3", 15, 2, true, 1200000);
  expect("99999.5", 5, 0, true, 0);     // rounds to six digits: overflow, 0
  expect("99999.4", 5, 0, true, 99999);
  expect("1e999999999", 38, 0, true, 0);
  expect("0e999999999", 38, 0, true, 0);
  expect("-69e58", 38, 0, true, 0);
  expect("0.9", 1, 1, true, 9);
  expect("1", 1, 1, true, 0);
  expect("1E2", 38, 0, true, 100);

  // every prefix of a few long texts, at several target types, through each byte map
  const std::vector<std::string> longs = {
      "-12345678901234567890123456789012345678901234567890.12345678901234567890123456789012345678901234567890e-17",
      "+.00000000000000000000000000000000000000000000000000000000000000000000000123456789e+60",
      "99999999999999999999999999999999999999.99999999999999999999999999999999999999999999E0",
      "000000000000000000000000000000000000000000000000000000000000000000000000000000001.5e000000009"};
  const int types[5][2] = {{38, 0}, {38, 38}, {15, 2}, {5, 0}, {1, 1}};
  unsigned long long sum = 0;
  long parsed = 0;
  for (auto& t : longs)
    for (size_t k = 0; k <= t.size(); k++)
      for (auto& pt : types)
        for (int map = 0; map < 3; map++) {
          gdv_int128 v = 0;
          if (parse(t.substr(0, k), pt[0], pt[1], map, &v)) { sum += (unsigned long long)v; parsed++; }
        }
  // a pseudo-random walk over the bytes the grammar knows and a few it does not
  const char palette[] = "0123456789+-.eE ,x";
  unsigned long long state = 88172645463325252ull;
  for (int r = 0; r < 20000; r++) {
    std::string t;
    state ^= state << 13; state ^= state >> 7; state ^= state << 17;
    const int len = (int)(state % 24);
    for (int k = 0; k < len; k++) {
      state ^= state << 13; state ^= state >> 7; state ^= state << 17;
      t.push_back(palette[(state >> 11) % (sizeof(palette) - 1)]);
    }
    gdv_int128 v = 0;
    if (parse(t, 38, (int)(state % 39), 0, &v)) { sum += (unsigned long long)v; parsed++; }
  }
  std::printf("parsed %ld texts, checksum %llu\n", parsed, sum);
  if (failures) { std::printf("decimal_parse_check: FAILED (%d)\n", failures); return 1; }
  std::printf("decimal_parse_check: ok\n");
  return 0;
}
