// Stand-alone program over the HOST build of upper / lower under GDV_UTF8_CASE=1 (gdv_device_lib.hpp: the walker gdv_utf8_case,
// the lookup, the copy gdv_copy_utf8_case; the committed table), meant to be built with -fsanitize=address,undefined and run as
// a child process (tests/test_utf8_case_cpu.py).  Every text sits in a heap block of exactly its length (views without
// GDV_STR_INBUF) or its length + 8 (views that claim it: 8-byte loads that start inside the view), every result in a block of
// exactly the reported length: a read or a write one byte too far is a heap-buffer-overflow.  Prints "utf8_case_check: ok".
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
#include "gdv_utf8_case_table.inc"

static int failures = 0;

// upper (dir 1) / lower (dir 2) of `text` through a view with / without GDV_STR_INBUF and the ASCII byte map `map`; false
// when the row raises
static bool run(const std::string& text, int dir, bool inbuf, int map, std::string* out) {
  const size_t n = text.size(), pad = inbuf ? 8 : 0;
  unsigned char* block = static_cast<unsigned char*>(std::malloc(n + pad ? n + pad : 1));
  if (n) std::memcpy(block, text.data(), n);
  if (pad) std::memset(block + n, 0xC3, pad);  // (what lies behind the text must not matter: a lead byte)
  gdv_str s = gdv_make_str(block, 0, static_cast<gdv_int32>(n), block + n + pad, inbuf ? GDV_STR_INBUF : 0);
  s.map = map;
  unsigned err = 0;
  gdv_ctx ctx{&err};
  const gdv_str r = gdv_utf8_case(ctx, s, dir == 1 ? gdv_utf8_upper_table : gdv_utf8_lower_table);
  out->clear();
  if (err == 0 && r.len > 0) {
    unsigned char* dst = static_cast<unsigned char*>(std::malloc(r.len));
    std::memset(dst, 0xEE, r.len);
    gdv_copy_utf8_case(dst, r);
    out->assign(reinterpret_cast<const char*>(dst), r.len);
    std::free(dst);
  }
  std::free(block);
  if (err != 0 && err != GDV_ERR_BAD_ARG) { std::printf("FAIL: error bits %u\n", err); failures++; }
  return err == 0;
}

static std::string encode(unsigned cp) {
  std::string s;
  if (cp < 0x80) s.push_back((char)cp);
  else if (cp < 0x800) { s.push_back((char)(0xC0 | (cp >> 6))); s.push_back((char)(0x80 | (cp & 0x3F))); }
  else if (cp < 0x10000) { s.push_back((char)(0xE0 | (cp >> 12))); s.push_back((char)(0x80 | ((cp >> 6) & 0x3F))); s.push_back((char)(0x80 | (cp & 0x3F))); }
  else { s.push_back((char)(0xF0 | (cp >> 18))); s.push_back((char)(0x80 | ((cp >> 12) & 0x3F))); s.push_back((char)(0x80 | ((cp >> 6) & 0x3F))); s.push_back((char)(0x80 | (cp & 0x3F))); }
  return s;
}

static void expect(const std::string& text, int dir, bool ok, const std::string& want) {
  for (int inbuf = 0; inbuf < 2; inbuf++) {
    std::string got;
    const bool taken = run(text, dir, inbuf != 0, 0, &got);
    if (taken != ok || (ok && got != want)) {
      std::printf("FAIL: dir %d inbuf %d '%s': taken %d '%s', want taken %d '%s'\n", dir, inbuf, text.c_str(), (int)taken, got.c_str(), (int)ok,
                  want.c_str());
      failures++;
    }
  }
}

int main() {
  expect("", 1, true, "");
  expect("h\xc3\xa9llo", 1, true, "H\xc3\x89LLO");
  expect("H\xc3\x89LLO wOrld", 2, true, "h\xc3\xa9llo world");
  expect("\xc3\x9f", 1, true, "\xe1\xba\x9e");              // ß -> U+1E9E
  expect("\xc4\xb1\xc5\xbf", 1, true, "IS");                 // dotless i, long s
  expect("\xc9\x90", 1, true, "\xe2\xb1\xaf");               // U+0250 -> U+2C6F
  expect("\xe2\x84\xaa", 2, true, "k");                      // Kelvin sign
  expect("\xf0\x90\x90\xa8", 1, true, "\xf0\x90\x90\x80");   // U+10428 -> U+10400
  expect("\xf0\x9e\xa4\x80", 2, true, "\xf0\x9e\xa4\xa2");   // U+1E900 -> U+1E922
  expect("a\x80", 1, false, "");
  expect("\xc3", 1, false, "");
  expect("abcdefg\xe2\x82", 2, false, "");
  expect("\xf8\x88\x80\x80\x80", 1, false, "");
  expect("a\xc0\xaf" "b", 1, true, "A\xc0\xaf" "B");         // an over-long form: copied
  expect("\xed\xa0\x80", 2, true, "\xed\xa0\x80");           // a surrogate: copied
  expect("\xc1\xa1", 1, true, "\xc1\xa1");                   // over-long 'a' is not 'a'
  expect("\xf4\x90\x80\x80", 1, true, "\xf4\x90\x80\x80");   // above U+10FFFF: copied

  // every code point, one per row and in rows of 16, both directions, both kinds of view; the maps are idempotent and a
  // mapped code point is one code point
  unsigned long long sum = 0;
  long changed[3] = {0, 0, 0};
  for (int dir = 1; dir <= 2; dir++) {
    std::string row, want_row;
    for (unsigned cp = 0; cp < 0x110000; cp++) {
      if (cp >= 0xD800 && cp <= 0xDFFF) continue;
      const std::string text = encode(cp);
      std::string got, again, got_raw;
      if (!run(text, dir, true, 0, &got) || !run(text, dir, false, 0, &got_raw) || got != got_raw) { std::printf("FAIL: U+%04X dir %d\n", cp, dir); failures++; continue; }
      if (got != text) changed[dir]++;
      if (!run(got, dir, true, 0, &again) || again != got) { std::printf("FAIL: U+%04X dir %d is not idempotent\n", cp, dir); failures++; }
      const unsigned to = gdv_utf8_case_lookup(dir == 1 ? gdv_utf8_upper_table : gdv_utf8_lower_table, cp);
      if (cp >= 0x80 && got != encode(to)) { std::printf("FAIL: U+%04X dir %d: copy and lookup disagree\n", cp, dir); failures++; }
      sum += to;
      row += text;
      want_row += got;
      if (cp % 16 == 15) {
        std::string got_row;
        for (int inbuf = 0; inbuf < 2; inbuf++)
          if (!run(row, dir, inbuf != 0, 0, &got_row) || got_row != want_row) { std::printf("FAIL: row ending at U+%04X dir %d inbuf %d\n", cp, dir, inbuf); failures++; }
        row.clear();
        want_row.clear();
      }
    }
  }
  // (ASCII letters are part of the count here: 1480 + 26 and 1462 + 26)
  if (changed[1] != 1506 || changed[2] != 1488) { std::printf("FAIL: %ld / %ld code points change\n", changed[1], changed[2]); failures++; }

  // every prefix of mixed texts (a prefix that cuts a character raises), through each ASCII byte map
  const std::vector<std::string> mixed = {
      "Stra\xc3\x9f" "e \xc4\xb1\xc5\xbf \xc9\x90\xc4\xb0\xc8\xba \xe2\x84\xaa\xe2\x84\xa6\xe1\xba\x9e \xf0\x90\x90\xa8\xf0\x9e\xa4\xa2 end of the Text",
      "abcdefgh\xc3\xa9" "ABCDEFG\xc3\x89" "abcdef\xe2\x84\xaaxyzXYZ0123456789\xf0\x90\x90\x80"};
  long rows = 0;
  for (auto& t : mixed)
    for (size_t k = 0; k <= t.size(); k++)
      for (int dir = 1; dir <= 2; dir++)
        for (int map = 0; map < 3; map++)
          for (int inbuf = 0; inbuf < 2; inbuf++) {
            std::string got;
            const bool cut = k < t.size() && ((unsigned char)t[k] & 0xC0) == 0x80;
            if (run(t.substr(0, k), dir, inbuf != 0, map, &got) == cut) { std::printf("FAIL: prefix %zu\n", k); failures++; }
            rows++;
          }
  // a pseudo-random walk over bytes of every class: most rows raise, none reads or writes out of bounds
  const unsigned char palette[] = {'a', 'Z', '0', ' ', 0x80, 0xBF, 0xC0, 0xC3, 0xC4, 0xC9, 0xDF, 0xE0, 0xE1, 0xE2, 0xED, 0xEF, 0xF0, 0xF4, 0xF8, 0xFF,
                                   0x90, 0xA8, 0xB1, 0x9F, 0x84, 0xAA};
  unsigned long long state = 88172645463325252ull;
  for (int r = 0; r < 40000; r++) {
    std::string t;
    state ^= state << 13; state ^= state >> 7; state ^= state << 17;
    const int len = (int)(state % 28);
    for (int k = 0; k < len; k++) {
      state ^= state << 13; state ^= state >> 7; state ^= state << 17;
      t.push_back((char)palette[(state >> 11) % sizeof(palette)]);
    }
    std::string got;
    if (run(t, 1 + (r & 1), (r & 2) != 0, (r >> 2) % 3, &got)) sum += got.size();
    rows++;
  }
  std::printf("%ld further rows, checksum %llu\n", rows, sum);
  if (failures) { std::printf("utf8_case_check: FAILED (%d)\n", failures); return 1; }
  std::printf("utf8_case_check: ok\n");
  return 0;
}
