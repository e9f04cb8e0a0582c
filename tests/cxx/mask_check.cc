// Stand-alone program over the HOST build of the data-masking family (gdv_device_lib.hpp: gdv_mask, the position walks, the copy
// gdv_copy_masked), meant to be built with -fsanitize=address,undefined and run as a child process (tests/test_mask_cpu.py).
// Every text sits at the end of a heap block of exactly its length (views without GDV_STR_INBUF) or its length + 7 (views that
// claim it: the most an 8-byte load that starts inside the view may reach), every result in a block of exactly the text's
// length: a read or a write one byte too far is a heap-buffer-overflow.  Results are compared with a byte-at-a-time
// restatement of the rules.  Prints "mask_check: ok".
#include <climits>
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
static long rows = 0;

// the rules, one byte at a time: character index of every byte, then the class of the bytes whose character is masked
static std::string restate(const std::string& text, int mode, int n, int map, const char* reps) {
  long c = 0;
  for (unsigned char b : text) c += (b & 0xC0) != 0x80;
  const long k = n < 0 ? 0 : (n > c ? c : n);
  long c0 = 0, c1 = c;
  if (mode == 1) c1 = k;
  if (mode == 2) c0 = c - k;
  if (mode == 3) c0 = k;
  if (mode == 4) c1 = c - k;
  std::string out = text;
  long ci = -1;
  for (size_t i = 0; i < text.size(); i++) {
    unsigned char b = (unsigned char)text[i];
    if ((b & 0xC0) != 0x80) ci++;
    if (map == 1 && b >= 'a' && b <= 'z') b -= 32;
    if (map == 2 && b >= 'A' && b <= 'Z') b += 32;
    if (ci >= c0 && ci < c1) {
      if (b >= 'A' && b <= 'Z') b = (unsigned char)reps[0];
      else if (b >= 'a' && b <= 'z') b = (unsigned char)reps[1];
      else if (b >= '0' && b <= '9') b = (unsigned char)reps[2];
    }
    out[i] = (char)b;
  }
  return out;
}

static void run(const std::string& text, int mode, int n, bool inbuf, int map, const char* reps = "Xxn") {
  const size_t len = text.size(), pad = inbuf ? 7 : 0;
  unsigned char* block = static_cast<unsigned char*>(std::malloc(len + pad ? len + pad : 1));
  if (len) std::memcpy(block, text.data(), len);
  if (pad) std::memcpy(block + len, "Zz9AbC0", pad);  // (what lies behind the text must not matter)
  gdv_str s = gdv_make_str(block, 0, static_cast<gdv_int32>(len), block + len + pad, inbuf ? GDV_STR_INBUF : 0);
  s.map = map;
  const gdv_uint32 packed = (unsigned char)reps[0] | ((unsigned char)reps[1] << 8) | ((unsigned char)reps[2] << 16);
  const gdv_str r = gdv_mask(s, mode, n, packed);
  std::string got;
  if ((size_t)r.len != len || !(r.map & GDV_MAP_MASK)) { std::printf("FAIL: length %d of %zu\n", r.len, len); failures++; }
  if (r.len > 0) {
    unsigned char* dst = static_cast<unsigned char*>(std::malloc(r.len));
    std::memset(dst, 0xEE, r.len);
    gdv_copy_masked(dst, r);
    got.assign(reinterpret_cast<const char*>(dst), r.len);
    std::free(dst);
  }
  std::free(block);
  rows++;
  if (got != restate(text, mode, n, map, reps)) {
    std::printf("FAIL: mode %d n %d inbuf %d map %d row of %zu bytes\n", mode, n, (int)inbuf, map, len);
    failures++;
  }
}

static void expect(const std::string& text, int mode, int n, const std::string& want, const char* reps = "Xxn") {
  if (restate(text, mode, n, 0, reps) != want) { std::printf("FAIL: the restatement on '%s'\n", text.c_str()); failures++; }
  for (int inbuf = 0; inbuf < 2; inbuf++) run(text, mode, n, inbuf != 0, 0, reps);
}

static std::string fill(size_t n) {
  static const char cyc[] = "aB3-Zz09 Qx";
  std::string s;
  for (size_t i = 0; i < n; i++) s.push_back(cyc[i % (sizeof(cyc) - 1)]);
  return s;
}

int main() {
  expect("H\xc3\xa9llo 42", 0, 0, "X\xc3\xa9xxx nn");
  expect("Ab1", 0, 0, "Ul#", "Ul#");
  expect("Hello-123", 1, 4, "Xxxxo-123");
  expect("Hello-123", 2, 4, "Hello-nnn");
  expect("Hello-123", 3, 2, "Hexxx-nnn");
  expect("Hello-123", 4, 2, "Xxxxx-n23");
  expect("\xc3\xa9" "A", 1, 1, "\xc3\xa9" "A");
  expect("\xc3\xa9" "A", 1, 2, "\xc3\xa9" "X");
  expect("", 0, 0, "");

  const size_t lengths[] = {0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 257, 4101};
  const char* chars[] = {"\xc3\xa9", "\xe2\x82\xac", "\xf0\x90\x90\xa8"};
  std::vector<std::string> texts;
  for (size_t L : lengths) {
    texts.push_back(fill(L));
    texts.push_back(std::string(L, '\x80'));  // continuation bytes only
    if (L >= 1) texts.push_back(fill(L - 1) + "\xc3");  // ends in a cut character
    if (L >= 2) texts.push_back(fill(L - 2) + "\xe2\x82");
    for (const char* ch : chars) {
      const size_t cl = std::strlen(ch);
      if (L < cl) continue;
      std::string t = fill(L);  // the character across every 8-byte boundary it fits on
      for (size_t b = 8; b < L; b += 8)
        if (b - 1 + cl <= L) t.replace(b - 1, cl, ch);
      texts.push_back(t);
      texts.push_back(std::string(ch) + fill(L - cl));
      texts.push_back(fill(L - cl) + ch);
    }
  }
  for (auto& t : texts) {
    long c = 0;
    for (unsigned char b : t) c += (b & 0xC0) != 0x80;
    const long ns[] = {INT_MIN, -1, 0, 1, 7, 8, 9, c - 1, c, c + 1, INT_MAX};
    for (int inbuf = 0; inbuf < 2; inbuf++)
      for (int map = 0; map < 3; map++) {
        run(t, 0, 0, inbuf != 0, map);
        for (int mode = 1; mode <= 4; mode++)
          for (long n : ns) run(t, mode, (int)n, inbuf != 0, map);
      }
  }
  // a pseudo-random walk over bytes of every class
  const unsigned char palette[] = {'a', 'Z', '0', '9', 'A', 'z', ' ', '@', '[', '`', '{', '/', ':', 0x80, 0xBF, 0xC3, 0xE2, 0xF0, 0xFF, 0x7F, 0x00};
  unsigned long long state = 88172645463325252ull;
  for (int r = 0; r < 40000; r++) {
    std::string t;
    state ^= state << 13; state ^= state >> 7; state ^= state << 17;
    const int len = (int)(state % 41);
    for (int k = 0; k < len; k++) {
      state ^= state << 13; state ^= state >> 7; state ^= state << 17;
      t.push_back((char)palette[(state >> 11) % sizeof(palette)]);
    }
    state ^= state << 13; state ^= state >> 7; state ^= state << 17;
    run(t, r % 5, (int)((state >> 20) % 45) - 2, (r & 8) != 0, (r >> 4) % 3, "#l*");
  }
  std::printf("%ld rows\n", rows);
  if (failures) { std::printf("mask_check: FAILED (%d)\n", failures); return 1; }
  std::printf("mask_check: ok\n");
  return 0;
}
