// Test-only HOST build of regexp_extract's device function (gdv_regex_extract).  Built and driven by
// tests/test_regexp_extract_cpu.py the way test_string_tail_cpu.py drives host_string_tail.cc.
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

extern "C" {

// Row i of the column (offsets `off`, bytes `data`, readable 16 bytes past `size`), read through upper (text_map 1) / lower
// (2), against `table` (what gdv_compile_regex_extract lays out): out_from[i] / out_len[i] = where the result lies in the
// row (from = 0 for an empty result).  Returns the number of rows whose view left its row (0 is the only right answer).
long host_regexp_extract(const int* off, const unsigned char* data, long size, const unsigned char* table, long n, int text_map,
                         int* out_from, int* out_len) {
  long outside = 0;
  for (long i = 0; i < n; i++) {
    gdv_str s = gdv_make_str(data, off[i], off[i + 1], data + size + 16, 0);
    if (text_map == 1) s = upper_utf8(s);
    if (text_map == 2) s = lower_utf8(s);
    const gdv_str r = gdv_regex_extract(s, table);
    const long from = r.p - (data + off[i]);
    out_len[i] = r.len;
    out_from[i] = r.len > 0 ? (int)from : 0;
    if (r.len < 0 || (r.len > 0 && (from < 0 || from + r.len > off[i + 1] - off[i]))) outside++;
  }
  return outside;
}

}  // extern "C"
