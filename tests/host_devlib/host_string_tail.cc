// Test-only HOST build of the string-tail functions of the device library (split_part, substring_index, repeat,
// space, translate) and of the copy entry that plans holding a translate() use (gdv_str_copy_ext).  Built and driven
// by tests/test_string_tail_cpu.py the way test_device_lib_on_host.py drives host_devlib.cc.
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
struct Col { const int* off; const unsigned char* data; long size; };
// a row of a column whose data buffer is readable 16 bytes past `size` (so GDV_STR_INBUF may be claimed)
gdv_str row(const Col& c, long i, int flags) {
  const gdv_uint8* lim = c.data + c.size + 16;
  return gdv_make_str(c.data, c.off[i], c.off[i + 1], lim, flags);
}
gdv_str case_map(gdv_str s, int map) {
  if (map == 1) return upper_utf8(s);
  if (map == 2) return lower_utf8(s);
  return s;
}
}  // namespace

extern "C" {

// fn: 0 split_part, 1 substring_index (text, delimiter, k[i]); 2 repeat (text, k[i]); 3 space (k[i]); 4 translate (text,
// `table` laid out as the planner lays it out).  The delimiter is the literal `lit` when `off1` is null, else row i of the
// second column (read through `dmap`).  `text_map`: the text read through upper (1) / lower (2).  `inbuf`: claim
// GDV_STR_INBUF for text rows and the literal (word-at-a-time search); `ascii`: claim GDV_STR_ASCII for text rows (only
// for all-ASCII buffers).  Every value is materialised with gdv_str_copy_ext; err_rows[i] = the row's error bits.
// Returns the bytes written.
long host_string_tail(int fn, const int* off0, const unsigned char* d0, long s0, const int* off1, const unsigned char* d1,
                      long s1, const unsigned char* lit, int litlen, const int* k, const unsigned char* table, long n,
                      int text_map, int dmap, int inbuf, int ascii, int* out_off, unsigned char* out_data,
                      unsigned char* err_rows) {
  const Col c0{off0, d0, s0}, c1{off1, d1, s1};
  const int tflags = (inbuf ? GDV_STR_INBUF : 0) | (ascii ? GDV_STR_ASCII : 0);
  long at = 0;
  out_off[0] = 0;
  for (long i = 0; i < n; i++) {
    unsigned err = 0;
    gdv_ctx ctx{&err};
    const gdv_str s = case_map(row(c0, i, tflags), text_map);
    gdv_str d = off1 != nullptr ? case_map(row(c1, i, inbuf ? GDV_STR_INBUF : 0), dmap)
                                : gdv_make_str(lit, 0, litlen, lit + litlen + 8, inbuf ? GDV_STR_INBUF : 0);
    gdv_str r;
    switch (fn) {
      case 0: r = split_part_utf8_utf8_int32(ctx, s, d, k[i]); break;
      case 1: r = substring_index_utf8_utf8_int32(ctx, s, d, k[i]); break;
      case 2: r = repeat_utf8_int32(ctx, s, k[i]); break;
      case 3: r = space_int32(ctx, k[i]); break;
      default: r = gdv_translate(ctx, s, table); break;
    }
    err_rows[i] = (unsigned char)err;
    if (r.len > 0) gdv_str_copy_ext(out_data + at, r);
    at += r.len;
    out_off[i + 1] = (int)at;
  }
  return at;
}

// space(int64): the lengths only (huge counts are errors, never materialised here)
void host_space64(const long long* k, long n, int* out_len, unsigned char* err_rows) {
  for (long i = 0; i < n; i++) {
    unsigned err = 0;
    gdv_ctx ctx{&err};
    out_len[i] = space_int64(ctx, k[i]).len;
    err_rows[i] = (unsigned char)err;
  }
}

}  // extern "C"
