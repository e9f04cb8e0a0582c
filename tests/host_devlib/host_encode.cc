// Test-only HOST build of the hex / unhex / base64 / unbase64 / crc32 functions of the device library and of the copy entry
// that plans holding such a value use (gdv_str_copy_enc).  Built and driven by tests/test_encode_cpu.py the way
// test_temporal_text_cpu.py drives host_temporal_text.cc.
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
// row i of (off, data) as the kernels see it: the buffer is readable 16 bytes past `size`, so GDV_STR_INBUF may be claimed
// (`inbuf`); `text_map`: the text read through upper (1) / lower (2)
gdv_str row_view(const int* off, const unsigned char* data, long size, long i, int inbuf, int text_map) {
  gdv_str s = gdv_make_str(data, off[i], off[i + 1], data + size + 16, inbuf ? GDV_STR_INBUF : 0);
  if (text_map == 1) s = upper_utf8(s);
  if (text_map == 2) s = lower_utf8(s);
  return s;
}
}  // namespace

extern "C" {

// fn: 0 hex, 1 unhex, 2 base64, 3 unbase64 over the rows of (off, data); valid[i] == 0: a null row (the function is not
// called, as in a plan; its length is 0).  Every value is materialised with gdv_str_copy_enc into out_data at
// `shift` + the running offset; err_rows[i] = the row's error bits after the function AND its copy.  Returns the bytes written.
long host_encode(int fn, const int* off, const unsigned char* data, long size, const unsigned char* valid, long n, int inbuf,
                 int text_map, int shift, int* out_off, unsigned char* out_data, unsigned char* err_rows) {
  long at = 0;
  out_off[0] = 0;
  for (long i = 0; i < n; i++) {
    unsigned err = 0;
    gdv_ctx ctx{&err};
    gdv_str r = gdv_empty_str();
    if (valid[i]) {
      const gdv_str s = row_view(off, data, size, i, inbuf, text_map);
      r = fn == 0 ? hex_utf8(ctx, s) : fn == 1 ? unhex_utf8(ctx, s) : fn == 2 ? base64_binary(ctx, s) : unbase64_utf8(ctx, s);
    }
    if (r.len > 0) gdv_str_copy_enc(out_data + shift + at, r);
    err_rows[i] = (unsigned char)err;
    at += r.len;
    out_off[i + 1] = (int)at;
  }
  return at;
}

// the length functions alone (what a pre-pass runs): lens[i] = the result's length, err_rows[i] the bits they raise
void host_encode_len(int fn, const int* off, const unsigned char* data, long size, long n, int* lens, unsigned char* err_rows) {
  for (long i = 0; i < n; i++) {
    unsigned err = 0;
    gdv_ctx ctx{&err};
    const gdv_str s = row_view(off, data, size, i, 1, 0);
    lens[i] = (fn == 0 ? hex_binary(ctx, s) : fn == 1 ? unhex_utf8(ctx, s) : fn == 2 ? base64_utf8(ctx, s) : unbase64_utf8(ctx, s)).len;
    err_rows[i] = (unsigned char)err;
  }
}

// hex(int32) (bits 32: v[i] is narrowed) / hex(int64), materialised as above
long host_hex_int(int bits, const long long* v, long n, int shift, int* out_off, unsigned char* out_data) {
  long at = 0;
  out_off[0] = 0;
  unsigned err = 0;
  gdv_ctx ctx{&err};
  for (long i = 0; i < n; i++) {
    const gdv_str r = bits == 32 ? hex_int32(ctx, (gdv_int32)v[i]) : hex_int64(ctx, v[i]);
    gdv_str_copy_enc(out_data + shift + at, r);
    at += r.len;
    out_off[i + 1] = (int)at;
  }
  return at;
}

void host_crc32(const int* off, const unsigned char* data, long size, long n, int inbuf, int text_map, long long* out) {
  for (long i = 0; i < n; i++) out[i] = crc32_utf8(row_view(off, data, size, i, inbuf, text_map));
}

// a value that is no encode value goes through gdv_str_copy_enc as through gdv_str_copy
void host_plain_copy(const unsigned char* data, int len, int text_map, unsigned char* out) {
  gdv_str s = gdv_make_str(data, 0, len, data + len + 16, GDV_STR_INBUF);
  if (text_map == 1) s = upper_utf8(s);
  if (len > 0) gdv_str_copy_enc(out, s);
}

}  // extern "C"
