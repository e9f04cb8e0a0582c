// Test-only HOST build of the text <-> date / time functions of the device library (castDATE / castTIMESTAMP / castTIME
// of text, castVARCHAR of date32 / date64 / timestamp / time32, castTIME(timestamp), castTIMESTAMP(date32)) and of the
// copy entry that plans holding such a castVARCHAR use (gdv_str_copy_dt).  Built and driven by
// tests/test_temporal_text_cpu.py the way test_string_tail_cpu.py drives host_string_tail.cc.
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

// fn: 0 castDATE, 1 castTIMESTAMP, 2 castTIME over the rows of (off, data); the data buffer is readable 16 bytes past
// `size`, so GDV_STR_INBUF may be claimed (`inbuf`: the word-at-a-time fast path applies).  `text_map`: the text read
// through upper (1) / lower (2).  out[i] = the value (date64 / timestamp milliseconds, time32 widened), err_rows[i] = the
// row's error bits.
void host_temporal_parse(int fn, const int* off, const unsigned char* data, long size, long n, int inbuf, int text_map,
                         long long* out, unsigned char* err_rows) {
  const gdv_uint8* lim = data + size + 16;
  for (long i = 0; i < n; i++) {
    unsigned err = 0;
    gdv_ctx ctx{&err};
    gdv_str s = gdv_make_str(data, off[i], off[i + 1], lim, inbuf ? GDV_STR_INBUF : 0);
    if (text_map == 1) s = upper_utf8(s);
    if (text_map == 2) s = lower_utf8(s);
    out[i] = fn == 0 ? castDATE_utf8(ctx, s) : fn == 1 ? castTIMESTAMP_utf8(ctx, s) : (long long)castTIME_utf8(ctx, s);
    err_rows[i] = (unsigned char)err;
  }
}

// kind: 0 castVARCHAR(timestamp), 1 (date64), 2 (date32: v[i] days), 3 (time32: v[i] milliseconds) with n = k[i]; every
// value is materialised with gdv_str_copy_dt into out_data at the running offset.  Returns the bytes written.
long host_temporal_format(int kind, const long long* v, const long long* k, long n, int* out_off, unsigned char* out_data,
                          unsigned char* err_rows) {
  long at = 0;
  out_off[0] = 0;
  for (long i = 0; i < n; i++) {
    unsigned err = 0;
    gdv_ctx ctx{&err};
    gdv_str r;
    switch (kind) {
      case 0: r = castVARCHAR_timestamp_int64(ctx, v[i], k[i]); break;
      case 1: r = castVARCHAR_date64_int64(ctx, v[i], k[i]); break;
      case 2: r = castVARCHAR_date32_int64(ctx, (gdv_date32)v[i], k[i]); break;
      default: r = castVARCHAR_time32_int64(ctx, (gdv_time32)v[i], k[i]); break;
    }
    err_rows[i] = (unsigned char)err;
    if (r.len > 0) gdv_str_copy_dt(out_data + at, r);
    at += r.len;
    out_off[i + 1] = (int)at;
  }
  return at;
}

// castTIME(timestamp) (fn 0) and castTIMESTAMP(date32) (fn 1)
void host_temporal_fixed(int fn, const long long* v, long n, long long* out) {
  for (long i = 0; i < n; i++) out[i] = fn == 0 ? (long long)castTIME_timestamp(v[i]) : castTIMESTAMP_date32((gdv_date32)v[i]);
}

}  // extern "C"
