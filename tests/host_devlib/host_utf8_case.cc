// Test-only HOST build of upper / lower under GDV_UTF8_CASE=1 (gdv_device_lib.hpp: gdv_utf8_case, gdv_utf8_case_lookup,
// gdv_copy_utf8_case) over the committed table (gdv_utf8_case_table.inc).  Built and driven by tests/test_utf8_case_cpu.py the
// way test_string_tail_cpu.py drives host_string_tail.cc.
#include <cmath>
#include <cstdint>
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

#include "../../gandiva_amd/csrc/gdv_device_lib.hpp"
#include "../../gandiva_amd/csrc/gdv_utf8_case_table.inc"

extern "C" {

// dir: 1 upper, 2 lower.  Rows of a column whose data buffer is readable 16 bytes past `size` (so `inbuf` may claim
// GDV_STR_INBUF: the word-at-a-time paths); `text_map`: the view carries the ASCII upper (1) / lower (2) byte map.  A row with
// valid[i] == 0 is not evaluated (as the kernel's guard does).  Every value is copied twice, over 0x00 and over 0xFF: a byte
// that differs afterwards was not written.  written_ok[i] = exactly the bytes [0, reported length) were written, the 16
// behind them included in the check.  err_rows[i] = the row's error bits.  Returns the bytes of the output.
long host_utf8_case(int dir, const int* off, const unsigned char* data, long size, const unsigned char* valid, long n, int text_map,
                    int inbuf, int* out_off, unsigned char* out_data, unsigned char* err_rows, unsigned char* written_ok) {
  const unsigned char* tab = dir == 1 ? gdv_utf8_upper_table : gdv_utf8_lower_table;
  long at = 0;
  out_off[0] = 0;
  std::vector<unsigned char> a, b;
  for (long i = 0; i < n; i++) {
    unsigned err = 0;
    gdv_ctx ctx{&err};
    gdv_str s = gdv_make_str(data, off[i], off[i + 1], data + size + 16, inbuf ? GDV_STR_INBUF : 0);
    if (text_map == 1) s = upper_utf8(s);
    if (text_map == 2) s = lower_utf8(s);
    const gdv_str r = valid[i] ? gdv_utf8_case(ctx, s, tab) : gdv_empty_str();
    err_rows[i] = (unsigned char)err;
    bool ok = true;
    if (r.len > 0) {
      a.assign(r.len + 16, 0x00);
      b.assign(r.len + 16, 0xFF);
      gdv_copy_utf8_case(a.data(), r);
      gdv_copy_utf8_case(b.data(), r);
      for (int j = 0; j < r.len; j++) ok = ok && a[j] == b[j];
      for (int j = r.len; j < r.len + 16; j++) ok = ok && a[j] == 0x00 && b[j] == 0xFF;
      std::memcpy(out_data + at, a.data(), r.len);
    }
    written_ok[i] = ok ? 1 : 0;
    at += r.len;
    out_off[i + 1] = (int)at;
  }
  return at;
}

// the table's answer for one code point (the code point itself when the map leaves it alone)
unsigned host_utf8_case_lookup(int dir, unsigned cp) {
  return gdv_utf8_case_lookup(dir == 1 ? gdv_utf8_upper_table : gdv_utf8_lower_table, cp);
}

long host_utf8_case_table_bytes(int dir) { return dir == 1 ? sizeof(gdv_utf8_upper_table) : sizeof(gdv_utf8_lower_table); }

}  // extern "C"
