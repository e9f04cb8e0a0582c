// Test-only HOST build of the data-masking family (gdv_device_lib.hpp: gdv_mask, gdv_copy_masked and the two position walks).
// Built and driven by tests/test_mask_cpu.py the way test_string_tail_cpu.py drives host_string_tail.cc.
#include <cmath>
#include <cstdint>
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

#include "../../gandiva_amd/csrc/gdv_device_lib.hpp"

extern "C" {

// mode: 0 mask, 1 mask_first_n, 2 mask_last_n, 3 mask_show_first_n, 4 mask_show_last_n; ns[i]: row i's n; reps: upper | lower
// << 8 | digit << 16.  Every row is first moved to the END of a heap block of its own: exactly its length for views without
// GDV_STR_INBUF (`inbuf` 0), its length + 7 bytes of ASCII letters and digits for views that claim it (the most an 8-byte load
// that starts inside the view may reach), so the row's last word load is the block's last.  `text_map`: the view carries the
// ASCII upper (1) / lower (2) byte map.  A row with valid[i] == 0 is not evaluated.  Every value is copied twice, over 0x00 and
// over 0xFF, into a block with 16 guard bytes on both sides.  Returns the number of bytes written OUTSIDE [dst, dst + len) over
// all rows; *unwritten = bytes inside that one of the copies left alone.  out_off / out_data: the column.
long host_mask(int mode, const int* ns, unsigned reps, const int* off, const unsigned char* data, const unsigned char* valid, long n,
               int text_map, int inbuf, int* out_off, unsigned char* out_data, long* unwritten) {
  long at = 0, outside = 0, missed = 0;
  out_off[0] = 0;
  std::vector<unsigned char> a, b;
  static const char pad[] = "Zz9AbC0";
  for (long i = 0; i < n; i++) {
    const int len = off[i + 1] - off[i], extra = inbuf ? 7 : 0;
    unsigned char* block = static_cast<unsigned char*>(std::malloc(len + extra ? len + extra : 1));
    if (len) std::memcpy(block, data + off[i], len);
    std::memcpy(block + len, pad, extra);
    gdv_str s = gdv_make_str(block, 0, len, block + len + extra, inbuf ? GDV_STR_INBUF : 0);
    if (text_map == 1) s = upper_utf8(s);
    if (text_map == 2) s = lower_utf8(s);
    const gdv_str r = valid[i] ? gdv_mask(s, mode, ns[i], reps) : gdv_empty_str();
    if (r.len > 0) {
      a.assign(r.len + 32, 0x00);
      b.assign(r.len + 32, 0xFF);
      GDV_COPY_MASK(a.data() + 16, r, missed += r.len);
      GDV_COPY_MASK(b.data() + 16, r, missed += r.len);
      for (int j = 0; j < r.len + 32; j++) {
        const bool inside = j >= 16 && j < 16 + r.len;
        if (inside) missed += a[j] != b[j];
        else outside += (a[j] != 0x00) + (b[j] != 0xFF);
      }
      std::memcpy(out_data + at, a.data() + 16, r.len);
    }
    std::free(block);
    at += r.len;
    out_off[i + 1] = (int)at;
  }
  *unwritten = missed;
  return outside;
}

}  // extern "C"
