// Test-only HOST build of the calendar tail of the device library (gandiva_amd/csrc/gdv_device_lib.hpp): months_between,
// next_day, add_months, and the functions that date_trunc('unit', t) and the extractor names year, month, day ... resolve
// to.  Built and driven by tests/test_calendar_tail_cpu.py.  One entry point calls a device function by its symbol over
// dense columns; the dispatch expands from gdv_tier0_fns.inc, the list the tier-0 interpreter's call switch expands from,
// so a symbol listed there and missing here does not compile.
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

typedef gdv_int32 T_I32;
typedef gdv_int64 T_I64;
typedef gdv_float32 T_F32;
typedef gdv_float64 T_F64;

extern "C" {

// out[i] = symbol(a[i]) or symbol(a[i], b[i]); columns are dense arrays of the C types of the symbol's signature
// (date32 / time32 as int32, date64 / timestamp as int64).  Returns 0, or -1 where gdv_tier0_fns.inc has no such symbol.
int host_call(const char* symbol, const void* a, const void* b, void* out, long n) {
#define GDV_T0_F1(sym, R, A)                                                                  \
  if (!std::strcmp(symbol, #sym)) {                                                           \
    for (long i = 0; i < n; i++) ((T_##R*)out)[i] = sym(((const T_##A*)a)[i]);                \
    return 0;                                                                                 \
  }
#define GDV_T0_F2(sym, R, A, B)                                                               \
  if (!std::strcmp(symbol, #sym)) {                                                           \
    for (long i = 0; i < n; i++) ((T_##R*)out)[i] = sym(((const T_##A*)a)[i], ((const T_##B*)b)[i]); \
    return 0;                                                                                 \
  }
#include "../../gandiva_amd/csrc/gdv_tier0_fns.inc"
#undef GDV_T0_F1
#undef GDV_T0_F2
  return -1;
}

}  // extern "C"
