// gandiva_amd device function library (gfx950 / CDNA4, wave64).
//
// This header is the fixed library the fused kernels are assembled from: it replaces the
// reference's `precompiled/*.cc` bitcode library and
// `BitMapAccumulator` / `bitmap.cc` helpers (rows 8, 13).  It is embedded verbatim in
// libgandiva_amd.so and handed to the runtime compiler together with the kernel body the
// planner emits for one Projector / Filter (gdv_planner.cc and its units).  Function names follow the
// reference's `<name>_<type>_<type>` convention so a plan dump reads like the
// reference's IR.  Everything is written for 64-wide wavefronts: one wavefront handles
// 64 consecutive rows per sub-tile, i.e. exactly one 64-bit Arrow validity word
// (LSB-first bit order: pyarrow/include/arrow/util/bit_util.h:173-175).
//
// Build flags that are part of the semantics: -ffp-contract=off (no FMA fusion: results
// must be bit-identical to separate IEEE mul + add), correctly rounded f32 divide/sqrt.
#pragma once

typedef signed char gdv_int8;
typedef short gdv_int16;
typedef int gdv_int32;
typedef long long gdv_int64;
typedef unsigned char gdv_uint8;
typedef unsigned short gdv_uint16;
typedef unsigned int gdv_uint32;
typedef unsigned long long gdv_uint64;
typedef float gdv_float32;
typedef double gdv_float64;
typedef __int128 gdv_int128;
typedef unsigned __int128 gdv_uint128;
typedef bool gdv_boolean;
typedef gdv_int32 gdv_date32;
typedef gdv_int64 gdv_date64;
typedef gdv_int64 gdv_timestamp;
typedef gdv_int32 gdv_time32;
typedef gdv_int64 gdv_time64;

#define GDV_DEV static __device__ __forceinline__
#define GDV_WAVE 64

// Error bits a kernel can raise (-> Status::ExecutionError on the host).
#define GDV_ERR_DIV_ZERO 1u
#define GDV_ERR_OVERFLOW 2u
#define GDV_ERR_BAD_ARG 4u

struct gdv_ctx {
  gdv_uint32* err;
};
// A bit is raised ONCE, not once per raiser: same-address read-modify-write atomics are served one
// after the other (~12 ns each, profiles/r02_k2_singlepass_proto.txt) — round 4 found the C5 kernels
// taking 2.3 ms instead of 1.0 on a batch where nearly every wave tile raised NOTASCII (195 000 atomicOr
// on one word).  A relaxed agent-scope load first (loads of one address are not serialised); the few
// raisers that read the word before the first atomic landed do the atomic, everyone after them does not.
#ifdef GDV_HOST_BUILD
GDV_DEV void gdv_raise_bits(gdv_uint32* err, gdv_uint32 bit) { *err |= bit; }
#else
GDV_DEV void gdv_raise_bits(gdv_uint32* err, gdv_uint32 bit) {
  typedef __attribute__((address_space(1))) gdv_uint32 gdv_gu32;
  if ((__hip_atomic_load((gdv_gu32*)err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) != bit) atomicOr(err, bit);
}
#endif
GDV_DEV void gdv_raise(gdv_ctx ctx, gdv_uint32 bit) { gdv_raise_bits(ctx.err, bit); }

// ------------------------------------------------------------------ memory access
//
// Values buffers are streamed exactly once: loads are plain coalesced loads (one row per
// lane -> 64*sizeof(T) contiguous bytes per wave instruction), stores are non-temporal
// so the written lines do not displace input lines in L2 / Infinity Cache.
template <typename T>
GDV_DEV T gdv_ld(const T* p, gdv_int64 i) { return p[i]; }
template <typename T>
GDV_DEV T gdv_ldnt(const T* p, gdv_int64 i) { return __builtin_nontemporal_load(p + i); }
template <typename T>
GDV_DEV void gdv_st(T* p, gdv_int64 i, T v) { p[i] = v; }
template <typename T>
GDV_DEV void gdv_stnt(T* p, gdv_int64 i, T v) { __builtin_nontemporal_store(v, p + i); }

// rows of a selection-mode launch whose slot count sits in device memory: never more than the
// capacity n the outputs and the grid were sized for, never negative
GDV_DEV gdv_int64 gdv_clamp_rows(gdv_int64 count, gdv_int64 n) { return count < 0 ? 0 : (count > n ? n : count); }
// A bitmap as the kernels see it: 8-byte aligned word pointer + a bit shift < 64 (Arrow
// array offsets and unaligned buffers are folded into these two by the host) + the
// number of words that may be read (>= 1).  A column without a validity buffer is bound to
// a one-word all-ones bitmap (nwords == 1): indices are clamped, never branched on, so
// the load phase of a tile contains no control flow and all loads issue back to back.
struct gdv_bitmap {
  const gdv_uint64* p;
  gdv_int32 shift;
  gdv_int64 nwords;
};

// The GDV_U validity words of one wave tile, fetched with ONE vector load: lane u
// (u < nsub) returns the 64 bits covering rows [64*(wbase+u), 64*(wbase+u)+64).  Words past
// the end of the buffer are clamped to the last word: they only cover rows >= n, which
// the caller masks with its live-row mask.
GDV_DEV gdv_uint64 gdv_bitmap_tile(const gdv_bitmap& bm, gdv_int64 wbase, int lane, int nsub) {
  // No exec masking: lanes >= nsub re-read word nsub-1 (same cache line, result unused),
  // so the two loads carry no control dependence and overlap with the value loads.
  const int l = lane < nsub ? lane : nsub - 1;
  const gdv_int64 last = bm.nwords - 1;
  gdv_int64 i0 = wbase + l;
  gdv_int64 i1 = i0 + 1;
  i0 = i0 < last ? i0 : last;
  i1 = i1 < last ? i1 : last;
  const gdv_uint64 lo = bm.p[i0];
  const gdv_uint64 hi = bm.p[i1];
  // funnel shift that is also correct for shift == 0 (no shift-by-64)
  return (lo >> bm.shift) | ((hi << 1) << (63 - bm.shift));
}

// Word `w` (wave-uniform index) of a bitmap, through the SCALAR data path: the input bitmaps are
// read-only for the kernel, so they are addressed as constant memory (address space 4) and the
// two 8-byte loads become one s_load — no VGPRs, no vmcnt slot, nothing the value loads of the
// tile have to queue behind (round 2: the vector-load + readlane form made the compiler wait for
// the bitmap words in the middle of the value loads: 7 of 32 loads in flight in the C3 kernel).
#ifdef GDV_HOST_BUILD
typedef const gdv_uint64 gdv_cu64;
#else
typedef const __attribute__((address_space(4))) gdv_uint64 gdv_cu64;
#endif
GDV_DEV gdv_uint64 gdv_bitmap_word(const gdv_bitmap& bm, gdv_int64 w) {
  const gdv_int64 last = bm.nwords - 1;
  const gdv_int64 i0 = w < last ? w : last;
  const gdv_int64 i1 = w + 1 < last ? w + 1 : last;
  gdv_cu64* q = (gdv_cu64*)bm.p;
  const gdv_uint64 lo = q[i0], hi = q[i1];
  return (lo >> bm.shift) | ((hi << 1) << (63 - bm.shift));  // also correct for shift == 0
}

// Word `u` of a tile fetched by gdv_bitmap_tile, as a wave-uniform value (SGPR pair):
// merging the validity of several columns is then s_and_b64, not per-lane work.
GDV_DEV gdv_uint64 gdv_tile_word(gdv_uint64 tile, int u) {
  gdv_uint32 lo = __builtin_amdgcn_readlane((gdv_uint32)tile, u);
  gdv_uint32 hi = __builtin_amdgcn_readlane((gdv_uint32)(tile >> 32), u);
  return ((gdv_uint64)hi << 32) | lo;
}

// Deposit the wave-uniform `word` into lane `u` of the accumulator: after GDV_U deposits
// lanes 0..GDV_U-1 hold the wave's output words and store them with one coalesced store.
// ---- wave-level prefix sum / sum of a 32-bit value (64 lanes), on the DPP data path:
// row_shr 1,2,3 + row_shr 4/8 with bank masks, then row_bcast 15 / 31 across the four rows
// (the classic GCN/CDNA scan; no LDS traffic, no cross-lane permute instructions).
template <int CTRL, int ROW_MASK, int BANK_MASK>
GDV_DEV gdv_int32 gdv_dpp_add(gdv_int32 acc, gdv_int32 src) {
  // lanes the masks disable, and lanes whose source falls outside the row, contribute 0
  return acc + __builtin_amdgcn_update_dpp(0, src, CTRL, ROW_MASK, BANK_MASK, false);
}
GDV_DEV gdv_int32 gdv_wave_scan_incl(gdv_int32 v) {
  gdv_int32 r = v;
  r = gdv_dpp_add<0x111, 0xf, 0xf>(r, v);  // row_shr:1
  r = gdv_dpp_add<0x112, 0xf, 0xf>(r, v);  // row_shr:2
  r = gdv_dpp_add<0x113, 0xf, 0xf>(r, v);  // row_shr:3
  r = gdv_dpp_add<0x114, 0xf, 0xe>(r, r);  // row_shr:4, banks 1-3
  r = gdv_dpp_add<0x118, 0xf, 0xc>(r, r);  // row_shr:8, banks 2-3
  r = gdv_dpp_add<0x142, 0xa, 0xf>(r, r);  // row_bcast:15 into rows 1 and 3
  r = gdv_dpp_add<0x143, 0xc, 0xf>(r, r);  // row_bcast:31 into rows 2 and 3
  return r;
}
GDV_DEV gdv_int32 gdv_wave_last(gdv_int32 v) { return __builtin_amdgcn_readlane(v, 63); }
// Byte totals of a wave tile must not wrap: a few very long strings (or a concat of them) can
// exceed 2^31 bytes inside one tile.  Lanes accumulate with saturation, the wave sum is taken
// on 16-bit halves, and a total of 2^31 or more is reported as exactly 2^31 — enough for the
// host's "var-len output exceeds 2 GiB" check, which then never launches the byte pass.
GDV_DEV gdv_int32 gdv_sat_add31(gdv_int32 a, gdv_int32 b) {
  const gdv_uint32 s = (gdv_uint32)a + (gdv_uint32)b;
  return s > 0x7fffffffu ? 0x7fffffff : (gdv_int32)s;
}
GDV_DEV gdv_uint32 gdv_tile_total(gdv_int32 lane_total) {  // lane_total in [0, 2^31)
  const gdv_uint64 lo = (gdv_uint32)__builtin_amdgcn_readlane(gdv_wave_scan_incl(lane_total & 0xffff), 63);
  const gdv_uint64 hi = (gdv_uint32)__builtin_amdgcn_readlane(gdv_wave_scan_incl(lane_total >> 16), 63);
  const gdv_uint64 t = lo + (hi << 16);
  return t >= 0x80000000ull ? 0x80000000u : (gdv_uint32)t;
}
GDV_DEV gdv_int32 gdv_wave_sum(gdv_int32 v) { return gdv_wave_last(gdv_wave_scan_incl(v)); }

// bitmap words of a tile leave with one store per wave tile
#define GDV_WORD_ST(p, v) (*(gdv_uint64*)(p) = (v))
#define GDV_WORD_ST_NT(p, v) __builtin_nontemporal_store((gdv_uint64)(v), (gdv_uint64*)(p))
GDV_DEV gdv_uint64 gdv_deposit_word(gdv_uint64 acc, int u, gdv_uint64 word, int lane) {
  return (lane == u) ? word : acc;  // v_cndmask with a scalar source
}

// Per-sub-tile register arrays inside a loop that is NOT unrolled: the current sub-tile's
// element is always index 0 and every array rotates left by one at the end of an iteration
// (static indices only: the arrays stay in registers; after GDV_U iterations they are back in
// their original order, and a value written at [0] in iteration u ends up at [u]).
#ifdef GDV_UNROLL_ROWS
#define GDV_ROW_LOOP _Pragma("unroll")
#elif defined(GDV_ROW_UNROLL2)
#define GDV_ROW_LOOP _Pragma("unroll 2")
#else
#define GDV_ROW_LOOP _Pragma("nounroll")
#endif
// 16 bytes to HBM (unaligned): plain, or non-temporal (experiment: -DGDV_NT_STRING_STORES)
typedef gdv_uint64 gdv_u64x2_t __attribute__((ext_vector_type(2)));
GDV_DEV void gdv_store16(gdv_uint8* dst, gdv_uint64 lo, gdv_uint64 hi) {
#ifdef GDV_NT_STRING_STORES
  typedef gdv_u64x2_t __attribute__((aligned(1))) unaligned_t;
  gdv_u64x2_t v;
  v.x = lo;
  v.y = hi;
  __builtin_nontemporal_store(v, (unaligned_t*)dst);
#else
  gdv_uint64 q[2] = {lo, hi};
  __builtin_memcpy(dst, q, 16);
#endif
}
#ifdef GDV_U
template <typename T>
GDV_DEV void gdv_rot(T (&a)[GDV_U]) {
  const T t = a[0];
#pragma unroll
  for (int k = 0; k + 1 < GDV_U; k++) a[k] = a[k + 1];
  a[GDV_U - 1] = t;
}
#endif

// Bit of an arbitrary row (selection-vector path: rows are gathered, no word structure).
GDV_DEV bool gdv_bitmap_bit(const gdv_bitmap& bm, gdv_int64 row) {
  gdv_int64 pos = row + bm.shift;
  gdv_int64 i = pos >> 6;
  i = i < bm.nwords - 1 ? i : bm.nwords - 1;
  return (bm.p[i] >> (pos & 63)) & 1ull;
}

GDV_DEV bool gdv_lane_bit(gdv_uint64 word, int lane) { return (word >> lane) & 1ull; }

// ------------------------------------------------------------------ arithmetic
// Integer arithmetic wraps (two's complement); done in the unsigned domain so that the
// wrap is defined behaviour.  Names: <op>_<type>_<type>, as in the reference's
// precompiled arithmetic_ops.cc.

#define GDV_INT_TYPES(X) \
  X(int8, uint8) X(int16, uint16) X(int32, uint32) X(int64, uint64) \
  X(uint8, uint8) X(uint16, uint16) X(uint32, uint32) X(uint64, uint64)
#define GDV_FLOAT_TYPES(X) X(float32) X(float64)
#define GDV_NUMERIC_TYPES(X) \
  X(int8) X(int16) X(int32) X(int64) X(uint8) X(uint16) X(uint32) X(uint64) X(float32) X(float64)

#define GDV_INT_ARITH(T, U)                                                                      \
  GDV_DEV gdv_##T add_##T##_##T(gdv_##T a, gdv_##T b) {                                          \
    return (gdv_##T)(gdv_##U)((gdv_##U)a + (gdv_##U)b);                                          \
  }                                                                                              \
  GDV_DEV gdv_##T subtract_##T##_##T(gdv_##T a, gdv_##T b) {                                     \
    return (gdv_##T)(gdv_##U)((gdv_##U)a - (gdv_##U)b);                                          \
  }                                                                                              \
  GDV_DEV gdv_##T multiply_##T##_##T(gdv_##T a, gdv_##T b) {                                     \
    return (gdv_##T)(gdv_##U)((gdv_##U)a * (gdv_##U)b);                                          \
  }                                                                                              \
  /* x / 0 raises "divide by zero error" and yields 0; MIN / -1 wraps to MIN. */                 \
  GDV_DEV gdv_##T divide_##T##_##T(gdv_ctx ctx, gdv_##T a, gdv_##T b) {                          \
    if (b == 0) { gdv_raise(ctx, GDV_ERR_DIV_ZERO); return 0; }                                  \
    if ((gdv_##T)(-1) < 0 && b == (gdv_##T)(-1)) return (gdv_##T)(gdv_##U)(0 - (gdv_##U)a);      \
    return (gdv_##T)(a / b);                                                                     \
  }
GDV_INT_TYPES(GDV_INT_ARITH)

#define GDV_FLOAT_ARITH(T)                                                                       \
  GDV_DEV gdv_##T add_##T##_##T(gdv_##T a, gdv_##T b) { return a + b; }                          \
  GDV_DEV gdv_##T subtract_##T##_##T(gdv_##T a, gdv_##T b) { return a - b; }                     \
  GDV_DEV gdv_##T multiply_##T##_##T(gdv_##T a, gdv_##T b) { return a * b; }                     \
  GDV_DEV gdv_##T divide_##T##_##T(gdv_ctx ctx, gdv_##T a, gdv_##T b) {                          \
    if (b == 0) { gdv_raise(ctx, GDV_ERR_DIV_ZERO); return 0; }                                  \
    return a / b;                                                                                \
  }
GDV_FLOAT_TYPES(GDV_FLOAT_ARITH)

// mod: a zero divisor returns the dividend unchanged (integer) / raises (float64).
GDV_DEV gdv_int32 mod_int64_int32(gdv_int64 a, gdv_int32 b) {
  if (b == 0) return (gdv_int32)a;
  if (b == -1) return 0;
  return (gdv_int32)(a % b);
}
GDV_DEV gdv_int64 mod_int64_int64(gdv_int64 a, gdv_int64 b) {
  if (b == 0) return a;
  if (b == -1) return 0;
  return a % b;
}
GDV_DEV gdv_int32 mod_int32_int32(gdv_int32 a, gdv_int32 b) {
  if (b == 0) return a;
  if (b == -1) return 0;
  return a % b;
}
GDV_DEV gdv_float64 mod_float64_float64(gdv_ctx ctx, gdv_float64 a, gdv_float64 b) {
  if (b == 0.0) { gdv_raise(ctx, GDV_ERR_DIV_ZERO); return 0.0; }
  return fmod(a, b);
}

GDV_DEV gdv_int32 negative_int32(gdv_int32 a) { return (gdv_int32)(0u - (gdv_uint32)a); }
GDV_DEV gdv_int64 negative_int64(gdv_int64 a) { return (gdv_int64)(0ull - (gdv_uint64)a); }
GDV_DEV gdv_float32 negative_float32(gdv_float32 a) { return -a; }
GDV_DEV gdv_float64 negative_float64(gdv_float64 a) { return -a; }
GDV_DEV gdv_int32 abs_int32(gdv_int32 a) { return a < 0 ? negative_int32(a) : a; }
GDV_DEV gdv_int64 abs_int64(gdv_int64 a) { return a < 0 ? negative_int64(a) : a; }
GDV_DEV gdv_float32 abs_float32(gdv_float32 a) { return fabsf(a); }
GDV_DEV gdv_float64 abs_float64(gdv_float64 a) { return fabs(a); }

// ------------------------------------------------------------------ relational

#define GDV_RELOPS(T)                                                                         \
  GDV_DEV bool equal_##T##_##T(gdv_##T a, gdv_##T b) { return a == b; }                       \
  GDV_DEV bool not_equal_##T##_##T(gdv_##T a, gdv_##T b) { return a != b; }                   \
  GDV_DEV bool less_than_##T##_##T(gdv_##T a, gdv_##T b) { return a < b; }                    \
  GDV_DEV bool less_than_or_equal_to_##T##_##T(gdv_##T a, gdv_##T b) { return a <= b; }       \
  GDV_DEV bool greater_than_##T##_##T(gdv_##T a, gdv_##T b) { return a > b; }                 \
  GDV_DEV bool greater_than_or_equal_to_##T##_##T(gdv_##T a, gdv_##T b) { return a >= b; }
GDV_NUMERIC_TYPES(GDV_RELOPS)
GDV_RELOPS(boolean)
GDV_RELOPS(date32)
GDV_RELOPS(date64)
GDV_RELOPS(timestamp)
GDV_RELOPS(time32)
GDV_RELOPS(time64)

GDV_DEV bool not_boolean(bool a) { return !a; }

// null-aware predicates: the value function sees (value, validity) pairs
template <typename T>
GDV_DEV bool gdv_isnull(T, bool valid) { return !valid; }
template <typename T>
GDV_DEV bool gdv_isnotnull(T, bool valid) { return valid; }
template <typename T>
GDV_DEV bool gdv_is_distinct_from(T a, bool av, T b, bool bv) {
  if (av != bv) return true;
  if (!av) return false;
  return a != b;
}
template <typename T>
GDV_DEV bool gdv_is_not_distinct_from(T a, bool av, T b, bool bv) {
  return !gdv_is_distinct_from(a, av, b, bv);
}

// IN-lists compare zero-extended bit images, so one sorted uint64 table serves every
// fixed-width type.
GDV_DEV gdv_uint64 gdv_bits64(gdv_int8 v) { return (gdv_uint8)v; }
GDV_DEV gdv_uint64 gdv_bits64(gdv_uint8 v) { return v; }
GDV_DEV gdv_uint64 gdv_bits64(gdv_int16 v) { return (gdv_uint16)v; }
GDV_DEV gdv_uint64 gdv_bits64(gdv_uint16 v) { return v; }
GDV_DEV gdv_uint64 gdv_bits64(gdv_int32 v) { return (gdv_uint32)v; }
GDV_DEV gdv_uint64 gdv_bits64(gdv_uint32 v) { return v; }
GDV_DEV gdv_uint64 gdv_bits64(gdv_int64 v) { return (gdv_uint64)v; }
GDV_DEV gdv_uint64 gdv_bits64(gdv_uint64 v) { return v; }
GDV_DEV gdv_uint64 gdv_bits64(gdv_float32 v) { return __float_as_uint(v); }
GDV_DEV gdv_uint64 gdv_bits64(gdv_float64 v) { return (gdv_uint64)__double_as_longlong(v); }
GDV_DEV bool gdv_in_sorted(gdv_uint64 x, const gdv_uint64* tab, int n) {
  int lo = 0, hi = n;
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (tab[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo < n && tab[lo] == x;
}
GDV_DEV gdv_int128 gdv_make_int128(gdv_uint64 hi, gdv_uint64 lo) {
  return (gdv_int128)(((gdv_uint128)hi << 64) | lo);
}

// min/max style helpers of later reference versions
#define GDV_MINMAX(T)                                                                 \
  GDV_DEV gdv_##T greatest_##T##_##T(gdv_##T a, gdv_##T b) { return a > b ? a : b; }  \
  GDV_DEV gdv_##T least_##T##_##T(gdv_##T a, gdv_##T b) { return a < b ? a : b; }
GDV_MINMAX(int32) GDV_MINMAX(int64) GDV_MINMAX(float32) GDV_MINMAX(float64)

// ------------------------------------------------------------------ bitwise / boolean tests / nvl
#define GDV_BITWISE(T)                                                                       \
  GDV_DEV gdv_##T bitwise_and_##T##_##T(gdv_##T a, gdv_##T b) { return (gdv_##T)(a & b); }   \
  GDV_DEV gdv_##T bitwise_or_##T##_##T(gdv_##T a, gdv_##T b) { return (gdv_##T)(a | b); }    \
  GDV_DEV gdv_##T bitwise_xor_##T##_##T(gdv_##T a, gdv_##T b) { return (gdv_##T)(a ^ b); }   \
  GDV_DEV gdv_##T bitwise_not_##T(gdv_##T a) { return (gdv_##T)(~a); }
GDV_BITWISE(int32) GDV_BITWISE(int64) GDV_BITWISE(uint32) GDV_BITWISE(uint64)
// null-aware boolean tests: never null themselves
GDV_DEV bool istrue_boolean(bool v, bool valid) { return valid && v; }
GDV_DEV bool isfalse_boolean(bool v, bool valid) { return valid && !v; }
GDV_DEV bool isnottrue_boolean(bool v, bool valid) { return !(valid && v); }
GDV_DEV bool isnotfalse_boolean(bool v, bool valid) { return !(valid && !v); }
// nvl(a, b): a when a is valid, else b; null only when both are null
template <typename T>
GDV_DEV T gdv_nvl(T a, bool av, T b, bool bv, bool* out_valid) {
  *out_valid = av || bv;
  return av ? a : b;
}

// ------------------------------------------------------------------ casts
GDV_DEV gdv_int64 castBIGINT_int32(gdv_int32 a) { return (gdv_int64)a; }
GDV_DEV gdv_int32 castINT_int64(gdv_int64 a) { return (gdv_int32)(gdv_uint32)(gdv_uint64)a; }
GDV_DEV gdv_float32 castFLOAT4_int32(gdv_int32 a) { return (gdv_float32)a; }
GDV_DEV gdv_float32 castFLOAT4_int64(gdv_int64 a) { return (gdv_float32)a; }
GDV_DEV gdv_float32 castFLOAT4_float64(gdv_float64 a) { return (gdv_float32)a; }
GDV_DEV gdv_float64 castFLOAT8_int32(gdv_int32 a) { return (gdv_float64)a; }
GDV_DEV gdv_float64 castFLOAT8_int64(gdv_int64 a) { return (gdv_float64)a; }
GDV_DEV gdv_float64 castFLOAT8_float32(gdv_float32 a) { return (gdv_float64)a; }
// float -> integer casts round half away from zero and saturate (out-of-range and NaN
// inputs are undefined on the reference's CPU path; saturation / 0 keeps them defined).
// GDV_CAST_X86_INDEFINITE (set at Make through the environment variable of that name; round 6): what the reference's JIT
// yields on x86 for such inputs instead — cvttsd2si's "indefinite integer", 0x8000...0 of the destination width, for NaN
// and for everything outside the destination's range (bit-exactness with the CPU path where a caller depends on it).
#ifdef GDV_CAST_X86_INDEFINITE
GDV_DEV gdv_int64 gdv_sat_i64(gdv_float64 r) {
  if (!(r < 9223372036854775808.0 && r >= -9223372036854775808.0)) return (gdv_int64)0x8000000000000000ULL;
  return (gdv_int64)r;
}
GDV_DEV gdv_int32 gdv_sat_i32(gdv_float64 r) {
  if (!(r < 2147483648.0 && r > -2147483649.0)) return (gdv_int32)0x80000000u;
  return (gdv_int32)r;
}
#else
GDV_DEV gdv_int64 gdv_sat_i64(gdv_float64 r) {
  if (r != r) return 0;
  if (r >= 9223372036854775808.0) return 0x7fffffffffffffffLL;
  if (r <= -9223372036854775808.0) return (gdv_int64)0x8000000000000000ULL;
  return (gdv_int64)r;
}
GDV_DEV gdv_int32 gdv_sat_i32(gdv_float64 r) {
  if (r != r) return 0;
  if (r >= 2147483647.0) return 2147483647;
  if (r <= -2147483648.0) return (gdv_int32)0x80000000u;
  return (gdv_int32)r;
}
#endif
// round half away from zero the way the reference writes it (precompiled extended_math_ops:
// `trunc(x + (x >= 0 ? 0.5 : -0.5))`), NOT C round(): the sum is itself rounded to nearest even,
// so 0.49999999999999994 -> 1 and odd integers in [2^52, 2^53) move to the next even one.
// float32 arguments are widened first (the reference's 0.5 is a double literal): exact.
GDV_DEV gdv_float64 gdv_round_half_away(gdv_float64 a) { return trunc(a + (a >= 0 ? 0.5 : -0.5)); }
GDV_DEV gdv_int64 castBIGINT_float32(gdv_float32 a) { return gdv_sat_i64(gdv_round_half_away((gdv_float64)a)); }
GDV_DEV gdv_int64 castBIGINT_float64(gdv_float64 a) { return gdv_sat_i64(gdv_round_half_away(a)); }
GDV_DEV gdv_int32 castINT_float32(gdv_float32 a) { return gdv_sat_i32(gdv_round_half_away((gdv_float64)a)); }
GDV_DEV gdv_int32 castINT_float64(gdv_float64 a) { return gdv_sat_i32(gdv_round_half_away(a)); }

GDV_DEV gdv_date64 castDATE_int64(gdv_int64 a) { return a; }
GDV_DEV gdv_timestamp castTIMESTAMP_int64(gdv_int64 a) { return a; }
GDV_DEV gdv_timestamp castTIMESTAMP_date64(gdv_date64 a) { return a; }
GDV_DEV gdv_int64 castBIGINT_date64(gdv_date64 a) { return a; }
GDV_DEV gdv_int64 castBIGINT_timestamp(gdv_timestamp a) { return a; }

// ------------------------------------------------------------------ extended math
GDV_DEV gdv_float64 cbrt_float64(gdv_float64 a) { return cbrt(a); }
GDV_DEV gdv_float64 exp_float64(gdv_float64 a) { return exp(a); }
GDV_DEV gdv_float64 log_float64(gdv_float64 a) { return log(a); }
GDV_DEV gdv_float64 log10_float64(gdv_float64 a) { return log10(a); }
GDV_DEV gdv_float64 sqrt_float64(gdv_float64 a) { return sqrt(a); }
GDV_DEV gdv_float64 power_float64_float64(gdv_float64 a, gdv_float64 b) { return pow(a, b); }
GDV_DEV gdv_float64 log_float64_float64(gdv_ctx ctx, gdv_float64 base, gdv_float64 v) {
  gdv_float64 lb = log(base);
  if (lb == 0.0) { gdv_raise(ctx, GDV_ERR_DIV_ZERO); return 0.0; }
  return log(v) / lb;
}
GDV_DEV gdv_float64 floor_float64(gdv_float64 a) { return floor(a); }
GDV_DEV gdv_float64 ceil_float64(gdv_float64 a) { return ceil(a); }
GDV_DEV gdv_float64 round_float64(gdv_float64 a) { return gdv_round_half_away(a); }
GDV_DEV gdv_float64 truncate_float64(gdv_float64 a) { return trunc(a); }

// ------------------------------------------------------------------ numeric tail: trigonometry, sign, pmod, round to a
// scale, shifts, gcd / lcm.  All null-if-null, none takes a context, none raises; integer work is done in unsigned types
// (no signed overflow, no shift by the width or more).  What is recollection and what was decided: PARITY.md, numeric tail.
//
// Trigonometry and angles: the argument is converted to double once, the result is float64.  cot is tan(pi/2 - x) with
// ONE subtraction from the double nearest pi/2 (the lineage's formula as recalled, not the mathematical cotangent: for
// large |x| the subtraction absorbs pi/2); degrees / radians are ONE multiplication by the double 180/pi, pi/180.
#define GDV_PI 3.14159265358979323846
GDV_DEV gdv_float64 gdv_cot(gdv_float64 x) { return tan(GDV_PI / 2 - x); }
GDV_DEV gdv_float64 gdv_degrees(gdv_float64 x) { return x * (180.0 / GDV_PI); }
GDV_DEV gdv_float64 gdv_radians(gdv_float64 x) { return x * (GDV_PI / 180.0); }
#define GDV_TRIG_FNS(X, T)                                                                                  \
  X(sin, sin, T) X(cos, cos, T) X(tan, tan, T) X(asin, asin, T) X(acos, acos, T) X(atan, atan, T)           \
  X(sinh, sinh, T) X(cosh, cosh, T) X(tanh, tanh, T) X(cot, gdv_cot, T) X(degrees, gdv_degrees, T)          \
  X(radians, gdv_radians, T)
#define GDV_TRIG(name, f, T) GDV_DEV gdv_float64 name##_##T(gdv_##T a) { return f((gdv_float64)a); }
GDV_TRIG_FNS(GDV_TRIG, int32) GDV_TRIG_FNS(GDV_TRIG, int64) GDV_TRIG_FNS(GDV_TRIG, float32) GDV_TRIG_FNS(GDV_TRIG, float64)
GDV_DEV gdv_float64 atan2_float64_float64(gdv_float64 y, gdv_float64 x) { return atan2(y, x); }

// sign: -1, 0 or 1 in the argument's type; +-0 -> +0.0, NaN -> NaN
GDV_DEV gdv_int32 sign_int32(gdv_int32 a) { return (a > 0) - (a < 0); }
GDV_DEV gdv_int64 sign_int64(gdv_int64 a) { return (gdv_int64)((a > 0) - (a < 0)); }
GDV_DEV gdv_float32 sign_float32(gdv_float32 a) { return a != a ? a : a > 0 ? 1.0f : a < 0 ? -1.0f : 0.0f; }
GDV_DEV gdv_float64 sign_float64(gdv_float64 a) { return a != a ? a : a > 0 ? 1.0 : a < 0 ? -1.0 : 0.0; }

// pmod: the floored modulus (the divisor's sign); a zero divisor returns the dividend, as integer mod does.  The
// remainder is moved by the divisor only where their signs differ, so the sum cannot leave the type.
#define GDV_PMOD(T, U)                                                       \
  GDV_DEV gdv_##T pmod_##T##_##T(gdv_##T a, gdv_##T n) {                     \
    if (n == 0) return a;                                                    \
    if (n == -1) return 0;                                                   \
    const gdv_##T r = a % n;                                                 \
    if (r != 0 && ((r ^ n) < 0)) return (gdv_##T)((gdv_##U)r + (gdv_##U)n);  \
    return r;                                                                \
  }
GDV_PMOD(int32, uint32) GDV_PMOD(int64, uint64)

// round / truncate of an integer to a scale: scale >= 0 gives the value, scale s < 0 a multiple of 10^-s (round: half away
// from zero, truncate: toward zero), |s| above 9 / 18 gives 0.  The magnitude is taken unsigned; a result that does not
// fit wraps modulo 2^w.
GDV_DEV gdv_uint64 gdv_pow10_u64(int k) {  // k in 0..19
  gdv_uint64 p = 1;
  for (int i = 0; i < k; i++) p *= 10u;
  return p;
}
#define GDV_INT_SCALE(T, U, MAXS)                                                                  \
  GDV_DEV gdv_##T gdv_to_scale_##T(gdv_##T a, gdv_int32 s, bool half) {                            \
    if (s >= 0) return a;                                                                          \
    if (s < -(MAXS)) return 0;                                                                     \
    const gdv_##U p = (gdv_##U)gdv_pow10_u64(-s);                                                  \
    const gdv_##U mag = a < 0 ? (gdv_##U)0 - (gdv_##U)a : (gdv_##U)a;                              \
    const gdv_##U r = mag % p;                                                                     \
    gdv_##U q = mag - r;                                                                           \
    if (half && r >= p - r) q += p;                                                                \
    return (gdv_##T)(a < 0 ? (gdv_##U)0 - q : q);                                                  \
  }                                                                                                \
  GDV_DEV gdv_##T round_##T(gdv_##T a) { return a; }                                               \
  GDV_DEV gdv_##T round_##T##_int32(gdv_##T a, gdv_int32 s) { return gdv_to_scale_##T(a, s, true); } \
  GDV_DEV gdv_##T truncate_##T##_int32(gdv_##T a, gdv_int32 s) { return gdv_to_scale_##T(a, s, false); }
GDV_INT_SCALE(int32, uint32, 9) GDV_INT_SCALE(int64, uint64, 18)

// round of a float to a scale: trunc(x * m + (x >= 0 ? 0.5 : -0.5)) / m in double, m = the double nearest 10^s from a
// constant table (-308 <= s <= 308; no pow).  NaN and infinities are returned as they are, and so is x where x * m is
// not finite or s > 308; s < -308 gives 0.0 with x's sign.  float32: widened first, narrowed once at the end.
#define GDV_P10_ROW(p) p##0, p##1, p##2, p##3, p##4, p##5, p##6, p##7, p##8, p##9
#define GDV_P10_TABLE(e)                                                                                              \
  GDV_P10_ROW(e), GDV_P10_ROW(e##1), GDV_P10_ROW(e##2), GDV_P10_ROW(e##3), GDV_P10_ROW(e##4), GDV_P10_ROW(e##5),      \
  GDV_P10_ROW(e##6), GDV_P10_ROW(e##7), GDV_P10_ROW(e##8), GDV_P10_ROW(e##9), GDV_P10_ROW(e##10), GDV_P10_ROW(e##11), \
  GDV_P10_ROW(e##12), GDV_P10_ROW(e##13), GDV_P10_ROW(e##14), GDV_P10_ROW(e##15), GDV_P10_ROW(e##16),                 \
  GDV_P10_ROW(e##17), GDV_P10_ROW(e##18), GDV_P10_ROW(e##19), GDV_P10_ROW(e##20), GDV_P10_ROW(e##21),                 \
  GDV_P10_ROW(e##22), GDV_P10_ROW(e##23), GDV_P10_ROW(e##24), GDV_P10_ROW(e##25), GDV_P10_ROW(e##26),                 \
  GDV_P10_ROW(e##27), GDV_P10_ROW(e##28), GDV_P10_ROW(e##29), e##300, e##301, e##302, e##303, e##304, e##305, e##306, \
  e##307, e##308
GDV_DEV gdv_float64 gdv_pow10_f64(gdv_int32 s) {  // s in -308..308
  static constexpr gdv_float64 kUp[309] = {GDV_P10_TABLE(1e)};
  static constexpr gdv_float64 kDown[309] = {GDV_P10_TABLE(1e-)};
  return s >= 0 ? kUp[s] : kDown[-s];
}
GDV_DEV gdv_float64 round_float64_int32(gdv_float64 x, gdv_int32 s) {
  if (!(fabs(x) <= 1.7976931348623157e308)) return x;  // NaN, +-inf
  if (s > 308) return x;
  if (s < -308) return copysign(0.0, x);
  const gdv_float64 m = gdv_pow10_f64(s);
  const gdv_float64 xm = x * m;
  if (!(fabs(xm) <= 1.7976931348623157e308)) return x;
  return trunc(xm + (x >= 0 ? 0.5 : -0.5)) / m;
}
GDV_DEV gdv_float32 round_float32_int32(gdv_float32 x, gdv_int32 s) {
  if (!(fabsf(x) <= 3.40282347e38f)) return x;
  return (gdv_float32)round_float64_int32((gdv_float64)x, s);
}

// shifts: the count is taken modulo the width (Java's rule), so negative counts follow from the mask
#define GDV_SHIFTS(T, U, MASK)                                                                                    \
  GDV_DEV gdv_##T shift_left_##T##_int32(gdv_##T a, gdv_int32 n) { return (gdv_##T)((gdv_##U)a << (n & MASK)); }  \
  GDV_DEV gdv_##T shift_right_unsigned_##T##_int32(gdv_##T a, gdv_int32 n) {                                      \
    return (gdv_##T)((gdv_##U)a >> (n & MASK));                                                                   \
  }                                                                                                               \
  GDV_DEV gdv_##T shift_right_##T##_int32(gdv_##T a, gdv_int32 n) { /* arithmetic: the sign fills from the top */ \
    const gdv_##U fill = a < 0 ? ~(~(gdv_##U)0 >> (n & MASK)) : (gdv_##U)0;                                       \
    return (gdv_##T)(((gdv_##U)a >> (n & MASK)) | fill);                                                          \
  }
GDV_SHIFTS(int32, uint32, 31) GDV_SHIFTS(int64, uint64, 63)

// gcd / lcm over the magnitudes as uint64: the non-negative value, gcd(0, 0) = 0, lcm(0, x) = 0; a result of 2^63 or
// above wraps.  Binary GCD on count-trailing-zeros: shifts and subtractions, no 64-bit division (a software routine here).
GDV_DEV gdv_uint64 gdv_gcd_u64(gdv_uint64 a, gdv_uint64 b) {
  if (a == 0) return b;
  if (b == 0) return a;
  const int shift = __builtin_ctzll(a | b);
  a >>= __builtin_ctzll(a);
  do {
    b >>= __builtin_ctzll(b);
    if (a > b) { const gdv_uint64 t = a; a = b; b = t; }
    b -= a;
  } while (b != 0);
  return a << shift;
}
GDV_DEV gdv_uint64 gdv_mag_u64(gdv_int64 a) { return a < 0 ? 0ull - (gdv_uint64)a : (gdv_uint64)a; }
GDV_DEV gdv_int64 gcd_int64_int64(gdv_int64 a, gdv_int64 b) { return (gdv_int64)gdv_gcd_u64(gdv_mag_u64(a), gdv_mag_u64(b)); }
GDV_DEV gdv_int64 lcm_int64_int64(gdv_int64 a, gdv_int64 b) {
  const gdv_uint64 x = gdv_mag_u64(a), y = gdv_mag_u64(b);
  if (x == 0 || y == 0) return 0;
  return (gdv_int64)(x / gdv_gcd_u64(x, y) * y);
}

// ------------------------------------------------------------------ hash
// Murmur3-derived hashes over the 8-byte image of the value as a double (every numeric
// type is first converted to double).  A null input hashes to the seed (0 without seed).
GDV_DEV gdv_uint64 gdv_rotl64(gdv_uint64 v, int d) { return (v << d) | (v >> (64 - d)); }
GDV_DEV gdv_uint64 gdv_fmix64(gdv_uint64 k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdULL;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ULL;
  k ^= k >> 33;
  return k;
}
GDV_DEV gdv_int64 gdv_murmur3_64(gdv_uint64 val, gdv_int32 seed) {
  gdv_uint64 h1 = (gdv_uint64)(gdv_int64)seed;
  gdv_uint64 h2 = (gdv_uint64)(gdv_int64)seed;
  const gdv_uint64 c1 = 0x87c37b91114253d5ULL;
  const gdv_uint64 c2 = 0x4cf5ad432745937fULL;
  const gdv_uint64 length = 8;
  gdv_uint64 k1 = val;
  k1 *= c1;
  k1 = gdv_rotl64(k1, 31);
  k1 *= c2;
  h1 ^= k1;
  h1 ^= length;
  h2 ^= length;
  h1 += h2;
  h2 += h1;
  h1 = gdv_fmix64(h1);
  h2 = gdv_fmix64(h2);
  h1 += h2;
  return (gdv_int64)h1;
}
GDV_DEV gdv_int32 gdv_murmur3_32(gdv_uint64 val, gdv_int32 seed) {
  const gdv_uint32 c1 = 0xcc9e2d51u;
  const gdv_uint32 c2 = 0x1b873593u;
  gdv_uint32 h = (gdv_uint32)seed;
  for (int i = 0; i < 2; i++) {
    gdv_uint32 k = (gdv_uint32)(val >> (i * 32));
    k *= c1;
    k = (k << 15) | (k >> 17);
    k *= c2;
    h ^= k;
    h = (h << 13) | (h >> 19);
    h = h * 5u + 0xe6546b64u;
  }
  h ^= 8u;
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return (gdv_int32)h;
}
GDV_DEV gdv_uint64 gdv_double_bits(gdv_float64 v) { return (gdv_uint64)__double_as_longlong(v); }

#define GDV_HASH(T)                                                                              \
  GDV_DEV gdv_int32 hash32_##T(gdv_##T v, bool valid) {                                          \
    return valid ? gdv_murmur3_32(gdv_double_bits((gdv_float64)v), 0) : 0;                       \
  }                                                                                              \
  GDV_DEV gdv_int32 hash32_##T##_int32(gdv_##T v, bool valid, gdv_int32 seed, bool sv) {         \
    gdv_int32 s = sv ? seed : 0;                                                                 \
    return valid ? gdv_murmur3_32(gdv_double_bits((gdv_float64)v), s) : s;                       \
  }                                                                                              \
  GDV_DEV gdv_int64 hash64_##T(gdv_##T v, bool valid) {                                          \
    return valid ? gdv_murmur3_64(gdv_double_bits((gdv_float64)v), 0) : 0;                       \
  }                                                                                              \
  GDV_DEV gdv_int64 hash64_##T##_int64(gdv_##T v, bool valid, gdv_int64 seed, bool sv) {         \
    gdv_int64 s = sv ? seed : 0;                                                                 \
    return valid ? gdv_murmur3_64(gdv_double_bits((gdv_float64)v), (gdv_int32)s) : s;            \
  }
GDV_NUMERIC_TYPES(GDV_HASH)
GDV_HASH(boolean)
GDV_HASH(date32)
GDV_HASH(date64)
GDV_HASH(timestamp)
GDV_HASH(time32)

// ------------------------------------------------------------------ date / time
// Civil-calendar arithmetic on day counts since 1970-01-01 (proleptic Gregorian), the
// public-domain algorithms of H. Hinnant's date library that the reference vendors
// (present here as pyarrow/include/arrow/vendored/datetime/date.h).
#define GDV_MILLIS_IN_DAY 86400000LL

GDV_DEV gdv_int64 gdv_floor_div(gdv_int64 a, gdv_int64 b) {
  gdv_int64 q = a / b;
  return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q;
}
// (from the remainder, not as a - floor_div * b: that product leaves int64 within the first partial day above INT64_MIN)
GDV_DEV gdv_int64 gdv_floor_mod(gdv_int64 a, gdv_int64 b) {
  const gdv_int64 r = a % b;
  return (r != 0 && ((r < 0) != (b < 0))) ? r + b : r;
}

struct gdv_ymd {
  gdv_int64 y;
  gdv_int32 m;  // 1..12
  gdv_int32 d;  // 1..31
};
GDV_DEV gdv_ymd gdv_civil_from_days(gdv_int64 z) {
  z += 719468;
  const gdv_int64 era = (z >= 0 ? z : z - 146096) / 146097;
  const gdv_uint32 doe = (gdv_uint32)(z - era * 146097);
  const gdv_uint32 yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
  const gdv_int64 y = (gdv_int64)yoe + era * 400;
  const gdv_uint32 doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
  const gdv_uint32 mp = (5 * doy + 2) / 153;
  const gdv_uint32 d = doy - (153 * mp + 2) / 5 + 1;
  const gdv_uint32 m = mp < 10 ? mp + 3 : mp - 9;
  gdv_ymd r;
  r.y = y + (m <= 2);
  r.m = (gdv_int32)m;
  r.d = (gdv_int32)d;
  return r;
}
GDV_DEV gdv_int64 gdv_days_from_civil(gdv_int64 y, gdv_int32 m, gdv_int32 d) {
  y -= m <= 2;
  const gdv_int64 era = (y >= 0 ? y : y - 399) / 400;
  const gdv_uint32 yoe = (gdv_uint32)(y - era * 400);
  const gdv_uint32 doy = (153 * (m > 2 ? m - 3 : m + 9) + 2) / 5 + d - 1;
  const gdv_uint32 doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  return era * 146097 + (gdv_int64)doe - 719468;
}
GDV_DEV bool gdv_is_leap(gdv_int64 y) { return (y % 4 == 0) && (y % 100 != 0 || y % 400 == 0); }
GDV_DEV gdv_int32 gdv_last_day_of_month(gdv_int64 y, gdv_int32 m) {
  const gdv_int32 t[12] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
  return (m == 2 && gdv_is_leap(y)) ? 29 : t[m - 1];
}

#define GDV_EXTRACT(T, TO_MILLIS)                                                                 \
  GDV_DEV gdv_int64 extractYear_##T(gdv_##T v) {                                                  \
    return gdv_civil_from_days(gdv_floor_div(TO_MILLIS(v), GDV_MILLIS_IN_DAY)).y;                 \
  }                                                                                               \
  GDV_DEV gdv_int64 extractMonth_##T(gdv_##T v) {                                                 \
    return gdv_civil_from_days(gdv_floor_div(TO_MILLIS(v), GDV_MILLIS_IN_DAY)).m;                 \
  }                                                                                               \
  GDV_DEV gdv_int64 extractDay_##T(gdv_##T v) {                                                   \
    return gdv_civil_from_days(gdv_floor_div(TO_MILLIS(v), GDV_MILLIS_IN_DAY)).d;                 \
  }                                                                                               \
  GDV_DEV gdv_int64 extractQuarter_##T(gdv_##T v) { return (extractMonth_##T(v) - 1) / 3 + 1; }   \
  GDV_DEV gdv_int64 extractDoy_##T(gdv_##T v) {                                                   \
    gdv_int64 days = gdv_floor_div(TO_MILLIS(v), GDV_MILLIS_IN_DAY);                              \
    return days - gdv_days_from_civil(gdv_civil_from_days(days).y, 1, 1) + 1;                     \
  }                                                                                               \
  /* 1 = Sunday … 7 = Saturday */                                                                 \
  GDV_DEV gdv_int64 extractDow_##T(gdv_##T v) {                                                   \
    gdv_int64 days = gdv_floor_div(TO_MILLIS(v), GDV_MILLIS_IN_DAY);                              \
    return gdv_floor_mod(days + 4, 7) + 1;                                                        \
  }                                                                                               \
  GDV_DEV gdv_int64 extractHour_##T(gdv_##T v) {                                                  \
    return gdv_floor_mod(TO_MILLIS(v), GDV_MILLIS_IN_DAY) / 3600000LL;                            \
  }                                                                                               \
  GDV_DEV gdv_int64 extractMinute_##T(gdv_##T v) {                                                \
    return (gdv_floor_mod(TO_MILLIS(v), GDV_MILLIS_IN_DAY) / 60000LL) % 60;                       \
  }                                                                                               \
  GDV_DEV gdv_int64 extractSecond_##T(gdv_##T v) {                                                \
    return (gdv_floor_mod(TO_MILLIS(v), GDV_MILLIS_IN_DAY) / 1000LL) % 60;                        \
  }                                                                                               \
  GDV_DEV gdv_int64 extractEpoch_##T(gdv_##T v) { return gdv_floor_div(TO_MILLIS(v), 1000LL); }   \
  GDV_DEV gdv_int64 extractDecade_##T(gdv_##T v) { return extractYear_##T(v) / 10; }              \
  GDV_DEV gdv_int64 extractCentury_##T(gdv_##T v) { return (extractYear_##T(v) - 1) / 100 + 1; }  \
  GDV_DEV gdv_int64 extractMillennium_##T(gdv_##T v) {                                            \
    return (extractYear_##T(v) - 1) / 1000 + 1;                                                   \
  }
#define GDV_MS_IDENT(v) ((gdv_int64)(v))
#define GDV_MS_FROM_DAYS(v) ((gdv_int64)(v) * GDV_MILLIS_IN_DAY)
GDV_EXTRACT(date64, GDV_MS_IDENT)
GDV_EXTRACT(timestamp, GDV_MS_IDENT)
GDV_EXTRACT(date32, GDV_MS_FROM_DAYS)

// date_trunc_<Unit>(date64 | timestamp) [recalled: precompiled/time.cc DATE_TRUNC_FUNCTIONS over EpochTimePoint]:
// the start of the unit the instant lies in; weeks start on Monday.  Round 5, after the round-4 advisor's and the
// builder's recollections of upstream's macros agreed: the FIXED units (Second, Minute, Hour, Day) are upstream's
// DATE_TRUNC_FIXED_UNIT `(millis / N) * N` — C++ division, so an instant before 1970 goes UP, towards zero — and
// Decade / Century / Millennium are DATE_TRUNC_YEAR_UNITS `((year - 1) / N) * N + 1`: decades start in year ...1
// like centuries (2015 -> 2011-01-01), not at year / 10 * 10 as rounds 3-4 had it.  The calendar units go through
// the civil date of the floored day, as EpochTimePoint does.  extractWeek / weekofyear: the ISO-8601 week (week 1 holds January 4th).
// last_day: midnight of the last day of the instant's month.
GDV_DEV gdv_int64 gdv_trunc_to_ymd(gdv_int64 y, gdv_int32 m) { return gdv_days_from_civil(y, m, 1) * GDV_MILLIS_IN_DAY; }
GDV_DEV gdv_int64 gdv_iso_week(gdv_int64 days) {
  // the Thursday of this date's ISO week decides the ISO year; the week number is that Thursday's ordinal week
  const gdv_int64 thu = days - gdv_floor_mod(days + 3, 7) + 3;
  return (thu - gdv_days_from_civil(gdv_civil_from_days(thu).y, 1, 1)) / 7 + 1;
}
#define GDV_DATE_TRUNC(T)                                                                                   \
  GDV_DEV gdv_##T date_trunc_Second_##T(gdv_##T v) { return v / 1000LL * 1000LL; }                          \
  GDV_DEV gdv_##T date_trunc_Minute_##T(gdv_##T v) { return v / 60000LL * 60000LL; }                        \
  GDV_DEV gdv_##T date_trunc_Hour_##T(gdv_##T v) { return v / 3600000LL * 3600000LL; }                      \
  GDV_DEV gdv_##T date_trunc_Day_##T(gdv_##T v) { return v / GDV_MILLIS_IN_DAY * GDV_MILLIS_IN_DAY; }        \
  GDV_DEV gdv_##T date_trunc_Week_##T(gdv_##T v) {                                                          \
    const gdv_int64 days = gdv_floor_div(v, GDV_MILLIS_IN_DAY);                                             \
    return (days - gdv_floor_mod(days + 3, 7)) * GDV_MILLIS_IN_DAY; /* day 0 was a Thursday */              \
  }                                                                                                         \
  GDV_DEV gdv_##T date_trunc_Month_##T(gdv_##T v) {                                                         \
    const gdv_ymd c = gdv_civil_from_days(gdv_floor_div(v, GDV_MILLIS_IN_DAY));                             \
    return gdv_trunc_to_ymd(c.y, c.m);                                                                      \
  }                                                                                                         \
  GDV_DEV gdv_##T date_trunc_Quarter_##T(gdv_##T v) {                                                       \
    const gdv_ymd c = gdv_civil_from_days(gdv_floor_div(v, GDV_MILLIS_IN_DAY));                             \
    return gdv_trunc_to_ymd(c.y, (c.m - 1) / 3 * 3 + 1);                                                    \
  }                                                                                                         \
  GDV_DEV gdv_##T date_trunc_Year_##T(gdv_##T v) { return gdv_trunc_to_ymd(extractYear_##T(v), 1); }        \
  GDV_DEV gdv_##T date_trunc_Decade_##T(gdv_##T v) {                                                        \
    return gdv_trunc_to_ymd((extractYear_##T(v) - 1) / 10 * 10 + 1, 1);                                     \
  }                                                                                                         \
  GDV_DEV gdv_##T date_trunc_Century_##T(gdv_##T v) {                                                       \
    return gdv_trunc_to_ymd((extractYear_##T(v) - 1) / 100 * 100 + 1, 1);                                   \
  }                                                                                                         \
  GDV_DEV gdv_##T date_trunc_Millennium_##T(gdv_##T v) {                                                    \
    return gdv_trunc_to_ymd((extractYear_##T(v) - 1) / 1000 * 1000 + 1, 1);                                 \
  }                                                                                                         \
  GDV_DEV gdv_int64 extractWeek_##T(gdv_##T v) { return gdv_iso_week(gdv_floor_div(v, GDV_MILLIS_IN_DAY)); } \
  GDV_DEV gdv_date64 last_day_##T(gdv_##T v) {                                                              \
    const gdv_ymd c = gdv_civil_from_days(gdv_floor_div(v, GDV_MILLIS_IN_DAY));                             \
    return gdv_days_from_civil(c.y, c.m, gdv_last_day_of_month(c.y, c.m)) * GDV_MILLIS_IN_DAY;              \
  }
GDV_DATE_TRUNC(date64)
GDV_DATE_TRUNC(timestamp)

GDV_DEV gdv_int64 extractHour_time32(gdv_time32 v) { return (gdv_int64)v / 3600000; }
GDV_DEV gdv_int64 extractMinute_time32(gdv_time32 v) { return ((gdv_int64)v / 60000) % 60; }
GDV_DEV gdv_int64 extractSecond_time32(gdv_time32 v) { return ((gdv_int64)v / 1000) % 60; }

// Month arithmetic clamps the day to the last day of the target month.
GDV_DEV gdv_int64 gdv_add_months_ms(gdv_int64 millis, gdv_int64 months) {
  gdv_int64 days = gdv_floor_div(millis, GDV_MILLIS_IN_DAY);
  gdv_int64 tod = gdv_floor_mod(millis, GDV_MILLIS_IN_DAY);
  gdv_ymd c = gdv_civil_from_days(days);
  gdv_int64 total = c.y * 12 + (c.m - 1) + months;
  gdv_int64 ny = gdv_floor_div(total, 12);
  gdv_int32 nm = (gdv_int32)(total - ny * 12) + 1;
  gdv_int32 last = gdv_last_day_of_month(ny, nm);
  gdv_int32 nd = c.d > last ? last : c.d;
  return gdv_days_from_civil(ny, nm, nd) * GDV_MILLIS_IN_DAY + tod;
}

#define GDV_TSADD(T)                                                                              \
  GDV_DEV gdv_##T timestampaddSecond_int64_##T(gdv_int64 c, gdv_##T v) { return v + c * 1000LL; } \
  GDV_DEV gdv_##T timestampaddMinute_int64_##T(gdv_int64 c, gdv_##T v) { return v + c * 60000LL; }\
  GDV_DEV gdv_##T timestampaddHour_int64_##T(gdv_int64 c, gdv_##T v) { return v + c * 3600000LL; }\
  GDV_DEV gdv_##T timestampaddDay_int64_##T(gdv_int64 c, gdv_##T v) {                             \
    return v + c * GDV_MILLIS_IN_DAY;                                                             \
  }                                                                                               \
  GDV_DEV gdv_##T timestampaddWeek_int64_##T(gdv_int64 c, gdv_##T v) {                            \
    return v + c * 7 * GDV_MILLIS_IN_DAY;                                                         \
  }                                                                                               \
  GDV_DEV gdv_##T timestampaddMonth_int64_##T(gdv_int64 c, gdv_##T v) {                           \
    return gdv_add_months_ms(v, c);                                                               \
  }                                                                                               \
  GDV_DEV gdv_##T timestampaddQuarter_int64_##T(gdv_int64 c, gdv_##T v) {                         \
    return gdv_add_months_ms(v, c * 3);                                                           \
  }                                                                                               \
  GDV_DEV gdv_##T timestampaddYear_int64_##T(gdv_int64 c, gdv_##T v) {                            \
    return gdv_add_months_ms(v, c * 12);                                                          \
  }                                                                                               \
  GDV_DEV gdv_##T date_add_##T##_int64(gdv_##T v, gdv_int64 c) { return v + c * GDV_MILLIS_IN_DAY; } \
  GDV_DEV gdv_##T date_sub_##T##_int64(gdv_##T v, gdv_int64 c) { return v - c * GDV_MILLIS_IN_DAY; } \
  GDV_DEV gdv_##T date_add_##T##_int32(gdv_##T v, gdv_int32 c) { return v + c * GDV_MILLIS_IN_DAY; } \
  GDV_DEV gdv_##T date_sub_##T##_int32(gdv_##T v, gdv_int32 c) { return v - c * GDV_MILLIS_IN_DAY; }
GDV_TSADD(date64)
GDV_TSADD(timestamp)

// Differences.  timestampdiff<Unit>(start, end) = whole units from start to end, truncated
// toward zero; datediff(end, start) = calendar days (Hive semantics).
#define GDV_TSDIFF(T)                                                                             \
  GDV_DEV gdv_int32 timestampdiffSecond_##T##_##T(gdv_##T s, gdv_##T e) {                         \
    return (gdv_int32)((e - s) / 1000LL);                                                         \
  }                                                                                               \
  GDV_DEV gdv_int32 timestampdiffMinute_##T##_##T(gdv_##T s, gdv_##T e) {                         \
    return (gdv_int32)((e - s) / 60000LL);                                                        \
  }                                                                                               \
  GDV_DEV gdv_int32 timestampdiffHour_##T##_##T(gdv_##T s, gdv_##T e) {                           \
    return (gdv_int32)((e - s) / 3600000LL);                                                      \
  }                                                                                               \
  GDV_DEV gdv_int32 timestampdiffDay_##T##_##T(gdv_##T s, gdv_##T e) {                            \
    return (gdv_int32)((e - s) / GDV_MILLIS_IN_DAY);                                              \
  }                                                                                               \
  GDV_DEV gdv_int32 timestampdiffWeek_##T##_##T(gdv_##T s, gdv_##T e) {                           \
    return (gdv_int32)((e - s) / (7 * GDV_MILLIS_IN_DAY));                                        \
  }                                                                                               \
  GDV_DEV gdv_int32 datediff_##T##_##T(gdv_##T e, gdv_##T s) {                                    \
    return (gdv_int32)(gdv_floor_div(e, GDV_MILLIS_IN_DAY) - gdv_floor_div(s, GDV_MILLIS_IN_DAY)); \
  }
GDV_TSDIFF(date64)
GDV_TSDIFF(timestamp)
// timestampdiffMonth / Quarter / Year(start, end): whole calendar months from start to end,
// counted on (start, end) swapped into ascending order and negated afterwards.  The last month
// counts when the end's day of month has reached the start's — or the end IS the last day of its
// month (Jan 31 -> Feb 28 is one month) — and, on the same day of month, when the end's time of
// day (whole seconds) has reached the start's.  The count is exact in 64 bits (instants 2^31 months apart are about
// 179 million years apart, and int64 milliseconds reach +-292 million): Quarter and Year divide the exact count and
// only then narrow to the int32 the signature returns, so a result that fits is right even where the months do not.
GDV_DEV gdv_int64 gdv_months_between(gdv_int64 s, gdv_int64 e) {
  const bool fwd = e > s;
  if (!fwd) { const gdv_int64 t = s; s = e; e = t; }
  const gdv_int64 sday = gdv_floor_div(s, GDV_MILLIS_IN_DAY), eday = gdv_floor_div(e, GDV_MILLIS_IN_DAY);
  const gdv_ymd a = gdv_civil_from_days(sday), b = gdv_civil_from_days(eday);
  gdv_int64 m = 12 * (b.y - a.y) + (b.m - a.m);
  if (b.d < a.d) {
    m -= b.d == gdv_last_day_of_month(b.y, b.m) ? 0 : 1;
  } else if (b.d == a.d) {
    m -= gdv_floor_mod(e, GDV_MILLIS_IN_DAY) / 1000 >= gdv_floor_mod(s, GDV_MILLIS_IN_DAY) / 1000 ? 0 : 1;
  }
  return fwd ? m : -m;
}
#define GDV_TSDIFF_MONTHS(T)                                                                      \
  GDV_DEV gdv_int32 timestampdiffMonth_##T##_##T(gdv_##T s, gdv_##T e) { return (gdv_int32)gdv_months_between(s, e); } \
  GDV_DEV gdv_int32 timestampdiffQuarter_##T##_##T(gdv_##T s, gdv_##T e) {                        \
    return (gdv_int32)(gdv_months_between(s, e) / 3);                                             \
  }                                                                                               \
  GDV_DEV gdv_int32 timestampdiffYear_##T##_##T(gdv_##T s, gdv_##T e) {                           \
    return (gdv_int32)(gdv_months_between(s, e) / 12);                                            \
  }
GDV_TSDIFF_MONTHS(date64)
GDV_TSDIFF_MONTHS(timestamp)
GDV_DEV gdv_int32 datediff_date32_date32(gdv_date32 e, gdv_date32 s) {
  return (gdv_int32)((gdv_uint32)e - (gdv_uint32)s);
}
GDV_DEV gdv_date64 castDATE_date32(gdv_date32 d) { return (gdv_int64)d * GDV_MILLIS_IN_DAY; }
GDV_DEV gdv_date32 castDATE32_date64(gdv_date64 d) {
  return (gdv_date32)gdv_floor_div(d, GDV_MILLIS_IN_DAY);
}
GDV_DEV gdv_date64 castDATE_timestamp(gdv_timestamp t) {
  return gdv_floor_div(t, GDV_MILLIS_IN_DAY) * GDV_MILLIS_IN_DAY;
}

// The calendar tail: months_between, next_day, add_months (date_trunc('unit', t), next_day(t, 'name') and the extractor
// names year, month, day ... are rewritten or aliased onto functions above: gdv_node.h, gdv_registry.cc).  None raises.
// months_between(end, start) -> float64 [Hive's rule, as recalled; NOT rounded to 8 digits: decided]: the month count of
// the two civil dates; a whole number when the days of month agree or both are the last of their months (the times of
// day are ignored then), else plus the difference of the days of month and of the times of day in 31-day months.
// Every step is ONE IEEE double operation in the order written (the kernels are compiled with -ffp-contract=off).  The
// month count stays below 2^33 on all of int64 milliseconds.
GDV_DEV gdv_float64 gdv_months_between_f64(gdv_int64 e, gdv_int64 s) {
  const gdv_ymd a = gdv_civil_from_days(gdv_floor_div(e, GDV_MILLIS_IN_DAY)), b = gdv_civil_from_days(gdv_floor_div(s, GDV_MILLIS_IN_DAY));
  const gdv_int64 n = (a.y - b.y) * 12 + (a.m - b.m);
  if (a.d == b.d || (a.d == gdv_last_day_of_month(a.y, a.m) && b.d == gdv_last_day_of_month(b.y, b.m))) return (gdv_float64)n;
  const gdv_int64 te = gdv_floor_mod(e, GDV_MILLIS_IN_DAY), ts = gdv_floor_mod(s, GDV_MILLIS_IN_DAY);
  return (gdv_float64)n + ((gdv_float64)(a.d - b.d) + (gdv_float64)(te - ts) / 86400000.0) / 31.0;
}
// next_day(t, dow) -> date64: midnight of the first day strictly after t's day whose weekday is dow, in extractDow's
// numbering (1 = Sunday ... 7 = Saturday); a dow outside 1..7 is reduced by the floored modulus (widened first:
// INT32_MIN - 1 does not fit).  The product is taken modulo 2^64: within 7 days of INT64_MAX the exact result leaves int64.
GDV_DEV gdv_date64 gdv_next_day(gdv_int64 v, gdv_int32 dow) {
  const gdv_int64 day = gdv_floor_div(v, GDV_MILLIS_IN_DAY);
  const gdv_int64 want = gdv_floor_mod((gdv_int64)dow - 1, 7) + 1, cur = gdv_floor_mod(day + 4, 7) + 1;
  const gdv_int64 delta = gdv_floor_mod(want - cur, 7);
  return (gdv_int64)((gdv_uint64)(day + (delta == 0 ? 7 : delta)) * (gdv_uint64)GDV_MILLIS_IN_DAY);
}
// add_months(t, n) = timestampaddMonth(n, t), the count second
#define GDV_CALENDAR_TAIL(T)                                                                                              \
  GDV_DEV gdv_float64 months_between_##T##_##T(gdv_##T e, gdv_##T s) { return gdv_months_between_f64(e, s); }             \
  GDV_DEV gdv_date64 next_day_##T##_int32(gdv_##T v, gdv_int32 dow) { return gdv_next_day(v, dow); }                      \
  GDV_DEV gdv_##T add_months_##T##_int32(gdv_##T v, gdv_int32 n) { return timestampaddMonth_int64_##T((gdv_int64)n, v); } \
  GDV_DEV gdv_##T add_months_##T##_int64(gdv_##T v, gdv_int64 n) { return timestampaddMonth_int64_##T(n, v); }
GDV_CALENDAR_TAIL(date64)
GDV_CALENDAR_TAIL(timestamp)

// ------------------------------------------------------------------ decimal128
// Arrow decimal128 = 128-bit two's complement integer + (precision, scale) in the type.
// Precision and scale of the operands and of the result are PLAN constants: the planner passes
// them as literals, every call is inlined, and the branches below fold away, leaving for the
// common case (no down-scaling, e.g. dec(15,2) * dec(15,2) -> dec(31,4)) a bare 128-bit
// multiply or add.  Result-type rules: DecimalResultType in gdv_registry.cc.  When the rules
// had to cut the scale (precision capped at 38) the exact result is divided by 10^delta and
// rounded half away from zero.  A result that does not fit 38 digits yields 0.
GDV_DEV gdv_int128 gdv_pow10_128(int e) {
  gdv_int128 r = 1;
  for (int i = 0; i < e; i++) r *= 10;
  return r;
}
GDV_DEV gdv_int128 gdv_dec_max38() { return gdv_pow10_128(38) - 1; }
GDV_DEV gdv_int128 gdv_dec_clip38(gdv_int128 v) {
  const gdv_int128 m = gdv_dec_max38();
  return (v > m || v < -m) ? (gdv_int128)0 : v;
}
// v / 10^e rounded half away from zero
GDV_DEV gdv_int128 gdv_dec_reduce(gdv_int128 v, int e) {
  if (e <= 0) return v;
  const gdv_int128 d = gdv_pow10_128(e);
  gdv_int128 q = v / d, r = v % d;
  if (r < 0) r = -r;
  if (r >= d - r) q += (v < 0) ? -1 : 1;  // 2r >= d without forming 2r (d can be 10^38)
  return q;
}

struct gdv_u256 { gdv_uint64 w[4]; };  // little-endian limbs
GDV_DEV gdv_u256 gdv_mul_128x128(gdv_uint128 a, gdv_uint128 b) {
  const gdv_uint64 a0 = (gdv_uint64)a, a1 = (gdv_uint64)(a >> 64);
  const gdv_uint64 b0 = (gdv_uint64)b, b1 = (gdv_uint64)(b >> 64);
  const gdv_uint128 p00 = (gdv_uint128)a0 * b0, p01 = (gdv_uint128)a0 * b1;
  const gdv_uint128 p10 = (gdv_uint128)a1 * b0, p11 = (gdv_uint128)a1 * b1;
  gdv_u256 r;
  r.w[0] = (gdv_uint64)p00;
  gdv_uint128 mid = (p00 >> 64) + (gdv_uint64)p01 + (gdv_uint64)p10;
  r.w[1] = (gdv_uint64)mid;
  gdv_uint128 hi = (mid >> 64) + (p01 >> 64) + (p10 >> 64) + (gdv_uint64)p11;
  r.w[2] = (gdv_uint64)hi;
  r.w[3] = (gdv_uint64)((hi >> 64) + (p11 >> 64));
  return r;
}
GDV_DEV gdv_u256 gdv_mul_128x64(gdv_uint128 a, gdv_uint64 b) {
  const gdv_uint128 p0 = (gdv_uint128)(gdv_uint64)a * b, p1 = (gdv_uint128)(gdv_uint64)(a >> 64) * b;
  gdv_u256 r;
  r.w[0] = (gdv_uint64)p0;
  const gdv_uint128 mid = (p0 >> 64) + (gdv_uint64)p1;
  r.w[1] = (gdv_uint64)mid;
  r.w[2] = (gdv_uint64)((mid >> 64) + (p1 >> 64));
  r.w[3] = 0;
  return r;
}
// in-place divide by a 64-bit divisor, returns the remainder
GDV_DEV gdv_uint64 gdv_divmod_u256_u64(gdv_u256& v, gdv_uint64 d) {
  gdv_uint128 rem = 0;
  for (int i = 3; i >= 0; i--) {
    gdv_uint128 cur = (rem << 64) | v.w[i];
    v.w[i] = (gdv_uint64)(cur / d);
    rem = cur % d;
  }
  return (gdv_uint64)rem;
}

// p /= 10^delta, rounded half away from zero, in chunks of <= 10^18 (least significant digits
// first).  The last chunk removed holds the most significant removed digits and alone decides
// the rounding: 2*R >= 10^delta  <=>  2*last_rem >= last_div  (last_div is even, so lower
// chunks can neither create nor break the tie).
GDV_DEV void gdv_u256_div_pow10_round(gdv_u256& p, int delta) {
  gdv_uint64 last_rem = 0, last_div = 1;
  int left = delta;
  while (left > 0) {
    const int step = left > 18 ? 18 : left;
    gdv_uint64 d = 1;
    for (int i = 0; i < step; i++) d *= 10;
    last_rem = gdv_divmod_u256_u64(p, d);
    last_div = d;
    left -= step;
  }
  if (delta > 0 && 2 * (gdv_uint128)last_rem >= (gdv_uint128)last_div) {
    for (int i = 0; i < 4; i++) { if (++p.w[i] != 0) break; }
  }
}

GDV_DEV gdv_int128 gdv_dec_rescale_up(gdv_int128 v, int by) { return by > 0 ? v * gdv_pow10_128(by) : v; }

GDV_DEV gdv_int128 gdv_dec_add_large(gdv_int128 x, int xs, gdv_int128 y, int ys, int os);
GDV_DEV gdv_int128 add_decimal128_decimal128(gdv_int128 x, int xp, int xs, gdv_int128 y, int yp, int ys,
                                             int op, int os) {
  const int hs = xs > ys ? xs : ys;  // exact result scale
  // Digits the operands can have once aligned to that scale — a compile-time fact.  Up to 37
  // the aligned values and their sum fit 128 bits; beyond, the sum is formed in 256 bits.
  const int xd = xp + hs - xs, yd = yp + hs - ys;
  if ((xd > yd ? xd : yd) > 37) return gdv_dec_add_large(x, xs, y, ys, os);
  gdv_int128 sum = gdv_dec_rescale_up(x, hs - xs) + gdv_dec_rescale_up(y, hs - ys);
  return gdv_dec_clip38(gdv_dec_reduce(sum, hs - os));
}
GDV_DEV gdv_int128 subtract_decimal128_decimal128(gdv_int128 x, int xp, int xs, gdv_int128 y, int yp,
                                                  int ys, int op, int os) {
  return add_decimal128_decimal128(x, xp, xs, -y, yp, ys, op, os);
}
GDV_DEV gdv_int128 multiply_decimal128_decimal128(gdv_int128 x, int xp, int xs, gdv_int128 y, int yp,
                                                  int ys, int op, int os) {
  const int delta = xs + ys - os;  // digits the result-type rule cut from the scale
  // Everything below is decided from the operand PRECISIONS, i.e. at compile time (they are
  // literals in the generated kernel): no per-row branch is added.
  if (xp + yp <= 38 && delta == 0) {  // cannot overflow 38 digits
    // <= 18 digits fits int64 by type: one signed 64x64->128 multiply instead of 128x128
    if (xp <= 18 && yp <= 18) return (gdv_int128)(gdv_int64)x * (gdv_int128)(gdv_int64)y;
    return x * y;
  }
  const bool neg = (x < 0) != (y < 0);
  const gdv_uint128 ax = x < 0 ? (gdv_uint128)(-x) : (gdv_uint128)x;
  const gdv_uint128 ay = y < 0 ? (gdv_uint128)(-y) : (gdv_uint128)y;
  // a factor of <= 18 digits has a zero high word: half of the partial products vanish
  gdv_u256 p = yp <= 18   ? gdv_mul_128x64(ax, (gdv_uint64)ay)
               : xp <= 18 ? gdv_mul_128x64(ay, (gdv_uint64)ax)
                          : gdv_mul_128x128(ax, ay);
  gdv_u256_div_pow10_round(p, delta);
  if (p.w[3] != 0 || p.w[2] != 0) return 0;  // overflow
  gdv_uint128 mag = ((gdv_uint128)p.w[1] << 64) | p.w[0];
  if (mag > (gdv_uint128)gdv_dec_max38()) return 0;
  return neg ? -(gdv_int128)mag : (gdv_int128)mag;
}

// ---- 256-bit helpers for divide / mod: binary long division (256 shift-subtract steps).
// Decimal division is expected to be slow; it is exact.
GDV_DEV int gdv_u256_cmp(const gdv_u256& a, const gdv_u256& b) {
  for (int i = 3; i >= 0; i--)
    if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
  return 0;
}
GDV_DEV void gdv_u256_sub(gdv_u256& a, const gdv_u256& b) {  // a -= b (a >= b)
  gdv_uint64 borrow = 0;
  for (int i = 0; i < 4; i++) {
    const gdv_uint128 d = (gdv_uint128)a.w[i] - b.w[i] - borrow;
    a.w[i] = (gdv_uint64)d;
    borrow = (gdv_uint64)(d >> 64) & 1;
  }
}
GDV_DEV void gdv_u256_shl1(gdv_u256& a, gdv_uint64 in_bit) {
  for (int i = 3; i > 0; i--) a.w[i] = (a.w[i] << 1) | (a.w[i - 1] >> 63);
  a.w[0] = (a.w[0] << 1) | in_bit;
}
GDV_DEV bool gdv_u256_is_zero(const gdv_u256& a) { return (a.w[0] | a.w[1] | a.w[2] | a.w[3]) == 0; }
GDV_DEV void gdv_u256_divmod(const gdv_u256& num, const gdv_u256& den, gdv_u256* q, gdv_u256* r) {
  gdv_u256 quo = {{0, 0, 0, 0}}, rem = {{0, 0, 0, 0}};
  for (int bit = 255; bit >= 0; bit--) {
    gdv_u256_shl1(rem, (num.w[bit >> 6] >> (bit & 63)) & 1ull);
    gdv_u256_shl1(quo, 0);
    if (gdv_u256_cmp(rem, den) >= 0) {
      gdv_u256_sub(rem, den);
      quo.w[0] |= 1ull;
    }
  }
  *q = quo;
  *r = rem;
}
GDV_DEV gdv_u256 gdv_u256_from_u128(gdv_uint128 v) {
  gdv_u256 r = {{(gdv_uint64)v, (gdv_uint64)(v >> 64), 0, 0}};
  return r;
}
GDV_DEV gdv_int128 gdv_dec_from_mag(const gdv_u256& mag, bool neg) {  // 0 when it needs > 38 digits
  if (mag.w[3] != 0 || mag.w[2] != 0) return 0;
  const gdv_uint128 m = ((gdv_uint128)mag.w[1] << 64) | mag.w[0];
  if (m > (gdv_uint128)gdv_dec_max38()) return 0;
  return neg ? -(gdv_int128)m : (gdv_int128)m;
}
// x + y when the aligned operands can exceed 37 digits: signed-magnitude sum in 256 bits,
// then the scale reduction (round half away from zero) and the 38-digit check
GDV_DEV void gdv_u256_add(gdv_u256& a, const gdv_u256& b) {
  gdv_uint64 carry = 0;
  for (int i = 0; i < 4; i++) {
    const gdv_uint128 t = (gdv_uint128)a.w[i] + b.w[i] + carry;
    a.w[i] = (gdv_uint64)t;
    carry = (gdv_uint64)(t >> 64);
  }
}
GDV_DEV gdv_int128 gdv_dec_add_large(gdv_int128 x, int xs, gdv_int128 y, int ys, int os) {
  const int hs = xs > ys ? xs : ys;
  const bool xneg = x < 0, yneg = y < 0;
  const gdv_u256 X = gdv_mul_128x128(xneg ? (gdv_uint128)(-x) : (gdv_uint128)x, (gdv_uint128)gdv_pow10_128(hs - xs));
  const gdv_u256 Y = gdv_mul_128x128(yneg ? (gdv_uint128)(-y) : (gdv_uint128)y, (gdv_uint128)gdv_pow10_128(hs - ys));
  gdv_u256 sum;
  bool neg;
  if (xneg == yneg) { sum = X; gdv_u256_add(sum, Y); neg = xneg; }
  else if (gdv_u256_cmp(X, Y) >= 0) { sum = X; gdv_u256_sub(sum, Y); neg = xneg; }
  else { sum = Y; gdv_u256_sub(sum, X); neg = yneg; }
  gdv_u256_div_pow10_round(sum, hs - os);
  return gdv_dec_from_mag(sum, neg);
}
// x / y at the result scale `os`: round_half_away(x * 10^(os - xs + ys) / y).  y == 0 raises.
GDV_DEV gdv_int128 divide_decimal128_decimal128(gdv_ctx ctx, gdv_int128 x, int xp, int xs, gdv_int128 y,
                                                int yp, int ys, int op, int os) {
  if (y == 0) { gdv_raise(ctx, GDV_ERR_DIV_ZERO); return 0; }
  const int delta = os - xs + ys;  // >= 0 for every result type the rules produce
  const bool neg = (x < 0) != (y < 0);
  const gdv_uint128 ax = x < 0 ? (gdv_uint128)(-x) : (gdv_uint128)x;
  const gdv_uint128 ay = y < 0 ? (gdv_uint128)(-y) : (gdv_uint128)y;
  // numerator = |x| * 10^delta; delta can exceed 38 (e.g. dec(38,0) / dec(38,37)), so the
  // power of ten is applied in two steps and a numerator that leaves 256 bits means a
  // quotient of more than 38 digits: overflow -> 0
  const int d1 = delta > 38 ? 38 : (delta > 0 ? delta : 0);
  gdv_u256 num = gdv_mul_128x128(ax, (gdv_uint128)gdv_pow10_128(d1));
  for (int left = delta - d1; left > 0; left -= 18) {
    gdv_uint64 m = 1;
    for (int i = 0; i < (left > 18 ? 18 : left); i++) m *= 10;
    gdv_uint64 carry = 0;
    for (int i = 0; i < 4; i++) {
      const gdv_uint128 t = (gdv_uint128)num.w[i] * m + carry;
      num.w[i] = (gdv_uint64)t;
      carry = (gdv_uint64)(t >> 64);
    }
    if (carry != 0) return 0;
  }
  gdv_u256 den = gdv_u256_from_u128(ay), q, r;
  gdv_u256_divmod(num, den, &q, &r);
  gdv_u256_shl1(r, 0);                       // 2 * remainder (den < 2^127, no overflow)
  if (gdv_u256_cmp(r, den) >= 0) { for (int i = 0; i < 4; i++) if (++q.w[i] != 0) break; }
  return gdv_dec_from_mag(q, neg);
}
// x mod y at scale max(xs, ys), sign of the dividend.  y == 0 raises.
GDV_DEV gdv_int128 mod_decimal128_decimal128(gdv_ctx ctx, gdv_int128 x, int xp, int xs, gdv_int128 y,
                                             int yp, int ys, int op, int os) {
  if (y == 0) { gdv_raise(ctx, GDV_ERR_DIV_ZERO); return 0; }
  const gdv_uint128 ax = x < 0 ? (gdv_uint128)(-x) : (gdv_uint128)x;
  const gdv_uint128 ay = y < 0 ? (gdv_uint128)(-y) : (gdv_uint128)y;
  gdv_u256 a = gdv_mul_128x128(ax, (gdv_uint128)gdv_pow10_128(ys > xs ? ys - xs : 0));
  gdv_u256 b = gdv_mul_128x128(ay, (gdv_uint128)gdv_pow10_128(xs > ys ? xs - ys : 0));
  gdv_u256 q, r;
  gdv_u256_divmod(a, b, &q, &r);
  return gdv_dec_from_mag(r, x < 0);
}

// comparisons bring both sides to the larger scale (exact: |v| < 10^38 and the scale
// difference keeps 10^38 * 10^diff inside 256 bits only for small diffs, so compare via
// 256-bit products when the rescale could overflow 128 bits)
GDV_DEV int gdv_dec_compare(gdv_int128 x, int xp, int xs, gdv_int128 y, int yp, int ys) {
  if (xs == ys) return x < y ? -1 : (x > y ? 1 : 0);
  const bool xneg = x < 0, yneg = y < 0;
  if (xneg != yneg) return xneg ? -1 : 1;
  const gdv_uint128 ax = xneg ? (gdv_uint128)(-x) : (gdv_uint128)x;
  const gdv_uint128 ay = yneg ? (gdv_uint128)(-y) : (gdv_uint128)y;
  gdv_u256 a = gdv_mul_128x128(ax, (gdv_uint128)gdv_pow10_128(ys > xs ? ys - xs : 0));
  gdv_u256 b = gdv_mul_128x128(ay, (gdv_uint128)gdv_pow10_128(xs > ys ? xs - ys : 0));
  int c = 0;
  for (int i = 3; i >= 0 && c == 0; i--) c = a.w[i] < b.w[i] ? -1 : (a.w[i] > b.w[i] ? 1 : 0);
  return xneg ? -c : c;
}
#define GDV_DEC_REL(name, expr)                                                                    \
  GDV_DEV bool name##_decimal128_decimal128(gdv_int128 x, int xp, int xs, gdv_int128 y, int yp,   \
                                            int ys, int op, int os) {                              \
    const int c = gdv_dec_compare(x, xp, xs, y, yp, ys);                                           \
    return expr;                                                                                   \
  }
GDV_DEC_REL(equal, c == 0)
GDV_DEC_REL(not_equal, c != 0)
GDV_DEC_REL(less_than, c < 0)
GDV_DEC_REL(less_than_or_equal_to, c <= 0)
GDV_DEC_REL(greater_than, c > 0)
GDV_DEC_REL(greater_than_or_equal_to, c >= 0)

GDV_DEV gdv_int128 negative_decimal128(gdv_int128 x, int xp, int xs, int op, int os) { return -x; }
GDV_DEV gdv_int128 abs_decimal128(gdv_int128 x, int xp, int xs, int op, int os) { return x < 0 ? -x : x; }
// int64 -> decimal(op, os): value * 10^os (0 on overflow of the declared precision)
GDV_DEV gdv_int128 castDECIMAL_int64(gdv_int64 v, int op, int os) {
  // |v| must stay below 10^(op - os); checked BEFORE scaling so the product cannot wrap
  if (v == 0) return 0;
  if (op - os <= 0) return 0;
  const gdv_int128 lim = gdv_pow10_128(op - os);
  if ((gdv_int128)v >= lim || (gdv_int128)v <= -lim) return 0;
  return (gdv_int128)v * gdv_pow10_128(os);
}
GDV_DEV gdv_int128 castDECIMAL_int32(gdv_int32 v, int op, int os) { return castDECIMAL_int64(v, op, os); }
// decimal -> decimal with another (precision, scale): rescale, round half away from zero
GDV_DEV gdv_int128 castDECIMAL_decimal128(gdv_int128 x, int xp, int xs, int op, int os) {
  if (os >= xs) {  // scale up: |x| must stay below 10^(op - (os - xs)), checked before scaling
    const int by = os - xs;
    if (x == 0) return 0;
    if (op - by <= 0) return 0;
    const gdv_int128 lim_in = gdv_pow10_128(op - by);
    if (x >= lim_in || x <= -lim_in) return 0;
    return x * gdv_pow10_128(by);
  }
  const gdv_int128 r = gdv_dec_reduce(x, xs - os);
  const gdv_int128 lim = gdv_pow10_128(op);
  return (r >= lim || r <= -lim) ? (gdv_int128)0 : r;
}
// ---- round / truncate / ceil / floor over decimal128 (round 5) [recalled: precompiled/decimal_ops.cc Round / Truncate /
// Ceil / Floor: the value is brought to `k` fractional digits (k < 0: to a multiple of 10^-k) — half away from zero,
// towards zero, up, down — and then expressed in the (precision, scale) the EXPRESSION declares, which is the caller's
// to choose as in the lineage; a result that does not fit that precision is 0, like every decimal overflow here].
// mode: 0 half away from zero, 1 towards zero, 2 towards +inf, 3 towards -inf.
GDV_DEV gdv_int128 gdv_dec_round_to(gdv_int128 x, int xs, gdv_int32 k, int mode, int op, int os) {
  if (k > xs) k = xs;
  if (k < -38) return 0;  // every representable value is nearer to 0 than to 10^39
  const int drop = xs - (int)k;  // digits that go
  gdv_int128 r = x;
  if (drop > 0) {
    if (drop > 38) {
      r = 0;
      if (mode == 2 && x > 0) r = 1;
      if (mode == 3 && x < 0) r = -1;
    } else {
      const gdv_int128 d = gdv_pow10_128(drop);
      gdv_int128 q = x / d, m = x % d;  // C division: towards zero
      if (mode == 0) {
        const gdv_int128 a = m < 0 ? -m : m;
        if (a >= d - a) q += x < 0 ? -1 : 1;
      } else if (mode == 2) {
        if (m > 0) q += 1;
      } else if (mode == 3) {
        if (m < 0) q -= 1;
      }
      r = q;
    }
  }
  // r counts units of 10^-k (k >= 0: at scale k; k < 0: multiples of 10^-k, i.e. scale 0 after multiplying back)
  const int have = drop > 0 ? (int)k : xs;  // the scale r is expressed at (may be negative)
  return castDECIMAL_decimal128(have < 0 ? r * gdv_pow10_128(-have > 38 ? 38 : -have) : r, 38, have < 0 ? 0 : have, op, os);
}
GDV_DEV gdv_int128 round_decimal128(gdv_int128 x, int xp, int xs, int op, int os) { return gdv_dec_round_to(x, xs, 0, 0, op, os); }
GDV_DEV gdv_int128 round_decimal128_int32(gdv_int128 x, int xp, int xs, gdv_int32 k, int op, int os) { return gdv_dec_round_to(x, xs, k, 0, op, os); }
GDV_DEV gdv_int128 truncate_decimal128(gdv_int128 x, int xp, int xs, int op, int os) { return gdv_dec_round_to(x, xs, 0, 1, op, os); }
GDV_DEV gdv_int128 truncate_decimal128_int32(gdv_int128 x, int xp, int xs, gdv_int32 k, int op, int os) { return gdv_dec_round_to(x, xs, k, 1, op, os); }
GDV_DEV gdv_int128 ceil_decimal128(gdv_int128 x, int xp, int xs, int op, int os) { return gdv_dec_round_to(x, xs, 0, 2, op, os); }
GDV_DEV gdv_int128 floor_decimal128(gdv_int128 x, int xp, int xs, int op, int os) { return gdv_dec_round_to(x, xs, 0, 3, op, os); }
// the double nearest to a 128-bit magnitude, ties to even, rounded ONCE: below 2^64 the conversion of the uint64 is that;
// above, the top 64 significant bits are kept, every bit shifted out is ORed into the lowest one (it lies ten places
// below the rounding position, so it can only break a tie, never make one) and the exact power of two is multiplied back
GDV_DEV gdv_float64 gdv_u128_to_f64(gdv_uint128 mag) {
  gdv_uint64 h = (gdv_uint64)(mag >> 64);
  if (h == 0) return (gdv_float64)(gdv_uint64)mag;
  int sh = 1;  // the bit length of the high word
  gdv_float64 two_sh = 2.0;
  if (h >> 32) { h >>= 32; sh += 32; two_sh *= 4294967296.0; }
  if (h >> 16) { h >>= 16; sh += 16; two_sh *= 65536.0; }
  if (h >> 8) { h >>= 8; sh += 8; two_sh *= 256.0; }
  if (h >> 4) { h >>= 4; sh += 4; two_sh *= 16.0; }
  if (h >> 2) { h >>= 2; sh += 2; two_sh *= 4.0; }
  if (h >> 1) { sh += 1; two_sh *= 2.0; }
  const gdv_uint64 top = (gdv_uint64)(mag >> sh);
  const gdv_uint64 sticky = (mag & (((gdv_uint128)1 << sh) - 1)) != 0 ? 1ull : 0ull;
  return (gdv_float64)(top | sticky) * two_sh;
}
GDV_DEV gdv_float64 castFLOAT8_decimal128(gdv_int128 x, int xp, int xs, int op, int os) {
  // two correctly rounded steps: int128 -> the nearest double, then one division by p, where p is 1.0 multiplied by 10.0
  // `xs` times (exactly 10^xs up to xs = 22; beyond, p itself carries the rounding of those multiplications)
  gdv_float64 p = 1.0;
  for (int i = 0; i < xs; i++) p *= 10.0;
  const gdv_uint128 mag = x < 0 ? (gdv_uint128)(-x) : (gdv_uint128)x;
  const gdv_float64 m = gdv_u128_to_f64(mag);
  return (x < 0 ? -m : m) / p;
}
GDV_DEV gdv_int64 castBIGINT_decimal128(gdv_int128 x, int xp, int xs, int op, int os) {
  return (gdv_int64)gdv_dec_reduce(x, xs);
}
// ---- decimal tail: casts from floats, the cast that answers NULL on overflow, nvl / greatest / least and the null-safe
// comparisons.  (castDECIMAL of text sits next to castBIGINT_utf8, the hashes behind GDV_HASH_BUF.)
// the double nearest to 10^k, k in [0, 38]: the literals, so host and device compilers agree on every one
GDV_DEV gdv_float64 gdv_dec_pow10_f64(int k) {
  const gdv_float64 t[39] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11, 1e12,
                             1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22, 1e23, 1e24, 1e25,
                             1e26, 1e27, 1e28, 1e29, 1e30, 1e31, 1e32, 1e33, 1e34, 1e35, 1e36, 1e37, 1e38};
  return t[k < 0 ? 0 : (k > 38 ? 38 : k)];
}
// float64 -> decimal(op, os) [recalled: the lineage's FromDouble]: u = x * 10^os in ONE IEEE multiplication, rounded to an
// integer half away from zero; NaN or |r| >= 10^op: 0, like every decimal overflow here.  The integer-valued double is split
// into two 64-bit halves (exact: it has at most 53 significant bits), never cast to a 64-bit integer as a whole.
GDV_DEV gdv_int128 castDECIMAL_float64(gdv_float64 x, int op, int os) {
  const gdv_float64 u = x * gdv_dec_pow10_f64(os);
  if (u != u) return 0;
  gdv_float64 t = trunc(u);
  if (fabs(u - t) >= 0.5) t += u < 0 ? -1.0 : 1.0;  // (|u| + 0.5 would round 0.49999999999999994 up)
  const gdv_float64 a = fabs(t);
  if (!(a < 170141183460469231731687303715884105728.0)) return 0;  // 2^127 > 10^38; +-inf ends here
  const gdv_uint64 hi = (gdv_uint64)(a * 5.421010862427522170037264004349708557128906250e-20);  // a / 2^64, truncated
  const gdv_uint64 lo = (gdv_uint64)(a - (gdv_float64)hi * 18446744073709551616.0);
  const gdv_uint128 mag = ((gdv_uint128)hi << 64) | lo;
  if (mag >= (gdv_uint128)gdv_pow10_128(op)) return 0;
  return t < 0 ? -(gdv_int128)mag : (gdv_int128)mag;
}
GDV_DEV gdv_int128 castDECIMAL_float32(gdv_float32 x, int op, int os) { return castDECIMAL_float64((gdv_float64)x, op, os); }
// castDECIMAL_decimal128 with NULL instead of 0 where the value does not fit the declared precision (0 is a value)
GDV_DEV gdv_int128 castDECIMALNullOnOverflow_decimal128(gdv_int128 x, int xp, int xs, bool xv, int op, int os, bool* out_valid) {
  *out_valid = false;
  if (!xv) return 0;
  gdv_int128 r;
  if (os >= xs) {
    const int by = os - xs;
    if (x != 0) {
      if (op - by <= 0) return 0;
      const gdv_int128 lim_in = gdv_pow10_128(op - by);
      if (x >= lim_in || x <= -lim_in) return 0;
    }
    r = x * gdv_pow10_128(by);
  } else {
    r = gdv_dec_reduce(x, xs - os);
    const gdv_int128 lim = gdv_pow10_128(op);
    if (r >= lim || r <= -lim) return 0;
  }
  *out_valid = true;
  return r;
}
// nvl / greatest / least: both sides and the result have one (precision, scale) (checked at Make): plain 128-bit integers
GDV_DEV gdv_int128 nvl_decimal128_decimal128(gdv_int128 a, int ap, int asc, bool av, gdv_int128 b, int bp, int bs, bool bv,
                                             int op, int os, bool* out_valid) {
  *out_valid = av || bv;
  return av ? a : b;
}
GDV_DEV gdv_int128 greatest_decimal128_decimal128(gdv_int128 x, int xp, int xs, gdv_int128 y, int yp, int ys, int op, int os) {
  return x > y ? x : y;
}
GDV_DEV gdv_int128 least_decimal128_decimal128(gdv_int128 x, int xp, int xs, gdv_int128 y, int yp, int ys, int op, int os) {
  return x < y ? x : y;
}
// by VALUE over any two (precision, scale): 1.0 and 1 are not distinct (the generic template compares bit images)
GDV_DEV bool is_distinct_from_decimal128_decimal128(gdv_int128 x, int xp, int xs, bool xv, gdv_int128 y, int yp, int ys, bool yv) {
  if (xv != yv) return true;
  if (!xv) return false;
  return gdv_dec_compare(x, xp, xs, y, yp, ys) != 0;
}
GDV_DEV bool is_not_distinct_from_decimal128_decimal128(gdv_int128 x, int xp, int xs, bool xv, gdv_int128 y, int yp, int ys, bool yv) {
  return !is_distinct_from_decimal128_decimal128(x, xp, xs, xv, y, yp, ys, yv);
}

// ------------------------------------------------------------------ utf8 / binary
// A string value inside a kernel is a VIEW: pointer + byte length into an input data buffer
// (or a literal in the plan's constant block) plus a byte map applied on read (0 none, 1 ASCII
// upper, 2 ASCII lower).  substr / trim produce narrower views, upper / lower set the map, so no
// per-row scratch is ever needed; the bytes are materialised exactly once, by the copy stage of
// a var-len output, or consumed in place by predicates (like, equal ...).
//
// Round 2: views carry no register cache any more.  Kernels over var-len columns first SWEEP the
// contiguous byte span of a wave tile with lanes over BYTES (16 B/lane, coalesced): that pass
// answers the tile-wide questions byte-parallel (is every byte ASCII?  where does '%needle%'
// match?) and leaves the lines in L2 / L1 for the per-row functions below.
// Two kinds of value are not plain views (round 2, registry tail): `map & GDV_MAP_REVERSE` — the
// characters of the view in reverse order — and `map & GDV_MAP_DIGITS` — the decimal digits of the
// integer stored in `p`, cut to `len` bytes.  Only the copy stage of a var-len output can read
// them (the planner rejects every other consumer), so the readers below never see these bits.
#define GDV_MAP_CASE 3
#define GDV_MAP_REVERSE 4
#define GDV_MAP_DIGITS 8
#define GDV_MAP_REPLACE 16  // `lim` points at a replace table (constant block), flags >> 2 = source length
#define GDV_MAP_INITCAP 128  // (32 is GDV_MAP_HITS, further down) round 5: the view's bytes with every word's first letter in upper case, the others in lower case
// round 5: lower-case hex text of a message digest; (map >> 8) & 3 = 0 SHA-256, 1 SHA-1, 2 MD5; bit 10 (1024): the message is
// the 8 bytes of `lead`, else the `lead` bytes at `lead_p` (read through the low map bits)
#define GDV_MAP_DIGEST 64
// round 5, arguments that are not literals: GDV_MAP_CYCLE — the `lead` bytes at `p`, repeated cyclically to `len` bytes (the
// fill of lpad / rpad); GDV_MAP_REPLACE_ROW — replace() with per-row from / to: `lim` = from's bytes, `lead_p` = to's,
// lead = text length | from length << 32 | to length << 48, flags >> 8 = from's case map | to's << 2
#define GDV_MAP_CYCLE 2048
#define GDV_MAP_REPLACE_ROW 4096
#define GDV_MAP_SPECIAL (GDV_MAP_REVERSE | GDV_MAP_DIGITS | GDV_MAP_REPLACE | GDV_MAP_INITCAP | GDV_MAP_DIGEST | GDV_MAP_CYCLE | GDV_MAP_REPLACE_ROW)  // only the output copy reads these
// GDV_MAP_DIGITS with GDV_STR_DECIMAL in `flags` (round 4): the text of the decimal128 whose low / high
// words sit in `p` / `lim`, scale = flags >> 8, cut to `len` bytes (castVARCHAR(decimal, n))
#define GDV_STR_DECIMAL 128
#define GDV_STR_ASCII 1  // flags: every byte of the buffer range this view came from is < 0x80
#define GDV_STR_INBUF 2  // flags: 8-byte loads starting anywhere inside the view stay inside its buffer
#define GDV_STR_LEAD 4   // flags: `lead` / `lead_p` are set (exact variant of the wave kernels, rows with bytes >= 0x80)
// (out-of-line device functions fault on this stack — measured, profiles/r02_c5_codesize.txt —
// so cold paths stay inline and the row loop of string kernels is simply not unrolled)
#define GDV_COLD __forceinline__
struct gdv_str {
  const gdv_uint8* p;
  gdv_int32 len;
  gdv_int32 map;
  const gdv_uint8* lim;  // end of the readable buffer p points into (8-byte loads stop here)
  gdv_int32 flags;
  // GDV_STR_LEAD (round 4): bit i of `lead` = the byte lead_p[i] STARTS a character (is not 10xxxxxx),
  // i < 64 — the row's lead-byte mask, taken from the byte sweep's bitmap.  Character counts and
  // positions of any view inside [lead_p, lead_p + 64) are popcount / select on it: no byte of the row is
  // read again (gdv_lead_window).  Untouched (dead) in kernels that never set the flag.
  gdv_uint64 lead;
  const gdv_uint8* lead_p;
};
GDV_DEV gdv_str gdv_make_str(const gdv_uint8* base, gdv_int32 begin, gdv_int32 end,
                             const gdv_uint8* lim, gdv_int32 flags = 0) {
  gdv_str s;
  s.p = base + begin;
  s.len = end - begin;
  s.map = 0;
  s.lim = lim;
  s.flags = flags;
  s.lead = 0;
  s.lead_p = nullptr;
  return s;
}
// the lead-byte mask of view s (bit i: byte i of s starts a character), when the view lies inside the
// 64 bytes its row's mask covers
GDV_DEV bool gdv_lead_window(const gdv_str& s, gdv_uint64* m) {
  if (!(s.flags & GDV_STR_LEAD)) return false;
  const gdv_int64 off = s.p - s.lead_p;
  if (off < 0 || off + s.len > 64 || s.len < 0) return false;
  const gdv_uint64 w = off >= 64 ? 0ull : (s.lead >> off);
  *m = s.len >= 64 ? w : (w & ((1ull << s.len) - 1ull));
  return true;
}
GDV_DEV gdv_uint8 gdv_map_byte(gdv_uint8 c, gdv_int32 map) {
  if (map == 1) return (c >= 'a' && c <= 'z') ? (gdv_uint8)(c - 32) : c;
  if (map == 2) return (c >= 'A' && c <= 'Z') ? (gdv_uint8)(c + 32) : c;
  return c;
}
GDV_DEV gdv_uint8 gdv_str_at(const gdv_str& s, gdv_int32 i) { return gdv_map_byte(s.p[i], s.map); }

// ---- word-at-a-time (SWAR) primitives: strings are processed 8 bytes per step with one
// unaligned 8-byte load instead of 8 dependent byte loads; ASCII case mapping, UTF-8
// continuation-byte counting and substring search all work on the 64-bit word.
#define GDV_B80 0x8080808080808080ull
#define GDV_B7F 0x7f7f7f7f7f7f7f7full
// 8 bytes at p; bytes at or past `lim` read as 0.  In the last 8 bytes of the buffer the load
// is moved back to end exactly at `lim` and shifted (one load, no byte loop).  Precondition
// (the engine and the literal tables guarantee it): at least 8 readable bytes end at `lim`.
GDV_DEV gdv_uint64 gdv_load8(const gdv_uint8* p, const gdv_uint8* lim) {
  gdv_uint64 w;
  if (p + 8 <= lim) {
    __builtin_memcpy(&w, p, 8);
    return w;
  }
  const gdv_int64 over = (gdv_int64)(p - lim) + 8;  // 1.. bytes of [p, p+8) past lim
  __builtin_memcpy(&w, lim - 8, 8);
  return over >= 8 ? 0ull : w >> (8 * over);
}
// the same without the limit check, for loads a wave-uniform test proved in range
GDV_DEV gdv_uint64 gdv_load8_raw(const gdv_uint8* p) {
  gdv_uint64 w;
  __builtin_memcpy(&w, p, 8);
  return w;
}
GDV_DEV gdv_uint64 gdv_low_bytes_mask(gdv_int32 nbytes) {  // nbytes in [0, 8]
  return nbytes >= 8 ? ~0ull : ((1ull << (8 * nbytes)) - 1ull);
}
GDV_DEV gdv_uint64 gdv_map8(gdv_uint64 w, gdv_int32 map) {
  if (map == 0) return w;
  const gdv_uint64 h = w & GDV_B7F;
  const gdv_uint64 ascii = ~w & GDV_B80;
  // top bit of each byte: h >= lo  and  h > hi, computed without cross-byte carries
  const gdv_uint64 lo = map == 1 ? 0x1f1f1f1f1f1f1f1full : 0x3f3f3f3f3f3f3f3full;  // 0x80 - 'a' | 0x80 - 'A'
  const gdv_uint64 hi = map == 1 ? 0x0505050505050505ull : 0x2525252525252525ull;  // 0x7f - 'z' | 0x7f - 'Z'
  const gdv_uint64 in_range = (h + lo) & ~(h + hi) & ascii;
  return w ^ (in_range >> 2);  // toggle bit 5 (0x20) of the letters in range
}
// raw bytes [i, i+8) of the string (bytes past the buffer limit read as 0)
GDV_DEV gdv_uint64 gdv_raw_word_at(const gdv_str& s, gdv_int32 i) {
  // INBUF is wave-uniform (one range test per tile / literal tables are padded): a scalar branch
  if (s.flags & GDV_STR_INBUF) return gdv_load8_raw(s.p + i);
  return gdv_load8(s.p + i, s.lim);
}
// mapped bytes [i, i+8) of the string (bytes past the buffer limit read as 0)
GDV_DEV gdv_uint64 gdv_word_at(const gdv_str& s, gdv_int32 i) {
  return gdv_map8(gdv_raw_word_at(s, i), s.map);
}
// ---- copies of the two non-view kinds (P: pointer into HBM or into the LDS staging window)
GDV_DEV gdv_int32 gdv_utf8_declared_len(gdv_uint8 c) {  // bytes the lead byte announces; 0: not a lead byte
  if (c < 0x80) return 1;
  if ((c & 0xE0) == 0xC0) return 2;
  if ((c & 0xF0) == 0xE0) return 3;
  if ((c & 0xF8) == 0xF0) return 4;
  return 0;
}
template <typename P>
GDV_DEV void gdv_store_low_bytes(P dst, gdv_uint64 w, gdv_int32 r) {  // the low r (0..7) bytes of w
  gdv_int32 i = 0;
  if (r & 4) { const gdv_uint32 v = (gdv_uint32)w; __builtin_memcpy(dst, &v, 4); i = 4; w >>= 32; }
  if (r & 2) { const gdv_uint16 v = (gdv_uint16)w; __builtin_memcpy(dst + i, &v, 2); i += 2; w >>= 16; }
  if (r & 1) dst[i] = (gdv_uint8)w;
}
template <typename P>
GDV_DEV void gdv_copy_reversed(P dst, const gdv_str& s) {
  const gdv_int32 len = s.len, cm = s.map & GDV_MAP_CASE;
  if (s.flags & GDV_STR_ASCII) {
    // output byte i is source byte len-1-i: 8 at a time from the end, byte-swapped
    gdv_int32 i = 0;
    for (; i + 8 <= len; i += 8) {
      const gdv_uint64 w = __builtin_bswap64(gdv_map8(gdv_load8_raw(s.p + (len - i - 8)), cm));
      __builtin_memcpy(dst + i, &w, 8);
    }
    const gdv_int32 r = len - i;  // source bytes [0, r) are left
    if (r > 0) {
      gdv_str head = s;
      head.map = 0;
      gdv_store_low_bytes(dst + i, __builtin_bswap64(gdv_map8(gdv_raw_word_at(head, 0), cm) << (8 * (8 - r))), r);
    }
    return;
  }
  // characters keep their byte order; a character is what its lead byte announces
  for (gdv_int32 i = 0; i < len;) {
    gdv_int32 cl = gdv_utf8_declared_len(s.p[i]);
    if (cl == 0) cl = 1;
    if (cl > len - i) cl = len - i;
    for (gdv_int32 j = 0; j < cl; j++) dst[len - i - cl + j] = gdv_map_byte(s.p[i + j], cm);
    i += cl;
  }
}
GDV_DEV gdv_int32 gdv_count_digits(gdv_uint64 v) {
  gdv_int32 n = 1;
  for (gdv_uint64 p = 10; n < 20 && v >= p; p *= 10) n++;
  return n;
}
// ---- decimal128 -> text, Arrow's Decimal128::ToString(scale) [arrow/util/decimal.cc
// AdjustIntegerStringWithScale, as recalled; pinned against pyarrow's decimal -> string cast in
// tests/test_registry_tail.py]: digits D (no leading zeros, "0" for zero), nd of them,
// adjusted exponent adj = nd - 1 - scale;
//   scale == 0              ->  [-]D
//   adj < -6                ->  [-]d[.ddd]E-x      (x = -adj: the only scientific case for scale >= 0)
//   nd > scale              ->  [-]ddd.ddd         (point scale digits from the right)
//   otherwise               ->  [-]0.000ddd        (scale - nd zeros)
struct gdv_dec_text {
  gdv_uint64 hi, lo;  // |value| = hi * 10^19 + lo
  gdv_int32 nd, scale, neg, len;
};
GDV_DEV gdv_dec_text gdv_dec_text_of(gdv_int128 v, gdv_int32 scale) {
  gdv_dec_text t;
  t.neg = v < 0 ? 1 : 0;
  const gdv_uint128 mag = t.neg ? (gdv_uint128)0 - (gdv_uint128)v : (gdv_uint128)v;
  const gdv_uint64 p19 = 10000000000000000000ull;
  t.hi = (gdv_uint64)(mag / p19);
  t.lo = (gdv_uint64)(mag % p19);
  t.nd = t.hi != 0 ? 19 + gdv_count_digits(t.hi) : gdv_count_digits(t.lo);
  t.scale = scale;
  const gdv_int32 adj = t.nd - 1 - scale;
  if (scale <= 0) t.len = t.neg + t.nd;
  else if (adj < -6) t.len = t.neg + t.nd + (t.nd > 1 ? 1 : 0) + 2 + (-adj >= 10 ? 2 : 1);
  else if (t.nd > scale) t.len = t.neg + t.nd + 1;
  else t.len = t.neg + 2 + scale;
  return t;
}
// the first `len` bytes of the text (len <= t.len), one byte store each (registry tail: not a hot path)
template <typename P>
GDV_DEV void gdv_copy_dec_text(P dst, const gdv_dec_text& t, gdv_int32 len) {
  const gdv_int32 adj = t.nd - 1 - t.scale;
  const bool sci = t.scale > 0 && adj < -6, lead0 = t.scale > 0 && !sci && t.nd <= t.scale;
  const gdv_int32 point = t.scale <= 0 ? -1 : sci ? (t.nd > 1 ? t.neg + 1 : -1) : lead0 ? t.neg + 1 : t.neg + t.nd - t.scale;
  if (t.neg && len > 0) dst[0] = (gdv_uint8)'-';
  if (point >= 0 && point < len) dst[point] = (gdv_uint8)'.';
  gdv_int32 first = t.neg;  // text position of the most significant digit
  if (lead0) {
    if (t.neg < len) dst[t.neg] = (gdv_uint8)'0';
    first = t.neg + 2 + (t.scale - t.nd);
    for (gdv_int32 k = t.neg + 2; k < first && k < len; k++) dst[k] = (gdv_uint8)'0';
  }
  gdv_uint64 chunk = t.lo;
  for (gdv_int32 i = t.nd - 1; i >= 0; i--) {  // least significant digit first
    if (i == t.nd - 20) chunk = t.hi;         // the 19 digits of `lo` are out
    const gdv_uint8 d = (gdv_uint8)('0' + (gdv_int32)(chunk % 10));
    chunk /= 10;
    gdv_int32 pos = first + i;
    if (point >= 0 && !lead0 && pos >= point) pos++;
    if (pos < len) dst[pos] = d;
  }
  if (sci) {
    gdv_int32 at = t.neg + t.nd + (t.nd > 1 ? 1 : 0);
    const gdv_int32 x = -adj;
    if (at < len) dst[at] = (gdv_uint8)'E';
    if (at + 1 < len) dst[at + 1] = (gdv_uint8)'-';
    if (x >= 10) {
      if (at + 2 < len) dst[at + 2] = (gdv_uint8)('0' + x / 10);
      if (at + 3 < len) dst[at + 3] = (gdv_uint8)('0' + x % 10);
    } else if (at + 2 < len) {
      dst[at + 2] = (gdv_uint8)('0' + x);
    }
  }
}
// ---- float32 / float64 -> text (round 5).  castVARCHAR(real, n) keeps the value's SHORTEST round-trip
// decimal digits (gdv_shortest_digits, further down) in the view: `p` = the digits as an integer D
// (no trailing zeros, at most 17), `lim` = nd | (k + 2048) << 8 | neg << 24 | kind << 25 where
// value = 0.D * 10^k and kind = 0 finite non-zero, 1 zero, 2 infinity, 3 NaN.  The text is the
// Java-compatible form of gandiva/formatting_utils.h [as recalled: FloatToStringGdvMixin —
// double-conversion ToShortest with "Infinity", "NaN", 'E', decimal_in_shortest_low -3, high 7,
// trailing ".0"]:  x = k - 1 (the decimal exponent)
//   -3 <= x < 7   ->  [-]ddd.ddd   (at least one digit either side of the point: 100.0, 0.001)
//   otherwise     ->  [-]d.dddE[-]x (1.0E7, 1.234E-5)
#define GDV_STR_REAL 64  // flags, with GDV_MAP_DIGITS
struct gdv_real_text {
  gdv_uint64 digits;
  gdv_int32 nd, k, neg, kind, len;
};
GDV_DEV gdv_real_text gdv_real_text_of(gdv_uint64 digits, gdv_uint64 info) {
  gdv_real_text t;
  t.digits = digits;
  t.nd = (gdv_int32)(info & 255);
  t.k = (gdv_int32)((info >> 8) & 0xffff) - 2048;
  t.neg = (gdv_int32)((info >> 24) & 1);
  t.kind = (gdv_int32)((info >> 25) & 3);
  const gdv_int32 x = t.k - 1, ax = x < 0 ? -x : x;
  if (t.kind == 3) t.len = 3;                      // NaN (no sign)
  else if (t.kind == 2) t.len = t.neg + 8;         // [-]Infinity
  else if (t.kind == 1) t.len = t.neg + 3;         // [-]0.0
  else if (x >= -3 && x < 7) t.len = t.neg + (t.k <= 0 ? 2 - t.k + t.nd : t.nd <= t.k ? t.k + 2 : t.nd + 1);
  else t.len = t.neg + 2 + (t.nd > 1 ? t.nd - 1 : 1) + 1 + (x < 0 ? 1 : 0) + (ax >= 100 ? 3 : ax >= 10 ? 2 : 1);
  return t;
}
// the first `len` bytes of the text (len <= t.len), one byte store each (registry tail: not a hot path)
template <typename P>
GDV_DEV void gdv_copy_real_text(P dst, const gdv_real_text& t, gdv_int32 len) {
  if (t.neg && t.kind != 3 && len > 0) dst[0] = (gdv_uint8)'-';
  if (t.kind >= 2) {
    const gdv_uint64 w = t.kind == 3 ? 0x4e614eull : 0x7974696e69666e49ull;  // "NaN" / "Infinity", first byte lowest
    const gdv_int32 at = t.kind == 3 ? 0 : t.neg, nb = t.kind == 3 ? 3 : 8;
    for (gdv_int32 i = 0; i < nb && at + i < len; i++) dst[at + i] = (gdv_uint8)(w >> (8 * i));
    return;
  }
  if (t.kind == 1) {
    if (t.neg < len) dst[t.neg] = (gdv_uint8)'0';
    if (t.neg + 1 < len) dst[t.neg + 1] = (gdv_uint8)'.';
    if (t.neg + 2 < len) dst[t.neg + 2] = (gdv_uint8)'0';
    return;
  }
  const gdv_int32 x = t.k - 1;
  const bool fixed = x >= -3 && x < 7;
  // text position of the most significant digit and of the point
  gdv_int32 first = t.neg, point;
  if (!fixed) point = t.neg + 1;
  else if (t.k <= 0) { point = t.neg + 1; first = t.neg + 2 - t.k; }
  else point = t.neg + t.k;
  if (fixed && t.k <= 0)
    for (gdv_int32 i = t.neg; i < first && i < len; i++) dst[i] = (gdv_uint8)'0';  // "0.000": the point overwrites its place below
  if (fixed && t.k > t.nd)
    for (gdv_int32 i = t.neg + t.nd; i < t.neg + t.k && i < len; i++) dst[i] = (gdv_uint8)'0';  // 1200000.0
  if (point < len) dst[point] = (gdv_uint8)'.';
  if ((fixed ? t.k >= t.nd : t.nd == 1) && point + 1 < len) dst[point + 1] = (gdv_uint8)'0';  // the lone digit behind the point
  gdv_uint64 d = t.digits;
  for (gdv_int32 i = t.nd - 1; i >= 0; i--) {  // least significant digit first
    gdv_int32 pos = first + i;
    if (pos >= point && !(fixed && t.k <= 0)) pos++;
    if (pos < len) dst[pos] = (gdv_uint8)('0' + (gdv_int32)(d % 10));
    d /= 10;
  }
  if (!fixed) {
    gdv_int32 at = t.neg + 2 + (t.nd > 1 ? t.nd - 1 : 1);
    gdv_int32 ax = x < 0 ? -x : x;
    if (at < len) dst[at] = (gdv_uint8)'E';
    at++;
    if (x < 0) { if (at < len) dst[at] = (gdv_uint8)'-'; at++; }
    if (ax >= 100) { if (at < len) dst[at] = (gdv_uint8)('0' + ax / 100); at++; }
    if (ax >= 10) { if (at < len) dst[at] = (gdv_uint8)('0' + ax / 10 % 10); at++; }
    if (at < len) dst[at] = (gdv_uint8)('0' + ax % 10);
  }
}
template <typename P>
GDV_DEV void gdv_copy_digits(P dst, const gdv_str& s) {
  if (s.flags & GDV_STR_REAL) {
    gdv_copy_real_text(dst, gdv_real_text_of((gdv_uint64)s.p, (gdv_uint64)s.lim), s.len);
    return;
  }
  if (s.flags & GDV_STR_DECIMAL) {
    const gdv_int128 v = (gdv_int128)(((gdv_uint128)(gdv_uint64)s.lim << 64) | (gdv_uint64)s.p);
    gdv_copy_dec_text(dst, gdv_dec_text_of(v, s.flags >> 8), s.len);
    return;
  }
  const gdv_int64 v = (gdv_int64)(gdv_uint64)s.p;
  const gdv_int32 neg = v < 0 ? 1 : 0;
  gdv_uint64 mag = neg ? 0ull - (gdv_uint64)v : (gdv_uint64)v;
  const gdv_int32 total = gdv_count_digits(mag) + neg;
  gdv_uint64 w0 = neg ? (gdv_uint64)'-' : 0ull, w1 = 0, w2 = 0;  // the text, left-aligned in 24 bytes
  for (gdv_int32 k = total - 1; k >= neg; k--) {
    const gdv_uint64 b = (gdv_uint64)('0' + (gdv_int32)(mag % 10)) << (8 * (k & 7));
    mag /= 10;
    if (k < 8) w0 |= b; else if (k < 16) w1 |= b; else w2 |= b;
  }
  const gdv_int32 len = s.len;  // <= total
  if (len >= 8) __builtin_memcpy(dst, &w0, 8); else gdv_store_low_bytes(dst, w0, len);
  if (len >= 16) __builtin_memcpy(dst + 8, &w1, 8); else if (len > 8) gdv_store_low_bytes(dst + 8, w1, len - 8);
  if (len > 16) gdv_store_low_bytes(dst + 16, w2, len - 16 > 7 ? 7 : len - 16);
}
// replace table: int32 from_len, int32 to_len, 8 bytes unused, `from` bytes, (16-byte aligned) `to` bytes
GDV_DEV bool gdv_replace_match(const gdv_uint8* p, gdv_int32 i, gdv_int32 len, gdv_int32 cm, const gdv_uint8* from,
                               gdv_int32 fl) {
  bool m = i + fl <= len;
  for (gdv_int32 j = 0; m && j < fl; j++) m = gdv_map_byte(p[i + j], cm) == from[j];
  return m;
}
// First occurrence at or after byte `from` of the m-byte needle (m >= 1, readable 8 bytes past its
// end) in bytes [0, len) of p read through case map cm; -1 when absent.  Eight candidate positions
// per step: zero-byte tests on (word ^ splat of the needle's first byte) and of its second byte,
// candidates verified on a 64-bit window (the scheme of '%needle%' and locate).  Raw 8-byte loads:
// the caller guarantees GDV_STR_INBUF for the bytes it hands in.  (round 3: replace() counted and
// copied byte by byte — 5.3 ms at 5 * 10^7 rows, the slowest function of the library.)
GDV_DEV gdv_int32 gdv_find_raw(const gdv_uint8* p, gdv_int32 len, gdv_int32 cm, gdv_int32 from,
                               const gdv_uint8* needle, gdv_int32 m) {
  const gdv_int32 last = len - m;
  if (from > last) return -1;
  const gdv_uint64 mask = gdv_low_bytes_mask(m);
  const gdv_uint64 first = gdv_load8_raw(needle) & mask;
  const gdv_uint64 splat = (first & 0xffull) * 0x0101010101010101ull;
  const gdv_uint64 splat2 = ((first >> 8) & 0xffull) * 0x0101010101010101ull;
  gdv_uint64 cur = gdv_map8(gdv_load8_raw(p + from), cm);
  for (gdv_int32 base = from; base <= last; base += 8) {
    const gdv_uint64 nxt = (base + 8 < len) ? gdv_map8(gdv_load8_raw(p + base + 8), cm) : 0ull;
    const gdv_uint64 x = cur ^ splat;
    gdv_uint64 cand = (x - 0x0101010101010101ull) & ~x & 0x8080808080808080ull;
    if (m >= 2) {
      const gdv_uint64 y = ((cur >> 8) | (nxt << 56)) ^ splat2;
      cand &= (y - 0x0101010101010101ull) & ~y & 0x8080808080808080ull;
    }
    while (cand) {
      const int k = __builtin_ctzll(cand) >> 3;
      cand &= cand - 1;
      if (base + k > last) break;
      const gdv_uint64 win = k == 0 ? cur : ((cur >> (8 * k)) | (nxt << (64 - 8 * k)));
      bool eq = (win & mask) == first;
      for (gdv_int32 j = 8; eq && j < m; j += 8)
        eq = ((gdv_map8(gdv_load8_raw(p + base + k + j), cm) ^ gdv_load8_raw(needle + j)) & gdv_low_bytes_mask(m - j)) == 0;
      if (eq) return base + k;
    }
    cur = nxt;
  }
  return -1;
}
template <typename P>
GDV_DEV void gdv_copy_replaced(P dst, const gdv_str& s) {
  const gdv_uint8* desc = s.lim;
  const gdv_int32 fl = ((const gdv_int32*)desc)[0], tl = ((const gdv_int32*)desc)[1];
  const gdv_uint8* from = desc + 16;
  const gdv_uint8* to = from + ((fl + 15) & ~15);
  const gdv_int32 len = s.flags >> 2, cm = s.map & GDV_MAP_CASE;
  gdv_int32 o = 0;
  if (s.flags & GDV_STR_INBUF) {
    // word-at-a-time: the stretch up to the next match, then `to`
    for (gdv_int32 i = 0;;) {
      const gdv_int32 j = gdv_find_raw(s.p, len, cm, i, from, fl);
      const gdv_int32 stop = j < 0 ? len : j;
      gdv_int32 k = i;
      for (; k + 8 <= stop; k += 8, o += 8) {
        const gdv_uint64 w = gdv_map8(gdv_load8_raw(s.p + k), cm);
        __builtin_memcpy(dst + o, &w, 8);
      }
      if (k < stop) {
        gdv_store_low_bytes(dst + o, gdv_map8(gdv_load8_raw(s.p + k), cm), stop - k);
        o += stop - k;
      }
      if (j < 0) break;
      gdv_int32 t = 0;
      for (; t + 8 <= tl; t += 8, o += 8) {
        const gdv_uint64 w = gdv_load8_raw(to + t);
        __builtin_memcpy(dst + o, &w, 8);
      }
      if (t < tl) {
        gdv_store_low_bytes(dst + o, gdv_load8_raw(to + t), tl - t);
        o += tl - t;
      }
      i = j + fl;
    }
    return;
  }
  for (gdv_int32 i = 0; i < len;) {
    if (gdv_replace_match(s.p, i, len, cm, from, fl)) {
      for (gdv_int32 j = 0; j < tl; j++) dst[o++] = to[j];
      i += fl;
    } else {
      dst[o++] = gdv_map_byte(s.p[i], cm);
      i++;
    }
  }
}
// initcap [recalled: string_ops.cc initcap_utf8 — "any character is considered as space, except if it is
// alphanumeric"]: a letter that follows a non-alphanumeric character (or starts the text) goes to upper case, every other
// letter to lower case; digits are word characters.  ASCII only: bytes >= 0x80 are copied as they are and count as
// word characters (upstream maps them through utf8proc — stated in the oracle's recollection list).  The length of the
// text does not change.
template <typename P>
GDV_DEV void gdv_copy_initcap(P dst, const gdv_str& s) {
  const gdv_int32 cm = s.map & GDV_MAP_CASE;
  bool in_word = false;
  for (gdv_int32 i = 0; i < s.len; i += 8) {
    const gdv_int32 nb = s.len - i < 8 ? s.len - i : 8;
    gdv_str plain = s;
    plain.map = 0;
    const gdv_uint64 w = gdv_map8(gdv_raw_word_at(plain, i), cm);
    gdv_uint64 o = 0;
    for (gdv_int32 j = 0; j < nb; j++) {
      gdv_uint32 b = (gdv_uint32)(w >> (8 * j)) & 0xffu;
      const bool lower = b - 0x61u < 26u, upper = b - 0x41u < 26u;
      if (lower && !in_word) b -= 0x20u;
      else if (upper && in_word) b += 0x20u;
      in_word = lower || upper || b - 0x30u < 10u || b >= 0x80u;
      o |= (gdv_uint64)b << (8 * j);
    }
    if (nb == 8) __builtin_memcpy(dst + i, &o, 8);
    else gdv_store_low_bytes(dst + i, o, nb);
  }
}

// ---- message digests (round 5): hashSHA256 / hashSHA1 / hashMD5 [recalled: gandiva/hash_utils.cc + gdv_function_stubs:
// the digest of a string's bytes; of a NUMBER the digest of the 8 bytes of (double)value — the numeric types all go
// through gdv_double_to_long, as hash32 / hash64 do; of a NULL the digest of the empty message; the result is the
// lower-case hexadecimal text, never null].  FIPS 180-4 / RFC 1321.  Every loop below has a constant trip count and
// is fully unrolled, so the 16-word schedule and the state live in registers (nothing of these kernels may sit in
// scratch memory).  The text is produced by the output copy, like every value that only exists once it is written.
GDV_DEV gdv_uint32 gdv_rotl32(gdv_uint32 x, int n) { return (x << n) | (x >> (32 - n)); }
GDV_DEV gdv_uint32 gdv_rotr32(gdv_uint32 x, int n) { return (x >> n) | (x << (32 - n)); }
GDV_DEV gdv_int32 gdv_digest_message_len(const gdv_str& s) { return (s.map & 1024) ? 8 : (gdv_int32)s.lead; }
// message bytes [8k, 8k + 8) with the padding's 0x80 byte in place (the 64-bit bit count is the caller's)
GDV_DEV gdv_uint64 gdv_digest_chunk(const gdv_str& s, gdv_int32 k) {
  const gdv_int32 mlen = gdv_digest_message_len(s);
  const gdv_int32 at = 8 * k;
  gdv_uint64 w = 0;
  if (at < mlen) {
    if (s.map & 1024) {
      w = s.lead;
    } else {
      gdv_str src = s;
      src.p = s.lead_p;
      src.len = mlen;
      src.map = 0;
      src.flags = s.flags & GDV_STR_INBUF;
      w = gdv_map8(gdv_raw_word_at(src, at), s.map & GDV_MAP_CASE) & gdv_low_bytes_mask(mlen - at);
    }
  }
  if (mlen >= at && mlen < at + 8) w |= 0x80ull << (8 * (mlen - at));
  return w;
}
GDV_DEV void gdv_sha256_block(gdv_uint32 (&h)[8], gdv_uint32 (&w)[16]) {
  static constexpr gdv_uint32 K[64] = {
      0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u,
      0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu,
      0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u,
      0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
      0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u,
      0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
      0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
  gdv_uint32 a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
  for (int t = 0; t < 64; t++) {
    if (t >= 16) {
      const gdv_uint32 w1 = w[(t + 1) & 15], w14 = w[(t + 14) & 15];
      w[t & 15] += (gdv_rotr32(w1, 7) ^ gdv_rotr32(w1, 18) ^ (w1 >> 3)) + w[(t + 9) & 15] +
                   (gdv_rotr32(w14, 17) ^ gdv_rotr32(w14, 19) ^ (w14 >> 10));
    }
    const gdv_uint32 t1 = hh + (gdv_rotr32(e, 6) ^ gdv_rotr32(e, 11) ^ gdv_rotr32(e, 25)) + ((e & f) ^ (~e & g)) + K[t] + w[t & 15];
    const gdv_uint32 t2 = (gdv_rotr32(a, 2) ^ gdv_rotr32(a, 13) ^ gdv_rotr32(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
    hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}
GDV_DEV void gdv_sha1_block(gdv_uint32 (&h)[8], gdv_uint32 (&w)[16]) {
  gdv_uint32 a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
#pragma unroll
  for (int t = 0; t < 80; t++) {
    if (t >= 16) w[t & 15] = gdv_rotl32(w[(t + 13) & 15] ^ w[(t + 8) & 15] ^ w[(t + 2) & 15] ^ w[t & 15], 1);
    const gdv_uint32 f = t < 20 ? ((b & c) | (~b & d)) : t < 40 ? (b ^ c ^ d) : t < 60 ? ((b & c) | (b & d) | (c & d)) : (b ^ c ^ d);
    const gdv_uint32 k = t < 20 ? 0x5a827999u : t < 40 ? 0x6ed9eba1u : t < 60 ? 0x8f1bbcdcu : 0xca62c1d6u;
    const gdv_uint32 tmp = gdv_rotl32(a, 5) + f + e + k + w[t & 15];
    e = d; d = c; c = gdv_rotl32(b, 30); b = a; a = tmp;
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e;
}
GDV_DEV void gdv_md5_block(gdv_uint32 (&h)[8], gdv_uint32 (&w)[16]) {
  static constexpr gdv_uint32 K[64] = {
      0xd76aa478u, 0xe8c7b756u, 0x242070dbu, 0xc1bdceeeu, 0xf57c0fafu, 0x4787c62au, 0xa8304613u, 0xfd469501u, 0x698098d8u, 0x8b44f7afu,
      0xffff5bb1u, 0x895cd7beu, 0x6b901122u, 0xfd987193u, 0xa679438eu, 0x49b40821u, 0xf61e2562u, 0xc040b340u, 0x265e5a51u, 0xe9b6c7aau,
      0xd62f105du, 0x02441453u, 0xd8a1e681u, 0xe7d3fbc8u, 0x21e1cde6u, 0xc33707d6u, 0xf4d50d87u, 0x455a14edu, 0xa9e3e905u, 0xfcefa3f8u,
      0x676f02d9u, 0x8d2a4c8au, 0xfffa3942u, 0x8771f681u, 0x6d9d6122u, 0xfde5380cu, 0xa4beea44u, 0x4bdecfa9u, 0xf6bb4b60u, 0xbebfbc70u,
      0x289b7ec6u, 0xeaa127fau, 0xd4ef3085u, 0x04881d05u, 0xd9d4d039u, 0xe6db99e5u, 0x1fa27cf8u, 0xc4ac5665u, 0xf4292244u, 0x432aff97u,
      0xab9423a7u, 0xfc93a039u, 0x655b59c3u, 0x8f0ccc92u, 0xffeff47du, 0x85845dd1u, 0x6fa87e4fu, 0xfe2ce6e0u, 0xa3014314u, 0x4e0811a1u,
      0xf7537e82u, 0xbd3af235u, 0x2ad7d2bbu, 0xeb86d391u};
  static constexpr int R[64] = {7, 12, 17, 22, 7, 12, 17, 22, 7, 12, 17, 22, 7, 12, 17, 22, 5, 9,  14, 20, 5, 9,  14, 20, 5, 9,  14, 20, 5, 9,  14, 20,
                                4, 11, 16, 23, 4, 11, 16, 23, 4, 11, 16, 23, 4, 11, 16, 23, 6, 10, 15, 21, 6, 10, 15, 21, 6, 10, 15, 21, 6, 10, 15, 21};
  gdv_uint32 a = h[0], b = h[1], c = h[2], d = h[3];
#pragma unroll
  for (int t = 0; t < 64; t++) {
    const gdv_uint32 f = t < 16 ? ((b & c) | (~b & d)) : t < 32 ? ((d & b) | (~d & c)) : t < 48 ? (b ^ c ^ d) : (c ^ (b | ~d));
    const int g = t < 16 ? t : t < 32 ? (5 * t + 1) & 15 : t < 48 ? (3 * t + 5) & 15 : (7 * t) & 15;
    const gdv_uint32 tmp = d;
    d = c;
    c = b;
    b = b + gdv_rotl32(a + f + K[t] + w[g], R[t]);
    a = tmp;
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d;
}
// eight hexadecimal digits of x, most significant first, as the 8 bytes of one word
GDV_DEV gdv_uint64 gdv_hex8(gdv_uint32 x) {
  gdv_uint64 v = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) v |= (gdv_uint64)((x >> (28 - 4 * j)) & 0xfu) << (8 * j);
  const gdv_uint64 letter = ((v + 0x0606060606060606ull) >> 4) & 0x0101010101010101ull;  // 1 where the nibble is 10..15
  return v + 0x3030303030303030ull + letter * 39ull;
}
template <typename P>
GDV_DEV void gdv_copy_digest(P dst, const gdv_str& s) {
  const int algo = (s.map >> 8) & 3;  // 0 SHA-256, 1 SHA-1, 2 MD5
  gdv_uint32 h[8];
  if (algo == 0) {
    h[0] = 0x6a09e667u; h[1] = 0xbb67ae85u; h[2] = 0x3c6ef372u; h[3] = 0xa54ff53au;
    h[4] = 0x510e527fu; h[5] = 0x9b05688cu; h[6] = 0x1f83d9abu; h[7] = 0x5be0cd19u;
  } else {
    h[0] = 0x67452301u; h[1] = 0xefcdab89u; h[2] = 0x98badcfeu; h[3] = 0x10325476u; h[4] = 0xc3d2e1f0u; h[5] = 0; h[6] = 0; h[7] = 0;
  }
  const gdv_int32 mlen = gdv_digest_message_len(s);
  const gdv_int32 nblocks = (mlen + 9 + 63) / 64;
  const gdv_uint64 bits = (gdv_uint64)mlen * 8;
  for (gdv_int32 b = 0; b < nblocks; b++) {
    gdv_uint32 w[16];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      gdv_uint64 c = gdv_digest_chunk(s, 8 * b + j);
      if (b == nblocks - 1 && j == 7) c = algo == 2 ? bits : __builtin_bswap64(bits);  // the closing 64-bit bit count
      // SHA reads the message as big-endian 32-bit words, MD5 as little-endian ones
      w[2 * j] = algo == 2 ? (gdv_uint32)c : __builtin_bswap32((gdv_uint32)c);
      w[2 * j + 1] = algo == 2 ? (gdv_uint32)(c >> 32) : __builtin_bswap32((gdv_uint32)(c >> 32));
    }
    if (algo == 0) gdv_sha256_block(h, w);
    else if (algo == 1) gdv_sha1_block(h, w);
    else gdv_md5_block(h, w);
  }
  const int words = algo == 0 ? 8 : algo == 1 ? 5 : 4;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    if (j < words) {
      const gdv_uint64 t = gdv_hex8(algo == 2 ? __builtin_bswap32(h[j]) : h[j]);
      __builtin_memcpy(dst + 8 * j, &t, 8);
    }
  }
}
// (byte loops: the per-row-argument forms are registry-tail paths; the literal forms above keep the word-at-a-time code)
template <typename P>
GDV_DEV void gdv_copy_cycle(P dst, const gdv_str& s) {
  const gdv_int32 period = (gdv_int32)s.lead, cm = s.map & GDV_MAP_CASE;
  for (gdv_int32 j = 0, k = 0; j < s.len; j++) {
    dst[j] = gdv_map_byte(s.p[k], cm);
    if (++k == period) k = 0;
  }
}
GDV_DEV bool gdv_match_row(const gdv_uint8* p, gdv_int32 i, gdv_int32 len, gdv_int32 cm, const gdv_uint8* from, gdv_int32 fl, gdv_int32 fm) {
  bool m = i + fl <= len;
  for (gdv_int32 j = 0; m && j < fl; j++) m = gdv_map_byte(p[i + j], cm) == gdv_map_byte(from[j], fm);
  return m;
}
template <typename P>
GDV_DEV void gdv_copy_replaced_row(P dst, const gdv_str& s) {
  const gdv_int32 len = (gdv_int32)(gdv_uint32)s.lead, fl = (gdv_int32)((s.lead >> 32) & 0xffff), tl = (gdv_int32)(s.lead >> 48);
  const gdv_int32 cm = s.map & GDV_MAP_CASE, fm = (s.flags >> 8) & 3, tm = (s.flags >> 10) & 3;
  gdv_int32 o = 0;
  for (gdv_int32 i = 0; i < len;) {
    if (gdv_match_row(s.p, i, len, cm, s.lim, fl, fm)) {
      for (gdv_int32 j = 0; j < tl; j++) dst[o++] = gdv_map_byte(s.lead_p[j], tm);
      i += fl;
    } else {
      dst[o++] = gdv_map_byte(s.p[i], cm);
      i++;
    }
  }
}
template <typename P>
GDV_DEV void gdv_copy_special(P dst, const gdv_str& s) {
  if (s.map & GDV_MAP_CYCLE) { gdv_copy_cycle(dst, s); return; }
  if (s.map & GDV_MAP_REPLACE_ROW) { gdv_copy_replaced_row(dst, s); return; }
  if (s.map & GDV_MAP_DIGEST) gdv_copy_digest(dst, s);
  else if (s.map & GDV_MAP_INITCAP) gdv_copy_initcap(dst, s);
  else if (s.map & GDV_MAP_DIGITS) gdv_copy_digits(dst, s);
  else if (s.map & GDV_MAP_REPLACE) gdv_copy_replaced(dst, s);
  else gdv_copy_reversed(dst, s);
}
// Copy with as few (scattered) store instructions as possible: whole words, then ONE
// overlapping store for the tail (the last 8 bytes again for len >= 8, two overlapping
// 4-byte stores for 4..7) instead of a 4 + 2 + 1 byte ladder.
GDV_DEV void gdv_str_copy(gdv_uint8* dst, const gdv_str& s) {
  if (s.map & GDV_MAP_SPECIAL) { gdv_copy_special(dst, s); return; }
  if (s.len >= 8) {
    gdv_int32 i = 0;
    for (; i + 8 <= s.len; i += 8) {
      const gdv_uint64 w = gdv_word_at(s, i);
      __builtin_memcpy(dst + i, &w, 8);
    }
    if (i < s.len) {
      const gdv_uint64 w = gdv_word_at(s, s.len - 8);
      __builtin_memcpy(dst + s.len - 8, &w, 8);
    }
  } else if (s.len >= 4) {
    const gdv_uint64 w = gdv_word_at(s, 0);
    const gdv_uint32 lo = (gdv_uint32)w, hi = (gdv_uint32)(w >> (8 * (s.len - 4)));
    __builtin_memcpy(dst, &lo, 4);
    __builtin_memcpy(dst + s.len - 4, &hi, 4);
  } else if (s.len > 0) {
    const gdv_uint64 w = gdv_word_at(s, 0);
    dst[0] = (gdv_uint8)w;
    if (s.len > 1) dst[1] = (gdv_uint8)(w >> 8);
    if (s.len > 2) dst[2] = (gdv_uint8)(w >> 16);
  }
}
#ifndef GDV_HOST_BUILD
// One row's bytes into the wave's LDS staging window: whole words, then a 4/2/1 ladder.
typedef __attribute__((address_space(3))) gdv_uint8 gdv_lds_u8;
GDV_DEV void gdv_stage_copy(gdv_lds_u8* dst, const gdv_str& s) {
  if (s.map & GDV_MAP_SPECIAL) { gdv_copy_special(dst, s); return; }
  const gdv_int32 len = s.len;
  gdv_int32 i = 0;
  for (; i + 8 <= len; i += 8) {
    const gdv_uint64 w = gdv_word_at(s, i);
    __builtin_memcpy(dst + i, &w, 8);
  }
  const gdv_int32 r = len - i;
  if (r > 0) {
    gdv_uint64 w = gdv_word_at(s, i);  // bytes past the view are never stored
    if (r & 4) { const gdv_uint32 v = (gdv_uint32)w; __builtin_memcpy(dst + i, &v, 4); i += 4; w >>= 32; }
    if (r & 2) { const gdv_uint16 v = (gdv_uint16)w; __builtin_memcpy(dst + i, &v, 2); i += 2; w >>= 16; }
    if (r & 1) dst[i] = (gdv_uint8)w;
  }
}
// Wave-shaped kernels sweep one sub-tile (64 rows) — since round 6 a group of GDV_SG sub-tiles — at a time and keep its
// span in LDS: GDV_SUB_SPAN = bytes of span the match bitmaps and the mirror cover (32 per row on average for one
// sub-tile, 20 for a group of four; longer spans — wave-uniform — take the per-row search and read HBM).
#ifndef GDV_SUB_SPAN
#define GDV_SUB_SPAN 2048
#endif
typedef __attribute__((address_space(3))) gdv_uint64 gdv_lds_u64;
// 8 bytes at byte offset d of the LDS mirror (base 16-byte aligned, readable 16 bytes past any
// valid offset): two ALIGNED words and a funnel shift — no unaligned LDS read
GDV_DEV gdv_uint64 gdv_mirror_word(const gdv_lds_u8* mir, gdv_int32 d) {
  const gdv_lds_u64* q = (const gdv_lds_u64*)(mir + (d & ~7));
  const gdv_uint64 lo = q[0], hi = q[1];
  const gdv_int32 sh = (d & 7) * 8;
  return (lo >> sh) | ((hi << 1) << (63 - sh));
}
// gdv_stage_copy for a view that lies inside the mirrored span [mbase, mbase + mlen) of its column:
// the bytes come from LDS (the sweep put them there) instead of a second trip to L2 / the fabric.
// Any other view — literals, other columns, spans too long for the mirror (mlen = 0) — and the
// non-view kinds take the ordinary copy.  The test is per lane.
GDV_DEV void gdv_stage_copy_mir(gdv_lds_u8* dst, const gdv_str& s, const gdv_lds_u8* mir, const gdv_uint8* mbase,
                                gdv_int32 mlen) {
  const gdv_int64 d64 = s.p - mbase;
  if ((s.map & GDV_MAP_SPECIAL) || d64 < 0 || d64 + s.len > (gdv_int64)mlen) {
    gdv_stage_copy(dst, s);
    return;
  }
  const gdv_int32 d = (gdv_int32)d64, len = s.len;
  gdv_int32 i = 0;
  for (; i + 8 <= len; i += 8) {
    const gdv_uint64 w = gdv_map8(gdv_mirror_word(mir, d + i), s.map);
    __builtin_memcpy(dst + i, &w, 8);
  }
  const gdv_int32 r = len - i;
  if (r > 0) {
    gdv_uint64 w = gdv_map8(gdv_mirror_word(mir, d + i), s.map);  // bytes past the view are never stored
    if (r & 4) { const gdv_uint32 v = (gdv_uint32)w; __builtin_memcpy(dst + i, &v, 4); i += 4; w >>= 32; }
    if (r & 2) { const gdv_uint16 v = (gdv_uint16)w; __builtin_memcpy(dst + i, &v, 2); i += 2; w >>= 16; }
    if (r & 1) dst[i] = (gdv_uint8)w;
  }
}
#endif
// the same out of line: rows that bypass the LDS staging window (wave tiles whose bytes do not
// fit it) — rare, and inlining it at every sub-tile of every output doubles the kernel
static __device__ GDV_COLD void gdv_str_copy_direct(gdv_uint8* dst, const gdv_uint8* p, gdv_int32 len, gdv_int32 map,
                                                   const gdv_uint8* lim) {
  gdv_str s;
  s.p = p; s.len = len; s.map = map; s.lim = lim; s.flags = 0;
  gdv_str_copy(dst, s);
}
// ---- LDS staging of var-len output bytes.  Every lane writes its row's bytes into the wave's
// private LDS window at the row's offset inside the wave tile (byte-granular, unaligned LDS
// writes: cheap), then the wave streams the window to HBM as consecutive 16-byte pieces, the last
// one shifted back to end exactly at the total (it overlaps its neighbour with identical bytes) —
// one coalesced store instruction per KiB instead of several scattered stores per row.  (Pieces
// aligned in the output with head / tail bytes stored singly measured 2 % slower.)
#ifndef GDV_OUT_WIN
#define GDV_OUT_WIN (GDV_U * 64 * 8)  // staged bytes per wave tile and output: 8 per row on average
#endif
#ifndef GDV_HOST_BUILD
GDV_DEV void gdv_flush_out(gdv_uint8* __restrict__ dst, const gdv_uint8* win, gdv_int32 cnt, int lane) {
  __builtin_amdgcn_wave_barrier();  // LDS ops of one wave execute in order: ordering only
#ifdef GDV_FLUSH_ALIGNED
  // experiment: 16-byte stores aligned in the OUTPUT, ragged head and tail byte by byte
  {
    gdv_int32 head = (gdv_int32)((16 - ((gdv_uint64)dst & 15)) & 15);
    head = head < cnt ? head : cnt;
    if (lane < head) dst[lane] = win[lane];
    const gdv_int32 body = (cnt - head) & ~15;
    for (gdv_int32 i = lane * 16; i < body; i += 1024) {
      gdv_uint64 w[2];
      __builtin_memcpy(w, win + head + i, 16);
      __builtin_memcpy(__builtin_assume_aligned(dst + head + i, 16), w, 16);
    }
    const gdv_int32 t0 = head + body;
    if (t0 + lane < cnt) dst[t0 + lane] = win[t0 + lane];
    __builtin_amdgcn_wave_barrier();
    return;
  }
#endif
  if (cnt >= 16) {
    for (gdv_int32 i = lane * 16; i < cnt; i += 1024) {
      const gdv_int32 j = i + 16 <= cnt ? i : cnt - 16;  // the last piece is shifted back to end at cnt
      gdv_uint64 w[2];
      __builtin_memcpy(w, win + j, 16);
      gdv_store16(dst + j, w[0], w[1]);
    }
  } else if (lane < cnt) {
    dst[lane] = win[lane];
  }
  __builtin_amdgcn_wave_barrier();
}
// The output bytes of a wave tile ARE the (mapped) bytes of a contiguous input span (an input
// column passed through, upper(col), lower(col) with no row dropped): stream them, lanes over
// bytes, 16 B per lane.
GDV_DEV void gdv_flat_copy(gdv_uint8* __restrict__ dst, const gdv_uint8* __restrict__ src, gdv_int32 cnt,
                           gdv_int32 map, int lane) {
  if (cnt >= 16) {
    for (gdv_int32 i = lane * 16; i < cnt; i += 1024) {
      const gdv_int32 j = i + 16 <= cnt ? i : cnt - 16;
      gdv_uint64 w[2];
      __builtin_memcpy(w, src + j, 16);
      w[0] = gdv_map8(w[0], map);
      w[1] = gdv_map8(w[1], map);
      __builtin_memcpy(dst + j, w, 16);
    }
  } else if (lane < cnt) {
    dst[lane] = gdv_map_byte(src[lane], map);
  }
}
#endif

GDV_DEV bool gdv_is_utf8_lead(gdv_uint8 c) { return (c & 0xC0) != 0x80; }
// number of UTF-8 characters = bytes that are not continuation bytes (10xxxxxx)
GDV_DEV gdv_uint64 gdv_mask_upto(gdv_int32 nbytes) {  // any nbytes: <= 0 -> 0, >= 8 -> all ones
  return nbytes <= 0 ? 0ull : gdv_low_bytes_mask(nbytes);
}
GDV_DEV gdv_int32 gdv_utf8_count(const gdv_str& s) {
  if (s.flags & GDV_STR_ASCII) return s.len;
  gdv_uint64 lead;
  if (gdv_lead_window(s, &lead)) return (gdv_int32)__popcll(lead);
  gdv_int32 cont = 0;
  for (gdv_int32 i = 0; i < s.len; i += 8) {
    gdv_uint64 w = gdv_raw_word_at(s, i) & gdv_low_bytes_mask(s.len - i);
    cont += __popcll(w & GDV_B80 & ~((w << 1) & GDV_B80));
  }
  return s.len - cont;
}
static __device__ GDV_COLD bool gdv_bytes_are_ascii(const gdv_uint8* p, gdv_int32 len, const gdv_uint8* lim) {
  gdv_uint64 acc = 0;
  for (gdv_int32 i = 0; i < len; i += 8) acc |= gdv_load8(p + i, lim) & gdv_low_bytes_mask(len - i);
  return (acc & GDV_B80) == 0;
}
// the same test inlined: selection-mode wave kernels run it on every row they copy (round 5)
GDV_DEV bool gdv_row_is_ascii(const gdv_str& s) {
  gdv_uint64 acc = 0;
  for (gdv_int32 i = 0; i < s.len; i += 8) acc |= gdv_load8(s.p + i, s.lim) & gdv_low_bytes_mask(s.len - i);
  return (acc & GDV_B80) == 0;
}
GDV_DEV bool gdv_str_is_ascii(const gdv_str& s) {
  if (s.flags & GDV_STR_ASCII) return true;  // answered for the whole tile by the byte sweep
  // (a row the exact variant flagged holds a byte >= 0x80 itself or shares a 16-byte piece with one
  // that does: the general paths are exact either way, and with the lead mask they read no byte)
  if (s.flags & GDV_STR_LEAD) return false;
  return gdv_bytes_are_ascii(s.p, s.len, s.lim);
}
// bytes [i, i+n) of s equal the n bytes at q (n >= 0; q readable up to qlim)
GDV_DEV bool gdv_bytes_equal(const gdv_str& s, gdv_int32 i, const gdv_uint8* q, const gdv_uint8* qlim,
                             gdv_int32 n) {
  for (gdv_int32 k = 0; k < n; k += 8) {
    const gdv_uint64 m = gdv_low_bytes_mask(n - k);
    if (((gdv_word_at(s, i + k) ^ gdv_load8(q + k, qlim)) & m) != 0) return false;
  }
  return true;
}

// ---- hash of var-len values: MurmurHash3 over the (mapped) bytes, 8 bytes per load.
// x64_128 variant, first 64 bits of the digest (hash64) and x86_32 variant (hash32); both
// seeds start h1 (= h2) as the numeric variants above do.  Null hashes to the seed.
GDV_DEV gdv_int64 gdv_murmur3_64_buf(const gdv_str& s, gdv_int32 seed) {
  const gdv_uint64 c1 = 0x87c37b91114253d5ULL, c2 = 0x4cf5ad432745937fULL;
  gdv_uint64 h1 = (gdv_uint64)(gdv_int64)seed, h2 = h1;
  gdv_int32 i = 0;
  for (; i + 16 <= s.len; i += 16) {
    gdv_uint64 k1 = gdv_word_at(s, i), k2 = gdv_word_at(s, i + 8);
    k1 *= c1; k1 = gdv_rotl64(k1, 31); k1 *= c2; h1 ^= k1;
    h1 = gdv_rotl64(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729;
    k2 *= c2; k2 = gdv_rotl64(k2, 33); k2 *= c1; h2 ^= k2;
    h2 = gdv_rotl64(h2, 31); h2 += h1; h2 = h2 * 5 + 0x38495ab5;
  }
  const gdv_int32 rem = s.len - i;  // 0..15 tail bytes, zero-extended into (k1, k2)
  if (rem > 8) {
    gdv_uint64 k2 = gdv_word_at(s, i + 8) & gdv_low_bytes_mask(rem - 8);
    k2 *= c2; k2 = gdv_rotl64(k2, 33); k2 *= c1; h2 ^= k2;
  }
  if (rem > 0) {
    gdv_uint64 k1 = gdv_word_at(s, i) & gdv_low_bytes_mask(rem);
    k1 *= c1; k1 = gdv_rotl64(k1, 31); k1 *= c2; h1 ^= k1;
  }
  h1 ^= (gdv_uint64)s.len; h2 ^= (gdv_uint64)s.len;
  h1 += h2; h2 += h1;
  h1 = gdv_fmix64(h1); h2 = gdv_fmix64(h2);
  h1 += h2;
  return (gdv_int64)h1;
}
GDV_DEV gdv_uint32 gdv_mm32_block(gdv_uint32 h, gdv_uint32 k) {
  k *= 0xcc9e2d51u; k = (k << 15) | (k >> 17); k *= 0x1b873593u;
  h ^= k; h = (h << 13) | (h >> 19);
  return h * 5u + 0xe6546b64u;
}
GDV_DEV gdv_uint32 gdv_mm32_tail(gdv_uint32 h, gdv_uint32 k) {
  k *= 0xcc9e2d51u; k = (k << 15) | (k >> 17); k *= 0x1b873593u;
  return h ^ k;
}
GDV_DEV gdv_int32 gdv_murmur3_32_buf(const gdv_str& s, gdv_int32 seed) {
  gdv_uint32 h = (gdv_uint32)seed;
  for (gdv_int32 i = 0; i < s.len; i += 8) {
    const gdv_int32 rem = s.len - i;
    const gdv_uint64 w = gdv_word_at(s, i) & gdv_low_bytes_mask(rem);
    const gdv_uint32 lo = (gdv_uint32)w, hi = (gdv_uint32)(w >> 32);
    h = rem >= 4 ? gdv_mm32_block(h, lo) : gdv_mm32_tail(h, lo);
    if (rem >= 8) h = gdv_mm32_block(h, hi);
    else if (rem > 4) h = gdv_mm32_tail(h, hi);
  }
  h ^= (gdv_uint32)s.len;
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return (gdv_int32)h;
}
#define GDV_HASH_BUF(T)                                                                          \
  GDV_DEV gdv_int32 hash32_##T(gdv_str v, bool valid) { return valid ? gdv_murmur3_32_buf(v, 0) : 0; } \
  GDV_DEV gdv_int32 hash32_##T##_int32(gdv_str v, bool valid, gdv_int32 seed, bool sv) {         \
    gdv_int32 s = sv ? seed : 0;                                                                 \
    return valid ? gdv_murmur3_32_buf(v, s) : s;                                                 \
  }                                                                                              \
  GDV_DEV gdv_int64 hash64_##T(gdv_str v, bool valid) { return valid ? gdv_murmur3_64_buf(v, 0) : 0; } \
  GDV_DEV gdv_int64 hash64_##T##_int64(gdv_str v, bool valid, gdv_int64 seed, bool sv) {         \
    gdv_int64 s = sv ? seed : 0;                                                                 \
    return valid ? gdv_murmur3_64_buf(v, (gdv_int32)s) : s;                                      \
  }
GDV_HASH_BUF(utf8)
GDV_HASH_BUF(binary)
// decimal128: MurmurHash3 over the 16 little-endian bytes of the value, as over a binary of that length; a NULL hashes to
// the seed (0 without one).  The two words are read back 8 bytes at a time: the loops above have a known trip count.
GDV_DEV gdv_int32 gdv_dec_hash32(gdv_int128 v, gdv_int32 seed) {
  const gdv_uint64 w[2] = {(gdv_uint64)v, (gdv_uint64)((gdv_uint128)v >> 64)};
  return gdv_murmur3_32_buf(gdv_make_str((const gdv_uint8*)w, 0, 16, (const gdv_uint8*)(w + 2), GDV_STR_INBUF), seed);
}
GDV_DEV gdv_int64 gdv_dec_hash64(gdv_int128 v, gdv_int32 seed) {
  const gdv_uint64 w[2] = {(gdv_uint64)v, (gdv_uint64)((gdv_uint128)v >> 64)};
  return gdv_murmur3_64_buf(gdv_make_str((const gdv_uint8*)w, 0, 16, (const gdv_uint8*)(w + 2), GDV_STR_INBUF), seed);
}
GDV_DEV gdv_int32 hash32_decimal128(gdv_int128 v, int vp, int vs, bool valid) { return valid ? gdv_dec_hash32(v, 0) : 0; }
GDV_DEV gdv_int32 hash32_decimal128_int32(gdv_int128 v, int vp, int vs, bool valid, gdv_int32 seed, bool sv) {
  const gdv_int32 s = sv ? seed : 0;
  return valid ? gdv_dec_hash32(v, s) : s;
}
GDV_DEV gdv_int64 hash64_decimal128(gdv_int128 v, int vp, int vs, bool valid) { return valid ? gdv_dec_hash64(v, 0) : 0; }
GDV_DEV gdv_int64 hash64_decimal128_int64(gdv_int128 v, int vp, int vs, bool valid, gdv_int64 seed, bool sv) {
  const gdv_int64 s = sv ? seed : 0;
  return valid ? gdv_dec_hash64(v, (gdv_int32)s) : s;
}

GDV_DEV gdv_int32 octet_length_utf8(gdv_str s) { return s.len; }
GDV_DEV gdv_int32 bit_length_utf8(gdv_str s) { return s.len * 8; }
GDV_DEV gdv_int32 char_length_utf8(gdv_str s) { return gdv_utf8_count(s); }
GDV_DEV gdv_str upper_utf8(gdv_str s) { s.map = 1; return s; }
GDV_DEV gdv_str lower_utf8(gdv_str s) { s.map = 2; return s; }

// Comparisons work on 8-byte words (from the register cache where the view has one), not on
// single bytes.  Bytes are compared as unsigned values in memory order, which is the little-end
// byte of the first differing word.
GDV_DEV int gdv_str_compare(const gdv_str& a, const gdv_str& b) {
  const gdv_int32 n = a.len < b.len ? a.len : b.len;
  for (gdv_int32 i = 0; i < n; i += 8) {
    const gdv_uint64 m = gdv_low_bytes_mask(n - i);
    const gdv_uint64 wa = gdv_word_at(a, i) & m, wb = gdv_word_at(b, i) & m;
    const gdv_uint64 x = wa ^ wb;
    if (x != 0) {
      const int sh = __builtin_ctzll(x) & ~7;
      return ((wa >> sh) & 0xffull) < ((wb >> sh) & 0xffull) ? -1 : 1;
    }
  }
  return a.len < b.len ? -1 : (a.len > b.len ? 1 : 0);
}
GDV_DEV bool gdv_str_equal_words(const gdv_str& a, gdv_int32 at, const gdv_str& b, gdv_int32 n) {
  for (gdv_int32 i = 0; i < n; i += 8) {  // bytes [at, at+n) of a against bytes [0, n) of b
    const gdv_uint64 m = gdv_low_bytes_mask(n - i);
    if (((gdv_word_at(a, at + i) ^ gdv_word_at(b, i)) & m) != 0) return false;
  }
  return true;
}
GDV_DEV bool equal_utf8_utf8(gdv_str a, gdv_str b) { return a.len == b.len && gdv_str_equal_words(a, 0, b, a.len); }
GDV_DEV bool not_equal_utf8_utf8(gdv_str a, gdv_str b) { return !equal_utf8_utf8(a, b); }
GDV_DEV bool less_than_utf8_utf8(gdv_str a, gdv_str b) { return gdv_str_compare(a, b) < 0; }
GDV_DEV bool less_than_or_equal_to_utf8_utf8(gdv_str a, gdv_str b) { return gdv_str_compare(a, b) <= 0; }
GDV_DEV bool greater_than_utf8_utf8(gdv_str a, gdv_str b) { return gdv_str_compare(a, b) > 0; }
GDV_DEV bool greater_than_or_equal_to_utf8_utf8(gdv_str a, gdv_str b) { return gdv_str_compare(a, b) >= 0; }
GDV_DEV bool starts_with_utf8_utf8(gdv_str s, gdv_str prefix) {
  return prefix.len <= s.len && gdv_str_equal_words(s, 0, prefix, prefix.len);
}
GDV_DEV bool ends_with_utf8_utf8(gdv_str s, gdv_str suffix) {
  return suffix.len <= s.len && gdv_str_equal_words(s, s.len - suffix.len, suffix, suffix.len);
}

// byte offset of the character with 0-based index `ci` in a string that is not pure ASCII
// (s.len when the string has fewer characters): 8 bytes per step — the lead bytes of a word are
// counted with one popcount, and only the word holding the wanted character is looked into
static __device__ GDV_COLD gdv_int32 gdv_utf8_byte_pos_general(const gdv_str& s, gdv_int32 ci) {
  gdv_uint64 lm;
  if (gdv_lead_window(s, &lm)) {  // select: the position of the ci-th set bit of the lead mask
    if (ci < 0 || ci >= (gdv_int32)__popcll(lm)) return ci < 0 ? 0 : s.len;
    for (gdv_int32 k = ci; k > 0; k--) lm &= lm - 1;
    return (gdv_int32)__builtin_ctzll(lm);
  }
  gdv_int32 seen = 0;
  for (gdv_int32 i = 0; i < s.len; i += 8) {
    const gdv_uint64 w = gdv_raw_word_at(s, i);
    // bit 7 of every byte that STARTS a character (not 10xxxxxx), bytes past the end excluded
    gdv_uint64 lead = ~(w & ~(w << 1)) & GDV_B80 & gdv_low_bytes_mask(s.len - i);
    const gdv_int32 c = __popcll(lead);
    if (seen + c > ci) {
      for (gdv_int32 k = ci - seen; k > 0; k--) lead &= lead - 1;  // drop the characters before it
      return i + (__builtin_ctzll(lead) >> 3);
    }
    seen += c;
  }
  return s.len;
}
// the general (non-ASCII) substr; tiles of pure ASCII never call it
static __device__ GDV_COLD gdv_str gdv_substr_utf8_general(gdv_str s, gdv_int64 from, gdv_int64 count) {
  gdv_str r = s;
  r.len = 0;
  const gdv_int64 glyphs = gdv_utf8_count(s);
  gdv_int64 start = from > 0 ? from - 1 : (from < 0 ? glyphs + from : 0);
  if (start < 0 || start >= glyphs) return r;
  const gdv_int64 stop = start + count < glyphs ? start + count : glyphs;
  const gdv_int32 b0 = gdv_utf8_byte_pos_general(s, (gdv_int32)start);
  const gdv_int32 b1 = stop >= glyphs ? s.len : gdv_utf8_byte_pos_general(s, (gdv_int32)stop);
  r.p = s.p + b0;
  r.len = b1 - b0;
  return r;
}

// substr(s, from, len): 1-based character positions (UTF-8 aware); from < 0 counts from the
// end; from == 0 behaves like 1; len <= 0 or a start outside the string give "".
GDV_DEV gdv_str substr_utf8_int64_int64(gdv_str s, gdv_int64 from, gdv_int64 count) {
  gdv_str r = s;
  r.len = 0;
  if (count <= 0 || s.len <= 0) return r;
  if (gdv_str_is_ascii(s)) {  // character index == byte index
    gdv_int64 start = from > 0 ? from - 1 : (from < 0 ? (gdv_int64)s.len + from : 0);
    if (start < 0 || start >= s.len) return r;
    gdv_int64 stop = start + count < s.len ? start + count : s.len;
    r.p = s.p + start;
    r.len = (gdv_int32)(stop - start);
    return r;
  }
  return gdv_substr_utf8_general(s, from, count);
}
GDV_DEV gdv_str substr_utf8_int64(gdv_str s, gdv_int64 from) {
  return substr_utf8_int64_int64(s, from, 0x7fffffff);
}
// byte offset of the character with 0-based index `ci` (s.len when the string is shorter)
GDV_DEV gdv_int32 gdv_utf8_byte_pos(const gdv_str& s, gdv_int32 ci) {
  if (ci <= 0) return 0;
  if (s.flags & GDV_STR_ASCII) return ci < s.len ? ci : s.len;
  return gdv_utf8_byte_pos_general(s, ci);
}
GDV_DEV gdv_str gdv_empty_str() { return gdv_make_str(nullptr, 0, 0, nullptr, GDV_STR_ASCII | GDV_STR_INBUF); }
// left(s, n): the first n characters; n < 0: all but the last |n|
GDV_DEV gdv_str left_utf8_int32(gdv_str s, gdv_int32 n) {
  gdv_str r = s;
  r.len = 0;
  if (n == 0 || s.len <= 0) return r;
  const gdv_int32 chars = gdv_utf8_count(s);
  const gdv_int32 end = n > 0 ? (n < chars ? n : chars) : (chars + n > 0 ? chars + n : 0);
  r.len = gdv_utf8_byte_pos(s, end);
  return r;
}
// right(s, n): the last n characters; n < 0: all but the first |n|
GDV_DEV gdv_str right_utf8_int32(gdv_str s, gdv_int32 n) {
  gdv_str r = s;
  r.len = 0;
  if (n == 0 || s.len <= 0) return r;
  const gdv_int32 chars = gdv_utf8_count(s);
  const gdv_int32 start = n > 0 ? chars - (n < chars ? n : chars) : (-(gdv_int64)n < chars ? -n : chars);
  const gdv_int32 b = gdv_utf8_byte_pos(s, start);
  r.p = s.p + b;
  r.len = s.len - b;
  return r;
}
// castVARCHAR(s, n): s cut to at most n characters; n < 0 is an execution error
GDV_DEV gdv_str castVARCHAR_utf8_int64(gdv_ctx ctx, gdv_str s, gdv_int64 n) {
  gdv_str r = s;
  if (n < 0) { gdv_raise(ctx, GDV_ERR_BAD_ARG); r.len = 0; return r; }
  if (n >= s.len) return r;  // bytes >= characters
  r.len = gdv_utf8_byte_pos(s, (gdv_int32)n);
  return r;
}
// castVARCHAR(integer, n): the decimal text of the value, cut to n bytes; n < 0 is an execution error
GDV_DEV gdv_str castVARCHAR_int64_int64(gdv_ctx ctx, gdv_int64 v, gdv_int64 n) {
  gdv_str r = gdv_empty_str();
  if (n < 0) { gdv_raise(ctx, GDV_ERR_BAD_ARG); return r; }
  const gdv_int32 total = gdv_count_digits(v < 0 ? 0ull - (gdv_uint64)v : (gdv_uint64)v) + (v < 0 ? 1 : 0);
  r.p = (const gdv_uint8*)(gdv_uint64)v;
  r.len = n < total ? (gdv_int32)n : total;
  r.map = GDV_MAP_DIGITS;
  return r;
}
GDV_DEV gdv_str castVARCHAR_int32_int64(gdv_ctx ctx, gdv_int32 v, gdv_int64 n) {
  return castVARCHAR_int64_int64(ctx, (gdv_int64)v, n);
}
// castVARCHAR(decimal128, n): Arrow's text of the value at the type's scale, cut to n bytes
// [gdv_fn_dec_to_string + the length cut of castVARCHAR_decimal128_int64, as recalled]
GDV_DEV gdv_str castVARCHAR_decimal128_int64(gdv_ctx ctx, gdv_int128 v, int xp, int xs, gdv_int64 n, int op, int os) {
  (void)xp; (void)op; (void)os;
  gdv_str r = gdv_empty_str();
  if (n < 0) { gdv_raise(ctx, GDV_ERR_BAD_ARG); return r; }
  const gdv_int32 total = gdv_dec_text_of(v, xs).len;
  r.p = (const gdv_uint8*)(gdv_uint64)(gdv_uint128)v;
  r.lim = (const gdv_uint8*)(gdv_uint64)((gdv_uint128)v >> 64);
  r.len = n < total ? (gdv_int32)n : total;
  r.map = GDV_MAP_DIGITS;
  r.flags = GDV_STR_DECIMAL | (xs << 8);
  return r;
}
// ---- shortest round-trip digits of a binary floating-point value f * 2^e (round 5): the free-format
// algorithm of Burger & Dybvig ("Printing Floating-Point Numbers Quickly and Accurately", 1996) over
// exact integers — r / s = the value scaled into [0.1, 1), m- / m+ = the distances to the neighbouring
// values' midpoints; digits are generated while the remainder is further from both midpoints than the
// digits already out could be.  Per-lane big integers of up to 36 32-bit words (a double's 2^-1074
// scaled by 10^324 needs 1132 bits) in private memory, lengths tracked, so ordinary magnitudes touch a
// few words.  A registry-tail function: correct first (pinned to Python's repr and numpy's float32
// digits on the host build of this header), ~10^4 operations per value at the exponent range's ends.
#define GDV_BIG_WORDS 36
struct gdv_big {
  gdv_uint32 w[GDV_BIG_WORDS];
  gdv_int32 n;  // words in use; w[n..] are zero
};
GDV_DEV void gdv_big_set(gdv_big& b, gdv_uint64 v, gdv_int32 sh) {  // b = v << sh
  for (gdv_int32 i = 0; i < GDV_BIG_WORDS; i++) b.w[i] = 0;
  const gdv_int32 word = sh >> 5, bit = sh & 31;
  const gdv_uint128 t = (gdv_uint128)v << bit;
  b.w[word] = (gdv_uint32)t;
  if (word + 1 < GDV_BIG_WORDS) b.w[word + 1] = (gdv_uint32)(t >> 32);
  if (word + 2 < GDV_BIG_WORDS) b.w[word + 2] = (gdv_uint32)(t >> 64);
  b.n = word + 3 < GDV_BIG_WORDS ? word + 3 : GDV_BIG_WORDS;
  while (b.n > 0 && b.w[b.n - 1] == 0) b.n--;
}
GDV_DEV void gdv_big_mul(gdv_big& b, gdv_uint32 m) {
  gdv_uint64 carry = 0;
  for (gdv_int32 i = 0; i < b.n; i++) {
    const gdv_uint64 t = (gdv_uint64)b.w[i] * m + carry;
    b.w[i] = (gdv_uint32)t;
    carry = t >> 32;
  }
  if (carry != 0 && b.n < GDV_BIG_WORDS) b.w[b.n++] = (gdv_uint32)carry;
}
GDV_DEV void gdv_big_pow10(gdv_big& b, gdv_int32 k) {  // b *= 10^k, k >= 0
  for (; k >= 9; k -= 9) gdv_big_mul(b, 1000000000u);
  gdv_uint32 p = 1;
  for (; k > 0; k--) p *= 10u;
  if (p > 1) gdv_big_mul(b, p);
}
GDV_DEV gdv_int32 gdv_big_cmp(const gdv_big& a, const gdv_big& b) {
  if (a.n != b.n) return a.n < b.n ? -1 : 1;
  for (gdv_int32 i = a.n - 1; i >= 0; i--)
    if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
  return 0;
}
GDV_DEV void gdv_big_add(gdv_big& a, const gdv_big& b) {  // a += b
  const gdv_int32 n = a.n > b.n ? a.n : b.n;
  gdv_uint64 carry = 0;
  for (gdv_int32 i = 0; i < n; i++) {
    const gdv_uint64 t = (gdv_uint64)a.w[i] + b.w[i] + carry;
    a.w[i] = (gdv_uint32)t;
    carry = t >> 32;
  }
  a.n = n;
  if (carry != 0 && a.n < GDV_BIG_WORDS) a.w[a.n++] = (gdv_uint32)carry;
}
GDV_DEV void gdv_big_sub(gdv_big& a, const gdv_big& b) {  // a -= b, a >= b
  gdv_int64 borrow = 0;
  for (gdv_int32 i = 0; i < a.n; i++) {
    const gdv_int64 t = (gdv_int64)a.w[i] - (i < b.n ? b.w[i] : 0u) - borrow;
    a.w[i] = (gdv_uint32)t;
    borrow = t < 0 ? 1 : 0;
  }
  while (a.n > 0 && a.w[a.n - 1] == 0) a.n--;
}
struct gdv_real_digits {
  gdv_uint64 digits;  // no trailing zeros
  gdv_int32 nd, k;    // value = 0.digits * 10^k
};
// f != 0; `closer_below`: the neighbour below is half as far away as the one above (f is the smallest
// significand of its binade and not of the lowest binade)
GDV_DEV gdv_real_digits gdv_shortest_digits(gdv_uint64 f, gdv_int32 e, bool closer_below) {
  gdv_big r, s, m;
  const gdv_int32 sh = closer_below ? 2 : 1;
  gdv_big_set(r, f, sh + (e > 0 ? e : 0));
  gdv_big_set(s, 1, sh + (e < 0 ? -e : 0));
  gdv_big_set(m, 1, e > 0 ? e : 0);  // m- ; m+ = m- (twice m- when closer_below)
  const bool even = (f & 1) == 0;    // round-to-even reads the midpoints themselves back as f
  const gdv_int32 lg = e + 63 - __builtin_clzll(f);
  gdv_int32 k = (gdv_int32)ceil((double)lg * 0.30102999566398114 - 1e-10);  // ceil(log10 v) or one less
  if (k >= 0) gdv_big_pow10(s, k);
  else { gdv_big_pow10(r, -k); gdv_big_pow10(m, -k); }
  {  // the estimate was one too low when v + m+ reaches s
    gdv_big_add(r, m);
    if (closer_below) gdv_big_add(r, m);
    const gdv_int32 c = gdv_big_cmp(r, s);
    gdv_big_sub(r, m);
    if (closer_below) gdv_big_sub(r, m);
    if (even ? c >= 0 : c > 0) { k++; gdv_big_mul(s, 10u); }
  }
  gdv_real_digits out;
  out.digits = 0;
  out.nd = 0;
  out.k = k;
  for (;;) {
    gdv_big_mul(r, 10u);
    gdv_big_mul(m, 10u);
    gdv_int32 d = 0;
    while (d < 9 && gdv_big_cmp(r, s) >= 0) { gdv_big_sub(r, s); d++; }
    const gdv_int32 c1 = gdv_big_cmp(r, m);
    const bool tc1 = even ? c1 <= 0 : c1 < 0;  // the digits so far read back as f from below
    gdv_big_add(r, m);
    if (closer_below) gdv_big_add(r, m);
    const gdv_int32 c2 = gdv_big_cmp(r, s);
    gdv_big_sub(r, m);
    if (closer_below) gdv_big_sub(r, m);
    const bool tc2 = even ? c2 >= 0 : c2 > 0;  // ... with the last digit one up, from above
    if (!tc1 && !tc2 && out.nd < 17) {
      out.digits = out.digits * 10 + (gdv_uint64)d;
      out.nd++;
      continue;
    }
    if (tc1 && tc2) {  // both ends are in: the closer one; a tie goes to the even digit
      gdv_big_add(r, r);
      const gdv_int32 c = gdv_big_cmp(r, s);
      if (c > 0 || (c == 0 && (d & 1))) d++;
    } else if (tc2) {
      d++;
    }
    out.digits = out.digits * 10 + (gdv_uint64)d;
    out.nd++;
    break;
  }
  // (a final digit of 10 cannot happen — v + m+ < 10^k is the loop's invariant — but the integer form
  // absorbs it, and trailing zeros never survive)
  if (gdv_count_digits(out.digits) > out.nd) { out.k++; out.nd++; }
  while (out.digits != 0 && out.digits % 10 == 0) { out.digits /= 10; out.nd--; }
  return out;
}
GDV_DEV gdv_str gdv_real_view(gdv_ctx ctx, gdv_uint64 f, gdv_int32 e, bool closer_below, gdv_int32 neg, gdv_int32 kind, gdv_int64 n) {
  gdv_str r = gdv_empty_str();
  if (n < 0) { gdv_raise(ctx, GDV_ERR_BAD_ARG); return r; }
  gdv_real_digits d;
  d.digits = 0; d.nd = 0; d.k = 0;
  if (kind == 0) d = gdv_shortest_digits(f, e, closer_below);
  const gdv_uint64 info = (gdv_uint64)d.nd | ((gdv_uint64)(d.k + 2048) << 8) | ((gdv_uint64)neg << 24) | ((gdv_uint64)kind << 25);
  const gdv_int32 total = gdv_real_text_of(d.digits, info).len;
  r.p = (const gdv_uint8*)d.digits;
  r.lim = (const gdv_uint8*)info;
  r.len = n < total ? (gdv_int32)n : total;
  r.map = GDV_MAP_DIGITS;
  r.flags = GDV_STR_REAL;
  return r;
}
// castVARCHAR(float64 / float32, n): the shortest digits that read back as the value (of ITS type), in the
// Java-compatible layout above, cut to n bytes; n < 0 is an execution error
// [gdv_function_stubs.cc GDV_FN_CAST_VARCHAR_REAL over gandiva/formatting_utils.h, as recalled]
GDV_DEV gdv_str castVARCHAR_float64_int64(gdv_ctx ctx, gdv_float64 v, gdv_int64 n) {
  const gdv_uint64 b = (gdv_uint64)__double_as_longlong(v);
  const gdv_int32 ex = (gdv_int32)((b >> 52) & 2047);
  const gdv_uint64 mant = b & ((1ull << 52) - 1);
  const gdv_int32 kind = ex == 2047 ? (mant != 0 ? 3 : 2) : (ex == 0 && mant == 0 ? 1 : 0);
  return gdv_real_view(ctx, ex == 0 ? mant : (mant | (1ull << 52)), ex == 0 ? -1074 : ex - 1075, mant == 0 && ex > 1,
                       (gdv_int32)(b >> 63), kind, n);
}
GDV_DEV gdv_str castVARCHAR_float32_int64(gdv_ctx ctx, gdv_float32 v, gdv_int64 n) {
  const gdv_uint32 b = __float_as_uint(v);
  const gdv_int32 ex = (gdv_int32)((b >> 23) & 255);
  const gdv_uint32 mant = b & ((1u << 23) - 1);
  const gdv_int32 kind = ex == 255 ? (mant != 0 ? 3 : 2) : (ex == 0 && mant == 0 ? 1 : 0);
  return gdv_real_view(ctx, ex == 0 ? mant : (mant | (1u << 23)), ex == 0 ? -149 : ex - 150, mant == 0 && ex > 1,
                       (gdv_int32)(b >> 31), kind, n);
}
// ---- regexp_like / regexp_matches (round 5, late): does the text contain a match of the pattern?  The planner compiles the
// pattern to a position automaton of at most 63 positions whose edges carry GAP CONDITIONS (gdv_regex.h): what ^ $ \A \z \b \B
// ask of the gap between two bytes — conjunctions of 1 word boundary, 2 not a word boundary, 4 start of the text, 8 end of the
// text, at most 8 distinct ones per pattern (id 0 = none).  table (64-bit words) = flags | nullable | predicates[8] | first[8] |
// last[8] | follow[64][8] | match[256].  One 64-bit set of live positions per row: over the gap in front of byte b (the
// conditions it satisfies: `sat`) the set S becomes (first[c] | follow[p][c] for p in S, c in sat) & match[b]; a position of
// last[c], c satisfied by the gap behind the byte, ends a match.
GDV_DEV bool gdv_regex_word_byte(gdv_uint8 c) { return (c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '_'; }
GDV_DEV bool gdv_regex_search(const gdv_str& s, const gdv_uint8* table) {
  const gdv_uint64* t = (const gdv_uint64*)table;
  const gdv_uint32 used = (gdv_uint32)(t[0] >> 8) & 255u, nullable = (gdv_uint32)t[1];
  const bool start_only = (t[0] & 1) != 0;
  const gdv_uint64* preds = t + 2;
  const gdv_uint64* first = t + 10;
  const gdv_uint64* last = t + 18;
  const gdv_uint64* follow = t + 26;
  const gdv_uint64* match = t + 26 + 64 * 8;
  const gdv_int32 len = s.len > 0 ? s.len : 0;
  gdv_uint64 live = 0;
  bool prev_word = false;
  for (gdv_int32 i = 0; i <= len; i++) {
    // the gap in front of byte i (behind byte i - 1): its predicates, and the conditions of the pattern they satisfy.  RE2 looks
    // at BYTES here, and its search may begin at any byte: inside a multi-byte character (in front of a continuation byte) the
    // gap is "not a word boundary" for a match that BEGINS there, while a match under way — every atom consumes whole
    // characters — can neither end nor pass an assertion there
    const gdv_uint8 b = i < len ? gdv_str_at(s, i) : (gdv_uint8)0;
    const bool next_word = i < len && gdv_regex_word_byte(b);
    const bool inside = i < len && (b & 0xC0) == 0x80;
    const gdv_uint32 gap = (prev_word != next_word ? 1u : 2u) | (i == 0 ? 4u : 0u) | (i == len ? 8u : 0u);
    gdv_uint32 sat_new = 1u;
    for (gdv_uint32 w = used & ~1u; w != 0; w &= w - 1) {
      const int c = __builtin_ctz(w);
      if (((gdv_uint32)preds[c] & ~gap) == 0) sat_new |= 1u << c;
    }
    const gdv_uint32 sat_run = inside ? 1u : sat_new;
    // a match that ends here: the empty one, or a live position that may be left over this gap
    if ((nullable & sat_new) != 0) return true;
    gdv_uint64 ends = 0, next = 0;
    for (gdv_uint32 w = sat_run; w != 0; w &= w - 1) ends |= last[__builtin_ctz(w)];
    for (gdv_uint32 w = sat_new; w != 0; w &= w - 1) next |= first[__builtin_ctz(w)];
    if ((live & ends) != 0) return true;
    if (i == len) break;
    for (gdv_uint64 w = live; w != 0; w &= w - 1) {
      const gdv_uint64* f = follow + 8 * __builtin_ctzll(w);
      for (gdv_uint32 v = sat_run; v != 0; v &= v - 1) next |= f[__builtin_ctz(v)];
    }
    live = next & match[b];
    if (live == 0 && start_only) return false;  // nothing can begin behind the first byte
    prev_word = next_word;
  }
  return false;
}
// ---- regexp_extract(text, 'pattern', index): group `index` of the FIRST match RE2's unanchored search takes, as a narrower
// view of the text ("" without a match or when the group took no part).  The planner lays the pattern out as lists of ways
// in order of preference (gdv_regex.h, CompileRegexExtract): list p holds what may come behind position p, list 63 what may
// begin a match; a way = target (63: the match ends) | predicates of the gap << 6 | what happens to the group << 10.  The
// row keeps its live positions in that order, each with the extents of the group so far.  Over the gap in front of byte i
// every live position, most preferred first, offers its ways: a way whose predicates hold and whose target accepts the byte
// enters the next list unless a preferred one entered that target already; a way that ends the match records it and drops
// everything less preferred, the rest of its own list included.  While nothing has matched a new attempt joins at the end of
// the order (a later start is less preferred than any earlier one).  No backtracking: at most 63 entries per byte, each
// scanning one list.  The gap's predicates and the rule inside a multi-byte character are gdv_regex_search's: an attempt may
// begin there ("not a word boundary"), one under way passes no assertion there — and does not end there.
// Private state: the two lists (64 positions, 64 + 64 extents each: 1152 bytes of scratch per lane), nothing sized by the text.
GDV_DEV gdv_str gdv_regex_extract(gdv_str s, const gdv_uint8* table) {
  // the screen: regexp_like's table and walk (one 64-bit set per byte) come first; a row without a match is done
  if (!gdv_regex_search(s, table)) {
    s.len = 0;
    return s;
  }
  table += 6352;  // GDV_REGEX_TABLE_BYTES
  const gdv_uint64* t = (const gdv_uint64*)table;
  const bool start_only = (t[0] & 1) != 0;
  const gdv_uint64* match = t + 1;
  const gdv_uint64* targets = t + 257;
  const gdv_uint16* first = (const gdv_uint16*)(table + 2568);
  const gdv_uint16* ways = (const gdv_uint16*)(table + 2704);
  const gdv_int32 len = s.len > 0 ? s.len : 0;
  gdv_uint8 at[2][64];
  gdv_int32 from[2][64], to[2][64];
  gdv_int32 n = 0, cur = 0, found_from = -1, found_to = -1;
  bool found = false, prev_word = false;
  for (gdv_int32 i = 0; i <= len; i++) {
    const gdv_uint8 b = i < len ? gdv_str_at(s, i) : (gdv_uint8)0;
    const bool next_word = i < len && gdv_regex_word_byte(b);
    const bool inside = i < len && (b & 0xC0) == 0x80;
    const gdv_uint32 gap = (prev_word != next_word ? 1u : 2u) | (i == 0 ? 4u : 0u) | (i == len ? 8u : 0u);
    const gdv_uint32 run = inside ? 0u : gap;  // what a match under way may ask of this gap
    const gdv_uint64 fits = i < len ? match[b] : 0ull;
    const gdv_int32 nx = cur ^ 1;
    gdv_uint64 entered = 0;
    gdv_int32 m = 0;
    bool cut = false;
    // the live positions, then (k == n) a new attempt
    for (gdv_int32 k = 0; k <= n && !cut; k++) {
      const bool fresh = k == n;
      if (fresh && found) break;
      const gdv_int32 p = fresh ? 63 : (gdv_int32)at[cur][k];
      const gdv_uint32 may = fresh ? gap : run;
      const bool may_end = fresh || !inside;
      if ((targets[p] & ((fits & ~entered) | (may_end ? 1ull << 63 : 0ull))) == 0) continue;
      const gdv_int32 f0 = fresh ? -1 : from[cur][k], t0 = fresh ? -1 : to[cur][k];
      for (gdv_int32 e = first[p], e1 = first[p + 1]; e < e1; e++) {
        const gdv_uint32 w = ways[e];
        if ((((w >> 6) & 15u) & ~may) != 0) continue;
        const gdv_uint32 q = w & 63u, act = w >> 10;
        if (q != 63u && (((fits & ~entered) >> q) & 1ull) == 0) continue;
        if (q == 63u && !may_end) continue;
        const gdv_int32 f1 = act >= 2u ? i : f0;
        const gdv_int32 t1 = act == 2u ? -1 : act != 0u ? i : t0;
        if (q == 63u) {
          found = cut = true;
          found_from = f1;
          found_to = t1;
          break;
        }
        entered |= 1ull << q;
        at[nx][m] = (gdv_uint8)q;
        from[nx][m] = f1;
        to[nx][m] = t1;
        m++;
      }
    }
    n = m;
    cur = nx;
    if (n == 0 && (found || start_only)) break;  // settled, or nothing can begin behind the first gap
    prev_word = next_word;
  }
  if (found && found_from >= 0 && found_to >= found_from) {
    s.p += found_from;
    s.len = found_to - found_from;
  } else {
    s.len = 0;
  }
  return s;
}
// ---- to_date(text, 'pattern'[, suppress_errors]) (round 5).  The lineage's ToDateHolder turns the SQL pattern into a
// strptime format at Make time (date_utils.cc ToInternalFormat) and calls arrow::internal::ParseTimestampStrptime(...,
// ignore_time_in_day = true, allow_trailing_chars = true): the C library's strptime, then year / month / max(day, 1)
// through the civil-date arithmetic — the time fields are parsed, range-checked and dropped [as recalled].  Here the
// planner compiles the pattern to one byte per directive and the row interprets it the way glibc's strptime does:
//   ' '  any run of white space          'L' c  the byte c itself (text inside "double quotes" included)
//   'Y' 0..9999 (<= 4 digits)  'y' 0..99 (69-99 -> 19xx, else 20xx)  'm' 1..12  'd' 1..31  'j' 1..366 (<= 3 digits)
//   'H' 0..23  'I' 1..12  'M' 0..59  'S' 0..61          numbers: blanks skipped, at least one digit, further digits
//   'b' month name, 'a' weekday name (English, full or 3 letters, any case)  'p' AM / PM       while value * 10 <= max
// A text that does not match raises (suppress_errors = 0) or gives null (1).
GDV_DEV bool gdv_c_isspace(gdv_uint8 c) { return c == ' ' || (c >= 9 && c <= 13); }
GDV_DEV bool gdv_scan_number(const gdv_str& s, gdv_int32& i, gdv_int32 from, gdv_int32 to, gdv_int32 n, gdv_int32* val) {
  while (i < s.len && gdv_c_isspace(gdv_str_at(s, i))) i++;
  if (i >= s.len) return false;
  gdv_uint8 c = gdv_str_at(s, i);
  if (c < '0' || c > '9') return false;
  gdv_int32 v = 0;
  for (;;) {
    v = v * 10 + (c - '0');
    i++;
    if (--n <= 0 || v * 10 > to || i >= s.len) break;
    c = gdv_str_at(s, i);
    if (c < '0' || c > '9') break;
  }
  *val = v;
  return v >= from && v <= to;
}
// a name out of `count`: three letters packed low byte first in abbr[], the rest of the full name in rest[] (<= 6 letters);
// the full name is taken when all of it is there, else the three letters (glibc tries them in that order)
GDV_DEV gdv_int32 gdv_scan_name(const gdv_str& s, gdv_int32& i, const gdv_uint32* abbr, const gdv_uint64* rest, gdv_int32 count) {
  if (i + 3 > s.len) return -1;
  gdv_uint32 w = 0;
  for (gdv_int32 j = 0; j < 3; j++) w |= (gdv_uint32)(gdv_str_at(s, i + j) | 0x20) << (8 * j);
  for (gdv_int32 k = 0; k < count; k++) {
    if (abbr[k] != w) continue;
    gdv_int32 j = 0;
    bool full = true;
    for (gdv_uint64 r = rest[k]; r != 0; r >>= 8, j++)
      if (i + 3 + j >= s.len || (gdv_uint8)(gdv_str_at(s, i + 3 + j) | 0x20) != (gdv_uint8)r) { full = false; break; }
    i += 3 + (full ? j : 0);
    return k;
  }
  return -1;
}
GDV_DEV gdv_int64 gdv_parse_date(gdv_ctx ctx, gdv_str s, const gdv_uint8* ops, gdv_int32 nops, gdv_int32 suppress, bool in_valid,
                                 bool* out_valid) {
  *out_valid = false;
  if (!in_valid) return 0;
  const gdv_uint32 mon3[12] = {0x6e616a, 0x626566, 0x72616d, 0x727061, 0x79616d, 0x6e756a, 0x6c756a, 0x677561, 0x706573, 0x74636f, 0x766f6e, 0x636564};
  const gdv_uint64 monr[12] = {0x79726175ull, 0x7972617572ull, 0x6863ull, 0x6c69ull, 0ull, 0x65ull, 0x79ull, 0x747375ull, 0x7265626d6574ull, 0x7265626full,
                               0x7265626d65ull, 0x7265626d65ull};
  const gdv_uint32 day3[7] = {0x6e7573, 0x6e6f6d, 0x657574, 0x646577, 0x756874, 0x697266, 0x746173};
  const gdv_uint64 dayr[7] = {0x796164ull, 0x796164ull, 0x79616473ull, 0x79616473656eull, 0x7961647372ull, 0x796164ull, 0x7961647275ull};
  gdv_int32 year = 1900, mon = 1, mday = 0, yday = -1, i = 0, v = 0;
  bool ok = true, have_mon = false, have_mday = false, have_wday = false, want_xday = false;  // (glibc's names)
  for (gdv_int32 op = 0; ok && op < nops; op++) {
    const gdv_uint8 c = ops[op];
    if (c == ' ') { while (i < s.len && gdv_c_isspace(gdv_str_at(s, i))) i++; }
    else if (c == 'L') { op++; ok = i < s.len && gdv_str_at(s, i) == ops[op]; i++; }
    else if (c == 'Y') { ok = gdv_scan_number(s, i, 0, 9999, 4, &v); year = v; want_xday = true; }
    else if (c == 'y') { ok = gdv_scan_number(s, i, 0, 99, 2, &v); year = v >= 69 ? 1900 + v : 2000 + v; want_xday = true; }
    else if (c == 'm') { ok = gdv_scan_number(s, i, 1, 12, 2, &v); mon = v; have_mon = true; want_xday = true; }
    else if (c == 'd') { ok = gdv_scan_number(s, i, 1, 31, 2, &v); mday = v; have_mday = true; want_xday = true; }
    else if (c == 'j') { ok = gdv_scan_number(s, i, 1, 366, 3, &v); yday = v - 1; }
    else if (c == 'H') ok = gdv_scan_number(s, i, 0, 23, 2, &v);
    else if (c == 'I') ok = gdv_scan_number(s, i, 1, 12, 2, &v);
    else if (c == 'M') ok = gdv_scan_number(s, i, 0, 59, 2, &v);
    else if (c == 'S') ok = gdv_scan_number(s, i, 0, 61, 2, &v);
    else if (c == 'b') { v = gdv_scan_name(s, i, mon3, monr, 12); ok = v >= 0; mon = v + 1; have_mon = true; want_xday = true; }
    else if (c == 'a') { ok = gdv_scan_name(s, i, day3, dayr, 7) >= 0; have_wday = true; }
    else if (c == 'p') {
      ok = i + 2 <= s.len && (gdv_str_at(s, i + 1) | 0x20) == 'm' && ((gdv_str_at(s, i) | 0x20) == 'a' || (gdv_str_at(s, i) | 0x20) == 'p');
      i += 2;
    } else ok = false;
  }
  if (!ok) {
    if (!suppress) gdv_raise(ctx, GDV_ERR_BAD_ARG);
    return 0;
  }
  *out_valid = true;
  if (yday >= 0 && want_xday && !have_wday && !(have_mon && have_mday)) {
    // a day of the year fills in the month and / or the day of the month that the text did not give — glibc's strptime does
    // this itself, when a year / month / day directive asked for a calendar date at all and no weekday name was parsed
    const bool leap = (year % 4 == 0) && (year % 100 != 0 || year % 400 == 0);
    gdv_int32 t_mon = 1, first = 0;  // month t_mon starts at day-of-year `first`
    for (; t_mon < 12; t_mon++) {
      const gdv_int32 len = t_mon == 2 ? (leap ? 29 : 28) : (t_mon == 4 || t_mon == 6 || t_mon == 9 || t_mon == 11) ? 30 : 31;
      if (first + len > yday) break;
      first += len;
    }
    if (!have_mon) mon = t_mon;
    if (!have_mday) mday = yday - first + 1;
  }
  return gdv_days_from_civil(year, mon, mday < 1 ? 1 : mday) * GDV_MILLIS_IN_DAY;
}
// to_timestamp / to_time over numbers: seconds since the epoch -> milliseconds (time: of the day) [time.cc TO_TIMESTAMP /
// TO_TIME, as recalled: static_cast<int64>(seconds * MILLIS_IN_SEC), % MILLIS_IN_DAY]
#define GDV_TO_TIMESTAMP(T)                                                                                        \
  GDV_DEV gdv_int64 to_timestamp_##T(gdv_##T seconds) { return gdv_seconds_to_millis(seconds); }            \
  GDV_DEV gdv_int32 to_time_##T(gdv_##T seconds) { return (gdv_int32)(gdv_seconds_to_millis(seconds) % GDV_MILLIS_IN_DAY); }
GDV_DEV gdv_int64 gdv_seconds_to_millis(gdv_int32 s) { return (gdv_int64)s * 1000; }
GDV_DEV gdv_int64 gdv_seconds_to_millis(gdv_int64 s) { return (gdv_int64)((gdv_uint64)s * 1000ull); }
GDV_DEV gdv_int64 gdv_seconds_to_millis(gdv_float32 s) { return gdv_sat_i64((gdv_float64)(s * 1000.0f)); }
GDV_DEV gdv_int64 gdv_seconds_to_millis(gdv_float64 s) { return gdv_sat_i64(s * 1000.0); }
GDV_TO_TIMESTAMP(int32)
GDV_TO_TIMESTAMP(int64)
GDV_TO_TIMESTAMP(float32)
GDV_TO_TIMESTAMP(float64)
// reverse(s): the characters of s in reverse order.  A character is what its lead byte announces
// (1-4 bytes); a byte that cannot lead a character, or a character cut by the end of the string,
// is an execution error.
GDV_DEV gdv_str reverse_utf8(gdv_ctx ctx, gdv_str s) {
  if (!gdv_str_is_ascii(s)) {
    for (gdv_int32 i = 0; i < s.len;) {
      const gdv_int32 cl = gdv_utf8_declared_len(s.p[i]);
      if (cl == 0 || i + cl > s.len) { gdv_raise(ctx, GDV_ERR_BAD_ARG); s.len = 0; break; }
      i += cl;
    }
  }
  s.map |= GDV_MAP_REVERSE;
  return s;
}

// hashSHA256 / hashSHA1 / hashMD5 (and their sha256 / sha1 / sha / md5 aliases): a view whose text the output copy
// computes.  Never null: a NULL argument is the empty message.
GDV_DEV gdv_str gdv_digest_of_str(gdv_str s, bool valid, int algo) {
  gdv_str r = s;
  r.lead_p = s.p;
  r.lead = valid && s.len > 0 ? (gdv_uint64)s.len : 0ull;
  r.p = nullptr;
  r.len = algo == 0 ? 64 : algo == 1 ? 40 : 32;
  r.map = GDV_MAP_DIGEST | (algo << 8) | (s.map & GDV_MAP_CASE);
  return r;
}
GDV_DEV gdv_str gdv_digest_of_f64(gdv_float64 v, bool valid, int algo) {
  gdv_str r = gdv_empty_str();
  r.lead_p = nullptr;
  r.lead = 0;
  r.len = algo == 0 ? 64 : algo == 1 ? 40 : 32;
  r.map = GDV_MAP_DIGEST | (algo << 8);
  if (valid) {
    __builtin_memcpy(&r.lead, &v, 8);
    r.map |= 1024;
  }
  return r;
}
#define GDV_DIGEST_FNS(NAME, ALGO)                                                                                   \
  GDV_DEV gdv_str NAME##_utf8(gdv_str s, bool valid) { return gdv_digest_of_str(s, valid, ALGO); }                     \
  GDV_DEV gdv_str NAME##_binary(gdv_str s, bool valid) { return gdv_digest_of_str(s, valid, ALGO); }                   \
  GDV_DEV gdv_str NAME##_int32(gdv_int32 v, bool valid) { return gdv_digest_of_f64((gdv_float64)v, valid, ALGO); }     \
  GDV_DEV gdv_str NAME##_int64(gdv_int64 v, bool valid) { return gdv_digest_of_f64((gdv_float64)v, valid, ALGO); }     \
  GDV_DEV gdv_str NAME##_float32(gdv_float32 v, bool valid) { return gdv_digest_of_f64((gdv_float64)v, valid, ALGO); } \
  GDV_DEV gdv_str NAME##_float64(gdv_float64 v, bool valid) { return gdv_digest_of_f64(v, valid, ALGO); }
GDV_DIGEST_FNS(hashSHA256, 0)
GDV_DIGEST_FNS(hashSHA1, 1)
GDV_DIGEST_FNS(hashMD5, 2)
GDV_DEV gdv_str initcap_utf8(gdv_str s) {
  s.map |= GDV_MAP_INITCAP;
  return s;
}
// replace(s, from, to) with literal from / to (table in the constant block): every occurrence of
// `from`, found left to right without overlap, becomes `to`.  An empty s or from leaves s as it
// is; a result longer than 65535 bytes is an execution error.
GDV_DEV gdv_str gdv_replace(gdv_ctx ctx, gdv_str s, const gdv_uint8* desc) {
  const gdv_int32 fl = ((const gdv_int32*)desc)[0], tl = ((const gdv_int32*)desc)[1];
  if (s.len <= 0 || fl <= 0) return s;
  const gdv_int32 cm = s.map & GDV_MAP_CASE;
  gdv_int32 hits = 0;
  if (s.flags & GDV_STR_INBUF) {
    for (gdv_int32 i = gdv_find_raw(s.p, s.len, cm, 0, desc + 16, fl); i >= 0;
         i = gdv_find_raw(s.p, s.len, cm, i + fl, desc + 16, fl))
      hits++;
  } else {
    for (gdv_int32 i = 0; i + fl <= s.len;) {
      if (gdv_replace_match(s.p, i, s.len, cm, desc + 16, fl)) { hits++; i += fl; } else { i++; }
    }
  }
  if (hits == 0) return s;
  const gdv_int64 out = (gdv_int64)s.len + (gdv_int64)hits * (tl - fl);
  // (the view packs the source length into 30 bits of `flags`: a row of 512 MiB or more cannot be
  // described even when the replacements shrink it below the 65535-byte result limit)
  if (out > 65535 || s.len >= (1 << 29)) { gdv_raise(ctx, GDV_ERR_BAD_ARG); s.len = 0; return s; }
  s.flags = (s.flags & 3) | (s.len << 2);
  s.lim = desc;
  s.len = (gdv_int32)out;
  s.map |= GDV_MAP_REPLACE;
  return s;
}
// replace(s, from, to) with from / to that are not literals (round 5): the same rule, the arguments read through their own
// views.  A `from` of more than 65535 bytes that does occur in s cannot be described by the view: execution error.
GDV_DEV gdv_str gdv_replace_row(gdv_ctx ctx, gdv_str s, const gdv_str& from, const gdv_str& to) {
  if (s.len <= 0 || from.len <= 0 || from.len > s.len) return s;
  const gdv_int32 cm = s.map & GDV_MAP_CASE, fm = from.map & GDV_MAP_CASE;
  gdv_int32 hits = 0;
  for (gdv_int32 i = 0; i + from.len <= s.len;) {
    if (gdv_match_row(s.p, i, s.len, cm, from.p, from.len, fm)) { hits++; i += from.len; } else { i++; }
  }
  if (hits == 0) return s;
  const gdv_int64 out = (gdv_int64)s.len + (gdv_int64)hits * (to.len - from.len);
  if (out > 65535 || from.len > 65535) { gdv_raise(ctx, GDV_ERR_BAD_ARG); s.len = 0; return s; }
  s.lead = (gdv_uint64)(gdv_uint32)s.len | ((gdv_uint64)from.len << 32) | ((gdv_uint64)to.len << 48);  // (out <= 65535 with at least one hit bounds to.len by 65535 as well)
  s.lim = from.p;
  s.lead_p = to.p;
  s.flags = (fm << 8) | ((to.map & GDV_MAP_CASE) << 10);
  s.len = (gdv_int32)out;
  s.map = cm | GDV_MAP_REPLACE_ROW;
  return s;
}
// lpad / rpad(text, n, fill) with n or fill not a literal (round 5): the fill's characters, cyclically, up to n - chars(text)
// of them — whole repetitions and then a prefix, which in bytes is simply the fill's bytes read cyclically.  "" when nothing
// is to be added (an empty text, n <= 0, an empty fill, a text of n characters or more); more than 65536 characters: error.
GDV_DEV gdv_str gdv_pad_fill_row(gdv_ctx ctx, const gdv_str& s, gdv_int32 n, const gdv_str& fill) {
  gdv_str r = gdv_empty_str();
  if (s.len <= 0 || n <= 0 || fill.len <= 0) return r;
  const gdv_int32 pad = n - gdv_utf8_count(s);
  if (pad <= 0) return r;
  if (n > (1 << 16)) { gdv_raise(ctx, GDV_ERR_BAD_ARG); return r; }
  gdv_int32 fchars = gdv_utf8_count(fill);
  if (fchars <= 0) fchars = 1;
  const gdv_int32 reps = pad / fchars, part = pad - reps * fchars;
  r = fill;
  r.flags &= ~GDV_STR_LEAD;
  r.lead = (gdv_uint64)fill.len;
  r.len = reps * fill.len + (part > 0 ? gdv_utf8_byte_pos(fill, part) : 0);
  r.map = (fill.map & GDV_MAP_CASE) | GDV_MAP_CYCLE;
  return r;
}
// ---- replace() answered by the byte sweep (round 3).  Kernels whose replace() takes a whole
// column row and a 'from' of 2..8 bytes that cannot overlap itself let the sweep mark every
// match position of the sub-tile's span in the LDS bitmap the '%needle%' predicate uses; a row
// then COUNTS its matches with a popcount over its own bit range (no search loop: the per-row
// SWAR search made replace the most instruction-hungry function of the library, ~1000 VALU per
// 64 rows), and the copy walks the set bits.  Matches cannot overlap, so every marked position
// is a replacement, left to right.
#define GDV_MAP_HITS 32  // a GDV_MAP_REPLACE value whose matches are marked in the sweep's bitmap
// set bits in [lo, hi) of the bitmap (readable one word past any position)
GDV_DEV gdv_int32 gdv_range_count(const gdv_uint64* bm, gdv_int32 lo, gdv_int32 hi) {
  gdv_int32 cnt = 0;
  for (gdv_int32 p = lo; p < hi; p += 64) {
    const gdv_int32 w = p >> 6, sh = p & 63;
    gdv_uint64 x = (bm[w] >> sh) | ((bm[w + 1] << 1) << (63 - sh));  // positions p .. p+63
    const gdv_int32 left = hi - p;
    if (left < 64) x &= (1ull << left) - 1ull;
    cnt += (gdv_int32)__builtin_popcountll(x);
  }
  return cnt;
}
// the first set bit in [p, hi), or -1
GDV_DEV gdv_int32 gdv_range_next(const gdv_uint64* bm, gdv_int32 p, gdv_int32 hi) {
  for (; p < hi; p += 64) {
    const gdv_int32 w = p >> 6, sh = p & 63;
    gdv_uint64 x = (bm[w] >> sh) | ((bm[w + 1] << 1) << (63 - sh));
    const gdv_int32 left = hi - p;
    if (left < 64) x &= (1ull << left) - 1ull;
    if (x != 0) return p + (gdv_int32)__builtin_ctzll(x);
  }
  return -1;
}
// gdv_replace with the matches counted in the bitmap: bit `lo` = the row's first byte
GDV_DEV gdv_str gdv_replace_hits(gdv_ctx ctx, gdv_str s, const gdv_uint8* desc, const gdv_uint64* bm, gdv_int32 lo) {
  const gdv_int32 fl = ((const gdv_int32*)desc)[0], tl = ((const gdv_int32*)desc)[1];
  if (s.len <= 0 || fl <= 0) return s;
  const gdv_int32 hits = gdv_range_count(bm, lo, lo + s.len - fl + 1);
  if (hits == 0) return s;
  const gdv_int64 out = (gdv_int64)s.len + (gdv_int64)hits * (tl - fl);
  if (out > 65535 || s.len >= (1 << 29)) { gdv_raise(ctx, GDV_ERR_BAD_ARG); s.len = 0; return s; }
  s.flags = (s.flags & 3) | (s.len << 2);
  s.lim = desc;
  s.len = (gdv_int32)out;
  s.map |= GDV_MAP_REPLACE | GDV_MAP_HITS;
  return s;
}
// 8 raw bytes at offset k of a row in HBM (the LDS reader lives with the LDS mirror below)
struct gdv_rd_hbm {
  const gdv_uint8* p;
  __device__ __forceinline__ gdv_uint64 operator()(gdv_int32 k) const { return gdv_load8_raw(p + k); }
};
// the copy of such a value: the stretches between the marked positions, `to` at each of them.
// rd(k) = 8 raw bytes at offset k of the SOURCE row (up to 7 bytes past the row may be read,
// never used); bit `lo` of the bitmap = the row's first byte.
template <typename P, typename R>
GDV_DEV void gdv_copy_replaced_hits(P dst, const gdv_str& s, R rd, const gdv_uint64* bm, gdv_int32 lo) {
  const gdv_uint8* desc = s.lim;
  const gdv_int32 fl = ((const gdv_int32*)desc)[0], tl = ((const gdv_int32*)desc)[1];
  const gdv_uint8* to = desc + 16 + ((fl + 15) & ~15);
  const gdv_int32 len = s.flags >> 2, cm = s.map & GDV_MAP_CASE;
  const gdv_int32 hi = lo + len - fl + 1;
  gdv_int32 o = 0;
  for (gdv_int32 pos = 0;;) {
    const gdv_int32 j = gdv_range_next(bm, lo + pos, hi);
    const gdv_int32 stop = j < 0 ? len : j - lo;
    gdv_int32 k = pos;
    for (; k + 8 <= stop; k += 8, o += 8) {
      const gdv_uint64 w = gdv_map8(rd(k), cm);
      __builtin_memcpy(dst + o, &w, 8);
    }
    if (k < stop) {
      gdv_store_low_bytes(dst + o, gdv_map8(rd(k), cm), stop - k);
      o += stop - k;
    }
    if (j < 0) break;
    gdv_int32 t = 0;
    for (; t + 8 <= tl; t += 8, o += 8) {
      const gdv_uint64 w = gdv_load8_raw(to + t);
      __builtin_memcpy(dst + o, &w, 8);
    }
    if (t < tl) {
      gdv_store_low_bytes(dst + o, gdv_load8_raw(to + t), tl - t);
      o += tl - t;
    }
    pos = stop + fl;
  }
}
// lpad / rpad(text, n, fill): the result is two pieces, written back to back by the output copy —
// the text cut to n characters, and the first n - chars(text) characters of `tab` = fill repeated
// to n characters (n and fill are literals: the planner lays the table out in the constant
// block).  An empty text or n <= 0 gives "", an empty fill leaves the text as it is.
GDV_DEV gdv_str gdv_pad_text(gdv_str s, gdv_int32 n) {
  if (s.len <= 0 || n <= 0) { s.len = 0; return s; }
  if (n < s.len) s.len = gdv_utf8_byte_pos(s, n);  // (n >= bytes >= characters: nothing to cut)
  return s;
}
GDV_DEV gdv_str gdv_pad_fill(const gdv_str& s, gdv_int32 n, const gdv_uint8* tab, gdv_int32 tab_len,
                             bool tab_ascii) {
  gdv_str r = gdv_make_str(tab, 0, 0, tab + tab_len + 8, GDV_STR_INBUF | (tab_ascii ? GDV_STR_ASCII : 0));
  if (s.len <= 0 || n <= 0 || tab_len == 0) return r;
  const gdv_int32 pad = n - gdv_utf8_count(s);
  if (pad <= 0) return r;
  r.len = tab_len;
  r.len = gdv_utf8_byte_pos(r, pad);
  return r;
}
// byte position of the first occurrence of `sub` (non-empty) in `s` at or after byte `from`, -1 when
// absent: 8 candidate positions per step, filtered on the first two needle bytes with SWAR
// zero-byte tests, verified on a 64-bit window (the scheme of gdv_like_contains below, with the
// needle read through its own view)
static __device__ GDV_COLD gdv_int32 gdv_find(const gdv_str& s, gdv_int32 from, const gdv_str& sub) {
  const gdv_int32 m = sub.len, last = s.len - m;
  if (from > last) return -1;
  const gdv_uint64 mask = gdv_low_bytes_mask(m);
  const gdv_uint64 first = gdv_word_at(sub, 0) & mask;
  const gdv_uint64 splat = (first & 0xffull) * 0x0101010101010101ull;
  const gdv_uint64 splat2 = ((first >> 8) & 0xffull) * 0x0101010101010101ull;
  gdv_uint64 cur = gdv_word_at(s, from);
  for (gdv_int32 base = from; base <= last; base += 8) {
    const gdv_uint64 nxt = (base + 8 < s.len) ? gdv_word_at(s, base + 8) : 0ull;
    const gdv_uint64 x = cur ^ splat;
    gdv_uint64 cand = (x - 0x0101010101010101ull) & ~x & 0x8080808080808080ull;
    if (m >= 2) {
      const gdv_uint64 y = ((cur >> 8) | (nxt << 56)) ^ splat2;
      cand &= (y - 0x0101010101010101ull) & ~y & 0x8080808080808080ull;
    }
    while (cand) {
      const int k = __builtin_ctzll(cand) >> 3;
      cand &= cand - 1;
      if (base + k > last) break;
      const gdv_uint64 win = k == 0 ? cur : ((cur >> (8 * k)) | (nxt << (64 - 8 * k)));
      bool eq = (win & mask) == first;
      for (gdv_int32 j = 8; eq && j < m; j += 8)
        eq = ((gdv_word_at(s, base + k + j) ^ gdv_word_at(sub, j)) & gdv_low_bytes_mask(m - j)) == 0;
      if (eq) return base + k;
    }
    cur = nxt;
  }
  return -1;
}
// locate(sub, str[, start]): 1-based character position of the first occurrence of sub in
// str at or after character `start`; 0 when absent or when either string is empty
GDV_DEV gdv_int32 locate_utf8_utf8_int32(gdv_ctx ctx, gdv_str sub, gdv_str str, gdv_int32 start) {
  if (start < 1) { gdv_raise(ctx, GDV_ERR_BAD_ARG); return 0; }
  if (str.len <= 0 || sub.len <= 0) return 0;
  const gdv_int32 at = gdv_find(str, gdv_utf8_byte_pos(str, start - 1), sub);
  if (at < 0) return 0;
  gdv_str head = str;
  head.len = at;
  return gdv_utf8_count(head) + 1;
}
GDV_DEV gdv_int32 locate_utf8_utf8(gdv_ctx ctx, gdv_str sub, gdv_str str) {
  return locate_utf8_utf8_int32(ctx, sub, str, 1);
}
GDV_DEV gdv_int32 strpos_utf8_utf8(gdv_ctx ctx, gdv_str str, gdv_str sub) {
  return locate_utf8_utf8_int32(ctx, sub, str, 1);
}
// castINT / castBIGINT from text: blanks trimmed on both sides, then what Arrow's integer parser
// takes (arrow::internal::ParseValue, the primitive the reference's gdv_fn_cast*_utf8 stubs call;
// pyarrow/include/arrow/util/value_parsing.h:380-440): "0x" / "0X" + 1 .. 2*sizeof(T) hexadecimal
// digits, read as the type's bit pattern ("0xFFFFFFFF" is -1 as int32) — or an optional '-' and
// one or more decimal digits that fit the type.  Anything else is an execution error (the
// reference: "Failed to cast the string ... to int32").  `hex_digits` = 2 * sizeof(T).
GDV_DEV bool gdv_parse_int64(const gdv_str& s, gdv_int64 min_value, gdv_int64 max_value, gdv_int32 hex_digits,
                             gdv_int64* out) {
  gdv_int32 lo = 0, hi = s.len;
  while (lo < hi && gdv_str_at(s, lo) == ' ') lo++;
  while (hi > lo && gdv_str_at(s, hi - 1) == ' ') hi--;
  if (hi - lo > 2 && gdv_str_at(s, lo) == '0' && (gdv_str_at(s, lo + 1) | 0x20) == 'x') {
    lo += 2;
    if (hi - lo > hex_digits) return false;
    gdv_uint64 acc = 0;
    for (gdv_int32 i = lo; i < hi; i++) {
      const gdv_int32 c = gdv_str_at(s, i);
      gdv_int32 d;
      if (c >= '0' && c <= '9') d = c - '0';
      else if (c >= 'A' && c <= 'F') d = c - 'A' + 10;
      else if (c >= 'a' && c <= 'f') d = c - 'a' + 10;
      else return false;
      acc = (acc << 4) | (gdv_uint64)d;
    }
    // the unsigned image of the type's width, reinterpreted
    *out = hex_digits == 8 ? (gdv_int64)(gdv_int32)(gdv_uint32)acc : (gdv_int64)acc;
    return true;
  }
  bool neg = false;
  if (lo < hi && gdv_str_at(s, lo) == '-') { neg = true; lo++; }
  if (lo >= hi) return false;
  // accumulate as a NEGATIVE number so that the most negative value parses without overflow
  gdv_int64 acc = 0;
  const gdv_int64 floor_value = neg ? min_value : -max_value;
  for (gdv_int32 i = lo; i < hi; i++) {
    const gdv_int32 d = (gdv_int32)gdv_str_at(s, i) - '0';
    if (d < 0 || d > 9) return false;
    if (acc < (floor_value + d) / 10) return false;  // acc * 10 - d would pass the floor
    acc = acc * 10 - d;
  }
  *out = neg ? acc : -acc;
  return true;
}
GDV_DEV gdv_int64 castBIGINT_utf8(gdv_ctx ctx, gdv_str s) {
  gdv_int64 v = 0;
  if (!gdv_parse_int64(s, (gdv_int64)(-9223372036854775807LL - 1), 9223372036854775807LL, 16, &v)) {
    gdv_raise(ctx, GDV_ERR_BAD_ARG);
    return 0;
  }
  return v;
}
GDV_DEV gdv_int32 castINT_utf8(gdv_ctx ctx, gdv_str s) {
  gdv_int64 v = 0;
  if (!gdv_parse_int64(s, -2147483648LL, 2147483647LL, 8, &v)) {
    gdv_raise(ctx, GDV_ERR_BAD_ARG);
    return 0;
  }
  return (gdv_int32)v;
}
// castDECIMAL from text: [+-]? ( D+ ( '.' D* )? | '.' D+ ) ( [eE] [+-]? D+ )? over ASCII digits, nothing trimmed — the accept
// set of arrow::Decimal128::FromString, the parser the lineage calls; decided here: an exponent of more than 9 digits and a
// second sign in it ("1e+-5") are refused.  The value is the EXACT decimal value of the text rounded half away from zero to
// `os` fractional digits; more than `op` digits: 0, no error.  128-bit arithmetic, whatever the text's length: a first walk
// checks the grammar and finds the exponent (so a bad byte raises wherever it stands), a second one accumulates the digits
// of weight >= 10^-os; the first dropped digit alone decides the rounding (half-away ties round up).
GDV_DEV bool gdv_parse_decimal(const gdv_str& s, int op, int os, gdv_int128* out) {
  const gdv_int32 n = s.len;
  gdv_int32 i = 0;
  bool neg = false;
  if (i < n && (gdv_str_at(s, i) == '+' || gdv_str_at(s, i) == '-')) { neg = gdv_str_at(s, i) == '-'; i++; }
  const gdv_int32 int_begin = i;
  while (i < n && (gdv_uint8)(gdv_str_at(s, i) - '0') <= 9) i++;
  const gdv_int32 int_end = i;
  gdv_int32 frac_begin = i, frac_end = i;
  if (i < n && gdv_str_at(s, i) == '.') {
    i++;
    frac_begin = i;
    while (i < n && (gdv_uint8)(gdv_str_at(s, i) - '0') <= 9) i++;
    frac_end = i;
  }
  if (int_end == int_begin && frac_end == frac_begin) return false;  // no digit: "", ".", "+", ".e5"
  gdv_int64 exp10 = 0;
  if (i < n && (gdv_str_at(s, i) | 0x20) == 'e') {
    i++;
    bool eneg = false;
    if (i < n && (gdv_str_at(s, i) == '+' || gdv_str_at(s, i) == '-')) { eneg = gdv_str_at(s, i) == '-'; i++; }
    const gdv_int32 e_begin = i;
    while (i < n && (gdv_uint8)(gdv_str_at(s, i) - '0') <= 9) { exp10 = exp10 * 10 + (gdv_str_at(s, i) - '0'); i++; if (i - e_begin > 9) return false; }
    if (i == e_begin) return false;
    if (eneg) exp10 = -exp10;
  }
  if (i != n) return false;
  // digit k of the run (integer digits, then fraction digits) has weight 10^(int_digits - 1 - k + exp10)
  const gdv_int64 int_digits = int_end - int_begin;
  const gdv_int32 total = (int_end - int_begin) + (frac_end - frac_begin);
  const gdv_uint128 top = (gdv_uint128)gdv_pow10_128(37);
  gdv_uint128 acc = 0;  // < 10^38 throughout
  bool over = false;
  gdv_int64 w = int_digits - 1 + exp10;  // weight of the digit at hand
  for (gdv_int32 k = 0; k < total; k++, w--) {
    if (w < -(gdv_int64)os - 1) break;  // below the rounding digit: cannot change the result
    const gdv_int32 at = k < int_end - int_begin ? int_begin + k : frac_begin + (k - (int_end - int_begin));
    const gdv_uint32 d = (gdv_uint32)(gdv_str_at(s, at) - '0');
    if (w == -(gdv_int64)os - 1) {
      if (d >= 5 && !over) acc += 1;
      break;
    }
    if (acc >= top) over = true;  // one more digit makes 39
    if (!over) acc = acc * 10 + d;
  }
  // digits end above 10^-os ("12e3" at scale 2): the zeros that follow
  const gdv_int64 last_w = int_digits - (gdv_int64)total + exp10;  // weight of the last digit
  gdv_int128 r = 0;
  if (!over && acc != 0) {
    const gdv_int64 by = last_w + os > 0 ? last_w + os : 0;
    if (by > op || acc >= (gdv_uint128)gdv_pow10_128(op - (int)by)) over = true;
    else r = (gdv_int128)(acc * (gdv_uint128)gdv_pow10_128((int)by));
  }
  *out = over ? (gdv_int128)0 : (neg ? -r : r);
  return true;
}
GDV_DEV gdv_int128 castDECIMAL_utf8(gdv_ctx ctx, gdv_str s, int op, int os) {
  gdv_int128 v = 0;
  if (!gdv_parse_decimal(s, op, os, &v)) {
    gdv_raise(ctx, GDV_ERR_BAD_ARG);
    return 0;
  }
  return v;
}
// ascii(s): the first byte as a signed char (0 for the empty string)
GDV_DEV gdv_int32 ascii_utf8(gdv_str s) { return s.len > 0 ? (gdv_int32)(gdv_int8)gdv_str_at(s, 0) : 0; }

GDV_DEV bool gdv_is_space(gdv_uint8 c) { return c == ' '; }
GDV_DEV gdv_str ltrim_utf8(gdv_str s) {
  while (s.len > 0 && gdv_is_space(s.p[0])) { s.p++; s.len--; }
  return s;
}
GDV_DEV gdv_str rtrim_utf8(gdv_str s) {
  while (s.len > 0 && gdv_is_space(s.p[s.len - 1])) s.len--;
  return s;
}
GDV_DEV gdv_str btrim_utf8(gdv_str s) { return rtrim_utf8(ltrim_utf8(s)); }

// SQL LIKE.  The pattern is compiled at Make time (gdv_codegen_functions.cc, CompileLike) into parallel arrays in
// constant memory: kind[i] = 0 literal byte, 1 '_' (exactly one UTF-8 character),
// 2 '%' (any run, possibly empty); byte[i] = the literal.  Matching is the classic
// two-cursor wildcard walk with a single backtrack point (the last '%'): O(len * plen) worst
// case, O(len) for the usual '%needle%' / 'prefix%' shapes.  The whole string must match.
static __device__ GDV_COLD bool gdv_like(const gdv_str& s, const gdv_uint8* pbyte, const gdv_uint8* pkind, gdv_int32 plen) {
  gdv_int32 i = 0, j = 0, star_j = -1, star_i = 0;
  while (i < s.len) {
    if (j < plen && pkind[j] == 2) {
      star_j = j++;
      star_i = i;
    } else if (j < plen && pkind[j] == 1) {
      i++;
      while (i < s.len && !gdv_is_utf8_lead(s.p[i])) i++;  // swallow continuation bytes
      j++;
    } else if (j < plen && pkind[j] == 0 && gdv_str_at(s, i) == pbyte[j]) {
      i++;
      j++;
    } else if (star_j >= 0) {
      j = star_j + 1;
      star_i++;
      while (star_i < s.len && !gdv_is_utf8_lead(s.p[star_i])) star_i++;
      i = star_i;
    } else {
      return false;
    }
  }
  while (j < plen && pkind[j] == 2) j++;
  return j == plen;
}

// LIKE shapes the planner recognises at Make time and routes around the general matcher:
//   'literal'      -> gdv_like_equal       'literal%'  -> gdv_like_prefix
//   '%literal'     -> gdv_like_suffix      '%literal%' -> gdv_like_contains
// `nb` holds the literal (m bytes, readable 8 bytes past its end).
GDV_DEV bool gdv_like_prefix(const gdv_str& s, const gdv_uint8* nb, gdv_int32 m) {
  return m <= s.len && gdv_bytes_equal(s, 0, nb, nb + m + 8, m);
}
GDV_DEV bool gdv_like_suffix(const gdv_str& s, const gdv_uint8* nb, gdv_int32 m) {
  return m <= s.len && gdv_bytes_equal(s, s.len - m, nb, nb + m + 8, m);
}
GDV_DEV bool gdv_like_equal(const gdv_str& s, const gdv_uint8* nb, gdv_int32 m) {
  return m == s.len && gdv_bytes_equal(s, 0, nb, nb + m + 8, m);
}
// substring search, 8 candidate positions per step: a SWAR zero-byte test on
// (word ^ first-needle-byte) yields the positions whose byte equals the needle's first byte;
// only those are verified, on a 64-bit window assembled from the current and next word.
// (The zero-byte test can flag a byte above a true match — harmless, it is verified too.)
static __device__ GDV_COLD bool gdv_like_contains(const gdv_str& s, const gdv_uint8* nb, gdv_int32 m) {
  if (m == 0) return true;
  if (m > s.len) return false;
  const gdv_uint64 mask = gdv_low_bytes_mask(m);
  const gdv_uint64 first = gdv_load8(nb, nb + m + 8) & mask;
  const gdv_uint64 splat = (first & 0xffull) * 0x0101010101010101ull;
  const gdv_uint64 splat2 = ((first >> 8) & 0xffull) * 0x0101010101010101ull;
  const gdv_int32 last = s.len - m;  // last candidate start
  gdv_uint64 cur = gdv_word_at(s, 0);
  for (gdv_int32 base = 0; base <= last; base += 8) {
    const gdv_uint64 nxt = (base + 8 < s.len) ? gdv_word_at(s, base + 8) : 0ull;
    const gdv_uint64 x = cur ^ splat;
    gdv_uint64 cand = (x - 0x0101010101010101ull) & ~x & GDV_B80;
    if (m >= 2) {
      // second needle byte at the next position as well: with 64 lanes x 8 positions a
      // one-byte filter lets some lane into the verification loop on nearly every word
      const gdv_uint64 y = ((cur >> 8) | (nxt << 56)) ^ splat2;
      cand &= (y - 0x0101010101010101ull) & ~y & GDV_B80;
    }
    while (cand) {
      const int k = __builtin_ctzll(cand) >> 3;
      cand &= cand - 1;
      if (base + k > last) break;
      const gdv_uint64 win = k == 0 ? cur : ((cur >> (8 * k)) | (nxt << (64 - 8 * k)));
      if ((win & mask) == first &&
          (m <= 8 || gdv_bytes_equal(s, base + k + 8, nb + 8, nb + m + 8, m - 8)))
        return true;
    }
    cur = nxt;
  }
  return false;
}

// IN over strings: linear probe of the literal list (lists are short in practice)
GDV_DEV bool gdv_in_strings(const gdv_str& s, const gdv_uint8* bytes, const gdv_int32* offs, gdv_int32 n) {
  for (gdv_int32 k = 0; k < n; k++) {
    const gdv_int32 len = offs[k + 1] - offs[k];
    if (len != s.len) continue;
    bool eq = true;  // word-wise; the literal table is readable 8 bytes past its last byte
    for (gdv_int32 i = 0; i < len && eq; i += 8)
      eq = ((gdv_word_at(s, i) ^ gdv_load8_raw(bytes + offs[k] + i)) & gdv_low_bytes_mask(len - i)) == 0;
    if (eq) return true;
  }
  return false;
}


// ------------------------------------------------------------------ var-len kernels: byte sweep
// The rows of a wave tile occupy ONE contiguous span of the column's data buffer.  The sweep
// walks that span with lanes over bytes (16 B per lane and step, coalesced) and answers
// tile-wide questions once per byte instead of once per row and word:
//   * is any byte >= 0x80?  (ASCII tiles skip every UTF-8 walk: substr, left, length ...)
//   * where does a '%needle%' pattern match?  One bit per span byte in an LDS bitmap; a row then
//     tests its own byte range with two word reads (gdv_range_any) — no per-row search loop.
#define GDV_B01 0x0101010101010101ull
#ifndef GDV_SPAN_MAX
#define GDV_SPAN_MAX (GDV_U * 64 * 32)  // bytes of span the LDS match bitmaps cover (32 per row)
#endif
// bit k of the result: the m-byte needle (`first` = its bytes, `mask` = low m bytes set;
// 2 <= m <= 8) starts at byte k of `cur` (its bytes continue in `nxt`).  Two-byte SWAR filter
// (zero-byte tests on word ^ splat), exact verification of the few candidates.
GDV_DEV gdv_uint32 gdv_match8(gdv_uint64 cur, gdv_uint64 nxt, gdv_uint64 first, gdv_uint64 mask,
                              gdv_uint32 splat0_4, gdv_uint32 splat1_4) {
  // (the splats of the needle's first two bytes travel as 32-bit words: half the scalar registers)
  const gdv_uint64 splat0 = ((gdv_uint64)splat0_4 << 32) | splat0_4, splat1 = ((gdv_uint64)splat1_4 << 32) | splat1_4;
  const gdv_uint64 x = cur ^ splat0;
  gdv_uint64 cand = (x - GDV_B01) & ~x & GDV_B80;
  const gdv_uint64 y = ((cur >> 8) | (nxt << 56)) ^ splat1;
  cand &= (y - GDV_B01) & ~y & GDV_B80;
  gdv_uint32 m = 0;
  while (cand) {
    const int k = __builtin_ctzll(cand) >> 3;
    cand &= cand - 1;
    const gdv_uint64 win = k == 0 ? cur : ((cur >> (8 * k)) | (nxt << (64 - 8 * k)));
    if ((win & mask) == first) m |= 1u << k;
  }
  return m;
}
// One 16-byte piece of the byte sweep, written to a FLAT output as it is read (the output's bytes
// are the input's: its offsets are the input's minus the first one and need no scan).  Only
// pieces that lie entirely inside this wave's span [sp0, sp1) are stored here; the two ragged ends
// are written once per tile by gdv_sweep_edges as whole 16-byte pieces that OVERLAP their
// neighbours inside the span with identical bytes (a byte-wise edge loop cost 20 VGPRs: 72 -> 52
// on C5, i.e. 6 -> 8 waves per SIMD).  Nothing is stored at or past the capacity.  The output
// position and the capacity are 32-bit values (a flat output is below 2 GiB: its offsets are
// int32): a scalar base + 32-bit lane offset instead of 64-bit lane arithmetic.
GDV_DEV void gdv_sweep_store32(gdv_uint8* __restrict__ dst, gdv_int32 doff, const gdv_uint64 (&w)[2], gdv_int32 map,
                               bool inside, gdv_int32 cap31) {
  if (inside && doff <= cap31 - 16) gdv_store16(dst + (gdv_uint32)doff, gdv_map8(w[0], map), gdv_map8(w[1], map));
}
// the ends of the span: lane 0 writes bytes [sp0, sp0 + 16), lane 1 bytes [sp1 - 16, sp1) (spans
// shorter than 16 bytes: one byte per lane).  dst = output bytes, src = input bytes, both indexed
// by the input offset minus `rebase`.
GDV_DEV void gdv_sweep_edges(gdv_uint8* __restrict__ dst, const gdv_uint8* __restrict__ src, gdv_int32 sp0,
                             gdv_int32 sp1, gdv_int32 rebase, gdv_int32 map, gdv_int64 cap, int lane) {
  const gdv_int32 cnt = sp1 - sp0;
  if (cnt >= 16) {
    if (lane < 2) {
      const gdv_int32 at = lane == 0 ? sp0 : sp1 - 16;
      if ((gdv_int64)at - rebase + 16 <= cap) {
        gdv_uint64 q[2];
        __builtin_memcpy(q, src + at, 16);
        q[0] = gdv_map8(q[0], map);
        q[1] = gdv_map8(q[1], map);
        __builtin_memcpy(dst + (at - rebase), q, 16);
      }
    }
  } else if (lane < cnt && (gdv_int64)sp0 - rebase + lane < cap) {
    dst[sp0 - rebase + lane] = gdv_map_byte(src[sp0 + lane], map);
  }
}
// bit i of the result: byte i of the 16-byte piece (w0, w1) is a UTF-8 continuation byte (10xxxxxx)
GDV_DEV gdv_uint32 gdv_cont_mask16(gdv_uint64 w0, gdv_uint64 w1) {
  const gdv_uint64 c0 = (w0 & ~(w0 << 1) & GDV_B80) >> 7, c1 = (w1 & ~(w1 << 1) & GDV_B80) >> 7;  // bit 8j: byte j continues
  // (bits at multiples of 8 -> 8 adjacent bits: every partial product of the multiply lands on its own position)
  return (gdv_uint32)((c0 * 0x0102040810204080ull) >> 56) | ((gdv_uint32)((c1 * 0x0102040810204080ull) >> 56) << 8);
}
// Row view of the exact variant of the wave kernels.  "Character index == byte index" — what the
// ASCII fast paths assume — holds exactly when the row contains no CONTINUATION byte (a lone byte
// >= 0xC0 is one character either way), so that is the test, per row, on the sweep's continuation
// bitmap `cb` (bit = position in the sub-tile's span; readable one word past any position):
//   sub-tile without any byte >= 0x80 (wave-uniform)   -> ASCII, nothing is looked at
//   row of <= 64 bytes inside the bitmap's reach       -> ASCII if its 64-position window holds no
//        continuation bit; otherwise the window becomes the row's lead-byte mask (GDV_STR_LEAD):
//        character counts and positions are popcount / select on it, no byte is read again
//   anything else (long rows, spans beyond the bitmap) -> neither: the general paths walk the bytes
GDV_DEV gdv_str gdv_with_lead(gdv_str s, bool subtile_has_high, bool in_bitmap, const gdv_uint64* cb, gdv_int32 lo) {
  if (!subtile_has_high) {
    s.flags |= GDV_STR_ASCII;
    return s;
  }
  if (in_bitmap && s.len <= 64) {
    const gdv_int32 w = lo >> 6, sh = lo & 63;
    const gdv_uint64 x = (cb[w] >> sh) | ((cb[w + 1] << 1) << (63 - sh));
    const gdv_uint64 cont = s.len >= 64 ? x : (x & ((1ull << (s.len > 0 ? s.len : 0)) - 1ull));
    if (cont == 0) {
      s.flags |= GDV_STR_ASCII;
    } else {
      s.lead = ~x;
      s.lead_p = s.p;
      s.flags |= GDV_STR_LEAD;
    }
  }
  return s;
}
// any bit set in [lo, hi) of the bitmap (hi <= lo: empty range).  Branch-free for ranges of up
// to 64 positions (rows up to 64 + needle bytes long): two adjacent words, one funnel shift, one
// mask — the round-2 ablation (tools/c5_ablation.sh) priced the branchy word walk at 142 VALU
// per 64 rows, a third of the kernel.  The bitmap is readable one word past any position.
GDV_DEV bool gdv_range_any(const gdv_uint64* bm, gdv_int32 lo, gdv_int32 hi) {
  const gdv_int32 nbits = hi - lo;
  const gdv_int32 w = lo >> 6, s = lo & 63;
  const gdv_uint64 x = (bm[w] >> s) | ((bm[w + 1] << 1) << (63 - s));  // positions lo .. lo+63
  const gdv_uint64 m = nbits >= 64 ? ~0ull : ((1ull << (nbits > 0 ? nbits : 0)) - 1ull);
  bool any = nbits > 0 && (x & m) != 0;
  if (nbits > 64 && !any) {  // long rows: walk the remaining words
    gdv_int32 p = lo + 64;
    for (; p + 64 <= hi && !any; p += 64) {
      const gdv_int32 pw = p >> 6, ps = p & 63;
      any = ((bm[pw] >> ps) | ((bm[pw + 1] << 1) << (63 - ps))) != 0;
    }
    if (!any && p < hi) {
      const gdv_int32 pw = p >> 6, ps = p & 63;
      const gdv_uint64 y = (bm[pw] >> ps) | ((bm[pw + 1] << 1) << (63 - ps));
      any = (y & ((1ull << (hi - p)) - 1ull)) != 0;
    }
  }
  return any;
}

// ------------------------------------------------------------------ string tail: split_part, substring_index, repeat, space,
// translate.  split_part / substring_index return narrower views of their text (any consumer takes them, as it takes
// substr's); repeat / space are GDV_MAP_CYCLE values (the cyclic view lpad / rpad materialise); translate is a value of its
// own kind, GDV_MAP_TRANSLATE, which is NOT one of GDV_MAP_SPECIAL: only plans that hold a translate() copy their outputs
// through the *_ext entry points below, so every other plan's copy code stays what it was.
//
// The delimiter is searched for bytewise, left to right, without overlap, in the text read through its case map.  A
// delimiter without a case map of its own whose bytes — and the text's — are readable with raw 8-byte loads (literals in the
// constant block, column rows flagged GDV_STR_INBUF) takes the word-at-a-time search; anything else compares byte by byte.
GDV_DEV gdv_int32 gdv_find_delim(const gdv_str& s, gdv_int32 from, const gdv_str& d) {
  const gdv_int32 cm = s.map & GDV_MAP_CASE, dm = d.map & GDV_MAP_CASE;
  if ((s.flags & d.flags & GDV_STR_INBUF) && dm == 0) return gdv_find_raw(s.p, s.len, cm, from, d.p, d.len);
  for (gdv_int32 i = from; i + d.len <= s.len; i++)
    if (gdv_match_row(s.p, i, s.len, cm, d.p, d.len, dm)) return i;
  return -1;
}
// split_part(text, delimiter, index): field `index` (1-based) of text split on the delimiter.  index < 1 is an execution
// error; an empty text or delimiter gives the text; an index past the last field gives "".
GDV_DEV gdv_str split_part_utf8_utf8_int32(gdv_ctx ctx, gdv_str s, const gdv_str& d, gdv_int32 index) {
  if (index < 1) {
    gdv_raise(ctx, GDV_ERR_BAD_ARG);
    s.len = 0;
    return s;
  }
  if (s.len <= 0 || d.len <= 0) return s;
  for (gdv_int32 k = 1, start = 0;; k++) {
    const gdv_int32 at = gdv_find_delim(s, start, d);
    if (k == index) {
      const gdv_int32 end = at < 0 ? s.len : at;
      s.p += start;
      s.len = end - start;
      return s;
    }
    if (at < 0) {
      s.len = 0;
      return s;
    }
    start = at + d.len;
  }
}
// substring_index(text, delimiter, count): with n occurrences of the delimiter, count > 0: the bytes before occurrence
// `count` (the text when count > n); count < 0: the bytes after occurrence n - |count| + 1 (the text when |count| > n);
// count 0, an empty text or an empty delimiter: "".  Raises nothing (the context is the signature's).
GDV_DEV gdv_str substring_index_utf8_utf8_int32(gdv_ctx ctx, gdv_str s, const gdv_str& d, gdv_int32 count) {
  (void)ctx;
  if (count == 0 || s.len <= 0 || d.len <= 0) {
    s.len = 0;
    return s;
  }
  gdv_int64 want = count;
  if (count < 0) {  // occurrence n - |count| + 1 from the left: n first
    gdv_int64 n = 0;
    for (gdv_int32 at = gdv_find_delim(s, 0, d); at >= 0; at = gdv_find_delim(s, at + d.len, d)) n++;
    want = n + (gdv_int64)count + 1;
    if (want < 1) return s;
  }
  gdv_int32 at = -d.len;
  for (gdv_int64 k = 0; k < want; k++) {
    at = gdv_find_delim(s, at + d.len, d);
    if (at < 0) return s;  // (count > n)
  }
  if (count > 0) {
    s.len = at;
  } else {
    s.p += at + d.len;
    s.len -= at + d.len;
  }
  return s;
}
// repeat(text, n): the text n times — a cyclic view of it.  n < 0 is an execution error (an empty text gives "" first);
// results above INT32_MAX bytes are an execution error (larger batch totals are refused by the host, as for any output).
GDV_DEV gdv_str repeat_utf8_int32(gdv_ctx ctx, gdv_str s, gdv_int32 n) {
  gdv_str r = gdv_empty_str();
  if (n == 0 || s.len <= 0) return r;
  const gdv_int64 total = (gdv_int64)s.len * n;
  if (n < 0 || total > 0x7fffffffll) {
    gdv_raise(ctx, GDV_ERR_BAD_ARG);
    return r;
  }
  r = s;
  r.flags &= ~GDV_STR_LEAD;
  r.lead = (gdv_uint64)s.len;
  r.len = (gdv_int32)total;
  r.map = (s.map & GDV_MAP_CASE) | GDV_MAP_CYCLE;
  return r;
}
// space(n): n spaces — a one-byte literal read cyclically.  n <= 0 gives ""; above INT32_MAX bytes: execution error.
GDV_DEV gdv_str space_int64(gdv_ctx ctx, gdv_int64 n) {
  gdv_str r = gdv_empty_str();
  if (n <= 0) return r;
  if (n > 0x7fffffffll) {
    gdv_raise(ctx, GDV_ERR_BAD_ARG);
    return r;
  }
  r.p = (const gdv_uint8*)" ";
  r.lim = r.p + 1;
  r.flags = GDV_STR_ASCII;  // (no INBUF: the cyclic copy reads byte by byte)
  r.lead = 1;
  r.len = (gdv_int32)n;
  r.map = GDV_MAP_CYCLE;
  return r;
}
GDV_DEV gdv_str space_int32(gdv_ctx ctx, gdv_int32 n) { return space_int64(ctx, (gdv_int64)n); }

// translate(text, from, to) with literal from / to.  The planner lays out the table once per expression in the constant
// block: int32 kind, int32 count, 8 unused bytes, then
//   kind 0 (from and to both ASCII): 256 bytes, entry c = the byte ASCII character c becomes, GDV_TR_DELETE to drop it
//          (entries >= 0x80 are never read: continuation and lead bytes cannot match an ASCII character);
//   kind 1 (otherwise): `count` entries of four uint32 — key (the character's bytes, packed little-endian: one-to-one with
//          its code point), replacement length (0: deleted), replacement offset from the table start, unused — then the
//          replacement bytes.  First occurrence in `from` wins; the planner keeps only that one.
// The row function walks the characters, raises on text that is not UTF-8 (a byte that cannot lead a character, a
// character cut by the end of the text, a continuation byte that is not 10xxxxxx) and returns the result's length; the
// copy (gdv_copy_translated) only writes.  The value: p = the text, lead = its length, lead_p = the table.
#define GDV_MAP_TRANSLATE 8192
#define GDV_TR_DELETE 0xFF
// bytes of the well-formed character at byte i of p (length len), 0 when it is not one
GDV_DEV gdv_int32 gdv_utf8_char_len(const gdv_uint8* p, gdv_int32 i, gdv_int32 len) {
  const gdv_int32 cl = gdv_utf8_declared_len(p[i]);
  if (cl == 0 || i + cl > len) return 0;
  for (gdv_int32 j = 1; j < cl; j++)
    if ((p[i + j] & 0xC0) != 0x80) return 0;
  return cl;
}
GDV_DEV gdv_uint32 gdv_utf8_key(const gdv_uint8* p, gdv_int32 i, gdv_int32 cl, gdv_uint8 first) {
  gdv_uint32 k = first;
  for (gdv_int32 j = 1; j < cl; j++) k |= (gdv_uint32)p[i + j] << (8 * j);
  return k;
}
// entry of `key` in a kind-1 table, or nullptr
GDV_DEV const gdv_uint32* gdv_tr_find(const gdv_uint8* desc, gdv_uint32 key) {
  const gdv_int32 cnt = ((const gdv_int32*)desc)[1];
  const gdv_uint32* e = (const gdv_uint32*)(desc + 16);
  for (gdv_int32 k = 0; k < cnt; k++, e += 4)
    if (e[0] == key) return e;
  return nullptr;
}
GDV_DEV gdv_str gdv_translate(gdv_ctx ctx, gdv_str s, const gdv_uint8* desc) {
  if (s.len <= 0) return s;
  const gdv_int32 kind = ((const gdv_int32*)desc)[0], cm = s.map & GDV_MAP_CASE;
  const gdv_uint8* amap = desc + 16;
  gdv_int64 out = 0;
  for (gdv_int32 i = 0; i < s.len;) {
    const gdv_uint8 c = gdv_map_byte(s.p[i], cm);
    gdv_int32 cl = 1;
    if (c >= 0x80) {
      cl = gdv_utf8_char_len(s.p, i, s.len);
      if (cl == 0) {
        gdv_raise(ctx, GDV_ERR_BAD_ARG);
        s.len = 0;
        return s;
      }
    }
    if (kind == 0) {
      out += (c < 0x80 && amap[c] == GDV_TR_DELETE) ? 0 : cl;
    } else {
      const gdv_uint32* e = gdv_tr_find(desc, gdv_utf8_key(s.p, i, cl, c));
      out += e != nullptr ? (gdv_int64)e[1] : cl;
    }
    i += cl;
  }
  if (out > 0x7fffffffll) {
    gdv_raise(ctx, GDV_ERR_BAD_ARG);
    s.len = 0;
    return s;
  }
  s.lead = (gdv_uint64)s.len;
  s.lead_p = desc;
  s.flags = 0;
  s.len = (gdv_int32)out;
  s.map = cm | GDV_MAP_TRANSLATE;
  return s;
}
// (byte loop; never writes more than the row function's length)
template <typename P>
GDV_DEV void gdv_copy_translated(P dst, const gdv_str& s) {
  const gdv_uint8* desc = s.lead_p;
  const gdv_int32 kind = ((const gdv_int32*)desc)[0], len = (gdv_int32)s.lead, cm = s.map & GDV_MAP_CASE, cap = s.len;
  const gdv_uint8* amap = desc + 16;
  gdv_int32 o = 0;
  for (gdv_int32 i = 0; i < len;) {
    const gdv_uint8 c = gdv_map_byte(s.p[i], cm);
    gdv_int32 cl = 1;
    if (c >= 0x80) cl = gdv_utf8_char_len(s.p, i, len);
    if (cl == 0) return;  // (the row function raised: never reached with a length)
    const gdv_uint8* rep = nullptr;
    gdv_int32 rl = -1;
    if (kind == 0) {
      if (c < 0x80) {
        const gdv_uint8 b = amap[c];
        if (b != GDV_TR_DELETE) {
          if (o >= cap) return;
          dst[o++] = b;
        }
        i++;
        continue;
      }
    } else {
      const gdv_uint32* e = gdv_tr_find(desc, gdv_utf8_key(s.p, i, cl, c));
      if (e != nullptr) {
        rep = desc + e[2];
        rl = (gdv_int32)e[1];
      }
    }
    if (rl < 0) {
      if (o + cl > cap) return;
      dst[o++] = c;
      for (gdv_int32 j = 1; j < cl; j++) dst[o++] = s.p[i + j];
    } else {
      if (o + rl > cap) return;
      for (gdv_int32 j = 0; j < rl; j++) dst[o++] = rep[j];
    }
    i += cl;
  }
}
// the copy entry points of plans that hold a translate(): translate values here, everything else as before
GDV_DEV void gdv_str_copy_ext(gdv_uint8* dst, const gdv_str& s) {
  if (s.map & GDV_MAP_TRANSLATE) {
    gdv_copy_translated(dst, s);
    return;
  }
  gdv_str_copy(dst, s);
}

// ------------------------------------------------------------------ upper / lower under GDV_UTF8_CASE=1 at Make: every character
// through utf8proc's simple case map (tools/gen_utf8_case_table.py restates it from pyarrow into gdv_utf8_case_table.inc; the
// planner lays the direction a plan needs into its constant block).  The table: int32 kind (1 upper, 2 lower), int32 n1, int32
// offset of stage 2, int32 unused; 128 bytes, bit b = some code point of the 64-code-point block b of the BMP changes its UTF-8
// length; n1 bytes of stage 1 (entry b = the stage-2 block of code points 64 b .., 0: none of them changes); stage 2, blocks of
// 64 uint16 = (mapped - code point) mod 2^16, 0 = unchanged (a mapped code point stays in its 64 Ki plane).  A lookup is two
// dependent loads, never a search; both stages of one direction are below 16 KiB and stay in the vector L1 / L2.
// A value of its own kind, GDV_MAP_UTF8CASE, as translate's is: the row function walks the text, raises on text that is not
// UTF-8 by translate's rule (gdv_utf8_char_len) and returns the result's length; the copy only writes.  p = the text, lead =
// its length, lead_p = the table, flags keeps GDV_STR_INBUF.  Sequences that pass the structural rule but are not Unicode
// (over-long forms, surrogates, above U+10FFFF) are copied unchanged.  Stretches without a byte >= 0x80 of a view readable with
// raw 8-byte loads (GDV_STR_INBUF) are taken a word at a time in both passes: counted as they are, mapped with gdv_map8.
// The length differs from the source's only at the length-changing code points (34 upper, 27 lower): the row function looks a
// character up only when the 128-byte bitmap says its block holds one; four-byte characters never change length.
// Plans that hold such a value copy through GDV_COPY_UTF8CASE around the entry point they would use without it.
#define GDV_MAP_UTF8CASE 1048576
#define GDV_COPY_UTF8CASE(dst, v, otherwise) \
  do { if ((v).map & GDV_MAP_UTF8CASE) gdv_copy_utf8_case(dst, v); else otherwise; } while (0)
// the code point of the well-formed character of cl >= 2 bytes at byte i of p (first byte c); 0 when it is not Unicode
GDV_DEV gdv_uint32 gdv_utf8_decode(const gdv_uint8* p, gdv_int32 i, gdv_int32 cl, gdv_uint8 c) {
  if (cl == 2) {
    const gdv_uint32 cp = ((gdv_uint32)(c & 0x1F) << 6) | (p[i + 1] & 0x3F);
    return cp < 0x80 ? 0u : cp;
  }
  if (cl == 3) {
    const gdv_uint32 cp = ((gdv_uint32)(c & 0x0F) << 12) | ((gdv_uint32)(p[i + 1] & 0x3F) << 6) | (p[i + 2] & 0x3F);
    return (cp < 0x800 || (cp >= 0xD800 && cp <= 0xDFFF)) ? 0u : cp;
  }
  const gdv_uint32 cp = ((gdv_uint32)(c & 0x07) << 18) | ((gdv_uint32)(p[i + 1] & 0x3F) << 12) | ((gdv_uint32)(p[i + 2] & 0x3F) << 6) |
                        (p[i + 3] & 0x3F);
  return (cp < 0x10000 || cp > 0x10FFFF) ? 0u : cp;
}
GDV_DEV gdv_int32 gdv_utf8_cp_len(gdv_uint32 cp) { return cp < 0x80 ? 1 : cp < 0x800 ? 2 : cp < 0x10000 ? 3 : 4; }
// what cp maps to (cp itself when the map leaves it alone)
GDV_DEV gdv_uint32 gdv_utf8_case_lookup(const gdv_uint8* tab, gdv_uint32 cp) {
  const gdv_uint32 b = cp >> 6;
  if (b >= (gdv_uint32)((const gdv_int32*)tab)[1]) return cp;
  const gdv_uint32 blk = tab[16 + 128 + b];
  if (blk == 0) return cp;
  const gdv_uint32 d = ((const gdv_uint16*)(tab + ((const gdv_int32*)tab)[2]))[blk * 64 + (cp & 63)];
  return (cp & 0xFFFF0000u) | ((cp + d) & 0xFFFFu);
}
GDV_DEV gdv_str gdv_utf8_case(gdv_ctx ctx, gdv_str s, const gdv_uint8* tab) {
  if (s.len <= 0) return s;
  const bool words = (s.flags & GDV_STR_INBUF) != 0;
  const gdv_uint8* lenmap = tab + 16;
  gdv_int64 out = s.len;
  for (gdv_int32 i = 0; i < s.len;) {
    if (words) {
      const gdv_int32 r = s.len - i < 8 ? s.len - i : 8;
      if ((gdv_load8_raw(s.p + i) & gdv_low_bytes_mask(r) & GDV_B80) == 0) {
        i += r;
        continue;
      }
    }
    const gdv_uint8 c = s.p[i];
    if (c < 0x80) {
      i++;
      continue;
    }
    const gdv_int32 cl = gdv_utf8_char_len(s.p, i, s.len);
    if (cl == 0) {
      gdv_raise(ctx, GDV_ERR_BAD_ARG);
      s.len = 0;
      return s;
    }
    if (cl < 4) {
      const gdv_uint32 cp = gdv_utf8_decode(s.p, i, cl, c);
      if (cp != 0 && ((lenmap[cp >> 9] >> ((cp >> 6) & 7)) & 1)) out += gdv_utf8_cp_len(gdv_utf8_case_lookup(tab, cp)) - cl;
    }
    i += cl;
  }
  if (out > 0x7fffffffll) {
    gdv_raise(ctx, GDV_ERR_BAD_ARG);
    s.len = 0;
    return s;
  }
  s.lead = (gdv_uint64)s.len;
  s.lead_p = tab;
  s.flags &= GDV_STR_INBUF;
  s.len = (gdv_int32)out;
  s.map = (s.map & GDV_MAP_CASE) | GDV_MAP_UTF8CASE;
  return s;
}
// (never writes more than the row function's length)
template <typename P>
GDV_DEV void gdv_copy_utf8_case(P dst, const gdv_str& s) {
  const gdv_uint8* tab = s.lead_p;
  const gdv_int32 dir = ((const gdv_int32*)tab)[0], len = (gdv_int32)s.lead, cm = s.map & GDV_MAP_CASE, cap = s.len;
  const bool words = (s.flags & GDV_STR_INBUF) != 0;
  gdv_int32 o = 0;
  for (gdv_int32 i = 0; i < len;) {
    if (words) {
      const gdv_int32 r = len - i < 8 ? len - i : 8;
      gdv_uint64 w = gdv_load8_raw(s.p + i);
      if ((w & gdv_low_bytes_mask(r) & GDV_B80) == 0) {
        if (o + r > cap) return;
        w = gdv_map8(gdv_map8(w, cm), dir);
        if (r == 8) __builtin_memcpy(dst + o, &w, 8); else gdv_store_low_bytes(dst + o, w, r);
        o += r;
        i += r;
        continue;
      }
    }
    const gdv_uint8 c = gdv_map_byte(s.p[i], cm);
    if (c < 0x80) {
      if (o >= cap) return;
      dst[o++] = gdv_map_byte(c, dir);
      i++;
      continue;
    }
    const gdv_int32 cl = gdv_utf8_char_len(s.p, i, len);
    if (cl == 0) return;  // (the row function raised: never reached with a length)
    const gdv_uint32 cp = gdv_utf8_decode(s.p, i, cl, c);
    const gdv_uint32 to = cp != 0 ? gdv_utf8_case_lookup(tab, cp) : 0u;
    if (to == cp) {
      if (o + cl > cap) return;
      dst[o++] = c;
      for (gdv_int32 j = 1; j < cl; j++) dst[o++] = s.p[i + j];
    } else {
      const gdv_int32 ol = gdv_utf8_cp_len(to);
      if (o + ol > cap) return;
      if (ol == 1) {
        dst[o] = (gdv_uint8)to;
      } else if (ol == 2) {
        dst[o] = (gdv_uint8)(0xC0 | (to >> 6));
        dst[o + 1] = (gdv_uint8)(0x80 | (to & 0x3F));
      } else if (ol == 3) {
        dst[o] = (gdv_uint8)(0xE0 | (to >> 12));
        dst[o + 1] = (gdv_uint8)(0x80 | ((to >> 6) & 0x3F));
        dst[o + 2] = (gdv_uint8)(0x80 | (to & 0x3F));
      } else {
        dst[o] = (gdv_uint8)(0xF0 | (to >> 18));
        dst[o + 1] = (gdv_uint8)(0x80 | ((to >> 12) & 0x3F));
        dst[o + 2] = (gdv_uint8)(0x80 | ((to >> 6) & 0x3F));
        dst[o + 3] = (gdv_uint8)(0x80 | (to & 0x3F));
      }
      o += ol;
    }
    i += cl;
  }
}

// ------------------------------------------------------------------ data masking: mask, mask_first_n, mask_last_n,
// mask_show_first_n, mask_show_last_n.  A masked byte 'A'..'Z' becomes the upper replacement, 'a'..'z' the lower one, '0'..'9'
// the digit one (literals of one byte < 0x80: the planner checks them); every other byte, every byte >= 0x80 included, is
// copied, so the result has the text's length.  n counts characters; a character starts at every byte that is not 10xxxxxx
// (nothing is validated, nothing raises).  With c characters and k = min(max(n, 0), c): first_n masks characters [0, k),
// last_n [c - k, c), show_first_n [k, c), show_last_n [0, c - k).  [recollection + decisions: PARITY.md, `mask`]
// A value of its own kind, GDV_MAP_MASK, as translate's is: the row function reads no byte — it keeps p / len / the ASCII case
// map / GDV_STR_INBUF and packs into `lead` n (bits 0..31), the upper / lower / digit replacement (bits 32..55) and the mode
// (bits 56..58); lead_p is unused.  The copy does the work: the masked characters are one byte range [b0, b1) of the row, found
// from the lead bytes of its words (popcount of the "not 10xxxxxx" bits; the last_n pair walks back from the row's end), then
// every word is classified with the carry-free range tests of gdv_map8 and the replacement bytes are selected under a per-byte
// mask.  Views readable with raw 8-byte loads (GDV_STR_INBUF) go eight bytes per step; a byte loop serves the others.
// Plans that hold such a value copy through GDV_COPY_MASK around the entry point they would use without it.
#define GDV_MAP_MASK 2097152
#define GDV_COPY_MASK(dst, v, otherwise) \
  do { if ((v).map & GDV_MAP_MASK) gdv_copy_masked(dst, v); else otherwise; } while (0)
#define GDV_MASK_ALL 0
#define GDV_MASK_FIRST_N 1
#define GDV_MASK_LAST_N 2
#define GDV_MASK_SHOW_FIRST_N 3
#define GDV_MASK_SHOW_LAST_N 4
// reps: upper | lower << 8 | digit << 16
GDV_DEV gdv_str gdv_mask(gdv_str s, gdv_int32 mode, gdv_int32 n, gdv_uint32 reps) {
  s.lead = (gdv_uint64)(gdv_uint32)n | ((gdv_uint64)(reps & 0xFFFFFFu) << 32) | ((gdv_uint64)mode << 56);
  s.lead_p = nullptr;
  s.flags &= GDV_STR_INBUF;
  s.map = (s.map & GDV_MAP_CASE) | GDV_MAP_MASK;
  return s;
}
// bit 7 of every byte of w that starts a character (is not 10xxxxxx)
GDV_DEV gdv_uint64 gdv_lead_bits8(gdv_uint64 w) { return ~(w & ~(w << 1)) & GDV_B80; }
// byte offset of the character with 0-based index k >= 0 of the `len` bytes at p, `len` when there are fewer
GDV_DEV gdv_int32 gdv_mask_pos_fwd(const gdv_uint8* p, gdv_int32 len, bool words, gdv_int32 k) {
  if (words) {
    for (gdv_int32 i = 0; i < len; i += 8) {
      gdv_uint64 lead = gdv_lead_bits8(gdv_load8_raw(p + i)) & gdv_low_bytes_mask(len - i);
      const gdv_int32 c = (gdv_int32)__popcll(lead);
      if (k < c) {
        for (; k > 0; k--) lead &= lead - 1;  // drop the characters before it
        return i + (gdv_int32)(__builtin_ctzll(lead) >> 3);
      }
      k -= c;
    }
    return len;
  }
  for (gdv_int32 i = 0; i < len; i++)
    if ((p[i] & 0xC0) != 0x80 && k-- == 0) return i;
  return len;
}
// byte offset of the k-th character from the end (k >= 1), 0 when there are fewer
GDV_DEV gdv_int32 gdv_mask_pos_back(const gdv_uint8* p, gdv_int32 len, bool words, gdv_int32 k) {
  if (words) {
    for (gdv_int32 e = len; e > 0;) {
      const gdv_int32 b = e > 8 ? e - 8 : 0;  // (the load starts inside the view)
      gdv_uint64 lead = gdv_lead_bits8(gdv_load8_raw(p + b)) & gdv_low_bytes_mask(e - b);
      const gdv_int32 c = (gdv_int32)__popcll(lead);
      if (k <= c) {
        for (; k > 1; k--) lead &= ~(1ull << (63 - __builtin_clzll(lead)));  // drop the characters behind it
        return b + (gdv_int32)((63 - __builtin_clzll(lead)) >> 3);
      }
      k -= c;
      e = b;
    }
    return 0;
  }
  for (gdv_int32 i = len - 1; i >= 0; i--)
    if ((p[i] & 0xC0) != 0x80 && --k == 0) return i;
  return 0;
}
// the 0xFF bytes of the ASCII bytes of w in ['A','Z'] (*up), ['a','z'] (*lo), ['0','9'] (*dg): gdv_map8's range test, the top
// bit of each byte widened to the byte (no carry crosses a byte: 0x01 * 0xFF)
GDV_DEV void gdv_mask_classes8(gdv_uint64 w, gdv_uint64* up, gdv_uint64* lo, gdv_uint64* dg) {
  const gdv_uint64 h = w & GDV_B7F, ascii = ~w & GDV_B80;
  *up = (((h + 0x3f3f3f3f3f3f3f3full) & ~(h + 0x2525252525252525ull) & ascii) >> 7) * 0xFFull;  // 0x80 - 'A' | 0x7f - 'Z'
  *lo = (((h + 0x1f1f1f1f1f1f1f1full) & ~(h + 0x0505050505050505ull) & ascii) >> 7) * 0xFFull;  // 0x80 - 'a' | 0x7f - 'z'
  *dg = (((h + 0x5050505050505050ull) & ~(h + 0x4646464646464646ull) & ascii) >> 7) * 0xFFull;  // 0x80 - '0' | 0x7f - '9'
}
// (writes exactly the bytes [0, s.len) of dst)
template <typename P>
GDV_DEV void gdv_copy_masked(P dst, const gdv_str& s) {
  const gdv_int32 len = s.len, cm = s.map & GDV_MAP_CASE;
  if (len <= 0) return;
  const bool words = (s.flags & GDV_STR_INBUF) != 0;
  const gdv_int32 mode = (gdv_int32)((s.lead >> 56) & 7), n = (gdv_int32)(gdv_uint32)s.lead;
  const gdv_uint8 ru = (gdv_uint8)(s.lead >> 32), rl = (gdv_uint8)(s.lead >> 40), rd = (gdv_uint8)(s.lead >> 48);
  // the masked bytes [b0, b1): bytes >= 0x80 inside are copied anyway, so only whole characters' ASCII bytes matter
  gdv_int32 b0 = 0, b1 = len;
  if (mode == GDV_MASK_FIRST_N) b1 = n <= 0 ? 0 : gdv_mask_pos_fwd(s.p, len, words, n);
  else if (mode == GDV_MASK_SHOW_FIRST_N) b0 = n <= 0 ? 0 : gdv_mask_pos_fwd(s.p, len, words, n);
  else if (mode == GDV_MASK_LAST_N) b0 = n <= 0 ? len : gdv_mask_pos_back(s.p, len, words, n);
  else if (mode == GDV_MASK_SHOW_LAST_N) b1 = n <= 0 ? len : gdv_mask_pos_back(s.p, len, words, n);
  if (words) {
    const gdv_uint64 wu = ru * 0x0101010101010101ull, wl = rl * 0x0101010101010101ull, wd = rd * 0x0101010101010101ull;
    for (gdv_int32 i = 0; i < len; i += 8) {
      const gdv_int32 r = len - i < 8 ? len - i : 8;
      gdv_uint64 w = gdv_map8(gdv_load8_raw(s.p + i), cm);
      const gdv_int32 from = b0 - i < 0 ? 0 : (b0 - i > 8 ? 8 : b0 - i), to = b1 - i < 0 ? 0 : (b1 - i > 8 ? 8 : b1 - i);
      const gdv_uint64 in = gdv_low_bytes_mask(to) & ~gdv_low_bytes_mask(from);  // bytes of this word inside [b0, b1)
      gdv_uint64 up, lo, dg;
      gdv_mask_classes8(w, &up, &lo, &dg);
      up &= in;
      lo &= in;
      dg &= in;
      w = (w & ~(up | lo | dg)) | (wu & up) | (wl & lo) | (wd & dg);
      if (r == 8) __builtin_memcpy(dst + i, &w, 8); else gdv_store_low_bytes(dst + i, w, r);
    }
    return;
  }
  for (gdv_int32 i = 0; i < len; i++) {
    gdv_uint8 c = gdv_map_byte(s.p[i], cm);
    if (i >= b0 && i < b1) c = (c >= 'A' && c <= 'Z') ? ru : (c >= 'a' && c <= 'z') ? rl : (c >= '0' && c <= '9') ? rd : c;
    dst[i] = c;
  }
}

// ------------------------------------------------------------------ text <-> date / time: castDATE, castTIMESTAMP, castTIME
// of text; castVARCHAR of date32, date64, timestamp, time32; castTIME(timestamp), castTIMESTAMP(date32).  Timestamps and times
// are milliseconds.  Every function is null if null; a row that does not parse raises GDV_ERR_BAD_ARG.
// [recollection, PARITY.md "text <-> date / time"; the "decided" items are this library's own]
//   castDATE(text): at most three digit runs (year, month, day), each ended by any one byte that is not a digit (an empty
//     run is 0); reading stops after the third run's separator.  Fewer than three runs raise.  A year below 100 written with
//     fewer than 4 digits becomes 20yy when yy < 70, else 19yy.  The date must exist.  [decided: a year above 9999 raises; a
//     run of more than 9 digits raises]
//   castTIMESTAMP(text): exactly  Y{1,4} '-' M{1,2} '-' D{1,2} [(' ' | 'T') h{1,2} ':' m{1,2} [':' s{1,2} ['.' f{1,3}]]]
//     [' '? ('+' | '-') hh [':'? mm]]  read through the text's case map.  Years as castDATE; the fraction scaled to
//     milliseconds; hour 0..23, minute and second 0..59; an offset +hh:mm (the wall time is that far ahead of UTC) is
//     subtracted.  [decided: 'T' is accepted; the offset's hour 0..23 and minute 0..59]
//   castTIME(text): exactly  h{1,2} ':' m{1,2} [':' s{1,2} ['.' f{1,3}]]  -> milliseconds of the day, the same ranges.
//   castVARCHAR(timestamp, n): "yyyy-MM-dd hh:mm:ss.sss" of the civil UTC time (fields by floor division, so instants
//     before 1970 show their wall clock), cut to min(n, 23) bytes; date32 / date64: "yyyy-MM-dd", min(n, 10); time32:
//     "hh:mm:ss.sss", min(n, 12) [decided: of the value modulo one day, floor modulo].  A year outside 0..9999: '-' when
//     negative, then at least four digits, still cut.  n < 0 raises.  A row's length therefore follows from n alone.
// Parsers: an INBUF row in a canonical layout (yyyy-MM-dd, yyyy-MM-dd hh:mm:ss, yyyy-MM-dd hh:mm:ss.sss, hh:mm:ss,
// hh:mm:ss.sss) is checked with two or three 8-byte loads and SWAR masks, its digits taken from the words; any other row
// takes the byte scanner.  The fast path accepts nothing the scanner rejects and gives the same value.
// Formatters: a value of its own kind, GDV_MAP_DATETIME (lead = the instant in milliseconds, (map >> 16) & 3 = 0 timestamp,
// 1 date, 2 time), which is NOT one of GDV_MAP_SPECIAL: only plans that hold one copy their outputs through the *_dt
// entry points below, which build the text in registers and store it as whole words.
#define GDV_MAP_DATETIME 16384

// bytes of w at the positions of `dig` (0xFF per byte) are ASCII digits, those at `sep` are as in `pat` (0x30 at digits)
GDV_DEV bool gdv_dt_layout(gdv_uint64 w, gdv_uint64 dig, gdv_uint64 sep, gdv_uint64 pat) {
  const gdv_uint64 hi = (w & ((dig & 0xF0F0F0F0F0F0F0F0ull) | sep)) ^ pat;
  const gdv_uint64 lo = ((w & 0x0F0F0F0F0F0F0F0Full) + 0x0606060606060606ull) & 0x1010101010101010ull & dig;  // low nibble > 9
  return (hi | lo) == 0;
}
// the digit at byte i of w / the two-digit number at bytes i, i + 1
GDV_DEV gdv_int32 gdv_dt_d1(gdv_uint64 w, int i) { return (gdv_int32)((w >> (8 * i)) & 15); }
GDV_DEV gdv_int32 gdv_dt_d2(gdv_uint64 w, int i) { return 10 * gdv_dt_d1(w, i) + gdv_dt_d1(w, i + 1); }
GDV_DEV bool gdv_dt_is_digit(gdv_uint8 c) { return c >= '0' && c <= '9'; }
GDV_DEV gdv_int64 gdv_dt_year(gdv_int64 y, gdv_int32 ndigits) {
  return (y < 100 && ndigits < 4) ? (y < 70 ? 2000 + y : 1900 + y) : y;
}
// the day number of y-m-d, y in 0..9999; false when there is no such date
GDV_DEV bool gdv_dt_days(gdv_int64 y, gdv_int32 m, gdv_int32 d, gdv_int64* days) {
  if (y < 0 || y > 9999 || m < 1 || m > 12 || d < 1 || d > gdv_last_day_of_month(y, m)) return false;
  *days = gdv_days_from_civil(y, m, d);
  return true;
}
// yyyy-MM-dd in bytes 0..9 (w0 = bytes 0..7, w1 = bytes 8..): 1 and *days, 0 (no such date), -1 (not this layout)
GDV_DEV int gdv_dt_fast_date(gdv_uint64 w0, gdv_uint64 w1, gdv_int64* days) {
  if (!gdv_dt_layout(w0, 0x00ffff00ffffffffull, 0xff0000ff00000000ull, 0x2d30302d30303030ull) ||
      !gdv_dt_layout(w1, 0xffffull, 0, 0x3030ull))
    return -1;
  return gdv_dt_days(100 * gdv_dt_d2(w0, 0) + gdv_dt_d2(w0, 2), gdv_dt_d2(w0, 5), gdv_dt_d2(w1, 0), days) ? 1 : 0;
}
// the run of digits at byte i: its length (counted to max + 1 at most) and value
GDV_DEV gdv_int32 gdv_dt_run(const gdv_str& s, gdv_int32 i, gdv_int32 max, gdv_int32* v) {
  gdv_int32 n = 0, x = 0;
  for (; i + n < s.len && n <= max && gdv_dt_is_digit(s.p[i + n]); n++) x = 10 * x + (s.p[i + n] - '0');
  *v = x;
  return n;
}
GDV_DEV bool gdv_dt_at(const gdv_str& s, gdv_int32 i, gdv_uint8 c) { return i < s.len && gdv_str_at(s, i) == c; }
// castDATE's byte scanner
GDV_DEV bool gdv_dt_scan_date(const gdv_str& s, gdv_int64* days) {
  gdv_int32 k = 0, v = 0, n = 0, y = 0, yn = 0, m = 0, d = 0;
  for (gdv_int32 i = 0; i < s.len && k < 3; i++) {
    const gdv_uint8 c = s.p[i];
    if (gdv_dt_is_digit(c)) {
      if (++n > 9) return false;
      v = 10 * v + (c - '0');
      continue;
    }
    if (k == 0) { y = v; yn = n; } else if (k == 1) { m = v; } else { d = v; }
    k++;
    v = n = 0;
  }
  if (k < 3) {  // the last run ends with the text
    if (k == 0) { y = v; yn = n; } else if (k == 1) { m = v; } else { d = v; }
    k++;
  }
  return k == 3 && gdv_dt_days(gdv_dt_year(y, yn), m, d, days);
}
// h{1,2} ':' m{1,2} [':' s{1,2} ['.' f{1,3}]] at byte `at`: the bytes it takes (*ms set), or -1
GDV_DEV gdv_int32 gdv_dt_scan_clock(const gdv_str& s, gdv_int32 at, gdv_int64* ms) {
  gdv_int32 i = at, h = 0, mi = 0, sec = 0, f = 0, n = gdv_dt_run(s, i, 2, &h);
  if (n < 1 || n > 2 || !gdv_dt_at(s, i += n, ':')) return -1;
  n = gdv_dt_run(s, ++i, 2, &mi);
  if (n < 1 || n > 2) return -1;
  i += n;
  if (gdv_dt_at(s, i, ':')) {
    n = gdv_dt_run(s, ++i, 2, &sec);
    if (n < 1 || n > 2) return -1;
    i += n;
    if (gdv_dt_at(s, i, '.')) {
      n = gdv_dt_run(s, ++i, 3, &f);
      if (n < 1 || n > 3) return -1;
      i += n;
      f *= n == 1 ? 100 : n == 2 ? 10 : 1;
    }
  }
  if (h > 23 || mi > 59 || sec > 59) return -1;
  *ms = h * 3600000ll + mi * 60000ll + sec * 1000ll + f;
  return i - at;
}
// castTIMESTAMP's byte scanner
GDV_DEV bool gdv_dt_scan_ts(const gdv_str& s, gdv_int64* ms) {
  gdv_int32 y = 0, m = 0, d = 0, i = 0, n = gdv_dt_run(s, 0, 4, &y);
  const gdv_int32 yn = n;
  if (n < 1 || n > 4 || !gdv_dt_at(s, i += n, '-')) return false;
  n = gdv_dt_run(s, ++i, 2, &m);
  if (n < 1 || n > 2 || !gdv_dt_at(s, i += n, '-')) return false;
  n = gdv_dt_run(s, ++i, 2, &d);
  if (n < 1 || n > 2) return false;
  i += n;
  gdv_int64 days = 0, t = 0;
  if (!gdv_dt_days(gdv_dt_year(y, yn), m, d, &days)) return false;
  if ((gdv_dt_at(s, i, ' ') || gdv_dt_at(s, i, 'T')) && i + 1 < s.len && gdv_dt_is_digit(s.p[i + 1])) {
    n = gdv_dt_scan_clock(s, i + 1, &t);
    if (n < 0) return false;
    i += 1 + n;
  }
  if (i < s.len) {  // the offset
    if (gdv_dt_at(s, i, ' ')) i++;
    const bool neg = gdv_dt_at(s, i, '-');
    if (!neg && !gdv_dt_at(s, i, '+')) return false;
    gdv_int32 oh = 0, om = 0;
    n = gdv_dt_run(s, ++i, 4, &oh);
    if (n == 4) {
      om = oh % 100;
      oh /= 100;
    } else if (n == 2 && gdv_dt_at(s, i + 2, ':')) {
      n = 3 + gdv_dt_run(s, i + 3, 2, &om);
      if (n != 5) return false;
    } else if (n != 2) {
      return false;
    }
    if (i + n != s.len || oh > 23 || om > 59) return false;
    const gdv_int64 off = oh * 3600000ll + om * 60000ll;
    t += neg ? off : -off;
  }
  *ms = days * GDV_MILLIS_IN_DAY + t;
  return true;
}
GDV_DEV gdv_date64 castDATE_utf8(gdv_ctx ctx, gdv_str s) {
  gdv_int64 days = 0;
  int r = -1;
  if ((s.flags & GDV_STR_INBUF) && s.len >= 10) {
    const gdv_uint64 w1 = gdv_load8_raw(s.p + 8);
    if (s.len == 10 || !gdv_dt_is_digit((gdv_uint8)(w1 >> 16))) r = gdv_dt_fast_date(gdv_load8_raw(s.p), w1, &days);
  }
  if (r < 0) r = gdv_dt_scan_date(s, &days) ? 1 : 0;
  if (r == 0) {
    gdv_raise(ctx, GDV_ERR_BAD_ARG);
    return 0;
  }
  return days * GDV_MILLIS_IN_DAY;
}
GDV_DEV gdv_timestamp castTIMESTAMP_utf8(gdv_ctx ctx, gdv_str s) {
  gdv_int64 ms = 0;
  int r = -1;
  if ((s.flags & GDV_STR_INBUF) && (s.len == 10 || s.len == 19 || s.len == 23)) {
    const gdv_uint64 w0 = gdv_load8_raw(s.p), w1 = gdv_load8_raw(s.p + 8);
    gdv_int64 days = 0;
    if (s.len == 10) {
      r = gdv_dt_fast_date(w0, w1, &days);
    } else {
      const gdv_uint64 w2 = gdv_load8_raw(s.p + 16);
      const bool shape =
          gdv_dt_layout(w0, 0x00ffff00ffffffffull, 0xff0000ff00000000ull, 0x2d30302d30303030ull) &&
          gdv_dt_layout(w1, 0xffff00ffff00ffffull, 0x0000ff0000ff0000ull, 0x30303a3030203030ull) &&
          (s.len == 19 ? gdv_dt_layout(w2, 0xffff00ull, 0xffull, 0x30303aull)
                       : gdv_dt_layout(w2, 0x00ffffff00ffff00ull, 0x00000000ff0000ffull, 0x003030302e30303aull));
      if (shape) {
        const gdv_int32 h = gdv_dt_d2(w1, 3), mi = gdv_dt_d2(w1, 6), sec = gdv_dt_d2(w2, 1);
        r = gdv_dt_days(100 * gdv_dt_d2(w0, 0) + gdv_dt_d2(w0, 2), gdv_dt_d2(w0, 5), gdv_dt_d2(w1, 0), &days) && h <= 23 &&
            mi <= 59 && sec <= 59;
        ms = h * 3600000ll + mi * 60000ll + sec * 1000ll + (s.len == 23 ? 100 * gdv_dt_d1(w2, 4) + gdv_dt_d2(w2, 5) : 0);
      }
    }
    ms += days * GDV_MILLIS_IN_DAY;
  }
  if (r < 0) r = gdv_dt_scan_ts(s, &ms) ? 1 : 0;
  if (r == 0) {
    gdv_raise(ctx, GDV_ERR_BAD_ARG);
    return 0;
  }
  return ms;
}
GDV_DEV gdv_time32 castTIME_utf8(gdv_ctx ctx, gdv_str s) {
  gdv_int64 ms = 0;
  int r = -1;
  if ((s.flags & GDV_STR_INBUF) && (s.len == 8 || s.len == 12)) {
    const gdv_uint64 w0 = gdv_load8_raw(s.p), w1 = s.len == 12 ? gdv_load8_raw(s.p + 8) : 0ull;
    if (gdv_dt_layout(w0, 0xffff00ffff00ffffull, 0x0000ff0000ff0000ull, 0x30303a30303a3030ull) &&
        (s.len == 8 || gdv_dt_layout(w1, 0xffffff00ull, 0xffull, 0x3030302eull))) {
      const gdv_int32 h = gdv_dt_d2(w0, 0), mi = gdv_dt_d2(w0, 3), sec = gdv_dt_d2(w0, 6);
      r = h <= 23 && mi <= 59 && sec <= 59;
      ms = h * 3600000ll + mi * 60000ll + sec * 1000ll + (s.len == 12 ? 100 * gdv_dt_d1(w1, 1) + gdv_dt_d2(w1, 2) : 0);
    }
  }
  if (r < 0) r = gdv_dt_scan_clock(s, 0, &ms) == s.len ? 1 : 0;
  if (r == 0) {
    gdv_raise(ctx, GDV_ERR_BAD_ARG);
    return 0;
  }
  return (gdv_time32)ms;
}
GDV_DEV gdv_time32 castTIME_timestamp(gdv_timestamp t) {
  const gdv_int64 r = t % GDV_MILLIS_IN_DAY;
  return (gdv_time32)(r < 0 ? r + GDV_MILLIS_IN_DAY : r);
}
GDV_DEV gdv_timestamp castTIMESTAMP_date32(gdv_date32 d) { return (gdv_int64)d * GDV_MILLIS_IN_DAY; }

GDV_DEV gdv_str gdv_dt_text(gdv_ctx ctx, gdv_int64 ms, gdv_int32 kind, gdv_int32 full, gdv_int64 n) {
  gdv_str r = gdv_empty_str();
  if (n < 0) {
    gdv_raise(ctx, GDV_ERR_BAD_ARG);
    return r;
  }
  r.len = n < full ? (gdv_int32)n : full;
  r.map = GDV_MAP_DATETIME | (kind << 16);
  r.flags = 0;
  r.lead = (gdv_uint64)ms;
  return r;
}
GDV_DEV gdv_str castVARCHAR_timestamp_int64(gdv_ctx ctx, gdv_timestamp v, gdv_int64 n) { return gdv_dt_text(ctx, v, 0, 23, n); }
GDV_DEV gdv_str castVARCHAR_date64_int64(gdv_ctx ctx, gdv_date64 v, gdv_int64 n) { return gdv_dt_text(ctx, v, 1, 10, n); }
GDV_DEV gdv_str castVARCHAR_date32_int64(gdv_ctx ctx, gdv_date32 v, gdv_int64 n) {
  return gdv_dt_text(ctx, (gdv_int64)v * GDV_MILLIS_IN_DAY, 1, 10, n);
}
GDV_DEV gdv_str castVARCHAR_time32_int64(gdv_ctx ctx, gdv_time32 v, gdv_int64 n) { return gdv_dt_text(ctx, v, 2, 12, n); }

// two ASCII digits of v (0..99), first digit in the low byte
GDV_DEV gdv_uint64 gdv_dt_pair(gdv_int32 v) { return (gdv_uint64)(0x30 + v / 10) | ((gdv_uint64)(0x30 + v % 10) << 8); }
// the first 24 bytes of the text of a date / timestamp whose year is outside 0..9999 (cold: byte by byte, in registers)
GDV_DEV void gdv_dt_wide_year(const gdv_ymd& c, gdv_int32 t, gdv_uint64* w0, gdv_uint64* w1, gdv_uint64* w2) {
  gdv_uint64 a = 0, b = 0, e = 0;
  gdv_int32 at = 0;
  auto put = [&](gdv_int64 ch) {
    const gdv_uint64 x = (gdv_uint64)(ch & 0xFF) << (8 * (at & 7));
    if (at < 8) a |= x; else if (at < 16) b |= x; else if (at < 24) e |= x;
    at++;
  };
  const gdv_uint64 ay = c.y < 0 ? 0ull - (gdv_uint64)c.y : (gdv_uint64)c.y;
  if (c.y < 0) put('-');
  gdv_uint64 p = 1000;
  while (p * 10 <= ay) p *= 10;
  for (; p > 0; p /= 10) put('0' + (gdv_int64)(ay / p % 10));
  auto two = [&](gdv_int64 sep, gdv_int32 v) {
    put(sep);
    put('0' + v / 10);
    put('0' + v % 10);
  };
  two('-', c.m);
  two('-', c.d);
  two(' ', t / 3600000);
  two(':', t / 60000 % 60);
  two(':', t / 1000 % 60);
  put('.');
  put('0' + t % 1000 / 100);
  put('0' + t % 100 / 10);
  put('0' + t % 10);  // (bytes past the 24th are dropped)
  *w0 = a;
  *w1 = b;
  *w2 = e;
}
// bytes [0, len) of the text in w0 | w1 | w2, len <= 24: whole words, the tail as one overlapping word (or 4 + 4 bytes)
template <typename P>
GDV_DEV void gdv_dt_store(P dst, gdv_uint64 w0, gdv_uint64 w1, gdv_uint64 w2, gdv_int32 len) {
  if (len >= 8) {
    __builtin_memcpy(dst, &w0, 8);
    gdv_uint64 tail;
    if (len >= 16) {
      __builtin_memcpy(dst + 8, &w1, 8);
      if (len == 16) return;
      tail = (w1 >> (8 * (len - 16))) | (w2 << (8 * (24 - len)));
    } else {
      if (len == 8) return;
      tail = (w0 >> (8 * (len - 8))) | (w1 << (8 * (16 - len)));
    }
    __builtin_memcpy(dst + len - 8, &tail, 8);
  } else if (len >= 4) {
    const gdv_uint32 lo = (gdv_uint32)w0, hi = (gdv_uint32)(w0 >> (8 * (len - 4)));
    __builtin_memcpy(dst, &lo, 4);
    __builtin_memcpy(dst + len - 4, &hi, 4);
  } else {
    gdv_store_low_bytes(dst, w0, len);
  }
}
template <typename P>
GDV_DEV void gdv_copy_datetime(P dst, const gdv_str& s) {
  const gdv_int64 v = (gdv_int64)s.lead, days = gdv_floor_div(v, GDV_MILLIS_IN_DAY), r = v % GDV_MILLIS_IN_DAY;
  const gdv_int32 t = (gdv_int32)(r < 0 ? r + GDV_MILLIS_IN_DAY : r);  // (no days * GDV_MILLIS_IN_DAY: it overflows near INT64_MIN)
  const gdv_int32 h = t / 3600000, mi = t / 60000 % 60, sec = t / 1000 % 60, f = t % 1000;
  gdv_uint64 w0, w1, w2 = 0;
  if (((s.map >> 16) & 3) == 2) {  // hh:mm:ss.sss
    w0 = gdv_dt_pair(h) | (gdv_uint64)':' << 16 | gdv_dt_pair(mi) << 24 | (gdv_uint64)':' << 40 | gdv_dt_pair(sec) << 48;
    w1 = (gdv_uint64)'.' | (gdv_uint64)(0x30 + f / 100) << 8 | gdv_dt_pair(f % 100) << 16;
  } else {
    const gdv_ymd c = gdv_civil_from_days(days);
    if (c.y >= 0 && c.y <= 9999) {  // yyyy-MM-dd hh:mm:ss.sss (a date stops after dd)
      const gdv_int32 y = (gdv_int32)c.y;
      w0 = gdv_dt_pair(y / 100) | gdv_dt_pair(y % 100) << 16 | (gdv_uint64)'-' << 32 | gdv_dt_pair(c.m) << 40 |
           (gdv_uint64)'-' << 56;
      w1 = gdv_dt_pair(c.d) | (gdv_uint64)' ' << 16 | gdv_dt_pair(h) << 24 | (gdv_uint64)':' << 40 | gdv_dt_pair(mi) << 48;
      w2 = (gdv_uint64)':' | gdv_dt_pair(sec) << 8 | (gdv_uint64)'.' << 24 | (gdv_uint64)(0x30 + f / 100) << 32 |
           gdv_dt_pair(f % 100) << 40;
    } else {
      gdv_dt_wide_year(c, t, &w0, &w1, &w2);
    }
  }
  gdv_dt_store(dst, w0, w1, w2, s.len);
}
// the copy entry points of plans that hold a castVARCHAR of a date / time: those values here, everything else as the plan
// would copy it without them (gdv_str_copy, or gdv_str_copy_ext when it also holds a translate())
GDV_DEV void gdv_str_copy_dt(gdv_uint8* dst, const gdv_str& s) {
  if (s.map & GDV_MAP_DATETIME) {
    gdv_copy_datetime(dst, s);
    return;
  }
  gdv_str_copy(dst, s);
}
GDV_DEV void gdv_str_copy_ext_dt(gdv_uint8* dst, const gdv_str& s) {
  if (s.map & GDV_MAP_DATETIME) {
    gdv_copy_datetime(dst, s);
    return;
  }
  gdv_str_copy_ext(dst, s);
}

// ------------------------------------------------------------------ hex / unhex / base64 / unbase64 / crc32 over text and binary
// (to_hex and from_hex are other names of hex and unhex.)  Every function is null if null.
//   hex(t):      two UPPER-case hex digits per byte, in byte order.  hex(int32 / int64): the two's-complement value as
//                %X / %lX — upper case, no leading zeros, 0 -> "0".  [letter case and negative integers: recollection]
//   unhex(text): one byte per two hex digits of either letter case; an odd length or a byte that is not a hex digit
//                raises GDV_ERR_BAD_ARG.  [raise rather than NULL: recollection]
//   base64(t):   RFC 4648, standard alphabet, '=' padding, no line breaks.
//   unbase64(text): the inverse.  The length must be a multiple of 4, every byte an alphabet byte, '=' only in the last one or
//                two positions (xx==, xxx=); anything else raises.  The unused low bits of the last digit before the padding
//                are not checked.  [decided here]
//   crc32(t):    the zlib / IEEE 802.3 CRC-32 (reflected 0xEDB88320, initial value and final XOR 0xFFFFFFFF) of the bytes, as a
//                non-negative int64; crc32("") = 0.  [widened to int64: recollection]
// The four var-len results are values of one kind, GDV_MAP_ENCODE, which is NOT one of GDV_MAP_SPECIAL: only plans that hold
// one copy their outputs through the *_enc entry points below.  p / lim / flags & GDV_STR_INBUF / map & GDV_MAP_CASE describe
// the SOURCE view, `lead` is its length, `len` the length of the result and (map >> 16) & 7 the sub-kind.  The length of a
// result follows from the source's length alone (unbase64: and from its last two bytes, the padding), so the functions read
// no byte of the text; the copy reads the source 8 bytes at a time through its case map, converts the word in registers
// (SWAR) and stores whole words plus one overlapping tail word.  The decoders validate the words they convert and raise
// there, once per row, through the error word kept in `lead_p`.
#define GDV_MAP_ENCODE 32768
#define GDV_ENC_HEX 0
#define GDV_ENC_UNHEX 1
#define GDV_ENC_BASE64 2
#define GDV_ENC_UNBASE64 3
#define GDV_ENC_HEXINT 4  // `lead` is the integer itself

GDV_DEV gdv_str gdv_enc_value(const gdv_str& s, gdv_int64 len, gdv_int32 sub) {
  gdv_str r = s;
  r.lead = (gdv_uint64)(s.len > 0 ? s.len : 0);
  r.lead_p = nullptr;
  r.len = (gdv_int32)len;
  r.flags = s.flags & GDV_STR_INBUF;
  r.map = GDV_MAP_ENCODE | (sub << 16) | (s.map & GDV_MAP_CASE);
  return r;
}
// the result lengths (INT32_MAX bytes at most: longer results raise, as repeat's do)
GDV_DEV gdv_str hex_utf8(gdv_ctx ctx, gdv_str s) {
  if (s.len <= 0) return gdv_empty_str();
  if (s.len > 0x3fffffff) {
    gdv_raise(ctx, GDV_ERR_BAD_ARG);
    return gdv_empty_str();
  }
  return gdv_enc_value(s, 2ll * s.len, GDV_ENC_HEX);
}
GDV_DEV gdv_str hex_binary(gdv_ctx ctx, gdv_str s) { return hex_utf8(ctx, s); }
GDV_DEV gdv_str base64_utf8(gdv_ctx ctx, gdv_str s) {
  if (s.len <= 0) return gdv_empty_str();
  const gdv_int64 len = ((gdv_int64)s.len + 2) / 3 * 4;
  if (len > 0x7fffffffll) {
    gdv_raise(ctx, GDV_ERR_BAD_ARG);
    return gdv_empty_str();
  }
  return gdv_enc_value(s, len, GDV_ENC_BASE64);
}
GDV_DEV gdv_str base64_binary(gdv_ctx ctx, gdv_str s) { return base64_utf8(ctx, s); }
GDV_DEV gdv_str unhex_utf8(gdv_ctx ctx, gdv_str s) {
  if (s.len <= 0) return gdv_empty_str();
  if (s.len & 1) {
    gdv_raise(ctx, GDV_ERR_BAD_ARG);
    return gdv_empty_str();
  }
  gdv_str r = gdv_enc_value(s, s.len / 2, GDV_ENC_UNHEX);
  r.lead_p = (const gdv_uint8*)ctx.err;
  return r;
}
GDV_DEV gdv_str unbase64_utf8(gdv_ctx ctx, gdv_str s) {
  if (s.len <= 0) return gdv_empty_str();
  if (s.len & 3) {
    gdv_raise(ctx, GDV_ERR_BAD_ARG);
    return gdv_empty_str();
  }
  // the padding: the row's last two bytes, out of its last word
  const gdv_uint32 last2 = (gdv_uint32)(s.len >= 8 ? gdv_raw_word_at(s, s.len - 8) >> 48 : gdv_raw_word_at(s, 0) >> (8 * (s.len - 2))) & 0xffffu;
  const gdv_int32 pad = (last2 >> 8) != '=' ? 0 : (last2 & 0xffu) != '=' ? 1 : 2;
  gdv_str r = gdv_enc_value(s, s.len / 4 * 3 - pad, GDV_ENC_UNBASE64);  // (at least one byte)
  r.lead_p = (const gdv_uint8*)ctx.err;
  return r;
}
// hex of an integer: `bits` = 32 or 64, the width whose two's complement is printed
GDV_DEV gdv_str gdv_enc_hex_int(gdv_uint64 v, gdv_int32 bits) {
  gdv_str r = gdv_empty_str();
  if (bits == 32) v &= 0xffffffffull;
  r.lead = v;
  r.len = v == 0 ? 1 : (67 - __builtin_clzll(v)) / 4;
  r.flags = 0;
  r.map = GDV_MAP_ENCODE | (GDV_ENC_HEXINT << 16);
  return r;
}
GDV_DEV gdv_str hex_int32(gdv_ctx ctx, gdv_int32 v) { return gdv_enc_hex_int((gdv_uint64)(gdv_uint32)v, 32); }
GDV_DEV gdv_str hex_int64(gdv_ctx ctx, gdv_int64 v) { return gdv_enc_hex_int((gdv_uint64)v, 64); }

// ---- the word conversions
// bytes b0..b3 of x as eight upper-case hex digits, b0's high digit in the low byte (the nibble spread, then gdv_hex8's
// digit / letter select with 'A' - '9' - 1 = 7 in place of 39)
GDV_DEV gdv_uint64 gdv_enc_hex4(gdv_uint32 x) {
  gdv_uint64 t = x;
  t = (t | (t << 16)) & 0x0000ffff0000ffffull;
  t = (t | (t << 8)) & 0x00ff00ff00ff00ffull;  // one source byte per 16 bits
  const gdv_uint64 v = ((t >> 4) & 0x000f000f000f000full) | ((t & 0x000f000f000f000full) << 8);
  const gdv_uint64 letter = ((v + 0x0606060606060606ull) >> 4) & 0x0101010101010101ull;  // 1 where the nibble is 10..15
  return v + 0x3030303030303030ull + letter * 7ull;
}
// gdv_hex8 in upper case: eight hex digits of x, most significant first
GDV_DEV gdv_uint64 gdv_hex8_upper(gdv_uint32 x) { return gdv_enc_hex4(__builtin_bswap32(x)); }
// 1 in every byte of h (all bytes < 0x80) that lies in [lo, hi]: a = 0x80 - lo, b = 0x7f - hi in every byte
GDV_DEV gdv_uint64 gdv_enc_range(gdv_uint64 h, gdv_uint64 a, gdv_uint64 b) { return (((h + a) & ~(h + b)) >> 7) & 0x0101010101010101ull; }
// the 4 bytes the eight hex digits of w spell; *bad becomes non-zero when a byte of w is not a hex digit
GDV_DEV gdv_uint32 gdv_enc_unhex8(gdv_uint64 w, gdv_uint64* bad) {
  const gdv_uint64 h = w & GDV_B7F, one = 0x0101010101010101ull;
  const gdv_uint64 digit = gdv_enc_range(h, 0x5050505050505050ull, 0x4646464646464646ull);                              // '0'..'9'
  const gdv_uint64 letter = gdv_enc_range(h & 0x5f5f5f5f5f5f5f5full, 0x3f3f3f3f3f3f3f3full, 0x3939393939393939ull);  // 'A'..'F', 'a'..'f'
  *bad |= ((digit | letter) ^ one) | ((w >> 7) & one);
  const gdv_uint64 n = (h & 0x0f0f0f0f0f0f0f0full) + letter * 9ull;
  gdv_uint64 p = ((n << 4) | (n >> 8)) & 0x00ff00ff00ff00ffull;  // one result byte per 16 bits
  p = (p | (p >> 8)) & 0x0000ffff0000ffffull;
  return (gdv_uint32)(p | (p >> 16));
}
// the four sextets of the bytes b0 b1 b2 (the low three bytes of x), the first in the low byte
GDV_DEV gdv_uint32 gdv_enc_sextets(gdv_uint32 x) {
  const gdv_uint32 t = __builtin_bswap32(x) >> 8;  // b0 << 16 | b1 << 8 | b2
  return ((t >> 18) & 0x3fu) | ((t >> 4) & 0x3f00u) | ((t << 10) & 0x3f0000u) | ((t << 24) & 0x3f000000u);
}
// eight sextets (one per byte) -> their alphabet bytes: 'A' + s, + 6 from 26 ('a'), - 75 from 52 ('0'), - 15 at 62 ('+'),
// + 3 at 63 ('/') — range compares on the word, no table
GDV_DEV gdv_uint64 gdv_enc_b64_chars(gdv_uint64 s) {
  const gdv_uint64 one = 0x0101010101010101ull;
  const gdv_uint64 ge26 = ((s + 0x6666666666666666ull) >> 7) & one, ge52 = ((s + 0x4c4c4c4c4c4c4c4cull) >> 7) & one;
  const gdv_uint64 ge62 = ((s + 0x4242424242424242ull) >> 7) & one, ge63 = ((s + 0x4141414141414141ull) >> 7) & one;
  return s + 0x4141414141414141ull + ge26 * 6ull + ge63 * 3ull - ge52 * 75ull - ge62 * 15ull;
}
// the eight alphabet bytes of the 6 source bytes in the low 48 bits of w
GDV_DEV gdv_uint64 gdv_enc_b64_word(gdv_uint64 w) {
  return gdv_enc_b64_chars((gdv_uint64)gdv_enc_sextets((gdv_uint32)w) | (gdv_uint64)gdv_enc_sextets((gdv_uint32)(w >> 24)) << 32);
}
// the 6 bytes (low 48 bits) the eight alphabet bytes of w spell; *bad becomes non-zero when a byte is outside the alphabet
GDV_DEV gdv_uint64 gdv_enc_unb64_word(gdv_uint64 w, gdv_uint64* bad) {
  const gdv_uint64 h = w & GDV_B7F, one = 0x0101010101010101ull;
  const gdv_uint64 up = gdv_enc_range(h, 0x3f3f3f3f3f3f3f3full, 0x2525252525252525ull);     // 'A'..'Z' -> 0..25
  const gdv_uint64 low = gdv_enc_range(h, 0x1f1f1f1f1f1f1f1full, 0x0505050505050505ull);    // 'a'..'z' -> 26..51
  const gdv_uint64 dig = gdv_enc_range(h, 0x5050505050505050ull, 0x4646464646464646ull);    // '0'..'9' -> 52..61
  const gdv_uint64 plus = gdv_enc_range(h, 0x5555555555555555ull, 0x5454545454545454ull);   // '+' -> 62
  const gdv_uint64 slash = gdv_enc_range(h, 0x5151515151515151ull, 0x5050505050505050ull);  // '/' -> 63
  *bad |= ((up | low | dig | plus | slash) ^ one) | ((w >> 7) & one);
  const gdv_uint64 s = (h + dig * 4ull + plus * 19ull + slash * 16ull - up * 65ull - low * 71ull) & 0x3f3f3f3f3f3f3f3full;
  const gdv_uint32 a = (gdv_uint32)s, b = (gdv_uint32)(s >> 32);
  const gdv_uint32 na = (a & 0x3fu) << 18 | (a & 0x3f00u) << 4 | (a & 0x3f0000u) >> 10 | a >> 24;  // s0 << 18 | s1 << 12 | s2 << 6 | s3
  const gdv_uint32 nb = (b & 0x3fu) << 18 | (b & 0x3f00u) << 4 | (b & 0x3f0000u) >> 10 | b >> 24;
  return (gdv_uint64)(__builtin_bswap32(na) >> 8) | (gdv_uint64)(__builtin_bswap32(nb) >> 8) << 24;
}
// bytes [0, len) of w, len in 1..8: one word, two overlapping half words, or the 2 + 1 ladder
template <typename P>
GDV_DEV void gdv_enc_store_short(P dst, gdv_uint64 w, gdv_int32 len) {
  if (len >= 8) {
    __builtin_memcpy(dst, &w, 8);
  } else if (len >= 4) {
    const gdv_uint32 lo = (gdv_uint32)w, hi = (gdv_uint32)(w >> (8 * (len - 4)));
    __builtin_memcpy(dst, &lo, 4);
    __builtin_memcpy(dst + len - 4, &hi, 4);
  } else {
    gdv_store_low_bytes(dst, w, len);
  }
}
// A result written as a stream of words: `acc` holds the `n` (0..7) bytes not stored yet, `last` the word stored before
// them, `at` the bytes stored.  gdv_enc_put appends the low k (1..8) bytes of w (the bytes above them are zero);
// gdv_enc_finish stores the rest as one word that overlaps the last one (a result below 8 bytes: gdv_enc_store_short).
template <typename P>
GDV_DEV void gdv_enc_put(P dst, gdv_uint64& acc, gdv_uint64& last, gdv_int32& n, gdv_int32& at, gdv_uint64 w, gdv_int32 k) {
  acc |= w << (8 * n);
  if (n + k >= 8) {
    __builtin_memcpy(dst + at, &acc, 8);
    last = acc;
    at += 8;
    acc = n > 0 ? w >> (8 * (8 - n)) : 0ull;
    n += k - 8;
  } else {
    n += k;
  }
}
template <typename P>
GDV_DEV void gdv_enc_finish(P dst, gdv_uint64 acc, gdv_uint64 last, gdv_int32 n, gdv_int32 at) {
  if (n == 0) return;
  if (at > 0) {
    const gdv_uint64 tail = (last >> (8 * n)) | (acc << (8 * (8 - n)));
    __builtin_memcpy(dst + at + n - 8, &tail, 8);
  } else {
    gdv_enc_store_short(dst, acc, n);
  }
}
// the source view of an encode value, read through its case map
GDV_DEV gdv_str gdv_enc_source(const gdv_str& s) {
  gdv_str src = s;
  src.len = (gdv_int32)s.lead;
  src.map = s.map & GDV_MAP_CASE;
  src.flags = s.flags & GDV_STR_INBUF;
  return src;
}
template <typename P>
GDV_DEV void gdv_copy_hex(P dst, const gdv_str& s) {
  const gdv_str src = gdv_enc_source(s);
  const gdv_int32 n = src.len;
  gdv_int32 i = 0;
  for (; i + 8 <= n; i += 8) {
    const gdv_uint64 w = gdv_word_at(src, i);
    const gdv_uint64 a = gdv_enc_hex4((gdv_uint32)w), b = gdv_enc_hex4((gdv_uint32)(w >> 32));
    __builtin_memcpy(dst + 2 * i, &a, 8);
    __builtin_memcpy(dst + 2 * i + 8, &b, 8);
  }
  if (n - i >= 4) {
    const gdv_uint64 a = gdv_enc_hex4((gdv_uint32)gdv_word_at(src, i));
    __builtin_memcpy(dst + 2 * i, &a, 8);
    i += 4;
  }
  if (i == n) return;
  if (n >= 4) {  // the last four source bytes again: one word that overlaps what is written
    const gdv_uint64 a = gdv_enc_hex4((gdv_uint32)gdv_word_at(src, n - 4));
    __builtin_memcpy(dst + 2 * n - 8, &a, 8);
  } else {
    gdv_enc_store_short(dst, gdv_enc_hex4((gdv_uint32)gdv_word_at(src, 0)), 2 * n);
  }
}
template <typename P>
GDV_DEV void gdv_copy_hex_int(P dst, const gdv_str& s) {
  const gdv_uint64 w0 = gdv_hex8_upper((gdv_uint32)(s.lead >> 32)), w1 = gdv_hex8_upper((gdv_uint32)s.lead);
  const gdv_int32 skip = 16 - s.len;  // leading zeros that are not printed
  gdv_uint64 o0, o1 = 0;
  if (skip >= 8) {
    o0 = w1 >> (8 * (skip - 8));
  } else if (skip > 0) {
    o0 = (w0 >> (8 * skip)) | (w1 << (8 * (8 - skip)));
    o1 = w1 >> (8 * skip);
  } else {
    o0 = w0;
    o1 = w1;
  }
  gdv_dt_store(dst, o0, o1, 0ull, s.len);
}
template <typename P>
GDV_DEV void gdv_copy_unhex(P dst, const gdv_str& s) {
  const gdv_str src = gdv_enc_source(s);
  const gdv_int32 n = src.len, out = s.len;  // n = 2 * out
  gdv_uint64 bad = 0;
  gdv_int32 i = 0;
  for (; i + 16 <= n; i += 16) {
    const gdv_uint64 w = (gdv_uint64)gdv_enc_unhex8(gdv_word_at(src, i), &bad) | (gdv_uint64)gdv_enc_unhex8(gdv_word_at(src, i + 8), &bad) << 32;
    __builtin_memcpy(dst + i / 2, &w, 8);
  }
  if (i < n) {
    if (n >= 16) {  // the last sixteen digits again: one word that overlaps what is written
      const gdv_uint64 w = (gdv_uint64)gdv_enc_unhex8(gdv_word_at(src, n - 16), &bad) | (gdv_uint64)gdv_enc_unhex8(gdv_word_at(src, n - 8), &bad) << 32;
      __builtin_memcpy(dst + out - 8, &w, 8);
    } else {  // 2..14 digits: the bytes past them read as '0'
      const gdv_uint64 zeros = 0x3030303030303030ull;
      const gdv_uint64 m0 = gdv_low_bytes_mask(n), m1 = gdv_low_bytes_mask(n > 8 ? n - 8 : 0);
      const gdv_uint64 w0 = (gdv_word_at(src, 0) & m0) | (zeros & ~m0);
      const gdv_uint64 w1 = n > 8 ? (gdv_word_at(src, 8) & m1) | (zeros & ~m1) : zeros;
      gdv_enc_store_short(dst, (gdv_uint64)gdv_enc_unhex8(w0, &bad) | (gdv_uint64)gdv_enc_unhex8(w1, &bad) << 32, out);
    }
  }
  if (bad != 0) gdv_raise_bits((gdv_uint32*)s.lead_p, GDV_ERR_BAD_ARG);
}
template <typename P>
GDV_DEV void gdv_copy_base64(P dst, const gdv_str& s) {
  const gdv_str src = gdv_enc_source(s);
  const gdv_int32 n = src.len;
  gdv_int32 i = 0, o = 0;
  for (; i + 6 <= n; i += 6, o += 8) {  // (the word's last two bytes belong to the next step)
    const gdv_uint64 c = gdv_enc_b64_word(gdv_word_at(src, i));
    __builtin_memcpy(dst + o, &c, 8);
  }
  const gdv_int32 r = n - i;  // 0..5 bytes left: 4 or 8 more bytes of text, '=' where a sextet has no source byte
  if (r == 0) return;
  gdv_uint64 c = gdv_enc_b64_word(gdv_word_at(src, i) & gdv_low_bytes_mask(r));
  const gdv_uint64 eq = 0x3d3d3d3d3d3d3d3dull;
  const gdv_int32 keep = r + 1 + (r > 3 ? 1 : 0);  // alphabet bytes: 2, 3, 4, 6, 7
  if (r != 3) c = (c & gdv_low_bytes_mask(keep)) | (eq & ~gdv_low_bytes_mask(keep));
  if (r > 3) {
    __builtin_memcpy(dst + o, &c, 8);
  } else {
    const gdv_uint32 c4 = (gdv_uint32)c;
    __builtin_memcpy(dst + o, &c4, 4);
  }
}
template <typename P>
GDV_DEV void gdv_copy_unbase64(P dst, const gdv_str& s) {
  const gdv_str src = gdv_enc_source(s);
  const gdv_int32 n = src.len, out = s.len, pad = n / 4 * 3 - out;  // n is a multiple of 4, pad 0..2
  gdv_uint64 bad = 0, acc = 0, last = 0;
  gdv_int32 fill = 0, at = 0;
  for (gdv_int32 i = 0; i < n; i += 8) {
    // the characters of this step: 8, or the text's last 4; the one or two '=' that end the text, like the bytes past it,
    // count as 'A'
    const gdv_int32 nc = (n - i < 8 ? 4 : 8) - (i + 8 >= n ? pad : 0);
    const gdv_uint64 w = (gdv_word_at(src, i) & gdv_low_bytes_mask(nc)) | (0x4141414141414141ull & ~gdv_low_bytes_mask(nc));
    const gdv_uint64 b = gdv_enc_unb64_word(w, &bad);
    const gdv_int32 k = out - (i / 8 * 6) < 6 ? out - (i / 8 * 6) : 6;  // result bytes of this step
    gdv_enc_put(dst, acc, last, fill, at, b & gdv_low_bytes_mask(k), k);
  }
  gdv_enc_finish(dst, acc, last, fill, at);
  if (bad != 0) gdv_raise_bits((gdv_uint32*)s.lead_p, GDV_ERR_BAD_ARG);
}
template <typename P>
GDV_DEV void gdv_copy_encode(P dst, const gdv_str& s) {
  const gdv_int32 sub = (s.map >> 16) & 7;
  if (sub == GDV_ENC_HEX) gdv_copy_hex(dst, s);
  else if (sub == GDV_ENC_BASE64) gdv_copy_base64(dst, s);
  else if (sub == GDV_ENC_UNHEX) gdv_copy_unhex(dst, s);
  else if (sub == GDV_ENC_UNBASE64) gdv_copy_unbase64(dst, s);
  else gdv_copy_hex_int(dst, s);
}

// ---- crc32: slice-by-8 — eight table reads and seven XORs per 8 source bytes, the tail's r < 8 bytes with r reads.  The
// tables (8 KiB) are computed when the kernel is compiled and sit in its constant data.
struct gdv_crc32_tables {
  gdv_uint32 t[8][256];
  constexpr gdv_crc32_tables() : t() {
    for (gdv_uint32 i = 0; i < 256; i++) {
      gdv_uint32 c = i;
      for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
      t[0][i] = c;
    }
    for (int k = 1; k < 8; k++)
      for (gdv_uint32 i = 0; i < 256; i++) t[k][i] = t[0][t[k - 1][i] & 0xffu] ^ (t[k - 1][i] >> 8);
  }
};
GDV_DEV gdv_int64 gdv_crc32_buf(const gdv_str& s) {
  static constexpr gdv_crc32_tables T{};
  gdv_uint32 crc = 0xffffffffu;
  gdv_int32 i = 0;
  for (; i + 8 <= s.len; i += 8) {
    const gdv_uint64 x = gdv_word_at(s, i) ^ (gdv_uint64)crc;
    crc = T.t[7][x & 0xff] ^ T.t[6][(x >> 8) & 0xff] ^ T.t[5][(x >> 16) & 0xff] ^ T.t[4][(x >> 24) & 0xff] ^
          T.t[3][(x >> 32) & 0xff] ^ T.t[2][(x >> 40) & 0xff] ^ T.t[1][(x >> 48) & 0xff] ^ T.t[0][x >> 56];
  }
  const gdv_int32 r = s.len - i;
  if (r > 0) {  // byte j of the last r: table r - 1 - j; the state's bytes past them move down
    const gdv_uint64 x = (gdv_word_at(s, i) & gdv_low_bytes_mask(r)) ^ (gdv_uint64)crc;
    crc = r < 4 ? crc >> (8 * r) : 0u;
#pragma unroll
    for (int j = 0; j < 7; j++)
      if (j < r) crc ^= T.t[(r - 1 - j) & 7][(x >> (8 * j)) & 0xff];
  }
  return (gdv_int64)(crc ^ 0xffffffffu);
}
GDV_DEV gdv_int64 crc32_utf8(gdv_str s) { return gdv_crc32_buf(s); }
GDV_DEV gdv_int64 crc32_binary(gdv_str s) { return gdv_crc32_buf(s); }

// the copy entry points of plans that hold an encode value: those values here, everything else as the plan would copy it
// without them
GDV_DEV void gdv_str_copy_enc(gdv_uint8* dst, const gdv_str& s) {
  if (s.map & GDV_MAP_ENCODE) {
    gdv_copy_encode(dst, s);
    return;
  }
  gdv_str_copy(dst, s);
}
GDV_DEV void gdv_str_copy_ext_enc(gdv_uint8* dst, const gdv_str& s) {
  if (s.map & GDV_MAP_ENCODE) {
    gdv_copy_encode(dst, s);
    return;
  }
  gdv_str_copy_ext(dst, s);
}
GDV_DEV void gdv_str_copy_dt_enc(gdv_uint8* dst, const gdv_str& s) {
  if (s.map & GDV_MAP_ENCODE) {
    gdv_copy_encode(dst, s);
    return;
  }
  gdv_str_copy_dt(dst, s);
}
GDV_DEV void gdv_str_copy_ext_dt_enc(gdv_uint8* dst, const gdv_str& s) {
  if (s.map & GDV_MAP_ENCODE) {
    gdv_copy_encode(dst, s);
    return;
  }
  gdv_str_copy_ext_dt(dst, s);
}

#ifndef GDV_HOST_BUILD
// the value the NEXT lane holds (lane 63 gets 0): DPP wave_shl:1, no LDS traffic
GDV_DEV gdv_uint64 gdv_next_lane(gdv_uint64 v) {
  const gdv_uint32 lo = (gdv_uint32)__builtin_amdgcn_update_dpp(0, (int)(gdv_uint32)v, 0x130, 0xf, 0xf, false);
  const gdv_uint32 hi = (gdv_uint32)__builtin_amdgcn_update_dpp(0, (int)(gdv_uint32)(v >> 32), 0x130, 0xf, 0xf, false);
  return ((gdv_uint64)hi << 32) | lo;
}

// the END offset of each lane's row when only the start offsets were loaded: the next lane's
// start (DPP wave_shl:1), lane 63 takes `after` = the first start of the next sub-tile / the tile's end
GDV_DEV gdv_int32 gdv_next_lane_i32(gdv_int32 v, gdv_int32 after, int lane) {
  const gdv_int32 nx = __builtin_amdgcn_update_dpp(0, v, 0x130, 0xf, 0xf, false);
  return lane == 63 ? after : nx;
}

// ---- staged copies of kernels whose replace() is answered by the sweep: the SOURCE row of a
// replace() value inside the mirrored span is copied from LDS along the marked positions;
// everything else as gdv_stage_copy_mir
struct gdv_rd_lds {
  const gdv_lds_u8* mir;
  gdv_int32 d;  // offset of the row's first byte inside the mirror
  __device__ __forceinline__ gdv_uint64 operator()(gdv_int32 k) const { return gdv_mirror_word(mir, d + k); }
};
GDV_DEV void gdv_stage_copy_mirh(gdv_lds_u8* dst, const gdv_str& s, const gdv_lds_u8* mir, const gdv_uint8* mbase,
                                 gdv_int32 mlen, const gdv_uint64* bm) {
  if (s.map & GDV_MAP_REPLACE) {
    const gdv_int64 d64 = s.p - mbase;
    const gdv_int32 src = s.flags >> 2;
    if ((s.map & GDV_MAP_HITS) && d64 >= 0 && d64 + src <= (gdv_int64)mlen)
      gdv_copy_replaced_hits(dst, s, gdv_rd_lds{mir, (gdv_int32)d64}, bm, (gdv_int32)d64);
    else
      gdv_copy_special(dst, s);
    return;
  }
  gdv_stage_copy_mir(dst, s, mir, mbase, mlen);
}

// the staged copies of plans that hold a translate() (gdv_str_copy_ext's counterparts)
GDV_DEV void gdv_stage_copy_ext(gdv_lds_u8* dst, const gdv_str& s) {
  if (s.map & GDV_MAP_TRANSLATE) {
    gdv_copy_translated(dst, s);
    return;
  }
  gdv_stage_copy(dst, s);
}
GDV_DEV void gdv_stage_copy_mir_ext(gdv_lds_u8* dst, const gdv_str& s, const gdv_lds_u8* mir, const gdv_uint8* mbase,
                                    gdv_int32 mlen) {
  if (s.map & GDV_MAP_TRANSLATE) {
    gdv_copy_translated(dst, s);
    return;
  }
  gdv_stage_copy_mir(dst, s, mir, mbase, mlen);
}
GDV_DEV void gdv_stage_copy_mirh_ext(gdv_lds_u8* dst, const gdv_str& s, const gdv_lds_u8* mir, const gdv_uint8* mbase,
                                     gdv_int32 mlen, const gdv_uint64* bm) {
  if (s.map & GDV_MAP_TRANSLATE) {
    gdv_copy_translated(dst, s);
    return;
  }
  gdv_stage_copy_mirh(dst, s, mir, mbase, mlen, bm);
}

// the staged copies of plans that hold a castVARCHAR of a date / time (gdv_str_copy_dt's counterparts)
GDV_DEV void gdv_stage_copy_dt(gdv_lds_u8* dst, const gdv_str& s) {
  if (s.map & GDV_MAP_DATETIME) {
    gdv_copy_datetime(dst, s);
    return;
  }
  gdv_stage_copy(dst, s);
}
GDV_DEV void gdv_stage_copy_mir_dt(gdv_lds_u8* dst, const gdv_str& s, const gdv_lds_u8* mir, const gdv_uint8* mbase,
                                   gdv_int32 mlen) {
  if (s.map & GDV_MAP_DATETIME) {
    gdv_copy_datetime(dst, s);
    return;
  }
  gdv_stage_copy_mir(dst, s, mir, mbase, mlen);
}
GDV_DEV void gdv_stage_copy_mirh_dt(gdv_lds_u8* dst, const gdv_str& s, const gdv_lds_u8* mir, const gdv_uint8* mbase,
                                    gdv_int32 mlen, const gdv_uint64* bm) {
  if (s.map & GDV_MAP_DATETIME) {
    gdv_copy_datetime(dst, s);
    return;
  }
  gdv_stage_copy_mirh(dst, s, mir, mbase, mlen, bm);
}
GDV_DEV void gdv_stage_copy_ext_dt(gdv_lds_u8* dst, const gdv_str& s) {
  if (s.map & GDV_MAP_DATETIME) {
    gdv_copy_datetime(dst, s);
    return;
  }
  gdv_stage_copy_ext(dst, s);
}
GDV_DEV void gdv_stage_copy_mir_ext_dt(gdv_lds_u8* dst, const gdv_str& s, const gdv_lds_u8* mir, const gdv_uint8* mbase,
                                       gdv_int32 mlen) {
  if (s.map & GDV_MAP_DATETIME) {
    gdv_copy_datetime(dst, s);
    return;
  }
  gdv_stage_copy_mir_ext(dst, s, mir, mbase, mlen);
}
GDV_DEV void gdv_stage_copy_mirh_ext_dt(gdv_lds_u8* dst, const gdv_str& s, const gdv_lds_u8* mir, const gdv_uint8* mbase,
                                        gdv_int32 mlen, const gdv_uint64* bm) {
  if (s.map & GDV_MAP_DATETIME) {
    gdv_copy_datetime(dst, s);
    return;
  }
  gdv_stage_copy_mirh_ext(dst, s, mir, mbase, mlen, bm);
}

// the staged copies of plans that hold an encode value (gdv_str_copy_enc's counterparts)
GDV_DEV void gdv_stage_copy_enc(gdv_lds_u8* dst, const gdv_str& s) {
  if (s.map & GDV_MAP_ENCODE) {
    gdv_copy_encode(dst, s);
    return;
  }
  gdv_stage_copy(dst, s);
}
GDV_DEV void gdv_stage_copy_mir_enc(gdv_lds_u8* dst, const gdv_str& s, const gdv_lds_u8* mir, const gdv_uint8* mbase, gdv_int32 mlen) {
  if (s.map & GDV_MAP_ENCODE) {
    gdv_copy_encode(dst, s);
    return;
  }
  gdv_stage_copy_mir(dst, s, mir, mbase, mlen);
}
GDV_DEV void gdv_stage_copy_mirh_enc(gdv_lds_u8* dst, const gdv_str& s, const gdv_lds_u8* mir, const gdv_uint8* mbase, gdv_int32 mlen, const gdv_uint64* bm) {
  if (s.map & GDV_MAP_ENCODE) {
    gdv_copy_encode(dst, s);
    return;
  }
  gdv_stage_copy_mirh(dst, s, mir, mbase, mlen, bm);
}
GDV_DEV void gdv_stage_copy_ext_enc(gdv_lds_u8* dst, const gdv_str& s) {
  if (s.map & GDV_MAP_ENCODE) {
    gdv_copy_encode(dst, s);
    return;
  }
  gdv_stage_copy_ext(dst, s);
}
GDV_DEV void gdv_stage_copy_mir_ext_enc(gdv_lds_u8* dst, const gdv_str& s, const gdv_lds_u8* mir, const gdv_uint8* mbase, gdv_int32 mlen) {
  if (s.map & GDV_MAP_ENCODE) {
    gdv_copy_encode(dst, s);
    return;
  }
  gdv_stage_copy_mir_ext(dst, s, mir, mbase, mlen);
}
GDV_DEV void gdv_stage_copy_mirh_ext_enc(gdv_lds_u8* dst, const gdv_str& s, const gdv_lds_u8* mir, const gdv_uint8* mbase, gdv_int32 mlen, const gdv_uint64* bm) {
  if (s.map & GDV_MAP_ENCODE) {
    gdv_copy_encode(dst, s);
    return;
  }
  gdv_stage_copy_mirh_ext(dst, s, mir, mbase, mlen, bm);
}
GDV_DEV void gdv_stage_copy_dt_enc(gdv_lds_u8* dst, const gdv_str& s) {
  if (s.map & GDV_MAP_ENCODE) {
    gdv_copy_encode(dst, s);
    return;
  }
  gdv_stage_copy_dt(dst, s);
}
GDV_DEV void gdv_stage_copy_mir_dt_enc(gdv_lds_u8* dst, const gdv_str& s, const gdv_lds_u8* mir, const gdv_uint8* mbase, gdv_int32 mlen) {
  if (s.map & GDV_MAP_ENCODE) {
    gdv_copy_encode(dst, s);
    return;
  }
  gdv_stage_copy_mir_dt(dst, s, mir, mbase, mlen);
}
GDV_DEV void gdv_stage_copy_mirh_dt_enc(gdv_lds_u8* dst, const gdv_str& s, const gdv_lds_u8* mir, const gdv_uint8* mbase, gdv_int32 mlen, const gdv_uint64* bm) {
  if (s.map & GDV_MAP_ENCODE) {
    gdv_copy_encode(dst, s);
    return;
  }
  gdv_stage_copy_mirh_dt(dst, s, mir, mbase, mlen, bm);
}
GDV_DEV void gdv_stage_copy_ext_dt_enc(gdv_lds_u8* dst, const gdv_str& s) {
  if (s.map & GDV_MAP_ENCODE) {
    gdv_copy_encode(dst, s);
    return;
  }
  gdv_stage_copy_ext_dt(dst, s);
}
GDV_DEV void gdv_stage_copy_mir_ext_dt_enc(gdv_lds_u8* dst, const gdv_str& s, const gdv_lds_u8* mir, const gdv_uint8* mbase, gdv_int32 mlen) {
  if (s.map & GDV_MAP_ENCODE) {
    gdv_copy_encode(dst, s);
    return;
  }
  gdv_stage_copy_mir_ext_dt(dst, s, mir, mbase, mlen);
}
GDV_DEV void gdv_stage_copy_mirh_ext_dt_enc(gdv_lds_u8* dst, const gdv_str& s, const gdv_lds_u8* mir, const gdv_uint8* mbase, gdv_int32 mlen, const gdv_uint64* bm) {
  if (s.map & GDV_MAP_ENCODE) {
    gdv_copy_encode(dst, s);
    return;
  }
  gdv_stage_copy_mirh_ext_dt(dst, s, mir, mbase, mlen, bm);
}

// ------------------------------------------------------------------ small-batch filter: scan + emission in the predicate's own workgroup
// A batch of up to GDV_SMALL_MAX_TILES wave tiles (the reference's 4K-64K-row batches) is filtered
// by ONE workgroup in ONE launch: after its waves have run the predicate over every wave tile
// (match words -> `mask`, one count per wave tile -> `counts`), wave 0 prefix-sums the counts into
// LDS, then every wave turns 64 match words at a time into ascending row indices — the algorithm
// of the ahead-of-time scan / index-emission kernels (gdv_kernels.hip), which large batches keep
// using.  Several batches: one workgroup each (the grid's second dimension), still one launch.
#define GDV_SMALL_MAX_TILES 1024
typedef __attribute__((address_space(3))) gdv_uint32 gdv_lds_u32;
GDV_DEV void gdv_small_filter_finish(const gdv_uint64* __restrict__ mask, const gdv_uint32* __restrict__ counts,
                                     gdv_int64 n, void* __restrict__ out, gdv_int32 index_bytes,
                                     gdv_int64* __restrict__ count_out, gdv_uint32* lds_offsets,
                                     gdv_uint16* lds_stage, int lane, int wave, int nwaves, int subtiles) {
  const gdv_int64 nwords = (n + 63) >> 6;
  const gdv_int32 m = (gdv_int32)((nwords + subtiles - 1) / subtiles);  // wave tiles = counts
  if (wave == 0) {
    gdv_uint32 base = 0;
    for (gdv_int32 i0 = 0; i0 < m; i0 += 64) {
      const gdv_int32 i = i0 + lane;
      const gdv_int32 c = i < m ? (gdv_int32)counts[i] : 0;
      const gdv_int32 incl = gdv_wave_scan_incl(c);
      if (i < m) lds_offsets[i] = base + (gdv_uint32)(incl - c);
      base += (gdv_uint32)gdv_wave_last(incl);
    }
    if (lane == 0 && count_out != nullptr) *count_out = (gdv_int64)base;
  }
  __syncthreads();
  gdv_uint16* const buf = lds_stage + (gdv_int64)wave * (64 * 64);
  const gdv_int64 ntiles = (nwords + 63) / 64;  // emission tiles: 64 match words = 4096 rows
  for (gdv_int64 t = wave; t < ntiles; t += nwaves) {
    const gdv_int64 w = t * 64 + lane;
    gdv_uint64 bits = w < nwords ? mask[w] : 0ull;
    const gdv_uint32 base = lds_offsets[(t * 64) / subtiles];
    const gdv_int32 c = (gdv_int32)__popcll(bits);
    const gdv_int32 incl = gdv_wave_scan_incl(c);
    const gdv_uint32 total = (gdv_uint32)gdv_wave_last(incl);
    gdv_uint32 slot = (gdv_uint32)(incl - c);
    while (bits) {
      buf[slot++] = (gdv_uint16)((lane << 6) + __builtin_ctzll(bits));
      bits &= bits - 1;
    }
    __builtin_amdgcn_wave_barrier();
    const gdv_int64 row0 = t * 4096;
    for (gdv_uint32 j = (gdv_uint32)lane; j < total; j += 64) {
      const gdv_int64 v = row0 + buf[j];
      if (index_bytes == 4) ((gdv_uint32*)out)[base + j] = (gdv_uint32)v;
      else if (index_bytes == 2) ((gdv_uint16*)out)[base + j] = (gdv_uint16)v;
      else ((gdv_uint64*)out)[base + j] = (gdv_uint64)v;
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// ------------------------------------------------------------------ var-len kernels: output offsets
// ONE launch produces offsets and bytes: a workgroup tile (GDV_WAVES x GDV_U x 64 rows) needs the
// byte total of every tile before it.  Workers post their tile's totals as an 8-byte granule and
// poll ONE granule for the answer; a single scanner wave (workgroup 0) is the only reader of the
// posted totals: it resolves the longest posted run in bulk and writes every tile's exclusive
// prefix.  (Measured on MI355X, profiles/r02_k4_singlepass_proto.txt: agent-scope granule
// accesses are priced per lane-access at the fabric, so classic decoupled look-back — every
// tile polling up to 64 predecessors — costs more than the second pass it replaces.)
// Granule: bits 63..62 status (0 nothing, 1 posted), bits 61..31 and 30..0 two 31-bit values
// (two var-len outputs share a granule; Arrow offsets are int32, sums saturate at 2^31-1 and
// the host rejects such a total).  Relaxed agent-scope atomics: the granule is its own flag.
typedef __attribute__((address_space(1))) unsigned long long gdv_gu64;
#define GDV_LB_POSTED (1ull << 62)
#define GDV_LB_M31 0x7fffffffull
#ifndef GDV_LB_WSLEEP
#define GDV_LB_WSLEEP 4  // worker poll pace, in units of 64 clocks (sweep: profiles/r02_c5_poll_pace.txt)
#endif
#define GDV_ERR_STALL 8u
#ifndef GDV_LB_STALL_TICKS
#define GDV_LB_STALL_TICKS 500000000ull  // 5 s of the 100 MHz constant clock without progress = stalled
#endif
#define GDV_ERR_NOTFLAT 16u  // an optimistic flat output met a null row that carries bytes: host re-runs
#define GDV_ERR_NOTASCII 32u  // pre-scanned plan (lengths from offsets under the ASCII assumption) met a byte >= 0x80: host re-runs
#define GDV_ERR_SAWUTF8 64u   // exact variant of a wave plan: this batch did hold a byte >= 0x80 (not an error: the host keeps the exact kernels for the next batch)
GDV_DEV void gdv_lb_store(gdv_uint64* p, gdv_uint64 v) {
  __hip_atomic_store((gdv_gu64*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
GDV_DEV gdv_uint64 gdv_lb_load(const gdv_uint64* p) {
  return __hip_atomic_load((gdv_gu64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
GDV_DEV gdv_uint64 gdv_sat31(gdv_uint64 v) { return v > GDV_LB_M31 ? GDV_LB_M31 : v; }
GDV_DEV gdv_uint64 gdv_wave_excl_scan_u64(gdv_uint64 v, int lane, gdv_uint64* total) {
  gdv_uint64 incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const gdv_uint64 o = __shfl_up(incl, d, 64);
    if (lane >= d) incl += o;
  }
  *total = __shfl(incl, 63, 64);
  return incl - v;
}
// Scanner wave.  agg/pre: NG granule arrays of `ntiles` entries each (array g at g * ntiles).
// totals[2 * g], totals[2 * g + 1]: grand totals of the two values of granule g.
// Bounded: if nothing is posted for a very long time the scanner raises GDV_ERR_STALL and
// leaves (the host then re-runs the batch in the serial-safe configuration).
template <int NG>
GDV_DEV void gdv_scanner(const gdv_uint64* agg, gdv_uint64* pre, gdv_int64 ntiles, gdv_uint64* totals,
                         gdv_uint32* err, int lane) {
  constexpr int K = 8;
  gdv_int64 pos[NG];
  gdv_uint64 c0[NG], c1[NG];
#pragma unroll
  for (int g = 0; g < NG; g++) { pos[g] = 0; c0[g] = 0; c1[g] = 0; }
  gdv_uint32 idle = 0;
  gdv_uint64 idle_since = 0;
  for (;;) {
    bool all_done = true, progressed = false;
#pragma unroll
    for (int g = 0; g < NG; g++) {
      if (pos[g] >= ntiles) continue;
      all_done = false;
      const gdv_uint64* a = agg + (gdv_int64)g * ntiles;
      gdv_uint64 s[K];
#pragma unroll
      for (int k = 0; k < K; k++) {
        const gdv_int64 idx = pos[g] + (gdv_int64)lane * K + k;
        s[k] = idx < ntiles ? gdv_lb_load(a + idx) : 0ull;
      }
      int lead = 0;
      bool run = true;
      gdv_uint64 a0 = 0, a1 = 0;
#pragma unroll
      for (int k = 0; k < K; k++) {
        run = run && (s[k] >> 62) == 1;
        if (run) { lead++; a0 += s[k] & GDV_LB_M31; a1 += (s[k] >> 31) & GDV_LB_M31; }
      }
      const gdv_uint64 fullmask = __ballot(lead == K);
      const int nf = fullmask == ~0ull ? 64 : __builtin_ctzll(~fullmask);
      const int part = nf < 64 ? __builtin_amdgcn_readlane(lead, nf) : 0;
      const int total_run = nf * K + part;
      if (total_run == 0) continue;
      progressed = true;
      const int consumed = lane < nf ? K : (lane == nf ? part : 0);
      gdv_uint64 t0, t1;
      gdv_uint64 e0 = gdv_wave_excl_scan_u64(lane <= nf ? a0 : 0ull, lane, &t0) + c0[g];
      gdv_uint64 e1 = gdv_wave_excl_scan_u64(lane <= nf ? a1 : 0ull, lane, &t1) + c1[g];
      gdv_uint64* p = pre + (gdv_int64)g * ntiles + pos[g] + (gdv_int64)lane * K;
#pragma unroll
      for (int k = 0; k < K; k++) {
        if (k < consumed) {
          gdv_lb_store(p + k, GDV_LB_POSTED | (gdv_sat31(e1) << 31) | gdv_sat31(e0));
          e0 += s[k] & GDV_LB_M31;
          e1 += (s[k] >> 31) & GDV_LB_M31;
        }
      }
      c0[g] += t0;
      c1[g] += t1;
      pos[g] += total_run;
    }
    if (all_done) break;
    if (progressed) {
      idle = 0;
    } else {
      // bounded by WALL CLOCK (the 100 MHz constant counter), not by an iteration count: a shared
      // or profiled device may keep workers off the chip for long stretches (round-2 advisor)
      __builtin_amdgcn_s_sleep(2);
      const gdv_uint64 now = __builtin_amdgcn_s_memrealtime();
      if (idle == 0) { idle = 1; idle_since = now; }
      else if (now - idle_since > GDV_LB_STALL_TICKS) {
        if (lane == 0) atomicOr(err, GDV_ERR_STALL);
        return;
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int g = 0; g < NG; g++) { totals[2 * g] = c0[g]; totals[2 * g + 1] = c1[g]; }
  }
}
// Worker side, ONE thread: post the tile's granule g, later wait for its exclusive prefix.
GDV_DEV void gdv_lb_post(gdv_uint64* agg, gdv_int64 ntiles, gdv_int64 tile, int g, gdv_uint64 v0, gdv_uint64 v1) {
  gdv_lb_store(agg + (gdv_int64)g * ntiles + tile, GDV_LB_POSTED | (gdv_sat31(v1) << 31) | gdv_sat31(v0));
}
GDV_DEV gdv_uint64 gdv_lb_wait(const gdv_uint64* pre, gdv_int64 ntiles, gdv_int64 tile, int g, gdv_uint32* err) {
  const gdv_uint64* p = pre + (gdv_int64)g * ntiles + tile;
  gdv_uint64 since = 0;
  for (gdv_uint32 spins = 0;; spins++) {
    const gdv_uint64 v = gdv_lb_load(p);
    if ((v >> 62) == 1) return v;
    __builtin_amdgcn_s_sleep(GDV_LB_WSLEEP);
    if ((spins & 1023u) == 1023u) {  // look at the wall clock now and then
      const gdv_uint64 now = __builtin_amdgcn_s_memrealtime();
      if (since == 0) since = now;
      else if (now - since > GDV_LB_STALL_TICKS) {
        atomicOr(err, GDV_ERR_STALL);
        return 0;
      }
    }
  }
}
// ------------------------------------------------------------------ fused filter -> project (K2F, round 4)
// ONE pass: predicate, the output base of every workgroup tile by a decoupled look-back over the
// workgroup tiles' selected-row counts, projections of the selected rows stored compacted (and the
// selection vector itself, if asked for).  A workgroup tile's granule: bits 63..62 = status (0
// nothing, 1 the tile's own count, 2 the inclusive prefix through the tile), bits 61..0 = value;
// relaxed agent-scope atomics, the granule is its own flag.  ONE wave per workgroup looks back (the
// waves' counts meet in LDS first): tools/proto/k2_proto.hip measured the per-wave window at 4.3 ms
// and this workgroup-level form at 3.56 ms on the 10^9-row filter (profiles/r02_k2_singlepass_proto.txt).
// A workgroup's tile is the TICKET it drew when it started (round 6; rounds 4-5: its block index) and it waits only for
// lower tiles — workgroups that drew earlier, hence already running: no deadlock under any dispatch order.
#define GDV_FP_AGG (1ull << 62)
#define GDV_FP_PFX (2ull << 62)
#define GDV_FP_VAL ((1ull << 62) - 1)
// Exclusive prefix of `agg` over tiles [0, tile); wave-uniform; all 64 lanes call it.  Aggregates are
// workgroup-tile counts (< 2^25): 64 of them sum in 32 bits; the prefix value is taken apart.
GDV_DEV gdv_uint64 gdv_fp_lookback(gdv_uint64* state, gdv_int64 tile, gdv_uint32 agg, int lane, gdv_uint32* err) {
  if (tile == 0) {
    if (lane == 0) gdv_lb_store(state, GDV_FP_PFX | agg);
    return 0;
  }
  if (lane == 0) gdv_lb_store(state + tile, GDV_FP_AGG | agg);
  gdv_uint64 excl = 0;
  gdv_int64 pos = tile - 1;
  gdv_uint64 since = 0;
  for (gdv_uint32 spins = 0;; spins++) {
    const gdv_int64 idx = pos - lane;
    const gdv_uint64 s = idx >= 0 ? gdv_lb_load(state + idx) : GDV_FP_PFX;  // a virtual prefix 0 before tile 0
    const gdv_uint32 st = (gdv_uint32)(s >> 62);
    const gdv_uint64 missing = __ballot(st == 0);
    const gdv_uint64 pmask = __ballot(st == 2);
    // window = lanes up to and including the nearest prefix (all 64 when there is none)
    const int fp = pmask ? __builtin_ctzll(pmask) : 63;
    const gdv_uint64 need = fp == 63 ? ~0ull : ((2ull << fp) - 1);
    if (missing & need) {
      __builtin_amdgcn_s_sleep(1);
      if ((spins & 4095u) == 4095u) {  // bounded by wall clock, like the scanner shape's hand-off
        const gdv_uint64 now = __builtin_amdgcn_s_memrealtime();
        if (since == 0) since = now;
        else if (now - since > GDV_LB_STALL_TICKS) {
          if (lane == 0) atomicOr(err, GDV_ERR_STALL);
          return 0;
        }
      }
      continue;
    }
    const gdv_uint64 v = lane <= fp ? (s & GDV_FP_VAL) : 0;
    const gdv_uint64 pv = pmask ? (((gdv_uint64)(gdv_uint32)__builtin_amdgcn_readlane((gdv_uint32)(v >> 32), fp) << 32) |
                                   (gdv_uint32)__builtin_amdgcn_readlane((gdv_uint32)v, fp)) : 0;
    excl += pv + (gdv_uint32)gdv_wave_sum((pmask && lane == fp) ? 0 : (gdv_int32)(gdv_uint32)v);
    if (pmask) break;
    pos -= 64;
  }
  if (lane == 0) gdv_lb_store(state + tile, GDV_FP_PFX | (excl + agg));
  return excl;
}
// rank of this lane among the set bits of a wave-uniform mask (bits below its own)
GDV_DEV int gdv_rank_below(gdv_uint64 m) {
  return (int)__builtin_amdgcn_mbcnt_hi((gdv_uint32)(m >> 32), __builtin_amdgcn_mbcnt_lo((gdv_uint32)m, 0));
}
// The bits of `word` at the set positions of `fm`, packed into the low cnt = popcount(fm) bits
// (wave-uniform result): the compacted validity / bool word of the selected rows of one sub-tile.
// Selected lanes send their bit to lane `rank`, the others to the lanes behind (a full permutation:
// every lane is written exactly once), one ds_permute through the LDS crossbar, no LDS memory.
GDV_DEV gdv_uint64 gdv_compact_word(gdv_uint64 word, gdv_uint64 fm, int below, int cnt, int lane) {
  const gdv_uint64 ones = cnt >= 64 ? ~0ull : ((1ull << cnt) - 1);
  if ((fm & ~word) == 0) return ones;  // wave-uniform: every selected row's bit is set
  const bool sel = (fm >> lane) & 1;
  const int dest = sel ? below : cnt + (lane - below);
  const int got = __builtin_amdgcn_ds_permute(dest << 2, (int)((word >> lane) & 1));
  return __ballot(got != 0) & ones;
}
// Output bitmap words of a wave tile, one per lane: lane j holds word (first >> 6) + j, `first` = the
// tile's first output position.  Appends the low `cnt` bits of the wave-uniform `bits` at output
// position `at` (>= first; everything a wave appends is contiguous).
GDV_DEV gdv_uint64 gdv_bits_append(gdv_uint64 acc, gdv_int64 first, gdv_int64 at, gdv_uint64 bits, int cnt, int lane) {
  if (cnt == 0) return acc;
  const gdv_int64 q = at - (first & ~63ll);   // bit position relative to the tile's first word
  const int w = (int)(q >> 6), s = (int)(q & 63);
  if (lane == w) acc |= bits << s;
  if (lane == w + 1 && s != 0) acc |= bits >> (64 - s);
  return acc;
}
// ... and stores them: a word that lies entirely inside [first, first + total) belongs to this wave
// alone (plain store); the first and the last word may be shared with the neighbouring tiles and are
// OR-ed into the pre-zeroed buffer.
GDV_DEV void gdv_bits_flush(gdv_uint64* bm, gdv_uint64 acc, gdv_int64 first, gdv_int64 total, int lane) {
  if (total <= 0) return;
  const gdv_int64 w0 = first >> 6, w1 = (first + total - 1) >> 6;
  const gdv_int64 w = w0 + lane;
  if (w > w1) return;
  const bool whole = w * 64 >= first && (w + 1) * 64 <= first + total;
  if (whole) bm[w] = acc;
  else if (acc != 0) atomicOr((unsigned long long*)(bm + w), (unsigned long long)acc);
}
// ---- the windowed shape (round 5): bitmap words accumulated at WAVE-LOCAL bit positions (lane j = bits
// [64 j, 64 j + 64) of the wave tile's own compacted stream, appended with first = 0) before the output base
// is known; once it is, the stream moves up by first & 63 bits — lane j then holds output word (first >> 6) + j —
// and leaves like gdv_bits_flush's.
GDV_DEV gdv_uint64 gdv_from_lane_below(gdv_uint64 x, int lane) {  // lane j: the value of lane j - 1 (lane 0: 0)
  const int src = ((lane + 63) & 63) << 2;
  const gdv_uint32 lo = (gdv_uint32)__builtin_amdgcn_ds_bpermute(src, (int)(gdv_uint32)x);
  const gdv_uint32 hi = (gdv_uint32)__builtin_amdgcn_ds_bpermute(src, (int)(gdv_uint32)(x >> 32));
  return lane == 0 ? 0ull : (((gdv_uint64)hi << 32) | lo);
}
GDV_DEV void gdv_bits_flush_local(gdv_uint64* bm, gdv_uint64 acc, gdv_int64 first, gdv_int64 total, int lane) {
  const int s = (int)(first & 63);
  const gdv_uint64 below = gdv_from_lane_below(acc, lane);
  const gdv_uint64 moved = s == 0 ? acc : ((acc << s) | (below >> (64 - s)));
  gdv_bits_flush(bm, moved, first, total, lane);
}
// a value that answers every index with itself: the rows beyond the window are re-read one sub-tile at a time
// under the names of the tile's register arrays (`c0[u]` in the generated body)
template <typename T>
struct gdv_one {
  T v;
  __device__ __forceinline__ T operator[](int) const { return v; }
};
#endif  // GDV_HOST_BUILD
