"""Shared comparison helpers for the parity tests."""
import numpy as np
import pyarrow as pa


def validity_np(arr):
    """bool numpy array: True where the slot is valid."""
    if arr.null_count == 0 and arr.buffers()[0] is None:
        return np.ones(len(arr), dtype=bool)
    buf = arr.buffers()[0]
    bits = np.unpackbits(np.frombuffer(buf, dtype=np.uint8), bitorder="little")
    return bits[arr.offset: arr.offset + len(arr)].astype(bool)


def values_bits_np(arr):
    """Raw bit image of every slot (uint8/16/32/64 view; bool -> 0/1)."""
    t = arr.type
    if pa.types.is_boolean(t):
        bits = np.unpackbits(np.frombuffer(arr.buffers()[1], dtype=np.uint8), bitorder="little")
        return bits[arr.offset: arr.offset + len(arr)]
    w = t.bit_width // 8
    if w == 16:  # decimal128: compare as (lo, hi) pairs packed into one structured value
        raw = np.frombuffer(arr.buffers()[1], dtype=np.dtype([("lo", np.uint64), ("hi", np.uint64)]))
        return raw[arr.offset: arr.offset + len(arr)]
    dt = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[w]
    raw = np.frombuffer(arr.buffers()[1], dtype=dt)
    return raw[arr.offset: arr.offset + len(arr)]


def assert_bit_exact(got, want, what=""):
    """Same type, same length, same validity bitmap, bit-identical values at valid slots
    (values under nulls are unspecified in Arrow and not compared)."""
    assert got.type == want.type, f"{what}: type {got.type} != {want.type}"
    assert len(got) == len(want), f"{what}: length {len(got)} != {len(want)}"
    if len(got) == 0:
        return
    gv, wv = validity_np(got), validity_np(want)
    if not np.array_equal(gv, wv):
        bad = np.flatnonzero(gv != wv)
        raise AssertionError(f"{what}: validity differs at {len(bad)} rows, first {bad[:8]}")
    if pa.types.is_string(got.type) or pa.types.is_binary(got.type):
        # var-len: the bytes of every valid row (offsets themselves may legitimately differ
        # under nulls); cast to binary so invalid UTF-8 cannot hide behind a decode error
        g, w = got.cast(pa.binary()).to_pylist(), want.cast(pa.binary()).to_pylist()
        if g != w:
            bad = [i for i, (x, y) in enumerate(zip(g, w)) if x != y]
            raise AssertionError(f"{what}: bytes differ at {len(bad)} rows, first {bad[:8]}: "
                                 f"{g[bad[0]]!r} vs {w[bad[0]]!r}")
        return
    gb, wb = values_bits_np(got)[wv], values_bits_np(want)[wv]
    if pa.types.is_floating(got.type):
        # every NaN is the same value: sign and payload of a generated NaN are not part of
        # IEEE-754 arithmetic semantics (x86 SSE yields -qNaN for inf-inf, CDNA4 +qNaN)
        ft = np.float32 if pa.types.is_float32(got.type) else np.float64
        gnan, wnan = np.isnan(gb.view(ft)), np.isnan(wb.view(ft))
        if not np.array_equal(gnan, wnan):
            bad = np.flatnonzero(gnan != wnan)
            raise AssertionError(f"{what}: NaN-ness differs at {len(bad)} valid rows, first {bad[:8]}")
        gb, wb = gb[~gnan], wb[~wnan]
    if not np.array_equal(gb, wb):
        bad = np.flatnonzero(gb != wb)
        raise AssertionError(f"{what}: values differ at {len(bad)} valid rows, first idx {bad[:8]}: "
                             f"{gb[bad[:4]]} vs {wb[bad[:4]]}")


def assert_bit_exact_where(got, want, keep, what=""):
    """assert_bit_exact on the rows of the bool numpy array `keep`; on every other row only the validity is compared (a
    row whose expected value is not defined, such as one whose exact result leaves int64, is still NULL or not NULL)."""
    assert len(got) == len(want) == len(keep), f"{what}: lengths {len(got)}, {len(want)}, {len(keep)}"
    gv, wv = validity_np(got), validity_np(want)
    if not np.array_equal(gv, wv):
        bad = np.flatnonzero(gv != wv)
        raise AssertionError(f"{what}: validity differs at {len(bad)} rows, first {bad[:8]}")
    mask = pa.array(np.asarray(keep, dtype=bool))
    assert_bit_exact(got.filter(mask), want.filter(mask), what)


def ulp_distance(g, w):
    """max distance in units of last place between two float64 numpy arrays."""
    both_nan = np.isnan(g) & np.isnan(w)
    gi = np.ascontiguousarray(g).view(np.int64)
    wi = np.ascontiguousarray(w).view(np.int64)
    gi = np.where(gi < 0, np.int64(-2**63) - gi, gi)
    wi = np.where(wi < 0, np.int64(-2**63) - wi, wi)
    d = np.abs(gi - wi)
    d[both_nan] = 0
    return int(d.max(initial=0))


def assert_within_ulp(got, want, ulps=1, what=""):
    """Floating point results of library math functions: <= `ulps` ULP at valid slots."""
    gv, wv = validity_np(got), validity_np(want)
    assert np.array_equal(gv, wv), f"{what}: validity differs"
    g = np.asarray(got.to_numpy(zero_copy_only=False), dtype=np.float64)[wv]
    w = np.asarray(want.to_numpy(zero_copy_only=False), dtype=np.float64)[wv]
    both_nan = np.isnan(g) & np.isnan(w)
    gi = g.view(np.int64)
    wi = w.view(np.int64)
    # map to a monotonic integer line
    gi = np.where(gi < 0, np.int64(-2**63) - gi, gi)
    wi = np.where(wi < 0, np.int64(-2**63) - wi, wi)
    d = np.abs(gi - wi)
    d[both_nan] = 0
    assert d.max(initial=0) <= ulps, f"{what}: max ulp distance {d.max()}"


def random_array(rng, t, n, null_fraction=0.1, special=True):
    """Random pyarrow array of fixed-width type t with edge values mixed in."""
    if pa.types.is_boolean(t):
        vals = rng.integers(0, 2, n).astype(bool)
    elif pa.types.is_floating(t):
        dt = np.float32 if pa.types.is_float32(t) else np.float64
        vals = rng.standard_normal(n).astype(dt) * dt(1000.0)
        if special and n >= 8:
            idx = rng.integers(0, n, 8)
            vals[idx] = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, np.finfo(dt).tiny / 4,
                                  np.finfo(dt).max, 1.0], dtype=dt)
    elif pa.types.is_integer(t):
        info = np.iinfo(t.to_pandas_dtype())
        small = max(info.min, -1000), min(info.max, 1000)
        vals = rng.integers(small[0], small[1], n, dtype=np.int64).astype(t.to_pandas_dtype())
        if special and n >= 4:
            idx = rng.integers(0, n, 4)
            vals[idx] = np.array([info.min, info.max, 0, 1], dtype=t.to_pandas_dtype())
    elif pa.types.is_date32(t):
        return pa.array(rng.integers(-30000, 60000, n).astype(np.int32), type=pa.int32(),
                        mask=_mask(rng, n, null_fraction)).cast(t)
    elif pa.types.is_date64(t):
        days = rng.integers(-30000, 60000, n).astype(np.int64)
        return pa.array(days * 86400000, type=pa.int64(), mask=_mask(rng, n, null_fraction)).cast(t)
    elif pa.types.is_timestamp(t):
        ms = rng.integers(-2_000_000_000_000, 4_000_000_000_000, n).astype(np.int64)
        return pa.array(ms, type=pa.int64(), mask=_mask(rng, n, null_fraction)).cast(t)
    else:
        raise NotImplementedError(str(t))
    return pa.array(vals, type=t, mask=_mask(rng, n, null_fraction))


def _mask(rng, n, null_fraction):
    if null_fraction <= 0:
        return None
    if null_fraction >= 1:
        return np.ones(n, dtype=bool)
    return rng.random(n) < null_fraction


def py_murmur3_x64_128_h1(data: bytes, seed: int) -> int:
    """Independent pure-Python MurmurHash3_x64_128, first 64 bits (signed)."""
    M = (1 << 64) - 1
    c1, c2 = 0x87c37b91114253d5, 0x4cf5ad432745937f
    rotl = lambda v, d: ((v << d) | (v >> (64 - d))) & M

    def fmix(k):
        k ^= k >> 33; k = k * 0xff51afd7ed558ccd & M; k ^= k >> 33
        k = k * 0xc4ceb9fe1a85ec53 & M; k ^= k >> 33
        return k
    h1 = h2 = seed & M
    nblocks = len(data) // 16
    for b in range(nblocks):
        k1 = int.from_bytes(data[16 * b: 16 * b + 8], "little")
        k2 = int.from_bytes(data[16 * b + 8: 16 * b + 16], "little")
        k1 = k1 * c1 & M; k1 = rotl(k1, 31); k1 = k1 * c2 & M; h1 ^= k1
        h1 = rotl(h1, 27); h1 = (h1 + h2) & M; h1 = (h1 * 5 + 0x52dce729) & M
        k2 = k2 * c2 & M; k2 = rotl(k2, 33); k2 = k2 * c1 & M; h2 ^= k2
        h2 = rotl(h2, 31); h2 = (h2 + h1) & M; h2 = (h2 * 5 + 0x38495ab5) & M
    tail = data[16 * nblocks:]
    if len(tail) > 8:
        k2 = int.from_bytes(tail[8:], "little")
        k2 = k2 * c2 & M; k2 = rotl(k2, 33); k2 = k2 * c1 & M; h2 ^= k2
    if tail:
        k1 = int.from_bytes(tail[:8], "little")
        k1 = k1 * c1 & M; k1 = rotl(k1, 31); k1 = k1 * c2 & M; h1 ^= k1
    h1 ^= len(data); h2 ^= len(data)
    h1 = (h1 + h2) & M; h2 = (h2 + h1) & M
    h1, h2 = fmix(h1), fmix(h2)
    h1 = (h1 + h2) & M
    return h1 - (1 << 64) if h1 >> 63 else h1


def py_murmur3_x86_32(data: bytes, seed: int) -> int:
    """Independent pure-Python MurmurHash3_x86_32 (signed); the seed is taken modulo 2^32."""
    M = 0xffffffff
    rotl = lambda v, d: ((v << d) | (v >> (32 - d))) & M
    h = seed & M
    nblocks = len(data) // 4
    for b in range(nblocks):
        k = int.from_bytes(data[4 * b: 4 * b + 4], "little")
        k = k * 0xcc9e2d51 & M; k = rotl(k, 15); k = k * 0x1b873593 & M
        h ^= k; h = rotl(h, 13); h = (h * 5 + 0xe6546b64) & M
    tail = data[4 * nblocks:]
    if tail:
        k = int.from_bytes(tail, "little")
        k = k * 0xcc9e2d51 & M; k = rotl(k, 15); k = k * 0x1b873593 & M
        h ^= k
    h ^= len(data)
    h ^= h >> 16; h = h * 0x85ebca6b & M; h ^= h >> 13; h = h * 0xc2b2ae35 & M; h ^= h >> 16
    return h - (1 << 32) if h >> 31 else h


# ---- full-range operands (tests/test_full_range_numeric*.py)----------------------------------------------------------

def _np_dtype(t):
    return np.dtype(t.to_pandas_dtype())


def edge_values(t):
    """The values of numeric type t at which magnitude-dependent code goes wrong, most important first, deduplicated.

    Integers of width w (a Python list, clipped to the type): min, min+1, max-1, max, -1, 0, 1, 2; +-2^(w/2) and its two
    neighbours; for unsigned types the values on either side of 2^(w-1); where they fit, the integers that a conversion
    to float must round (2^24 + 1, 2^24 + 3, 2^53 + 1, 2^53 + 3, and 2^54 + 2^30 + 1, which rounds the other way when
    it is rounded to float64 first and to float32 after); then 2^k and 2^k - 1 for every k < w.
    Floats (a numpy array): +-0, the smallest and largest denormal, the smallest normal, 1, 1 +- 1 ulp, 0.5 - 1 ulp, max,
    inf, one NaN, then 2^24, 2^24 + 1, 2^53, 2^53 + 1 (each as the type rounds it), 2147483647.5, 2^31, 2^63 and its
    lower neighbour, all with both signs."""
    if pa.types.is_integer(t):
        w = t.bit_width
        signed = pa.types.is_signed_integer(t)
        lo, hi = (-(1 << (w - 1)), (1 << (w - 1)) - 1) if signed else (0, (1 << w) - 1)
        h = 1 << (w // 2)
        vals = [lo, lo + 1, hi - 1, hi, -1, 0, 1, 2, h - 1, h, h + 1, -h + 1, -h, -h - 1]
        if not signed:
            vals += [(1 << (w - 1)) - 1, 1 << (w - 1), (1 << (w - 1)) + 1]
        round_me = [(1 << 24) + 1, (1 << 24) + 3, (1 << 53) + 1, (1 << 53) + 3, (1 << 54) + (1 << 30) + 1]
        vals += [s * v for v in round_me if v <= hi for s in (1, -1)]
        for k in range(w):
            vals += [1 << k, (1 << k) - 1]
        out = []
        for v in vals:
            v = min(max(v, lo), hi)
            if v not in out:
                out.append(v)
        return out
    dt = np.float32 if pa.types.is_float32(t) else np.float64
    fi = np.finfo(dt)
    one = dt(1.0)
    with np.errstate(over="ignore"):
        pos = [dt(0.0), fi.smallest_subnormal, np.nextafter(fi.tiny, dt(0.0)), fi.tiny, one, np.nextafter(one, dt(2.0)),
               np.nextafter(one, dt(0.0)), np.nextafter(dt(0.5), dt(0.0)), fi.max, dt(np.inf),
               dt(2.0 ** 24), dt(2.0 ** 24 + 1), dt(2.0 ** 53), dt(np.float64(2 ** 53 + 2) if dt is np.float64 else 2.0 ** 53),
               dt(2147483647.5), dt(2.0 ** 31), dt(2.0 ** 63), np.nextafter(dt(2.0 ** 63), dt(0.0))]
    out, seen = [], set()
    for i, v in enumerate(pos):
        for s in (v, -v):
            bits = np.array([s], dtype=dt).tobytes()
            if bits not in seen:
                seen.add(bits)
                out.append(s)
        if i == 9:
            out.append(dt(np.nan))
    return np.array(out, dtype=dt)


def full_range_values(rng, t, n):
    """n values of numeric type t (numpy) in which every magnitude is equally likely: integers are uniformly random bit
    images shifted right by a random 0..w-1 (arithmetically for signed types: the sign is kept); floats are uniformly
    random bit images (exponent-uniform, denormals included) with NaN images thinned to at most 1 % of the rows."""
    dt = _np_dtype(t)
    w = t.bit_width
    raw = rng.integers(0, 1 << 64, n, dtype=np.uint64) >> np.uint64(64 - w)
    if pa.types.is_integer(t):
        vals = raw.astype({8: np.uint8, 16: np.uint16, 32: np.uint32, 64: np.uint64}[w]).view(dt)
        return vals >> rng.integers(0, w, n).astype(dt)
    vals = raw.astype(np.uint32 if w == 32 else np.uint64).view(dt)
    surplus = np.flatnonzero(np.isnan(vals))[n // 100:]
    bits = vals.view(np.uint32 if w == 32 else np.uint64)
    bits[surplus] &= ~(bits.dtype.type(1) << bits.dtype.type(w - 2))     # the exponent's top bit cleared: finite
    return vals


def full_range_array(rng, t, n, null_fraction=0.1):
    """full_range_values as a pyarrow array with a random validity bitmap."""
    return pa.array(full_range_values(rng, t, n), type=t, mask=_mask(rng, n, null_fraction))


def nonzero_divisors(vals):
    """A divisor column: 0 becomes 1 and +-0.0 becomes +-1.0 (that x / 0 raises is pinned elsewhere); nothing else changes."""
    vals = vals.copy()
    if vals.dtype.kind == "f":
        zero = vals == 0
        vals[zero] = np.copysign(vals.dtype.type(1), vals[zero])
    else:
        vals[vals == 0] = 1
    return vals


def edge_pair_values(rng, t, n=4099, cross=32):
    """Two operand columns (numpy) of n rows: the first k * k rows are the cross product E x E of the first k = min(cross,
    len(E)) edge values of t, random full-range rows follow, and every third of those carries a value of the whole edge
    list in its first, its second or both columns (lists longer than `cross` are covered that way).  4099 rows hold the
    cross product of 32 values and about 3000 random rows."""
    dt = _np_dtype(t)
    edges = np.array(edge_values(t), dtype=dt)
    k = min(cross, len(edges))
    assert k * k < n
    a, b = full_range_values(rng, t, n), full_range_values(rng, t, n)
    a[:k * k] = np.repeat(edges[:k], k)
    b[:k * k] = np.tile(edges[:k], k)
    rows = np.arange(k * k, n, 3)
    which = rng.integers(0, 3, len(rows))
    ea, eb = edges[rng.integers(0, len(edges), len(rows))], edges[rng.integers(0, len(edges), len(rows))]
    a[rows[which != 1]] = ea[which != 1]
    b[rows[which != 0]] = eb[which != 0]
    return a, b
