"""An independent reference for the numeric core — arithmetic, compares, casts, exact and libm-backed math, hashes —
on full-range operands.  It shares no code with the oracle (oracle/gdv_oracle.c) or with the device library
(gdv_device_lib.hpp): integers are Python `int`s reduced modulo 2^w, float64 is numpy's IEEE arithmetic, float32 is
float64 rounded once, integer -> float conversion is written out on Python integers, the libm-backed functions are
computed in x87 extended precision and rounded once, hashes are a pure-Python MurmurHash3 over the 8 bytes of float(v).

The second half holds the cases that tests/test_full_range_numeric_cpu.py (oracle, host build of the device library)
and tests/test_full_range_numeric.py (GPU: specialised kernels and the tier-0 interpreter) share: one schema with
operand columns for every numeric type, the families of expressions over it, and their expected results."""
import functools
import struct

import numpy as np
import pyarrow as pa

from helpers import edge_pair_values, full_range_values, nonzero_divisors, py_murmur3_x64_128_h1, validity_np

# The host must compute with denormals (a flush-to-zero mode would make this module agree with a flushing device).
assert np.float64(5e-324) * np.float64(1) != 0 and np.float32(1e-45) * np.float32(1) != 0, "the host flushes denormals"
# np.longdouble must be wider than float64 (x87: 64-bit significand), or "rounded once" below would mean nothing.
assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is not an extended format on this host"

TYPES = {"i8": pa.int8(), "i16": pa.int16(), "i32": pa.int32(), "i64": pa.int64(), "u8": pa.uint8(), "u16": pa.uint16(),
         "u32": pa.uint32(), "u64": pa.uint64(), "f32": pa.float32(), "f64": pa.float64(), "bool": pa.bool_()}
NUMERIC = ["i8", "i16", "i32", "i64", "u8", "u16", "u32", "u64", "f32", "f64"]
INTS = NUMERIC[:8]


def _is_int(tn):
    return tn[0] in "iu"


def wrap(v, tn):
    """Python integer v reduced modulo 2^w and re-read as signed where the type is signed."""
    w = int(tn[1:])
    v &= (1 << w) - 1
    return v - (1 << w) if tn[0] == "i" and v >> (w - 1) else v


def _trunc_div(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _trunc_mod(a, b):
    r = abs(a) % abs(b)
    return -r if a < 0 else r


def int_to_float(v, mant_bits, max_exp):
    """Python integer -> the nearest value with a `mant_bits`-bit significand, ties to even, as a Python float (exact:
    mant_bits <= 53); magnitudes of 2^max_exp and above cannot occur for 64-bit inputs."""
    m, s = abs(v), (-1.0 if v < 0 else 1.0)
    extra = m.bit_length() - mant_bits
    if extra > 0:
        low, half = m & ((1 << extra) - 1), 1 << (extra - 1)
        m >>= extra
        if low > half or (low == half and (m & 1)):       # above the tie, or the tie with an odd significand
            m += 1
        m <<= extra
    assert m < (1 << max_exp)
    return s * float(m)                                  # at most mant_bits significant bits: the conversion is exact


def _murmur3_32(data, seed):
    """MurmurHash3_x86_32 of a whole number of 4-byte blocks (pure Python), as a signed 32-bit integer."""
    M = 0xffffffff
    h = seed & M
    for i in range(0, len(data), 4):
        k = int.from_bytes(data[i:i + 4], "little") * 0xcc9e2d51 & M
        k = ((k << 15) | (k >> 17)) & M
        h ^= k * 0x1b873593 & M
        h = ((h << 13) | (h >> 19)) & M
        h = (h * 5 + 0xe6546b64) & M
    h ^= len(data)
    h ^= h >> 16
    h = h * 0x85ebca6b & M
    h ^= h >> 13
    h = h * 0xc2b2ae35 & M
    h ^= h >> 16
    return h - (1 << 32) if h >> 31 else h


def _double_bytes(v):
    return struct.pack("<d", float(v))                    # Python's int -> float conversion rounds to nearest even


_CMP = {"equal": lambda a, b: a == b, "not_equal": lambda a, b: a != b, "less_than": lambda a, b: a < b,
        "less_than_or_equal_to": lambda a, b: a <= b, "greater_than": lambda a, b: a > b,
        "greater_than_or_equal_to": lambda a, b: a >= b}
_LIBM = {"cbrt": np.cbrt, "exp": np.exp, "log": np.log, "log10": np.log10}


def _values(arr, fill):
    """The valid values of a pyarrow array as numpy, `fill` under nulls."""
    tn = [k for k, t in TYPES.items() if t == arr.type][0]
    v = np.asarray(arr.fill_null(fill) if arr.null_count else arr)
    return tn, v


def expected(fn, args, ret):
    """The result of registry function `fn` over pyarrow arrays `args`, as a pyarrow array of type TYPES[ret]."""
    n = len(args[0])
    valid = [validity_np(a) for a in args]
    cols = [_values(a, 1) for a in args]
    tn = cols[0][0]
    vals = [c[1] for c in cols]
    out_valid = np.logical_and.reduce(valid)
    rdt = np.dtype(TYPES[ret].to_pandas_dtype())

    if fn in ("hash", "hash32", "hash64"):
        wide = fn == "hash64"
        v0 = vals[0].tolist()
        if len(args) == 2:         # the seed chain: a NULL seed is 0, a NULL value hashes to the seed; int64 seeds are narrowed
            seeds = [s if ok else 0 for s, ok in zip(vals[1].tolist(), valid[1])]
        else:
            seeds = [0] * n
        res = [((py_murmur3_x64_128_h1(_double_bytes(v), wrap(s, "i32")) if wide else _murmur3_32(_double_bytes(v), s)) if ok else s)
               for v, s, ok in zip(v0, seeds, valid[0])]
        return pa.array(res, TYPES[ret])
    if fn in ("is_distinct_from", "is_not_distinct_from"):
        with np.errstate(invalid="ignore"):
            differ = np.array([a != b for a, b in zip(vals[0].tolist(), vals[1].tolist())]) if _is_int(tn) else vals[0] != vals[1]
        d = np.where(valid[0] != valid[1], True, np.where(valid[0], differ, False))
        return pa.array(d if fn == "is_distinct_from" else ~d, pa.bool_())

    if _is_int(tn) and fn not in ("castFLOAT4", "castFLOAT8"):
        a = vals[0].tolist()
        b = vals[1].tolist() if len(vals) > 1 else None
        if fn in ("add", "subtract", "multiply"):
            op = {"add": int.__add__, "subtract": int.__sub__, "multiply": int.__mul__}[fn]
            res = [wrap(op(x, y), ret) for x, y in zip(a, b)]
        elif fn == "divide":                               # toward zero; MIN / -1 wraps to MIN
            res = [wrap(_trunc_div(x, y), ret) for x, y in zip(a, b)]
        elif fn in ("mod", "modulo"):                      # sign of the dividend; x mod 0 = x, narrowed as C's cast does
            res = [wrap(x if y == 0 else _trunc_mod(x, y), ret) for x, y in zip(a, b)]
        elif fn in _CMP:
            res = [_CMP[fn](x, y) for x, y in zip(a, b)]
        elif fn in ("greatest", "least"):
            res = [(max if fn == "greatest" else min)(x, y) for x, y in zip(a, b)]
        elif fn in ("negative", "abs"):
            res = [wrap(-x if fn == "negative" else abs(x), ret) for x in a]
        elif fn in ("castINT", "castBIGINT"):
            res = [wrap(x, ret) for x in a]
        elif fn == "bitwise_not":
            res = [wrap(~x, ret) for x in a]
        else:
            op = {"bitwise_and": int.__and__, "bitwise_or": int.__or__, "bitwise_xor": int.__xor__}[fn]
            res = [wrap(op(x, y), ret) for x, y in zip(a, b)]
        return pa.array(np.array(res, dtype=rdt), TYPES[ret], mask=~out_valid)

    with np.errstate(all="ignore"):
        x = vals[0]
        y = vals[1] if len(vals) > 1 else None
        if fn in ("castFLOAT4", "castFLOAT8") and _is_int(tn):
            mant, mexp = (24, 128) if fn == "castFLOAT4" else (53, 1024)
            res = np.array([int_to_float(v, mant, mexp) for v in x.tolist()], dtype=np.float64).astype(rdt)   # exact
            assert np.array_equal(res, x.astype(rdt)), "numpy's integer -> float conversion disagrees with round-to-nearest-even"
        elif fn in ("castFLOAT4", "castFLOAT8"):
            res = x.astype(rdt)
        elif fn in ("castINT", "castBIGINT"):              # trunc(x +- 0.5) in float64, then saturation; NaN -> 0
            x = x.astype(np.float64)
            r = np.trunc(x + np.where(x >= 0, 0.5, -0.5))
            lo, hi = (-2 ** 31, 2 ** 31 - 1) if fn == "castINT" else (-2 ** 63, 2 ** 63 - 1)
            res = np.array([0 if v != v else hi if v >= hi else lo if v <= lo else int(v) for v in r.tolist()], dtype=rdt)
        elif fn in ("add", "subtract", "multiply", "divide"):
            op = {"add": np.add, "subtract": np.subtract, "multiply": np.multiply, "divide": np.divide}[fn]
            res = op(x.astype(np.float64), y.astype(np.float64)).astype(rdt)      # float32: float64, rounded once
        elif fn in ("mod", "modulo"):
            res = np.fmod(x, y)                            # fmod is exact in every format
        elif fn in _CMP:
            res = _CMP[fn](x, y)
        elif fn == "greatest":
            res = np.where(x > y, x, y)                    # the library's stated rule: a > b ? a : b
        elif fn == "least":
            res = np.where(x < y, x, y)
        elif fn == "negative":
            res = -x
        elif fn == "abs":
            res = np.abs(x)
        elif fn == "round":
            res = np.trunc(x + np.where(x >= 0, 0.5, -0.5))
        elif fn in ("floor", "ceil", "truncate"):
            res = {"floor": np.floor, "ceil": np.ceil, "truncate": np.trunc}[fn](x)
        elif fn == "sqrt":
            res = np.sqrt(x)                               # correctly rounded in IEEE arithmetic
        elif fn in _LIBM:
            res = _LIBM[fn](x.astype(np.longdouble)).astype(np.float64)
        elif fn in ("power", "pow"):
            res = np.power(x.astype(np.longdouble), y.astype(np.longdouble)).astype(np.float64)
        else:
            raise NotImplementedError(fn)
    if ret == "bool":
        return pa.array(np.asarray(res, dtype=bool), pa.bool_(), mask=~out_valid)
    return pa.array(np.asarray(res, dtype=rdt), TYPES[ret], mask=~out_valid)


def ulp_distances(g, w):
    """Per-row distance in units of the last place between two float64 numpy arrays (0 where both are NaN)."""
    gi, wi = np.ascontiguousarray(g).view(np.int64), np.ascontiguousarray(w).view(np.int64)
    gi = np.where(gi < 0, np.int64(-2 ** 63) - gi, gi).astype(object)
    wi = np.where(wi < 0, np.int64(-2 ** 63) - wi, wi).astype(object)
    d = np.abs(gi - wi)
    d[np.isnan(g) & np.isnan(w)] = 0
    return d


def max_ulp_on_ordinary_rows(got, want):
    """Largest ulp distance over the valid rows whose correctly rounded result is neither 0, inf nor NaN."""
    ok = validity_np(want)
    g, w = np.asarray(got.fill_null(0.0))[ok], np.asarray(want.fill_null(0.0))[ok]
    ordinary = np.isfinite(w) & (w != 0)
    return int(max(ulp_distances(g[ordinary], w[ordinary]), default=0))


def assert_class_and_ulp(got, want, ulps, what=""):
    """A libm-backed result against the correctly rounded one: the same validity; rows whose correct result is 0, inf or
    NaN agree exactly in class and sign; every other valid row lies within `ulps` units of the last place."""
    assert got.type == want.type and len(got) == len(want), what
    ok = validity_np(want)
    assert np.array_equal(validity_np(got), ok), f"{what}: validity differs"
    g, w = np.asarray(got.fill_null(0.0))[ok], np.asarray(want.fill_null(0.0))[ok]
    special = ~(np.isfinite(w) & (w != 0))
    gs, ws = g[special], w[special]
    same = (np.isnan(gs) & np.isnan(ws)) | (gs.view(np.uint64) == ws.view(np.uint64))
    assert same.all(), f"{what}: {int((~same).sum())} rows differ in class or sign, first {gs[~same][:4]} for {ws[~same][:4]}"
    d = ulp_distances(g[~special], w[~special])
    worst = int(max(d, default=0))
    assert worst <= ulps, f"{what}: {worst} ulp from the correctly rounded value (bound {ulps}) at {g[~special][np.argmax(d)]!r}"


# ---- the shared cases --------------------------------------------------------------------------------------------------
ROWS = 4099
MATH_COLS = ["m_exp", "m_pos", "m_any", "m_px1", "m_py1", "m_px2", "m_py2"]
COLUMNS = [(tn + s, tn) for tn in NUMERIC for s in ("_a", "_b", "_d")] + [(c, "f64") for c in MATH_COLS]
SCHEMA = pa.schema([(name, TYPES[tn]) for name, tn in COLUMNS])
FAMILIES = ["arith", "divmod", "casts", "minmax_bitwise", "exact", "libm", "hash"]


def _math_values(rng, n):
    pos = np.abs(full_range_values(rng, pa.float64(), n))
    pos[np.isnan(pos)] = 1.0
    pos[:8] = [0.0, 5e-324, 2.2250738585072009e-308, 2.2250738585072014e-308, 1.0, np.nextafter(1.0, 2.0), 1.7976931348623157e308, np.inf]
    anyx = full_range_values(rng, pa.float64(), n)
    anyx[:12] = [0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, -1.0, 8.0, -27.0, 1.7976931348623157e308, np.inf, -np.inf, np.nan]
    ex = rng.uniform(-750.0, 710.0, n)
    ex[:8] = [0.0, -0.0, 709.782712893384, 709.782712893385, -745.1332191019411, -745.1332191019412, -708.3964185322641, 1.0]
    px1 = np.exp2(rng.uniform(np.log2(1e-300), np.log2(1e300), n))
    py1 = rng.uniform(-3.0, 3.0, n)
    px2 = rng.uniform(0.5, 2.0, n)
    py2 = rng.uniform(-1000.0, 1000.0, n)
    return {"m_exp": ex, "m_pos": pos, "m_any": anyx, "m_px1": px1, "m_py1": py1, "m_px2": px2, "m_py2": py2}


@functools.lru_cache(maxsize=None)
def batch(nulls):
    """The 4099-row batch over SCHEMA: per type the edge cross product and full-range rows in _a / _b, _d = _b with its
    zeros replaced (the divisor column); `nulls` = the fraction of null rows in every column."""
    rng = np.random.default_rng(20251 + int(nulls * 100))
    cols = {}
    for tn in NUMERIC:
        a, b = edge_pair_values(rng, TYPES[tn], ROWS)
        cols[tn + "_a"], cols[tn + "_b"], cols[tn + "_d"] = a, b, nonzero_divisors(b)
    cols.update(_math_values(rng, ROWS))
    arrays = [pa.array(cols[name], TYPES[tn], mask=(rng.random(ROWS) < nulls) if nulls > 0 else None) for name, tn in COLUMNS]
    return pa.RecordBatch.from_arrays(arrays, schema=SCHEMA)


def _spec(fn, args, ret, tier0=True, ulps=None, host=None, oracle_ulps=None):
    """An expression: `args` are column names or, for a nested call, specs themselves."""
    label = "%s(%s)" % (fn, ",".join(a if isinstance(a, str) else a["label"] for a in args))
    return {"label": label, "fn": fn, "args": list(args), "ret": ret, "tier0": tier0, "ulps": ulps, "host": host, "oracle_ulps": oracle_ulps}


# What exceeds the project's bound of 1 ulp on the wider domains, measured against the x87 reference on an MI355X
# (profiles/full_range_numeric.txt, PARITY.md's math row): function and sub-domain -> the measured maximum.  Empty: none.
MEASURED_ULPS = {}
# The same for the oracle (the host's libm), measured on the same rows: glibc's cbrt reaches 3 ulp, everything else 1.
# Decided, not fixed (PARITY.md's math row): the oracle calls the C library, as the reference's CPU path does.
ORACLE_MEASURED_ULPS = {("cbrt", "m_any"): 3}


@functools.lru_cache(maxsize=None)
def family_specs(family):
    """The expressions of a family: label, registry name, argument columns, result type, whether the tier-0 interpreter
    takes it, the ulp bound (None: bit for bit) and the host-build entry point that computes it (None: no such entry)."""
    s = []
    if family == "arith":
        for k, tn in enumerate(NUMERIC):
            group = "int" if _is_int(tn) else "float"
            for op, fn in enumerate(("add", "subtract", "multiply")):
                s.append(_spec(fn, [tn + "_a", tn + "_b"], tn, host=(group + "_binary", k if group == "int" else k - 8, op)))
            for op, fn in enumerate(_CMP):
                s.append(_spec(fn, [tn + "_a", tn + "_b"], "bool", host=("compare", k, op)))
            s.append(_spec("is_distinct_from", [tn + "_a", tn + "_b"], "bool"))
        # a wrapped sum, difference or product read by a compare: the interpreter keeps every value in a 64-bit slot, and a
        # result that is not brought back to its type's width shows only to a consumer (the store truncates by itself)
        for tn in INTS:
            for fn in ("add", "subtract", "multiply"):
                s.append(_spec("less_than", [_spec(fn, [tn + "_a", tn + "_b"], tn), tn + "_b"], "bool"))
            s.append(_spec("equal", [_spec("multiply", [tn + "_a", tn + "_b"], tn), tn + "_a"], "bool"))
    elif family == "divmod":
        for k, tn in enumerate(NUMERIC):
            group = "int" if _is_int(tn) else "float"
            s.append(_spec("divide", [tn + "_a", tn + "_d"], tn, tier0=False, host=(group + "_binary", k if group == "int" else k - 8, 3)))
        for name in ("mod", "modulo"):
            for k, (x, y, r) in enumerate((("i64_a", "i32_b", "i32"), ("i64_a", "i64_b", "i64"), ("i32_a", "i32_b", "i32"))):
                s.append(_spec(name, [x, y], r, host=("mod", k, 0)))
            s.append(_spec(name, ["f64_a", "f64_d"], "f64", tier0=False))
    elif family == "casts":
        for op, (fn, x, r) in enumerate((("castBIGINT", "i32", "i64"), ("castINT", "i64", "i32"), ("castFLOAT4", "i32", "f32"),
                                         ("castFLOAT4", "i64", "f32"), ("castFLOAT4", "f64", "f32"), ("castFLOAT8", "i32", "f64"),
                                         ("castFLOAT8", "i64", "f64"), ("castFLOAT8", "f32", "f64"), ("castBIGINT", "f32", "i64"),
                                         ("castBIGINT", "f64", "i64"), ("castINT", "f32", "i32"), ("castINT", "f64", "i32"))):
            s += [_spec(fn, [x + "_a"], r, host=("cast", op, 0)), _spec(fn, [x + "_b"], r, host=("cast", op, 0))]
    elif family == "minmax_bitwise":
        for k, tn in enumerate(("i32", "i64", "f32", "f64")):
            s += [_spec("greatest", [tn + "_a", tn + "_b"], tn, host=("minmax", k, 0)), _spec("least", [tn + "_a", tn + "_b"], tn, host=("minmax", k, 1)),
                  _spec("negative", [tn + "_a"], tn, host=("unary", k, 0)), _spec("abs", [tn + "_a"], tn, host=("unary", k, 1))]
        for tn in ("i32", "i64", "u32", "u64"):
            s += [_spec(fn, [tn + "_a", tn + "_b"], tn) for fn in ("bitwise_and", "bitwise_or", "bitwise_xor")] + [_spec("bitwise_not", [tn + "_a"], tn)]
    elif family == "exact":
        for c in ("f64_a", "f64_b", "m_any"):
            s += [_spec(fn, [c], "f64") for fn in ("round", "floor", "ceil", "truncate", "sqrt")]
    elif family == "libm":
        def libm(fn, cols, dom):
            return _spec(fn, cols, "f64", ulps=MEASURED_ULPS.get((fn, dom), 1), oracle_ulps=ORACLE_MEASURED_ULPS.get((fn, dom), 1))
        s += [libm("exp", ["m_exp"], "m_exp"), libm("log", ["m_pos"], "m_pos"), libm("log10", ["m_pos"], "m_pos"), libm("cbrt", ["m_any"], "m_any")]
        for fn in ("power", "pow"):           # (the two tables know both names as "power")
            s += [dict(libm("power", ["m_px1", "m_py1"], "wide base"), fn=fn, label=fn + "(m_px1,m_py1)"),
                  dict(libm("power", ["m_px2", "m_py2"], "large exponent"), fn=fn, label=fn + "(m_px2,m_py2)")]
    elif family == "hash":
        for k, tn in ((2, "i32"), (3, "i64"), (6, "u32"), (7, "u64"), (8, "f32"), (9, "f64")):
            s += [_spec(fn, [tn + c], r, tier0=False, host=("hash", k, w)) for fn, r, w in (("hash32", "i32", 0), ("hash64", "i64", 1), ("hash", "i32", 0))
                  for c in ("_a", "_b")]
    else:
        raise KeyError(family)
    return s


HASH_CHAINS = [_spec("hash64", ["f64_a", "i64_b"], "i64", tier0=False), _spec("hash32", ["i64_a", "i32_b"], "i32", tier0=False)]


@functools.lru_cache(maxsize=None)
def expected_columns(family, nulls):
    """The reference's result for every expression of a family over batch(nulls): computed once, shared, never changed."""
    b = batch(nulls)
    return [expected_of(sp, b) for sp in family_specs(family)]


def expected_of(sp, b):
    """The reference's result of one spec over a batch (nested calls evaluated first)."""
    return expected(sp["fn"], [b.column(a) if isinstance(a, str) else expected_of(a, b) for a in sp["args"]], sp["ret"])


def build_expressions(gandiva, specs):
    """gandiva expressions for a list of specs, over SCHEMA."""
    b = gandiva.TreeExprBuilder()
    out = []

    def node_of(sp):
        args = [b.make_field(SCHEMA.field(a)) if isinstance(a, str) else node_of(a) for a in sp["args"]]
        return b.make_function(sp["fn"], args, TYPES[sp["ret"]])
    for i, sp in enumerate(specs):
        out.append(b.make_expression(node_of(sp), pa.field("r%d" % i, TYPES[sp["ret"]])))
    return out
