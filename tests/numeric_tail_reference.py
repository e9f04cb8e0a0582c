"""An independent reference for the numeric tail — trigonometry and angles, sign, pmod, round / truncate to a scale,
shifts, gcd / lcm — on full-range operands.  It shares no code with the device library (gdv_device_lib.hpp):

  * sin cos tan asin acos atan sinh cosh tanh atan2: mpmath at 250 bits on the argument converted to double, rounded ONCE
    to double (through an exact fraction, so denormal results are rounded once too); mpmath reduces huge arguments exactly;
  * cot: the restated formula tan(pi/2 - x) — the subtraction in numpy double from the double nearest pi/2, then mpmath.tan;
  * degrees / radians: the numpy double multiplication by the double 180/pi, pi/180;
  * sign, pmod, integer round / truncate to a scale, shifts, gcd / lcm: Python integers, `%`, math.gcd and wrap() modulo 2^w;
  * float round to a scale: trunc(x * m + (x >= 0 ? 0.5 : -0.5)) / m in numpy float64 with m = float("1e%d" % s).

The second half holds the cases that tests/test_numeric_tail_cpu.py (host build of the device library) and
tests/test_numeric_tail.py (GPU: specialised kernels and the tier-0 interpreter) share, in the pattern of
tests/numeric_reference.py: one 4099-row schema, families of expressions over it and their expected results."""
import functools
import math
from fractions import Fraction

import mpmath
import numpy as np
import pyarrow as pa

from helpers import edge_pair_values, edge_values, full_range_values, validity_np
from numeric_reference import assert_class_and_ulp, max_ulp_on_ordinary_rows, ulp_distances, wrap  # noqa: F401 (the child reads them here)

assert np.float64(5e-324) * np.float64(1) != 0, "the host flushes denormals"

TYPES = {"i32": pa.int32(), "i64": pa.int64(), "f32": pa.float32(), "f64": pa.float64(), "bool": pa.bool_()}
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
PI = math.pi                      # the double nearest pi
HALF_PI = math.pi / 2             # halving is exact: the double nearest pi/2
DEG = 180.0 / math.pi             # ONE double constant each, as the issue states them
RAD = math.pi / 180.0
MP = mpmath.mp.clone()
MP.prec = 250

TRIG = ("sin", "cos", "tan", "asin", "acos", "atan", "sinh", "cosh", "tanh", "cot")
ANGLES = ("degrees", "radians")


# ---- rounding an mpmath value once to double ----------------------------------------------------------------------------
def _once(m):
    """An mpf rounded once to the nearest double, ties to even, denormals included; overflow gives the infinity."""
    if MP.isnan(m):
        return math.nan
    if MP.isinf(m):
        return math.inf if m > 0 else -math.inf
    sign, man, exp, bc = m._mpf_
    if man == 0:
        return 0.0
    top = int(exp) + int(bc)       # the value lies in [2^(top - 1), 2^top)
    if top > 1024:                 # 2^1024 and above (sinh of a huge argument: no fraction is built from such an exponent)
        r = math.inf
    elif top < -1080:              # below half the smallest denormal
        r = 0.0
    else:
        try:
            r = float(Fraction(int(man)) * (Fraction(2) ** int(exp)))     # int / int true division: correctly rounded
        except OverflowError:      # rounds up to 2^1024
            r = math.inf
    return -r if sign else r


def _signed(fn, x):
    """fn on |x| with x's sign put back: for the odd functions, so that a result that rounds to 0 keeps its sign."""
    r = _once(fn(MP.mpf(abs(x))))
    return -r if math.copysign(1.0, x) < 0 else r


def libm_one(fn, x):
    """The correctly rounded double of fn at the double x."""
    if x != x:
        return math.nan
    if fn == "cot":
        return libm_one("tan", float(np.float64(HALF_PI) - np.float64(x)))
    if fn in ("sin", "cos", "tan"):
        if math.isinf(x):
            return math.nan
        if fn == "cos":
            return _once(MP.cos(MP.mpf(x)))
        return _signed(MP.sin if fn == "sin" else MP.tan, x)
    if fn in ("asin", "acos"):
        if abs(x) > 1:
            return math.nan
        return _signed(MP.asin, x) if fn == "asin" else _once(MP.acos(MP.mpf(x)))
    if fn == "atan":
        return math.copysign(_once(MP.pi / 2), x) if math.isinf(x) else _signed(MP.atan, x)
    if fn == "sinh":               # (from 711 on the value is above DBL_MAX: sinh(710.4758600739439) is the last finite one)
        return math.copysign(math.inf, x) if abs(x) >= 711 else _signed(MP.sinh, x)
    if fn == "cosh":
        return math.inf if abs(x) >= 711 else _once(MP.cosh(MP.mpf(x)))
    if fn == "tanh":               # (1 - tanh(20) = 8.5e-18, below half an ulp of 1)
        return math.copysign(1.0, x) if abs(x) >= 20 else _signed(MP.tanh, x)
    raise KeyError(fn)


def atan2_one(y, x):
    """C99's atan2 with its special cases written out (mpmath has no signed zero), correctly rounded elsewhere."""
    if y != y or x != x:
        return math.nan
    sy = math.copysign(1.0, y)
    x_neg = math.copysign(1.0, x) < 0
    if y == 0:
        return sy * (_once(+MP.pi) if x_neg else 0.0)
    if x == 0:
        return sy * _once(MP.pi / 2)
    if math.isinf(y):
        if math.isinf(x):
            return sy * _once(3 * MP.pi / 4 if x_neg else MP.pi / 4)
        return sy * _once(MP.pi / 2)
    if math.isinf(x):
        return sy * (_once(+MP.pi) if x_neg else 0.0)
    return sy * _once(MP.atan2(MP.mpf(abs(y)), MP.mpf(x)))


# ---- the exact families -------------------------------------------------------------------------------------------------
def sign_int(a):
    return (a > 0) - (a < 0)


def sign_float(x):
    """numpy array in, same dtype out: -1, 0, 1; +-0 -> +0.0; NaN stays NaN"""
    one = x.dtype.type(1)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), x, np.where(x > 0, one, np.where(x < 0, -one, x.dtype.type(0))))


def pmod(a, n, tn):
    return wrap(a if n == 0 else a % n, tn)                 # Python's % is the floored modulus


def int_to_scale(a, s, tn, half):
    if s >= 0:
        return a
    if -s > (9 if tn == "i32" else 18):
        return 0
    p = 10 ** -s
    mag = abs(a)
    q = mag // p * p
    if half and 2 * (mag - q) >= p:
        q += p
    return wrap(-q if a < 0 else q, tn)


def shift(fn, a, n, tn):
    w = int(tn[1:])
    c = n & (w - 1)
    if fn == "shift_left":
        return wrap(a << c, tn)
    if fn == "shift_right":
        return a >> c                                       # Python's >> is arithmetic
    return wrap((a & ((1 << w) - 1)) >> c, tn)


def gcd(a, b):
    return wrap(math.gcd(abs(a), abs(b)), "i64")


def lcm(a, b):
    if a == 0 or b == 0:
        return 0
    return wrap(abs(a) // math.gcd(abs(a), abs(b)) * abs(b), "i64")


def float_to_scale(x, s):
    """x: numpy float64 array, s: Python ints -> numpy float64, the formula and the decided cases of the issue."""
    out = np.empty(len(x), dtype=np.float64)
    with np.errstate(all="ignore"):
        for i, (v, k) in enumerate(zip(x, s)):
            if not np.isfinite(v) or k > 308:
                out[i] = v
            elif k < -308:
                out[i] = np.copysign(np.float64(0.0), v)
            else:
                m = np.float64(float("1e%d" % k))
                vm = v * m
                out[i] = v if not np.isfinite(vm) else np.trunc(vm + (np.float64(0.5) if v >= 0 else np.float64(-0.5))) / m
    return out


# ---- evaluation of a registry call over pyarrow arrays ------------------------------------------------------------------------
def _tn(arr):
    return [k for k, t in TYPES.items() if t == arr.type][0]


def _np(arr):
    return np.asarray(arr.fill_null(1) if arr.null_count else arr)


def _as_double(arr):
    """The argument conversion of the trigonometric functions: to double, once (int64: round to nearest even)."""
    with np.errstate(invalid="ignore"):
        return _np(arr).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _libm_cached(fn, xbits):
    return libm_one(fn, np.frombuffer(np.uint64(xbits).tobytes(), dtype=np.float64)[0].item())


def expected(fn, args, ret):
    """The result of registry function `fn` over pyarrow arrays `args`, as a pyarrow array of type TYPES[ret]."""
    out_valid = np.logical_and.reduce([validity_np(a) for a in args])
    tn = _tn(args[0])
    rdt = np.dtype(TYPES[ret].to_pandas_dtype())

    def done(res):
        return pa.array(np.asarray(res, dtype=rdt), TYPES[ret], mask=~out_valid)

    if fn in TRIG:
        x = _as_double(args[0])
        return done([_libm_cached(fn, b) for b in x.view(np.uint64).tolist()])
    if fn == "atan2":
        return done([atan2_one(y, x) for y, x in zip(_np(args[0]).tolist(), _np(args[1]).tolist())])
    if fn in ANGLES:
        with np.errstate(all="ignore"):
            return done(_as_double(args[0]) * np.float64(DEG if fn == "degrees" else RAD))
    if fn == "sign":
        return done(sign_float(_np(args[0])) if tn[0] == "f" else [sign_int(a) for a in _np(args[0]).tolist()])
    if fn == "round" and len(args) == 1:
        return done(_np(args[0]))
    if fn == "round" and tn[0] == "f":
        with np.errstate(all="ignore"):
            return done(float_to_scale(_np(args[0]).astype(np.float64), _np(args[1]).tolist()).astype(rdt))
    a, b = _np(args[0]).tolist(), _np(args[1]).tolist()
    if fn == "pmod":
        return done([pmod(x, y, tn) for x, y in zip(a, b)])
    if fn in ("round", "truncate"):
        return done([int_to_scale(x, s, tn, fn == "round") for x, s in zip(a, b)])
    if fn.startswith("shift_"):
        return done([shift(fn, x, n, tn) for x, n in zip(a, b)])
    if fn == "gcd":
        return done([gcd(x, y) for x, y in zip(a, b)])
    if fn == "lcm":
        return done([lcm(x, y) for x, y in zip(a, b)])
    raise NotImplementedError(fn)


# ---- the shared cases --------------------------------------------------------------------------------------------------
ROWS = 4099
# scales and counts: every value in -25..25, the table's ends and one past them, the counts at and around both widths,
# INT32_MIN and INT32_MAX
SCALES = sorted(set(range(-25, 26)) | {308, -308, 309, -309, INT32_MIN, INT32_MAX, 31, 32, 33, 63, 64, 65, -31, -32, -33, -63, -64, -65})
PER_SCALE = ROWS // len(SCALES)          # value rows per scale in the cross product (61)
ROUND_ME = [2.5, -2.5, 0.125, -0.125, 1e308, -1e308, 1.005, 2.675, -2.675, 1234.5678, -1234.5678, 0.5, -0.5, 1.5, 0.05, 0.15, 0.25, 0.35,
            4503599627370496.5, 123456789.125, 15.0, 149.99999999999997, 1e22, 1e-7, 5e-8, 0.49999999999999994, 1e300, 9.995e307]

COLUMNS = [("i32_a", "i32"), ("i32_b", "i32"), ("i64_a", "i64"), ("i64_b", "i64"), ("f32_a", "f32"), ("f64_a", "f64"), ("f64_b", "f64"),
           ("t_wide", "f64"), ("t_dense", "f64"), ("t_unit", "f64"), ("t_hyp", "f64"),
           ("s_i32", "i32"), ("s_i64", "i64"), ("s_f32", "f32"), ("s_f64", "f64"), ("sc", "i32")]
SCHEMA = pa.schema([(name, TYPES[tn]) for name, tn in COLUMNS])
FAMILIES = ["trig", "trig_narrow", "angles_sign", "pmod_gcd", "scale", "shifts"]


def _scaled_column(rng, tn):
    """PER_SCALE values x every scale: value j at rows [j * len(SCALES), (j + 1) * len(SCALES)); random rows follow."""
    t = TYPES[tn]
    dt = np.dtype(t.to_pandas_dtype())
    vals = full_range_values(rng, t, ROWS)
    if tn[0] == "f":
        with np.errstate(over="ignore"):          # (1e308 as float32 is the infinity)
            e = np.concatenate([np.array(ROUND_ME, dtype=np.float64).astype(dt), edge_values(t)])[:PER_SCALE]
    else:
        hand = [125, -125, 2147483647, 15, 25, 35, -15, 5, -5, 4, -4, 49, 50, 51, 499999999, 500000000, 1500000000]
        e = np.array((hand + edge_values(t))[:PER_SCALE], dtype=dt)
    assert len(e) == PER_SCALE
    vals[:PER_SCALE * len(SCALES)] = np.repeat(e, len(SCALES))
    return vals


@functools.lru_cache(maxsize=None)
def _columns():
    """The values of every column (numpy), the same for both null shares: only the validity differs between batches."""
    rng = np.random.default_rng(20261)
    cols = {}
    for tn in ("i32", "i64", "f64"):
        cols[tn + "_a"], cols[tn + "_b"] = edge_pair_values(rng, TYPES[tn], ROWS)
    cols["f32_a"] = edge_pair_values(rng, TYPES["f32"], ROWS)[0]
    wide = full_range_values(rng, pa.float64(), ROWS)                       # exponent-uniform, huge arguments included
    e = edge_values(pa.float64())
    wide[:len(e)] = e
    cols["t_wide"] = wide
    dense = rng.uniform(-2 * math.pi, 2 * math.pi, ROWS)
    near = np.array([k * HALF_PI for k in range(-60, 61)])                  # the doubles nearest k pi/2 and their neighbours
    near = np.concatenate([near, np.nextafter(near, np.inf), np.nextafter(near, -np.inf)])
    dense[:len(near)] = near
    cols["t_dense"] = dense
    unit = rng.uniform(-1.0, 1.0, ROWS)
    u = [0.0, -0.0, 1.0, -1.0, np.nextafter(1.0, 2.0), -np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), 0.5, -0.5, 2.0, -1.5, 1e300,
         np.inf, -np.inf, np.nan, 5e-324, -5e-324, 2.2250738585072014e-308, 1e-9, -1e-9, 0.7071067811865476]
    unit[:len(u)] = u
    unit[len(u):len(u) + 400] = np.exp2(rng.uniform(-1074, 0, 400)) * rng.choice([-1.0, 1.0], 400)   # every magnitude below 1
    cols["t_unit"] = unit
    hyp = rng.uniform(-711.0, 711.0, ROWS)
    h = [0.0, -0.0, 710.4758600739439, 710.475860073944, -710.4758600739439, -710.475860073944, 711.5, -711.5, 720.0, -720.0, 1e3, -1e3,
         1e308, np.inf, -np.inf, np.nan, 5e-324, 1e-9, -1e-9, 22.0, -22.0, 19.061547465398498, 0.5493061443340549]
    hyp[:len(h)] = h
    hyp[len(h):len(h) + 400] = np.exp2(rng.uniform(-1074, 0, 400)) * rng.choice([-1.0, 1.0], 400)
    cols["t_hyp"] = hyp
    for tn in ("i32", "i64", "f32", "f64"):
        cols["s_" + tn] = _scaled_column(rng, tn)
    sc = np.array(SCALES, dtype=np.int64)[rng.integers(0, len(SCALES), ROWS)]
    sc[:PER_SCALE * len(SCALES)] = np.tile(np.array(SCALES, dtype=np.int64), PER_SCALE)
    cols["sc"] = sc.astype(np.int32)
    return cols


@functools.lru_cache(maxsize=None)
def batch(nulls):
    """The 4099-row batch over SCHEMA; `nulls` = the fraction of null rows in every column."""
    rng = np.random.default_rng(20262 + int(nulls * 100))
    cols = _columns()
    arrays = [pa.array(cols[name], TYPES[tn], mask=(rng.random(ROWS) < nulls) if nulls > 0 else None) for name, tn in COLUMNS]
    return pa.RecordBatch.from_arrays(arrays, schema=SCHEMA)


def _spec(fn, args, ret, ulps=None, host_ulps=None, domain=None):
    label = "%s(%s)" % (fn, ",".join(a if isinstance(a, str) else a["label"] for a in args))
    return {"label": label, "fn": fn, "args": list(args), "ret": ret, "tier0": True, "ulps": ulps, "host_ulps": host_ulps, "domain": domain}


# The largest distance from the correctly rounded value, in ulps, per (function, domain column): measured on an MI355X
# (the specialised kernel and the interpreter agree bit for bit, so one figure serves both) and, separately, for the host
# build's libm (glibc).  The project's bar is 1 ulp (PARITY.md, `round trunc ... power`); an entry above it is a measurement
# named in PARITY.md's numeric-tail row, never a silent widening.  profiles/numeric_tail.txt holds the same figures.
BAR = 1
MEASURED_ULPS = {}
HOST_MEASURED_ULPS = {}

TRIG_DOMAINS = {"sin": ("t_wide", "t_dense"), "cos": ("t_wide", "t_dense"), "tan": ("t_wide", "t_dense"), "cot": ("t_wide", "t_dense"),
                "asin": ("t_unit",), "acos": ("t_unit",), "atan": ("t_wide", "t_dense"), "sinh": ("t_hyp",), "cosh": ("t_hyp",),
                "tanh": ("t_hyp", "t_wide")}
NARROW = ("i32_a", "i64_a", "f32_a")      # the int32 / int64 / float32 signatures: the argument converted to double first


def _libm(fn, cols, dom):
    return _spec(fn, cols, "f64", ulps=MEASURED_ULPS.get((fn, dom), BAR), host_ulps=HOST_MEASURED_ULPS.get((fn, dom), BAR), domain=dom)


@functools.lru_cache(maxsize=None)
def family_specs(family):
    s = []
    if family == "trig":
        for fn in TRIG:
            s += [_libm(fn, [c], c) for c in TRIG_DOMAINS[fn]]
        s.append(_libm("atan2", ["f64_a", "f64_b"], "f64_a"))
    elif family == "trig_narrow":
        for fn in TRIG:
            s += [_libm(fn, [c], c) for c in NARROW]
    elif family == "angles_sign":
        for fn in ANGLES:
            s += [_spec(fn, [c], "f64") for c in ("t_wide", "t_dense") + NARROW]
        s += [_spec("sign", [c], c[:3]) for c in ("i32_a", "i64_a", "f32_a", "f64_a")] + [_spec("sign", ["t_wide"], "f64")]
    elif family == "pmod_gcd":
        for tn in ("i32", "i64"):
            s += [_spec("pmod", [tn + "_a", tn + "_b"], tn), _spec("pmod", [tn + "_b", tn + "_a"], tn)]
        s += [_spec(fn, ["i64_a", "i64_b"], "i64") for fn in ("gcd", "lcm")]
    elif family == "scale":
        for tn in ("i32", "i64"):
            s += [_spec("round", ["s_" + tn], tn), _spec("round", ["s_" + tn, "sc"], tn), _spec("truncate", ["s_" + tn, "sc"], tn),
                  _spec("round", [tn + "_a", "sc"], tn), _spec("truncate", [tn + "_a", "sc"], tn)]
        s += [_spec("round", ["s_f32", "sc"], "f32"), _spec("round", ["s_f64", "sc"], "f64"), _spec("round", ["f32_a", "sc"], "f32"),
              _spec("round", ["f64_a", "sc"], "f64"), _spec("round", ["t_dense", "sc"], "f64")]
    elif family == "shifts":
        for tn in ("i32", "i64"):
            for fn in ("shift_left", "shift_right", "shift_right_unsigned"):
                s += [_spec(fn, ["s_" + tn, "sc"], tn), _spec(fn, [tn + "_a", "i32_b"], tn)]
    else:
        raise KeyError(family)
    return s


def expected_of(sp, b):
    return expected(sp["fn"], [b.column(a) if isinstance(a, str) else expected_of(a, b) for a in sp["args"]], sp["ret"])


@functools.lru_cache(maxsize=None)
def expected_columns(family, nulls):
    """The reference's result for every expression of a family over batch(nulls): computed once, shared, never changed."""
    b = batch(nulls)
    return [expected_of(sp, b) for sp in family_specs(family)]


def build_expressions(gandiva, specs, schema=None):
    """gandiva expressions for a list of specs, over SCHEMA."""
    schema = SCHEMA if schema is None else schema
    b = gandiva.TreeExprBuilder()
    out = []

    def node_of(sp):
        args = [b.make_field(schema.field(a)) if isinstance(a, str) else node_of(a) for a in sp["args"]]
        return b.make_function(sp["fn"], args, TYPES[sp["ret"]])
    for i, sp in enumerate(specs):
        out.append(b.make_expression(node_of(sp), pa.field("r%d" % i, TYPES[sp["ret"]])))
    return out
