"""An independent reference for the date and time functions — extractors, date_trunc_*, last_day, the adds, the diffs,
the fixed-width casts and to_timestamp / to_time over numbers — on full-range operands: all of date32, all of int64
milliseconds.  It shares no code with the oracle (oracle/gdv_oracle.c) or with the device library (gdv_device_lib.hpp)
and does not restate their day-count formulas: the civil date of a day count is datetime.date.fromordinal of the day
shifted by whole 146097-day cycles into 2000-01-01..2399-12-31, plus 400 years per cycle; day of year, ISO week and
weekday are those of the shifted date (a whole number of weeks and of leap-year cycles lies between the two).  Every
rule is written on Python `int`: divmod floors, tdiv truncates, results are narrowed to their type at the very end.

A result is None ("left out") where the exact result or an exact intermediate of the device library's arithmetic
(c * unit, v + c * unit, e - s, day * 86400000) lies outside int64: signed overflow is undefined there.  Narrowing to
int32 is never a reason: the expected value is the two's-complement narrowing of the exact one.

The second half holds the cases that tests/test_full_range_temporal_cpu.py (oracle, host build of the device library)
and tests/test_full_range_temporal.py (GPU: specialised kernels and the tier-0 interpreter) share."""
import calendar
import datetime as dt
import functools

import numpy as np
import pyarrow as pa

from helpers import edge_values, full_range_values, validity_np

MS = 86400000
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
CYCLE = 146097                                             # days in 400 Gregorian years, a multiple of 7
_ORD_2000 = dt.date(2000, 1, 1).toordinal()
_DAY_2000 = _ORD_2000 - dt.date(1970, 1, 1).toordinal()    # the day count of 2000-01-01
assert dt.date(2400, 1, 1).toordinal() - _ORD_2000 == CYCLE and CYCLE % 7 == 0


def tdiv(a, b):
    """a / b truncated toward zero."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def tmod(a, b):
    return a - tdiv(a, b) * b


def wrap(v, w):
    """Python integer v reduced modulo 2^w and re-read as signed."""
    v &= (1 << w) - 1
    return v - (1 << w) if v >> (w - 1) else v


def _in64(v):
    return I64_MIN <= v <= I64_MAX


@functools.lru_cache(maxsize=None)
def civil(day):
    """(year, month, day of month, the date shifted into 2000..2399) of a day count since 1970-01-01, any Python int."""
    q, r = divmod(day - _DAY_2000, CYCLE)
    d = dt.date.fromordinal(_ORD_2000 + r)
    return d.year + 400 * q, d.month, d.day, d


def day_of(y, m, d):
    """The day count since 1970-01-01 of a proleptic Gregorian date, any year."""
    q, yy = divmod(y - 2000, 400)
    return dt.date(2000 + yy, m, d).toordinal() - _ORD_2000 + _DAY_2000 + q * CYCLE


def last_dom(y, m):
    return calendar.monthrange(2000 + (y - 2000) % 400, m)[1]


# ---- the rules (PARITY.md; the comments of gdv_device_lib.hpp's date / time section) -----------------------------------
_FIXED = {"Second": 1000, "Minute": 60000, "Hour": 3600000, "Day": MS, "Week": 7 * MS}
_PER = {"Month": 1, "Quarter": 3, "Year": 12}
EXTRACT_PARTS = ["Year", "Month", "Day", "Quarter", "Doy", "Dow", "Hour", "Minute", "Second", "Epoch", "Decade", "Century", "Millennium"]
TRUNC_UNITS = ["Second", "Minute", "Hour", "Day", "Week", "Month", "Quarter", "Year", "Decade", "Century", "Millennium"]
ADD_UNITS = DIFF_UNITS = ["Second", "Minute", "Hour", "Day", "Week", "Month", "Quarter", "Year"]


def extract(part, tn, v):
    if tn == "t32":
        return {"Hour": v // 3600000, "Minute": v // 60000 % 60, "Second": v // 1000 % 60}[part]
    ms = v * MS if tn == "d32" else v
    day, tod = divmod(ms, MS)                              # floored day, time of day in [0, 86400000)
    if part == "Hour":
        return tod // 3600000
    if part == "Minute":
        return tod // 60000 % 60
    if part == "Second":
        return tod // 1000 % 60
    if part == "Epoch":
        return ms // 1000
    y, m, d, shifted = civil(day)
    if part == "Year":
        return y
    if part == "Month":
        return m
    if part == "Day":
        return d
    if part == "Quarter":
        return (m - 1) // 3 + 1
    if part == "Doy":
        return shifted.timetuple().tm_yday
    if part == "Dow":
        return shifted.isoweekday() % 7 + 1                # 1 = Sunday ... 7 = Saturday
    if part == "Week":
        return shifted.isocalendar()[1]
    if part == "Decade":
        return tdiv(y, 10)
    return tdiv(y - 1, {"Century": 100, "Millennium": 1000}[part]) + 1


def date_trunc(unit, v):
    """Start of the unit: fixed units toward zero; weeks from Monday; Decade / Century / Millennium start in year ...1."""
    if unit in _FIXED and unit != "Week":
        return tdiv(v, _FIXED[unit]) * _FIXED[unit]
    day = v // MS
    y, m, _, shifted = civil(day)
    if unit == "Week":
        r = day - (shifted.isoweekday() - 1)
    elif unit == "Month":
        r = day_of(y, m, 1)
    elif unit == "Quarter":
        r = day_of(y, (m - 1) // 3 * 3 + 1, 1)
    elif unit == "Year":
        r = day_of(y, 1, 1)
    elif unit == "Last":
        r = day_of(y, m, last_dom(y, m))
    else:
        n = {"Decade": 10, "Century": 100, "Millennium": 1000}[unit]
        r = day_of(tdiv(y - 1, n) * n + 1, 1, 1)
    return r * MS if _in64(r * MS) else None


def add_months(v, months):
    """Month addition, the day of month clamped to the target month's last."""
    day, tod = divmod(v, MS)
    y, m, d, _ = civil(day)
    ny, nm = divmod(y * 12 + (m - 1) + months, 12)
    nm += 1
    p = day_of(ny, nm, min(d, last_dom(ny, nm))) * MS
    return p + tod if _in64(months) and _in64(p) and _in64(p + tod) else None


def timestampadd(unit, c, v):
    if unit in _PER:
        return add_months(v, c * _PER[unit]) if _in64(c * _PER[unit]) else None
    p = c * _FIXED[unit]
    return v + p if _in64(p) and _in64(v + p) else None


def date_add(v, c, sign):
    p = c * MS
    return v + sign * p if _in64(p) and _in64(v + sign * p) else None


def months_between(s, e):
    """Whole calendar months from s to e, on the pair in ascending order: the last month counts when the end's day of month
    has reached the start's, or the end is the last day of its month, and on the same day of month when the end's time of
    day in whole seconds has reached the start's."""
    fwd = e > s
    if not fwd:
        s, e = e, s
    (sday, stod), (eday, etod) = divmod(s, MS), divmod(e, MS)
    ay, am, ad, _ = civil(sday)
    by, bm, bd, _ = civil(eday)
    m = 12 * (by - ay) + (bm - am)
    if bd < ad:
        m -= 0 if bd == last_dom(by, bm) else 1
    elif bd == ad:
        m -= 0 if etod // 1000 >= stod // 1000 else 1
    return m if fwd else -m


def timestampdiff(unit, s, e):
    if unit in _PER:
        return wrap(tdiv(months_between(s, e), _PER[unit]), 32)     # the exact count divided, then narrowed
    return wrap(tdiv(e - s, _FIXED[unit]), 32) if _in64(e - s) else None


def datediff(tn, e, s):
    return wrap(e - s, 32) if tn == "d32" else wrap(e // MS - s // MS, 32)


def _saturate(x):
    """float -> int64: truncated, saturating, NaN -> 0."""
    if x != x:
        return 0
    if x >= 2.0 ** 63:
        return I64_MAX
    if x <= -2.0 ** 63:
        return I64_MIN
    return int(x)


def seconds_to_millis(tn, v):
    """to_timestamp: integer seconds * 1000 modulo 2^64; float seconds * 1000 rounded once in their own format (v arrives as
    a numpy scalar of that format), then converted saturating."""
    if tn in ("i32", "i64"):
        return wrap(v * 1000, 64)
    with np.errstate(over="ignore", invalid="ignore"):
        return _saturate(float(v * type(v)(1000)))


def cast(fn, tn, v):
    if fn == "castDATE" and tn == "ts":
        r = v // MS * MS
        return r if _in64(r) else None
    if fn in ("castDATE", "castTIMESTAMP") and tn == "d32":
        return v * MS
    if fn == "castDATE32":
        return wrap(v // MS, 32)
    if fn == "castTIME":
        return v % MS
    return v                                                 # castDATE / castTIMESTAMP / castBIGINT between 64-bit types


def row_function(fn, tns):
    """The rule of registry function `fn` over argument types `tns` as a function of one row's Python values."""
    t0 = tns[0]
    if fn in ("extractWeek", "weekofyear"):
        return lambda v: extract("Week", t0, v)
    if fn.startswith("extract"):
        return lambda v: extract(fn[7:], t0, v)
    if fn.startswith("date_trunc_"):
        return lambda v: date_trunc(fn[11:], v)
    if fn == "last_day":
        return lambda v: date_trunc("Last", v)
    if fn.startswith("timestampadd"):
        return lambda c, v: timestampadd(fn[12:], c, v)
    if fn in ("date_add", "date_sub"):
        return lambda v, c: date_add(v, c, 1 if fn == "date_add" else -1)
    if fn.startswith("timestampdiff"):
        return lambda s, e: timestampdiff(fn[13:], s, e)
    if fn in ("datediff", "date_diff"):
        return lambda e, s: datediff(t0, e, s)
    if fn == "to_timestamp":
        return lambda v: seconds_to_millis(t0, v)
    if fn == "to_time":
        return lambda v: tmod(seconds_to_millis(t0, v), MS)
    if fn.startswith("cast"):
        return lambda v: cast(fn, t0, v)
    raise NotImplementedError(fn)


# ---- the shared cases --------------------------------------------------------------------------------------------------
TYPES = {"d32": pa.date32(), "d64": pa.date64(), "ts": pa.timestamp("ms"), "t32": pa.time32("ms"), "i32": pa.int32(),
         "i64": pa.int64(), "f32": pa.float32(), "f64": pa.float64()}
STORAGE = {"d32": pa.int32(), "d64": pa.int64(), "ts": pa.int64(), "t32": pa.int32(), "i32": pa.int32(), "i64": pa.int64(),
            "f32": pa.float32(), "f64": pa.float64()}
TYPE_NAMES = {"d32": "date32", "d64": "date64", "ts": "timestamp", "t32": "time32", "i32": "int32", "i64": "int64",
              "f32": "float32", "f64": "float64"}
ROWS = 4099
CROSS = 32
COLUMNS = [("d32_a", "d32"), ("d32_b", "d32"), ("d64_a", "d64"), ("d64_b", "d64"), ("ts_a", "ts"), ("ts_b", "ts"), ("t32_a", "t32"),
           ("c_i32", "i32"), ("c_i64", "i64"), ("c_n64", "i64"), ("s_i32", "i32"), ("s_i64", "i64"), ("s_f32", "f32"), ("s_f64", "f64")]
SCHEMA = pa.schema([(name, TYPES[tn]) for name, tn in COLUMNS])
FAMILIES = ["extract", "trunc", "add", "diff", "casts_seconds"]
MAX_LEFT_OUT = 0.10

# the two pairs on which timestampdiffQuarter / Year once divided a month count already narrowed to 32 bits:
# (start, end, Month, Quarter, Year).  The exact counts are 3276778018 months (-1047928-02-19 05:18:09.579 to
# 272016907-01-14 22:47:06.794: 12 * 273064835 - 1, less one as the 14th has not reached the 19th) and 2310287929
# (1969-12-31 23:59:52.820 to 192525964-02-27 01:18:58.731): neither fits int32, so Month is the narrowed count, while
# Quarter and Year fit and must be exact.
MONTH_COUNT_PAIRS = [(-33131576515310421, 8583962311378026794, wrap(3276778018, 32), 1092259339, 273064834),
                     (-7180, 6075470442388738731, wrap(2310287929, 32), 770095976, 192523994)]

EDGE_DATES = [(0, 2, 29), (0, 3, 1), (1, 1, 1), (-1, 12, 31), (-400, 2, 29), (-100, 3, 1), (1582, 10, 15), (1600, 2, 29),
              (1900, 2, 28), (1900, 3, 1), (2000, 2, 29), (2100, 2, 28), (2400, 2, 29), (9999, 12, 31), (10000, 1, 1)] + \
             [(2023, m, 31) for m in (1, 3, 5, 7, 8, 10, 12)] + \
             [(2020, 12, 31), (2021, 1, 3), (2021, 1, 4), (2026, 12, 31), (0, 1, 1), (0, 1, 2), (0, 1, 3)]
COUNT_EDGES = [0, 1, -1, 12, -13, 1200, 2 ** 31 - 1, -2 ** 31]
# Quarter and Year take narrower counts, per row (column c_n64, below 2^27) and as literals: 2^31 quarters are 537 million
# years and 2^31 years need no saying, so next to +-292 million years of int64 milliseconds every row would be left out
NARROW_COUNT_EDGES = {"Quarter": COUNT_EDGES[:6] + [2 ** 29 - 1, -2 ** 29], "Year": COUNT_EDGES[:6] + [2 ** 27 - 1, -2 ** 27]}


def ms_edges():
    """Edge instants in milliseconds, most important first: the type's ends, 0, +-1, +-1 day +-1 ms, then the first and
    last millisecond of every edge date, then the operands of MONTH_COUNT_PAIRS."""
    out = [I64_MIN, I64_MAX, 0, 1, -1, MS + 1, MS - 1, -MS + 1, -MS - 1]
    for y, m, d in EDGE_DATES:
        out += [day_of(y, m, d) * MS, day_of(y, m, d) * MS + MS - 1]
    for s, e, *_ in MONTH_COUNT_PAIRS:
        out += [s, e]
    return out


def day_edges():
    return [-(1 << 31), (1 << 31) - 1, 0, 1, -1] + [day_of(y, m, d) for y, m, d in EDGE_DATES]


def _exponent_uniform(rng, n, w):
    """n signed integers below 2^(w-1) in magnitude in which every magnitude is equally likely, as int64."""
    raw = rng.integers(-(1 << (w - 1)), (1 << (w - 1)) - 1, n, dtype=np.int64, endpoint=True)
    return raw >> rng.integers(0, w - 1, n)


def _rule_pair(rng):
    """A pair on the edges of the month-count rule (end = start moved by whole months, nudged; or month ends against a 29th
    to 31st), at a random shift of whole 400-year cycles."""
    from dateutil.relativedelta import relativedelta
    epoch = dt.datetime(1970, 1, 1)
    if rng.integers(0, 2):
        start = dt.datetime(2000, 1, 1) + dt.timedelta(milliseconds=int(rng.integers(0, CYCLE * MS)))
        end = start + relativedelta(months=int(rng.integers(-40, 41)))
        nudge = [0, 1000, -1000, MS, -MS, 999, -999, 0][int(rng.integers(0, 8))]
    else:
        y, m = int(rng.integers(2000, 2400)), int(rng.integers(1, 13))
        start = dt.datetime(int(rng.integers(2000, 2400)), [1, 3, 5, 7, 8, 10, 12][int(rng.integers(0, 7))], int(rng.integers(28, 32)),
                            int(rng.integers(0, 24)), int(rng.integers(0, 60)), int(rng.integers(0, 60)))
        end = dt.datetime(y, m, calendar.monthrange(y, m)[1], int(rng.integers(0, 24)), int(rng.integers(0, 60)), int(rng.integers(0, 60)))
        nudge = 0
    limit = (I64_MAX // MS - 2 * CYCLE) // CYCLE              # whole cycles that keep the pair inside int64 milliseconds
    shift = min(max(int(_exponent_uniform(rng, 1, 21)[0]), -limit), limit)
    to_ms = lambda t: (t - epoch) // dt.timedelta(milliseconds=1) + shift * CYCLE * MS
    return to_ms(start), to_ms(end) + nudge


def instant_pairs(rng, n=ROWS):
    """Two int64 millisecond columns: the cross product of the first CROSS edges, the pairs of MONTH_COUNT_PAIRS, then random
    rows: exponent-uniform firsts; one row in eight a pair on the month-count rule's edges, one in three (of the rest)
    carrying an edge of the whole list in either or both columns, half of the others the first plus an exponent-uniform
    offset of up to 2^40 ms and half independent."""
    edges = np.array(ms_edges(), dtype=np.int64)
    a, b = _exponent_uniform(rng, n, 64), _exponent_uniform(rng, n, 64)
    near = np.array([min(max(x + o, I64_MIN), I64_MAX) for x, o in zip(a.tolist(), _exponent_uniform(rng, n, 42).tolist())], dtype=np.int64)
    k = CROSS * CROSS
    for i in range(k, n):
        r = i - k
        if r % 8 == 0:
            a[i], b[i] = _rule_pair(rng)
        elif r % 3 == 1:
            which = int(rng.integers(0, 3))
            if which != 1:
                a[i] = edges[int(rng.integers(0, len(edges)))]
            if which != 0:
                b[i] = edges[int(rng.integers(0, len(edges)))]
        elif r % 2 == 0:
            b[i] = near[i]
    a[:k], b[:k] = np.repeat(edges[:CROSS], CROSS), np.tile(edges[:CROSS], CROSS)
    for j, (s, e, *_) in enumerate(MONTH_COUNT_PAIRS):
        a[k + j], b[k + j] = s, e
    return a, b


def day_pairs(rng, n=ROWS):
    """Two date32 columns (int32 days) laid out like instant_pairs, the near offset up to 2^20 days."""
    edges = np.array(day_edges(), dtype=np.int64)
    a, b = _exponent_uniform(rng, n, 32), _exponent_uniform(rng, n, 32)
    near = np.clip(a + _exponent_uniform(rng, n, 22), -(1 << 31), (1 << 31) - 1)
    k = CROSS * CROSS
    r = np.arange(n) - k
    b = np.where((r % 3 != 1) & (r % 2 == 0), near, b)
    pick = np.flatnonzero((r >= 0) & (r % 3 == 1))
    which = rng.integers(0, 3, len(pick))
    a[pick[which != 1]] = edges[rng.integers(0, len(edges), int((which != 1).sum()))]
    b[pick[which != 0]] = edges[rng.integers(0, len(edges), int((which != 0).sum()))]
    a[:k], b[:k] = np.repeat(edges[:CROSS], CROSS), np.tile(edges[:CROSS], CROSS)
    return a.astype(np.int32), b.astype(np.int32)


def _front(edges, vals):
    vals = vals.copy()
    vals[:len(edges)] = edges
    return vals


@functools.lru_cache(maxsize=None)
def batch(nulls):
    """The 4099-row batch over SCHEMA; `nulls` = the fraction of null rows in every column."""
    rng = np.random.default_rng(20261 + int(nulls * 100))
    cols = {}
    cols["d32_a"], cols["d32_b"] = day_pairs(rng)
    cols["d64_a"], cols["d64_b"] = instant_pairs(rng)
    cols["ts_a"], cols["ts_b"] = instant_pairs(rng)
    # a legal time of day, every magnitude: the extractors over time32 are defined on [0, 86400000)
    cols["t32_a"] = _front([0, 1, 999, 1000, 59999, 60000, 3599999, 3600000, MS - 1], np.abs(_exponent_uniform(rng, ROWS, 32)) % MS).astype(np.int32)
    # counts: every row of the cross product's first column meets every literal-count edge; exponent-uniform below 2^31
    i = np.arange(ROWS)
    cycle = np.array(COUNT_EDGES, dtype=np.int64)[(i + i // CROSS) % len(COUNT_EDGES)]
    for name in ("c_i32", "c_i64"):
        c = _exponent_uniform(rng, ROWS, 32)
        c[:CROSS * CROSS] = cycle[:CROSS * CROSS]
        cols[name] = c.astype(np.int32 if name == "c_i32" else np.int64)
    cols["c_n64"] = _exponent_uniform(rng, ROWS, 28)
    cols["c_n64"][:CROSS * CROSS] = np.array(NARROW_COUNT_EDGES["Year"], dtype=np.int64)[(i + i // CROSS) % len(COUNT_EDGES)][:CROSS * CROSS]
    for name, tn in (("s_i32", "i32"), ("s_i64", "i64")):
        cols[name] = _front(np.array(edge_values(TYPES[tn])), full_range_values(rng, TYPES[tn], ROWS))
    # seconds as floats: the type's edges, the products on either side of 2^63 ms, halves and thousandths, a day's ends
    extra = [9223372036854775.0, 9223372036854776.0, 9223372036854777.0, -9223372036854776.0, 1.5, -1.5, 0.0005, -0.0005, 0.001,
             86399.999, 86400.0, -86400.001, 1e15, -1e15, 4.2e9, 253402300799.999]
    for name, tn in (("s_f32", "f32"), ("s_f64", "f64")):
        e = np.concatenate([edge_values(TYPES[tn]), np.array(extra).astype(TYPES[tn].to_pandas_dtype())])
        cols[name] = _front(e, full_range_values(rng, TYPES[tn], ROWS))
    arrays = []
    for name, tn in COLUMNS:
        mask = (rng.random(ROWS) < nulls) if nulls > 0 else None
        arrays.append(pa.array(cols[name], STORAGE[tn], mask=mask).view(TYPES[tn]))
    return pa.RecordBatch.from_arrays(arrays, schema=SCHEMA)


def _lit(v, tn):
    return {"lit": v, "type": tn}


def _spec(fn, args, ret, host=None):
    """An expression: `args` are column names or literals; `host` names the host-build entry point that computes it."""
    label = "%s(%s)" % (fn, ",".join(a if isinstance(a, str) else str(a["lit"]) for a in args))
    return {"label": label, "fn": fn, "args": list(args), "ret": ret, "tier0": True, "ulps": None, "host": host}


def arg_type(a):
    return dict(COLUMNS)[a] if isinstance(a, str) else a["type"]


def symbol_of(sp):
    """The device library's symbol for a spec, as gdv_tier0_fns.inc spells it (an alias shares its target's)."""
    fn = {"weekofyear": "extractWeek", "date_diff": "datediff"}.get(sp["fn"], sp["fn"])
    return fn + "_" + "_".join(TYPE_NAMES[arg_type(a)] for a in sp["args"])


@functools.lru_cache(maxsize=None)
def family_specs(family):
    s = []
    if family == "extract":
        for k, tn in enumerate(("d32", "d64", "ts")):
            for c in ("_a", "_b"):
                s += [_spec("extract" + part, [tn + c], "i64", host=("unary", k, op)) for op, part in enumerate(EXTRACT_PARTS)]
        s += [_spec("extract" + part, ["t32_a"], "i64", host=("cast", 10 + op, 0)) for op, part in enumerate(("Hour", "Minute", "Second"))]
    elif family == "trunc":
        for k, tn in ((1, "d64"), (2, "ts")):
            for c in ("_a", "_b"):
                s += [_spec("date_trunc_" + u, [tn + c], tn, host=("trunc", k, op)) for op, u in enumerate(TRUNC_UNITS)]
                s += [_spec("extractWeek", [tn + c], "i64", host=("trunc", k, 11)), _spec("weekofyear", [tn + c], "i64", host=("trunc", k, 11)),
                      _spec("last_day", [tn + c], "d64", host=("trunc", k, 12))]
    elif family == "add":
        for k, tn in ((1, "d64"), (2, "ts")):
            s += [_spec("timestampadd" + u, ["c_n64" if u in NARROW_COUNT_EDGES else "c_i64", tn + "_a"], tn, host=("add", k, op)) for op, u in enumerate(ADD_UNITS)]
            s += [_spec("date_add", [tn + "_a", "c_i64"], tn, host=("add", k, 8)), _spec("date_sub", [tn + "_a", "c_i64"], tn, host=("add", k, 9)),
                  _spec("date_add", [tn + "_a", "c_i32"], tn, host=("add", k, 10)), _spec("date_sub", [tn + "_a", "c_i32"], tn, host=("add", k, 11))]
            for j, c in enumerate(COUNT_EDGES):
                s += [_spec("timestampadd" + u, [_lit(NARROW_COUNT_EDGES.get(u, COUNT_EDGES)[j], "i64"), tn + "_b"], tn, host=("add", k, ADD_UNITS.index(u)))
                      for u in ("Month", "Quarter", "Year", "Day")]
                s.append(_spec("date_add", [tn + "_b", _lit(c, "i32")], tn, host=("add", k, 10)))
    elif family == "diff":
        for k, tn in ((1, "d64"), (2, "ts")):
            s += [_spec("timestampdiff" + u, [tn + "_a", tn + "_b"], "i32", host=("diff", k, op)) for op, u in enumerate(DIFF_UNITS)]
            s += [_spec("timestampdiff" + u, [tn + "_b", tn + "_a"], "i32", host=("diff", k, 5 + op)) for op, u in enumerate(("Month", "Quarter", "Year"))]
            s += [_spec(fn, [tn + "_a", tn + "_b"], "i32", host=("diff", k, 8)) for fn in ("datediff", "date_diff")]
        s += [_spec(fn, ["d32_a", "d32_b"], "i32", host=("diff", 0, 8)) for fn in ("datediff", "date_diff")]
    elif family == "casts_seconds":
        for c in ("_a", "_b"):
            s += [_spec("castDATE", ["d32" + c], "d64", host=("cast", 0, 0)), _spec("castDATE", ["ts" + c], "d64", host=("cast", 1, 0)),
                  _spec("castDATE32", ["d64" + c], "d32", host=("cast", 2, 0)), _spec("castTIMESTAMP", ["d32" + c], "ts", host=("cast", 3, 0)),
                  _spec("castTIME", ["ts" + c], "t32", host=("cast", 4, 0)), _spec("castTIMESTAMP", ["d64" + c], "ts", host=("cast", 5, 0)),
                  _spec("castBIGINT", ["d64" + c], "i64", host=("cast", 6, 0)), _spec("castBIGINT", ["ts" + c], "i64", host=("cast", 7, 0))]
        s += [_spec("castDATE", ["s_i64"], "d64", host=("cast", 8, 0)), _spec("castTIMESTAMP", ["s_i64"], "ts", host=("cast", 9, 0))]
        for k, tn in enumerate(("i32", "i64", "f32", "f64")):
            s += [_spec("to_timestamp", ["s_" + tn], "ts", host=("to", k, 0)), _spec("to_time", ["s_" + tn], "t32", host=("to", k, 1))]
    else:
        raise KeyError(family)
    return s


def column_values(arr, tn):
    """The values of a column as Python ints (floats: numpy scalars of their format), 0 under nulls."""
    v = np.asarray(arr.view(STORAGE[tn]).fill_null(0))
    return list(v) if tn in ("f32", "f64") else v.tolist()


def expected_of(sp, b):
    """(expected pyarrow array, left-out bool numpy array) of one spec over a batch: NULL where an argument is NULL; a row
    that is left out holds 0 and is compared for validity only."""
    n = b.num_rows
    tns = [arg_type(a) for a in sp["args"]]
    vals = [column_values(b.column(a), tn) if isinstance(a, str) else [a["lit"]] * n for a, tn in zip(sp["args"], tns)]
    valid = np.logical_and.reduce([validity_np(b.column(a)) for a in sp["args"] if isinstance(a, str)])
    f = row_function(sp["fn"], tns)
    res = [f(*row) for row in zip(*vals)]
    left_out = np.array([r is None for r in res]) & valid
    out = np.array([0 if r is None else r for r in res], dtype=np.dtype(STORAGE[sp["ret"]].to_pandas_dtype()))
    share = left_out.sum() / max(valid.sum(), 1)
    assert share <= MAX_LEFT_OUT, "%s leaves out %.1f %% of its valid rows" % (sp["label"], 100 * share)
    return pa.array(out, STORAGE[sp["ret"]], mask=~valid).view(TYPES[sp["ret"]]), left_out


@functools.lru_cache(maxsize=None)
def expected_pairs(family, nulls):
    """(expected, left out) for every expression of a family over batch(nulls): computed once, shared, never changed."""
    b = batch(nulls)
    return [expected_of(sp, b) for sp in family_specs(family)]


def expected_columns(family, nulls):
    return [e for e, _ in expected_pairs(family, nulls)]


def left_out_columns(family, nulls):
    return [x for _, x in expected_pairs(family, nulls)]


def build_expressions(gandiva, specs):
    """gandiva expressions for a list of specs, over SCHEMA."""
    b = gandiva.TreeExprBuilder()
    out = []
    for i, sp in enumerate(specs):
        args = [b.make_field(SCHEMA.field(a)) if isinstance(a, str) else b.make_literal(a["lit"], TYPES[a["type"]]) for a in sp["args"]]
        out.append(b.make_expression(b.make_function(sp["fn"], args, TYPES[sp["ret"]]), pa.field("r%d" % i, TYPES[sp["ret"]])))
    return out
