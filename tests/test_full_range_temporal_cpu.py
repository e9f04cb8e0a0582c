"""The date and time functions on full-range operands, without a GPU: the independent reference
(tests/temporal_reference.py) against datetime, numpy's unbounded proleptic calendar and dateutil; then against the
oracle and against the host build of the device library, on the 4099-row batches of edge cross products and
exponent-uniform random rows that tests/test_full_range_temporal.py runs on the GPU.  A wrong reference, a wrong oracle
or a wrong device function is found here first."""
import ctypes as C
import datetime as dt
import os
import re

import numpy as np
import pyarrow as pa
import pytest
from dateutil.relativedelta import relativedelta

import gandiva_amd as gandiva
from oracle import oracle
import temporal_reference as R
from helpers import assert_bit_exact_where
from test_device_lib_on_host import hostlib  # noqa: F401  (the fixture that builds tests/host_devlib)

NULLS = (0.0, 0.1)
EPOCH_ORD = dt.date(1970, 1, 1).toordinal()
FNS_INC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gandiva_amd", "csrc", "gdv_tier0_fns.inc")


# ---- the reference against engines that share nothing with it ----------------------------------------------------------
def test_calendar_matches_datetime_on_years_1_to_9999():
    """Civil date, its inverse, day of year, weekday and ISO week against datetime itself: every 11th day of years
    1..9999, and Jan 1, Feb 28 / 29, Mar 1 and Dec 31 of every year (so of every year divisible by 100 and by 400)."""
    civil = R.civil.__wrapped__
    ordinals = set(range(1, dt.date(9999, 12, 31).toordinal() + 1, 11))
    for y in range(1, 10000):
        leap = y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)
        for m, d in ((1, 1), (2, 28), (2, 29) if leap else (2, 28), (3, 1), (12, 31)):
            ordinals.add(dt.date(y, m, d).toordinal())
        assert R.last_dom(y, 2) == (29 if leap else 28)
    for o in ordinals:
        d = dt.date.fromordinal(o)
        day = o - EPOCH_ORD
        y, m, dd, shifted = civil(day)
        assert (y, m, dd) == (d.year, d.month, d.day), d
        assert R.day_of(d.year, d.month, d.day) == day, d
        assert (shifted.timetuple().tm_yday, shifted.isoweekday(), shifted.isocalendar()[1]) == \
               (d.timetuple().tm_yday, d.isoweekday(), d.isocalendar()[1]), d
    d = dt.date(2021, 1, 3)     # a Sunday in ISO week 53 of 2020
    assert (R.extract("Dow", "d32", d.toordinal() - EPOCH_ORD), R.extract("Week", "ts", (d.toordinal() - EPOCH_ORD) * R.MS)) == (1, 53)


def test_year_month_and_day_match_numpy_over_all_of_date32_and_int64_milliseconds():
    """numpy's datetime64 calendar is proleptic Gregorian and unbounded: year, month and day of month of every day and
    instant of the shared batches and of 20000 more exponent-uniform ones, INT64_MIN (numpy's NaT) aside."""
    rng = np.random.default_rng(5)
    b = R.batch(0.0)
    days = np.concatenate([np.asarray(b.column(c).view(pa.int32())) for c in ("d32_a", "d32_b")] + [R._exponent_uniform(rng, 20000, 32)]).astype(np.int64)
    ms = np.concatenate([np.asarray(b.column(c).view(pa.int64())) for c in ("d64_a", "d64_b", "ts_a", "ts_b")] + [R._exponent_uniform(rng, 20000, 64)])
    ms = ms[ms != R.I64_MIN]
    for unit, vals, tn in (("D", days, "d32"), ("ms", ms, "ts")):
        t = vals.astype("datetime64[%s]" % unit)
        months = t.astype("datetime64[M]").astype(np.int64)
        dom = (t.astype("datetime64[D]") - t.astype("datetime64[M]").astype("datetime64[D]")).astype(np.int64) + 1
        want = list(zip((1970 + months // 12).tolist(), (months % 12 + 1).tolist(), dom.tolist()))
        got = [(R.extract("Year", tn, v), R.extract("Month", tn, v), R.extract("Day", tn, v)) for v in vals.tolist()]
        assert got == want, unit
        assert {abs(y).bit_length() for y, _, _ in got} >= set(range(8, 23 if unit == "D" else 29)), "a magnitude of year never occurs"
        assert min(y for y, _, _ in got) < -(5 if unit == "D" else 250) * 10 ** 6 and max(y for y, _, _ in got) > (5 if unit == "D" else 250) * 10 ** 6


def test_month_addition_matches_dateutil_at_any_shift_of_400_years():
    rng = np.random.default_rng(6)
    epoch = dt.datetime(1970, 1, 1)
    for _ in range(3000):
        start = dt.datetime(2000, 1, 1) + dt.timedelta(milliseconds=int(rng.integers(0, R.CYCLE * R.MS)))
        if rng.integers(0, 3) == 0:       # month ends, where the day is clamped
            start = start.replace(day=R.last_dom(start.year, start.month))
        k = int(rng.integers(-2400, 2401))
        want = (start + relativedelta(months=k) - epoch) // dt.timedelta(milliseconds=1)
        v = (start - epoch) // dt.timedelta(milliseconds=1)
        shift = int(R._exponent_uniform(rng, 1, 20)[0]) * R.CYCLE * R.MS
        assert R.add_months(v, k) == want and R.add_months(v + shift, k) == want + shift, (start, k, shift)
    assert R.add_months(R.I64_MAX, 1) is None and R.add_months(R.I64_MIN, 0) is None and R.add_months(R.I64_MIN + R.MS, 0) == R.I64_MIN + R.MS


def test_month_count_matches_the_search_with_dateutil_at_any_shift_of_400_years():
    """The month-count rule against test_registry_tail_r3's _python_months (the largest k with start + k months <= end,
    searched with dateutil), on its own pairs and on the same pairs moved by whole 400-year cycles."""
    import test_registry_tail_r3 as T
    rng = np.random.default_rng(7)
    s, e = T._timestamps(rng, 1500)
    compared = 0
    for a, z in zip(s.tolist(), e.tolist()):
        want = T._python_months(a, z)
        if want is None:
            continue
        shift = int(R._exponent_uniform(rng, 1, 20)[0]) * R.CYCLE * R.MS
        assert R.months_between(a, z) == want and R.months_between(a + shift, z + shift) == want, (a, z, shift)
        compared += 1
    assert compared > 1400


def test_rules_at_their_corners():
    day = R.day_of
    assert [R.civil(d)[:3] for d in (day(0, 2, 29), day(0, 3, 1) - 1, day(1, 1, 1) - 1, day(-400, 3, 1) - 1, day(-100, 3, 1) - 1)] == \
           [(0, 2, 29), (0, 2, 29), (0, 12, 31), (-400, 2, 29), (-100, 2, 28)]
    assert day(1970, 1, 1) == 0 and day(0, 3, 1) == -719468 and day(1582, 10, 15) == -141427
    # Decade truncates (year -5 is in decade 0, as year 5 is); Century and Millennium count from year 1
    assert [R.extract(p, "d32", day(y, 6, 1)) for p, y in (("Decade", -5), ("Decade", -15), ("Century", 0), ("Century", 1), ("Century", -100),
                                                          ("Millennium", 2000), ("Millennium", 2001), ("Millennium", -1))] == [0, -1, 1, 1, 0, 2, 3, 1]
    # fixed units toward zero: 1 ms before the epoch truncates up to it; the calendar units floor, but (year - 1) / N is
    # C's division, so the years -98..0 belong to the century that "starts" in year 1
    assert R.date_trunc("Second", -1) == 0 and R.date_trunc("Day", -R.MS - 1) == -R.MS and R.date_trunc("Month", -1) == day(1969, 12, 1) * R.MS
    assert R.date_trunc("Week", day(2021, 1, 3) * R.MS + 5) == day(2020, 12, 28) * R.MS
    assert R.date_trunc("Decade", day(2020, 5, 5) * R.MS) == day(2011, 1, 1) * R.MS and R.date_trunc("Century", day(-5, 5, 5) * R.MS) == day(1, 1, 1) * R.MS
    assert R.date_trunc("Last", day(1900, 2, 3) * R.MS + 7) == day(1900, 2, 28) * R.MS and R.date_trunc("Year", R.I64_MIN) is None
    assert R.timestampdiff("Second", 0, -1999) == -1 and R.timestampdiff("Day", R.I64_MIN, R.I64_MAX) is None
    assert R.timestampdiff("Second", -(1 << 62), (1 << 62) - 1) == R.wrap(((1 << 63) - 1) // 1000, 32) and R.timestampdiff("Second", -(1 << 62), 1 << 62) is None
    assert R.datediff("ts", 0, -1) == 1 and R.datediff("d32", (1 << 31) - 1, -(1 << 31)) == -1
    assert R.cast("castTIME", "ts", -1) == R.MS - 1 and R.cast("castDATE32", "d64", R.I64_MIN) == R.wrap(R.I64_MIN // R.MS, 32)
    assert R.seconds_to_millis("i64", (1 << 63) - 1) == -1000 and R.seconds_to_millis("f64", np.float64("nan")) == 0
    assert R.seconds_to_millis("f32", np.float32(3.4e38)) == R.I64_MAX and R.seconds_to_millis("f64", np.float64(-1.9995)) == -1999
    # float32 seconds are multiplied in float32: 16777217 s does not exist there, and 0.001f * 1000f rounds to 1
    assert R.seconds_to_millis("f32", np.float32(16777217.0)) == 16777216000 and R.seconds_to_millis("f32", np.float32(0.001)) == 1
    for s, e, months, quarters, years in R.MONTH_COUNT_PAIRS:
        assert [R.timestampdiff(u, s, e) for u in ("Month", "Quarter", "Year")] == [months, quarters, years]
        assert [R.timestampdiff(u, e, s) for u in ("Quarter", "Year")] == [-quarters, -years]


def test_generators_cover_the_edges_and_every_magnitude():
    k = R.CROSS * R.CROSS
    assert R.ROWS - k - len(R.MONTH_COUNT_PAIRS) >= 3000, "fewer than 3000 random rows"
    for nulls in NULLS:
        b = R.batch(nulls)
        assert b.num_rows == R.ROWS and b.schema == R.SCHEMA
        for name, _ in R.COLUMNS:
            share = b.column(name).null_count / R.ROWS
            assert share == 0 if nulls == 0 else 0.05 < share < 0.15, name
    b = R.batch(0.0)
    for pair, edges, w in (("d32", R.day_edges(), 32), ("d64", R.ms_edges(), 64), ("ts", R.ms_edges(), 64)):
        a, z = (np.asarray(b.column(pair + c).view(R.STORAGE[pair])).astype(np.int64) for c in ("_a", "_b"))
        assert a[:k].tolist() == np.repeat(edges[:R.CROSS], R.CROSS).tolist() and z[:k].tolist() == np.tile(edges[:R.CROSS], R.CROSS).tolist()
        assert set(edges) <= set(a.tolist()) | set(z.tolist()), "an edge value is in neither column"
        for col in (a, z):
            bits = {abs(v).bit_length() for v in col[k:].tolist()}
            assert set(range(1, w)) <= bits, "a magnitude never occurs in " + pair
            assert 0.3 < (col[k:] < 0).mean() < 0.7
        if w == 64:
            assert [(a[k + j], z[k + j]) for j in range(2)] == [(s, e) for s, e, *_ in R.MONTH_COUNT_PAIRS]
            gap = np.abs(a[k:].astype(object) - z[k:].astype(object))
            assert (gap < 1 << 41).mean() > 0.3 and (gap > 1 << 50).mean() > 0.1, "close pairs at far dates, and far pairs"
    for name, w in (("c_i32", 32), ("c_i64", 32), ("c_n64", 28)):
        c = np.asarray(b.column(name)).astype(np.int64)
        assert set(range(1, w)) <= {abs(v).bit_length() for v in c.tolist()} and np.abs(c).max() <= 1 << (w - 1)
    assert set(R.COUNT_EDGES) <= set(np.asarray(b.column("c_i64"))[:R.CROSS].tolist())
    t = np.asarray(b.column("t32_a").view(pa.int32()))
    assert t.min() == 0 and t.max() == R.MS - 1


def test_every_temporal_signature_of_the_interpreter_table_has_a_full_range_case():
    """gdv_tier0_fns.inc lists one line per device-library symbol: every date / time one of them (extract*, date_trunc_*,
    extractWeek, last_day, the adds, the diffs, the fixed-width casts, to_timestamp / to_time) must occur in a family, so
    a signature added later without a full-range case is noticed."""
    with open(FNS_INC) as f:
        symbols = re.findall(r"^GDV_T0_F[12]\((\w+),", f.read(), re.M)
    temporal = [s for s in symbols if re.match(r"extract|date_trunc_|last_day|timestampadd|timestampdiff|date_add|date_sub|datediff|to_time|"
                                                 r"castDATE|castTIME|castBIGINT_(date64|timestamp)", s)]
    assert len(temporal) >= 129, len(temporal)
    covered = {R.symbol_of(sp) for family in R.FAMILIES for sp in R.family_specs(family)}
    assert not sorted(set(temporal) - covered), "no full-range case for %s" % sorted(set(temporal) - covered)
    assert covered <= set(symbols), "a case names no symbol of the table: %s" % sorted(covered - set(symbols))


@pytest.mark.parametrize("nulls", NULLS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_no_expression_leaves_out_more_than_a_tenth_of_its_valid_rows(family, nulls):
    b = R.batch(nulls)
    for sp, (want, left_out) in zip(R.family_specs(family), R.expected_pairs(family, nulls)):
        valid = np.logical_and.reduce([np.asarray(b.column(a).is_valid()) for a in sp["args"] if isinstance(a, str)])
        assert not (left_out & ~valid).any()
        share = left_out.sum() / valid.sum()
        assert share <= 0.10, "%s leaves out %.1f %%" % (sp["label"], 100 * share)
        if sp["fn"].startswith(("extract", "weekofyear", "to_", "datediff", "date_diff", "timestampdiffMonth", "timestampdiffQuarter", "timestampdiffYear")):
            assert not left_out.any(), sp["label"]


# ---- the oracle and the host build of the device library against the reference -----------------------------------------
@pytest.mark.parametrize("nulls", NULLS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_oracle_matches_the_reference_on_full_range_dates_and_times(family, nulls):
    batch = R.batch(nulls)
    specs = R.family_specs(family)
    got = oracle.project(R.build_expressions(gandiva, specs), batch)
    for sp, g, (want, left_out) in zip(specs, got, R.expected_pairs(family, nulls)):
        assert_bit_exact_where(g, want, ~left_out, "oracle %s nulls=%s" % (sp["label"], nulls))


def _host_result(hostlib, sp, batch, left_out):
    """The spec's rows through the device library's own function compiled for the host; rows that are left out (and null
    rows) are computed on 0, so no signed overflow is executed."""
    entry, k, op = sp["host"]
    n = batch.num_rows
    args = []
    for a in sp["args"]:
        dtype = np.dtype(R.STORAGE[R.arg_type(a)].to_pandas_dtype())
        v = np.asarray(batch.column(a).view(R.STORAGE[R.arg_type(a)]).fill_null(0)).copy() if isinstance(a, str) else np.full(n, a["lit"], dtype=dtype)
        v[left_out] = 0
        args.append(np.ascontiguousarray(v))
    ptr = [a.ctypes.data_as(C.c_void_p) for a in args]
    out = np.zeros(n, dtype=np.dtype(R.STORAGE[sp["ret"]].to_pandas_dtype()))
    o = out.ctypes.data_as(C.c_void_p)
    if entry == "unary":
        hostlib.host_temporal_unary(k, op, ptr[0], o, C.c_long(n))
    elif entry == "trunc":
        hostlib.host_temporal_trunc(k, op, ptr[0], o, C.c_long(n))
    elif entry == "add":          # timestampadd*(count, v); date_add / date_sub(v, count)
        count, v = (ptr[0], ptr[1]) if op < 8 else (ptr[1], ptr[0])
        hostlib.host_temporal_add(k, op, count, v, o, C.c_long(n))
    elif entry == "diff":
        hostlib.host_temporal_diff(k, op, ptr[0], ptr[1], o, C.c_long(n))
    elif entry == "cast":
        hostlib.host_temporal_cast(k, ptr[0], o, C.c_long(n))
    else:
        ts, tm = np.zeros(n, np.int64), np.zeros(n, np.int32)
        hostlib.host_to_timestamp(k, ptr[0], C.c_long(n), ts.ctypes.data_as(C.c_void_p), tm.ctypes.data_as(C.c_void_p))
        out = tm if op else ts
    return out


@pytest.mark.parametrize("nulls", NULLS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_host_build_of_the_device_library_matches_the_reference(hostlib, family, nulls):
    """Every expression, per row through the device library's own function compiled for the host."""
    batch = R.batch(nulls)
    for sp, (want, left_out) in zip(R.family_specs(family), R.expected_pairs(family, nulls)):
        assert sp["host"] is not None, sp["label"]
        raw = _host_result(hostlib, sp, batch, left_out)
        got = pa.array(raw, R.STORAGE[sp["ret"]], mask=np.asarray(want.is_null())).view(R.TYPES[sp["ret"]])
        assert_bit_exact_where(got, want, ~left_out, "host build %s nulls=%s" % (sp["label"], nulls))


def test_quarter_and_year_divide_the_exact_month_count_before_narrowing(hostlib):
    """timestampdiffQuarter / Year of instants more than 2^31 months apart: the month count does not fit int32, the
    quarters and years do.  The device library once divided the count after narrowing it (gdv_months_between returned
    int32) and gave 1092259339 -> -339396426 quarters for the first pair; it carries the count in 64 bits now."""
    s = np.array([p[0] for p in R.MONTH_COUNT_PAIRS] + [p[1] for p in R.MONTH_COUNT_PAIRS], dtype=np.int64)
    e = np.array([p[1] for p in R.MONTH_COUNT_PAIRS] + [p[0] for p in R.MONTH_COUNT_PAIRS], dtype=np.int64)
    want = {"Month": [-1018189278, -1984679367, 1018189278, 1984679367], "Quarter": [1092259339, 770095976, -1092259339, -770095976],
            "Year": [273064834, 192523994, -273064834, -192523994]}
    batch = pa.RecordBatch.from_arrays([pa.array(s).view(pa.timestamp("ms")), pa.array(e).view(pa.timestamp("ms"))], names=["t0", "t1"])
    b = gandiva.TreeExprBuilder()
    for unit, (name, expected) in enumerate(want.items()):
        assert [R.timestampdiff(name, x, y) for x, y in zip(s.tolist(), e.tolist())] == expected, "reference " + name
        out = np.zeros(len(s), dtype=np.int32)
        hostlib.host_months_between(s.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), C.c_long(len(s)), unit, out.ctypes.data_as(C.c_void_p))
        assert out.tolist() == expected, "device library (host build) timestampdiff" + name
        node = b.make_function("timestampdiff" + name, [b.make_field(batch.schema.field(0)), b.make_field(batch.schema.field(1))], pa.int32())
        assert oracle.project_one(node, pa.int32(), batch).to_pylist() == expected, "oracle timestampdiff" + name
