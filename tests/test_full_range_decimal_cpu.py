"""The decimal128 core on full-range operands, without a GPU: the independent reference (tests/decimal_reference.py) against
Python's `decimal` module, pyarrow.compute and Decimal.quantize; the oracle and the host build of the device library
against the reference, bit for bit, on the 4099-row batches that tests/test_full_range_decimal.py runs on the GPU; the
device functions once more as a stand-alone program under AddressSanitizer / UBSan (tests/cxx/decimal_core_check.cc).
The batches' own conditions are asserted here — exact ties of the half-away rounding and their neighbours one unit
either side, the share of overflow -> 0 rows, value-equal rows across scales, results at +-(10^38 - 1) and one past —
so that a batch that degenerated fails here and does not pass silently on the GPU."""
import ctypes as C
import decimal
import os
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import gandiva_amd as gandiva
from oracle import oracle
import decimal_reference as R
from full_range_child import NULLS
from helpers import assert_bit_exact, validity_np
from test_device_lib_on_host import hostlib  # noqa: F401  (the fixture that builds tests/host_devlib)

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "gandiva_amd", "csrc")
CTX = decimal.Context(prec=100, rounding=decimal.ROUND_HALF_UP)
OPS = ("add", "subtract", "multiply", "divide", "mod")


def _operands(k, op):
    x, y, _ = R.pair_rows(k)
    return x, ([v if v != 0 else 1 for v in y] if op in ("divide", "mod") else y)


# ------------------------------------------------------------------ 1. the batches' conditions

@pytest.mark.parametrize("k", range(R.NPAIRS))
def test_batches_hold_ties_neighbours_boundaries_and_few_overflows(k):
    """Per binary expression: at most two thirds of the rows overflow; where the rounding drops digits, at least 20 exact
    ties, 20 rows one unit of an operand below a tie and 20 one unit above.  Per cross-scale pair at least 50 value-equal rows."""
    ta, tb = R.PAIRS[k]
    x, y, kcol = R.pair_rows(k)
    assert len(x) == len(y) == len(kcol) == R.ROWS
    assert all(abs(v) < 10 ** ta[0] for v in x) and all(abs(v) < 10 ** tb[0] for v in y), "a row does not fit its type"
    ax, ay = R.anchors(ta[0]), R.anchors(tb[0])
    assert x[:len(ax) * len(ay)] == [u for u in ax for _ in ay] and y[:len(ax) * len(ay)] == ay * len(ax), "the anchor cross product does not lead"
    assert {0, 1, -1, 10 ** ta[0] - 1, 1 - 10 ** ta[0]} <= set(ax) and (ta[0] < 20 or {2 ** 64 - 1, 2 ** 64, 2 ** 64 + 1, 2 ** 63} <= set(ax))
    assert kcol[:9] == [0, ta[1], ta[1] + 1, -1, -37, -38, -39, R.INT32_MIN, R.INT32_MAX]
    for op in OPS[:4]:
        xs, ys = _operands(k, op)
        rounded = [R.half_away(*R.exact_ratio(op, ta, tb, u, v)) for u, v in zip(xs, ys)]
        share = sum(abs(r) >= R.LIMIT for r in rounded) / R.ROWS
        print("%s %s %s: %.0f %% overflow rows" % (op, ta, tb, 100 * share))
        assert share <= 2 / 3, "%s %s %s: %.0f %% of the rows overflow" % (op, ta, tb, 100 * share)
        if R.exact_ratio(op, ta, tb, 1, 1)[1] == 1 and op != "divide":
            continue                                   # nothing is dropped: no rounding
        tie = [R.is_tie(op, ta, tb, u, v) for u, v in zip(xs, ys)]
        below = sum(not t and (R.is_tie(op, ta, tb, u + 1, v) or R.is_tie(op, ta, tb, u, v + 1)) for t, u, v in zip(tie, xs, ys))
        above = sum(not t and (R.is_tie(op, ta, tb, u - 1, v) or R.is_tie(op, ta, tb, u, v - 1)) for t, u, v in zip(tie, xs, ys))
        assert sum(tie) >= 20 and below >= 20 and above >= 20, "%s %s %s: %d ties, %d / %d neighbours" % (op, ta, tb, sum(tie), below, above)
    e = R.result_type("divide", ta, tb)[1] - ta[1] + tb[1]
    if e > 38:      # divide forms |x| * 10^e in 256 bits: rows where it does not fit and its low 256 bits alone would pass for a quotient
        xs, ys = _operands(k, "divide")
        n = sum(abs(u) * 10 ** e >= 2 ** 256 and abs(u) * 10 ** e % 2 ** 256 // abs(v) < R.LIMIT for u, v in zip(xs, ys))
        assert n >= 20, "%d rows on which a carry out of 256 bits would go unnoticed" % n
    if ta[1] != tb[1]:
        assert sum(R.compare(ta, tb, u, v) == 0 for u, v in zip(x, y)) >= 50, "fewer than 50 value-equal rows across the scales"
    # the unary functions' ties: as many as the type admits, 20 at the most asked for
    for e in R.unary_drops(ta):
        admits = 2 * max(0, (10 ** ta[0] - 5 * 10 ** (e - 1) - 2) // 10 ** e + 1)
        for d in (-1, 0, 1):
            n = sum(abs(v) % 10 ** e == 5 * 10 ** (e - 1) + d for v in x)
            with_k = sum(abs(v) % 10 ** e == 5 * 10 ** (e - 1) + d and kk == ta[1] - e for v, kk in zip(x, kcol))
            assert n >= min(20, admits) and with_k >= min(20, admits), "%s drops %d digits: %d rows at tie%+d, %d with that k" % (ta, e, n, d, with_k)


def test_results_at_the_largest_value_and_one_past_it_occur():
    """+-(10^38 - 1) as a result and an exact +-10^38 (-> 0), for every operator and type pair that can reach them."""
    reach = {"add": (0, 1, 3, 4), "subtract": (0, 1, 3, 4), "multiply": (0, 1, 3, 4, 10, 12), "divide": (0, 2, 10)}
    for op, pairs in reach.items():
        for k in pairs:
            ta, tb = R.PAIRS[k]
            xs, ys = _operands(k, op)
            r = [R.half_away(*R.exact_ratio(op, ta, tb, u, v)) for u, v in zip(xs, ys)]
            for want in (R.LIMIT - 1, 1 - R.LIMIT, R.LIMIT, -R.LIMIT):
                assert want in r, "%s %s %s never gives %d" % (op, ta, tb, want)


# ------------------------------------------------------------------ 2. the reference against other engines

def _dec(v, scale):
    return decimal.Decimal(v).scaleb(-scale, CTX)


@pytest.mark.parametrize("k", range(R.NPAIRS))
def test_reference_matches_python_decimal_on_the_five_operators(k):
    ta, tb = R.PAIRS[k]
    for op in OPS:
        xs, ys = _operands(k, op)
        _, os_ = R.result_type(op, ta, tb)
        q = decimal.Decimal(1).scaleb(-os_)
        for u, v in zip(xs, ys):
            a, b = _dec(u, ta[1]), _dec(v, tb[1])
            if op == "divide":                         # CTX.divide rounds to 100 digits first: widen until the quotient is exact or long enough
                w = decimal.Context(prec=200, rounding=decimal.ROUND_HALF_UP).divide(a, b)
            else:
                w = {"add": CTX.add, "subtract": CTX.subtract, "multiply": CTX.multiply, "mod": CTX.remainder}[op](a, b)
            w = w.quantize(q, rounding=decimal.ROUND_HALF_UP, context=decimal.Context(prec=200))
            w = int(w.scaleb(os_, decimal.Context(prec=200)))
            assert R.binary(op, ta, tb, u, v) == (0 if abs(w) >= R.LIMIT else w), (op, ta, tb, u, v)


@pytest.mark.parametrize("k", range(R.NPAIRS))
def test_reference_matches_pyarrow_compute_where_no_scale_is_cut(k):
    ta, tb = R.PAIRS[k]
    x, y, _ = R.pair_rows(k)
    a, b = R.dec_array(x, ta), R.dec_array(y, tb)
    ran = 0
    for op, fn in (("add", pc.add), ("subtract", pc.subtract), ("multiply", pc.multiply)):
        p, s = R.result_type(op, ta, tb)
        exact_scale = max(ta[1], tb[1]) if op != "multiply" else ta[1] + tb[1]
        exact_precision = (max(ta[0] - ta[1], tb[0] - tb[1]) + exact_scale + 1) if op != "multiply" else ta[0] + tb[0] + 1
        if s != exact_scale or exact_precision > 38:
            continue                                   # libarrow refuses precisions above 38 and never cuts a scale
        got = fn(a, b)
        assert (got.type.precision, got.type.scale) == (p, s)
        assert R.dec_ints(got) == [R.binary(op, ta, tb, u, v) for u, v in zip(x, y)], (op, ta, tb)
        ran += 1
    assert ran == {5: 3, 6: 3, 7: 3, 8: 2, 9: 2}.get(k, 0)


ROUNDINGS = {"round": decimal.ROUND_HALF_UP, "truncate": decimal.ROUND_DOWN, "ceil": decimal.ROUND_CEILING, "floor": decimal.ROUND_FLOOR}


@pytest.mark.parametrize("k", range(R.NPAIRS))
def test_reference_rounding_family_matches_decimal_quantize(k):
    ta, _ = R.PAIRS[k]
    x, _, kcol = R.pair_rows(k)
    big = decimal.Context(prec=200)
    to_int, same, lower = R.rounding_result_types(ta)
    for fn, with_k, rt in [(f, False, to_int) for f in ROUNDINGS] + [(f, True, t) for f in ("round", "truncate") for t in (same, lower)]:
        for u, kk in list(zip(x, kcol))[::2]:
            kk = kk if with_k else 0
            v = _dec(u, ta[1])
            if kk < -38:
                r = decimal.Decimal(0)
            else:
                r = v if kk >= ta[1] else v.quantize(decimal.Decimal(1).scaleb(-kk, big), rounding=ROUNDINGS[fn], context=big)
            r = int(r.quantize(decimal.Decimal(1).scaleb(-rt[1], big), rounding=decimal.ROUND_HALF_UP, context=big).scaleb(rt[1], big))
            assert R.round_to(fn, u, ta[1], kk, *rt) == (0 if abs(r) >= 10 ** rt[0] else r), (fn, ta, u, kk, rt)


def test_reference_casts_by_hand():
    assert R.rescale(15, 1, 5, 0) == 2 and R.rescale(-15, 1, 5, 0) == -2 and R.rescale(14, 1, 5, 0) == 1
    assert R.rescale(99999, 0, 5, 0) == 99999 and R.rescale(999995, 1, 5, 0) == 0 and R.rescale(1, 0, 18, 18) == 0
    assert R.wrap64(R.half_away(2 ** 63 * 10, 10)) == -2 ** 63 and R.wrap64(2 ** 64 + 5) == 5 and R.wrap64(-(2 ** 63) - 1) == 2 ** 63 - 1
    assert R.to_float8(2 ** 64 + 2 ** 11 + 1, 0) == 2.0 ** 64 + 2.0 ** 12          # above the tie: up (hi and lo converted apart round down)
    assert R.to_float8(123, 2) == 1.23 and R.to_float8(-5, 1) == -0.5
    assert R.ulps_from_correct(1.23, 123, 2) == 0 and R.ulps_from_correct(np.nextafter(1.23, 2.0), 123, 2) == 1 and R.ulps_from_correct(-0.0, 0, 5) == 0
    assert R.round_to("round", 15, 1, -38, 38, 0) == 0 and R.round_to("ceil", 1, 38, 0, 1, 0) == 1 and R.round_to("floor", -1, 38, 0, 1, 0) == -1
    assert R.round_to("round", 5 * 10 ** 37, 0, -38, 38, 0) == 0                   # rounds to 10^38, which no precision holds
    assert R.round_to("round", 125, 2, 1, 38, 2) == 130 and R.round_to("truncate", -125, 2, 1, 38, 0) == -1


def test_cast_float8_distance_to_the_correctly_rounded_quotient_per_scale():
    """float(x) / p against the exact quotient: a recorded measurement (profiles/full_range_decimal.txt), not a tolerance —
    the comparisons with this formula are bit for bit.  p is exactly 10^scale up to scale 22, so there the two roundings
    stay within 1 unit; printed for every scale of the batches."""
    worst = {}
    for k, (ta, _) in enumerate(R.PAIRS):
        x, _, _ = R.pair_rows(k)
        worst[ta[1]] = max(worst.get(ta[1], 0), max(R.ulps_from_correct(R.to_float8(v, ta[1]), v, ta[1]) for v in x))
    print("castFLOAT8 max ulp from the correctly rounded quotient, per scale: %s" % sorted(worst.items()))
    assert all(w <= 1 for s, w in worst.items() if s <= 22), worst


# ------------------------------------------------------------------ 3. the oracle against the reference

@pytest.mark.parametrize("nulls", NULLS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_oracle_matches_the_reference_on_full_range_operands(family, nulls):
    batch = R.batch(nulls)
    specs = R.family_specs(family)
    got = oracle.project(R.build_expressions(gandiva, specs), batch)
    for sp, g, w in zip(specs, got, R.expected_columns(family, nulls)):
        assert_bit_exact(g, w, "oracle %s nulls=%s" % (sp["label"], nulls))


def test_oracle_filter_matches_the_reference_across_scales():
    batch = R.batch(0.1)
    b = gandiva.TreeExprBuilder()
    specs = [sp for sp in R.extra_specs() if sp["fn"] == "less_than"]
    assert len(specs) >= 5
    for sp, e in zip(specs, R.build_expressions(gandiva, specs)):
        want = np.flatnonzero(np.asarray(R.expected_of(sp, batch).fill_null(False)))
        got = oracle.filter_indices(b.make_condition(e.root()), batch, "int32")
        assert np.array_equal(np.asarray(got), want), sp["label"]


# ------------------------------------------------------------------ 4. the host build of the device functions

def _raw(arr):
    return np.frombuffer(arr.buffers()[1], dtype=np.uint64)[2 * arr.offset: 2 * (arr.offset + len(arr))].copy()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _host_result(lib, sp, batch):
    """The spec through the device library's own function compiled for the host, as (values, type name); None: no entry."""
    fn, n = sp["fn"], R.ROWS
    if fn in ("if", "greatest", "least"):
        return None
    a0 = sp["args"][0]
    tx = R.COLUMN_TYPE[a0]
    out = np.zeros(2 * n, dtype=np.uint64)
    if tx[0] != "d":                                       # castDECIMAL of an integer column
        v = np.ascontiguousarray(np.asarray(batch.column(a0).fill_null(0)).astype(np.int64))
        lib.host_decimal_from_int64(_p(v), *R._pair(sp["ret"]), _p(out), C.c_long(n))
        return out
    (xp, xs), x = R._pair(tx), _raw(batch.column(a0))
    if fn in OPS or fn in R.CMP:
        (yp, ys), y = R._pair(R.COLUMN_TYPE[sp["args"][1]]), _raw(batch.column(sp["args"][1]))
        if fn in OPS:
            err = lib.host_decimal_binary(OPS.index(fn), _p(x), xp, xs, _p(y), yp, ys, *R._pair(sp["ret"]), _p(out), C.c_long(n))
            assert err == 0
            return out
        c = np.zeros(n, dtype=np.int8)
        lib.host_decimal_compare(_p(x), xp, xs, _p(y), yp, ys, _p(c), C.c_long(n))
        return np.array([R.CMP[fn](int(v)) for v in c])
    if fn == "castDECIMAL":
        lib.host_decimal_cast(_p(x), xp, xs, *R._pair(sp["ret"]), _p(out), C.c_long(n))
    elif fn == "castBIGINT":
        out = np.zeros(n, dtype=np.int64)
        lib.host_decimal_to_int64(_p(x), xp, xs, _p(out), C.c_long(n))
    elif fn in ("castFLOAT8", "abs", "negative"):
        out = np.zeros(n, dtype=np.float64) if fn == "castFLOAT8" else out
        lib.host_decimal_unary(("castFLOAT8", "abs", "negative").index(fn), _p(x), xp, xs, _p(out), C.c_long(n))
    elif fn == "castVARCHAR":
        off, data = np.zeros(n + 1, dtype=np.int32), np.zeros(n * 48 + 64, dtype=np.uint8)
        err = lib.host_cast_varchar_decimal(_p(x), xp, xs, C.c_long(n), C.c_longlong(sp["args"][1]["lit"]), _p(off), _p(data))
        assert err == 0
        raw = data.tobytes()
        return [raw[off[i]:off[i + 1]].decode() for i in range(n)]
    else:
        kcol = None
        if len(sp["args"]) == 2:
            kcol = np.ascontiguousarray(np.asarray(batch.column(sp["args"][1]).fill_null(0)).astype(np.int32))
        lib.host_decimal_round(("round", "truncate", "ceil", "floor").index(fn), _p(x), xp, xs, None if kcol is None else _p(kcol),
                               *R._pair(sp["ret"]), _p(out), C.c_long(n))
    return out


@pytest.mark.parametrize("family", R.FAMILIES)
def test_host_build_of_the_device_library_matches_the_reference(hostlib, family):
    """Every expression with a host entry point, per row through the device library's own function compiled for the host
    (the plain loop computes under nulls too; the comparison takes the expression's valid rows)."""
    hostlib.host_decimal_round.restype = None
    ran = 0
    for nulls in NULLS:
        batch = R.batch(nulls)
        for sp, want in zip(R.family_specs(family), R.expected_columns(family, nulls)):
            raw = _host_result(hostlib, sp, batch)
            if raw is None:
                continue
            valid = validity_np(want)
            if sp["ret"][0] == "d":
                got = pa.Array.from_buffers(want.type, R.ROWS, [want.buffers()[0], pa.py_buffer(raw.tobytes())], null_count=want.null_count)
            elif sp["ret"] == "utf8":
                got = pa.array([v if ok else None for v, ok in zip(raw, valid.tolist())], pa.string())
            else:
                got = pa.array(raw, want.type, mask=~valid)
            assert_bit_exact(got, want, "host build %s nulls=%s" % (sp["label"], nulls))
            ran += 1
    assert ran >= 2 * R.NPAIRS


# ------------------------------------------------------------------ 5. under sanitizers, as a child process

@pytest.mark.parametrize("name,extra", [("plain", []), ("asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"])])
def test_decimal_core_has_no_signed_overflow_on_the_anchor_cross_products(tmp_path, name, extra):
    """tests/cxx/decimal_core_check.cc over the anchor cross product of every type pair: a stand-alone program with its
    own main, nothing preloaded; its operator results and compares are held to the reference."""
    exe = str(tmp_path / ("decimal_core_check_" + name))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-unused-function", "-Wno-unused-variable", "-Wno-attributes"] +
                          extra + ["-I", CSRC, os.path.join(HERE, "cxx", "decimal_core_check.cc"), "-o", exe])
    rows, want = [], []
    for k, (ta, tb) in enumerate(R.PAIRS):
        types = " ".join("%d %d" % R.result_type(op, ta, tb) for op in OPS)
        for x in R.anchors(ta[0]):
            for y in R.anchors(tb[0]):
                rows.append("%d %d %d %d %s %d %d" % (ta + tb + (types, x, y)))
                want.append(" ".join(str(R.binary(op, ta, tb, x, y if y != 0 or op in OPS[:3] else 1)) for op in OPS) + " %d" % R.compare(ta, tb, x, y))
    (tmp_path / "rows.txt").write_text("\n".join(rows) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe, str(tmp_path / "rows.txt"), str(tmp_path / "out.txt")], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, f"exit {run.returncode}\n{run.stdout}\n{run.stderr}"
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    assert "decimal_core_check: ok (%d rows" % len(rows) in run.stdout
    got = (tmp_path / "out.txt").read_text().splitlines()
    bad = [(r, g, w) for r, g, w in zip(rows, got, want) if g != w]
    assert len(got) == len(want) and not bad, "%d rows differ, first %s" % (len(bad), bad[:3])
