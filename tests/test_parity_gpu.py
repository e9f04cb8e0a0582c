"""HIP path vs CPU oracle on identical seeded batches (bit-exact), through the C ABI.

Covers the hot path of SURVEY.md §8a: fused projection with validity-word merging, if/else
and three-valued AND/OR (per-lane validity), bool outputs (ballot-packed), array offsets
(misaligned bitmaps), ragged lengths around the 64-row word and the workgroup tile, null
densities 0/10/50/100 %, IEEE specials, integer wrap, filter -> selection vector for all
three index widths, selection-vector-driven projection, and execution errors.
"""
import os
import numpy as np
import pyarrow as pa
import pytest

import gandiva_amd as gandiva
from gandiva_amd import workloads as W
from oracle import oracle
from helpers import assert_bit_exact, assert_within_ulp, random_array

pytestmark = pytest.mark.gpu

LENGTHS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099, 100003]


def _batch(rng, types, n, null_fraction, names=None):
    names = names or [chr(ord('a') + i) for i in range(len(types))]
    cols = [random_array(rng, t, n, null_fraction) for t in types]
    return pa.RecordBatch.from_arrays(cols, names=names)


def _check_project(exprs, batch, sel_mode="NONE"):
    proj = gandiva.make_projector(batch.schema, exprs, pa.default_memory_pool(), sel_mode)
    got = proj.evaluate(batch)
    want = oracle.project(exprs, batch)
    for i, (g, w) in enumerate(zip(got, want)):
        assert_bit_exact(g, w, f"expr {i}: {exprs[i]}")
    return got


# ------------------------------------------------------------------ BASELINE configs

@pytest.mark.parametrize("n", [1 << 10, (1 << 16) + 13])
def test_c1_int32_plumbing(n):
    _check_project(W.c1_expressions(), W.c1_batch(n))


@pytest.mark.parametrize("n", LENGTHS + [1 << 20])
def test_c2_ten_float64_expressions(n):
    _check_project(W.c2_expressions(), W.c2_batch(n))


@pytest.mark.parametrize("n", LENGTHS + [(1 << 20) + 77])
@pytest.mark.parametrize("nulls", [0.0, 0.1])
def test_c3_filter(n, nulls):
    batch = W.c3_batch(n, nulls)
    cond = W.c3_condition()
    flt = gandiva.make_filter(batch.schema, cond)
    for dtype in ("int32", "int64"):
        got = flt.evaluate(batch, pa.default_memory_pool(), dtype).to_array()
        want = oracle.filter_indices(cond, batch, dtype)
        assert got.equals(want), f"{dtype}: {len(got)} vs {len(want)} slots"
    if n <= 65536:
        got = flt.evaluate(batch, pa.default_memory_pool(), "int16").to_array()
        assert got.equals(oracle.filter_indices(cond, batch, "int16"))


# ------------------------------------------------------------------ arithmetic over all types

NUMERIC = [pa.int8(), pa.int16(), pa.int32(), pa.int64(), pa.uint8(), pa.uint16(), pa.uint32(),
           pa.uint64(), pa.float32(), pa.float64()]


@pytest.mark.parametrize("t", NUMERIC, ids=str)
@pytest.mark.parametrize("nulls", [0.0, 0.1, 0.5, 1.0])
def test_arithmetic_and_compare(t, nulls):
    rng = np.random.default_rng(hash((str(t), nulls)) & 0xffff)
    n = 2999
    batch = _batch(rng, [t, t], n, nulls)
    b = gandiva.TreeExprBuilder()
    fa, fb = b.make_field(batch.schema.field(0)), b.make_field(batch.schema.field(1))
    exprs = []
    for name in ("add", "subtract", "multiply"):
        exprs.append(b.make_expression(b.make_function(name, [fa, fb], t), pa.field(name, t)))
    for name in ("equal", "not_equal", "less_than", "less_than_or_equal_to", "greater_than",
                 "greater_than_or_equal_to"):
        exprs.append(b.make_expression(b.make_function(name, [fa, fb], pa.bool_()),
                                       pa.field(name, pa.bool_())))
    _check_project(exprs, batch)


@pytest.mark.parametrize("offset", [1, 7, 8, 63, 64, 65, 500])
def test_array_offsets(offset):
    """Sliced batches: validity bits start mid-word, values pointers are only 8-byte aligned."""
    rng = np.random.default_rng(offset)
    full = _batch(rng, [pa.float64(), pa.float64(), pa.int32(), pa.bool_()], 3000, 0.2)
    batch = full.slice(offset, 1717)
    b = gandiva.TreeExprBuilder()
    f = [b.make_field(batch.schema.field(i)) for i in range(4)]
    e0 = b.make_expression(b.make_function("add", [f[0], f[1]], pa.float64()), pa.field("s", pa.float64()))
    k = b.make_literal(3, pa.int32())
    e1 = b.make_expression(b.make_function("multiply", [f[2], k], pa.int32()), pa.field("m", pa.int32()))
    e2 = b.make_expression(b.make_function("not", [f[3]], pa.bool_()), pa.field("n", pa.bool_()))
    e3 = b.make_expression(b.make_if(f[3], f[0], f[1], pa.float64()), pa.field("i", pa.float64()))
    _check_project([e0, e1, e2, e3], batch)


@pytest.mark.parametrize("n", [5, 64, 1000, 70001])
def test_if_else_and_boolean_3vl(n):
    rng = np.random.default_rng(n)
    batch = _batch(rng, [pa.int64(), pa.int64(), pa.float64(), pa.bool_()], n, 0.3)
    b = gandiva.TreeExprBuilder()
    a, c, d, z = (b.make_field(batch.schema.field(i)) for i in range(4))
    zero = b.make_literal(0, pa.int64())
    gt = b.make_function("greater_than", [a, c], pa.bool_())
    lt = b.make_function("less_than", [a, zero], pa.bool_())
    nested = b.make_if(gt, a, b.make_if(lt, c, zero, pa.int64()), pa.int64())
    exprs = [
        b.make_expression(nested, pa.field("nested", pa.int64())),
        b.make_expression(b.make_and([gt, z]), pa.field("and", pa.bool_())),
        b.make_expression(b.make_or([gt, z, lt]), pa.field("or", pa.bool_())),
        b.make_expression(b.make_and([b.make_or([gt, z]), b.make_function("not", [lt], pa.bool_())]),
                          pa.field("mix", pa.bool_())),
        b.make_expression(b.make_function("isnull", [d], pa.bool_()), pa.field("isnull", pa.bool_())),
        b.make_expression(b.make_function("isnotnull", [a], pa.bool_()), pa.field("isnotnull", pa.bool_())),
        b.make_expression(b.make_function("is_distinct_from", [a, c], pa.bool_()), pa.field("idf", pa.bool_())),
        b.make_expression(b.make_if(b.make_function("isnull", [a], pa.bool_()), c, a, pa.int64()),
                          pa.field("coalesce", pa.int64())),
        b.make_expression(b.make_null(pa.int64()), pa.field("null", pa.int64())),
    ]
    _check_project(exprs, batch)


def test_casts_hash_and_dates():
    rng = np.random.default_rng(11)
    n = 5000
    batch = _batch(rng, [pa.int32(), pa.int64(), pa.float32(), pa.float64(), pa.date64(),
                         pa.timestamp('ms'), pa.date32()], n, 0.15)
    b = gandiva.TreeExprBuilder()
    i32, i64, f32, f64, d64, ts, d32 = (b.make_field(batch.schema.field(i)) for i in range(7))

    def ex(name, args, t):
        return b.make_expression(b.make_function(name, args, t), pa.field(name + str(len(exprs)), t))
    exprs = []
    exprs += [ex("castBIGINT", [i32], pa.int64()), ex("castINT", [i64], pa.int32()),
              ex("castFLOAT4", [i32], pa.float32()), ex("castFLOAT4", [i64], pa.float32()),
              ex("castFLOAT4", [f64], pa.float32()), ex("castFLOAT8", [i32], pa.float64()),
              ex("castFLOAT8", [i64], pa.float64()), ex("castFLOAT8", [f32], pa.float64()),
              ex("castBIGINT", [f64], pa.int64()), ex("castINT", [f32], pa.int32())]
    for t, node in ((pa.int32(), i32), (pa.int64(), i64), (pa.float32(), f32), (pa.float64(), f64),
                    (pa.date64(), d64), (pa.timestamp('ms'), ts)):
        exprs += [ex("hash32", [node], pa.int32()), ex("hash64", [node], pa.int64()),
                  ex("hash", [node], pa.int32())]
    exprs += [ex("hash64", [f64, i64], pa.int64()), ex("hash32", [i64, i32], pa.int32())]
    for part in ("Year", "Month", "Day", "Quarter", "Doy", "Dow", "Hour", "Minute", "Second",
                 "Epoch", "Decade", "Century", "Millennium"):
        exprs += [ex("extract" + part, [d64], pa.int64()), ex("extract" + part, [ts], pa.int64())]
    for part in ("Year", "Month", "Day", "Doy", "Dow"):
        exprs.append(ex("extract" + part, [d32], pa.int64()))
    seven = b.make_literal(7, pa.int64())
    for unit in ("Second", "Minute", "Hour", "Day", "Week", "Month", "Quarter", "Year"):
        exprs.append(ex("timestampadd" + unit, [seven, ts], pa.timestamp('ms')))
    exprs += [ex("date_add", [d64, seven], pa.date64()), ex("date_sub", [ts, seven], pa.timestamp('ms')),
              ex("timestampdiffDay", [ts, ts], pa.int32()), ex("datediff", [d64, d64], pa.int32()),
              ex("castDATE", [ts], pa.date64()), ex("castDATE", [d32], pa.date64())]
    d32b = b.make_literal(10561, pa.date32())  # 1998-12-01
    exprs.append(ex("datediff", [d32b, d32], pa.int32()))
    _check_project(exprs, batch)


def test_round_and_float_casts_on_the_edges_of_the_rule():
    """trunc(x +- 0.5) vs C round(): the values where the two differ, on the device."""
    from test_oracle_crosscheck import ROUND_EDGES
    rng = np.random.default_rng(3)
    vals = ROUND_EDGES + list(rng.integers(-10**6, 10**6, 3000) + 0.5) + list(rng.normal(0, 1e6, 3000))
    f64 = pa.array(vals, pa.float64())
    f32 = pa.array(np.array(vals, dtype=np.float64).astype(np.float32), pa.float32())
    batch = pa.RecordBatch.from_arrays([f64, f32], names=["d", "f"])
    b = gandiva.TreeExprBuilder()
    d, f = b.make_field(batch.schema.field(0)), b.make_field(batch.schema.field(1))
    exprs = [b.make_expression(b.make_function("round", [d], pa.float64()), pa.field("r", pa.float64())),
             b.make_expression(b.make_function("castBIGINT", [d], pa.int64()), pa.field("b", pa.int64())),
             b.make_expression(b.make_function("castINT", [d], pa.int32()), pa.field("i", pa.int32())),
             b.make_expression(b.make_function("castBIGINT", [f], pa.int64()), pa.field("bf", pa.int64())),
             b.make_expression(b.make_function("castINT", [f], pa.int32()), pa.field("if", pa.int32()))]
    _check_project(exprs, batch)


def test_float_to_integer_casts_can_follow_the_x86_jit_on_nan_and_out_of_range_values(monkeypatch):
    """Round 6 (PARITY.md): by default a float -> integer cast saturates and sends NaN to 0; the reference's JIT on
    x86 yields cvttsd2si's "indefinite integer" (0x80..0 of the destination width) for NaN and for everything
    outside the destination's range.  GDV_CAST_X86_INDEFINITE=1 at Make selects that; the oracle restates both."""
    vals = [float("nan"), float("inf"), float("-inf"), 9.3e18, -9.3e18, 2147483647.4, 2147483647.6, 2147483648.0, -2147483648.4,
            -2147483648.6, 3e9, -3e9, 1e300, -1e300, 0.5, -0.5, 123456.5, 9223372036854775807.0, -9223372036854775808.0]
    batch = pa.RecordBatch.from_arrays([pa.array(vals, pa.float64()), pa.array(np.array(vals).astype(np.float32), pa.float32())],
                                       names=["d", "f"])
    b = gandiva.TreeExprBuilder()
    d, f = b.make_field(batch.schema.field(0)), b.make_field(batch.schema.field(1))
    exprs = [b.make_expression(b.make_function("castBIGINT", [d], pa.int64()), pa.field("b", pa.int64())),
             b.make_expression(b.make_function("castINT", [d], pa.int32()), pa.field("i", pa.int32())),
             b.make_expression(b.make_function("castBIGINT", [f], pa.int64()), pa.field("bf", pa.int64())),
             b.make_expression(b.make_function("castINT", [f], pa.int32()), pa.field("if", pa.int32()))]
    saturating = gandiva.make_projector(batch.schema, exprs, None).evaluate(batch)
    assert saturating[0].to_pylist()[:5] == [0, 2**63 - 1, -2**63, 2**63 - 1, -2**63]
    assert saturating[1].to_pylist()[:3] == [0, 2**31 - 1, -2**31]
    monkeypatch.setenv("GDV_CAST_X86_INDEFINITE", "1")
    indefinite = gandiva.make_projector(batch.schema, exprs, None).evaluate(batch)
    oracle.cast_indefinite(True)
    try:
        want = oracle.project(exprs, batch)
    finally:
        oracle.cast_indefinite(False)
    for g, w, e in zip(indefinite, want, "b i bf if".split()):
        assert_bit_exact(g, w, "x86 indefinite, " + e)
    assert indefinite[0].to_pylist()[:5] == [-2**63] * 5 and indefinite[1].to_pylist()[:3] == [-2**31] * 3
    assert indefinite[1].to_pylist()[5:8] == [2147483647, -2**31, -2**31]    # 2147483647.4 rounds inside, .6 and 2^31 do not fit


def test_math_functions_within_one_ulp():
    """exp/log/pow/cbrt come from math libraries on both sides (ROCm device libs / host
    libm), so they are not bit-comparable with each other.  north_star's tolerance is 1 ulp:
    the HIP result must be within 1 ulp of the correctly rounded value, computed here in x87
    extended precision (numpy longdouble) and rounded once; the oracle (host libm) is held to
    its own documented bound."""
    from helpers import ulp_distance
    rng = np.random.default_rng(5)
    n = 20000
    xs = rng.random(n) * 100 + 0.01
    ys = rng.random(n) * 3
    batch = pa.RecordBatch.from_arrays([pa.array(xs), pa.array(ys)], names=["x", "y"])
    b = gandiva.TreeExprBuilder()
    fx, fy = b.make_field(batch.schema.field(0)), b.make_field(batch.schema.field(1))
    f64 = pa.float64()
    lx, ly = xs.astype(np.longdouble), ys.astype(np.longdouble)
    cases = [("exp", [fy], np.exp(ly)), ("log", [fx], np.log(lx)), ("log10", [fx], np.log10(lx)),
             ("cbrt", [fx], np.cbrt(lx)), ("sqrt", [fx], np.sqrt(lx)),
             ("power", [fx, fy], np.power(lx, ly))]
    exprs = [b.make_expression(b.make_function(nm, args, f64), pa.field(nm, f64)) for nm, args, _ in cases]
    proj = gandiva.make_projector(batch.schema, exprs, pa.default_memory_pool())
    got = proj.evaluate(batch)
    want = oracle.project(exprs, batch)
    report = {}
    for (nm, _, exact), g, w in zip(cases, got, want):
        ref = exact.astype(np.float64)
        report[nm] = (ulp_distance(g.to_numpy(), ref), ulp_distance(w.to_numpy(), ref))
    print("max ulp (hip, oracle) vs correctly rounded:", report)
    for nm, (hip_ulp, cpu_ulp) in report.items():
        assert hip_ulp <= 1, f"{nm}: HIP result {hip_ulp} ulp from the correctly rounded value"
        # the host libm is not the product: glibc documents up to 4 ulp for cbrt
        assert cpu_ulp <= 4, f"{nm}: oracle result {cpu_ulp} ulp from the correctly rounded value"


def test_divide_by_zero_is_an_execution_error_but_guards_work():
    a = pa.array([10, 20, 30, None], type=pa.int64())
    z = pa.array([2, 0, 5, 0], type=pa.int64())
    batch = pa.RecordBatch.from_arrays([a, z], names=["a", "z"])
    b = gandiva.TreeExprBuilder()
    fa, fz = b.make_field(batch.schema.field(0)), b.make_field(batch.schema.field(1))
    div = b.make_function("divide", [fa, fz], pa.int64())
    proj = gandiva.make_projector(batch.schema, [b.make_expression(div, pa.field("q", pa.int64()))],
                                  pa.default_memory_pool())
    with pytest.raises(pa.lib.ArrowException, match="divide by zero"):
        proj.evaluate(batch)
    with pytest.raises(oracle.OracleError, match="divide by zero"):
        oracle.project([b.make_expression(div, pa.field("q", pa.int64()))], batch)
    # `if (z != 0) a / z else -1` must not raise: the divide only runs on the taken branch
    zero = b.make_literal(0, pa.int64())
    guard = b.make_function("not_equal", [fz, zero], pa.bool_())
    safe = b.make_if(guard, div, b.make_literal(-1, pa.int64()), pa.int64())
    _check_project([b.make_expression(safe, pa.field("q", pa.int64()))], batch)
    # a null divisor row does not raise either (functions that can fail run on valid rows only)
    z2 = pa.array([2, None, 5, 1], type=pa.int64())
    _check_project([b.make_expression(div, pa.field("q", pa.int64()))],
                   pa.RecordBatch.from_arrays([a, z2], names=["a", "z"]))


@pytest.mark.parametrize("n", [10, 1000, 100000])
@pytest.mark.parametrize("dtype,mode", [("int16", "UINT16"), ("int32", "UINT32"), ("int64", "UINT64")])
def test_filter_then_project_with_selection_vector(n, dtype, mode):
    rng = np.random.default_rng(n)
    batch = _batch(rng, [pa.int32(), pa.int32(), pa.float64()], n, 0.2)
    b = gandiva.TreeExprBuilder()
    a, c, d = (b.make_field(batch.schema.field(i)) for i in range(3))
    cond = b.make_condition(b.make_function("greater_than", [a, c], pa.bool_()))
    e0 = b.make_expression(b.make_if(b.make_function("less_than", [a, c], pa.bool_()), a, c, pa.int32()),
                           pa.field("m", pa.int32()))
    e1 = b.make_expression(b.make_function("multiply", [d, d], pa.float64()), pa.field("sq", pa.float64()))
    e2 = b.make_expression(b.make_function("isnull", [d], pa.bool_()), pa.field("nul", pa.bool_()))
    flt = gandiva.make_filter(batch.schema, cond)
    proj = gandiva.make_projector(batch.schema, [e0, e1, e2], pa.default_memory_pool(), mode)
    if dtype == "int16" and n > 65536:
        # a uint16 selection vector addresses 65536 rows: a larger batch is refused (not truncated), and the
        # largest batch it can address takes the whole filter -> project path
        with pytest.raises(pa.lib.ArrowException, match="uint16 selection vector cannot address"):
            flt.evaluate(batch, pa.default_memory_pool(), dtype)
        batch = batch.slice(0, 65536)
    sel = flt.evaluate(batch, pa.default_memory_pool(), dtype)
    want_sel = oracle.filter_indices(cond, batch, dtype)
    assert sel.to_array().equals(want_sel)
    if sel.num_slots == 0:
        return
    got = proj.evaluate(batch, sel)
    want = oracle.project([e0, e1, e2], oracle.take_rows(batch, want_sel.to_numpy()))
    for g, w in zip(got, want):
        assert_bit_exact(g, w)


def test_in_expression_large_list():
    rng = np.random.default_rng(3)
    batch = _batch(rng, [pa.int64(), pa.int32()], 10000, 0.1)
    b = gandiva.TreeExprBuilder()
    a, c = b.make_field(batch.schema.field(0)), b.make_field(batch.schema.field(1))
    big = [int(v) for v in rng.integers(-1000, 1000, 300)]
    small = [-3, 0, 7]
    for node, vals, t in ((a, big, pa.int64()), (c, small, pa.int32()), (c, big, pa.int32())):
        cond = b.make_condition(b.make_in_expression(node, vals, t))
        got = gandiva.make_filter(batch.schema, cond).evaluate(batch, None).to_array()
        assert got.equals(oracle.filter_indices(cond, batch, "int32"))


def test_device_resident_batches_match_host_path():
    """Zero-copy HBM path == staged host path == oracle."""
    import torch
    n = 200003
    batch = W.c2_batch(n)
    exprs = W.c2_expressions()
    proj = gandiva.make_projector(batch.schema, exprs, None)
    dbatch = gandiva.DeviceBatch.from_arrow(batch)
    outs = proj.evaluate_device(dbatch)
    torch.cuda.synchronize()
    want = oracle.project(exprs, batch)
    for o, w in zip(outs, want):
        assert_bit_exact(o.to_arrow(), w)
    cond = W.c3_condition()
    b3 = W.c3_batch(n, 0.1)
    flt = gandiva.make_filter(b3.schema, cond)
    sel = flt.evaluate_device(gandiva.DeviceBatch.from_arrow(b3), "int32")
    assert sel.to_array().equals(oracle.filter_indices(cond, b3, "int32"))


def test_full_size_properties_c2():
    """BASELINE C2 at a size the oracle cannot hold: size-independent properties.
    (a) linearity of validity: popcount(valid(e0)) == popcount(valid(a) & valid(b));
    (b) e0 + e1 == 2a bit-exactly where all valid and finite (a+b + a-b need not be exact,
        so instead check the exact identities) e2 == a*b recomputed by torch in fp64;
    (c) a prefix slice copied to the host is bit-exact against the oracle."""
    import torch
    n = 1 << 26
    dbatch = W.c2_device_batch(n)
    exprs = W.c2_expressions()
    proj = gandiva.make_projector(W.c2_schema(), exprs, None)
    outs = proj.evaluate_device(dbatch)
    torch.cuda.synchronize()
    a = dbatch.columns[0].data.view(torch.float64)
    bcol = dbatch.columns[1].data.view(torch.float64)
    e0 = outs[0].data.view(torch.float64)[:n]
    e2 = outs[2].data.view(torch.float64)[:n]
    assert torch.equal(e0.view(torch.int64), (a + bcol).view(torch.int64))
    assert torch.equal(e2.view(torch.int64), (a * bcol).view(torch.int64))
    nb = (n + 7) // 8
    va, vb = dbatch.columns[0].validity[:nb], dbatch.columns[1].validity[:nb]
    assert torch.equal(outs[0].validity[:nb], va & vb)
    assert torch.equal(outs[1].validity[:nb], va & vb)
    vc, vd = dbatch.columns[2].validity[:nb], dbatch.columns[3].validity[:nb]
    assert torch.equal(outs[9].validity[:nb], va & vb & vc & vd)
    # prefix vs oracle
    m = 100000
    host_cols = []
    for c in dbatch.columns:
        host_cols.append(pa.Array.from_buffers(pa.float64(), m, [
            pa.py_buffer(c.validity[:(m + 7) // 8 + 8].cpu().numpy()),
            pa.py_buffer(c.data[:m * 8].cpu().numpy())]))
    hb = pa.RecordBatch.from_arrays(host_cols, schema=W.c2_schema())
    want = oracle.project(exprs, hb)
    for o, w in zip(outs, want):
        got = pa.Array.from_buffers(pa.float64(), m, [
            pa.py_buffer(o.validity[:(m + 7) // 8 + 8].cpu().numpy()),
            pa.py_buffer(o.data[:m * 8].cpu().numpy())])
        assert_bit_exact(got, w)


def test_concurrent_evaluate_is_reentrant():
    """The reference's bindings are `nogil`: Evaluate on ONE projector/filter from many threads
    at once (per-call scratch only).  8 threads x 20 evaluations on distinct batches."""
    import threading
    exprs = W.c2_expressions()
    proj = gandiva.make_projector(W.c2_schema(), exprs, None)
    cond = W.c3_condition()
    flt = gandiva.make_filter(W.c3_schema(), cond)
    batches = [W.c2_batch(5000 + 997 * i, seed_offset=i) for i in range(8)]
    fbatches = [W.c3_batch(7000 + 313 * i, 0.1) for i in range(8)]
    want = [oracle.project(exprs, b) for b in batches]
    fwant = [oracle.filter_indices(cond, b, "int32") for b in fbatches]
    errors = []

    def work(i):
        try:
            for _ in range(20):
                got = proj.evaluate(batches[i])
                for g, w in zip(got, want[i]):
                    assert_bit_exact(g, w)
                assert flt.evaluate(fbatches[i], None).to_array().equals(fwant[i])
        except Exception as e:  # noqa: BLE001
            errors.append((i, repr(e)))
    threads = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_wide_projection_many_columns():
    """64 input columns, 48 outputs: the by-value kernel argument block is ~5 KB."""
    rng = np.random.default_rng(64)
    n = 3001
    ncol = 64
    cols = [random_array(rng, pa.int64(), n, 0.1, special=False) for _ in range(ncol)]
    batch = pa.RecordBatch.from_arrays(cols, names=[f"c{i}" for i in range(ncol)])
    b = gandiva.TreeExprBuilder()
    f = [b.make_field(batch.schema.field(i)) for i in range(ncol)]
    exprs = []
    for i in range(48):
        node = b.make_function("add", [f[i], b.make_function("multiply", [f[(i + 7) % ncol], f[(i + 13) % ncol]],
                                                             pa.int64())], pa.int64())
        exprs.append(b.make_expression(node, pa.field(f"o{i}", pa.int64())))
    _check_project(exprs, batch)


def test_uint_and_narrow_types_in_filters():
    rng = np.random.default_rng(77)
    n = 20001
    batch = _batch(rng, [pa.uint8(), pa.int16(), pa.uint32(), pa.float32(), pa.date32()], n, 0.2)
    b = gandiva.TreeExprBuilder()
    u8, i16, u32, f32, d32 = (b.make_field(batch.schema.field(i)) for i in range(5))
    conds = [
        b.make_function("greater_than", [u8, b.make_literal(100, pa.uint8())], pa.bool_()),
        b.make_function("less_than", [i16, b.make_literal(-5, pa.int16())], pa.bool_()),
        b.make_function("not_equal", [u32, b.make_literal(7, pa.uint32())], pa.bool_()),
        b.make_function("less_than_or_equal_to", [f32, b.make_literal(0.5, pa.float32())], pa.bool_()),
        b.make_function("greater_than_or_equal_to", [d32, b.make_literal(10000, pa.date32())], pa.bool_()),
    ]
    for c in conds + [b.make_and(conds[:3]), b.make_or(conds[2:])]:
        cond = b.make_condition(c)
        got = gandiva.make_filter(batch.schema, cond).evaluate(batch, None, "int64").to_array()
        assert got.equals(oracle.filter_indices(cond, batch, "int64"))


def test_make_is_cached_and_invalid_inputs_are_rejected():
    exprs = W.c1_expressions()
    schema = W.c1_schema()
    p1 = gandiva.make_projector(schema, exprs, None)
    p2 = gandiva.make_projector(schema, W.c1_expressions(), None)   # same key -> cached plan
    assert p1.llvm_ir == p2.llvm_ir
    with pytest.raises(pa.ArrowInvalid):                            # empty batch
        p1.evaluate(W.c1_batch(8).slice(0, 0))
    with pytest.raises(pa.ArrowInvalid):                            # schema mismatch
        p1.evaluate(W.c2_batch(8))
    with pytest.raises(pa.ArrowInvalid):                            # selection on a NONE-mode projector
        p1.evaluate(W.c1_batch(8), gandiva.SelectionVector(2, np.zeros(4, np.uint32), 4))


def test_device_path_with_array_offsets_and_misaligned_bitmaps():
    """Zero-copy path: Arrow array offsets (bit offset inside the validity word) and a
    validity buffer that does not start on an 8-byte boundary (FoldBitmap, gdv_engine.cc)."""
    import torch
    rng = np.random.default_rng(123)
    n_full = 9000
    full = _batch(rng, [pa.float64(), pa.int64(), pa.bool_()], n_full, 0.25, names=["x", "y", "z"])
    b = gandiva.TreeExprBuilder()
    x, y, z = (b.make_field(full.schema.field(i)) for i in range(3))
    exprs = [
        b.make_expression(b.make_function("multiply", [x, x], pa.float64()), pa.field("sq", pa.float64())),
        b.make_expression(b.make_if(z, y, b.make_function("negative", [y], pa.int64()), pa.int64()),
                          pa.field("sel", pa.int64())),
        b.make_expression(b.make_and([z, b.make_function("greater_than", [y, b.make_literal(0, pa.int64())],
                                                         pa.bool_())]), pa.field("p", pa.bool_())),
    ]
    proj = gandiva.make_projector(full.schema, exprs, None)
    base = gandiva.DeviceBatch.from_arrow(full)
    for off, length in ((1, 4000), (63, 1234), (64, 8000), (777, 8223)):
        cols = []
        for c in base.columns:
            # shift every bitmap by 3 bytes so its address is not 8-byte aligned: copy into a
            # padded tensor at byte offset 3 and move the array offset back by 24 bits
            def shifted(t):
                s = torch.zeros(t.numel() + 64, dtype=torch.uint8, device="cuda")
                s[3:3 + t.numel()] = t
                return s[3:]
            validity = shifted(c.validity) if c.validity is not None else None
            data = shifted(c.data) if pa.types.is_boolean(c.type) else c.data
            cols.append(gandiva.DeviceColumn(c.type, length, validity, data, None, off))
        dbatch = gandiva.DeviceBatch(full.schema, cols, length)
        outs = proj.evaluate_device(dbatch)
        torch.cuda.synchronize()
        want = oracle.project(exprs, full.slice(off, length))
        for o, w in zip(outs, want):
            assert_bit_exact(o.to_arrow(), w, f"offset {off}")


def test_bitwise_boolean_tests_and_nvl():
    rng = np.random.default_rng(31)
    n = 7001
    batch = _batch(rng, [pa.int64(), pa.int64(), pa.uint32(), pa.uint32(), pa.bool_(), pa.float64(), pa.float64()],
                   n, 0.3)
    b = gandiva.TreeExprBuilder()
    i1, i2, u1, u2, z, f1, f2 = (b.make_field(batch.schema.field(i)) for i in range(7))
    exprs = []
    for name in ("bitwise_and", "bitwise_or", "bitwise_xor"):
        exprs.append(b.make_expression(b.make_function(name, [i1, i2], pa.int64()), pa.field(name, pa.int64())))
        exprs.append(b.make_expression(b.make_function(name, [u1, u2], pa.uint32()), pa.field(name + "u", pa.uint32())))
    exprs.append(b.make_expression(b.make_function("bitwise_not", [i1], pa.int64()), pa.field("not", pa.int64())))
    for name in ("istrue", "isfalse", "isnottrue", "isnotfalse"):
        exprs.append(b.make_expression(b.make_function(name, [z], pa.bool_()), pa.field(name, pa.bool_())))
    exprs.append(b.make_expression(b.make_function("nvl", [f1, f2], pa.float64()), pa.field("nvl", pa.float64())))
    exprs.append(b.make_expression(b.make_function("nvl", [i1, b.make_literal(-1, pa.int64())], pa.int64()),
                                   pa.field("nvl_lit", pa.int64())))
    exprs.append(b.make_expression(b.make_function("add", [b.make_function("nvl", [i1, i2], pa.int64()), i2],
                                                   pa.int64()), pa.field("nvl_add", pa.int64())))
    _check_project(exprs, batch)


def test_more_than_2_to_32_rows_device_resident():
    """Maximum sizes: a batch of 2^32 + 4099 int8 rows (row indices need 64 bits).
    Projection: add(a, b) wraps like two's complement, checked against torch on the GPU.
    Filter: a > 100 with a uint64 selection vector — count, ascending order, and the head /
    tail windows against torch.nonzero."""
    import torch
    n = (1 << 32) + 4099
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    a = torch.empty(n, dtype=torch.int8, device="cuda")
    bcol = torch.empty(n, dtype=torch.int8, device="cuda")
    chunk = 1 << 30
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        a[lo:hi] = torch.randint(-128, 128, (hi - lo,), dtype=torch.int8, device="cuda", generator=g)
        bcol[lo:hi] = torch.randint(-128, 128, (hi - lo,), dtype=torch.int8, device="cuda", generator=g)
    schema = pa.schema([pa.field("a", pa.int8()), pa.field("b", pa.int8())])
    dbatch = gandiva.DeviceBatch(schema, [
        gandiva.DeviceColumn(pa.int8(), n, None, a.view(torch.uint8)),
        gandiva.DeviceColumn(pa.int8(), n, None, bcol.view(torch.uint8))], n)
    b = gandiva.TreeExprBuilder()
    fa, fb = b.make_field(schema.field(0)), b.make_field(schema.field(1))
    proj = gandiva.make_projector(schema, [b.make_expression(b.make_function("add", [fa, fb], pa.int8()),
                                                              pa.field("s", pa.int8()))], None)
    out, = proj.evaluate_device(dbatch)
    torch.cuda.synchronize()
    got = out.data[:n].view(torch.int8)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        assert torch.equal(got[lo:hi], a[lo:hi] + bcol[lo:hi])
    nb = (n + 7) // 8
    assert bool((out.validity[:nb - 1] == 255).all()) and int(out.validity[nb - 1]) == (1 << (n % 8)) - 1
    del out, got
    cond = b.make_condition(b.make_function("greater_than", [fa, b.make_literal(100, pa.int8())], pa.bool_()))
    flt = gandiva.make_filter(schema, cond)
    idx = torch.empty(n, dtype=torch.int64, device="cuda")
    sel = flt.evaluate_device(dbatch, "int64", out=idx)
    k = sel.num_slots
    want_count = sum(int((a[lo:min(n, lo + chunk)] > 100).sum()) for lo in range(0, n, chunk))
    assert k == want_count
    ids = idx[:k]
    assert bool((ids[1:] > ids[:-1]).all())
    head = torch.nonzero(a[:1 << 20] > 100).flatten()
    assert torch.equal(ids[:head.numel()], head)
    tail_lo = n - (1 << 20)
    tail = torch.nonzero(a[tail_lo:] > 100).flatten() + tail_lo
    assert torch.equal(ids[k - tail.numel():], tail)
    assert int(ids[-1]) >= (1 << 32) - 4096  # indices really exceed 32 bits' reach


def test_plan_cache_distinguishes_trees_that_render_alike():
    """The reference's ToString() is pinned without parentheses around nested AND/OR and with
    unescaped string literals, so different trees can render to the same text.  The plan cache
    must not confuse them (round-1 advisor finding): both nestings built in ONE process, each
    against the oracle; same for an IN list whose quoting is ambiguous."""
    rng = np.random.default_rng(5)
    n = 3000
    batch = _batch(rng, [pa.bool_(), pa.bool_(), pa.bool_()], n, 0.2)
    b = gandiva.TreeExprBuilder()
    x, y, z = (b.make_field(batch.schema.field(i)) for i in range(3))
    left = b.make_or([b.make_and([x, y]), z])     # (x AND y) OR z
    right = b.make_and([x, b.make_or([y, z])])    # x AND (y OR z)
    assert str(left) == str(right)
    for tree in (left, right):
        _check_project([b.make_expression(tree, pa.field("r", pa.bool_()))], batch)
        cond = b.make_condition(tree)
        got = gandiva.make_filter(batch.schema, cond).evaluate(batch, None)
        assert got.to_array().equals(oracle.filter_indices(cond, batch, "int32"))
    sb = pa.RecordBatch.from_arrays([pa.array(["a", "b", "a', 'b", None, "c"])], names=["s"])
    s = b.make_field(sb.schema.field(0))
    two = b.make_in_expression(s, ["a", "b"], pa.string())
    one = b.make_in_expression(s, ["a', 'b"], pa.string())
    assert str(two) == str(one)
    for tree in (two, one):
        _check_project([b.make_expression(tree, pa.field("r", pa.bool_()))], sb)


def test_literals_are_kernel_arguments_not_source_text():
    """`a > 499` / `a > 500`, IN lists of equal size and LIKE needles of equal length share ONE
    compiled kernel (round-1 verdict: every distinct constant was a fresh hipRTC compile); each
    instance still computes with its own values."""
    import re
    rng = np.random.default_rng(77)
    n = 5000
    batch = pa.RecordBatch.from_arrays(
        [pa.array(rng.integers(0, 1000, n)), pa.array(rng.standard_normal(n)),
         pa.array([["spark", "flink", "a spark b", "xflinky", None][int(i)] for i in rng.integers(0, 5, n)])],
        names=["a", "x", "s"])
    b = gandiva.TreeExprBuilder()
    a, x, s = (b.make_field(batch.schema.field(i)) for i in range(3))
    names = set()
    for k, f, pat, inl in ((499, 0.25, "%spark%", [1, 5, 9]), (500, -1.5, "%flink%", [2, 500, 777])):
        cond = b.make_condition(b.make_and([
            b.make_function("greater_than", [a, b.make_literal(k, pa.int64())], pa.bool_()),
            b.make_or([b.make_function("less_than", [x, b.make_literal(f, pa.float64())], pa.bool_()),
                       b.make_function("like", [s, b.make_literal(pat, pa.string())], pa.bool_()),
                       b.make_in_expression(a, inl, pa.int64())])]))
        flt = gandiva.make_filter(batch.schema, cond)
        names.add(re.search(r"gdv_k_[0-9a-f]{16}", flt.llvm_ir).group(0))
        assert flt.evaluate(batch, None).to_array().equals(oracle.filter_indices(cond, batch, "int32"))
    assert len(names) == 1, names


@pytest.mark.parametrize("chunks", [2, 5, 8])
@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_pipelined_filter_chunks_match_the_oracle(monkeypatch, chunks, dtype):
    """Round 3: big HBM-resident batches are filtered in chunks — predicate kernel of chunk k + 1 on
    the caller's stream, offsets scan (carrying the running total) + index emission of chunk k on a
    side stream.  Forced here at a size the oracle handles: ragged last chunk, nulls, every chunk
    boundary inside the batch; indices ascending and identical to the unchunked result."""
    import torch
    n = 100_003
    rng = np.random.default_rng(chunks)
    batch = _batch(rng, [pa.int64(), pa.int64(), pa.float64()], n, 0.15)
    b = gandiva.TreeExprBuilder()
    a, c, d = (b.make_field(batch.schema.field(i)) for i in range(3))
    cond = b.make_condition(b.make_or([b.make_function("greater_than", [a, c], pa.bool_()),
                                       b.make_function("isnull", [d], pa.bool_())]))
    flt = gandiva.make_filter(batch.schema, cond)
    flt.set_tuning("chunks", chunks)
    want = oracle.filter_indices(cond, batch, dtype)
    db = gandiva.DeviceBatch.from_arrow(batch)
    sel = flt.evaluate_device(db, dtype)
    torch.cuda.synchronize()
    assert sel.to_array().equals(want)
    # an Arrow offset that is not a multiple of 64 (funnel-shifted bitmaps) through the chunked path
    sl = batch.slice(37, n - 100)
    sel2 = flt.evaluate_device(gandiva.DeviceBatch.from_arrow(sl), dtype)
    assert sel2.to_array().equals(oracle.filter_indices(cond, sl, dtype))
    flt.set_tuning("chunks", 1)
    assert flt.evaluate_device(db, dtype).to_array().equals(want)


def test_asynchronous_filter_feeds_a_projector_without_a_host_round_trip():
    """filter (sync=False) -> selection-mode projector: the slot count stays in HBM between the two
    calls (gdv_filter_evaluate_async / gdv_projector_evaluate_selected); nothing waits until the
    results are read."""
    import torch
    n = 300_007
    rng = np.random.default_rng(17)
    batch = _batch(rng, [pa.int32(), pa.int32(), pa.float64()], n, 0.2)
    b = gandiva.TreeExprBuilder()
    a, c, d = (b.make_field(batch.schema.field(i)) for i in range(3))
    cond = b.make_condition(b.make_function("greater_than", [a, c], pa.bool_()))
    exprs = [b.make_expression(b.make_function("add", [a, c], pa.int32()), pa.field("s", pa.int32())),
             b.make_expression(b.make_function("multiply", [d, d], pa.float64()), pa.field("sq", pa.float64())),
             b.make_expression(b.make_function("isnull", [d], pa.bool_()), pa.field("nul", pa.bool_()))]
    flt = gandiva.make_filter(batch.schema, cond)
    proj = gandiva.make_projector(batch.schema, exprs, None, "UINT32")
    db = gandiva.DeviceBatch.from_arrow(batch)
    for chunks in (1, 3):
        flt.set_tuning("chunks", chunks)
        try:
            sel = flt.evaluate_device(db, "int32", sync=False)
            assert sel.pending                                   # the count has not left the device
            outs = proj.evaluate_device(db, selection=sel, sync=False)
            assert sel.pending
            torch.cuda.synchronize()
        finally:
            flt.set_tuning("chunks", 1)
        want_sel = oracle.filter_indices(cond, batch, "int32")
        assert sel.num_slots == len(want_sel) and sel.to_array().equals(want_sel)
        want = oracle.project(exprs, oracle.take_rows(batch, want_sel.to_numpy()))
        for o, w in zip(outs, want):
            assert o.length == n                                 # sized for the capacity ...
            got = o.to_arrow()                                   # ... and trimmed to the count when read
            assert o.num_rows == sel.num_slots == len(got)
            assert_bit_exact(got, w)


def test_many_small_batches_in_one_launch_match_the_oracle():
    """gdv_projector_evaluate_many: 40 HBM-resident batches of 1 .. 70 000 rows, one launch (the grid's
    second dimension picks the batch), every batch bit-exact; plans without the multi-batch entry
    (var-len inputs) take the batch-by-batch fallback through the same call."""
    import torch
    rng = np.random.default_rng(99)
    sizes = [1, 63, 64, 65, 1000, 1024, 4096, 16384, 65536, 70_000] + [int(v) for v in rng.integers(1, 20_000, 30)]
    exprs = W.c2_expressions()
    proj = gandiva.make_projector(W.c2_schema(), exprs, None)
    batches = [W.c2_batch(n, seed_offset=k) if "seed_offset" in W.c2_batch.__code__.co_varnames else W.c2_batch(n)
               for k, n in enumerate(sizes)]
    dbs = [gandiva.DeviceBatch.from_arrow(b) for b in batches]
    outs = proj.evaluate_device_many(dbs)
    torch.cuda.synchronize()
    for b, o in zip(batches, outs):
        for g, w in zip(o, oracle.project(exprs, b)):
            assert_bit_exact(g.to_arrow(), w)
    # asynchronous, buffers reused
    outs2 = proj.evaluate_device_many(dbs, outputs=outs, sync=False)
    torch.cuda.synchronize()
    assert_bit_exact(outs2[9][3].to_arrow(), oracle.project(exprs, batches[9])[3])
    # a plan that can raise reports the error of whichever batch raised
    b = gandiva.TreeExprBuilder()
    sch = pa.schema([pa.field("a", pa.int64()), pa.field("z", pa.int64())])
    div = gandiva.make_projector(sch, [b.make_expression(b.make_function(
        "divide", [b.make_field(sch.field(0)), b.make_field(sch.field(1))], pa.int64()), pa.field("q", pa.int64()))], None)
    ok = pa.RecordBatch.from_arrays([pa.array([10, 20], pa.int64()), pa.array([2, 5], pa.int64())], schema=sch)
    bad = pa.RecordBatch.from_arrays([pa.array([10, 20], pa.int64()), pa.array([2, 0], pa.int64())], schema=sch)
    got = div.evaluate_device_many([gandiva.DeviceBatch.from_arrow(ok)] * 3)
    assert got[2][0].to_arrow().to_pylist() == [5, 4]
    with pytest.raises(pa.lib.ArrowException, match="divide by zero"):
        div.evaluate_device_many([gandiva.DeviceBatch.from_arrow(x) for x in (ok, bad, ok)])


@pytest.mark.parametrize("dtype", ["int16", "int32", "int64"])
def test_small_batch_filter_one_workgroup_per_batch(dtype):
    """Round 3: an HBM-resident batch of up to 2^17 rows is filtered by ONE workgroup in ONE launch
    (predicate, offsets scan, index emission back to back); many such batches still take one launch.
    Every index against the oracle, batch sizes around every tile boundary, nulls, all index widths;
    and the same batches through the three-launch path (GDV_NO_SMALL_FILTER) agree."""
    import torch
    rng = np.random.default_rng(5)
    sizes = [1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 16384, 50_001, 65536]
    if dtype != "int16":
        sizes += [65537, 100_000, 131072]
    b = gandiva.TreeExprBuilder()
    batches = [_batch(rng, [pa.int64(), pa.int64(), pa.float64()], n, 0.2) for n in sizes]
    a, c, d = (b.make_field(batches[0].schema.field(i)) for i in range(3))
    cond = b.make_condition(b.make_or([b.make_function("greater_than", [a, c], pa.bool_()),
                                       b.make_function("isnull", [d], pa.bool_())]))
    flt = gandiva.make_filter(batches[0].schema, cond)
    dbs = [gandiva.DeviceBatch.from_arrow(x) for x in batches]
    sels = flt.evaluate_device_many(dbs, dtype)
    for x, db, sv in zip(batches, dbs, sels):
        want = oracle.filter_indices(cond, x, dtype)
        assert sv.to_array().equals(want), x.num_rows
        assert flt.evaluate_device(db, dtype).to_array().equals(want)            # single batch: same kernel
        sva = flt.evaluate_device(db, dtype, sync=False)                          # ... asynchronously
        torch.cuda.synchronize()
        assert sva.to_array().equals(want)
    flt.set_tuning("small_filter", 0)
    try:
        assert flt.evaluate_device(dbs[-1], dtype).to_array().equals(oracle.filter_indices(cond, batches[-1], dtype))
    finally:
        flt.set_tuning("small_filter", 1)
    # an all-false and an all-true predicate
    t = b.make_condition(b.make_function("isnotnull", [b.make_literal(1, pa.int64())], pa.bool_()))
    full = gandiva.make_filter(batches[0].schema, t).evaluate_device(dbs[9], dtype)
    assert full.num_slots == sizes[9] and full.to_array().to_pylist() == list(range(sizes[9]))
    f = b.make_condition(b.make_function("isnull", [b.make_literal(1, pa.int64())], pa.bool_()))
    assert gandiva.make_filter(batches[0].schema, f).evaluate_device(dbs[9], dtype).num_slots == 0


def test_filters_that_can_raise_report_the_error_on_every_path():
    """divide inside a predicate: the fused small-batch kernel, the multi-batch launch and the
    three-launch path all hand the device error word back as an ExecutionError; guarded divides do
    not raise on any of them."""
    b = gandiva.TreeExprBuilder()
    sch = pa.schema([pa.field("a", pa.int64()), pa.field("z", pa.int64())])
    fa, fz = b.make_field(sch.field(0)), b.make_field(sch.field(1))
    div = b.make_function("divide", [fa, fz], pa.int64())
    raw = b.make_condition(b.make_function("greater_than", [div, b.make_literal(1, pa.int64())], pa.bool_()))
    guarded = b.make_condition(b.make_and([b.make_function("not_equal", [fz, b.make_literal(0, pa.int64())], pa.bool_()),
                                           b.make_function("greater_than", [div, b.make_literal(1, pa.int64())], pa.bool_())]))
    rng = np.random.default_rng(4)
    for n in (100, 5000, 300_000):           # fused kernel | fused kernel | three launches
        a = pa.array(rng.integers(-50, 50, n), pa.int64())
        z = pa.array(rng.integers(0, 4, n), pa.int64())
        batch = pa.RecordBatch.from_arrays([a, z], schema=sch)
        db = gandiva.DeviceBatch.from_arrow(batch)
        with pytest.raises(pa.lib.ArrowException, match="divide by zero"):
            gandiva.make_filter(sch, raw).evaluate_device(db, "int32")
        with pytest.raises(pa.lib.ArrowException, match="divide by zero"):
            gandiva.make_filter(sch, raw).evaluate(batch, None)
        g = gandiva.make_filter(sch, guarded)
        want = oracle.filter_indices(guarded, batch, "int32")
        assert g.evaluate_device(db, "int32").to_array().equals(want)
        assert g.evaluate_device(db, "int32", sync=False).to_array().equals(want)   # (plans that can raise wait anyway)
        if n <= 5000:
            assert g.evaluate_device_many([db, db], "int32")[1].to_array().equals(want)
            with pytest.raises(pa.lib.ArrowException, match="divide by zero"):
                gandiva.make_filter(sch, raw).evaluate_device_many([db, db], "int32")
