"""upper / lower under GDV_UTF8_CASE=1 at Make, on the GPU, through the C ABI (the gandiva_amd Python mirror).

PARITY STATUS (PARITY.md, `upper lower`): 2-engines against utf8proc itself — every expected value is what
pyarrow.compute.utf8_upper / utf8_lower give (the utf8proc linked into libarrow); the oracle does not know the option.
The rows, the alphabet and the forced lengths are those of tests/test_utf8_case_cpu.py."""
import os
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import gandiva_amd as gandiva
from helpers import assert_bit_exact
import test_utf8_case_cpu as R

STR, BOOL, I64, I32 = pa.string(), pa.bool_(), pa.int64(), pa.int32()
pytestmark = pytest.mark.gpu


class T:
    def __init__(self, schema):
        self.b = gandiva.TreeExprBuilder()
        self.f = {f.name: self.b.make_field(f) for f in schema}

    def lit(self, v, t=STR):
        return self.b.make_literal(v, t)

    def fn(self, name, args, t=STR):
        return self.b.make_function(name, args, t)

    def up(self, x):
        return self.fn("upper", [x])

    def lo(self, x):
        return self.fn("lower", [x])

    def expr(self, node, name, t=STR):
        return self.b.make_expression(node, pa.field(name, t))


def _make(monkeypatch, schema, exprs, mode="NONE", option=True):
    """Make with the variable set (or unset) — it is read at Make only"""
    if option:
        monkeypatch.setenv("GDV_UTF8_CASE", "1")
    else:
        monkeypatch.delenv("GDV_UTF8_CASE", raising=False)
    try:
        return gandiva.make_projector(schema, exprs, pa.default_memory_pool(), mode)
    finally:
        monkeypatch.delenv("GDV_UTF8_CASE", raising=False)


def _batch(n, seed):
    s = pa.array(R.batch_rows(n, seed), STR)
    t = pa.array(R.batch_rows(n, seed + 1000), STR)
    return pa.RecordBatch.from_arrays([s, t], names=["s", "t"])


def _same_buffers(got, want, what):
    """offsets, bytes and validity are equal (arrays without a slice offset)"""
    assert got.type == want.type and len(got) == len(want), what
    assert got.null_count == want.null_count, what
    if want.null_count:
        assert got.is_valid().equals(want.is_valid()), what
    go, gd = R.array_buffers(got)
    wo, wd = R.array_buffers(want)
    assert np.array_equal(go, wo), "%s: offsets differ first at row %s" % (what, np.flatnonzero(go != wo)[:4])
    assert np.array_equal(gd, wd), "%s: bytes differ first at byte %s" % (what, np.flatnonzero(gd != wd)[:4])


@pytest.mark.parametrize("n", [1, 257, 4099])
def test_row_mode_matches_utf8proc(monkeypatch, n):
    batch = _batch(n, seed=n)
    t = T(batch.schema)
    s = t.f["s"]
    exprs = [t.expr(t.up(s), "up"), t.expr(t.lo(s), "lo"),
             t.expr(t.fn("concat", [t.up(s), t.lit("-"), t.lo(s)]), "cat"),
             t.expr(t.up(t.fn("substr", [s, t.lit(2, I64), t.lit(5, I64)])), "up_sub")]
    got = _make(monkeypatch, batch.schema, exprs).evaluate(batch)
    col = batch.column(0)
    up, lo = pc.utf8_upper(col), pc.utf8_lower(col)
    cat = pa.array([(u or "") + "-" + (l or "") for u, l in zip(up.to_pylist(), lo.to_pylist())], STR)
    assert_bit_exact(got[0], up, f"upper n={n}")
    assert_bit_exact(got[1], lo, f"lower n={n}")
    assert_bit_exact(got[2], cat, f"concat n={n}")
    assert_bit_exact(got[3], pc.utf8_upper(pc.utf8_slice_codeunits(col, 1, 6)), f"upper(substr) n={n}")


def test_rows_that_grow_shrink_and_stay(monkeypatch):
    """every row of the first batch grows by half under upper (U+0250 -> U+2C6F), every row of the second halves (dotless i ->
    I), the third is pure ASCII; offsets, bytes and validity are equal to utf8proc's.  (Without the option — and on the parent
    commit — upper is the ASCII byte map and leaves the first two batches as they are.)"""
    rng = np.random.default_rng(7)
    lens = rng.integers(0, 20, 3001)
    ascii_rows = ["".join("abcXYZ 09-_"[int(k)] for k in rng.integers(0, 11, int(m))) for m in lens]
    for name, rows in (("grow", ["ɐ" * int(m) for m in lens]), ("shrink", ["ı" * int(m) for m in lens]), ("ascii", ascii_rows)):
        rows = [None if k % 10 == 3 else r for k, r in enumerate(rows)]
        batch = pa.RecordBatch.from_arrays([pa.array(rows, STR)], names=["s"])
        t = T(batch.schema)
        got, = _make(monkeypatch, batch.schema, [t.expr(t.up(t.f["s"]), "up")]).evaluate(batch)
        want = pc.utf8_upper(batch.column(0))
        assert_bit_exact(got, want, name)
        # the same rows without nulls: the buffers themselves
        dense = pa.RecordBatch.from_arrays([pa.array([r for r in rows if r is not None], STR)], names=["s"])
        got, = _make(monkeypatch, dense.schema, [t.expr(t.up(t.f["s"]), "up")]).evaluate(dense)
        _same_buffers(got, pc.utf8_upper(dense.column(0)), name)
        if name != "ascii":
            assert pc.sum(pc.binary_length(got)).as_py() != pc.sum(pc.binary_length(dense.column(0))).as_py()


def test_every_code_point(monkeypatch):
    off, data = R.all_code_points()
    col = R.string_array(off, data)
    assert len(col) == 1_112_064
    batch = pa.RecordBatch.from_arrays([col], names=["s"])
    t = T(batch.schema)
    up, lo = _make(monkeypatch, batch.schema, [t.expr(t.up(t.f["s"]), "up"), t.expr(t.lo(t.f["s"]), "lo")]).evaluate(batch)
    _same_buffers(up, pc.utf8_upper(col), "upper")
    _same_buffers(lo, pc.utf8_lower(col), "lower")


@pytest.mark.parametrize("mode,dtype", [("UINT16", "int16"), ("UINT32", "int32")])
def test_selection_mode(monkeypatch, mode, dtype):
    n = 20_011
    batch = _batch(n, seed=11)
    t = T(batch.schema)
    s = t.f["s"]
    flt = gandiva.make_filter(batch.schema, t.b.make_condition(t.fn("like", [s, t.lit("%a%")], BOOL)))
    sel = flt.evaluate(batch, pa.default_memory_pool(), dtype)
    idx = sel.to_array().to_numpy()
    assert 0 < len(idx) < n
    proj = _make(monkeypatch, batch.schema, [t.expr(t.lo(s), "lo"), t.expr(t.fn("concat", [t.up(s), t.lit("|")]), "cat")], mode)
    lo, cat = proj.evaluate(batch, sel)
    taken = batch.column(0).take(pa.array(idx))
    assert_bit_exact(lo, pc.utf8_lower(taken), "lower over a selection")
    assert_bit_exact(cat, pa.array([(u or "") + "|" for u in pc.utf8_upper(taken).to_pylist()], STR), "concat over a selection")


def test_staged_consumers_sync_and_async(monkeypatch):
    import torch
    n = 10_007
    batch = _batch(n, seed=13)
    t = T(batch.schema)
    a, b = t.f["s"], t.f["t"]
    exprs = [t.expr(t.fn("like", [t.up(a), t.lit("%É%")], BOOL), "like_up", BOOL),
             t.expr(t.fn("equal", [t.lo(a), t.lo(b)], BOOL), "eq_lo", BOOL),
             t.expr(t.up(t.lo(a)), "up_lo"),
             t.expr(t.fn("substr", [t.up(a), t.lit(1, I64), t.lit(3, I64)]), "sub_up")]
    # (two rows that are equal only after the whole map: the ASCII map would not make them so)
    fixed = pa.RecordBatch.from_arrays([pa.array(["Straße É", "ǅ"] + batch.column(0).to_pylist()[2:], STR),
                                        pa.array(["STRAßE é", "ǆ"] + batch.column(1).to_pylist()[2:], STR)], names=["s", "t"])
    proj = _make(monkeypatch, fixed.schema, exprs)
    ca, cb = fixed.column(0), fixed.column(1)
    want = [pc.match_like(pc.utf8_upper(ca), "%É%"), pc.equal(pc.utf8_lower(ca), pc.utf8_lower(cb)), pc.utf8_upper(pc.utf8_lower(ca)),
            pc.utf8_slice_codeunits(pc.utf8_upper(ca), 0, 3)]
    assert want[1][0].as_py() is True and want[1][1].as_py() is True and pc.sum(want[0].cast(pa.int32())).as_py() > 100
    got = proj.evaluate(fixed)
    for g, w, e in zip(got, want, exprs):
        assert_bit_exact(g, w, "staged, synchronous")
    db = gandiva.DeviceBatch.from_arrow(fixed)
    cap = 64 + 8 * sum(c.data.numel() for c in db.columns if c.offsets is not None)
    outs, result = proj.evaluate_device_async(db, capacity_bytes=cap)
    torch.cuda.synchronize()
    assert int(result[0].item()) == 0
    for o, w in zip(outs, want):
        assert_bit_exact(o.to_arrow(), w, "staged, asynchronous")


def _with_row(col, at, raw, null=False):
    """the string column with row `at` replaced by the bytes `raw` (which need not be UTF-8), null or not"""
    rows = [None if v is None else v.encode() for v in col.to_pylist()]
    rows[at] = raw
    off, data, valid = R.rows_to_buffers(rows)
    if null:
        valid[at] = 0
    bitmap = np.packbits(valid.astype(bool), bitorder="little")
    return pa.StringArray.from_buffers(len(rows), pa.py_buffer(off), pa.py_buffer(data), pa.py_buffer(bitmap))


def test_a_row_that_is_not_utf8_raises_a_null_or_guarded_one_does_not(monkeypatch):
    n, at = 4099, 3000
    base = _batch(n, seed=17).column(0)
    guard = pa.array([None if k == at else 1 for k in range(n)], I32)
    schema = pa.schema([pa.field("s", STR), pa.field("g", I32)])
    t = T(schema)
    s, g = t.f["s"], t.f["g"]
    plain = _make(monkeypatch, schema, [t.expr(t.up(s), "up"), t.expr(t.lo(s), "lo")])
    guarded = _make(monkeypatch, schema, [t.expr(t.b.make_if(t.fn("isnotnull", [g], BOOL), t.up(s), t.b.make_null(STR), STR), "up")])
    bad = pa.RecordBatch.from_arrays([_with_row(base, at, b"\xe2\x82"), guard], schema=schema)
    with pytest.raises(gandiva.GandivaError, match=r"invalid argument \(upper / lower under GDV_UTF8_CASE=1"):
        plain.evaluate(bad)
    # the same bytes in a null row: nothing raises; the next evaluation of the projector that raised is right
    nulled = pa.RecordBatch.from_arrays([_with_row(base, at, b"\xe2\x82", null=True), guard], schema=schema)
    up, lo = plain.evaluate(nulled)
    assert_bit_exact(up, pc.utf8_upper(_with_row(base, at, b"", null=True)), "upper, the bad bytes in a null row")
    assert_bit_exact(lo, pc.utf8_lower(_with_row(base, at, b"", null=True)), "lower, the bad bytes in a null row")
    # guarded: the row is skipped (null), every other row is mapped
    up, = guarded.evaluate(bad)
    assert_bit_exact(up, pc.utf8_upper(_with_row(base, at, b"", null=True)), "upper under if (isnotnull(g))")


def test_the_option_unset_in_the_same_process_is_still_the_ascii_map(monkeypatch):
    n = 4099
    batch = _batch(n, seed=19)
    t = T(batch.schema)
    e = [t.expr(t.up(t.f["s"]), "up"), t.expr(t.lo(t.f["s"]), "lo")]
    col = batch.column(0)
    with_it = _make(monkeypatch, batch.schema, e).evaluate(batch)
    without = _make(monkeypatch, batch.schema, e, option=False).evaluate(batch)
    again = _make(monkeypatch, batch.schema, e).evaluate(batch)
    assert_bit_exact(without[0], pc.ascii_upper(col), "upper, option unset")
    assert_bit_exact(without[1], pc.ascii_lower(col), "lower, option unset")
    for got in (with_it, again):
        assert_bit_exact(got[0], pc.utf8_upper(col), "upper, option set")
        assert_bit_exact(got[1], pc.utf8_lower(col), "lower, option set")
    assert not without[0].equals(with_it[0])


def test_the_option_through_the_cxx_api():
    cxx = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gandiva_amd", "cxx")
    subprocess.check_call(["make", "-C", cxx, "all", "test_cxx"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(cxx, "tests", "test_utf8_case_cxx")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
