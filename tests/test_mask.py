"""mask, mask_first_n, mask_last_n, mask_show_first_n, mask_show_last_n on the GPU, through the C ABI (the gandiva_amd Python
mirror).

PARITY STATUS (PARITY.md, `mask`): recollection + decisions; no second engine knows these functions.  Every expected value is
what the plain-Python restatement of tests/test_mask_cpu.py gives (checked there against re.sub, str slicing and
pyarrow.compute.utf8_length); the rows are its edge rows: every length around the 8-byte word, characters across the word
boundaries, continuation bytes only, rows that end in a cut character."""
import os
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import gandiva_amd as gandiva
from helpers import assert_bit_exact
import test_mask_cpu as R

STR, BOOL, I32, BIN = pa.string(), pa.bool_(), pa.int32(), pa.binary()
pytestmark = pytest.mark.gpu

N_POOL = [R.INT32_MIN, -1, 0, 1, 3, 7, 8, 9, 20, 70, R.INT32_MAX]
LITERAL_N = 4


def _strings(rows):
    """a string column of the given bytes (None: null), which need not be UTF-8"""
    return pa.array(rows, BIN).view(STR)


def _pool(ascii_only):
    if ascii_only:
        return [R._fill(L, sh) for L in R.LENGTHS for sh in (0, 3, 7)]
    return R.edge_rows()


def _batch(n, nulls, ascii_only, seed):
    """n rows drawn from the pool, a row beyond 256 bytes at the first and the last position, `nulls` of the rows null; k: the
    per-row n, null in a tenth of the rows when the batch has nulls at all"""
    rng = np.random.default_rng(seed)
    pool = _pool(ascii_only)
    long_rows = [r for r in pool if len(r) > 256]
    rows = [pool[int(i)] for i in rng.integers(0, len(pool), n)]
    rows[0] = long_rows[seed % len(long_rows)]
    rows[-1] = long_rows[(seed + 5) % len(long_rows)]
    assert len(rows[0]) > 256 and len(rows[-1]) > 256
    s = [None if rng.random() < nulls else r for r in rows]
    k = [None if nulls > 0 and rng.random() < 0.1 else N_POOL[int(i)] for i in rng.integers(0, len(N_POOL), n)]
    return pa.RecordBatch.from_arrays([_strings(s), pa.array(k, I32)], names=["s", "k"])


SCH = pa.schema([pa.field("s", STR), pa.field("k", I32)])


def _twelve(t):
    """(name, tree, function, n: 'literal' | 'column' | None, replacements): the eight signatures, the n forms twice"""
    s, k = t.f["s"], t.f["k"]
    out = [("m1", t.fn("mask", [s]), "mask", None, b"Xxn"),
           ("m2", t.fn("mask", [s, t.lit("U")]), "mask", None, b"Uxn"),
           ("m3", t.fn("mask", [s, t.lit("U"), t.lit("l")]), "mask", None, b"Uln"),
           ("m4", t.fn("mask", [s, t.lit("U"), t.lit("l"), t.lit("#")]), "mask", None, b"Ul#")]
    for f in R.N_FORMS:
        out.append((f + "_lit", t.fn(f, [s, t.lit(LITERAL_N, I32)]), f, "literal", b"Xxn"))
    for f in R.N_FORMS:
        out.append((f + "_col", t.fn(f, [s, k]), f, "column", b"Xxn"))
    return out


def _want(batch, fn, n_from, reps, text_map=0):
    s = batch.column(0).cast(BIN).to_pylist()
    k = batch.column(1).to_pylist() if n_from == "column" else [LITERAL_N] * len(s)
    return _strings([None if x is None or n is None else R.restate(fn, x, n, reps, text_map) for x, n in zip(s, k)])


@pytest.fixture(scope="module")
def twelve():
    t = R.T(SCH)
    cases = _twelve(t)
    proj = gandiva.make_projector(SCH, [t.expr(e, name) for name, e, _, _, _ in cases], pa.default_memory_pool())
    return proj, cases


def _check_projection(twelve, batch, what):
    proj, cases = twelve
    got = proj.evaluate(batch)
    assert len(got) == 12
    for (name, _, fn, n_from, reps), g in zip(cases, got):
        want = _want(batch, fn, n_from, reps)
        assert_bit_exact(g, want, f"{name} {what}")
        if batch.column(0).null_count == 0 and n_from != "column":   # the length is the text's: the offsets are the input's
            assert pc.binary_length(g).equals(pc.binary_length(batch.column(0))), f"{name} {what}: offsets"


@pytest.mark.parametrize("ascii_only", [True, False], ids=["ascii", "mixed"])
@pytest.mark.parametrize("nulls", [0, 0.1, 1.0])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1025, 3000])
def test_projection_matches_the_restatement(twelve, n, nulls, ascii_only):
    batch = _batch(n, nulls, ascii_only, seed=n + int(nulls * 10))
    _check_projection(twelve, batch, f"n={n} nulls={nulls} ascii={ascii_only}")


@pytest.mark.parametrize("ascii_only", [True, False], ids=["ascii", "mixed"])
@pytest.mark.parametrize("offset", [1, 63, 65])
def test_sliced_batches(twelve, offset, ascii_only):
    whole = _batch(1025 + offset, 0.1, ascii_only, seed=offset)
    batch = whole.slice(offset)
    assert batch.num_rows == 1025 and batch.column(0).offset == offset
    _check_projection(twelve, batch, f"slice at {offset} ascii={ascii_only}")


def _card_batch(n, seed):
    """edge rows up to 257 bytes, and every third row a card number whose last four digits come from a small set"""
    rng = np.random.default_rng(seed)
    pool = [r for r in R.edge_rows() if len(r) <= 257]
    rows = [pool[int(i)] for i in rng.integers(0, len(pool), n)]
    for i in range(0, n, 3):
        rows[i] = b"Card %04d-%04d-%04d-%04d" % (int(rng.integers(0, 10000)), int(rng.integers(0, 10000)), int(rng.integers(0, 10000)),
                                                  (42, 7, 1234)[int(rng.integers(0, 3))])
    s = [None if rng.random() < 0.1 else r for r in rows]
    k = [N_POOL[int(i)] for i in rng.integers(0, len(N_POOL), n)]
    return pa.RecordBatch.from_arrays([_strings(s), pa.array(k, I32)], names=["s", "k"])


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("mode,dtype", [("UINT16", "int16"), ("UINT32", "int32")])
def test_selection_mode_behind_a_filter(mode, dtype, where):
    n = 4099
    batch = _card_batch(n, seed=21)
    t = R.T(SCH)
    cases = _twelve(t)
    flt = gandiva.make_filter(SCH, t.b.make_condition(t.fn("like", [t.f["s"], t.lit("%a%")], BOOL)))
    proj = gandiva.make_projector(SCH, [t.expr(e, name) for name, e, _, _, _ in cases], pa.default_memory_pool(), mode)
    sel = flt.evaluate(batch, pa.default_memory_pool(), dtype)
    idx = sel.to_array().to_numpy()
    assert 0 < len(idx) < n
    taken = batch.take(pa.array(idx))
    if where == "host":
        got = proj.evaluate(batch, sel)
    else:
        db = gandiva.DeviceBatch.from_arrow(batch)
        got = [o.to_arrow() for o in proj.evaluate_device(db, selection=flt.evaluate_device(db, dtype))]
    for (name, _, fn, n_from, reps), g in zip(cases, got):
        assert_bit_exact(g, _want(taken, fn, n_from, reps), f"{name} {mode} {where}")


def test_a_filter_on_a_masked_value_then_a_selection_mode_projection():
    n = 4099
    batch = _card_batch(n, seed=22)
    t = R.T(SCH)
    s = t.f["s"]
    literal = "Xxxx nnnn-nnnn-nnnn-0042"
    flt = gandiva.make_filter(SCH, t.b.make_condition(t.fn("equal", [t.fn("mask_show_last_n", [s, t.lit(4, I32)]), t.lit(literal)], BOOL)))
    sel = flt.evaluate(batch, pa.default_memory_pool(), "int32")
    rows = batch.column(0).cast(BIN).to_pylist()
    want_idx = [i for i, r in enumerate(rows) if r is not None and R.restate("mask_show_last_n", r, 4) == literal.encode()]
    assert 100 < len(want_idx) < n // 3
    assert sel.to_array().to_pylist() == want_idx
    proj = gandiva.make_projector(SCH, [t.expr(t.fn("mask_show_last_n", [s, t.lit(4, I32)]), "o"), t.expr(t.fn("mask", [s]), "m")],
                                  pa.default_memory_pool(), "UINT32")
    shown, masked = proj.evaluate(batch, sel)
    assert shown.to_pylist() == [literal] * len(want_idx)
    assert masked.to_pylist() == ["Xxxx nnnn-nnnn-nnnn-nnnn"] * len(want_idx)


def test_staged_consumers_and_concat():
    n = 3001
    rng = np.random.default_rng(31)
    pool = [r for r in R.edge_rows() if R._is_utf8(r)]   # (the consumers have rules of their own for text that is not UTF-8)
    pool += [b"Qz" + r for r in pool if len(r) <= 257]   # (rows that 'Xx%' takes)
    rows = [None if rng.random() < 0.1 else pool[int(i)] for i in rng.integers(0, len(pool), n)]
    batch = pa.RecordBatch.from_arrays([_strings(rows), pa.array([1] * n, I32)], names=["s", "k"])
    t = R.T(SCH)
    s = t.f["s"]
    exprs = [t.expr(t.fn("like", [t.fn("mask", [s]), t.lit("Xx%")], BOOL), "like", BOOL),
             t.expr(t.fn("length", [t.fn("mask_first_n", [s, t.lit(3, I32)])], I32), "len", I32),
             t.expr(t.fn("upper", [t.fn("mask", [s])]), "up"),
             t.expr(t.fn("concat", [t.fn("mask", [s]), t.lit("-"), s]), "cat"),
             t.expr(t.fn("mask", [t.fn("upper", [s])]), "mask_up"),
             t.expr(t.fn("mask_last_n", [t.fn("lower", [s]), t.lit(9, I32)]), "last_lo")]
    got = gandiva.make_projector(SCH, exprs, pa.default_memory_pool()).evaluate(batch)
    m = [None if r is None else R.restate("mask", r) for r in rows]
    want = [pa.array([None if x is None else x.startswith(b"Xx") for x in m], BOOL),
            pc.utf8_length(_strings(rows)),
            _strings([None if x is None else x.upper() for x in m]),
            _strings([(b"" if x is None else x) + b"-" + (b"" if r is None else r) for x, r in zip(m, rows)]),
            _strings([None if r is None else R.restate("mask", r, text_map=1) for r in rows]),
            _strings([None if r is None else R.restate("mask_last_n", r, 9, text_map=2) for r in rows])]
    assert pc.sum(want[0].cast(I32)).as_py() > 100
    assert R.restate("mask", b"ab1", text_map=1) == b"XXn"
    for g, w, e in zip(got, want, ("like", "length", "upper", "concat", "mask(upper)", "mask_last_n(lower)")):
        assert_bit_exact(g, w, e)


def test_asynchronous_evaluation_of_device_batches():
    import torch
    batch = _batch(3000, 0.1, False, seed=41)
    t = R.T(SCH)
    s, k = t.f["s"], t.f["k"]
    proj = gandiva.make_projector(SCH, [t.expr(t.fn("mask", [s]), "m"), t.expr(t.fn("mask_show_first_n", [s, k]), "sf")],
                                  pa.default_memory_pool())
    db = gandiva.DeviceBatch.from_arrow(batch)
    cap = 64 + 8 * sum(c.data.numel() for c in db.columns if c.offsets is not None)
    outs, result = proj.evaluate_device_async(db, capacity_bytes=cap)
    torch.cuda.synchronize()
    assert int(result[0].item()) == 0
    assert_bit_exact(outs[0].to_arrow(), _want(batch, "mask", None, b"Xxn"), "mask, asynchronous")
    assert_bit_exact(outs[1].to_arrow(), _want(batch, "mask_show_first_n", "column", b"Xxn"), "mask_show_first_n, asynchronous")


def test_null_literals_give_all_null_columns():
    batch = _batch(65, 0, False, seed=51)
    t = R.T(SCH)
    s = t.f["s"]
    null_s, null_n = t.b.make_null(STR), t.b.make_null(I32)
    got = gandiva.make_projector(SCH, [t.expr(t.fn("mask", [s, null_s]), "a"), t.expr(t.fn("mask", [s, t.lit("U"), t.lit("l"), null_s]), "b"),
                                       t.expr(t.fn("mask_first_n", [s, null_n]), "c"), t.expr(t.fn("mask", [s]), "d")],
                                 pa.default_memory_pool()).evaluate(batch)
    for g in got[:3]:
        assert g.type == STR and len(g) == 65 and g.null_count == 65
    assert_bit_exact(got[3], _want(batch, "mask", None, b"Xxn"), "mask next to the null columns")


def test_mask_through_the_cxx_api():
    cxx = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gandiva_amd", "cxx")
    subprocess.check_call(["make", "-C", cxx, "all", "test_cxx"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(cxx, "tests", "test_mask_cxx")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
