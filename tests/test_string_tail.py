"""String tail on the GPU: split_part, substring_index, repeat, space and translate through the C ABI (the gandiva_amd
Python mirror), bit-exact against the plain-Python restatement of tests/test_string_tail_cpu.py.

PARITY STATUS: recollection (PARITY.md, string tail); the oracle does not know these functions."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import gandiva_amd as gandiva
from gandiva_amd import _capi, gandiva as gg, workloads as W
from helpers import assert_bit_exact
import test_string_tail_cpu as R

STR, I32, I64 = pa.string(), pa.int32(), pa.int64()
pytestmark = pytest.mark.gpu

ASCII_PIECES = ["a", "b", "/", ",", "@", "x", "A", "B", " ", "spark", ".org", "ab", "//"]
WIDE_PIECES = ["é", "€", "🙂", "ü"]
DELIMS = ["/", ",", "@", "ab", "é", "", "//"]


def _texts(rng, n, non_ascii):
    out = []
    for _ in range(n):
        m = int(rng.integers(0, 12)) if rng.random() < 0.97 else int(rng.integers(0, 60))
        wide = rng.random() < non_ascii
        pieces = ASCII_PIECES + WIDE_PIECES if wide else ASCII_PIECES
        t = "".join(pieces[int(rng.integers(0, len(pieces)))] for _ in range(m))
        if wide and not any(ord(c) > 127 for c in t):
            t += WIDE_PIECES[int(rng.integers(0, len(WIDE_PIECES)))]
        out.append(t)
    return out


def _batch(n, non_ascii, seed, offset=3, nulls=0.15):
    """columns s (text), d (per-row delimiter), k (per-row index / count), r (per-row repeat count), with 15 % nulls each
    and a nonzero array offset"""
    rng = np.random.default_rng(seed)
    m = n + offset

    def nullify(vals):
        return [None if rng.random() < nulls else v for v in vals]
    s = pa.array(nullify(_texts(rng, m, non_ascii)), STR)
    d = pa.array(nullify([DELIMS[int(rng.integers(0, len(DELIMS)))] for _ in range(m)]), STR)
    k = pa.array(nullify([int(rng.integers(1, 6)) for _ in range(m)]), I32)
    c = pa.array(nullify([int(rng.integers(-5, 6)) or 1 for _ in range(m)]), I32)
    r = pa.array(nullify([int(rng.integers(0, 5)) for _ in range(m)]), I32)
    cols = [a.slice(offset, n) for a in (s, d, k, c, r)]
    return pa.RecordBatch.from_arrays(cols, names=["s", "d", "k", "c", "r"])


def _enc(v):
    return None if v is None else v.encode()


def _expect(fn, *cols):
    """row-wise restatement; None when any argument is None (null if null)"""
    out = []
    for args in zip(*cols):
        if any(a is None for a in args):
            out.append(None)
        else:
            out.append(fn(*args).decode())
    return pa.array(out, STR)


class T:
    def __init__(self, schema):
        self.b = gandiva.TreeExprBuilder()
        self.f = {f.name: self.b.make_field(f) for f in schema}

    def lit(self, v, t=STR):
        return self.b.make_literal(v, t)

    def fn(self, name, args, t=STR):
        return self.b.make_function(name, args, t)

    def expr(self, node, name, t=STR):
        return self.b.make_expression(node, pa.field(name, t))


def _cases(t, big):
    """(name, tree, expected(batch)) of the projection"""
    s, d, k, c, r = (t.f[x] for x in "sdkcr")
    out = [("split_lit", t.fn("split_part", [s, t.lit("/"), t.lit(2, I32)]),
            lambda col: _expect(lambda x: R.split_part(x, b"/", 2), col("s"))),
           ("subidx_lit", t.fn("substring_index", [s, t.lit("@"), t.lit(-1, I32)]),
            lambda col: _expect(lambda x: R.substring_index(x, b"@", -1), col("s"))),
           ("translate_ascii", t.fn("translate", [s, t.lit("ab/"), t.lit("BA")]),
            lambda col: _expect(lambda x: R.translate(x, b"ab/", b"BA"), col("s")))]
    if big:
        return out
    return out + [
        ("split_row", t.fn("split_part", [s, d, k]),
         lambda col: _expect(R.split_part, col("s"), col("d"), col("k"))),
        ("subidx_row", t.fn("substring_index", [s, d, c]),
         lambda col: _expect(R.substring_index, col("s"), col("d"), col("c"))),
        ("split_upper", t.fn("split_part", [t.fn("upper", [s]), t.lit("B"), t.lit(2, I32)]),
         lambda col: _expect(lambda x: R.split_part(R.ascii_upper(x), b"B", 2), col("s"))),
        ("repeat_lit", t.fn("repeat", [s, t.lit(3, I32)]),
         lambda col: _expect(lambda x: R.repeat(x, 3), col("s"))),
        ("repeat_row", t.fn("repeat", [t.fn("lower", [s]), r]),
         lambda col: _expect(lambda x, y: R.repeat(R.ascii_lower(x), y), col("s"), col("r"))),
        ("space32", t.fn("space", [r]), lambda col: _expect(R.space, col("r"))),
        ("space64", t.fn("space", [t.fn("castBIGINT", [c], I64)]), lambda col: _expect(R.space, col("c"))),
        ("translate_wide", t.fn("translate", [s, t.lit("aé€/"), t.lit("ü1")]),
         lambda col: _expect(lambda x: R.translate(x, "aé€/".encode(), "ü1".encode()), col("s"))),
        ("translate_upper", t.fn("translate", [t.fn("upper", [s]), t.lit("AB"), t.lit("ba")]),
         lambda col: _expect(lambda x: R.translate(R.ascii_upper(x), b"AB", b"ba"), col("s"))),
        ("concat_translate", t.fn("concat", [t.fn("translate", [s, t.lit("x"), t.lit("yy")]), t.lit("|"), t.fn("space", [r])]),
         lambda col: pa.array([(("" if x is None else R.translate(x, b"x", b"yy").decode()) + "|" +
                                ("" if y is None else " " * max(y, 0))) for x, y in zip(col("s"), col("r"))], STR)),
    ]


def _columns(batch):
    py = {name: batch.column(i).to_pylist() for i, name in enumerate(batch.schema.names)}

    def col(name):
        v = py[name]
        return [_enc(x) for x in v] if name in ("s", "d") else v
    return col


SIZES = [(1, 0.0), (63, 0.3), (64, 0.01), (65, 0.3), (4096 + 13, 0.0), (4096 + 13, 0.01), (4096 + 13, 0.3),
         (2**20 + 7, 0.01)]


@pytest.mark.parametrize("n,non_ascii", SIZES)
def test_projection_matches_the_restatement(n, non_ascii):
    batch = _batch(n, non_ascii, seed=n + int(non_ascii * 100))
    t = T(batch.schema)
    cases = _cases(t, big=n > 100_000)
    proj = gandiva.make_projector(batch.schema, [t.expr(e, name) for name, e, _ in cases], pa.default_memory_pool())
    got = proj.evaluate(batch)
    col = _columns(batch)
    for (name, _, want), g in zip(cases, got):
        assert_bit_exact(g, want(col), f"{name} n={n} non-ascii={non_ascii}")


def test_filters_on_split_part_and_substring_index():
    n = 20_011
    batch = _batch(n, 0.01, seed=5)
    t = T(batch.schema)
    s, d, k = t.f["s"], t.f["d"], t.f["k"]
    col = _columns(batch)
    conds = [
        (t.fn("equal", [t.fn("split_part", [s, t.lit("/"), t.lit(2, I32)]), t.lit("a")], pa.bool_()),
         lambda x: R.split_part(x, b"/", 2) == b"a", ["s"]),
        (t.fn("like", [t.fn("substring_index", [s, t.lit("@"), t.lit(-1, I32)]), t.lit("%.org")], pa.bool_()),
         lambda x: R.substring_index(x, b"@", -1).endswith(b".org"), ["s"]),
        (t.fn("equal", [t.fn("split_part", [s, d, k]), t.lit("b")], pa.bool_()),
         lambda x, y, z: R.split_part(x, y, z) == b"b", ["s", "d", "k"]),
    ]
    for node, pred, names in conds:
        mask = [None if any(a is None for a in args) else pred(*args) for args in zip(*[col(x) for x in names])]
        want = pc.indices_nonzero(pc.fill_null(pa.array(mask, pa.bool_()), False))
        sel = gandiva.make_filter(batch.schema, t.b.make_condition(node)).evaluate(batch, pa.default_memory_pool(), "int32")
        assert sel.to_array().to_pylist() == want.to_pylist()


def test_filter_then_selection_mode_projector_sync_and_async():
    import torch
    n = 30_007
    batch = _batch(n, 0.3, seed=6)
    t = T(batch.schema)
    s, r = t.f["s"], t.f["r"]
    cond = t.b.make_condition(t.fn("like", [t.fn("split_part", [s, t.lit("/"), t.lit(1, I32)]), t.lit("%a%")], pa.bool_()))
    cases = _cases(t, big=False)
    exprs = [t.expr(e, name) for name, e, _ in cases]
    flt = gandiva.make_filter(batch.schema, cond)
    sel = flt.evaluate(batch, pa.default_memory_pool(), "int32")
    idx = sel.to_array().to_numpy()
    assert 0 < len(idx) < n
    taken = batch.take(pa.array(idx))
    col = _columns(taken)
    want = [w(col) for _, _, w in cases]
    psel = gandiva.make_projector(batch.schema, exprs, pa.default_memory_pool(), "UINT32")
    for (name, _, _), g, w in zip(cases, psel.evaluate(batch, sel), want):
        assert_bit_exact(g, w, f"selection mode, {name}")
    db = gandiva.DeviceBatch.from_arrow(batch)
    dsel = flt.evaluate_device(db, "int32")
    cap = 64 + 8 * sum(c.data.numel() for c in db.columns if c.offsets is not None)
    outs, result = psel.evaluate_device_async(db, selection=dsel, capacity_bytes=cap)
    torch.cuda.synchronize()
    assert int(result[0].item()) == 0
    for (name, _, _), o, w in zip(cases, outs, want):
        assert_bit_exact(o.to_arrow(), w, f"selection mode, asynchronous, {name}")


def test_staged_nestings():
    n = 10_007
    batch = _batch(n, 0.3, seed=7)
    t = T(batch.schema)
    s, r = t.f["s"], t.f["r"]
    col = _columns(batch)
    exprs = [t.expr(t.fn("upper", [t.fn("translate", [s, t.lit("abé"), t.lit("xy")])]), "up_tr"),
             t.expr(t.fn("length", [t.fn("repeat", [s, t.lit(3, I32)])], I32), "len_rep", I32),
             t.expr(t.fn("like", [t.fn("repeat", [s, r]), t.lit("%a/a%")], pa.bool_()), "like_rep", pa.bool_()),
             t.expr(t.fn("split_part", [t.fn("translate", [s, t.lit("@"), t.lit("/")]), t.lit("/"), t.lit(2, I32)]), "sp_tr")]
    got = gandiva.make_projector(batch.schema, exprs, pa.default_memory_pool()).evaluate(batch)
    S = col("s")
    assert_bit_exact(got[0], _expect(lambda x: R.ascii_upper(R.translate(x, "abé".encode(), b"xy")), S), "upper(translate)")
    assert_bit_exact(got[1], pa.array([None if x is None else len(R.repeat(x, 3).decode()) for x in S], I32), "length(repeat)")
    assert_bit_exact(got[2], pa.array([None if x is None or y is None else b"a/a" in R.repeat(x, y) for x, y in zip(S, col("r"))],
                                      pa.bool_()), "like(repeat)")
    assert_bit_exact(got[3], _expect(lambda x: R.split_part(R.translate(x, b"@", b"/"), b"/", 2), S), "split_part(translate)")


def test_error_rows_raise_and_the_next_evaluation_is_right():
    n = 5_003
    batch = _batch(n, 0.01, seed=8)
    t = T(batch.schema)
    s = t.f["s"]
    col = _columns(batch)
    good = t.expr(t.fn("split_part", [s, t.lit(","), t.lit(2, I32)]), "ok")
    for bad in (t.fn("split_part", [s, t.lit(","), t.lit(0, I32)]), t.fn("repeat", [s, t.lit(-1, I32)])):
        proj = gandiva.make_projector(batch.schema, [t.expr(bad, "bad"), good], pa.default_memory_pool())
        with pytest.raises(gandiva.GandivaError, match="invalid argument"):
            proj.evaluate(batch)
    # a per-row count that is negative on some rows only: the same projector is right on a batch without them
    r = t.f["c"]
    proj = gandiva.make_projector(batch.schema, [t.expr(t.fn("repeat", [s, r]), "rep"), good], pa.default_memory_pool())
    with pytest.raises(gandiva.GandivaError, match="invalid argument"):
        proj.evaluate(batch)
    pos = batch.filter(pc.fill_null(pc.greater_equal(batch.column(3), 0), True))
    pcol = _columns(pos)
    got = proj.evaluate(pos)
    assert_bit_exact(got[0], _expect(R.repeat, pcol("s"), pcol("c")), "repeat after an error")
    assert_bit_exact(got[1], _expect(lambda x: R.split_part(x, b",", 2), pcol("s")), "split_part after an error")
    del col


def test_one_tree_through_the_rebuilt_pyarrow_gandiva():
    from gandiva_amd import pyarrow_gandiva
    pg = pyarrow_gandiva.load()
    n = 4_099
    batch = _batch(n, 0.3, seed=9)
    b = pg.TreeExprBuilder()
    s = b.make_field(batch.schema.field("s"))
    e = b.make_function("substring_index", [b.make_function("translate", [s, b.make_literal("/", STR), b.make_literal("@", STR)],
                                                            STR), b.make_literal("@", STR), b.make_literal(2, I32)], STR)
    proj = pg.make_projector(batch.schema, [b.make_expression(e, pa.field("o", STR))], pa.default_memory_pool())
    got, = proj.evaluate(batch)
    want = _expect(lambda x: R.substring_index(R.translate(x, b"/", b"@"), b"@", 2), _columns(batch)("s"))
    assert got.equals(want)


def test_one_tree_through_make_from_proto():
    import proto_encode as P
    n = 4_099
    batch = _batch(n, 0.01, seed=10)
    t = T(batch.schema)
    s, k = t.f["s"], t.f["k"]
    exprs = [t.expr(t.fn("split_part", [s, t.lit("/"), k]), "sp"), t.expr(t.fn("repeat", [s, t.lit(2, I32)]), "rep"),
             t.expr(t.fn("translate", [s, t.lit("a"), t.lit("é")]), "tr")]
    lib = _capi.lib()
    sb, eb = P.schema(batch.schema), P.expression_list(exprs)
    ph = C.c_void_p()
    assert lib.gdv_projector_make_from_proto(sb, len(sb), eb, len(eb), 0, None, C.byref(ph)) == 0, _capi.last_error()
    got = gg.Projector(ph, batch.schema, 0, exprs).evaluate(batch)
    col = _columns(batch)
    assert_bit_exact(got[0], _expect(lambda x, y: R.split_part(x, b"/", y), col("s"), col("k")), "proto split_part")
    assert_bit_exact(got[1], _expect(lambda x: R.repeat(x, 2), col("s")), "proto repeat")
    assert_bit_exact(got[2], _expect(lambda x: R.translate(x, b"a", "é".encode()), col("s")), "proto translate")


def test_c5_column_at_ten_million_rows_two_windows():
    n = 10_000_000
    batch = W.c5_batch(n, 0.1, 0.01)
    t = T(batch.schema)
    s = t.f["s"]
    exprs = [t.expr(t.fn("split_part", [s, t.lit("a"), t.lit(2, I32)]), "sp"),
             t.expr(t.fn("translate", [s, t.lit("abcé"), t.lit("xyz")]), "tr")]
    got = gandiva.make_projector(batch.schema, exprs, pa.default_memory_pool()).evaluate(batch)
    for lo in (0, n - 50_000):
        window = batch.slice(lo, 50_000)
        S = [_enc(x) for x in window.column(0).to_pylist()]
        assert_bit_exact(got[0].slice(lo, 50_000), _expect(lambda x: R.split_part(x, b"a", 2), S), f"split_part window {lo}")
        assert_bit_exact(got[1].slice(lo, 50_000), _expect(lambda x: R.translate(x, "abcé".encode(), b"xyz"), S),
                         f"translate window {lo}")
