"""regexp_extract on the GPU, through the C ABI (the gandiva_amd Python mirror): offsets, data and validity bit-exact
against RE2 itself (pyarrow.compute.extract_regex), with the patterns, texts and the RE2 wrapper of
tests/test_regexp_extract_cpu.py.

PARITY STATUS: 2-engines for the extents (PARITY.md, regexp_extract)."""
import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import gandiva_amd as gandiva
from helpers import assert_bit_exact
import test_regexp_extract_cpu as R

STR, I32 = pa.string(), pa.int32()
pytestmark = pytest.mark.gpu

LONG = [b"x" * 130 + "é€".encode() * 20 + b" id=4711 k=spark; bob@example.org " + b"y" * 150,
        b"a" * 257 + b"b", "🙂".encode() * 70 + b"aab=c"]


def _patterns():
    """24 (pattern, index): every hand vector once, the rest from the random corpus — three projectors of eight"""
    out = []
    for case, (pattern, texts) in enumerate(R.HAND):
        groups = len(R._group_names(pattern))
        out.append((pattern, case % (groups + 1)))
    rng = np.random.default_rng(77)
    for pattern, texts, want in R.fuzz_corpus(count=40, seed=4242):
        if len(out) == 24:
            break
        if R.compile_table(pattern, 0)[0] is not None:
            out.append((pattern, int(rng.integers(0, len(want[0]) + 1))))
    assert len(out) == 24
    return out


def _pool():
    """texts the patterns find something in: the hand vectors', the corpus', empty, multi-byte and beyond 256 bytes"""
    pool = [b""] + LONG
    for _, texts in R.HAND:
        pool += texts
    for _, texts, _ in R.fuzz_corpus(count=40, seed=4242):
        pool += texts
    return pool


@pytest.fixture(scope="module")
def packed():
    """(patterns, the three projectors over them, the text pool)"""
    patterns = _patterns()
    schema = pa.schema([pa.field("s", STR)])
    b = gandiva.TreeExprBuilder()
    s = b.make_field(schema.field(0))
    projectors = []
    for at in range(0, 24, 8):
        exprs = [b.make_expression(b.make_function("regexp_extract", [s, b.make_literal(p, STR), b.make_literal(i, I32)], STR),
                                   pa.field(f"o{at + j}", STR)) for j, (p, i) in enumerate(patterns[at:at + 8])]
        projectors.append(gandiva.make_projector(schema, exprs, pa.default_memory_pool()))
    return patterns, projectors, _pool()


def _column(pool, rows, nulls, offset, seed):
    rng = np.random.default_rng(seed)
    texts = [pool[int(rng.integers(0, len(pool)))] for _ in range(rows + offset)]
    texts[0] = LONG[0]  # (every batch holds a row beyond 256 bytes, also behind the offset)
    texts[-1] = LONG[1]
    vals = [None if rng.random() < nulls else t.decode() for t in texts]
    return pa.array(vals, STR).slice(offset, rows)


def _expected(pattern, index, column):
    """RE2's answer for the column: null where the text is null"""
    vals = column.to_pylist()
    texts = [b"" if v is None else v.encode() for v in vals]
    want = R.re2_groups(pattern, texts)
    return pa.array([None if v is None else w[max(index - 1, 0)].decode() for v, w in zip(vals, want)], STR)


CASES = [(rows, nulls, 0) for rows in (1, 63, 64, 65, 1023, 1025, 3000) for nulls in (0.0, 0.1, 1.0)] + \
        [(1025, 0.1, offset) for offset in (1, 63, 65)]


@pytest.mark.parametrize("rows, nulls, offset", CASES)
def test_projection_is_bit_exact_against_re2(packed, rows, nulls, offset):
    patterns, projectors, pool = packed
    column = _column(pool, rows, nulls, offset, seed=rows * 7 + int(nulls * 10) + offset)
    batch = pa.RecordBatch.from_arrays([column], names=["s"])
    for k, proj in enumerate(projectors):
        got = proj.evaluate(batch)
        for (pattern, index), g in zip(patterns[8 * k:8 * k + 8], got):
            assert_bit_exact(g, _expected(pattern, index, column), f"{pattern!r} index {index} rows {rows} nulls {nulls} offset {offset}")


def test_null_literals_give_an_all_null_column():
    schema = pa.schema([pa.field("s", STR)])
    b = gandiva.TreeExprBuilder()
    s = b.make_field(schema.field(0))
    exprs = [b.make_expression(b.make_function("regexp_extract", [s, b.make_null(STR), b.make_literal(0, I32)], STR), pa.field("a", STR)),
             b.make_expression(b.make_function("regexp_extract", [s, b.make_literal("(a)", STR), b.make_null(I32)], STR), pa.field("b", STR))]
    batch = pa.RecordBatch.from_arrays([pa.array(["a", None, "xa", ""] * 20, STR)], names=["s"])
    for g in gandiva.make_projector(schema, exprs, pa.default_memory_pool()).evaluate(batch):
        assert_bit_exact(g, pa.array([None] * 80, STR), "null literal")


def _keyed_batch(rows, seed):
    """rows that all hold an id and a key: 'noise id=<digits> k=<word>; noise' (castINT of "" would raise)"""
    rng = np.random.default_rng(seed)
    words = ["spark", "sparks", "flink", "v", "é"]
    vals = []
    for _ in range(rows):
        if rng.random() < 0.1:
            vals.append(None)
            continue
        lead = R._noise(rng, int(rng.integers(0, 6))).decode().replace("=", "-")
        vals.append(f"{lead} id={int(rng.integers(0, 10**9))} k={words[int(rng.integers(0, len(words)))]}; " + "y" * int(rng.integers(0, 4)))
    return pa.RecordBatch.from_arrays([pa.array(vals, STR)], names=["s"])


def test_selection_mode_filter_and_cast_on_host_and_device_batches():
    import torch
    rows = 5003
    batch = _keyed_batch(rows, seed=11)
    column = batch.column(0)
    schema = batch.schema
    b = gandiva.TreeExprBuilder()
    s = b.make_field(schema.field(0))

    def extract(pattern, index):
        return b.make_function("regexp_extract", [s, b.make_literal(pattern, STR), b.make_literal(index, I32)], STR)
    ids = _expected("(?P<g0>id=(?P<g1>\\d+))", 2, column)
    keys = _expected("(?P<g0>k=(?P<g1>\\w+))", 2, column)
    db = gandiva.DeviceBatch.from_arrow(batch)

    # a filter on the extracted key
    cond = b.make_condition(b.make_function("equal", [extract("k=(\\w+)", 1), b.make_literal("spark", STR)], pa.bool_()))
    flt = gandiva.make_filter(schema, cond)
    want_idx = pc.indices_nonzero(pc.fill_null(pc.equal(keys, "spark"), False)).to_pylist()
    assert 0 < len(want_idx) < rows
    for dtype in ("int16", "int32"):
        assert flt.evaluate(batch, pa.default_memory_pool(), dtype).to_array().to_pylist() == want_idx
        assert flt.evaluate_device(db, dtype).to_array().to_pylist() == want_idx

    # castINT and length of the slice, and the slice itself
    exprs = [b.make_expression(b.make_function("castINT", [extract("id=(\\d+)", 1)], I32), pa.field("i", I32)),
             b.make_expression(b.make_function("length", [extract("k=(\\w+)", 1)], I32), pa.field("n", I32)),
             b.make_expression(extract("k=(\\w+)", 1), pa.field("k", STR))]
    want = [pa.array([None if v is None else int(v) for v in ids.to_pylist()], I32),
            pa.array([None if v is None else len(v) for v in keys.to_pylist()], I32), keys]
    proj = gandiva.make_projector(schema, exprs, pa.default_memory_pool())
    for name, got in (("host", proj.evaluate(batch)), ("device", [o.to_arrow() for o in proj.evaluate_device(db)])):
        for g, w in zip(got, want):
            assert_bit_exact(g, w, f"row mode, {name} batch")

    # the same expressions over the filter's selection, 16- and 32-bit indices
    take = pa.array(want_idx)
    for mode, dtype in (("UINT16", "int16"), ("UINT32", "int32")):
        psel = gandiva.make_projector(schema, exprs, pa.default_memory_pool(), mode)
        sel = flt.evaluate(batch, pa.default_memory_pool(), dtype)
        dsel = flt.evaluate_device(db, dtype)
        outs = psel.evaluate_device(db, selection=dsel)
        torch.cuda.synchronize()
        for name, got in (("host", psel.evaluate(batch, sel)), ("device", [o.to_arrow() for o in outs])):
            for g, w in zip(got, want):
                assert_bit_exact(g, w.take(take), f"selection mode {mode}, {name} batch")
