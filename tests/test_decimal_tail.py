"""The decimal tail on the GPU: castDECIMAL of float32 / float64 / text, castDECIMALNullOnOverflow, nvl / greatest / least,
is_distinct_from / is_not_distinct_from and hash / hash32 / hash64 over decimal128, through the C ABI (the Python mirror) and
once through the rebuilt pyarrow.gandiva.  Expected values: the plain-Python restatement of test_decimal_tail_cpu.py, bit for bit.

Row counts: 1 (one lane), 65 (a second 64-row sub-tile), 1025 (one row past a 16-sub-tile wave tile), 30 011 (many tiles, a
ragged tail).  Every column has 10 % nulls and starts 3 rows into its buffers, so no bitmap is aligned."""
import os
import subprocess

import numpy as np
import pyarrow as pa
import pytest

import gandiva_amd as gandiva
from gandiva_amd import gandiva as gg, workloads as W
from helpers import assert_bit_exact
from test_decimal_tail_cpu import (BOOL, D, F32, F64, I32, I64, STR, SCH, both, dec_of_float, dec_of_text, decimal_array,
                                   dense_decimals, every_signature_exprs, hash32_of, hash64_of, is_distinct, nvl_of,
                                   rescale_or_none, unscaled, valid_texts)

pytestmark = pytest.mark.gpu
ROWS = [1, 65, 1025, 30_011]
OFFSET = 3


def _nulls(rng, vals, fraction=0.1):
    return [None if rng.random() < fraction else v for v in vals]


def _sliced(vals, t):
    """a pyarrow array of vals that starts OFFSET rows into its buffers"""
    pad = {STR: "9"}.get(t, 1)
    return pa.array([pad] * OFFSET + list(vals), type=t).slice(OFFSET)


_BATCHES = {}


def _batch(n):
    """SCH's columns: s valid texts of 1-45 bytes, x / f floats of every magnitude, d / e decimal(15,2), g decimal(20,5),
    i / l seeds; computed once per row count and left unchanged"""
    if n in _BATCHES:
        return _BATCHES[n]
    rng = np.random.default_rng(1000 + n)
    texts = [t.decode() for t in valid_texts(rng, n)]
    x = np.concatenate([rng.integers(-10 ** 9, 10 ** 9, n - n // 2) / 8.0, rng.standard_normal(n // 2) * 10.0 ** rng.integers(-3, 18, n // 2)])
    x[:min(n, 6)] = [0.125, -0.125, np.nan, np.inf, 1e300, 0.49999999999999994][:min(n, 6)]
    f = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 12, n)).astype(np.float32)
    d = dense_decimals(rng, n, 15)
    e = [v if rng.random() < 0.3 else w for v, w in zip(d, dense_decimals(rng, n, 15))]
    g = [v * 1000 if rng.random() < 0.4 else w for v, w in zip(d, dense_decimals(rng, n, 20))]   # 40 % equal d by VALUE
    cols = {"s": _sliced(_nulls(rng, texts), STR), "x": _sliced(_nulls(rng, x.tolist()), F64), "f": _sliced(_nulls(rng, [float(v) for v in f]), F32),
            "d": decimal_array(_nulls(rng, d), D(15, 2), OFFSET), "e": decimal_array(_nulls(rng, e), D(15, 2), OFFSET),
            "g": decimal_array(_nulls(rng, g), D(20, 5), OFFSET), "i": _sliced(_nulls(rng, rng.integers(-2 ** 31, 2 ** 31, n).tolist()), I32),
            "l": _sliced(_nulls(rng, rng.integers(-2 ** 63, 2 ** 63 - 1, n).tolist()), I64)}
    _BATCHES[n] = pa.RecordBatch.from_arrays([cols[f.name] for f in SCH], schema=SCH)
    return _BATCHES[n]


def _col(batch, name):
    a = batch.column(batch.schema.get_field_index(name))
    return unscaled(a) if pa.types.is_decimal(a.type) else a.to_pylist()


def _lift(fn, *cols):
    """null if any argument is null"""
    return [None if any(a is None for a in args) else fn(*args) for args in zip(*cols)]


_EXPECTED = {}


def _expected(batch):
    """the restatement's column for each of every_signature_exprs' fourteen expressions, in order (computed once per batch)"""
    if batch.num_rows not in _EXPECTED:
        _EXPECTED[batch.num_rows] = _expected_columns(batch)
    return _EXPECTED[batch.num_rows]


def _expected_columns(batch):
    c = {f.name: _col(batch, f.name) for f in SCH}
    s = batch.column(0).cast(pa.binary()).to_pylist()
    return [_lift(lambda t: dec_of_text(t, 15, 2), s), _lift(lambda v: dec_of_float(v, 15, 2), c["x"]),
            _lift(lambda v: dec_of_float(v, 38, 10), c["f"]), _lift(lambda v: rescale_or_none(v, 5, 10, 2), c["g"]),
            [nvl_of(a, b) for a, b in zip(c["d"], c["e"])], [both(max)(a, b) for a, b in zip(c["d"], c["e"])],
            [both(min)(a, b) for a, b in zip(c["d"], c["e"])],
            [is_distinct(a, 2, b, 5) for a, b in zip(c["d"], c["g"])], [not is_distinct(a, 2, b, 5) for a, b in zip(c["d"], c["g"])],
            [hash32_of(v) for v in c["d"]], [hash32_of(v) for v in c["d"]], [hash64_of(v) for v in c["d"]],
            [hash32_of(v, k) for v, k in zip(c["d"], c["i"])], [hash64_of(v, k) for v, k in zip(c["d"], c["l"])]]


def _values(arr):
    return unscaled(arr) if pa.types.is_decimal(arr.type) else arr.to_pylist()


@pytest.mark.parametrize("family", ["cast", "pick", "distinct", "hash"])
@pytest.mark.parametrize("n", ROWS)
def test_one_projector_per_family(n, family):
    batch = _batch(n)
    b = gandiva.TreeExprBuilder()
    every = every_signature_exprs(b)
    pick = [k for k, (_, fam) in enumerate(every) if fam == family]
    got = gandiva.make_projector(SCH, [every[k][0] for k in pick], None).evaluate(batch)
    want = _expected(batch)
    for k, g in zip(pick, got):
        assert len(g) == n and _values(g) == want[k], (family, k, n)
    if family == "cast" and n >= 1025:
        assert sum(v is None for v in want[3]) > 0.05 * n and sum(v not in (None, 0) for v in want[3]) > 0.05 * n   # overflow -> NULL, and values
        assert sum(v not in (None, 0) for v in want[0]) > 0.3 * n
    if family in ("distinct", "hash"):
        assert all(g.null_count == 0 for g in got)


def _string_array(rows, valid):
    """utf8 array from raw buffers: a NULL row keeps its bytes"""
    n = len(rows)
    off = np.zeros(n + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(r) for r in rows])
    return pa.Array.from_buffers(STR, n, [pa.py_buffer(np.packbits(np.asarray(valid, dtype=bool), bitorder="little")), pa.py_buffer(off),
                                          pa.py_buffer(b"".join(rows) + b"\0" * 8)])


def test_an_invalid_text_raises_unless_its_row_is_null_or_guarded():
    n, at, bad = 1025, 777, b"12x.5"
    rng = np.random.default_rng(5)
    rows = valid_texts(rng, n)
    rows[at] = bad
    sch = pa.schema([pa.field("s", STR)])
    b = gandiva.TreeExprBuilder()
    s = b.make_field(sch.field(0))
    cast = b.make_function("castDECIMAL", [s], D(15, 2))
    proj = gandiva.make_projector(sch, [b.make_expression(cast, pa.field("o", D(15, 2)))], None)
    ones = np.ones(n, dtype=bool)
    with pytest.raises(gandiva.GandivaError, match="invalid argument"):
        proj.evaluate(pa.RecordBatch.from_arrays([_string_array(rows, ones)], schema=sch))
    # the same bytes in a NULL row: not parsed
    valid = ones.copy()
    valid[at] = False
    got, = proj.evaluate(pa.RecordBatch.from_arrays([_string_array(rows, valid)], schema=sch))
    assert unscaled(got) == [None if k == at else dec_of_text(r, 15, 2) for k, r in enumerate(rows)]
    # the same bytes behind a guard that does not evaluate the cast
    guarded = b.make_if(b.make_function("like", [s, b.make_literal("%x%", STR)], BOOL), b.make_literal(-100, D(15, 2)), cast, D(15, 2))
    got, = gandiva.make_projector(sch, [b.make_expression(guarded, pa.field("o", D(15, 2)))], None).evaluate(
        pa.RecordBatch.from_arrays([_string_array(rows, ones)], schema=sch))
    assert unscaled(got) == [-100 if k == at else dec_of_text(r, 15, 2) for k, r in enumerate(rows)]


def test_cast_of_a_trimmed_and_a_case_mapped_view():
    """nothing is trimmed by the cast itself: castDECIMAL(btrim(s)) reads the narrower view, castDECIMAL(upper(s)) reads through
    the byte map ('e' and 'E' are one letter); the padded text itself raises"""
    n = 1025
    rng = np.random.default_rng(6)
    plain = valid_texts(rng, n, 40)
    rows = [b" " * int(rng.integers(0, 3)) + t + b" " * int(rng.integers(0, 3)) for t in plain]
    rows[0] = b" " + plain[0]
    sch = pa.schema([pa.field("s", STR)])
    batch = pa.RecordBatch.from_arrays([_sliced(_nulls(rng, [r.decode() for r in rows]), STR)], schema=sch)
    b = gandiva.TreeExprBuilder()
    s = b.make_field(sch.field(0))
    exprs = [b.make_expression(b.make_function("castDECIMAL", [b.make_function(f, [b.make_function("btrim", [s], STR)], STR) if f else
                                                               b.make_function("btrim", [s], STR)], D(38, 6)), pa.field("o%d" % k, D(38, 6)))
             for k, f in enumerate((None, "upper", "lower"))]
    want = _lift(lambda t: dec_of_text(t.strip(b" "), 38, 6), batch.column(0).cast(pa.binary()).to_pylist())
    for g in gandiva.make_projector(sch, exprs, None).evaluate(batch):
        assert unscaled(g) == want
    with pytest.raises(gandiva.GandivaError, match="invalid argument"):
        gandiva.make_projector(sch, [b.make_expression(b.make_function("castDECIMAL", [s], D(38, 6)), pa.field("o", D(38, 6)))], None).evaluate(
            pa.RecordBatch.from_arrays([pa.array([r.decode() for r in rows], STR)], schema=sch))


def _c4_tree(b, ep, disc, tax, ship, one):
    """workloads.c4_expressions over the given operand nodes (`ship` None: without the day difference)"""
    one_minus = b.make_function("subtract", [one, disc], pa.decimal128(16, 2))
    disc_price = b.make_function("multiply", [ep, one_minus], pa.decimal128(32, 4))
    one_plus = b.make_function("add", [one, tax], pa.decimal128(16, 2))
    charge = b.make_function("multiply", [disc_price, one_plus], pa.decimal128(38, 6))
    exprs = [b.make_expression(disc_price, pa.field("disc_price", pa.decimal128(32, 4))),
             b.make_expression(charge, pa.field("charge", pa.decimal128(38, 6)))]
    if ship is not None:
        days = b.make_function("datediff", [b.make_literal(W.C4_DATE_1998_12_01, pa.date32()), ship], I32)
        exprs.append(b.make_expression(days, pa.field("days", I32)))
    return exprs


def _c4_as(batch, kind):
    """C4's batch with its three decimal columns rendered as text ("1234.56") or as doubles, OFFSET rows into their buffers"""
    cols = []
    for k in range(3):
        vals = unscaled(batch.column(k))
        assert all(v is None or dec_of_float(v / 100.0, 15, 2) == v for v in vals), "the doubles round-trip at scale 2"
        if kind == "text":
            cols.append(_sliced([None if v is None else "%d.%02d" % divmod(v, 100) for v in vals], STR))
        else:
            cols.append(_sliced([None if v is None else v / 100.0 for v in vals], F64))
    t = STR if kind == "text" else F64
    sch = pa.schema([pa.field("l_extendedprice", t), pa.field("l_discount", t), pa.field("l_tax", t), pa.field("l_shipdate", pa.date32())])
    return pa.RecordBatch.from_arrays(cols + [batch.column(3)], schema=sch)


def _c4_through(module, batch, cast_literal=False):
    """C4's three outputs over `batch`, whose first three columns are decimal(15,2), text or float64; `cast_literal`: the
    constant 1.00 as castDECIMAL(1) and no day difference (pyarrow.gandiva has neither decimal nor date32 literals)"""
    b = module.TreeExprBuilder()
    d152 = pa.decimal128(15, 2)
    nodes = []
    for k in range(3):
        f = b.make_field(batch.schema.field(k))
        nodes.append(f if pa.types.is_decimal(batch.schema.field(k).type) else b.make_function("castDECIMAL", [f], d152))
    one = b.make_function("castDECIMAL", [b.make_literal(1, I64)], d152) if cast_literal else b.make_literal(100, d152)
    exprs = _c4_tree(b, nodes[0], nodes[1], nodes[2], None if cast_literal else b.make_field(batch.schema.field(3)), one)
    return module.make_projector(batch.schema, exprs, pa.default_memory_pool()).evaluate(batch)


@pytest.mark.parametrize("n", ROWS)
def test_text_and_doubles_feed_c4(n):
    batch = W.c4_batch(n, 0.1)
    want = _c4_through(gandiva, batch)
    for kind in ("text", "double"):
        for g, w in zip(_c4_through(gandiva, _c4_as(batch, kind)), want):
            assert_bit_exact(g, w, f"C4 from {kind}, {n} rows")
    assert n < 1025 or sum(v not in (None, 0) for v in unscaled(want[1])) > 0.5 * n


def test_text_feeds_c4_through_pyarrow_gandiva():
    from gandiva_amd import pyarrow_gandiva
    pg = pyarrow_gandiva.load()
    batch = W.c4_batch(1025, 0.1)
    want = _c4_through(gandiva, batch)
    for kind in ("text", "double"):
        for g, w in zip(_c4_through(pg, _c4_as(batch, kind), cast_literal=True), want):
            assert_bit_exact(g, w, f"pyarrow.gandiva, C4 from {kind}")


@pytest.mark.parametrize("n", ROWS)
def test_is_distinct_from_of_a_cast_as_a_filter(n):
    rng = np.random.default_rng(2000 + n)
    d = dense_decimals(rng, n, 9)
    x = [v / 100.0 if rng.random() < 0.5 else float(rng.integers(-10 ** 7, 10 ** 7)) / 64.0 for v in d]
    sch = pa.schema([pa.field("x", F64), pa.field("d", D(15, 2))])
    batch = pa.RecordBatch.from_arrays([_sliced(_nulls(rng, x), F64), decimal_array(_nulls(rng, d), D(15, 2), OFFSET)], schema=sch)
    b = gandiva.TreeExprBuilder()
    fx, fd = b.make_field(sch.field(0)), b.make_field(sch.field(1))
    cond = b.make_condition(b.make_function("is_distinct_from", [b.make_function("castDECIMAL", [fx], D(15, 2)), fd], BOOL))
    sel = gandiva.make_filter(sch, cond).evaluate(batch, None, "int32")
    cast = _lift(lambda v: dec_of_float(v, 15, 2), batch.column(0).to_pylist())
    want = [k for k, (a, c) in enumerate(zip(cast, unscaled(batch.column(1)))) if is_distinct(a, 2, c, 2)]
    assert sel.to_array().to_pylist() == want
    assert n < 1025 or 0.3 * n < len(want) < 0.8 * n


@pytest.mark.parametrize("mode", ["UINT16", "UINT32"])
@pytest.mark.parametrize("n", ROWS)
def test_selection_mode_projector_over_nvl_and_greatest(n, mode):
    batch = _batch(n)
    rng = np.random.default_rng(3000 + n)
    idx = np.flatnonzero(rng.random(n) < 0.4) if n > 1 else np.array([0])
    b = gandiva.TreeExprBuilder()
    d, e = b.make_field(SCH.field("d")), b.make_field(SCH.field("e"))
    exprs = [b.make_expression(b.make_function("nvl", [d, e], D(15, 2)), pa.field("n", D(15, 2))),
             b.make_expression(b.make_function("greatest", [d, b.make_function("nvl", [e, d], D(15, 2))], D(15, 2)), pa.field("g", D(15, 2)))]
    m = gg._selection_mode(mode)
    sel = gandiva.SelectionVector(m, idx.astype(gg._SEL_DTYPE[m][1]), len(idx))
    got = gandiva.make_projector(SCH, exprs, None, mode).evaluate(batch, sel)
    dv, ev = _col(batch, "d"), _col(batch, "e")
    assert unscaled(got[0]) == [nvl_of(dv[k], ev[k]) for k in idx]
    assert unscaled(got[1]) == [both(max)(dv[k], nvl_of(ev[k], dv[k])) for k in idx]


def test_cxx_api_evaluates_the_decimal_tail():
    """gandiva_amd/cxx/tests/test_decimal_tail_cxx.cc with a GPU: known answers through gandiva::Projector, the execution error
    of a text that is no number, the validation error of nvl over two decimal types"""
    cxx = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gandiva_amd", "cxx")
    subprocess.check_call(["make", "-C", cxx, "all", "test_cxx"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(cxx, "tests", "test_decimal_tail_cxx")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
