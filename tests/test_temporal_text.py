"""Text <-> date / time on the GPU: castDATE / castTIMESTAMP / castTIME of text, castVARCHAR of date32 / date64 / timestamp
/ time32, castTIME(timestamp) and castTIMESTAMP(date32) through the C ABI (the gandiva_amd Python mirror), bit-exact
against the plain-Python restatement of tests/test_temporal_text_cpu.py.

PARITY STATUS: recollection (PARITY.md, text <-> date / time); the oracle does not know these functions."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pytest

import gandiva_amd as gandiva
from gandiva_amd import _capi, gandiva as gg
from helpers import assert_bit_exact
import test_temporal_text_cpu as R

STR, I64, BOOL = pa.string(), pa.int64(), pa.bool_()
TS, D64, D32, T32 = R.TS, R.D64, R.D32, R.T32
DAY = R.DAY
pytestmark = pytest.mark.gpu


def _time_variant(rng, c):
    """h{1,2}:m{1,2}[:s{1,2}[.f{1,3}]] of the clock of a canonical timestamp text"""
    strip = lambda x: (x.lstrip(b"0") or b"0") if rng.random() < 0.3 else x  # noqa: E731
    out = strip(c[11:13]) + b":" + strip(c[14:16])
    if rng.random() < 0.7:
        out += b":" + strip(c[17:19]) + (b"." + c[20:20 + int(rng.integers(1, 4))] if rng.random() < 0.6 else b"")
    return out


def _batch(n, seed, offset=3, nulls=0.15, variants=0.2):
    """columns s / d / t (texts castTIMESTAMP / castDATE / castTIME take: canonical, and `variants` of the rows in other
    layouts), c (canonical timestamp texts only), p (a date between spaces), ts (timestamps, 2 % of them outside years 0..9999), tsn (years 0..9999), d64,
    d32, t32 and n (castVARCHAR lengths); 15 % nulls in each column and a nonzero array offset"""
    rng = np.random.default_rng(seed)
    m = n + offset
    lo, hi = R.days_of(0, 1, 1) * DAY, R.days_of(9999, 12, 31) * DAY + DAY
    tsn = rng.integers(lo, hi, m)
    ts = np.where(rng.random(m) < 0.02, rng.integers(-(2**62), 2**62, m), tsn)
    canon = [x.replace("T", " ").encode() for x in np.datetime_as_string(tsn.astype("datetime64[ms]"), unit="ms")]
    s, d, t = list(canon), [c[:10] for c in canon], [c[11:] for c in canon]
    for i in np.nonzero(rng.random(m) < variants)[0]:
        for col, ref, cut in ((s, R.cast_timestamp, 0), (d, R.cast_date, 0), (t, R.cast_time, 1)):
            v = R._variant(rng, canon[i]) if cut == 0 else _time_variant(rng, canon[i])
            if v.isascii() and R._want(ref, v)[1] == 0:
                col[i] = v
    days = np.floor_divide(tsn, DAY)
    t32 = np.where(rng.random(m) < 0.05, rng.integers(-(2**31), 2**31, m), tsn - days * DAY)
    ns = rng.choice([0, 5, 10, 12, 23, 100], m)

    def arr(vals, typ):
        mask = rng.random(m) < nulls
        return pa.array([None if k else v for v, k in zip(vals, mask)], typ).slice(offset, n)
    cols = {"s": arr([x.decode() for x in s], STR), "d": arr([x.decode() for x in d], STR),
            "t": arr([x.decode() for x in t], STR), "c": arr([x.decode() for x in canon], STR), "p": arr([" " + x[:10].decode() + "  " for x in canon], STR),
            "ts": arr(ts.tolist(), I64).cast(TS), "tsn": arr(tsn.tolist(), I64).cast(TS),
            "d64": arr((days * DAY).tolist(), I64).cast(D64), "d32": arr(days.astype(np.int32).tolist(), pa.int32()).cast(D32),
            "t32": arr(t32.astype(np.int32).tolist(), pa.int32()).cast(T32), "n": arr(ns.tolist(), I64)}
    return pa.RecordBatch.from_arrays(list(cols.values()), names=list(cols))


def _columns(batch):
    """column name -> Python values: texts as bytes, temporal values as integers"""
    out = {}
    for name, a in zip(batch.schema.names, batch.columns):
        if pa.types.is_string(a.type):
            out[name] = [None if x is None else x.encode() for x in a.to_pylist()]
        else:
            out[name] = a.cast(I64 if a.type.bit_width == 64 else pa.int32()).to_pylist()
    return out


def _expect(fn, typ, *cols):
    vals = [None if any(a is None for a in args) else fn(*args) for args in zip(*cols)]
    if typ == STR:
        return pa.array([None if v is None else v.decode() for v in vals], STR)
    return pa.array(vals, I64 if typ.bit_width == 64 else pa.int32()).cast(typ)


class T:
    def __init__(self, schema):
        self.b = gandiva.TreeExprBuilder()
        self.f = {f.name: self.b.make_field(f) for f in schema}

    def lit(self, v, t=I64):
        return self.b.make_literal(v, t)

    def fn(self, name, args, t=STR):
        return self.b.make_function(name, args, t)

    def expr(self, node, name, t=STR):
        return self.b.make_expression(node, pa.field(name, t))


def _cases(t, big):
    """(name, tree, result type, expected(columns)) of the projection"""
    f, fn, lit = t.f, t.fn, t.lit
    vc = R.cast_varchar
    out = [("ts_of_text", fn("castTIMESTAMP", [f["s"]], TS), TS, lambda c: _expect(R.cast_timestamp, TS, c["s"])),
           ("date_of_text", fn("castDATE", [f["d"]], D64), D64, lambda c: _expect(R.cast_date, D64, c["d"])),
           ("text_of_ts", fn("castVARCHAR", [f["ts"], lit(23)]), STR, lambda c: _expect(lambda v: vc(v, 0, 23), STR, c["ts"])),
           ("text_of_d32", fn("castVARCHAR", [f["d32"], f["n"]]), STR,
            lambda c: _expect(lambda v, k: vc(v * DAY, 1, k), STR, c["d32"], c["n"]))]
    if big:
        return out
    return out + [
        ("time_of_text", fn("castTIME", [f["t"]], T32), T32, lambda c: _expect(R.cast_time, T32, c["t"])),
        ("date_of_ts_text", fn("castDATE", [f["s"]], D64), D64, lambda c: _expect(R.cast_date, D64, c["s"])),
        ("time_of_ts", fn("castTIME", [f["ts"]], T32), T32, lambda c: _expect(lambda v: v % DAY, T32, c["ts"])),
        ("ts_of_d32", fn("castTIMESTAMP", [f["d32"]], TS), TS, lambda c: _expect(lambda v: v * DAY, TS, c["d32"])),
        ("text_of_ts_n", fn("castVARCHAR", [f["ts"], f["n"]]), STR, lambda c: _expect(lambda v, k: vc(v, 0, k), STR, c["ts"], c["n"])),
        ("text_of_d64", fn("castVARCHAR", [f["d64"], lit(10)]), STR, lambda c: _expect(lambda v: vc(v, 1, 10), STR, c["d64"])),
        ("text_of_t32", fn("castVARCHAR", [f["t32"], lit(12)]), STR, lambda c: _expect(lambda v: vc(v, 2, 12), STR, c["t32"])),
        ("text_of_t32_5", fn("castVARCHAR", [f["t32"], lit(5)]), STR, lambda c: _expect(lambda v: vc(v, 2, 5), STR, c["t32"])),
        ("ts_of_canonical", fn("castTIMESTAMP", [f["c"]], TS), TS, lambda c: _expect(R.cast_timestamp, TS, c["c"])),
        ("ts_of_substr", fn("castTIMESTAMP", [fn("substr", [f["c"], lit(1), lit(19)])], TS), TS,
         lambda c: _expect(lambda x: R.cast_timestamp(x[:19]), TS, c["c"])),
        ("date_of_substr", fn("castDATE", [fn("substr", [f["p"], lit(2), lit(10)])], D64), D64,
         lambda c: _expect(lambda x: R.cast_date(x[1:11]), D64, c["p"])),
        ("date_of_trim", fn("castDATE", [fn("trim", [f["p"]])], D64), D64, lambda c: _expect(lambda x: R.cast_date(x.strip(b" ")), D64, c["p"])),
    ]


SIZES = [1, 65, 4096 + 13, 2**20 + 7]


@pytest.mark.parametrize("n", SIZES)
def test_projection_matches_the_restatement(n):
    batch = _batch(n, seed=n)
    t = T(batch.schema)
    cases = _cases(t, big=n > 100_000)
    proj = gandiva.make_projector(batch.schema, [t.expr(e, name, typ) for name, e, typ, _ in cases], pa.default_memory_pool())
    got = proj.evaluate(batch)
    col = _columns(batch)
    for (name, _, typ, want), g in zip(cases, got):
        assert g.type == typ, name
        assert_bit_exact(g, want(col), f"{name} n={n}")


def test_staged_consumers_and_round_trips():
    n = 20_011
    batch = _batch(n, seed=7)
    t = T(batch.schema)
    f, fn, lit = t.f, t.fn, t.lit
    txt = fn("castVARCHAR", [f["tsn"], lit(23)])
    exprs = [t.expr(fn("like", [fn("castVARCHAR", [f["ts"], lit(23)]), lit("2024-%", STR)], BOOL), "like", BOOL),
             t.expr(fn("concat", [fn("castVARCHAR", [f["d64"], lit(10)]), lit("|", STR), fn("castVARCHAR", [f["t32"], lit(12)])]), "cat"),
             t.expr(fn("substr", [txt, lit(12), lit(8)]), "clock"),
             t.expr(fn("castTIMESTAMP", [txt], TS), "rt_ts", TS),
             t.expr(fn("castDATE", [fn("castVARCHAR", [f["d64"], lit(10)])], D64), "rt_d64", D64),
             t.expr(fn("castDATE", [fn("castVARCHAR", [f["d32"], lit(10)])], D64), "rt_d32", D64)]
    got = gandiva.make_projector(batch.schema, exprs, pa.default_memory_pool()).evaluate(batch)
    c = _columns(batch)
    vc = R.cast_varchar
    assert_bit_exact(got[0], pa.array([None if v is None else vc(v, 0, 23).startswith(b"2024-") for v in c["ts"]], BOOL), "like")
    assert_bit_exact(got[1], pa.array([(b"" if a is None else vc(a, 1, 10)).decode() + "|" + (b"" if b is None else vc(b, 2, 12)).decode()
                                       for a, b in zip(c["d64"], c["t32"])], STR), "concat")
    assert_bit_exact(got[2], _expect(lambda v: vc(v, 0, 23)[11:19], STR, c["tsn"]), "substr")
    assert_bit_exact(got[3], batch.column(batch.schema.get_field_index("tsn")), "castTIMESTAMP(castVARCHAR(ts, 23))")
    assert_bit_exact(got[4], batch.column(batch.schema.get_field_index("d64")), "castDATE(castVARCHAR(d64, 10))")
    assert_bit_exact(got[5], batch.column(batch.schema.get_field_index("d32")).cast(D64), "castDATE(castVARCHAR(d32, 10))")


def _cond(t):
    return t.b.make_condition(t.fn("greater_than", [t.fn("castDATE", [t.f["d"]], D64), t.lit(R.days_of(5000, 1, 1) * DAY, D64)],
                                   BOOL))


def _selected(batch):
    c = _columns(batch)
    cut = R.days_of(5000, 1, 1) * DAY
    return [i for i, x in enumerate(c["d"]) if x is not None and R.cast_date(x) > cut]


def test_filter_and_filter_project_on_castdate():
    n = 30_007
    batch = _batch(n, seed=8)
    t = T(batch.schema)
    want = _selected(batch)
    assert 0 < len(want) < n
    sel = gandiva.make_filter(batch.schema, _cond(t)).evaluate(batch, pa.default_memory_pool(), "int32")
    assert sel.to_array().to_pylist() == want
    exprs = [t.expr(t.fn("castTIMESTAMP", [t.f["s"]], TS), "ts", TS), t.expr(t.fn("castTIME", [t.f["ts"]], T32), "tm", T32)]
    fp = gandiva.make_filter_project(batch.schema, _cond(t), exprs, "int32")
    arrays, sv = fp.evaluate(batch)
    taken = _columns(batch.take(pa.array(want, pa.int32())))
    assert_bit_exact(arrays[0], _expect(R.cast_timestamp, TS, taken["s"]), "filter -> castTIMESTAMP")
    assert_bit_exact(arrays[1], _expect(lambda v: v % DAY, T32, taken["ts"]), "filter -> castTIME(timestamp)")
    if sv is not None:
        assert sv.to_array().to_pylist() == want


def test_selection_mode_projection():
    n = 30_011
    batch = _batch(n, seed=9)
    t = T(batch.schema)
    sel = gandiva.make_filter(batch.schema, _cond(t)).evaluate(batch, pa.default_memory_pool(), "int32")
    cases = _cases(t, big=False)
    psel = gandiva.make_projector(batch.schema, [t.expr(e, name, typ) for name, e, typ, _ in cases], pa.default_memory_pool(), "UINT32")
    taken = _columns(batch.take(pa.array(_selected(batch), pa.int32())))
    for (name, _, _, want), g in zip(cases, psel.evaluate(batch, sel)):
        assert_bit_exact(g, want(taken), f"selection mode, {name}")


BAD = [("castDATE", "d", "2023-02-29", D64), ("castDATE", "d", "2024-01", D64),
       ("castTIMESTAMP", "s", "2024-01-15 10:20:30.1234", TS), ("castTIMESTAMP", "s", "2024-01-15 10:20 UTC", TS),
       ("castTIMESTAMP", "s", "2024-01-15 24:00:00", TS), ("castTIME", "t", "10:60", T32), ("castTIME", "t", "1:2:3.4567", T32)]


def test_each_error_class_raises_and_the_next_evaluation_is_right():
    n = 5_003
    batch = _batch(n, seed=10)
    t = T(batch.schema)
    for fname, colname, text, typ in BAD:
        i = batch.schema.get_field_index(colname)
        vals = batch.column(i).to_pylist()
        vals[n // 2] = text
        bad = pa.RecordBatch.from_arrays([pa.array(vals, STR) if k == i else a for k, a in enumerate(batch.columns)],
                                         schema=batch.schema)
        proj = gandiva.make_projector(batch.schema, [t.expr(t.fn(fname, [t.f[colname]], typ), "o", typ)], pa.default_memory_pool())
        with pytest.raises(gandiva.GandivaError, match="invalid argument"):
            proj.evaluate(bad)
        got, = proj.evaluate(batch)
        ref = {"castDATE": R.cast_date, "castTIMESTAMP": R.cast_timestamp, "castTIME": R.cast_time}[fname]
        assert_bit_exact(got, _expect(ref, typ, _columns(batch)[colname]), f"{fname} after an error")
    # castVARCHAR with a negative length on one row
    ns = batch.column(batch.schema.get_field_index("n")).to_pylist()
    tsv = _columns(batch)["ts"]
    k = next(i for i, (a, b) in enumerate(zip(ns, tsv)) if a is not None and b is not None)
    ns[k] = -1
    neg = batch.set_column(batch.schema.get_field_index("n"), "n", pa.array(ns, I64))
    proj = gandiva.make_projector(batch.schema, [t.expr(t.fn("castVARCHAR", [t.f["ts"], t.f["n"]]), "o")], pa.default_memory_pool())
    with pytest.raises(gandiva.GandivaError, match="invalid argument"):
        proj.evaluate(neg)


def test_one_tree_through_make_from_proto():
    import proto_encode as P
    n = 4_099
    batch = _batch(n, seed=11)
    t = T(batch.schema)
    exprs = [t.expr(t.fn("castTIMESTAMP", [t.f["s"]], TS), "ts", TS), t.expr(t.fn("castVARCHAR", [t.f["ts"], t.lit(23)]), "txt")]
    lib = _capi.lib()
    sb, eb = P.schema(batch.schema), P.expression_list(exprs)
    ph = C.c_void_p()
    assert lib.gdv_projector_make_from_proto(sb, len(sb), eb, len(eb), 0, None, C.byref(ph)) == 0, _capi.last_error()
    got = gg.Projector(ph, batch.schema, 0, exprs).evaluate(batch)
    c = _columns(batch)
    assert_bit_exact(got[0], _expect(R.cast_timestamp, TS, c["s"]), "proto castTIMESTAMP")
    assert_bit_exact(got[1], _expect(lambda v: R.cast_varchar(v, 0, 23), STR, c["ts"]), "proto castVARCHAR")
