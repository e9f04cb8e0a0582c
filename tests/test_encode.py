"""hex / to_hex, unhex / from_hex, base64, unbase64 and crc32 on the GPU through the C ABI (the gandiva_amd Python mirror, the
rebuilt pyarrow.gandiva, the C++ API), bit-exact against the plain-Python restatement of tests/test_encode_cpu.py.

PARITY STATUS (PARITY.md, hex / base64 / crc32): the byte-level encodings are 2-engines (RFC 4648, zlib: the restatement
is checked against binascii, base64 and zlib in test_encode_cpu.py); null, error and letter-case rules are recollection.
"Raises" is the library's own error status, returned normally."""
import ctypes as C
import os
import subprocess

import numpy as np
import pyarrow as pa
import pytest

import gandiva_amd as gandiva
from gandiva_amd import _capi, gandiva as gg, workloads as W
from helpers import assert_bit_exact
import test_encode_cpu as R

STR, BIN, I32, I64, BOOL = pa.string(), pa.binary(), pa.int32(), pa.int64(), pa.bool_()
pytestmark = pytest.mark.gpu


def _ascii_rows(rng, n, lo, hi):
    """printable ASCII texts (a utf8 column must hold UTF-8), upper- and lower-case letters, digits, punctuation"""
    lens = rng.integers(lo, hi + 1, n)
    raw = rng.integers(0x20, 0x7F, int(lens.sum()), dtype=np.uint8).tobytes()
    out, at = [], 0
    for k in lens:
        out.append(raw[at:at + int(k)])
        at += int(k)
    return out


def _batch(n, seed, lo=0, hi=70, offset=3, nulls=0.1):
    """s: ASCII text, b: any bytes, h: hex text of b (either letter case), e: base64 text of b, i / n: integers; 10 % nulls in
    each column and a nonzero array offset"""
    rng = np.random.default_rng(seed)
    m = n + offset
    s = _ascii_rows(rng, m, lo, hi)
    b = R._random_bytes(rng, m, lo, hi)
    h = [R.hex_of(x).lower() if k else R.hex_of(x) for x, k in zip(b, rng.random(m) < 0.5)]
    e = [R.base64_of(x) for x in b]
    i32 = np.where(rng.random(m) < 0.3, rng.integers(-300, 300, m), rng.integers(-2**31, 2**31, m))
    i64 = np.where(rng.random(m) < 0.3, rng.integers(-300, 300, m), rng.integers(-2**63, 2**63 - 1, m))

    def arr(vals, typ):
        mask = rng.random(m) < nulls
        return pa.array([None if k else v for v, k in zip(vals, mask)], typ).slice(offset, n)
    cols = {"s": arr([x.decode() for x in s], STR), "b": arr(b, BIN), "h": arr([x.decode() for x in h], STR),
            "e": arr([x.decode() for x in e], STR), "i": arr(i32.tolist(), I32), "n": arr(i64.tolist(), I64)}
    return pa.RecordBatch.from_arrays(list(cols.values()), names=list(cols))


def _columns(batch):
    out = {}
    for name, a in zip(batch.schema.names, batch.columns):
        vals = a.to_pylist()
        out[name] = [None if x is None else x.encode() for x in vals] if pa.types.is_string(a.type) else vals
    return out


def _expect(fn, typ, *cols):
    vals = [None if any(a is None for a in args) else fn(*args) for args in zip(*cols)]
    if typ == STR:
        return pa.array([None if v is None else v.decode() for v in vals], STR)
    return pa.array(vals, typ)


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


def _cases(t, big=False):
    """(name, tree, result type, expected(columns)) of the projection"""
    f, fn = t.f, t.fn
    out = [("hex_s", fn("hex", [f["s"]]), STR, lambda c: _expect(R.hex_of, STR, c["s"])),
           ("hex_b", fn("hex", [f["b"]]), STR, lambda c: _expect(R.hex_of, STR, c["b"])),
           ("unhex_h", fn("unhex", [f["h"]], BIN), BIN, lambda c: _expect(R.unhex_of, BIN, c["h"])),
           ("base64_b", fn("base64", [f["b"]]), STR, lambda c: _expect(R.base64_of, STR, c["b"])),
           ("unbase64_e", fn("unbase64", [f["e"]], BIN), BIN, lambda c: _expect(R.unbase64_of, BIN, c["e"])),
           ("crc32_s", fn("crc32", [f["s"]], I64), I64, lambda c: _expect(R.zlib.crc32, I64, c["s"])),
           ("crc32_b", fn("crc32", [f["b"]], I64), I64, lambda c: _expect(R.zlib.crc32, I64, c["b"]))]
    if big:
        return out
    return out + [
        ("base64_s", fn("base64", [f["s"]]), STR, lambda c: _expect(R.base64_of, STR, c["s"])),
        ("to_hex_b", fn("to_hex", [f["b"]]), STR, lambda c: _expect(R.hex_of, STR, c["b"])),
        ("from_hex_h", fn("from_hex", [f["h"]], BIN), BIN, lambda c: _expect(R.unhex_of, BIN, c["h"])),
        ("hex_i", fn("hex", [f["i"]]), STR, lambda c: _expect(lambda v: R.hex_of_int(v, 32), STR, c["i"])),
        ("hex_n", fn("hex", [f["n"]]), STR, lambda c: _expect(lambda v: R.hex_of_int(v, 64), STR, c["n"])),
        ("hex_upper", fn("hex", [fn("upper", [f["s"]])]), STR, lambda c: _expect(lambda x: R.hex_of(R.ascii_upper(x)), STR, c["s"])),
        ("base64_substr", fn("base64", [fn("substr", [f["s"], t.lit(2, I64), t.lit(9, I64)])]), STR,
         lambda c: _expect(lambda x: R.base64_of(x[1:10]), STR, c["s"])),
        ("unhex_lower", fn("unhex", [fn("lower", [f["h"]])], BIN), BIN, lambda c: _expect(R.unhex_of, BIN, c["h"])),
        ("crc32_upper", fn("crc32", [fn("upper", [f["s"]])], I64), I64, lambda c: _expect(lambda x: R.zlib.crc32(R.ascii_upper(x)), I64, c["s"])),
    ]


SIZES = [1, 65, 4096 + 13, 2**18 + 7]


@pytest.mark.parametrize("n", SIZES)
def test_projection_matches_the_restatement_host_and_device_batches(n):
    batch = _batch(n, seed=n)
    t = T(batch.schema)
    cases = _cases(t, big=n > 100_000)
    proj = gandiva.make_projector(batch.schema, [t.expr(e, name, typ) for name, e, typ, _ in cases], pa.default_memory_pool())
    col = _columns(batch)
    want = [w(col) for _, _, _, w in cases]
    for (name, _, typ, _), g, w in zip(cases, proj.evaluate(batch), want):
        assert g.type == typ, name
        assert_bit_exact(g, w, f"{name} n={n}, host batch")
    for (name, _, typ, _), g, w in zip(cases, proj.evaluate_device(gandiva.DeviceBatch.from_arrow(batch)), want):
        assert_bit_exact(g.to_arrow(), w, f"{name} n={n}, HBM-resident batch")


def test_column_of_c5s_shape():
    n = 200_003
    batch = _batch(n, seed=5, lo=4, hi=20)
    t = T(batch.schema)
    cases = _cases(t, big=True)
    got = gandiva.make_projector(batch.schema, [t.expr(e, name, typ) for name, e, typ, _ in cases], pa.default_memory_pool()).evaluate(batch)
    col = _columns(batch)
    for (name, _, _, want), g in zip(cases, got):
        assert_bit_exact(g, want(col), name)


def test_staged_trees_and_round_trips():
    n = 20_011
    batch = _batch(n, seed=7)
    t = T(batch.schema)
    f, fn = t.f, t.fn
    exprs = [t.expr(fn("like", [fn("hex", [f["s"]]), t.lit("%4A%")], BOOL), "like", BOOL),
             t.expr(fn("crc32", [fn("base64", [fn("upper", [f["s"]])])], I64), "crc", I64),
             t.expr(fn("unhex", [fn("hex", [f["b"]])], BIN), "rt_hex", BIN),
             t.expr(fn("unbase64", [fn("base64", [f["b"]])], BIN), "rt_b64", BIN),
             t.expr(fn("hex", [fn("hashMD5", [f["s"]])]), "hex_md5"),
             t.expr(fn("base64", [fn("castVARCHAR", [f["n"], t.lit(20, I64)])]), "b64_digits"),
             t.expr(fn("concat", [fn("hex", [f["b"]]), t.lit(":"), fn("base64", [f["b"]])]), "cat")]
    got = gandiva.make_projector(batch.schema, exprs, pa.default_memory_pool()).evaluate(batch)
    c = _columns(batch)
    import hashlib
    assert_bit_exact(got[0], _expect(lambda x: b"4A" in R.hex_of(x), BOOL, c["s"]), "like(hex(s), '%4A%')")
    assert_bit_exact(got[1], _expect(lambda x: R.zlib.crc32(R.base64_of(R.ascii_upper(x))), I64, c["s"]), "crc32(base64(upper(s)))")
    assert_bit_exact(got[2], batch.column(1), "unhex(hex(b))")
    assert_bit_exact(got[3], batch.column(1), "unbase64(base64(b))")
    # the digests never return null: a NULL hashes as the empty message
    assert_bit_exact(got[4], pa.array([R.hex_of(hashlib.md5(x or b"").hexdigest().encode()).decode() for x in c["s"]], STR), "hex(hashMD5(s))")
    assert_bit_exact(got[5], _expect(lambda v: R.base64_of(str(v).encode()), STR, c["n"]), "base64(castVARCHAR(n, 20))")
    assert_bit_exact(got[6], pa.array([("" if x is None else R.hex_of(x).decode()) + ":" + ("" if x is None else R.base64_of(x).decode())
                                       for x in c["b"]], STR), "concat(hex, ':', base64)")


def _cond(t):
    return t.b.make_condition(t.fn("equal", [t.fn("unhex", [t.fn("hex", [t.f["s"]])], BIN), t.f["b"]], BOOL))


def _same_rows(rng, batch):
    """the batch with b = the bytes of s on about a third of the rows"""
    s, b = batch.column(0).to_pylist(), batch.column(1).to_pylist()
    b = [x.encode() if x is not None and y is not None and rng.random() < 0.35 else y for x, y in zip(s, b)]
    return batch.set_column(1, "b", pa.array(b, BIN))


def test_filter_on_a_staged_round_trip_then_selection_mode_projection_sync_and_async():
    import torch
    n = 30_007
    batch = _same_rows(np.random.default_rng(3), _batch(n, seed=8))
    t = T(batch.schema)
    c = _columns(batch)
    want_idx = [i for i, (x, y) in enumerate(zip(c["s"], c["b"])) if x is not None and y is not None and x == y]
    assert 0 < len(want_idx) < n
    flt = gandiva.make_filter(batch.schema, _cond(t))
    sel = flt.evaluate(batch, pa.default_memory_pool(), "int32")
    assert sel.to_array().to_pylist() == want_idx
    cases = _cases(t)
    psel = gandiva.make_projector(batch.schema, [t.expr(e, name, typ) for name, e, typ, _ in cases], pa.default_memory_pool(), "UINT32")
    taken = _columns(batch.take(pa.array(want_idx, pa.int32())))
    want = [w(taken) for _, _, _, w in cases]
    for (name, _, _, _), g, w in zip(cases, psel.evaluate(batch, sel), want):
        assert_bit_exact(g, w, f"selection mode, {name}")
    # the asynchronous entry point over the same selection, HBM-resident
    db = gandiva.DeviceBatch.from_arrow(batch)
    dsel = gandiva.make_filter(batch.schema, t.b.make_condition(t.fn("greater_than", [t.f["i"], t.lit(0, I32)], BOOL))).evaluate_device(db, "int32")
    idx = dsel.indices[: dsel.num_slots].cpu().numpy().astype(np.int64)
    taken = _columns(batch.take(pa.array(idx)))
    cap = 64 + 8 * sum(col.data.numel() for col in db.columns if col.offsets is not None)
    outs, result = psel.evaluate_device_async(db, selection=dsel, capacity_bytes=cap)
    torch.cuda.synchronize()
    assert int(result[0].item()) == 0
    for (name, _, _, w), o in zip(cases, outs):
        assert_bit_exact(o.to_arrow(), w(taken), f"selection mode, asynchronous, {name}")


def test_filter_project_chain_with_binary_outputs():
    """filter -> project with var-len outputs is the chain of two operators (the fused kernel stays fixed-width); crc32 alone
    takes whichever shape the planner gives it"""
    n = 20_003
    batch = _batch(n, seed=9)
    t = T(batch.schema)
    cond = t.b.make_condition(t.fn("greater_than", [t.f["i"], t.lit(0, I32)], BOOL))
    c = _columns(batch)
    want_idx = [i for i, v in enumerate(c["i"]) if v is not None and v > 0]
    taken = _columns(batch.take(pa.array(want_idx, pa.int32())))
    exprs = [t.expr(t.fn("unhex", [t.f["h"]], BIN), "u", BIN), t.expr(t.fn("base64", [t.f["b"]]), "e")]
    arrays, sv = gandiva.make_filter_project(batch.schema, cond, exprs, "int32").evaluate(batch)
    assert_bit_exact(arrays[0], _expect(R.unhex_of, BIN, taken["h"]), "filter -> unhex")
    assert_bit_exact(arrays[1], _expect(R.base64_of, STR, taken["b"]), "filter -> base64")
    fixed = [t.expr(t.fn("crc32", [t.f["b"]], I64), "c", I64)]
    arrays, sv = gandiva.make_filter_project(batch.schema, cond, fixed, "int32").evaluate(batch)
    assert_bit_exact(arrays[0], _expect(R.zlib.crc32, I64, taken["b"]), "filter -> crc32")


BAD = [("unhex", "h", "4a6G"), ("unhex", "h", "4a6"), ("from_hex", "h", "4a 6"), ("unbase64", "e", "QQ="), ("unbase64", "e", "Q=Q="),
       ("unbase64", "e", "QQ==QQ=="), ("unbase64", "e", "Q Q="), ("unbase64", "e", "QUJD\n===")]


def test_one_invalid_row_is_an_execution_error_and_the_same_row_null_is_not():
    n = 5_003
    batch = _batch(n, seed=10)
    t = T(batch.schema)
    for fname, colname, text in BAD:
        i = batch.schema.get_field_index(colname)
        vals = batch.column(i).to_pylist()
        vals[n // 2] = text
        bad = batch.set_column(i, colname, pa.array(vals, STR))
        vals[n // 2] = None
        nulled = batch.set_column(i, colname, pa.array(vals, STR))
        proj = gandiva.make_projector(batch.schema, [t.expr(t.fn(fname, [t.f[colname]], BIN), "o", BIN)], pa.default_memory_pool())
        with pytest.raises(gandiva.GandivaError, match="invalid argument"):
            proj.evaluate(bad)
        ref = R.unbase64_of if fname == "unbase64" else R.unhex_of
        got, = proj.evaluate(nulled)
        assert_bit_exact(got, _expect(ref, BIN, _columns(nulled)[colname]), f"{fname}: the row null")
        got, = proj.evaluate_device(gandiva.DeviceBatch.from_arrow(nulled))
        assert_bit_exact(got.to_arrow(), _expect(ref, BIN, _columns(nulled)[colname]), f"{fname}: the row null, HBM-resident")
        with pytest.raises(gandiva.GandivaError, match="invalid argument"):
            proj.evaluate_device(gandiva.DeviceBatch.from_arrow(bad))
    # "QR==": the unused bits of the last digit are not checked
    one = pa.RecordBatch.from_arrays([pa.array(["QR==", "QQ=="], STR)], names=["e"])
    t1 = T(one.schema)
    got, = gandiva.make_projector(one.schema, [t1.expr(t1.fn("unbase64", [t1.f["e"]], BIN), "o", BIN)], pa.default_memory_pool()).evaluate(one)
    assert got.to_pylist() == [b"A", b"A"]


def test_binary_results_through_the_rebuilt_pyarrow_gandiva():
    from gandiva_amd import pyarrow_gandiva
    pg = pyarrow_gandiva.load()
    n = 4_099
    batch = _batch(n, seed=11)
    b = pg.TreeExprBuilder()
    h, e, raw = (b.make_field(batch.schema.field(k)) for k in ("h", "e", "b"))
    exprs = [b.make_expression(b.make_function("unhex", [h], BIN), pa.field("u", BIN)),
             b.make_expression(b.make_function("unbase64", [e], BIN), pa.field("v", BIN)),
             b.make_expression(b.make_function("hex", [raw], STR), pa.field("w", STR)),
             b.make_expression(b.make_function("crc32", [raw], I64), pa.field("c", I64))]
    got = pg.make_projector(batch.schema, exprs, pa.default_memory_pool()).evaluate(batch)
    c = _columns(batch)
    assert got[0].type == BIN and got[1].type == BIN
    assert got[0].equals(_expect(R.unhex_of, BIN, c["h"])) and got[1].equals(_expect(R.unbase64_of, BIN, c["e"]))
    assert got[2].equals(_expect(R.hex_of, STR, c["b"])) and got[3].equals(_expect(R.zlib.crc32, I64, c["b"]))


def test_binary_results_through_the_cxx_api():
    cxx = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gandiva_amd", "cxx")
    subprocess.check_call(["make", "-C", cxx, "all", "test_cxx"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(cxx, "tests", "test_encode_cxx")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr


def test_binary_results_through_make_from_proto():
    import proto_encode as P
    n = 4_099
    batch = _batch(n, seed=12)
    t = T(batch.schema)
    exprs = [t.expr(t.fn("unhex", [t.f["h"]], BIN), "u", BIN), t.expr(t.fn("base64", [t.f["b"]]), "e"),
             t.expr(t.fn("crc32", [t.f["s"]], I64), "c", I64)]
    lib = _capi.lib()
    sb, eb = P.schema(batch.schema), P.expression_list(exprs)
    ph = C.c_void_p()
    assert lib.gdv_projector_make_from_proto(sb, len(sb), eb, len(eb), 0, None, C.byref(ph)) == 0, _capi.last_error()
    got = gg.Projector(ph, batch.schema, 0, exprs).evaluate(batch)
    c = _columns(batch)
    assert got[0].type == BIN
    assert_bit_exact(got[0], _expect(R.unhex_of, BIN, c["h"]), "proto unhex")
    assert_bit_exact(got[1], _expect(R.base64_of, STR, c["b"]), "proto base64")
    assert_bit_exact(got[2], _expect(R.zlib.crc32, I64, c["s"]), "proto crc32")


def test_binary_results_through_the_sharded_entry_point():
    """ONE host batch over two device contexts (virtual contexts of the one GPU of a test box): binary outputs land in one
    set of host arrays"""
    from gandiva_amd import shard
    gandiva.set_virtual_devices(2)
    n = 50_021
    batch = _batch(n, seed=13)
    t = T(batch.schema)
    exprs = [t.expr(t.fn("unhex", [t.f["h"]], BIN), "u", BIN), t.expr(t.fn("unbase64", [t.f["e"]], BIN), "v", BIN),
             t.expr(t.fn("crc32", [t.f["b"]], I64), "c", I64)]
    proj = gandiva.make_projector(batch.schema, exprs, None)
    got = shard.evaluate_projector_host_sharded(proj, batch, [0, 1])
    c = _columns(batch)
    assert got[0].type == BIN and got[1].type == BIN
    assert_bit_exact(got[0], _expect(R.unhex_of, BIN, c["h"]), "sharded unhex")
    assert_bit_exact(got[1], _expect(R.unbase64_of, BIN, c["e"]), "sharded unbase64")
    assert_bit_exact(got[2], _expect(R.zlib.crc32, I64, c["b"]), "sharded crc32")


def test_c5_column_at_ten_million_rows_two_windows_and_total_bytes():
    n = 10_000_000
    batch = W.c5_batch(n, 0.1, 0.0)
    t = T(batch.schema)
    s = t.f[batch.schema.names[0]]
    exprs = [t.expr(t.fn("hex", [s]), "x"), t.expr(t.fn("base64", [s]), "e"), t.expr(t.fn("crc32", [s], I64), "c", I64)]
    got = gandiva.make_projector(batch.schema, exprs, pa.default_memory_pool()).evaluate(batch)
    col = batch.column(0)
    import pyarrow.compute as pc
    lens = pc.binary_length(col).fill_null(0).to_numpy()
    total_of = lambda a: int(pc.sum(pc.binary_length(a)).as_py())  # noqa: E731
    assert total_of(got[0]) == 2 * int(lens.sum())
    assert total_of(got[1]) == int((4 * ((lens + 2) // 3)).sum())
    for lo in (0, n - 50_000):
        S = [None if x is None else x.encode() for x in col.slice(lo, 50_000).to_pylist()]
        assert_bit_exact(got[0].slice(lo, 50_000), _expect(R.hex_of, STR, S), f"hex window {lo}")
        assert_bit_exact(got[1].slice(lo, 50_000), _expect(R.base64_of, STR, S), f"base64 window {lo}")
        assert_bit_exact(got[2].slice(lo, 50_000), _expect(R.zlib.crc32, I64, S), f"crc32 window {lo}")
    # the decoders over the encoded columns: the source comes back
    enc = pa.RecordBatch.from_arrays([got[0], got[1]], names=["h", "e"])
    te = T(enc.schema)
    back = gandiva.make_projector(enc.schema, [te.expr(te.fn("unhex", [te.f["h"]], BIN), "u", BIN),
                                               te.expr(te.fn("unbase64", [te.f["e"]], BIN), "v", BIN)], pa.default_memory_pool()).evaluate(enc)
    total = int(lens.sum())
    for g in back:
        assert total_of(g) == total
        for lo in (0, n - 50_000):
            assert_bit_exact(g.slice(lo, 50_000), col.slice(lo, 50_000).cast(BIN), f"decoder window {lo}")
