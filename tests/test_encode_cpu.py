"""hex / to_hex, unhex / from_hex, base64, unbase64 and crc32 over text and binary, without a GPU.

PARITY STATUS (PARITY.md, hex / base64 / crc32): the byte-level encodings are 2-engines — RFC 4648 and the zlib CRC-32 are
public standards, and Python's binascii, base64 and zlib share no code with the product.  The rules around them (null if
null, upper-case digits, raising on text the decoders do not take, hex of negative integers, crc32 widened to int64) are
recollection, the strict unbase64 grammar and its unchecked trailing bits are decided here.  The expected values come from
the plain-Python restatement below; the restatement itself is checked against the standard library.  Where the two could
differ on a later Python (what b64decode(validate=True) refuses), the restatement is the rule.  This file checks
  * the registry, through the Python mirror and through libgandiva.so's ExpressionRegistry (the rebuilt pyarrow.gandiva);
  * Make of every signature and of staged compositions, cross-compiled for gfx950 by hipRTC, which copy entry their kernels
    take and where their pre-passes read bytes;
  * the product's device functions and the copy entry of plans that hold such a value, compiled for the host
    (tests/host_devlib/host_encode.cc), against the restatement on random rows."""
import base64
import binascii
import ctypes as C
import os
import re
import subprocess
import zlib

import numpy as np
import pyarrow as pa
import pytest

import gandiva_amd as gandiva
from gandiva_amd import _capi, gandiva as gg

HERE = os.path.dirname(os.path.abspath(__file__))
STR, BIN, I32, I64, BOOL = pa.string(), pa.binary(), pa.int32(), pa.int64(), pa.bool_()


class RowError(Exception):
    """the row raises "invalid argument" (an execution error of the whole evaluation)"""


# ------------------------------------------------------------------ the restatement (bytes in, value or RowError out)

HEX_DIGITS = b"0123456789ABCDEF"
B64_ALPHABET = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"


def hex_of(b):
    return bytes(HEX_DIGITS[c >> 4 if k == 0 else c & 15] for c in b for k in (0, 1))


def hex_of_int(v, bits):
    """%X of the two's complement of v in `bits` bits"""
    v &= (1 << bits) - 1
    out = b""
    while True:
        out = HEX_DIGITS[v & 15:(v & 15) + 1] + out
        v >>= 4
        if v == 0:
            return out


def _nibble(c):
    if 0x30 <= c <= 0x39:
        return c - 0x30
    if 0x41 <= c <= 0x46 or 0x61 <= c <= 0x66:
        return (c & 0x0F) + 9
    raise RowError("not a hex digit")


def unhex_of(t):
    if len(t) % 2:
        raise RowError("odd length")
    return bytes(_nibble(t[i]) << 4 | _nibble(t[i + 1]) for i in range(0, len(t), 2))


def base64_of(b):
    out = bytearray()
    for i in range(0, len(b), 3):
        g = b[i:i + 3]
        v = int.from_bytes(g.ljust(3, b"\0"), "big")
        chars = bytes(B64_ALPHABET[(v >> s) & 63] for s in (18, 12, 6, 0))
        out += chars[:len(g) + 1] + b"=" * (3 - len(g))
    return bytes(out)


def unbase64_of(t):
    if len(t) % 4:
        raise RowError("length is not a multiple of 4")
    pad = 0 if not t.endswith(b"=") else 1 if not t.endswith(b"==") else 2
    body = t[:len(t) - pad]
    out = bytearray()
    for i in range(0, len(t), 4):
        v = 0
        for k in range(4):
            v <<= 6
            if i + k < len(body):
                s = B64_ALPHABET.find(bytes([body[i + k]]))
                if s < 0:
                    raise RowError("not an alphabet byte (an '=' anywhere but in the last one or two positions included)")
                v |= s
        out += v.to_bytes(3, "big")
    return bytes(out[:len(out) - pad]) if pad else bytes(out)


def crc32_of(b):
    """bit by bit: the reflected polynomial 0xEDB88320, initial value and final XOR 0xFFFFFFFF"""
    c = 0xFFFFFFFF
    for x in b:
        c ^= x
        for _ in range(8):
            c = (c >> 1) ^ (0xEDB88320 if c & 1 else 0)
    return c ^ 0xFFFFFFFF


def ascii_upper(b):
    return bytes(c - 32 if 0x61 <= c <= 0x7A else c for c in b)


def ascii_lower(b):
    return bytes(c + 32 if 0x41 <= c <= 0x5A else c for c in b)


# ------------------------------------------------------------------ 1. the restatement against the standard library

def _random_bytes(rng, n, lo=0, hi=70):
    lens = rng.integers(lo, hi + 1, n)
    raw = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8).tobytes()
    out, at = [], 0
    for k in lens:
        out.append(raw[at:at + int(k)])
        at += int(k)
    return out


def test_restatement_pins():
    assert hex_of(b"\x00\xffJk") == b"00FF4A6B" and hex_of(b"") == b""
    assert hex_of_int(0, 32) == b"0" and hex_of_int(-1, 32) == b"FFFFFFFF" and hex_of_int(-1, 64) == b"F" * 16
    assert hex_of_int(255, 64) == b"FF" and hex_of_int(-(1 << 31), 32) == b"80000000" and hex_of_int(0x1234ABCD, 32) == b"1234ABCD"
    assert unhex_of(b"4a6B") == b"Jk" and unhex_of(b"") == b""
    for bad in (b"4", b"4G", b"4a6", b" 4a6", b"0x4a", b"4a\x00\x00", b"\xb4a"):
        with pytest.raises(RowError):
            unhex_of(bad)
    assert base64_of(b"") == b"" and base64_of(b"A") == b"QQ==" and base64_of(b"AB") == b"QUI=" and base64_of(b"ABC") == b"QUJD"
    assert base64_of(b"\xfb\xff\xfe") == b"+//+"
    assert unbase64_of(b"QQ==") == b"A" and unbase64_of(b"QR==") == b"A" and unbase64_of(b"") == b""
    for bad in (b"QQ=", b"Q=Q=", b"QQ==QQ==", b"Q Q=", b"Q===", b"====", b"QUJD=", b"QUJ-", b"QUJ_", b"QQ=\n", b"QUJD\n"):
        with pytest.raises(RowError):
            unbase64_of(bad)
    assert crc32_of(b"") == 0 and crc32_of(b"spark") == 2635321133 and crc32_of(b"123456789") == 0xCBF43926


def test_restatement_against_binascii_base64_and_zlib():
    rng = np.random.default_rng(21)
    rows = _random_bytes(rng, 4000) + [bytes([c]) * k for c in (0, 0xFF, 0x41) for k in range(0, 20)]
    assert {len(r) % 8 for r in rows} == set(range(8)) and {len(r) % 6 for r in rows} == set(range(6))
    for r in rows:
        assert hex_of(r) == binascii.hexlify(r).upper()
        assert unhex_of(hex_of(r)) == unhex_of(hex_of(r).lower()) == binascii.unhexlify(hex_of(r)) == r
        assert base64_of(r) == base64.b64encode(r)
        assert unbase64_of(base64_of(r)) == base64.b64decode(base64_of(r), validate=True) == r
        assert crc32_of(r) == zlib.crc32(r)
    assert zlib.crc32(b"spark") == 2635321133
    # rejected inputs, where the two agree (on this image's Python; on a later one the restatement is the rule)
    for bad in (b"QQ=", b"Q=Q=", b"QQ==QQ==", b"Q Q="):
        with pytest.raises(binascii.Error):
            base64.b64decode(bad, validate=True)
        with pytest.raises(RowError):
            unbase64_of(bad)
    assert base64.b64decode(b"QR==", validate=True) == b"A" == unbase64_of(b"QR==")
    for bad in (b"4", b"4G", b"zz"):
        with pytest.raises(binascii.Error):
            binascii.unhexlify(bad)
        with pytest.raises(RowError):
            unhex_of(bad)
    for v in [int(x) for x in rng.integers(-2**63, 2**63 - 1, 2000)] + [0, 1, -1, 2**63 - 1, -2**63, 15, 16, 255, 256]:
        assert hex_of_int(v, 64) == format(v & (2**64 - 1), "X").encode()
        w = v & 0xFFFFFFFF
        assert hex_of_int(w - (1 << 32) if w >> 31 else w, 32) == format(w, "X").encode()


# ------------------------------------------------------------------ 2. registry

WANT = ([(f, [t], STR) for f in ("hex", "to_hex") for t in (STR, BIN, I32, I64)] +
        [(f, [STR], BIN) for f in ("unhex", "from_hex", "unbase64")] +
        [("base64", [t], STR) for t in (STR, BIN)] + [("crc32", [t], I64) for t in (STR, BIN)])


def _signatures(sigs):
    return {(s.name(), tuple(s.param_types())): s.return_type() for s in sigs}


def test_registry_lists_the_encode_functions():
    sigs = _signatures(gandiva.get_registered_function_signatures())
    for name, params, ret in WANT:
        assert sigs.get((name, tuple(params))) == ret, (name, params)


def test_registry_of_the_rebuilt_pyarrow_gandiva_lists_the_encode_functions():
    from gandiva_amd import pyarrow_gandiva
    sigs = _signatures(pyarrow_gandiva.load().get_registered_function_signatures())
    for name, params, ret in WANT:
        assert sigs.get((name, tuple(params))) == ret, (name, params)


# ------------------------------------------------------------------ 3. Make + cross-compile (hipRTC, no GPU)

def _precompile(monkeypatch, tmp_path, schema, exprs=None, cond=None):
    os.makedirs(tmp_path, exist_ok=True)
    monkeypatch.setenv("GDV_NO_DISK_CACHE", "1")
    monkeypatch.setenv("GDV_DUMP_SOURCE", "1")
    monkeypatch.setenv("GANDIVA_AMD_CACHE_DIR", str(tmp_path))
    lib = _capi.lib()
    sh = gg._make_schema(schema)
    try:
        if cond is not None:
            rc = lib.gdv_precompile_filter(sh, cond._h)
        else:
            arr = (C.c_void_p * len(exprs))(*[e._h for e in exprs])
            rc = lib.gdv_precompile_projector(sh, arr, len(exprs), 0)
        assert rc == 0, _capi.last_error()
    finally:
        lib.gdv_schema_free(sh)
    return [open(os.path.join(tmp_path, f)).read() for f in sorted(os.listdir(tmp_path)) if f.endswith(".hip")]


SCH = pa.schema([pa.field("s", STR), pa.field("b", BIN), pa.field("i", I32), pa.field("n", I64)])


class T:
    def __init__(self):
        self.b = gandiva.TreeExprBuilder()
        self.f = {f.name: self.b.make_field(f) for f in SCH}

    def fn(self, name, args, t=STR):
        return self.b.make_function(name, args, t)

    def lit(self, v, t=STR):
        return self.b.make_literal(v, t)

    def expr(self, node, name, t=STR):
        return self.b.make_expression(node, pa.field(name, t))


@pytest.mark.parametrize("name", sorted({n for n, _, _ in WANT}))
def test_make_of_every_signature(monkeypatch, tmp_path, name):
    """Make resolves every signature of the name and plans it; its kernels compile for gfx950 (on the parent commit: "no
    such signature")"""
    t = T()
    sigs = [(p[0], r) for n, p, r in WANT if n == name]
    arg = {STR: t.f["s"], BIN: t.f["b"], I32: t.f["i"], I64: t.f["n"]}
    exprs = [t.expr(t.fn(name, [arg[p]], r), f"o{k}", r) for k, (p, r) in enumerate(sigs)]
    texts = _precompile(monkeypatch, tmp_path, SCH, exprs=exprs)
    for p, r in sigs:
        sym = {"to_hex": "hex", "from_hex": "unhex"}.get(name, name) + "_" + {STR: "utf8", BIN: "binary", I32: "int32", I64: "int64"}[p]
        assert any(sym + "(" in x for x in texts), sym


def test_make_of_staged_compositions(monkeypatch, tmp_path):
    """consumers of an encode value run as staged plans, any depth; the digests' own text and castVARCHAR values are
    taken as arguments the same way"""
    t = T()
    s, b = t.f["s"], t.f["b"]
    trees = [(t.fn("like", [t.fn("hex", [s]), t.lit("%4A%")], BOOL), BOOL),
             (t.fn("equal", [t.fn("unhex", [t.fn("hex", [b])], BIN), b], BOOL), BOOL),
             (t.fn("crc32", [t.fn("base64", [t.fn("upper", [s])])], I64), I64),
             (t.fn("hex", [t.fn("hashMD5", [s])]), STR), (t.fn("base64", [t.fn("castVARCHAR", [t.f["n"], t.lit(20, I64)])]), STR),
             (t.fn("unbase64", [t.fn("base64", [t.fn("unhex", [t.fn("hex", [s])], BIN)])], BIN), BIN)]
    texts = _precompile(monkeypatch, tmp_path, SCH, exprs=[t.expr(node, f"o{k}", ret) for k, (node, ret) in enumerate(trees)])
    for sym in ("hex_utf8(", "hex_binary(", "unhex_utf8(", "base64_utf8(", "unbase64_utf8(", "crc32_utf8(", "hashMD5_utf8("):
        assert any(sym in x for x in texts), sym


LENGTH_FNS = ("hex_utf8", "hex_binary", "hex_int32", "hex_int64", "unhex_utf8", "base64_binary", "unbase64_utf8", "crc32_utf8")


def test_projection_with_every_new_function_cross_compiles(monkeypatch, tmp_path):
    t = T()
    f = t.f
    exprs = [t.expr(t.fn("hex", [f["s"]]), "a"), t.expr(t.fn("to_hex", [f["b"]]), "a2"), t.expr(t.fn("hex", [f["i"]]), "a3"),
             t.expr(t.fn("hex", [f["n"]]), "a4"), t.expr(t.fn("from_hex", [f["s"]], BIN), "c", BIN),
             t.expr(t.fn("base64", [f["b"]]), "d"), t.expr(t.fn("unbase64", [f["s"]], BIN), "e", BIN),
             t.expr(t.fn("crc32", [f["s"]], I64), "g", I64)]
    texts = _precompile(monkeypatch, tmp_path, SCH, exprs=exprs)
    for sym in LENGTH_FNS:
        assert any(sym + "(" in x for x in texts), sym
    # the kernels that copy var-len outputs take the encode copy entry, and only it
    main = [x for x in texts if "GDV_STAGE_COPY" in x]
    assert main and all(re.search(r"GDV_STAGE_COPY\(dst, v\) gdv_stage_copy(_mirh?)?_enc\(", x) for x in main)
    assert any("gdv_str_copy_enc(" in x for x in texts)
    assert not any("_ext" in x or "_dt" in x for x in texts)


def test_plans_without_the_new_functions_keep_their_copy_entry(monkeypatch, tmp_path):
    t = T()
    s, n = t.f["s"], t.f["n"]
    plain = [t.expr(t.fn("upper", [s]), "u"), t.expr(t.fn("castVARCHAR", [n, t.lit(20, I64)]), "v"),
             t.expr(t.fn("hashMD5", [s]), "h"), t.expr(t.fn("hash32", [s], I32), "k", I32)]
    for x in _precompile(monkeypatch, tmp_path / "plain", SCH, exprs=plain):
        assert "_enc" not in x and "GDV_MAP_ENCODE" not in x.split("gdv_device_lib")[0]
    # crc32 alone is a fixed-width result: no copy entry changes
    for x in _precompile(monkeypatch, tmp_path / "crc", SCH, exprs=[t.expr(t.fn("crc32", [s], I64), "g", I64), t.expr(s, "s")]):
        assert "_enc" not in x and "crc32_utf8(" in x


def test_encode_with_translate_and_castvarchar_takes_the_combined_entry(monkeypatch, tmp_path):
    t = T()
    ts = pa.schema(list(SCH) + [pa.field("ts", pa.timestamp("ms"))])
    exprs = [t.expr(t.fn("translate", [t.f["s"], t.lit("ab"), t.lit("x")]), "w"),
             t.expr(t.fn("castVARCHAR", [t.b.make_field(ts.field("ts")), t.lit(23, I64)]), "g"),
             t.expr(t.fn("base64", [t.f["s"]]), "h")]
    texts = _precompile(monkeypatch, tmp_path, ts, exprs=exprs)
    assert any(re.search(r"gdv_stage_copy(_mirh?)?_ext_dt_enc\(", x) for x in texts)


def test_like_over_hex_runs_staged_and_cross_compiles(monkeypatch, tmp_path):
    t = T()
    e = t.fn("like", [t.fn("hex", [t.f["s"]]), t.lit("%4A%")], BOOL)
    texts = _precompile(monkeypatch, tmp_path, SCH, exprs=[t.expr(e, "m", BOOL)])
    stage1 = [x for x in texts if "hex_utf8(" in x]
    stage2 = [x for x in texts if "gdv_like_contains" in x or "gdv_range_any" in x]
    assert stage1 and stage2 and not set(map(id, stage1)) & set(map(id, stage2))


def test_three_stage_tree_cross_compiles(monkeypatch, tmp_path):
    """crc32(base64(upper(s))) and a filter on equal(unhex(hex(s)), b): each value is a stage's output"""
    t = T()
    e = t.fn("crc32", [t.fn("base64", [t.fn("upper", [t.f["s"]])])], I64)
    texts = _precompile(monkeypatch, tmp_path / "p", SCH, exprs=[t.expr(e, "c", I64)])
    assert any("base64_utf8(" in x and "upper_utf8(" in x for x in texts) and any("crc32_utf8(" in x for x in texts)
    assert not any("base64_utf8(" in x and "crc32_utf8(" in x for x in texts)
    cond = t.b.make_condition(t.fn("equal", [t.fn("unhex", [t.fn("hex", [t.f["s"]])], BIN), t.f["b"]], BOOL))
    texts = _precompile(monkeypatch, tmp_path / "f", SCH, cond=cond)
    assert any("hex_utf8(" in x for x in texts) and any("unhex_utf8(" in x for x in texts)


# what a kernel that reads the BYTES of an encode value's source holds: the copy routine's entry (the word conversions are
# reached through it alone); unbase64's length function reads the row's last word and says so by its name
ARGS = {"hex": ("hex", "s", STR), "hex_binary": ("hex", "b", STR), "base64": ("base64", "s", STR), "unhex": ("unhex", "s", BIN),
        "hex_of_upper": ("hex", "upper", STR), "unbase64": ("unbase64", "s", BIN)}


@pytest.mark.parametrize("name", sorted(ARGS))
def test_prepass_reads_bytes_exactly_where_the_function_needs_them(monkeypatch, tmp_path, name):
    """hex, base64 and unhex over a column or a view are byte-free: their lengths follow from the source lengths, the
    pre-pass calls the length function and never the copy (unhex's errors are the main kernel's), and a plan restricted to
    byte-free pre-passes (GDV_WAVE_BYTEFREE_ONLY) keeps the wave shape.  unbase64 reads the row's last word for the padding
    count: its pre-pass exists, calls nothing but the length function, and is not byte-free."""
    t = T()
    fn, arg, ret = ARGS[name]
    a = t.fn("upper", [t.f["s"]]) if arg == "upper" else t.f[arg]
    exprs = [t.expr(t.fn(fn, [a], ret), "o", ret)]
    texts = _precompile(monkeypatch, tmp_path / "any", SCH, exprs=exprs)
    pre = [x for x in texts if "// pre-pass:" in x]
    assert len(pre) == 1
    body = pre[0].split('#include "gdv_device_lib.hpp"')[1]
    assert "_enc(" not in body and "gdv_copy_encode" not in body and "gdv_word_at" not in body
    sym = {"hex": "hex_utf8(", "hex_binary": "hex_binary(", "hex_of_upper": "hex_utf8(", "base64": "base64_utf8(",
           "unhex": "unhex_utf8(", "unbase64": "unbase64_utf8("}[name]
    assert sym in body
    monkeypatch.setenv("GDV_WAVE_BYTEFREE_ONLY", "1")
    texts = _precompile(monkeypatch, tmp_path / "bf", SCH, exprs=exprs)
    assert len([x for x in texts if "// pre-pass:" in x]) == (0 if name == "unbase64" else 1), name


# ------------------------------------------------------------------ 4. the device functions on the host

SRC = os.path.join(HERE, "host_devlib", "host_encode.cc")
LIB = os.path.join(HERE, "host_devlib", "libhost_encode.so")
HEX, UNHEX, B64, UNB64 = 0, 1, 2, 3


@pytest.fixture(scope="module")
def enclib():
    hdr = os.path.join(HERE, "..", "gandiva_amd", "csrc", "gdv_device_lib.hpp")
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off",
                               "-Wno-unused-function", "-Wno-unused-variable", "-Wno-attributes", SRC, "-o", LIB])
    lib = C.CDLL(LIB)
    lib.host_encode.restype = C.c_long
    lib.host_hex_int.restype = C.c_long
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _layout(rows, lead=0):
    """offsets + data of the rows, the first row `lead` bytes into the buffer, 24 readable bytes behind the last"""
    n = len(rows)
    off = np.zeros(n + 1, dtype=np.int32)
    off[0] = lead
    off[1:] = lead + np.cumsum([len(x) for x in rows])
    data = np.frombuffer(b"\xa5" * lead + b"".join(rows) + b"\0" * 24, dtype=np.uint8).copy()
    return off, data


def _run(lib, fn, rows, valid=None, inbuf=1, text_map=0, shift=0, lead=0, factor=2):
    n = len(rows)
    off, data = _layout(rows, lead)
    valid = np.ones(n, dtype=np.uint8) if valid is None else np.asarray(valid, dtype=np.uint8)
    out_off = np.zeros(n + 1, dtype=np.int32)
    cap = factor * int(off[-1] - off[0]) + 4 * n + 64
    out = np.full(cap + shift, 0xEE, dtype=np.uint8)
    err = np.zeros(n, dtype=np.uint8)
    total = lib.host_encode(fn, _p(off), _p(data), C.c_long(int(off[-1])), _p(valid), C.c_long(n), inbuf, text_map, shift,
                            _p(out_off), _p(out), _p(err))
    raw = out.tobytes()
    assert set(raw[:shift]) <= {0xEE} and set(raw[shift + total:]) <= {0xEE}, "bytes written outside the output"
    return [raw[shift + out_off[i]:shift + out_off[i + 1]] for i in range(n)], err


def _expect(fn, rows, valid, text_map=0):
    rule = {HEX: hex_of, UNHEX: unhex_of, B64: base64_of, UNB64: unbase64_of}[fn]
    mapped = {0: lambda x: x, 1: ascii_upper, 2: ascii_lower}[text_map]
    want = []
    for r, v in zip(rows, valid):
        if not v:
            want.append((b"", False))
            continue
        try:
            want.append((rule(mapped(r)), False))
        except RowError:
            want.append((None, True))
    return want


def _check(got, err, want, what):
    bad = [i for i, (g, e, (w, we)) in enumerate(zip(got, err, want)) if (e != 0) != we or (not we and g != w)]
    if bad:
        i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} rows differ; row {i}: got {got[i]!r} error {err[i]}, want {want[i]}")
    assert all(e in (0, 4) for e in err), "only GDV_ERR_BAD_ARG is raised"


def _spoil(rng, t, alphabet):
    """an invalid variant of the encoded text t: a byte outside the alphabet, a wrong length, a misplaced '='"""
    t = bytearray(t)
    k = rng.random()
    if len(t) == 0 or k < 0.25:
        return bytes(t) + b"0"
    outside = [c for c in range(256) if c not in alphabet]
    if k < 0.85:
        t[int(rng.integers(0, len(t)))] = int(rng.choice(outside))
        return bytes(t)
    if alphabet is B64_ALPHABET:
        t[int(rng.integers(0, max(1, len(t) - 2)))] = 0x3D  # '=' where it may not stand
        return bytes(t)
    return bytes(t[:-1])


def _decoder_rows(rng, n, fn):
    """encoded texts of random byte strings (hex in either letter case); 10 % spoiled"""
    rows = []
    for r in _random_bytes(rng, n):
        if fn == UNHEX:
            t = hex_of(r)
            t = t.lower() if rng.random() < 0.4 else bytes(c + 32 if c >= 0x41 and rng.random() < 0.5 else c for c in t)
            alphabet = b"0123456789abcdefABCDEF"
        else:
            t = base64_of(r)
            alphabet = B64_ALPHABET
        if rng.random() < 0.1:
            t = _spoil(rng, t, alphabet)
        rows.append(t)
    return rows


N_ROWS = 100_000


@pytest.mark.parametrize("fn", [HEX, B64], ids=["hex", "base64"])
def test_host_encoders_against_the_restatement(enclib, fn):
    rng = np.random.default_rng(31 + fn)
    rows = _random_bytes(rng, N_ROWS)
    rows[:71] = [bytes(rng.integers(0, 256, k, dtype=np.uint8)) for k in range(71)]
    valid = rng.random(N_ROWS) >= 0.1
    got, err = _run(enclib, fn, rows, valid)
    _check(got, err, _expect(fn, rows, valid), "encoder")
    # without the in-buffer promise (literals, staged columns at a buffer's end), and through the case maps
    for text_map, inbuf in ((0, 0), (1, 1), (2, 0)):
        sub, v = rows[:20_000], valid[:20_000]
        got, err = _run(enclib, fn, sub, v, inbuf=inbuf, text_map=text_map)
        _check(got, err, _expect(fn, sub, v, text_map), f"encoder map {text_map} inbuf {inbuf}")


@pytest.mark.parametrize("fn", [UNHEX, UNB64], ids=["unhex", "unbase64"])
def test_host_decoders_against_the_restatement(enclib, fn):
    rng = np.random.default_rng(41 + fn)
    rows = _decoder_rows(rng, N_ROWS, fn)
    rows[:8] = [b"", b"QQ=", b"Q=Q=", b"QQ==QQ==", b"Q Q=", b"QR==", b"====", b"4"]
    valid = rng.random(N_ROWS) >= 0.1
    want = _expect(fn, rows, valid)
    assert 0.05 < sum(we for _, we in want) / N_ROWS < 0.15
    got, err = _run(enclib, fn, rows, valid, factor=1)
    _check(got, err, want, "decoder")
    # a null row never raises, whatever its bytes are
    assert not any(e for e, v in zip(err, valid) if not v) and any(not v and we for v, (_, we) in zip(valid, _expect(fn, rows, np.ones(N_ROWS))))
    sub, v = rows[:20_000], valid[:20_000]
    got, err = _run(enclib, fn, sub, v, inbuf=0, factor=1)
    _check(got, err, _expect(fn, sub, v), "decoder without the in-buffer promise")
    if fn == UNHEX:  # digits keep their meaning under a case map; base64 text does not, and is read through it all the same
        got, err = _run(enclib, fn, sub, v, text_map=1, factor=1)
        _check(got, err, _expect(fn, sub, v, 1), "unhex(upper())")
    else:
        got, err = _run(enclib, fn, sub, v, text_map=2, factor=1)
        _check(got, err, _expect(fn, sub, v, 2), "unbase64(lower())")


@pytest.mark.parametrize("fn", [HEX, UNHEX, B64, UNB64], ids=["hex", "unhex", "base64", "unbase64"])
def test_host_copy_at_every_alignment(enclib, fn):
    """every source and destination pointer position mod 8, lengths 0..70"""
    rng = np.random.default_rng(51 + fn)
    base = [bytes(rng.integers(0, 256, k, dtype=np.uint8)) for k in range(71)]
    rows = base if fn in (HEX, B64) else [hex_of(r) if fn == UNHEX else base64_of(r) for r in base]
    valid = np.ones(len(rows), dtype=np.uint8)
    for lead in range(8):
        for shift in range(8):
            got, err = _run(enclib, fn, rows, valid, shift=shift, lead=lead, inbuf=(lead + shift) & 1)
            _check(got, err, _expect(fn, rows, valid), f"lead {lead} shift {shift}")


def test_host_length_functions_read_no_byte_but_unbase64s_last_word(enclib):
    """the lengths a pre-pass computes: from the source length alone; unbase64 from the row's last two bytes too — every other
    byte of the buffer may be anything"""
    rng = np.random.default_rng(61)
    rows = _random_bytes(rng, 5000, 0, 40)
    b64 = [base64_of(r) for r in rows]
    for fn, src, want in ((HEX, rows, [2 * len(r) for r in rows]), (B64, rows, [len(base64_of(r)) for r in rows]),
                          (UNHEX, [r + r for r in rows], [len(r) for r in rows]), (UNB64, b64, [len(r) for r in rows])):
        junk = [bytes(rng.integers(0, 256, max(0, len(t) - 2), dtype=np.uint8)) + t[max(0, len(t) - 2):] for t in src]
        off, data = _layout(junk)
        lens = np.zeros(len(src), dtype=np.int32)
        err = np.zeros(len(src), dtype=np.uint8)
        enclib.host_encode_len(fn, _p(off), _p(data), C.c_long(int(off[-1])), C.c_long(len(src)), _p(lens), _p(err))
        assert lens.tolist() == want and not err.any(), fn
    # odd / not-a-multiple-of-4 lengths raise there
    off, data = _layout([b"abc", b"abcde"])
    lens, err = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.uint8)
    for fn in (UNHEX, UNB64):
        enclib.host_encode_len(fn, _p(off), _p(data), C.c_long(8), C.c_long(2), _p(lens), _p(err))
        assert err.tolist() == [4, 4] and lens.tolist() == [0, 0]


def test_host_round_trips(enclib):
    rng = np.random.default_rng(71)
    rows = _random_bytes(rng, 50_000)
    valid = np.ones(len(rows), dtype=np.uint8)
    for enc, dec in ((HEX, UNHEX), (B64, UNB64)):
        mid, err = _run(enclib, enc, rows, valid)
        assert not err.any()
        back, err = _run(enclib, dec, mid, valid, factor=1)
        assert not err.any() and back == rows


@pytest.mark.parametrize("bits", [32, 64])
def test_host_hex_of_integers(enclib, bits):
    rng = np.random.default_rng(81 + bits)
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    vals = [int(v) for v in rng.integers(lo, hi, 100_000, dtype=np.int64)]
    vals += [int(v) >> int(k) for v, k in zip(rng.integers(lo, hi, 20_000, dtype=np.int64), rng.integers(0, bits, 20_000))]
    vals += [0, 1, -1, lo, hi, 15, 16, 255, 256, 0xABCDEF]
    n = len(vals)
    v = np.asarray(vals, dtype=np.int64)
    for shift in (0, 3):
        out_off = np.zeros(n + 1, dtype=np.int32)
        out = np.full(16 * n + 64, 0xEE, dtype=np.uint8)
        total = enclib.host_hex_int(bits, _p(v), C.c_long(n), shift, _p(out_off), _p(out))
        raw = out.tobytes()
        got = [raw[shift + out_off[i]:shift + out_off[i + 1]] for i in range(n)]
        assert got == [format(x & ((1 << bits) - 1), "X").encode() for x in vals] == [hex_of_int(x, bits) for x in vals]
        assert set(raw[shift + total:]) <= {0xEE}


def test_host_crc32(enclib):
    rng = np.random.default_rng(91)
    rows = _random_bytes(rng, N_ROWS)
    rows[:71] = [bytes(rng.integers(0, 256, k, dtype=np.uint8)) for k in range(71)]
    rows += [b"spark", b"", b"123456789"]
    for lead, inbuf, text_map in ((0, 1, 0), (3, 0, 0), (5, 1, 1), (0, 1, 2)):
        sub = rows if text_map == 0 and lead == 0 else rows[:20_000] + rows[-3:]
        off, data = _layout(sub, lead)
        out = np.zeros(len(sub), dtype=np.int64)
        enclib.host_crc32(_p(off), _p(data), C.c_long(int(off[-1])), C.c_long(len(sub)), inbuf, text_map, _p(out))
        mapped = {0: lambda x: x, 1: ascii_upper, 2: ascii_lower}[text_map]
        assert out.tolist() == [zlib.crc32(mapped(r)) for r in sub]
    assert out[-3] == zlib.crc32(b"spark") == 2635321133 and out[-2] == 0 and crc32_of(b"spark") == 2635321133


def test_host_copy_entry_copies_plain_views_as_before(enclib):
    for k in range(0, 40):
        src = np.frombuffer(bytes(range(97, 97 + k)) + b"\0" * 24, dtype=np.uint8).copy()
        out = np.full(64, 0xEE, dtype=np.uint8)
        enclib.host_plain_copy(_p(src), k, 1, _p(out))
        assert out.tobytes() == ascii_upper(src.tobytes()[:k]) + b"\xee" * (64 - k)


def test_cxx_binary_results_host_only():
    """the new C++ test source of binary results (gandiva_amd/cxx/tests/test_encode_cxx.cc): registry and trees, no GPU"""
    cxx = os.path.join(HERE, "..", "gandiva_amd", "cxx")
    subprocess.check_call(["make", "-C", cxx, "all", "test_cxx"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(cxx, "tests", "test_encode_cxx"), "--host-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "OK (host-only)" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("fn", [HEX, UNHEX, B64, UNB64], ids=["hex", "unhex", "base64", "unbase64"])
def test_host_copy_writes_nothing_past_a_row(enclib, fn):
    """every length 0..70 as the only row of its output: no byte before or behind it changes (in a batch the next row would
    hide a store that runs over)"""
    rng = np.random.default_rng(101 + fn)
    for k in range(71):
        b = bytes(rng.integers(0, 256, k, dtype=np.uint8))
        row = b if fn in (HEX, B64) else hex_of(b) if fn == UNHEX else base64_of(b)
        for shift in (0, 1, 5):
            got, err = _run(enclib, fn, [row], [1], shift=shift, lead=shift)
            _check(got, err, _expect(fn, [row], [1]), f"length {k} shift {shift}")
