"""String tail without a GPU: split_part, substring_index, repeat, space and translate.

PARITY STATUS: recollection (PARITY.md, string tail).  The expected values come from the plain-Python restatement below
(the oracle does not know these functions).  This file checks
  * the registry, through the Python mirror and through libgandiva.so's ExpressionRegistry (the rebuilt pyarrow.gandiva);
  * plans that use them, cross-compiled for gfx950 by hipRTC, and where their kernels read bytes;
  * the Make-time limit of translate (literal from / to only);
  * the product's device functions and the copy entry of translate plans, compiled for the host
    (tests/host_devlib/host_string_tail.cc), against the restatement on random rows."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pyarrow as pa
import pytest

import gandiva_amd as gandiva
from gandiva_amd import _capi, gandiva as gg

HERE = os.path.dirname(os.path.abspath(__file__))
STR, I32, I64 = pa.string(), pa.int32(), pa.int64()
INT32_MAX = 2**31 - 1


class RowError(Exception):
    """the row raises "invalid argument" (an execution error of the whole evaluation)"""


# ------------------------------------------------------------------ the restatement (bytes in, bytes out)

def _occurrences(t, d):
    """starts of the occurrences of d in t, left to right, without overlap"""
    out, i = [], 0
    while True:
        j = t.find(d, i)
        if j < 0:
            return out
        out.append(j)
        i = j + len(d)


def split_part(t, d, index):
    if index < 1:
        raise RowError("split_part index")
    if not t or not d:
        return t
    fields = t.split(d)
    return fields[index - 1] if index <= len(fields) else b""


def substring_index(t, d, count):
    if count == 0 or not t or not d:
        return b""
    occ = _occurrences(t, d)
    n = len(occ)
    if count > 0:
        return t if count > n else t[:occ[count - 1]]
    if -count > n:
        return t
    return t[occ[n + count] + len(d):]


def repeat(t, n):
    if n == 0 or not t:
        return b""
    if n < 0 or len(t) * n > INT32_MAX:
        raise RowError("repeat count")
    return t * n


def space(n):
    if n <= 0:
        return b""
    if n > INT32_MAX:
        raise RowError("space count")
    return b" " * n


def utf8_chars(t):
    """characters of a literal as the planner splits them: runs starting at a byte that is not 10xxxxxx"""
    out = []
    for c in t:
        if not out or (c & 0xC0) != 0x80:
            out.append(bytearray())
        out[-1].append(c)
    return [bytes(x) for x in out]


def _declared(c):
    return 1 if c < 0x80 else 2 if c & 0xE0 == 0xC0 else 3 if c & 0xF0 == 0xE0 else 4 if c & 0xF8 == 0xF0 else 0


def text_chars(t):
    """characters of a text; RowError unless it is UTF-8 (lead byte, complete, continuation bytes 10xxxxxx)"""
    out, i = [], 0
    while i < len(t):
        cl = _declared(t[i])
        if cl == 0 or i + cl > len(t) or any(b & 0xC0 != 0x80 for b in t[i + 1:i + cl]):
            raise RowError("translate: not UTF-8")
        out.append(t[i:i + cl])
        i += cl
    return out


def translate(t, frm, to):
    if not t or not frm:
        return t
    fc, tc = utf8_chars(frm), utf8_chars(to)
    m = {}
    for i, ch in enumerate(fc):
        if len(ch) <= 4 and ch not in m:
            m[ch] = tc[i] if i < len(tc) else b""
    return b"".join(m.get(ch, ch) for ch in text_chars(t))


def ascii_upper(t):
    return bytes(c - 32 if 0x61 <= c <= 0x7A else c for c in t)


def ascii_lower(t):
    return bytes(c + 32 if 0x41 <= c <= 0x5A else c for c in t)


def translate_table(frm, to):
    """the constant-block table the planner builds for translate (layout: gdv_device_lib.hpp, GDV_MAP_TRANSLATE)"""
    fc, tc = utf8_chars(frm), utf8_chars(to)
    if all(c < 0x80 for c in frm + to):
        m = bytearray(range(256))
        seen = set()
        for i, ch in enumerate(fc):
            if ch[0] in seen:
                continue
            seen.add(ch[0])
            m[ch[0]] = tc[i][0] if i < len(tc) else 0xFF
        return struct.pack("<ii8x", 0, 0) + bytes(m)
    entries, seen = [], set()
    for i, ch in enumerate(fc):
        if len(ch) > 4:
            continue
        key = int.from_bytes(ch, "little")
        if key in seen:
            continue
        seen.add(key)
        entries.append((key, tc[i] if i < len(tc) else b""))
    head, data = struct.pack("<ii8x", 1, len(entries)), b""
    at = 16 + 16 * len(entries)
    for key, rep in entries:
        head += struct.pack("<IIII", key, len(rep), at + len(data), 0)
        data += rep
    return head + data


# ------------------------------------------------------------------ 1. registry

WANT = [("split_part", [STR, STR, I32]), ("substring_index", [STR, STR, I32]), ("repeat", [STR, I32]),
        ("space", [I32]), ("space", [I64]), ("translate", [STR, STR, STR])]


def test_registry_lists_the_string_tail():
    sigs = {(s.name(), tuple(s.param_types())): s.return_type() for s in gandiva.get_registered_function_signatures()}
    for name, params in WANT:
        assert sigs.get((name, tuple(params))) == STR, (name, params)


def test_registry_of_the_rebuilt_pyarrow_gandiva_lists_the_string_tail():
    from gandiva_amd import pyarrow_gandiva
    pg = pyarrow_gandiva.load()
    sigs = {(s.name(), tuple(s.param_types())): s.return_type() for s in pg.get_registered_function_signatures()}
    for name, params in WANT:
        assert sigs.get((name, tuple(params))) == STR, (name, params)


# ------------------------------------------------------------------ 2. cross-compile (hipRTC, no GPU)

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
    return sorted(f for f in os.listdir(tmp_path) if f.endswith(".hip"))


SCH = pa.schema([pa.field("s", STR), pa.field("d", STR), pa.field("k", I32)])


def _tree():
    b = gandiva.TreeExprBuilder()
    s, d, k = (b.make_field(SCH.field(i)) for i in range(3))
    return b, s, d, k


def _fn(b, name, args, t=STR):
    return b.make_function(name, args, t)


def _lit(b, v, t=STR):
    return b.make_literal(v, t)


def _texts(tmp_path, files):
    return [open(tmp_path / f).read() for f in files]


def test_projection_with_all_five_cross_compiles(monkeypatch, tmp_path):
    b, s, d, k = _tree()
    exprs = [b.make_expression(_fn(b, "split_part", [s, _lit(b, "/"), _lit(b, 3, I32)]), pa.field("a", STR)),
             b.make_expression(_fn(b, "substring_index", [s, d, k]), pa.field("b", STR)),
             b.make_expression(_fn(b, "repeat", [s, _lit(b, 3, I32)]), pa.field("c", STR)),
             b.make_expression(_fn(b, "space", [k]), pa.field("e", STR)),
             b.make_expression(_fn(b, "translate", [s, _lit(b, "abc"), _lit(b, "xy")]), pa.field("f", STR)),
             b.make_expression(_fn(b, "translate", [s, _lit(b, "aé"), _lit(b, "éa")]), pa.field("g", STR))]
    files = _precompile(monkeypatch, tmp_path, SCH, exprs=exprs)
    assert len(files) >= 2, files
    texts = _texts(tmp_path, files)
    for t in texts:
        for sym in ("split_part_utf8_utf8_int32", "substring_index_utf8_utf8_int32", "repeat_utf8_int32", "space_int32",
                    "gdv_translate"):
            assert sym in t, (sym, files)
    # the main kernel materialises translate values through the separate copy entry
    main = [t for t in texts if "GDV_STAGE_COPY" in t and "gdv_stage_copy" in t]
    assert main and all("gdv_stage_copy_ext" in t or "gdv_stage_copy_mir_ext" in t or "gdv_stage_copy_mirh_ext" in t
                        for t in main), files
    assert any("gdv_str_copy_ext(" in t for t in texts)


def test_plans_without_translate_keep_the_plain_copy(monkeypatch, tmp_path):
    b, s, d, k = _tree()
    exprs = [b.make_expression(_fn(b, "split_part", [s, d, k]), pa.field("a", STR)),
             b.make_expression(_fn(b, "repeat", [s, k]), pa.field("c", STR))]
    for t in _texts(tmp_path, _precompile(monkeypatch, tmp_path, SCH, exprs=exprs)):
        assert "_ext" not in t


def test_filter_on_split_part_cross_compiles(monkeypatch, tmp_path):
    b, s, d, k = _tree()
    cond = b.make_condition(b.make_function("equal", [_fn(b, "split_part", [s, _lit(b, "/"), _lit(b, 3, I32)]),
                                                      _lit(b, "x")], pa.bool_()))
    texts = _texts(tmp_path, _precompile(monkeypatch, tmp_path, SCH, cond=cond))
    assert any("split_part_utf8_utf8_int32" in t for t in texts)


def test_like_over_substring_index_cross_compiles(monkeypatch, tmp_path):
    b, s, d, k = _tree()
    e = b.make_function("like", [_fn(b, "substring_index", [s, _lit(b, "@"), _lit(b, -1, I32)]), _lit(b, "%.org")],
                        pa.bool_())
    texts = _texts(tmp_path, _precompile(monkeypatch, tmp_path, SCH, exprs=[b.make_expression(e, pa.field("m", pa.bool_()))]))
    assert any("substring_index_utf8_utf8_int32" in t and "gdv_like_suffix" in t for t in texts)


BYTE_READERS = ("split_part_utf8_utf8_int32", "substring_index_utf8_utf8_int32", "gdv_translate(")


def _prepass(texts):
    """the wave shape's pre-pass kernel (byte totals per wave tile; no output is written)"""
    return [t for t in texts if "// pre-pass:" in t]


def test_staged_length_of_repeat_cross_compiles(monkeypatch, tmp_path):
    b, s, d, k = _tree()
    e = b.make_function("length", [_fn(b, "repeat", [s, _lit(b, 3, I32)])], I32)
    texts = _texts(tmp_path, _precompile(monkeypatch, tmp_path, SCH, exprs=[b.make_expression(e, pa.field("n", I32))]))
    # the first stage materialises repeat(s, 3) (its length follows from the offsets: a pre-pass that reads no byte);
    # the second stage takes the character count of that column
    stage1 = [t for t in texts if "repeat_utf8_int32" in t]
    stage2 = [t for t in texts if "char_length_utf8" in t]
    assert stage1 and stage2, [t[:200] for t in texts]
    assert _prepass(stage1) and not any(r in t for t in _prepass(stage1) for r in BYTE_READERS)


ARGS = {"split_part": lambda b, s, k: [s, _lit(b, " "), _lit(b, 2, I32)],
        "substring_index": lambda b, s, k: [s, _lit(b, " "), _lit(b, 1, I32)],
        "translate": lambda b, s, k: [s, _lit(b, "abc"), _lit(b, "xyz")],
        "repeat": lambda b, s, k: [s, _lit(b, 2, I32)],
        "repeat_per_row": lambda b, s, k: [s, k],
        "space": lambda b, s, k: [k]}


@pytest.mark.parametrize("name", sorted(ARGS))
def test_prepass_reads_bytes_exactly_where_the_function_needs_them(monkeypatch, tmp_path, name):
    """split_part / substring_index / translate need the bytes for their lengths: the pre-pass runs them over the rows.
    repeat / space (literal or fixed-width counts) are byte-free: a plan restricted to byte-free pre-passes
    (GDV_WAVE_BYTEFREE_ONLY) keeps the wave shape for them and only for them."""
    b, s, d, k = _tree()
    fn = name.split("_per_row")[0]
    exprs = [b.make_expression(_fn(b, fn, ARGS[name](b, s, k)), pa.field("o", STR))]
    needs_bytes = fn in ("split_part", "substring_index", "translate")
    pre = _prepass(_texts(tmp_path / "any", _precompile(monkeypatch, tmp_path / "any", SCH, exprs=exprs)))
    assert len(pre) == 1
    assert any(r in pre[0] for r in BYTE_READERS) == needs_bytes
    monkeypatch.setenv("GDV_WAVE_BYTEFREE_ONLY", "1")
    pre = _prepass(_texts(tmp_path / "bf", _precompile(monkeypatch, tmp_path / "bf", SCH, exprs=exprs)))
    assert len(pre) == (0 if needs_bytes else 1), name


# ------------------------------------------------------------------ 3. Make-time rejections

def test_translate_with_a_per_row_from_fails_at_make():
    b, s, d, k = _tree()
    e = b.make_expression(_fn(b, "translate", [s, d, _lit(b, "xy")]), pa.field("t", STR))
    with pytest.raises(Exception, match=r"translate.*literal from and to"):
        gandiva.make_projector(SCH, [e], pa.default_memory_pool())


def test_translate_with_a_per_row_to_fails_at_make():
    b, s, d, k = _tree()
    e = b.make_expression(_fn(b, "translate", [s, _lit(b, "ab"), d]), pa.field("t", STR))
    with pytest.raises(Exception, match=r"translate.*literal from and to"):
        gandiva.make_projector(SCH, [e], pa.default_memory_pool())


# ------------------------------------------------------------------ 4. the device functions on the host

SRC = os.path.join(HERE, "host_devlib", "host_string_tail.cc")
LIB = os.path.join(HERE, "host_devlib", "libhost_string_tail.so")


@pytest.fixture(scope="module")
def taillib():
    hdr = os.path.join(HERE, "..", "gandiva_amd", "csrc", "gdv_device_lib.hpp")
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off",
                               "-Wno-unused-function", "-Wno-unused-variable", SRC, "-o", LIB])
    return C.CDLL(LIB)


ALPHABET = [b"a", b"b", b"/", b",", b"@", b"x", b"A", b"B", b" ", b"\xc3\xa9", b"\xe2\x82\xac", b"\xf0\x9f\x99\x82", b"ab",
            b"//"]
DELIMS = [b"/", b",", b"ab", b"//", b"a/", b"\xc3\xa9", b"\xe2\x82\xac/", b"B", b"@@x", b"longer-delimiter"]


def _random_texts(rng, n, non_ascii=True, invalid=0.0):
    alpha = ALPHABET if non_ascii else [a for a in ALPHABET if a[0] < 0x80]
    out = []
    for _ in range(n):
        m = int(rng.integers(0, 24)) if rng.random() < 0.9 else int(rng.integers(0, 90))
        t = b"".join(alpha[int(rng.integers(0, len(alpha)))] for _ in range(m))
        if invalid and t and rng.random() < invalid:
            at = int(rng.integers(0, len(t)))
            t = t[:at] + [b"\x80", b"\xc3", b"\xff", b"\xe2\x82"][int(rng.integers(0, 4))] + t[at:]
        out.append(t)
    return out


def _pack(rows):
    off = np.zeros(len(rows) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(r) for r in rows])
    data = np.frombuffer(b"".join(rows) + b"\0" * 24, dtype=np.uint8).copy()
    return off, data, int(off[-1])


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _run(lib, fn, texts, k=None, delim=None, delims=None, table=None, text_map=0, dmap=0, inbuf=0, ascii=0):
    n = len(texts)
    off0, d0, s0 = _pack(texts)
    off1 = d1 = None
    s1 = 0
    if delims is not None:
        off1, d1, s1 = _pack(delims)
    lit = np.frombuffer((delim or b"") + b"\0" * 16, dtype=np.uint8).copy()
    kk = np.zeros(n, dtype=np.int32) if k is None else np.asarray(k, dtype=np.int32)
    tab = np.frombuffer((table or b"\0" * 16) + b"\0" * 16, dtype=np.uint8).copy()
    if fn == 2:
        cap = sum(len(t) * int(x) for t, x in zip(texts, kk) if 0 < len(t) * int(x) <= INT32_MAX)
    elif fn == 3:
        cap = int(np.clip(kk, 0, None).sum())
    else:
        cap = 4 * s0
    out_off = np.zeros(n + 1, dtype=np.int32)
    out = np.zeros(cap + 64, dtype=np.uint8)
    err = np.zeros(n, dtype=np.uint8)
    lib.host_string_tail.restype = C.c_long
    total = lib.host_string_tail(fn, _p(off0), _p(d0), C.c_long(s0), _p(off1), _p(d1), C.c_long(s1), _p(lit),
                                 len(delim or b""), _p(kk), _p(tab), C.c_long(n), text_map, dmap, inbuf, ascii,
                                 _p(out_off), _p(out), _p(err))
    assert total <= cap
    raw = out.tobytes()
    return [raw[out_off[i]:out_off[i + 1]] for i in range(n)], err


def _want(f, *args):
    try:
        return f(*args), 0
    except RowError:
        return b"", 4


def _check(got, err, want, what):
    for i, ((g, e), (w, we)) in enumerate(zip(zip(got, err), want)):
        assert (e != 0) == (we != 0), f"{what} row {i}: error bits {e}, want {'an error' if we else 'none'}"
        if not we:
            assert g == w, f"{what} row {i}: {g!r} != {w!r}"


def _mapped(t, m):
    return ascii_upper(t) if m == 1 else ascii_lower(t) if m == 2 else t


COUNTS = [0, 1, -1, 2, -2, 3, -3, 7, -7, 40, -40, 2**31 - 1, -2**31]


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("fn", [0, 1])
def test_split_part_and_substring_index_on_host(taillib, seed, fn):
    rng = np.random.default_rng(9100 + 10 * seed + fn)
    ref = split_part if fn == 0 else substring_index
    n = 2500
    texts = _random_texts(rng, n)
    k = [COUNTS[int(rng.integers(0, len(COUNTS)))] if rng.random() < 0.4 else int(rng.integers(-6, 7)) for _ in range(n)]
    for delim in DELIMS[:6] + [DELIMS[int(rng.integers(6, len(DELIMS)))]]:
        for text_map in (0, 1, 2):
            for inbuf in (0, 1):
                got, err = _run(taillib, fn, texts, k=k, delim=delim, text_map=text_map, inbuf=inbuf)
                want = [_want(ref, _mapped(t, text_map), delim, kk) for t, kk in zip(texts, k)]
                _check(got, err, want, f"fn {fn} delim {delim!r} map {text_map} inbuf {inbuf}")
    # per-row delimiters, some empty, read through a case map of their own
    delims = [DELIMS[int(rng.integers(0, len(DELIMS)))] if rng.random() < 0.9 else b"" for _ in range(n)]
    for text_map, dmap in ((0, 0), (1, 1), (0, 2), (2, 0)):
        for inbuf in (0, 1):
            got, err = _run(taillib, fn, texts, k=k, delims=delims, text_map=text_map, dmap=dmap, inbuf=inbuf)
            want = [_want(ref, _mapped(t, text_map), _mapped(d, dmap), kk) for t, d, kk in zip(texts, delims, k)]
            _check(got, err, want, f"fn {fn} per-row delimiters map {text_map}/{dmap} inbuf {inbuf}")


def test_split_part_edges_on_host(taillib):
    cases = [(b"", b"/", 1), (b"a/b/c", b"", 2), (b"/a/", b"/", 1), (b"/a/", b"/", 2), (b"/a/", b"/", 3), (b"/a/", b"/", 4),
             (b"a//b", b"/", 2), (b"a//b", b"/", 3), (b"abc", b"/", 1), (b"abc", b"/", 2), (b"a\xe2\x82\xacb", b"\xe2\x82\xac", 2),
             (b"aaa", b"aa", 2), (b"x", b"/", 0), (b"x", b"/", -5)]
    for fn, ref in ((0, split_part), (1, substring_index)):
        texts = [c[0] for c in cases]
        for inbuf in (0, 1):
            for i, (t, d, kk) in enumerate(cases):
                got, err = _run(taillib, fn, [t], k=[kk], delim=d, inbuf=inbuf)
                _check(got, err, [_want(ref, t, d, kk)], f"fn {fn} {cases[i]} inbuf {inbuf}")
        del texts


@pytest.mark.parametrize("seed", range(3))
def test_repeat_and_space_on_host(taillib, seed):
    rng = np.random.default_rng(9200 + seed)
    n = 3000
    texts = _random_texts(rng, n)
    k = [int(rng.integers(-3, 9)) if rng.random() < 0.95 else [0, -1, -2**31, 2**31 - 1, 1 << 20][int(rng.integers(0, 5))]
         for _ in range(n)]
    # huge counts over texts of two bytes or more: above INT32_MAX (an error) or a few MiB
    texts = [t + b"ab" if x > 1000 else t for t, x in zip(texts, k)]
    for text_map in (0, 1, 2):
        got, err = _run(taillib, 2, texts, k=k, text_map=text_map)
        _check(got, err, [_want(repeat, _mapped(t, text_map), kk) for t, kk in zip(texts, k)], f"repeat map {text_map}")
    ks = [int(rng.integers(-5, 70)) for _ in range(n)]
    got, err = _run(taillib, 3, [b""] * n, k=ks)
    _check(got, err, [_want(space, kk) for kk in ks], "space")


def test_space_int64_bounds_on_host(taillib):
    k = np.array([0, -1, 5, 2**31 - 1, 2**31, 2**40, -2**63], dtype=np.int64)
    out_len = np.zeros(len(k), dtype=np.int32)
    err = np.zeros(len(k), dtype=np.uint8)
    taillib.host_space64(_p(k), C.c_long(len(k)), _p(out_len), _p(err))
    assert list(out_len) == [0, 0, 5, 2**31 - 1, 0, 0, 0]
    assert list(err != 0) == [False, False, False, False, True, True, False]


TRANSLATES = [(b"abc", b"xyz"), (b"abc", b"x"), (b"aab", b"xyz"), (b"/ ,", b""), (b"aB", b"Ba"), (b"a\xc3\xa9", b"\xc3\xa9a"),
              (b"\xe2\x82\xac", b"E"), (b"a", b"\xf0\x9f\x99\x82"), (b"\xc3\xa9\xc3\xa9a", b"1\xe2\x82\xac2"),
              (b"\xf0\x9f\x99\x82b", b""), (b"x/", b"/x")]


@pytest.mark.parametrize("seed", range(3))
def test_translate_on_host(taillib, seed):
    rng = np.random.default_rng(9300 + seed)
    n = 2500
    for non_ascii in (False, True):
        texts = _random_texts(rng, n, non_ascii=non_ascii, invalid=0.05 if non_ascii else 0.0)
        for frm, to in TRANSLATES:
            for text_map in (0, 1, 2):
                ascii = int(not non_ascii and text_map == 0)
                got, err = _run(taillib, 4, texts, table=translate_table(frm, to), text_map=text_map, ascii=ascii)
                want = [_want(translate, _mapped(t, text_map), frm, to) for t in texts]
                _check(got, err, want, f"translate {frm!r} -> {to!r} map {text_map}")


def test_translate_invalid_utf8_raises_on_host(taillib):
    bad = [b"\x80", b"a\xc3", b"\xc3A", b"\xff", b"\xe2\x82", b"ok\xf0\x9f\x99"]
    for frm, to in ((b"a", b"b"), (b"\xc3\xa9", b"e")):
        got, err = _run(taillib, 4, bad + [b"fine \xc3\xa9"], table=translate_table(frm, to))
        assert all(e != 0 for e in err[:-1]) and err[-1] == 0
        assert got[-1] == translate(b"fine \xc3\xa9", frm, to)
