"""mask, mask_first_n, mask_last_n, mask_show_first_n, mask_show_last_n without a GPU.

PARITY STATUS (PARITY.md, `mask`): recollection + decisions.  No second engine knows these functions, so the rules are restated
here in plain Python (`restate`) and that restatement is checked against engines that share no code with it: re.sub with
[A-Z] / [a-z] / [0-9] for the whole-string mask, str slicing by code points plus that re.sub for the four n forms on valid UTF-8,
pyarrow.compute.utf8_length for the character count, and the issue's examples as hand vectors.  DIVERGENCE (stated): characters
outside ASCII are copied, never classified, so the result always has the text's byte length.

This file checks
  * the registry (gandiva_amd and the rebuilt pyarrow.gandiva list the eight signatures);
  * the restatement;
  * the product's device functions compiled for the host (tests/host_devlib/host_mask.cc) against the restatement, bit for bit,
    on rows of every interesting length at the very end of their buffers, with and without GDV_STR_INBUF, through views that
    carry an ASCII case map, with guard bytes around every destination;
  * the same functions under AddressSanitizer / UBSan as a stand-alone child process (tests/cxx/mask_check.cc);
  * the planner (plans cross-compile for gfx950, the pre-pass reads no byte, consumers are staged, Make-time refusals, plans
    without a mask function do not mention the new symbols);
  * that the C++ test builds and its trees build."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import gandiva_amd as gandiva

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "gandiva_amd", "csrc")
STR, I32, BOOL = pa.string(), pa.int32(), pa.bool_()
INT32_MIN, INT32_MAX = -2**31, 2**31 - 1

MODES = {"mask": 0, "mask_first_n": 1, "mask_last_n": 2, "mask_show_first_n": 3, "mask_show_last_n": 4}
N_FORMS = ("mask_first_n", "mask_last_n", "mask_show_first_n", "mask_show_last_n")
LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 257, 4101)
WANT = [("mask", [STR] * k) for k in (1, 2, 3, 4)] + [(f, [STR, I32]) for f in N_FORMS]


# ------------------------------------------------------------------ the rules, restated

def _table(reps):
    t = bytearray(range(256))
    for lo, hi, r in ((65, 90, reps[0]), (97, 122, reps[1]), (48, 57, reps[2])):
        for c in range(lo, hi + 1):
            t[c] = r
    return bytes(t)


def restate(fn, text, n=0, reps=b"Xxn", text_map=0):
    """the rules of the issue on the bytes `text`: a character starts at every byte that is not 10xxxxxx; with c characters and
    k = min(max(n, 0), c) the masked characters are [0, c) / [0, k) / [c - k, c) / [k, c) / [0, c - k); a masked byte A-Z, a-z,
    0-9 becomes reps[0], reps[1], reps[2], every other byte stays.  text_map: the argument is upper(text) (1) / lower(text) (2),
    ASCII letters only."""
    if text_map:
        text = text.upper() if text_map == 1 else text.lower()   # (bytes.upper / lower: ASCII letters only)
    starts = [i for i, b in enumerate(text) if b & 0xC0 != 0x80] + [len(text)]
    c = len(starts) - 1
    k = min(max(n, 0), c)
    c0, c1 = {"mask": (0, c), "mask_first_n": (0, k), "mask_last_n": (c - k, c), "mask_show_first_n": (k, c),
              "mask_show_last_n": (0, c - k)}[fn]
    # (bytes in front of the first character — continuation bytes — belong to none and are >= 0x80 anyway)
    b0, b1 = starts[c0], starts[c1]
    return text[:b0] + text[b0:b1].translate(_table(reps)) + text[b1:]


def _resub(s, reps="Xxn"):
    return re.sub("[0-9]", reps[2], re.sub("[a-z]", reps[1], re.sub("[A-Z]", reps[0], s)))


def _by_slicing(fn, s, n):
    c = len(s)
    k = min(max(n, 0), c)
    if fn == "mask_first_n":
        return _resub(s[:k]) + s[k:]
    if fn == "mask_last_n":
        return s[:c - k] + _resub(s[c - k:])
    if fn == "mask_show_first_n":
        return s[:k] + _resub(s[k:])
    return _resub(s[:c - k]) + s[c - k:]


def _fill(n, shift=0):
    cyc = b"aB3-Zz09 Qx"
    return bytes(cyc[(i + shift) % len(cyc)] for i in range(n))


def edge_rows():
    """rows of every length in LENGTHS: ASCII of all four classes; a 2-, 3- or 4-byte character across every 8-byte word
    boundary it fits on, at the first and at the last position; continuation bytes only; rows that end in a cut character"""
    rows = []
    for L in LENGTHS:
        rows.append(_fill(L))
        rows.append(b"\x80" * L)
        if L >= 1:
            rows.append(_fill(L - 1) + b"\xc3")
        if L >= 2:
            rows.append(_fill(L - 2) + b"\xe2\x82")
        for ch in ("é", "€", "\U00010428"):
            e = ch.encode()
            if L < len(e):
                continue
            t = bytearray(_fill(L))
            for b in range(8, L, 8):
                if b - 1 + len(e) <= L:
                    t[b - 1:b - 1 + len(e)] = e
            assert len(t) == L
            rows += [bytes(t), e + _fill(L - len(e)), _fill(L - len(e)) + e]
    return rows


def char_count(b):
    return sum(1 for x in b if x & 0xC0 != 0x80)


def n_values(c):
    return sorted({INT32_MIN, -1, 0, 1, 7, 8, 9, c - 1, c, c + 1, INT32_MAX})


def random_rows(rng, count, max_len=40):
    """texts of 0..max_len bytes over an alphabet of all classes; about one in eight is cut to an arbitrary byte prefix, so it may
    end inside a character"""
    alphabet = list("abzAZQ09 5-_@[`{/:") + ["é", "É", "ß", "日", "€", "\U00010428", "ñ"]
    out = []
    for _ in range(count):
        want = int(rng.integers(0, max_len + 1))
        t = b""
        while True:
            e = alphabet[int(rng.integers(0, len(alphabet)))].encode()
            if len(t) + len(e) > want:
                break
            t += e
        if rng.random() < 0.125 and t:
            t = t[:int(rng.integers(0, len(t) + 1))]
        out.append(t)
    return out


# ------------------------------------------------------------------ 1. registry

def test_registry_lists_the_masking_family():
    sigs = {(s.name(), tuple(s.param_types())): s.return_type() for s in gandiva.get_registered_function_signatures()}
    for name, params in WANT:
        assert sigs.get((name, tuple(params))) == STR, (name, params)
    assert sum(1 for (name, _) in sigs if name.startswith("mask")) == 8


def test_registry_of_the_rebuilt_pyarrow_gandiva_lists_the_masking_family():
    from gandiva_amd import pyarrow_gandiva
    pg = pyarrow_gandiva.load()
    sigs = {(s.name(), tuple(s.param_types())): s.return_type() for s in pg.get_registered_function_signatures()}
    for name, params in WANT:
        assert sigs.get((name, tuple(params))) == STR, (name, params)


# ------------------------------------------------------------------ 2. the restatement

def test_restatement_on_the_examples_of_the_issue():
    r = lambda fn, s, *a, **k: restate(fn, s.encode(), *a, **k).decode()
    assert r("mask", "Héllo 42") == "Xéxxx nn"
    assert r("mask", "Ab1", reps=b"Ul#") == "Ul#"
    assert r("mask_first_n", "Hello-123", 4) == "Xxxxo-123"
    assert r("mask_last_n", "Hello-123", 4) == "Hello-nnn"
    assert r("mask_show_first_n", "Hello-123", 2) == "Hexxx-nnn"
    assert r("mask_show_last_n", "Hello-123", 2) == "Xxxxx-n23"
    assert r("mask_first_n", "éA", 1) == "éA"
    assert r("mask_first_n", "éA", 2) == "éX"
    assert r("mask", "ab1", text_map=1) == "XXn"
    for fn in MODES:
        assert restate(fn, b"", 3) == b""
    # n <= 0 masks nothing for the first two and everything for the show pair; INT32_MIN / INT32_MAX are ordinary
    for n in (0, -1, INT32_MIN):
        assert r("mask_first_n", "Ab1", n) == "Ab1" and r("mask_last_n", "Ab1", n) == "Ab1"
        assert r("mask_show_first_n", "Ab1", n) == "Xxn" and r("mask_show_last_n", "Ab1", n) == "Xxn"
    assert r("mask_first_n", "Ab1", INT32_MAX) == "Xxn" and r("mask_show_last_n", "Ab1", INT32_MAX) == "Ab1"


def test_restatement_against_re_sub_slicing_and_utf8_length():
    rng = np.random.default_rng(5)
    rows = [t for t in random_rows(rng, 3000) + edge_rows() if _is_utf8(t)]
    assert len(rows) > 2500 and any(len(t) > 4096 for t in rows)
    counts = pc.utf8_length(pa.array([t.decode() for t in rows], STR)).to_pylist()
    for t, c in zip(rows, counts):
        s = t.decode()
        assert char_count(t) == c == len(s)
        assert restate("mask", t).decode() == _resub(s)
        assert restate("mask", t, reps=b"U#l").decode() == _resub(s, "U#l")
        assert len(restate("mask", t)) == len(t)
        for fn in N_FORMS:
            for n in n_values(c) if len(t) <= 70 else (3, c - 1):
                got = restate(fn, t, n)
                assert got.decode() == _by_slicing(fn, s, n), (fn, s, n)
                assert len(got) == len(t)


def _is_utf8(b):
    try:
        b.decode()
        return True
    except UnicodeDecodeError:
        return False


# ------------------------------------------------------------------ 3. the device functions on the host

@pytest.fixture(scope="module")
def masklib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_mask") / "libhost_mask.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unused-function",
                           "-Wno-unused-variable", "-Wno-attributes", os.path.join(HERE, "host_devlib", "host_mask.cc"), "-o", out])
    lib = C.CDLL(out)
    lib.host_mask.restype = C.c_long
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def run_host(lib, fn, rows, ns, reps=b"Xxn", valid=None, text_map=0, inbuf=1):
    """-> the result rows; asserts that no byte outside a destination was written and every byte inside was"""
    n = len(rows)
    off = np.zeros(n + 1, dtype=np.int32)
    np.cumsum([len(r) for r in rows], out=off[1:])
    data = np.frombuffer(b"".join(rows) + b"\0", dtype=np.uint8)
    ns = np.ascontiguousarray(ns, dtype=np.int32)
    assert len(ns) == n
    valid = np.ones(n, dtype=np.uint8) if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    out_off = np.zeros(n + 1, dtype=np.int32)
    out = np.zeros(int(off[-1]) + 1, dtype=np.uint8)
    unwritten = C.c_long(-1)
    packed = reps[0] | reps[1] << 8 | reps[2] << 16
    outside = lib.host_mask(MODES[fn], _p(ns), C.c_uint(packed), _p(off), _p(data), _p(valid), C.c_long(n), text_map, inbuf,
                            _p(out_off), _p(out), C.byref(unwritten))
    assert outside == 0, "%d bytes written outside [dst, dst + len)" % outside
    assert unwritten.value == 0, "%d bytes of a result left unwritten" % unwritten.value
    raw = out.tobytes()
    return [raw[out_off[i]:out_off[i + 1]] for i in range(n)]


def _check(lib, fn, rows, ns, **kw):
    want = [restate(fn, t, int(n), kw.get("reps", b"Xxn"), kw.get("text_map", 0)) for t, n in zip(rows, ns)]
    for inbuf in (1, 0):
        got = run_host(lib, fn, rows, ns, inbuf=inbuf, **kw)
        bad = [i for i in range(len(rows)) if got[i] != want[i]]
        assert not bad, (fn, inbuf, kw, [(rows[i][:40], int(ns[i]), got[i][:40], want[i][:40]) for i in bad[:3]])


def test_edge_rows_with_every_n_on_host(masklib):
    rows = edge_rows()
    assert {len(r) for r in rows} == set(LENGTHS) and max(len(r) for r in rows) > 4096
    _check(masklib, "mask", rows, [0] * len(rows))
    _check(masklib, "mask", rows, [0] * len(rows), reps=b"U#l")
    pairs = [(t, n) for t in rows for n in n_values(char_count(t))]
    for fn in N_FORMS:
        _check(masklib, fn, [t for t, _ in pairs], [n for _, n in pairs])


@pytest.mark.parametrize("text_map", [1, 2])
def test_views_that_carry_an_ascii_case_map_on_host(masklib, text_map):
    rows = [r for r in edge_rows() if len(r) <= 257]
    _check(masklib, "mask", rows, [0] * len(rows), text_map=text_map, reps=b"Ul#")
    pairs = [(t, n) for t in rows for n in (1, 8, char_count(t) - 1)]
    for fn in N_FORMS:
        _check(masklib, fn, [t for t, _ in pairs], [n for _, n in pairs], text_map=text_map, reps=b"Ul#")


@pytest.mark.parametrize("seed", [1, 2])
def test_random_rows_on_host(masklib, seed):
    rng = np.random.default_rng(seed)
    rows = random_rows(rng, 20000)
    ns = rng.integers(-2, 44, len(rows))
    assert any(not _is_utf8(t) for t in rows)
    for fn in MODES:
        _check(masklib, fn, rows, ns)
    _check(masklib, "mask_last_n", rows, ns, text_map=1 + seed % 2, reps=b"#l*")


def test_null_rows_are_not_evaluated_on_host(masklib):
    rows = [b"Hello-123", b"Ab1", b"", b"H\xc3\xa9llo 42"]
    got = run_host(masklib, "mask", rows, [0] * 4, valid=[1, 0, 1, 1])
    assert got == [b"Xxxxx-nnn", b"", b"", b"X\xc3\xa9xxx nn"]


# ------------------------------------------------------------------ 4. under sanitizers, as a child process

@pytest.mark.parametrize("name,extra", [("plain", []), ("asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"])])
def test_walks_and_copy_stay_inside_their_buffers(tmp_path, name, extra):
    exe = str(tmp_path / ("mask_check_" + name))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-unused-function", "-Wno-unused-variable", "-Wno-attributes"] +
                          extra + ["-I", CSRC, os.path.join(HERE, "cxx", "mask_check.cc"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, f"exit {run.returncode}\n{run.stdout}\n{run.stderr}"
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    assert "mask_check: ok" in run.stdout


# ------------------------------------------------------------------ 5. the planner

SCH = pa.schema([pa.field("s", STR), pa.field("t", STR), pa.field("k", I32)])
NEW_SYMBOLS = ("gdv_mask", "GDV_COPY_MASK", "GDV_MAP_MASK", "gdv_copy_masked", "GDV_MASK_")
# what reads a row's bytes in a pre-pass (test_string_tail_cpu.BYTE_READERS) and the readers a mask plan could be tempted by
BYTE_READERS = ("split_part_utf8_utf8_int32", "substring_index_utf8_utf8_int32", "gdv_translate(", "gdv_utf8_case(", "gdv_utf8_count",
                "char_length_utf8", "gdv_copy_masked", "gdv_mask_pos", "gdv_word_at", "gdv_load8")


class T:
    def __init__(self, schema=SCH):
        self.b = gandiva.TreeExprBuilder()
        self.f = {f.name: self.b.make_field(f) for f in schema}

    def lit(self, v, t=STR):
        return self.b.make_literal(v, t)

    def fn(self, name, args, t=STR):
        return self.b.make_function(name, args, t)

    def expr(self, node, name="o", t=STR):
        return self.b.make_expression(node, pa.field(name, t))

    def all_eight(self, n_node=None):
        """the eight signatures over column s; n: the literal 4 or the given node"""
        s = self.f["s"]
        n = (lambda: self.lit(4, I32)) if n_node is None else (lambda: n_node)
        return [self.expr(self.fn("mask", [s]), "m1"),
                self.expr(self.fn("mask", [s, self.lit("U")]), "m2"),
                self.expr(self.fn("mask", [s, self.lit("U"), self.lit("l")]), "m3"),
                self.expr(self.fn("mask", [s, self.lit("U"), self.lit("l"), self.lit("#")]), "m4")] + \
               [self.expr(self.fn(f, [s, n()]), f) for f in N_FORMS]


def _sources(monkeypatch, tmp_path, exprs, schema=SCH):
    from test_planner_cpu import _precompile
    tmp_path.mkdir(parents=True, exist_ok=True)
    files = _precompile(monkeypatch, tmp_path, schema, exprs=exprs if isinstance(exprs, list) else [exprs])
    return {f[:-4]: open(tmp_path / f).read() for f in files}


def _body(text):
    return text.split('#include "gdv_device_lib.hpp"')[-1]


def _prepass(src):
    return [t for t in src.values() if "// pre-pass:" in t]


@pytest.mark.parametrize("per_row_n", [False, True], ids=["literal_n", "column_n"])
def test_projection_with_all_eight_cross_compiles_and_its_prepass_reads_no_byte(monkeypatch, tmp_path, per_row_n):
    t = T()
    exprs = t.all_eight(t.f["k"] if per_row_n else None)
    src = _sources(monkeypatch, tmp_path / "any", exprs)   # (_precompile compiles every kernel of the plan for gfx950)
    assert src
    for text in src.values():
        assert "gdv_mask(" in _body(text)
    main = [x for x in src.values() if "// pre-pass:" not in x]
    assert main and all("GDV_COPY_MASK(dst, v, " in x for x in main)
    pre = _prepass(src)
    assert pre, "the plan takes the wave shape"
    for p in pre:
        assert not any(r in _body(p) for r in BYTE_READERS), [r for r in BYTE_READERS if r in _body(p)]
    # restricted to byte-free pre-passes the plan keeps the wave shape
    monkeypatch.setenv("GDV_WAVE_BYTEFREE_ONLY", "1")
    assert _prepass(_sources(monkeypatch, tmp_path / "bf", exprs))


def test_replacement_bytes_and_n_are_compiled_in(monkeypatch, tmp_path):
    t = T()
    src = _sources(monkeypatch, tmp_path, [t.expr(t.fn("mask", [t.f["s"], t.lit("U"), t.lit("l"), t.lit("#")])),
                                           t.expr(t.fn("mask_show_last_n", [t.f["s"], t.lit(4, I32)]), "p")])
    packed = ord("U") | ord("l") << 8 | ord("#") << 16
    default = ord("X") | ord("x") << 8 | ord("n") << 16
    assert any(re.search(r"gdv_mask\(\w+, 0, \(gdv_int32\)\(0\), %du\)" % packed, _body(x)) for x in src.values())
    assert any(re.search(r"gdv_mask\(\w+, 4, \(gdv_int32\)\(.*4.*\), %du\)" % default, _body(x)) for x in src.values())


def _stages(src):
    first = {n: x for n, x in src.items() if "__gdv_stage" not in x}
    second = {n: x for n, x in src.items() if "__gdv_stage0" in x}
    return first, second


def test_consumers_of_the_value_run_as_staged_plans(monkeypatch, tmp_path):
    t = T()
    s, u = t.f["s"], t.f["t"]
    cases = {
        "like": (t.expr(t.fn("like", [t.fn("mask", [s]), t.lit("Xx%")], BOOL), "o", BOOL), 1, "gdv_like"),
        "length": (t.expr(t.fn("length", [t.fn("mask_first_n", [s, t.lit(3, I32)])], I32), "o", I32), 1, "char_length_utf8"),
        "upper": (t.expr(t.fn("upper", [t.fn("mask", [s])])), 1, "upper_utf8"),
        "equal": (t.expr(t.fn("equal", [t.fn("mask", [s]), t.fn("mask", [u])], BOOL), "o", BOOL), 2, "equal_utf8_utf8"),
    }
    for name, (e, hoisted, consumer) in cases.items():
        src = _sources(monkeypatch, tmp_path / name, e)
        first, second = _stages(src)
        assert first and second, name
        assert all("gdv_mask(" in _body(x) for x in first.values()), name
        assert any("__gdv_stage%d" % (hoisted - 1) in x for x in second.values()), name
        # the consumer reads plain columns: no mask value in its plan
        assert all(not any(sym in _body(x) for sym in NEW_SYMBOLS) for x in second.values()), name
        assert any(consumer in _body(x) for x in second.values()), name


def test_concat_takes_the_value_in_one_plan(monkeypatch, tmp_path):
    t = T()
    s = t.f["s"]
    src = _sources(monkeypatch, tmp_path, t.expr(t.fn("concat", [t.fn("mask", [s]), t.lit("-"), s])))
    first, second = _stages(src)
    assert first and not second
    assert all("gdv_mask(" in _body(x) for x in first.values())


def test_mask_reads_its_argument_through_an_ascii_case_map_in_one_plan(monkeypatch, tmp_path):
    t = T()
    src = _sources(monkeypatch, tmp_path, t.expr(t.fn("mask", [t.fn("upper", [t.f["s"]])])))
    first, second = _stages(src)
    assert first and not second
    assert all("upper_utf8(" in _body(x) and "gdv_mask(" in _body(x) for x in first.values())


def test_a_plan_without_mask_functions_mentions_none_of_the_new_symbols(monkeypatch, tmp_path):
    t = T()
    s = t.f["s"]
    exprs = [t.expr(t.fn("like", [s, t.lit("%spark%")], BOOL), "a", BOOL),
             t.expr(t.fn("substr", [s, t.lit(2, pa.int64()), t.lit(5, pa.int64())]), "b"),
             t.expr(t.fn("upper", [s]), "c"),
             t.expr(t.fn("translate", [s, t.lit("abc"), t.lit("xyz")]), "d"),
             t.expr(t.fn("repeat", [s, t.lit(2, I32)]), "e")]
    src = _sources(monkeypatch, tmp_path, exprs)
    assert src
    for name, text in src.items():
        assert re.fullmatch(r"gdv_k_[0-9a-f]{16}", name)
        assert not any(sym in _body(text) for sym in NEW_SYMBOLS), [sym for sym in NEW_SYMBOLS if sym in _body(text)]


REFUSED = {"per_row": lambda t: t.f["t"], "empty": lambda t: t.lit(""), "two_bytes": lambda t: t.lit("XY"), "e_acute": lambda t: t.lit("é")}


@pytest.mark.parametrize("which", sorted(REFUSED))
@pytest.mark.parametrize("position", [1, 2, 3])
def test_replacements_that_are_not_one_ascii_byte_literals_fail_at_make(which, position):
    t = T()
    args = [t.f["s"]] + [t.lit("X") for _ in range(position - 1)] + [REFUSED[which](t)]
    e = t.expr(t.fn("mask", args))
    with pytest.raises(gandiva.GandivaError, match=r"(?s)^CodeGenError: .*mask\(.*literal replacement characters of exactly one byte below 0x80"):
        gandiva.make_projector(SCH, [e], pa.default_memory_pool())


def test_null_literals_plan_as_an_all_null_column(monkeypatch, tmp_path):
    t = T()
    s = t.f["s"]
    null_s, null_n = t.b.make_null(STR), t.b.make_null(I32)
    src = _sources(monkeypatch, tmp_path, [t.expr(t.fn("mask", [s, null_s]), "a"), t.expr(t.fn("mask", [s, t.lit("U"), t.lit("l"), null_s]), "b"),
                                           t.expr(t.fn("mask_first_n", [s, null_n]), "c")])
    assert src
    # a NULL replacement: nothing is materialised for it
    assert not any(re.search(r"gdv_mask\(\w+, 0,", _body(x)) for x in src.values())


# ------------------------------------------------------------------ 6. the C++ API

def test_cxx_mask_builds_its_trees_host_only():
    """gandiva_amd/cxx/tests/test_mask_cxx.cc: it builds, the trees build, gandiva::ExpressionRegistry lists the eight signatures"""
    cxx = os.path.join(HERE, "..", "gandiva_amd", "cxx")
    subprocess.check_call(["make", "-C", cxx, "all", "test_cxx"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(cxx, "tests", "test_mask_cxx"), "--host-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "OK (host-only)" in out.stdout, out.stdout + out.stderr
