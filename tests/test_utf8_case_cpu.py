"""upper / lower under GDV_UTF8_CASE=1 at Make, without a GPU.

PARITY STATUS (PARITY.md, `upper lower`): 2-engines.  The second engine is utf8proc itself, linked into this image's libarrow
and reached through pyarrow.compute.utf8_upper / utf8_lower: every expected value here and in test_utf8_case.py comes from
those two calls (the oracle does not know the option).  Decided here: sequences that pass translate's structural rule but are
not Unicode (over-long forms, surrogates, above U+10FFFF) are copied unchanged.

This file checks
  * that the committed table (gandiva_amd/csrc/gdv_utf8_case_table.inc) is what tools/gen_utf8_case_table.py builds today;
  * the product's device functions compiled for the host (tests/host_devlib/host_utf8_case.cc) on every code point, on random
    rows, on rows of forced lengths around the 8-byte word, through views that carry an ASCII case map, on rows that raise;
  * the walker, lookup and copy under AddressSanitizer / UBSan as a stand-alone child process (tests/cxx/utf8_case_check.cc);
  * the planner with the option set (plans cross-compile for gfx950, consumers are staged, names carry the tag) and unset
    (sources and names are the parent's)."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import gandiva_amd as gandiva
from gandiva_amd import workloads as W

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "gandiva_amd", "csrc")
STR = pa.string()

# the alphabet of test_strings.py::test_upper_lower_differ_from_utf8proc_exactly_on_rows_with_cased_non_ascii_letters, widened by
# the length-changing characters (both directions), two four-byte cased pairs
ALPHABET = (list("abcXYZ 09-_") + ["é", "É", "ß", "ñ", "Ω", "ω", "я", "Я", "ı", "ſ", "ÿ", "µ", "日", "本", "€", "ǆ", "ɐ"] +
            ["İ", "Ⱥ", "\u212a", "\u2126", "ẞ", "\U00010428", "\U00010400", "\U0001e922", "\U0001e900"])
FORCED_LENGTHS = (7, 8, 9, 15, 16, 17)


def random_rows(rng, n):
    """n texts of 0..40 bytes over ALPHABET"""
    out = []
    for _ in range(n):
        want = int(rng.integers(0, 41))
        t, size = [], 0
        while True:
            c = ALPHABET[int(rng.integers(0, len(ALPHABET)))]
            if size + len(c.encode()) > want:
                break
            t.append(c)
            size += len(c.encode())
        out.append("".join(t))
    return out


def forced_rows():
    """rows of exactly 7, 8, 9, 15, 16 and 17 bytes: one non-ASCII character at the first, the last and the word-straddling
    position (its bytes lie on both sides of byte 8 where the row is long enough, else in the middle), ASCII letters around it"""
    out = []
    for total in FORCED_LENGTHS:
        for ch in ("é", "ß", "ı", "ɐ", "\u212a", "ẞ", "Ⱥ", "\U00010428", "\U0001e900"):
            cl = len(ch.encode())
            straddle = 7 if 7 + cl <= total else (total - cl) // 2
            for at in sorted({0, total - cl, straddle}):
                fill = "aBcDeFgHiJkLmNoPq"
                row = fill[:at] + ch + fill[at:total - cl]
                assert len(row.encode()) == total
                out.append(row)
    return out


def batch_rows(n, seed, nulls=0.1):
    """the rows of the GPU tests: random rows, the forced ones mixed in where they fit, `nulls` of them null"""
    rng = np.random.default_rng(seed)
    rows = random_rows(rng, n)
    forced = forced_rows()
    if n >= 4 * len(forced):
        for k, r in enumerate(forced):
            rows[(k * 7 + 3) % n] = r
    return [None if rng.random() < nulls else r for r in rows]


def all_code_points():
    """(offsets int32[n + 1], data uint8[...]) of the column that holds every code point but the surrogates, one per row"""
    cps = np.concatenate([np.arange(0, 0xD800, dtype=np.uint32), np.arange(0xE000, 0x110000, dtype=np.uint32)])
    lens = np.where(cps < 0x80, 1, np.where(cps < 0x800, 2, np.where(cps < 0x10000, 3, 4))).astype(np.int32)
    off = np.zeros(len(cps) + 1, dtype=np.int32)
    np.cumsum(lens, out=off[1:])
    data = np.frombuffer("".join(map(chr, cps.tolist())).encode("utf-8"), dtype=np.uint8)
    assert len(data) == off[-1]
    return off, data


def string_array(off, data):
    return pa.StringArray.from_buffers(len(off) - 1, pa.py_buffer(off), pa.py_buffer(data))


def array_buffers(arr):
    """(offsets, data) of a string array, rebased to offset 0"""
    n = len(arr)
    off = np.frombuffer(arr.buffers()[1], dtype=np.int32)[arr.offset:arr.offset + n + 1]
    data = np.frombuffer(arr.buffers()[2], dtype=np.uint8) if arr.buffers()[2] is not None else np.zeros(0, np.uint8)
    return (off - off[0]).astype(np.int32), data[off[0]:off[-1]]


def arrow_case(upper):
    return pc.utf8_upper if upper else pc.utf8_lower


# ------------------------------------------------------------------ 1. the table

def _tool():
    spec = importlib.util.spec_from_file_location("gen_utf8_case_table", os.path.join(HERE, "..", "tools", "gen_utf8_case_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_committed_table_is_what_pyarrow_gives_today():
    tool = _tool()
    text = open(os.path.join(CSRC, "gdv_utf8_case_table.inc")).read()
    assert text.splitlines()[0].startswith("// generated by tools/gen_utf8_case_table.py from pyarrow " + pa.__version__)
    assert text == tool.render()
    # data only: a comment line and two byte arrays
    body = [l for l in text.splitlines()[1:] if not re.fullmatch(r"\s*(\d+,)+", l)]
    assert [re.sub(r"\[\d+\]", "[]", l) for l in body] == ["static const unsigned char gdv_utf8_upper_table[] = {", "};",
                                                            "static const unsigned char gdv_utf8_lower_table[] = {", "};"]
    for upper in (True, False):
        assert len(tool.table(upper)) <= tool.MAX_BYTES == 16384


def test_the_map_is_what_the_issue_counted():
    """the figures the table's layout rests on: a mapped code point is one code point, 1480 / 1462 change, 34 / 27 change their
    UTF-8 length, and it is not Python's map"""
    tool = _tool()
    up, lo = tool.case_map(True), tool.case_map(False)
    nonascii = lambda m: {k: v for k, v in m.items() if k >= 0x80}
    assert len(nonascii(up)) == 1480 and len(nonascii(lo)) == 1462
    changes = lambda m: sum(tool.utf8_len(k) != tool.utf8_len(v) for k, v in m.items())
    assert changes(up) == 34 and changes(lo) == 27
    assert up[0xDF] == 0x1E9E and "ß".upper() == "SS"


# ------------------------------------------------------------------ 2. the device functions on the host

@pytest.fixture(scope="module")
def caselib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_utf8_case") / "libhost_utf8_case.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unused-function",
                           "-Wno-unused-variable", "-Wno-attributes", os.path.join(HERE, "host_devlib", "host_utf8_case.cc"), "-o", out])
    lib = C.CDLL(out)
    lib.host_utf8_case.restype = C.c_long
    lib.host_utf8_case_lookup.restype = C.c_uint
    lib.host_utf8_case_table_bytes.restype = C.c_long
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def run_host(lib, upper, off, data, valid=None, text_map=0, inbuf=1):
    """-> (offsets, data, error bits per row); asserts that every row wrote exactly its reported length"""
    n = len(off) - 1
    off = np.ascontiguousarray(off, dtype=np.int32)
    padded = np.zeros(len(data) + 16, dtype=np.uint8)
    padded[:len(data)] = data
    padded[len(data):] = 0xC3  # (what lies behind the column must not matter)
    valid = np.ones(n, dtype=np.uint8) if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    out_off = np.zeros(n + 1, dtype=np.int32)
    out = np.zeros(len(data) * 3 // 2 + 64, dtype=np.uint8)  # (a character grows by half at the most: 2 -> 3 bytes)
    err = np.zeros(n, dtype=np.uint8)
    wrote = np.zeros(n, dtype=np.uint8)
    total = lib.host_utf8_case(1 if upper else 2, _p(off), _p(padded), C.c_long(len(data)), _p(valid), C.c_long(n), text_map, inbuf,
                               _p(out_off), _p(out), _p(err), _p(wrote))
    assert total == out_off[-1] <= len(out)
    assert wrote.all(), "rows whose written bytes are not [0, reported length): %s" % np.flatnonzero(wrote == 0)[:8]
    return out_off, out[:total], err


def rows_to_buffers(rows):
    """rows: bytes or None -> (offsets, data, valid)"""
    off = np.zeros(len(rows) + 1, dtype=np.int32)
    np.cumsum([0 if r is None else len(r) for r in rows], out=off[1:])
    data = np.frombuffer(b"".join(r or b"" for r in rows), dtype=np.uint8)
    return off, data, np.array([r is not None for r in rows], dtype=np.uint8)


@pytest.fixture(scope="module")
def code_points():
    return all_code_points()


@pytest.mark.parametrize("upper", [True, False], ids=["upper", "lower"])
def test_every_code_point_one_per_row_and_sixteen_per_row(caselib, code_points, upper):
    off, data = code_points
    want_off, want_data = array_buffers(arrow_case(upper)(string_array(off, data)))
    for inbuf in (1, 0):
        got_off, got_data, err = run_host(caselib, upper, off, data, inbuf=inbuf)
        assert not err.any()
        assert np.array_equal(got_off, want_off) and np.array_equal(got_data, want_data), inbuf
    # rows of 16 consecutive code points (of the column's order: the surrogates are skipped)
    off16 = np.ascontiguousarray(np.append(off[:-1:16], off[-1]))
    want_off, want_data = array_buffers(arrow_case(upper)(string_array(off16, data)))
    for inbuf in (1, 0):
        got_off, got_data, err = run_host(caselib, upper, off16, data, inbuf=inbuf)
        assert not err.any()
        assert np.array_equal(got_off, want_off) and np.array_equal(got_data, want_data), inbuf
    # the lookup alone
    arrow = arrow_case(upper)
    for ch in "ßıſɐİȺ\u212a\u2126ẞ\U00010428\U00010400\U0001e922\U0001e900éЯz":
        assert chr(caselib.host_utf8_case_lookup(1 if upper else 2, ord(ch))) == arrow(pa.scalar(ch)).as_py()
    assert caselib.host_utf8_case_table_bytes(1 if upper else 2) <= 16384


@pytest.mark.parametrize("upper", [True, False], ids=["upper", "lower"])
def test_random_and_forced_rows(caselib, upper):
    rng = np.random.default_rng(41)
    rows = random_rows(rng, 20000) + forced_rows()
    assert {len(r.encode()) for r in forced_rows()} == set(FORCED_LENGTHS)
    assert max(len(r.encode()) for r in rows) <= 40 and min(len(r) for r in rows) == 0
    arr = pa.array(rows, STR)
    off, data = array_buffers(arr)
    want_off, want_data = array_buffers(arrow_case(upper)(arr))
    for inbuf in (1, 0):
        got_off, got_data, err = run_host(caselib, upper, off, data, inbuf=inbuf)
        assert not err.any()
        assert np.array_equal(got_off, want_off) and np.array_equal(got_data, want_data), inbuf


@pytest.mark.parametrize("upper", [True, False], ids=["upper", "lower"])
@pytest.mark.parametrize("text_map", [1, 2])
def test_views_that_carry_an_ascii_case_map(caselib, upper, text_map):
    """the text is read through gdv_map_byte: ASCII letters first take the view's map, then the whole map applies"""
    rng = np.random.default_rng(42)
    arr = pa.array(random_rows(rng, 5000) + forced_rows(), STR)
    off, data = array_buffers(arr)
    through = (pc.ascii_upper if text_map == 1 else pc.ascii_lower)(arr)
    want_off, want_data = array_buffers(arrow_case(upper)(through))
    for inbuf in (1, 0):
        got_off, got_data, err = run_host(caselib, upper, off, data, text_map=text_map, inbuf=inbuf)
        assert not err.any()
        assert np.array_equal(got_off, want_off) and np.array_equal(got_data, want_data), inbuf


BAD = [b"a\x80", b"\xc3", b"\xe2\x82", b"\xf8\x88\x80\x80\x80"]


@pytest.mark.parametrize("upper", [True, False], ids=["upper", "lower"])
def test_rows_that_are_not_utf8_raise_wherever_they_stand_and_null_rows_never(caselib, upper):
    good = [b"plain", "héllo wörld".encode(), b"", "ɐı".encode()]
    for bad in BAD:
        for at in range(5):
            rows = good[:at] + [bad] + good[at:]
            off, data, valid = rows_to_buffers(rows)
            for inbuf in (1, 0):
                _, _, err = run_host(caselib, upper, off, data, valid, inbuf=inbuf)
                assert [bool(e) for e in err] == [k == at for k in range(len(rows))], (bad, at, inbuf)
                assert err[at] == 4, "GDV_ERR_BAD_ARG"
                # the same bytes in a null row: nothing raises, nothing is written for it
                valid2 = valid.copy()
                valid2[at] = 0
                got_off, _, err = run_host(caselib, upper, off, data, valid2, inbuf=inbuf)
                assert not err.any() and got_off[at] == got_off[at + 1]
        # the bad bytes inside a longer row, at its start, middle and end (for a cut character only the end is bad UTF-8 by
        # construction elsewhere, so a continuation-less follower is put behind it)
        for row in (bad + b"tail of the row", b"abcdefg" + bad + b"xyz", b"0123456789abcde" + bad):
            off, data, valid = rows_to_buffers([row])
            for inbuf in (1, 0):
                _, _, err = run_host(caselib, upper, off, data, valid, inbuf=inbuf)
                assert err[0] == 4, (row, inbuf)


@pytest.mark.parametrize("upper", [True, False], ids=["upper", "lower"])
def test_sequences_that_are_not_unicode_are_copied(caselib, upper):
    """decided (PARITY.md): over-long forms, surrogates and code points above U+10FFFF pass the structural rule and are copied
    unchanged, the characters around them are mapped"""
    odd = [b"\xc0\xaf", b"\xed\xa0\x80", b"\xc1\xa1", b"\xe0\x83\x9f", b"\xf0\x80\x83\x9f", b"\xf4\x90\x80\x80"]
    rows = odd + [b"aB" + o + "éÉzZ".encode() for o in odd] + [b"0123456" + o + b"x" for o in odd]
    off, data, valid = rows_to_buffers(rows)
    case = (lambda t: pc.utf8_upper(pa.scalar(t)).as_py()) if upper else (lambda t: pc.utf8_lower(pa.scalar(t)).as_py())
    want = odd + [case("aB").encode() + o + case("éÉzZ").encode() for o in odd] + [b"0123456" + o + case("x").encode() for o in odd]
    for inbuf in (1, 0):
        got_off, got_data, err = run_host(caselib, upper, off, data, valid, inbuf=inbuf)
        assert not err.any()
        got = [got_data[got_off[i]:got_off[i + 1]].tobytes() for i in range(len(rows))]
        assert got == want, inbuf


# ------------------------------------------------------------------ 3. under sanitizers, as a child process

@pytest.mark.parametrize("name,extra", [("plain", []), ("asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"])])
def test_walker_lookup_and_copy_stay_inside_their_buffers(tmp_path, name, extra):
    exe = str(tmp_path / ("utf8_case_check_" + name))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-unused-function", "-Wno-unused-variable", "-Wno-attributes"] +
                          extra + ["-I", CSRC, os.path.join(HERE, "cxx", "utf8_case_check.cc"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, f"exit {run.returncode}\n{run.stdout}\n{run.stderr}"
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    assert "utf8_case_check: ok" in run.stdout


# ------------------------------------------------------------------ 4. the planner

SCH = pa.schema([pa.field("s", STR), pa.field("t", STR)])
# upper(s) over a one-column schema with the option unset, generated by the PARENT commit's library
PARENT_UPPER_KERNELS = ["gdv_k_7ec152d40da66f68", "gdv_k_fdf7a97884a984bb"]


def _trees():
    b = gandiva.TreeExprBuilder()
    s, t = b.make_field(SCH.field(0)), b.make_field(SCH.field(1))
    fn, lit = b.make_function, b.make_literal
    up, lo = (lambda x: fn("upper", [x], STR)), (lambda x: fn("lower", [x], STR))
    out = lambda node, typ=STR: b.make_expression(node, pa.field("o", typ))
    return {
        "upper": out(up(s)), "lower": out(lo(s)),
        "concat": out(fn("concat", [up(s), lit("-", STR), lo(s)], STR)),
        "upper_substr": out(up(fn("substr", [s, lit(2, pa.int64()), lit(5, pa.int64())], STR))),
        "like_upper": out(fn("like", [up(s), lit("%É%", STR)], pa.bool_()), pa.bool_()),
        "equal_lower": out(fn("equal", [lo(s), lo(t)], pa.bool_()), pa.bool_()),
        "upper_lower": out(up(lo(s))),
        "plain": [out(fn("like", [s, lit("%spark%", STR)], pa.bool_()), pa.bool_()),
                  out(fn("substr", [s, lit(2, pa.int64()), lit(5, pa.int64())], STR)),
                  out(fn("translate", [s, lit("abc", STR), lit("xyz", STR)], STR))],
    }


def _sources(monkeypatch, tmp_path, exprs, schema=SCH):
    from test_planner_cpu import _precompile
    tmp_path.mkdir(parents=True, exist_ok=True)
    files = _precompile(monkeypatch, tmp_path, schema, exprs=exprs if isinstance(exprs, list) else [exprs])
    return {f[:-4]: open(tmp_path / f).read() for f in files}


def _body(text):
    return text.split('#include "gdv_device_lib.hpp"')[-1]


@pytest.mark.parametrize("which", ["upper", "lower", "concat", "upper_substr"])
def test_plans_with_the_option_cross_compile_and_carry_its_tag(monkeypatch, tmp_path, which):
    monkeypatch.setenv("GDV_UTF8_CASE", "1")
    src = _sources(monkeypatch, tmp_path, _trees()[which])   # (_precompile compiles every kernel of the plan for gfx950)
    assert src
    for name, text in src.items():
        assert re.fullmatch(r"gdv_k_[0-9a-f]{16}uc", name), name
        assert name in text and "gdv_utf8_case(ctx, " in text
        assert "upper_utf8(" not in _body(text) and "lower_utf8(" not in _body(text)
        # the row function runs only on live rows whose text is valid; the copies dispatch on the value's kind
        assert re.search(r"\(live && \w+\) \? gdv_utf8_case\(", text) or re.search(r"live \? gdv_utf8_case\(", text)
        assert "GDV_COPY_UTF8CASE(dst, v, " in text


@pytest.mark.parametrize("which,stage_one", [("like_upper", 1), ("equal_lower", 2), ("upper_lower", 1)])
def test_consumers_of_the_value_run_as_staged_plans(monkeypatch, tmp_path, which, stage_one):
    monkeypatch.setenv("GDV_UTF8_CASE", "1")
    src = _sources(monkeypatch, tmp_path, _trees()[which])
    first = {n: t for n, t in src.items() if "__gdv_stage" not in t}
    second = {n: t for n, t in src.items() if "__gdv_stage0" in t}
    assert first and second
    assert all(n.endswith("uc") and "gdv_utf8_case(ctx, " in t for n, t in first.items())
    assert any("__gdv_stage%d" % (stage_one - 1) in t for t in second.values())
    if which != "upper_lower":   # the consumer reads a plain column: no value of the option's kind in it
        assert all(not n.endswith("uc") and "gdv_utf8_case" not in _body(t) for n, t in second.items())


def test_without_the_option_sources_and_names_are_the_parents(monkeypatch, tmp_path):
    from test_decimal_tail_cpu import PARENT_KERNELS
    monkeypatch.delenv("GDV_UTF8_CASE", raising=False)
    c5 = _sources(monkeypatch, tmp_path / "c5", W.c5_expressions(), W.c5_schema())
    assert sorted(c5) == PARENT_KERNELS["c5"]
    one = pa.schema([pa.field("s", STR)])
    b = gandiva.TreeExprBuilder()
    e = b.make_expression(b.make_function("upper", [b.make_field(one.field(0))], STR), pa.field("o", STR))
    up = _sources(monkeypatch, tmp_path / "upper", e, one)
    assert sorted(up) == PARENT_UPPER_KERNELS
    assert all("gdv_utf8_case" not in _body(t) and "upper_utf8(" in t for t in up.values())
    # GDV_UTF8_CASE=0 is the option unset
    monkeypatch.setenv("GDV_UTF8_CASE", "0")
    assert sorted(_sources(monkeypatch, tmp_path / "zero", e, one)) == PARENT_UPPER_KERNELS


def test_a_plan_without_upper_or_lower_is_the_same_with_and_without_the_option(monkeypatch, tmp_path):
    monkeypatch.delenv("GDV_UTF8_CASE", raising=False)
    without = _sources(monkeypatch, tmp_path / "off", _trees()["plain"])
    monkeypatch.setenv("GDV_UTF8_CASE", "1")
    with_it = _sources(monkeypatch, tmp_path / "on", _trees()["plain"])
    assert without == with_it and without


# ------------------------------------------------------------------ 5. the C++ API

def test_cxx_case_builds_its_trees_host_only():
    """gandiva_amd/cxx/tests/test_utf8_case_cxx.cc sets the variable before Projector::Make; here: it builds, the trees build"""
    cxx = os.path.join(HERE, "..", "gandiva_amd", "cxx")
    subprocess.check_call(["make", "-C", cxx, "all", "test_cxx"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(cxx, "tests", "test_utf8_case_cxx"), "--host-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "OK (host-only)" in out.stdout, out.stdout + out.stderr
