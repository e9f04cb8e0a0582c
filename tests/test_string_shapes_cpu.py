"""The core string functions on rows that cross every kernel boundary, without a GPU: the corpus of
tests/string_shapes.py checked for the boundaries it claims, its reference against pyarrow.compute and Python's str,
the oracle and the host build of the device library against the reference, the corpus's ladders against the thresholds
of the kernels the planner generates for the groups of the GPU test (tests/test_string_shapes.py), the kernel shape of
each group, and the partition of the registry's text signatures into "covered here" and a named exclusion list."""
import ctypes as C
import os
import re

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import gandiva_amd as gandiva
from gandiva_amd import _capi, gandiva as gg
from oracle import oracle
import string_shapes as R
from helpers import assert_bit_exact, py_murmur3_x86_32
from test_device_lib_on_host import hostlib, _lit, _p  # noqa: F401  (the fixture that builds tests/host_devlib)

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gandiva_amd", "csrc", "gdv_device_lib.hpp")


# ---- the corpus stands where it says it stands ---------------------------------------------------------------------------
def _offsets(arr):
    return np.frombuffer(arr.buffers()[1], dtype=np.int32)[arr.offset: arr.offset + len(arr) + 1].astype(np.int64)


def _unit_totals(off, runs, prefix, unit):
    """Byte totals of every `unit`-aligned group of rows inside the runs whose name starts with `prefix`."""
    out = set()
    for name, spans in runs.items():
        if name.startswith(prefix):
            for first, rows in spans:
                out |= {int(off[r + unit] - off[r]) for r in range(first, first + rows - unit + 1, unit) if r % unit == 0}
    return out


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_corpus_holds_the_length_and_span_ladders(variant):
    rows, forced, anchor, runs = R.corpus(variant)
    for nulls in R.NULLS:
        b = R.batch(variant, nulls)
        b.validate(full=True)
        assert b.schema == R.SCHEMA and b.num_rows == len(rows) and b.nbytes < 2 << 20
        off = _offsets(b.column("s"))
        lengths = set(np.diff(off).tolist())
        assert set(R.LENGTH_LADDER) <= lengths and max(lengths) > 65536
        assert b.column("s").buffers()[2].size == off[-1], "the data buffer ends at the last row's last byte"
        assert all(first % R.SUB == 0 for spans in runs.values() for first, _ in spans), "a run is a sub-tile"
        # every (T, unit): a unit-aligned group of T - 1, T and T + 1 bytes, from equal rows and from one long row
        for t, unit in R.SPAN_LADDERS:
            for kind in ("equal_", "long_"):
                assert {t - 1, t, t + 1} <= _unit_totals(off, runs, kind, unit), (t, unit, kind, nulls)
        share = b.column("s").null_count / len(rows)
        assert (share < 0.05 if nulls == 0 else 0.05 < share < 0.16) and b.column("s").null_count >= len(forced)
    # ... and of the OUTPUTS that grow or shrink the text: 2048 / 4096 +- 1 bytes per tile of 4 / 8 sub-tiles
    if variant == "ascii":
        specs = [{"tree": t, "ret": "str"} for t in (
            R.F("concat", "str", "s", "t"), R.F("lpad", "str", "s", "k"), R.F("rpad", "str", "s", "k", "t"),
            R.F("replace", "str", "s", R.L("k"), R.L("kkkkk")), R.F("substr", "str", "s", R.I64(9)), R.F("right", "str", "s", R.I32(8)))]
        for sp, e in zip(specs, R.expected_of(specs, R.columns(variant, 0.0))):
            kind = "out_shrink" if sp["tree"]["fn"] in ("substr", "right") else "out_grow"
            for t, unit in ((2048, 256), (4096, 512)):
                want = {t - 1, t, t + 1} if sp["tree"]["fn"] != "right" else {t}
                assert want <= _unit_totals(_offsets(e), runs, kind, unit), (sp["tree"]["fn"], t)
        covered = {R._label(t) for _, _, trees in R.groups().values() for t in trees}
        assert {R._label(sp["tree"]) for sp in specs} <= covered, "an output-total expression is in no group"


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_corpus_places_every_needle_on_every_boundary(variant):
    rows, forced, _, runs = R.corpus(variant)
    b = R.batch(variant, 0.0)
    off = _offsets(b.column("s"))
    data = b.column("s").buffers()[2].to_pybytes()
    for needle in R.NEEDLES[1:]:
        nb, n = needle.encode(), len(needle)
        first, cnt = runs["placed_" + needle][0]
        assert off[first] % 1024 == 0 and cnt == 2 * R.SUB
        seen = set()
        for sub in (first, first + R.SUB):
            base, end = int(off[sub]), int(off[sub + R.SUB])
            assert end - base == 2048
            starts = [m.start() for m in re.finditer(re.escape(nb), data[base:end])]
            row_starts, row_ends = set((off[sub:sub + R.SUB] - base).tolist()), set((off[sub + 1:sub + R.SUB + 1] - base).tolist())
            for p in starts:
                seen |= {("ends at", u) for u in (16, 1024) if (p + n) % u == 0} | {("starts at", u) for u in (16, 1024) if p % u == 0}
                seen |= {("straddles", u) for u in (16, 1024) if p // u != (p + n - 1) // u and p % u}
                seen |= {("first in row",)} if p in row_starts else set()
                seen |= {("last in row",)} if p + n in row_ends else set()
                seen |= {("last in span",)} if p + n == 2048 else set()
        want = {(w, u) for w in ("ends at", "starts at", "straddles") for u in (16, 1024)} | {("first in row",), ("last in row",), ("last in span",)}
        assert want <= seen, (needle, want - seen)
    assert data.startswith(b"sparkling") and data.endswith(b"spark"), "a needle as the first and as the last bytes of the data buffer"
    # split needles: the two halves end one row and start the next, across a sub-tile, both wave tiles and a NULL row
    first, cnt = runs["split"][0]
    assert first % R.TILE == 0
    split_at = set()
    for needle in R.NEEDLES[1:]:
        h = len(needle) // 2
        for r in range(first, first + cnt - 1):
            if rows[r].endswith(needle[:h]) and rows[r + 1].startswith(needle[h:]) and needle not in rows[r] and needle not in rows[r + 1]:
                split_at.add((r + 1) % R.TILE)
    assert {0, 256, 64, 192} <= split_at and any(r % 64 for r in split_at), split_at
    nul = [r for r in forced if first <= r < first + cnt]
    assert len(nul) == 1 and rows[nul[0] - 1].endswith("spar") and rows[nul[0] + 1].startswith("k")
    # degenerate runs
    (e0, ec), (n0, nc) = runs["empty_tile"][0], runs["null_tile"][0]
    assert e0 % R.TILE == 0 and ec == R.TILE and set(rows[e0:e0 + ec]) == {""} and set(range(n0, n0 + nc)) <= forced and n0 % R.TILE == 0
    a0, _ = runs["alternating"][0]
    assert all((rows[a0 + i] == "") == (i % 2 == 0) for i in range(128))
    l0, lc = runs["long_then_short"][0]
    assert len(rows[l0].encode()) > 65536 and lc == R.TILE + 1 and all(len(r) == 1 for r in rows[l0 + 1:l0 + lc])
    s0, sc = runs["spaces"][0]
    assert {len(r) for r in rows[s0:s0 + sc] if r.strip(" ") == ""} >= {7, 8, 9, 15, 16, 17}
    if variant == "multibyte":
        # characters of 2, 3 and 4 bytes that straddle a multiple of 16 and of 1024 of their sub-tile's span
        widths = {16: set(), 1024: set()}
        text_of = b.column("s").to_pylist()
        for sub in range(0, len(rows) - R.SUB, R.SUB):
            at = 0
            for r in range(sub, sub + R.SUB):
                for ch in text_of[r] or "":
                    w = len(ch.encode())
                    if w > 1:
                        for u in (16, 1024):
                            if at // u != (at + w - 1) // u:
                                widths[u].add(w)
                    at += w
        assert widths[16] == {2, 3, 4} and widths[1024] == {2, 3, 4}, widths


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_layouts_are_what_they_are_named(layout):
    for variant in R.VARIANTS:
        b = R.layout_batch(layout, variant)
        b.validate(full=True)
        s = b.column("s")
        off, data = _offsets(s), s.buffers()[2].to_pybytes()
        want_s, _, want_b, _, rows = R.layout_columns(layout, variant)
        assert s.to_pylist() == want_s and b.column("b").to_pylist() == want_b
        if layout == "sliced":
            assert off[0] == 7 and data[:7] == b"SPA spa" and data[off[-1]:].startswith(b"k sparkling") and rows[0].startswith("k")
        if layout == "exact_end":
            assert len(data) == off[-1] and np.diff(off)[-9:].tolist() == [9, 8, 7, 6, 5, 4, 3, 2, 1]
        if layout == "null_bytes":
            nul = np.flatnonzero(~np.asarray(s.is_valid()))
            assert len(nul) > 5 and (np.diff(off)[nul] > 0).any(), "NULL rows that carry bytes"


# ---- the reference against second engines ------------------------------------------------------------------------------
def test_murmur3_x86_32_matches_sklearn():
    from sklearn.utils import murmurhash3_32
    for d in (b"", b"a", b"ab", b"abc", b"abcd", b"hello world!!", "日本語テキスト".encode(), b"x" * 300):
        for seed in (0, 17, -5, 1 << 31):
            assert py_murmur3_x86_32(d, seed) == murmurhash3_32(d, seed=seed & 0xffffffff, positive=False)


def _reference(tree, variant, nulls, ret):
    return R.expected_of([{"tree": tree, "ret": ret}], R.columns(variant, nulls))[0]


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_reference_matches_arrow_compute_and_python_str(variant):
    nulls = 0.1
    b = R.batch(variant, nulls)
    s, t, raw = b.column("s"), b.column("t"), b.column("b")
    F, L, I32, I64 = R.F, R.L, R.I32, R.I64
    pins = [(F("like", "bool", "s", L(p)), pc.match_like(s, p)) for p in ("%spark%", "spark%", "%sparkles", "s_ark%", "%a%b%", "_%_", "%sp%", "%")]
    pins += [(F("like", "bool", "s", L("100#%%"), L("#")), pc.match_like(s, "100\\%%")),
             (F("ilike", "bool", "s", L("%SpArK%")), pc.match_like(s, "%spark%", ignore_case=True) if variant == "ascii" else None),
             (F("regexp_like", "bool", "s", L(R.REGEX)), pc.match_substring_regex(s, R.REGEX))]
    for a, c in ((1, 1), (2, 8), (8, 9), (9, 16), (16, 17), (17, 2)):
        pins.append((F("substr", "str", "s", I64(a), I64(c)), pc.utf8_slice_codeunits(s, a - 1, a - 1 + c)))
    pins += [(F("substr", "str", "s", I64(9)), pc.utf8_slice_codeunits(s, 8)), (F("substr", "str", "s", I64(2)), pc.utf8_slice_codeunits(s, 1))]
    pins += [(F("left", "str", "s", I32(k)), pc.utf8_slice_codeunits(s, 0, k)) for k in (1, 8, 9, 16, 17)]
    pins += [(F("left", "str", "s", I32(-8)), pc.utf8_slice_codeunits(s, 0, -8)), (F("castVARCHAR", "str", "s", I64(9)), pc.utf8_slice_codeunits(s, 0, 9))]
    pins += [(F("upper", "str", "s"), pc.ascii_upper(s)), (F("lower", "str", "s"), pc.ascii_lower(s)), (F("reverse", "str", "s"), pc.utf8_reverse(s)),
             (F("char_length", "i32", "s"), pc.utf8_length(s)), (F("length", "i32", "s"), pc.utf8_length(s)),
             (F("octet_length", "i32", "s"), pc.binary_length(s)), (F("octet_length", "i32", "b"), pc.binary_length(raw)),
             (F("bit_length", "i32", "b"), pc.multiply(pc.binary_length(raw), 8)),
             (F("ltrim", "str", "s"), pc.utf8_ltrim(s, " ")), (F("rtrim", "str", "s"), pc.utf8_rtrim(s, " ")),
             (F("btrim", "str", "s"), pc.utf8_trim(s, " ")), (F("trim", "str", "s"), pc.utf8_trim(s, " "))]
    for needle in R.NEEDLES:
        pins.append((F("replace", "str", "s", L(needle), L("flink")), pc.replace_substring(s, needle, "flink")))
        pins.append((F("starts_with", "bool", "s", L(needle)), pc.starts_with(s, needle)))
        pins.append((F("ends_with", "bool", "s", L(needle)), pc.ends_with(s, needle)))
        if variant == "ascii":   # find_substring counts bytes, locate characters: the same number on ASCII text, 0 on an empty row
            found = pc.add(pc.find_substring(s, needle), 1).cast(pa.int32())
            pins.append((F("locate", "i32", L(needle), "s"), found))
            pins.append((F("strpos", "i32", "s", L(needle)), found))
    ops = {"equal": pc.equal, "not_equal": pc.not_equal, "less_than": pc.less, "less_than_or_equal_to": pc.less_equal,
           "greater_than": pc.greater, "greater_than_or_equal_to": pc.greater_equal}
    for name, op in ops.items():
        pins += [(F(name, "bool", "s", L("spark")), op(s.cast(pa.binary()), pa.scalar(b"spark"))), (F(name, "bool", "s", "t"), op(s.cast(pa.binary()), t.cast(pa.binary()))),
                 (F(name, "bool", "b", L("sparkles", "bin")), op(raw, pa.scalar(b"sparkles")))]
    pins += [(F("concatOperator", "str", "s", "t"), pc.binary_join_element_wise(s, t, "")),
             (F("concatOperator", "str", "t", L("|"), "s"), pc.binary_join_element_wise(t, s, "|")),
             (F("concat", "str", "s", "t"), pc.binary_join_element_wise(s, t, "", null_handling="replace", null_replacement="")),
             (F("isnull", "bool", "s"), pc.is_null(s)), (F("isnotnull", "bool", "b"), pc.is_valid(raw)),
             ({"in": "s", "values": ["spark", "k", ""]}, pc.if_else(pc.is_null(s), pa.scalar(None, pa.bool_()), pc.is_in(s, value_set=pa.array(["spark", "k", ""]))))]
    compared = 0
    for tree, want in pins:
        if want is None:
            continue
        got = _reference(tree, variant, nulls, R._ret(tree))
        assert got.equals(want.cast(got.type)), R._label(tree)
        compared += 1
    assert compared >= (76 if variant == "ascii" else 65)
    # Python's str for what Arrow has no kernel of: right(), negative starts, the pads with a one-character fill
    vals = s.to_pylist()
    assert _reference(F("right", "str", "s", I32(9)), variant, nulls, "str").to_pylist() == [None if v is None else v[-9:] for v in vals]
    assert _reference(F("substr", "str", "s", I64(-8), I64(8)), variant, nulls, "str").to_pylist() == [None if v is None else (v[-8:] if len(v) >= 8 else "") for v in vals]
    keep = pc.and_(pc.greater(pc.utf8_length(s), 0), pc.less_equal(pc.utf8_length(s), 17))
    for fn, arrow in (("lpad", pc.utf8_lpad), ("rpad", pc.utf8_rpad)):
        got = _reference(F(fn, "str", "s", I32(17), L("*")), variant, nulls, "str")
        assert got.filter(keep).equals(arrow(s, width=17, padding="*").filter(keep)), fn


# ---- the oracle against the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nulls", R.NULLS)
@pytest.mark.parametrize("variant", R.VARIANTS)
def test_oracle_matches_the_reference_on_every_row(variant, nulls):
    batch = R.batch(variant, nulls)
    pairs = expressions = 0
    for group in R.groups():
        specs = R.group_specs(group)
        got = oracle.project(R.build_expressions(gandiva, specs), batch)
        for sp, g, want in zip(specs, got, R.expected_columns(group, variant, nulls)):
            assert_bit_exact(g, want, "oracle %s %s nulls=%s" % (sp["label"], variant, nulls))
            pairs += len(g)
        expressions += len(specs)
    assert expressions == sum(len(t) for _, _, t in R.groups().values()) > 150 and pairs == expressions * batch.num_rows


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_oracle_matches_the_reference_on_the_layouts(layout):
    for variant in R.VARIANTS:
        batch = R.layout_batch(layout, variant)
        for group in R.groups():
            specs = R.group_specs(group)
            for sp, g, want in zip(specs, oracle.project(R.build_expressions(gandiva, specs), batch), R.expected_layout_columns(group, layout, variant)):
                assert_bit_exact(g, want, "oracle %s %s %s" % (sp["label"], layout, variant))


# ---- the host build of the device library against the reference -----------------------------------------------------------
def _raw_col(vals, pad=16):
    raw = [b"" if v is None else (v if isinstance(v, bytes) else v.encode()) for v in vals]
    off = np.zeros(len(raw) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(r) for r in raw])
    return off, np.frombuffer(b"".join(raw) + b"\0" * pad, dtype=np.uint8).copy(), int(off[-1])


def _simple_like(pat):
    """(host_str_pred_lit's function, needle) of a pattern that is a needle with a % at either end at most."""
    core = pat.strip("%")
    if "%" in core or "_" in core or pat in ("%", "%%"):
        return None
    fn = {(True, True): 0, (False, True): 1, (True, False): 2, (False, False): 3}[(pat.startswith("%") and len(pat) > 0, pat.endswith("%") and len(pat) > 1)]
    return fn, core


def _host_value(lib, tree, cols, variant):
    """The tree's value per row through the device library's own functions compiled for the host (a list of Python values
    over the rows' bytes, NULL rows as empty), or None where tests/host_devlib exposes no entry point for it."""
    if isinstance(tree, dict) and tree.get("in") == "s":      # IN over the literal list laid out as the planner lays it out
        raw = [v.encode() for v in tree["values"]]
        loffs = np.zeros(len(raw) + 1, dtype=np.int32)
        loffs[1:] = np.cumsum([len(r) for r in raw])
        lbytes = np.frombuffer(b"".join(raw) + b"\0" * 8, dtype=np.uint8).copy()
        off, data, size = _raw_col(cols[0])
        out = np.zeros(len(cols[0]), dtype=np.uint8)
        lib.host_str_in(_p(off), _p(data), C.c_long(size), C.c_long(len(out)), _p(lbytes), _p(loffs), len(raw), _p(out))
        return out.astype(bool).tolist()
    if not isinstance(tree, dict) or "fn" not in tree:
        return None
    fn, args = tree["fn"], tree["args"]
    mp = 0
    if fn in ("upper", "lower") and isinstance(args[0], dict) and args[0].get("fn") in ("substr", "left"):
        mp, tree = (1 if fn == "upper" else 2), args[0]
        fn, args = tree["fn"], tree["args"]
    if args[0] not in ("s", "b") and not (fn in ("locate", "position") and args[1] == "s"):
        return None
    s, t, _, k = cols
    n = len(s)
    off, data, size = _raw_col(s)
    base = (_p(off), _p(data), C.c_long(size), C.c_long(n))
    lits = [a["lit"] for a in args[1:] if isinstance(a, dict) and "lit" in a]
    all_lit = len(lits) == len(args) - 1
    as_bytes = lambda v: v if isinstance(v, bytes) else v.encode()  # noqa: E731

    def pred(code, needle, m=0):
        lb, ll = np.frombuffer(as_bytes(needle) + b"\0" * 8, np.uint8).copy(), len(as_bytes(needle))
        out = np.zeros(n, dtype=np.uint8)
        lib.host_str_pred_lit(code, *base, _p(lb), ll, m, _p(out))
        return out.astype(bool).tolist()

    def ints(entry, code, needle=b"", kk=0, m=0):
        lb, ll = np.frombuffer(as_bytes(needle) + b"\0" * 8, np.uint8).copy(), len(as_bytes(needle))
        out = np.zeros(n, dtype=np.int64)
        if entry == "k":
            lib.host_str_int_k(code, *base, _p(lb), ll, C.c_longlong(kk), _p(out))
        else:
            lib.host_str_int(code, *base, _p(lb), ll, m, _p(out))
        return out.tolist()

    def strings(out_off, out_data):
        return [bytes(out_data[out_off[i]:out_off[i + 1]]).decode() for i in range(n)]

    def view(code, a=0, c=0):
        out_off, out_data = np.zeros(n + 1, np.int32), np.zeros(size + 64, np.uint8)
        lib.host_str_view(code, *base, C.c_longlong(a), C.c_longlong(c), mp, _p(out_off), _p(out_data))
        return strings(out_off, out_data)

    if fn in ("like", "ilike") and len(args) == 2 and all_lit and _simple_like(lits[0]):
        code, needle = _simple_like(lits[0])
        return pred(code, R.ascii_lower(needle) if fn == "ilike" else needle, 2 if fn == "ilike" else 0)
    if fn in ("like", "ilike") and all_lit:      # the general matcher over a pattern compiled as CompileLike compiles it
        pat, esc = (R.ascii_lower(lits[0]) if fn == "ilike" else lits[0]), (lits[1] if len(lits) == 2 else None)
        pbyte, pkind, i = [], [], 0
        while i < len(pat):
            ch = pat[i]
            if esc and ch == esc and i + 1 < len(pat):
                i += 1
                ch, kind = pat[i], 0
            else:
                kind = 2 if ch == "%" else 1 if ch == "_" else 0
            for byte in ch.encode():
                pbyte.append(byte)
                pkind.append(kind)
            i += 1
        pb, pk = np.array(pbyte + [0] * 8, np.uint8), np.array(pkind + [0] * 8, np.uint8)
        out = np.zeros(n, dtype=np.uint8)
        lib.host_str_like(*base, _p(pb), _p(pk), len(pbyte), 2 if fn == "ilike" else 0, _p(out))
        return out.astype(bool).tolist()
    compares = {"equal": ("p", 4), "less_than": ("p", 5), "greater_than_or_equal_to": ("p", 8), "starts_with": ("p", 6), "ends_with": ("p", 7),
                "not_equal": ("k", 5), "less_than_or_equal_to": ("k", 6), "greater_than": ("k", 7)}
    if fn in compares and all_lit:
        entry, code = compares[fn]
        return pred(code, lits[0]) if entry == "p" else [bool(v) for v in ints("k", code, lits[0])]
    if fn in ("equal", "less_than", "starts_with", "ends_with") and args[1] == "t":
        offt, datat, sizet = _raw_col(t)
        out = np.zeros(n, dtype=np.uint8)
        lib.host_str_pred_col(["equal", "less_than", "starts_with", "ends_with"].index(fn), *base[:3], _p(offt), _p(datat), C.c_long(sizet), C.c_long(n), _p(out))
        return out.astype(bool).tolist()
    if fn in ("octet_length", "char_length", "length", "lengthUtf8", "ascii") and len(args) == 1:
        return ints("m", {"octet_length": 0, "ascii": 4}.get(fn, 1))
    if fn == "bit_length":
        return ints("k", 0)
    if fn in ("hash", "hash32", "hash32AsDouble"):
        return ints("m", 2) if len(args) == 1 else ints("k", 3, kk=lits[0])
    if fn in ("hash64", "hash64AsDouble"):
        return ints("m", 3) if len(args) == 1 else ints("k", 4, kk=lits[0])
    if fn in ("locate", "position") and isinstance(args[0], dict) and "lit" in args[0] and args[1] == "s":
        return ints("m", 5, args[0]["lit"]) if len(args) == 2 else ints("k", 1, args[0]["lit"], args[2]["lit"])
    if fn == "strpos" and all_lit:
        return ints("k", 2, lits[0])
    views = {"substr": 1, "substring": 1, "ltrim": 2, "rtrim": 3, "btrim": 4, "trim": 4, "left": 5, "right": 6, "castVARCHAR": 7}
    if fn in views and all_lit:
        if fn in ("substr", "substring") and len(lits) == 1:
            return view(8, lits[0])
        return view(views[fn], *lits)
    if fn in ("upper", "lower") and len(args) == 1 and args[0] == "s":
        mp = 1 if fn == "upper" else 2
        return view(0)
    if fn == "reverse":
        out_off, out_data = np.zeros(n + 1, np.int32), np.zeros(size + 64, np.uint8)
        assert lib.host_str_reverse(*base, 0, int(variant == "ascii"), _p(out_off), _p(out_data)) == 0
        return strings(out_off, out_data)
    if fn == "initcap":
        out_off, out_data = np.zeros(n + 1, np.int32), np.zeros(size + 64, np.uint8)
        lib.host_str_initcap(*base, 0, _p(out_off), _p(out_data))
        return strings(out_off, out_data)
    if fn in ("lpad", "rpad") and all_lit:
        want_n, fill = lits[0], (lits[1] if len(lits) == 2 else " ")
        tab = "".join(fill[j % len(fill)] for j in range(max(want_n, 0)))
        tb, tl = _lit(tab)
        out_off, out_data = np.zeros(n + 1, np.int32), np.zeros(size + 4 * max(want_n, 0) * n + 64, np.uint8)
        lib.host_str_pad(int(fn == "rpad"), *base, want_n, _p(tb), tl, int(tab.isascii()), _p(out_off), _p(out_data))
        return strings(out_off, out_data)
    if fn == "replace" and all_lit:
        fb, tb = lits[0].encode(), lits[1].encode()
        table = np.frombuffer(np.array([len(fb), len(tb), 0, 0], np.int32).tobytes() + fb + b"\0" * ((16 - len(fb) % 16) % 16) + tb + b"\0" * 8, np.uint8).copy()
        padded = np.concatenate([data[:size], np.frombuffer((fb * 32)[:32], np.uint8)])      # the needle itself behind the buffer
        results = []
        for entry in ("rows", "rows_inbuf", "hits"):
            if entry == "hits" and not (2 <= len(fb) <= 8):
                continue
            out_off, out_data = np.zeros(n + 1, np.int32), np.zeros(6 * size + 64 * n + 64, np.uint8)
            if entry == "hits":      # the match bitmap built the way the sweep builds it
                err = lib.host_str_replace_hits(_p(off), _p(padded), C.c_long(size), C.c_long(n), 0, _p(table), _p(out_off), _p(out_data))
            else:
                err = lib.host_str_replace(_p(off), _p(padded), C.c_long(size), C.c_long(n), 0, _p(table), _p(out_off), _p(out_data), int(entry == "rows_inbuf"))
            assert err == 0
            results.append(strings(out_off, out_data))
        assert all(r == results[0] for r in results), "the row search and the sweep's match bitmap disagree on replace(%r)" % lits[0]
        return results[0]
    return None


NOT_ON_THE_HOST = []      # labels of the expressions tests/host_devlib has no entry point for (filled by the test below)


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_host_build_of_the_device_library_matches_the_reference(hostlib, variant):  # noqa: F811
    """Every expression that tests/host_devlib exposes, per row through the device library's own function compiled for
    the host, over the whole corpus (no NULLs but the forced ones: a NULL row is computed as an empty one and left out)."""
    cols = R.columns(variant, 0.0)
    valid = np.array([v is not None for v in cols[0]])
    compared, missing = 0, []
    for group in R.groups():
        for sp, want in zip(R.group_specs(group), R.expected_columns(group, variant, 0.0)):
            got = _host_value(hostlib, sp["tree"], cols, variant)
            if got is None:
                missing.append(sp["label"])
                continue
            w = want.to_pylist()
            bad = [i for i in np.flatnonzero(valid).tolist() if got[i] != w[i]]
            assert not bad, "host build %s (%s): %d rows differ, first %d: %r vs %r" % (sp["label"], variant, len(bad), bad[0], got[bad[0]], w[bad[0]])
            compared += 1
    NOT_ON_THE_HOST[:] = missing
    # most per-row operands (t, k), the regular expression, the null tests, concat and if / else are planned by the code
    # generator, not single device functions: they are held by the oracle test above and on the GPU
    assert compared >= 148 and len(missing) <= 31, (compared, missing)


# ---- the kernels the planner generates for the groups of the GPU test -------------------------------------------------------
@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """{group: [text of every kernel of the group's row-mode projector]}, and the same under GDV_NO_WAVE_SHAPE=1."""
    mp = pytest.MonkeyPatch()
    out = {"wave": {}, "scanner": {}}
    try:
        mp.setenv("GDV_NO_DISK_CACHE", "1")
        mp.setenv("GDV_DUMP_SOURCE", "1")
        mp.setenv("GDV_PRECOMPILE_SKIP_GENERAL", "1")      # the main kernel and its pre-pass; the variants are built on demand
        lib = _capi.lib()
        for kind in ("wave", "scanner"):
            if kind == "scanner":
                mp.setenv("GDV_NO_WAVE_SHAPE", "1")
            for group in R.groups():
                d = tmp_path_factory.mktemp("%s_%s" % (kind, group))
                mp.setenv("GANDIVA_AMD_CACHE_DIR", str(d))
                exprs = R.build_expressions(gandiva, R.group_specs(group))
                sh = gg._make_schema(R.SCHEMA)
                try:
                    arr = (C.c_void_p * len(exprs))(*[e._h for e in exprs])
                    assert lib.gdv_precompile_projector(sh, arr, len(exprs), 0) == 0, "%s: %s" % (group, _capi.last_error())
                finally:
                    lib.gdv_schema_free(sh)
                out[kind][group] = [open(os.path.join(d, f)).read() for f in sorted(os.listdir(d)) if f.endswith(".hip")]
    finally:
        mp.undo()
    return out


def _define(text, name, env=None):
    """The value of `#define name expr` in a text; expr may use the names of env."""
    m = re.search(r"^#define %s (.+?)\s*(//.*)?$" % name, text, re.M)
    return None if m is None else int(eval(m.group(1), {"__builtins__": {}}, dict(env or {})))


def test_every_threshold_of_the_generated_kernels_is_a_ladder_of_the_corpus(generated):
    """GDV_U, GDV_SG and GDV_SUB_SPAN from the generated text (the header's default where the text defines none),
    GDV_OUT_WIN and GDV_SPAN_MAX from their definitions in gdv_device_lib.hpp: each (threshold, rows of its unit) must be
    one the corpus holds runs of T - 1, T and T + 1 bytes for.  A change of a tile size fails here."""
    header = open(HEADER).read()
    seen = set()
    for group, texts in generated["wave"].items():
        for text in texts:
            u = _define(text, "GDV_U")
            assert u in (4, 8), (group, u)
            sg = _define(text, "GDV_SG") or 1
            sub_span = _define(text, "GDV_SUB_SPAN") or _define(header, "GDV_SUB_SPAN")
            out_win, span_max = _define(header, "GDV_OUT_WIN", {"GDV_U": u}), _define(header, "GDV_SPAN_MAX", {"GDV_U": u})
            seen |= {(sub_span, 64 * sg), (out_win, 64 * u), (span_max, 64 * u)}
    assert seen <= set(R.SPAN_LADDERS), "no ladder in the corpus for %s" % sorted(seen - set(R.SPAN_LADDERS))
    assert {u for _, u in seen} >= {64, 256, 512}, "the groups no longer cover both tile sizes: %s" % sorted(seen)
    assert {1024, 2048, 4096, 8192, 16384} >= {t for t, _ in seen} and {t for t, _ in seen} <= {t for t in R.LENGTH_LADDER}


def test_each_group_is_planned_on_the_shape_it_is_meant_to_exercise(generated):
    """R.GROUP_SHAPES, the one table of the grouping: every row-mode group on a wave-shaped main kernel and its pre-pass
    (the staged group on two such pairs), with as many outputs in LDS windows as the table says and an exact variant
    where the optimistic kernels assume ASCII; upper(s) / lower(s) alone on the flat store; and every group on the scanner
    shape under GDV_NO_WAVE_SHAPE=1.  A group that the planner moves to another shape fails here."""
    assert set(R.GROUP_SHAPES) == set(R.groups()) and len(R.GROUP_SHAPES) <= 26
    for group, (shape, exact, windows, notflat) in R.GROUP_SHAPES.items():
        assert R.groups()[group][1] == shape
        texts = generated["wave"][group]
        main = [t for t in texts if "// wave shape:" in t]
        pre = [t for t in texts if "// pre-pass:" in t]
        if shape in ("wave", "stages"):
            stages = 2 if shape == "stages" else 1
            assert len(main) == stages and len(pre) == stages and len(texts) == 2 * stages, (group, len(texts))
            assert (stages == 2) == any("__gdv_stage0" in t for t in main), group
            main = [t for t in main if "__gdv_stage0" in t] if stages == 2 else main
            assert "gdv_scanner<GDV_NG>" not in main[0] and "rows = the slots of a selection vector" not in main[0], group
            staged = len(set(re.findall(r"gdv_uint8\* const (win\d+) = lds_out", main[0])))
            assert staged >= windows, "%s: %d outputs staged through LDS windows" % (group, staged)
            assert ("GDV_ERR_NOTASCII" in main[0]) == exact and ("GDV_ERR_NOTFLAT" in main[0]) == notflat, group
        else:      # one flat output: no scan, no pre-pass, the bytes stored by the sweep under the input's offsets
            assert len(main) == 1 and not pre and len(texts) == 1, (group, len(texts))
            assert "gdv_sweep_store" in main[0] and "GDV_ERR_NOTFLAT" in main[0] and notflat and " = lds_out + " not in main[0], group
            assert ("GDV_ERR_NOTASCII" in main[0]) == exact, group
        scanner = generated["scanner"][group]
        assert scanner and all("gdv_scanner<GDV_NG>" in t and "// wave shape:" not in t for t in scanner), group


# ---- every text signature of the registry is tested on shaped rows: here or in a named file ---------------------------------
EXCLUDED = {
    # name (every signature of it with a text parameter or result, unless the families above hold it): where, or why not here
    "hex": "tests/test_encode.py", "to_hex": "tests/test_encode.py", "unhex": "tests/test_encode.py", "from_hex": "tests/test_encode.py",
    "base64": "tests/test_encode.py", "unbase64": "tests/test_encode.py", "crc32": "tests/test_encode.py",
    "mask": "tests/test_mask.py", "mask_first_n": "tests/test_mask.py", "mask_last_n": "tests/test_mask.py",
    "mask_show_first_n": "tests/test_mask.py", "mask_show_last_n": "tests/test_mask.py",
    "split_part": "tests/test_string_tail.py", "substring_index": "tests/test_string_tail.py", "repeat": "tests/test_string_tail.py",
    "space": "tests/test_string_tail.py", "translate": "tests/test_string_tail.py",
    "regexp_extract": "tests/test_regexp_extract.py", "regexp_replace": "tests/test_registry_tail.py (a literal pattern only: planned as replace)",
    "regexp_matches": "tests/test_registry_tail.py (an alias of regexp_like, which is here)",
    "hashMD5": "tests/test_registry_tail.py", "md5": "tests/test_registry_tail.py", "hashSHA1": "tests/test_registry_tail.py", "sha1": "tests/test_registry_tail.py",
    "sha": "tests/test_registry_tail.py", "hashSHA256": "tests/test_registry_tail.py", "sha256": "tests/test_registry_tail.py",
    "castINT": "text of a number's grammar: tests/test_strings.py", "castBIGINT": "text of a number's grammar: tests/test_strings.py",
    "castDECIMAL": "text of a number's grammar: tests/test_decimal_tail.py",
    "castDATE": "text of a date's grammar: tests/test_temporal_text.py", "castTIME": "text of a time's grammar: tests/test_temporal_text.py",
    "castTIMESTAMP": "text of a timestamp's grammar: tests/test_temporal_text.py", "to_date": "text of a date's grammar: tests/test_registry_tail.py",
    "castVARCHAR": "of a value that is not text: tests/test_temporal_text.py, tests/test_registry_tail_r3.py, tests/test_decimal_tail.py",
}
_TYPE_NAMES = {pa.string(): "str", pa.binary(): "bin", pa.int32(): "i32", pa.int64(): "i64", pa.bool_(): "bool"}


def test_every_text_signature_is_in_a_family_or_in_the_named_exclusion_list():
    covered = set()
    for _, _, trees in R.groups().values():
        for t in trees:
            R.signatures_of(t, covered)
    covered_names = {name for name, _ in covered}
    unassigned, both, files = [], [], set()
    for sig in gandiva.get_registered_function_signatures():
        types = list(sig.param_types()) + [sig.return_type()]
        if not any(pa.types.is_string(t) or pa.types.is_binary(t) for t in types):
            continue
        key = (sig.name(), tuple(_TYPE_NAMES.get(t, str(t)) for t in sig.param_types()))
        here = key in covered
        text_cast = sig.name() == "castVARCHAR" and pa.types.is_string(sig.param_types()[0])
        there = sig.name() in EXCLUDED and not text_cast and not (sig.name() in covered_names and sig.name() != "castVARCHAR")
        if here and there:
            both.append(str(sig))
        if not here and not there:
            unassigned.append(str(sig))
        if there:
            files |= set(re.findall(r"tests/\w+\.py", EXCLUDED[sig.name()]))
    assert not unassigned, "in no family and not excluded: %s" % unassigned
    assert not both, both
    here = os.path.dirname(os.path.abspath(__file__))
    assert all(os.path.exists(os.path.join(here, "..", f)) for f in files), files


# ---- found by the corpus -------------------------------------------------------------------------------------------------
def test_a_per_row_pad_to_more_than_65536_characters_raises_in_the_oracle_as_on_the_device(hostlib):  # noqa: F811
    """lpad(s, k) / rpad(s, k, t) with k = 100000: the device library raises (gdv_pad_fill_row: more than 65536 characters
    is an error, as a literal length above it is refused when the projector is made); the oracle used to return the
    padded text.  Decided in PARITY.md: it raises on a row that needs the padding, and only there."""
    def rows(s, k, t="*"):
        return pa.RecordBatch.from_arrays([pa.array(s, pa.string()), pa.array([t] * len(s), pa.string()), pa.array(s, pa.string()).cast(pa.binary()),
                                           pa.array(k, pa.int32())], schema=R.SCHEMA)
    trees = [R.F("lpad", "str", "s", "k"), R.F("rpad", "str", "s", "k", "t")]
    specs = [{"tree": t, "ret": "str"} for t in trees]
    exprs = R.build_expressions(gandiva, specs)
    with pytest.raises(Exception, match="invalid argument"):
        oracle.project(exprs, rows(["a"], [65537]))
    with pytest.raises(Exception, match="invalid argument"):
        oracle.project(exprs[1:], rows(["ab", "a"], [3, 100000]))
    # 65536 characters are padded; an empty or NULL text, a NULL length, an empty fill and a text that is cut do not raise
    quiet = rows(["a", "", None, "b", "x" * 70000], [65536, 65537, 65537, None, 65537])
    for g, w in zip(oracle.project(exprs, quiet), R.expected_of(specs, [c.to_pylist() for c in quiet.columns])):
        assert_bit_exact(g, w, "pads at the limit")
    assert oracle.project(exprs[1:], rows(["a"], [65537], t=""))[0].to_pylist() == ["a"]
    # the device library's function itself (host build): error bit 4 on the same rows, none on the quiet ones
    for s, k, want_err in ((["a"], [65537], 4), (["a", "", "b" * 70000], [65536, 65537, 65537], 0)):
        off, data, size = _raw_col(s)
        offt, datat, sizet = _raw_col(["*"] * len(s))
        kk = np.array(k, np.int32)
        out_off, out_data, err = np.zeros(len(s) + 1, np.int32), np.zeros(size + 70000 * len(s) + 64, np.uint8), C.c_int(0)
        hostlib.host_pad_row(0, _p(off), _p(data), C.c_long(size), _p(kk), _p(offt), _p(datat), C.c_long(sizet), C.c_long(len(s)), _p(out_off), _p(out_data), C.byref(err))
        assert err.value == want_err, (s[0], k)
