"""regexp_extract without a GPU.

PARITY STATUS: 2-engines for the extents (PARITY.md, regexp_extract): the expected bytes come from RE2 itself, through
pyarrow.compute.extract_regex in this image's libarrow.  The rules around the extents (no match / a group that took no
part give "", null iff the text is null, literal pattern and index) are recollection.  This file checks
  * the pattern compiler (gdv_compile_regex_extract) and the device function compiled for the host
    (tests/host_devlib/host_regexp_extract.cc) against RE2: random patterns from a grammar confined to the accepted
    syntax, hand vectors, and a text on which a backtracking matcher does not finish;
  * the Make-time errors;
  * plans that use the function, cross-compiled for gfx950 by hipRTC; both registries; and that plans WITHOUT it
    generate what they generated before it is first used.
tests/test_regexp_extract.py (GPU) takes its patterns, texts and expected values from here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import gandiva_amd as gandiva
from gandiva_amd import _capi, gandiva as gg, workloads as W

HERE = os.path.dirname(os.path.abspath(__file__))
STR, I32 = pa.string(), pa.int32()
TABLE_MAX = 32768  # GDV_REGEX_EXTRACT_TABLE_MAX_BYTES

# ------------------------------------------------------------------ the two engines


def re2_groups(pattern, texts):
    """RE2: for every text the bytes of the groups g0 .. gN of `pattern` (every group named gK), "" for a group that
    took no part and for a text without a match"""
    names = _group_names(pattern)
    got = pc.extract_regex(_utf8(texts), pattern=pattern)
    out = []
    for x in got.to_pylist():
        out.append([b""] * len(names) if x is None else [(x[n] or "").encode() for n in names])
    return out


def _utf8(texts):
    """the texts as a utf8 array (over a binary array RE2 runs in Latin-1 mode: '.' would be one byte)"""
    return pa.array([t.decode("utf-8") for t in texts], pa.string())


def _group_names(pattern):
    raw = pattern if isinstance(pattern, bytes) else pattern.encode()
    names, at = [], 0
    while True:
        at = raw.find(b"(?P<g", at)
        if at < 0:
            return names
        end = raw.index(b">", at)
        names.append(raw[at + 4:end].decode())
        at = end


def compile_table(pattern, group):
    """(table, None) or (None, the reason)"""
    raw = pattern if isinstance(pattern, bytes) else pattern.encode()
    buf = np.zeros(TABLE_MAX + 16, dtype=np.uint8)
    n = C.c_int64(0)
    rc = _capi.lib().gdv_compile_regex_extract(raw, C.c_int64(len(raw)), C.c_int32(group), buf.ctypes.data_as(C.c_void_p),
                                               C.c_int64(TABLE_MAX), C.byref(n))
    if rc != 0:
        return None, _capi.last_error()
    assert 0 < n.value <= TABLE_MAX
    return buf[:n.value + 16].copy(), None


SRC = os.path.join(HERE, "host_devlib", "host_regexp_extract.cc")
LIB = os.path.join(HERE, "host_devlib", "libhost_regexp_extract.so")


@pytest.fixture(scope="module")
def hostlib():
    hdr = os.path.join(HERE, "..", "gandiva_amd", "csrc", "gdv_device_lib.hpp")
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off",
                               "-Wno-unused-function", "-Wno-unused-variable", "-Wno-attributes", SRC, "-o", LIB])
    lib = C.CDLL(LIB)
    lib.host_regexp_extract.restype = C.c_long
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_extract(lib, table, texts, text_map=0):
    off = np.zeros(len(texts) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(t) for t in texts])
    data = np.frombuffer(b"".join(texts) + b"\0" * 24, dtype=np.uint8).copy()
    frm = np.zeros(len(texts), dtype=np.int32)
    ln = np.zeros(len(texts), dtype=np.int32)
    outside = lib.host_regexp_extract(_p(off), _p(data), C.c_long(int(off[-1])), _p(table), C.c_long(len(texts)), text_map,
                                      _p(frm), _p(ln))
    assert outside == 0, "a result that is no slice of its row"
    return [t[a:a + n] for t, a, n in zip(texts, frm, ln)]


# ------------------------------------------------------------------ random patterns: a grammar inside the accepted syntax
#
# A pattern is a tree: ("lit", text, bytes) | ("set", text, [sample bytes]) | ("cat", [..]) | ("alt", [..]) |
# ("grp", k, x) | ("ncg", x) | ("rep", x, lo, hi | None, suffix) | ("asr", text).  It is rendered with every group named
# gK, g0 around everything, and sampled (assertions ignored: a sample need not match).

LITERALS = [(c, c.encode()) for c in "abcxyk s01_-@="] + [("\\.", b"."), ("\\+", b"+"), ("é", "é".encode()), ("€", "€".encode())]
SETS = [("[a-c]", [b"a", b"b", b"c"]), ("[0-9]", [b"0", b"5", b"9"]), ("\\d", [b"0", b"7"]), ("\\w", [b"a", b"_", b"3", b"X"]),
        ("\\s", [b" ", b"\t"]), ("[^a]", [b"b", b"x", "é".encode(), b" "]), ("\\D", [b"a", b"-", "€".encode()]),
        ("\\W", [b" ", b"@", "é".encode()]), (".", [b"a", b"x", b"0", "é".encode(), "🙂".encode()]),
        ("[[:alpha:]]", [b"a", b"Q"]), ("[ab_]", [b"a", b"b", b"_"]), ("[xyé]", [b"x", b"y", "é".encode()]),
        ("[^0-9x]", [b"a", b"-", "€".encode()]), ("\\S", [b"a", b"=", "é".encode()])]
TWO_POSITIONS = {"[^a]", "\\D", "\\W", ".", "[^0-9x]", "\\S"}  # a lead byte and its continuation bytes
ASSERTIONS = ["^", "$", "\\b", "\\B"]
NOISE = [b"a", b"b", b"c", b"x", b"y", b"k", b"s", b"0", b"1", b"_", b"-", b"@", b"=", b" ", b".", "é".encode(), "€".encode(),
         "🙂".encode(), b"A", b"K"]


def _positions(x, fold):
    k = x[0]
    if k == "lit":
        n = len(x[2])
        if fold and x[2] in (b"k", b"s"):
            n += 3  # the Kelvin sign / the long s fold onto them
        return n
    if k == "set":
        return (2 if x[1] in TWO_POSITIONS else 1) + (5 if fold else 0)
    if k in ("cat", "alt"):
        return sum(_positions(c, fold) for c in x[1])
    if k == "grp":
        return _positions(x[2], fold)
    if k == "ncg":
        return _positions(x[1], fold)
    if k == "rep":
        copies = x[3] if x[3] is not None else x[2] + 1
        return _positions(x[1], fold) * max(copies, 1)
    return 0


def _nullable(x):
    k = x[0]
    if k in ("lit", "set"):
        return False
    if k == "asr":
        return True
    if k == "cat":
        return all(_nullable(c) for c in x[1])
    if k == "alt":
        return any(_nullable(c) for c in x[1])
    if k == "grp":
        return _nullable(x[2])
    if k == "ncg":
        return _nullable(x[1])
    return x[2] == 0 or _nullable(x[1])


class PatternGen:
    def __init__(self, rng, fold):
        self.rng, self.fold, self.groups = rng, fold, 0

    def pick(self, xs):
        return xs[int(self.rng.integers(0, len(xs)))]

    def atom(self, depth):
        r = self.rng.random()
        if depth < 3 and r < 0.30:
            if self.rng.random() < 0.75:
                self.groups += 1
                k = self.groups  # numbered by opening parenthesis
                return ("grp", k, self.alt(depth + 1))
            return ("ncg", self.alt(depth + 1))
        if r < 0.62:
            lits = [l for l in LITERALS if not (self.fold and l[1][0] >= 0x80)]
            return ("lit",) + self.pick(lits)
        sets = [s for s in SETS if not (self.fold and any(b >= 0x80 for b in s[0].encode()))]
        return ("set",) + self.pick(sets)

    def piece(self, depth):
        if self.rng.random() < 0.08:
            return ("asr", self.pick(ASSERTIONS))
        x = self.atom(depth)
        if self.rng.random() < 0.42:
            lo, hi, text = self.pick([(0, None, "*"), (1, None, "+"), (0, 1, "?"), (2, 2, "{2}"), (1, None, "{1,}"), (1, 3, "{1,3}"),
                                      (0, 2, "{0,2}"), (2, 3, "{2,3}"), (0, None, "*"), (1, None, "+")])
            # a loop without an upper bound over a body that can be empty is refused: keep a few, bound the others
            if hi is None and _nullable(x) and self.rng.random() < 0.9:
                lo, hi, text = self.pick([(0, 1, "?"), (1, 2, "{1,2}")])
            if self.rng.random() < 0.3:
                text += "?"
            return ("rep", x, lo, hi, text)
        return x

    def cat(self, depth):
        return ("cat", [self.piece(depth) for _ in range(int(self.rng.integers(1, 5 if depth == 0 else 4)))])

    def alt(self, depth):
        n = 1 if self.rng.random() < 0.65 else int(self.rng.integers(2, 4))
        cats = [self.cat(depth) for _ in range(n)]
        return cats[0] if n == 1 else ("alt", cats)


def render(x):
    k = x[0]
    if k in ("lit", "set", "asr"):
        return x[1]
    if k == "cat":
        return "".join(render(c) for c in x[1])
    if k == "alt":
        return "|".join(render(c) for c in x[1])
    if k == "grp":
        return "(?P<g%d>%s)" % (x[1], render(x[2]))
    if k == "ncg":
        return "(?:%s)" % render(x[1])
    inner = render(x[1])
    if x[1][0] in ("cat", "alt", "rep", "asr"):
        inner = "(?:%s)" % inner
    return inner + x[4]


def sample(x, rng):
    k = x[0]
    if k == "lit":
        return x[2]
    if k == "set":
        return x[2][int(rng.integers(0, len(x[2])))]
    if k == "asr":
        return b""
    if k == "cat":
        return b"".join(sample(c, rng) for c in x[1])
    if k == "alt":
        return sample(x[1][int(rng.integers(0, len(x[1])))], rng)
    if k == "grp":
        return sample(x[2], rng)
    if k == "ncg":
        return sample(x[1], rng)
    hi = x[3] if x[3] is not None else x[2] + 2
    return b"".join(sample(x[1], rng) for _ in range(int(rng.integers(x[2], hi + 1))))


def random_pattern(rng):
    """(pattern text with groups g0 .. gN, its tree): at most 40 positions, groups nested at most 3 deep"""
    while True:
        fold = rng.random() < 0.12
        g = PatternGen(rng, fold)
        tree = g.alt(0)
        if g.groups == 0 or g.groups > 5 or _positions(tree, fold) > 40:
            continue
        return ("(?i)" if fold else "") + "(?P<g0>%s)" % render(tree), tree


def _noise(rng, n):
    return b"".join(NOISE[int(rng.integers(0, len(NOISE)))] for _ in range(n))


def texts_for(tree, rng, n=32):
    out = [b""]
    while len(out) < 21:  # samples of the pattern in noise
        out.append(_noise(rng, int(rng.integers(0, 5))) + sample(tree, rng) + _noise(rng, int(rng.integers(0, 5))))
    while len(out) < 24:  # two samples: the first match is the one to find
        out.append(sample(tree, rng) + _noise(rng, int(rng.integers(0, 3))) + sample(tree, rng))
    while len(out) < 29:
        out.append(_noise(rng, int(rng.integers(1, 14))))
    while len(out) < n:  # multi-byte characters around a sample
        out.append("é€".encode() + sample(tree, rng) + "🙂é".encode())
    return out


FUZZ_PATTERNS = 3000
_fuzz_cache = {}


def fuzz_corpus(count=FUZZ_PATTERNS, seed=20240611):
    """[(pattern, texts, RE2's groups per text)] — computed once per process, from RE2 alone"""
    key = (count, seed)
    if key not in _fuzz_cache:
        rng = np.random.default_rng(seed)
        corpus = []
        for _ in range(count):
            pattern, tree = random_pattern(rng)
            texts = texts_for(tree, rng)
            corpus.append((pattern, texts, re2_groups(pattern, texts)))  # raises if RE2 does not compile it
        _fuzz_cache[key] = corpus
    return _fuzz_cache[key]


def test_the_generator_gives_re2_something_to_find():
    """conditions on the corpus, from RE2 alone: every pattern compiles (re2_groups raises otherwise), at least 40 % of
    the (pattern, text) pairs match, at least 25 % have a non-empty group >= 1"""
    corpus = fuzz_corpus()
    assert len(corpus) >= 3000
    pairs = matched = with_group = 0
    for pattern, texts, want in corpus:
        assert len(texts) == 32
        hits = pc.match_substring_regex(_utf8(texts), pattern=pattern).to_pylist()
        for hit, groups in zip(hits, want):
            pairs += 1
            matched += bool(hit)
            with_group += any(g != b"" for g in groups[1:])
    print(f"pairs {pairs}, matching {matched / pairs:.3f}, with a non-empty group >= 1 {with_group / pairs:.3f}")
    assert matched >= 0.40 * pairs
    assert with_group >= 0.25 * pairs


REFUSAL_CONSTRUCTS = ("whose body can match the empty text", "automaton positions", "too many ways",
                      "distinct combinations of assertions")


def test_fuzz_against_re2(hostlib):
    corpus = fuzz_corpus()
    refused = 0
    for pattern, texts, want in corpus:
        ngroups = len(want[0])  # g0 .. gN: the product's indices 1 .. N + 1, and index 0 = the match = g0
        for index in range(ngroups + 1):
            table, why = compile_table(pattern, index)
            if table is None:
                assert index == 0, (pattern, index, why)  # a pattern is refused for every index or for none
                assert any(c in why for c in REFUSAL_CONSTRUCTS), (pattern, why)
                refused += 1
                break
            got = host_extract(hostlib, table, texts)
            expect = [w[max(index - 1, 0)] for w in want]
            for t, g, e in zip(texts, got, expect):
                assert g == e, f"{pattern!r} index {index} on {t!r}: {g!r}, RE2 {e!r}"
    print(f"refused {refused} of {len(corpus)}")
    assert refused <= 0.10 * len(corpus)


# ------------------------------------------------------------------ hand vectors

_A300 = b"x" * 140 + "é".encode() * 5 + b" key=val0 " + b"y" * 140
HAND = [
    ("(?P<g0>a|ab)", [b"ab", b"xab", b"b"]),
    ("(?P<g0>(?P<g1>a+?)(?P<g2>a*))", [b"aaa", b"baab", b"a"]),
    ("(?P<g0>(?:(?P<g1>a)|b)+)", [b"ab", b"ba", b"abab", b"bb", b"xbab"]),  # the group keeps 'a' over a later 'b' iteration
    ("(?P<g0>(?P<g1>a){2,3})", [b"aaaa", b"a", b"aa", b"baaa"]),
    ("(?P<g0>x*)", [b"", b"xx", b"axx"]),
    ("(?P<g0>(?P<g1>\\w+)@(?P<g2>\\w+))", [b"mail bob@example.com now", b"none", b"a@b", b"@b a@"]),
    ("(?P<g0>id=(?P<g1>\\d+))", [b"xx id=42;", b"id=", b"id=7", b"id=x id=123"]),  # (a match ending at the last byte)
    ("(?P<g0>(?P<g1>a|ab)(?P<g2>c|bcd)(?P<g3>d*))", [b"abcd", b"acdd"]),
    ("(?P<g0>(?P<g1>.)(?P<g2>.*?)$)", ["héllo".encode(), "€".encode(), b""]),
    ("(?P<g0>\\b(?P<g1>\\w+)\\s*$)", [b"foo bar  ", b"foo", b"  "]),
    ("(?P<g0>(?P<g1>[a-z]+)=(?P<g2>\\w*))",
     [b"k", b"k=v", b"0123456 key=val", b"0123456 key=val0", b"0123456 key=val01", _A300, b"=", b"a=" + b"w" * 290]),
    ("(?i)(?P<g0>(?P<g1>k+)s)", [b"KKs", "Ks".encode(), "kſ".encode(), b"ks"]),
    ("(?P<g0>(?P<g1>a*?)(?P<g2>b|$))", [b"aab", b"aa", b"c"]),
    ("(?P<g0>(?P<g1>x{2,})(?P<g2>x??)y)", [b"xxxxy", b"xy", b"xxy"]),
    ("(?P<g0>^(?P<g1>\\S+)\\s)", [b"first second", b" first", "é€ x".encode()]),
    ("(?P<g0>\\B(?P<g1>.))", ["aé".encode(), b"ab", b"a"]),
]
assert sorted({len(t) for t in HAND[10][1]} & {1, 15, 16, 17, 300}) == [1, 15, 16, 17, 300]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_hand_vectors_against_re2(hostlib, case):
    pattern, texts = HAND[case]
    want = re2_groups(pattern, texts)
    for index in range(len(want[0]) + 1):
        table, why = compile_table(pattern, index)
        assert table is not None, why
        assert host_extract(hostlib, table, texts) == [w[max(index - 1, 0)] for w in want], (pattern, index)


def test_the_group_keeps_its_last_iteration_as_re2_does():
    """(?:(a)|b)+ on 'ab': the second iteration takes 'b' and leaves the group alone — RE2 says so"""
    assert re2_groups("(?P<g0>(?:(?P<g1>a)|b)+)", [b"ab"]) == [[b"ab", b"a"]]


def test_text_read_through_a_case_map(hostlib):
    table, why = compile_table("([A-Z]+)=", 1)
    assert table is not None, why
    assert host_extract(hostlib, table, [b"ab key=1", b"KEY=2", b"="], text_map=1) == [b"key", b"KEY", b""]


def test_nested_quantifiers_take_linear_time(hostlib):
    """(a+)+$ over 2000 'a' and a 'b': no match.  A backtracking matcher does not finish this; finishing is the check."""
    texts = [b"a" * 2000 + b"b", b"a" * 2000]
    want = re2_groups("(?P<g0>(?P<g1>a+)+$)", texts)
    assert want[0] == [b"", b""]
    for index in (0, 1):
        table, why = compile_table("(a+)+$", index)
        assert table is not None, why
        assert host_extract(hostlib, table, texts) == [w[index] for w in want]


# ------------------------------------------------------------------ the compiler's refusals and the Make-time errors

@pytest.mark.parametrize("pattern, construct", [("(a*)*", "body can match the empty text"), ("(a|)+", "body can match the empty text"),
                                                ("(\\b)*", "body can match the empty text"), ("x(a?){2,}", "body can match the empty text"),
                                                ("a" * 64, "more than 63 automaton positions"), ("(a)\\1", "escape"),
                                                ("(?=a)", "look-around"), ("a*+", "possessive")])
def test_refused_constructs_are_named(pattern, construct):
    table, why = compile_table(pattern, 0)
    assert table is None and construct in why and "CodeGenError" in why, why


def test_63_positions_are_taken_and_groups_are_numbered_by_opening_parenthesis(hostlib):
    table, why = compile_table("a" * 63, 0)
    assert table is not None, why
    assert host_extract(hostlib, table, [b"b" + b"a" * 64, b"a" * 62]) == [b"a" * 63, b""]
    for index, want in ((1, b"abc"), (2, b"a"), (3, b"c")):  # (?: ) does not count, (?P<name> ) does
        table, why = compile_table("((a)(?:b)(?P<n>c))", index)
        assert table is not None, why
        assert host_extract(hostlib, table, [b"xabc"]) == [want]


@pytest.mark.parametrize("index, groups", [(-1, 2), (3, 2), (1, 0)])
def test_an_index_outside_the_groups_is_an_error_naming_both(index, groups):
    pattern = "(a)(?:b)(c)" if groups == 2 else "abc"
    table, why = compile_table(pattern, index)
    assert table is None and f"group index {index} " in why and f"0..{groups} " in why, why


SCH = pa.schema([pa.field("s", STR), pa.field("d", STR), pa.field("k", I32)])


def _tree():
    b = gandiva.TreeExprBuilder()
    s, d, k = (b.make_field(SCH.field(i)) for i in range(3))
    return b, s, d, k


def _extract(b, s, pattern, index):
    pat = pattern if not isinstance(pattern, str) else b.make_literal(pattern, STR)
    idx = index if not isinstance(index, int) else b.make_literal(index, I32)
    return b.make_function("regexp_extract", [s, pat, idx], STR)


def _make(node):
    b = gandiva.TreeExprBuilder()
    return gandiva.make_projector(SCH, [b.make_expression(node, pa.field("o", STR))], pa.default_memory_pool())


def test_index_out_of_range_fails_at_make():
    b, s, d, k = _tree()
    with pytest.raises(Exception, match=r"group index 2 is outside the groups 0\.\.1 "):
        _make(_extract(b, s, "id=(\\d+)", 2))
    with pytest.raises(Exception, match=r"group index -1 is outside the groups 0\.\.1 "):
        _make(_extract(b, s, "id=(\\d+)", -1))


def test_per_row_pattern_or_index_fails_at_make():
    b, s, d, k = _tree()
    with pytest.raises(Exception, match=r"regexp_extract.*literal pattern and a literal group index"):
        _make(_extract(b, s, d, 1))
    with pytest.raises(Exception, match=r"regexp_extract.*literal pattern and a literal group index"):
        _make(_extract(b, s, "(a)", k))


def test_refused_construct_and_64_positions_fail_at_make():
    b, s, d, k = _tree()
    with pytest.raises(Exception, match=r"body can match the empty text"):
        _make(_extract(b, s, "(a*)*", 1))
    with pytest.raises(Exception, match=r"more than 63 automaton positions"):
        _make(_extract(b, s, "(" + "a" * 64 + ")", 1))


def test_general_regexp_replace_stays_refused():
    b, s, d, k = _tree()
    with pytest.raises(Exception, match=r"regexp_replace"):
        _make(b.make_function("regexp_replace", [s, b.make_literal("a+", STR), b.make_literal("b", STR)], STR))


# ------------------------------------------------------------------ registries

def test_registry_lists_regexp_extract():
    sigs = {(s.name(), tuple(s.param_types())): s.return_type() for s in gandiva.get_registered_function_signatures()}
    assert sigs.get(("regexp_extract", (STR, STR, I32))) == STR


def test_registry_of_the_rebuilt_pyarrow_gandiva_lists_regexp_extract():
    from gandiva_amd import pyarrow_gandiva
    pg = pyarrow_gandiva.load()
    sigs = {(s.name(), tuple(s.param_types())): s.return_type() for s in pg.get_registered_function_signatures()}
    assert sigs.get(("regexp_extract", (STR, STR, I32))) == STR


# ------------------------------------------------------------------ plans (hipRTC cross-compile, no GPU)

def _precompile(monkeypatch, tmp_path, schema, exprs=None, cond=None, mode=0):
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
            rc = lib.gdv_precompile_projector(sh, arr, len(exprs), mode)
        assert rc == 0, _capi.last_error()
    finally:
        lib.gdv_schema_free(sh)
    return {f: open(os.path.join(tmp_path, f)).read() for f in sorted(os.listdir(tmp_path)) if f.endswith(".hip")}


def test_output_expression_cross_compiles_in_row_and_selection_mode(monkeypatch, tmp_path):
    b, s, d, k = _tree()
    exprs = [b.make_expression(_extract(b, s, "(\\w+)@(\\w+)", 2), pa.field("a", STR)),
             b.make_expression(_extract(b, s, "id=(\\d+)", 0), pa.field("b", STR))]
    for mode in (0, 1, 2):
        texts = _precompile(monkeypatch, tmp_path / str(mode), SCH, exprs=exprs, mode=mode)
        assert texts and any("gdv_regex_extract(" in t for t in texts.values()), mode


def test_consumers_of_a_slice_take_it_cross_compile(monkeypatch, tmp_path):
    b, s, d, k = _tree()
    as_int = b.make_function("castINT", [_extract(b, s, "id=(\\d+)", 1)], I32)
    length = b.make_function("length", [_extract(b, s, "(a+)", 1)], I32)
    texts = _precompile(monkeypatch, tmp_path / "p", SCH, exprs=[b.make_expression(as_int, pa.field("i", I32)),
                                                                 b.make_expression(length, pa.field("n", I32))])
    assert any("gdv_regex_extract(" in t and "castINT_utf8" in t and "char_length_utf8" in t for t in texts.values())
    cond = b.make_condition(b.make_function("equal", [_extract(b, s, "k=(\\w+)", 1), b.make_literal("v", STR)], pa.bool_()))
    texts = _precompile(monkeypatch, tmp_path / "f", SCH, cond=cond)
    assert any("gdv_regex_extract(" in t and "equal_utf8_utf8" in t for t in texts.values())


def _dump(monkeypatch, tmp_path, name):
    out = {}
    out.update(_precompile(monkeypatch, tmp_path / (name + "c2"), W.c2_schema(), exprs=W.c2_expressions()))
    out.update(_precompile(monkeypatch, tmp_path / (name + "c5"), W.c5_schema(), exprs=W.c5_expressions()))
    return out


def test_plans_without_the_function_generate_what_they_generated(monkeypatch, tmp_path):
    """C2's and C5's generated source (kernel names hash it, with the library functions it reaches) before and after
    the function is first planned; and neither mentions it"""
    before = _dump(monkeypatch, tmp_path, "before")
    b, s, d, k = _tree()
    _precompile(monkeypatch, tmp_path / "use", SCH, exprs=[b.make_expression(_extract(b, s, "(a)|b", 1), pa.field("a", STR))])
    after = _dump(monkeypatch, tmp_path, "after")
    assert before and before == after
    assert not any("regex_extract" in t for t in before.values())
