"""Round 4, registry tail: castVARCHAR(decimal128, n).  The text is Arrow's Decimal128::ToString(scale) —
pinned here against pyarrow's own decimal -> string cast (the same C++ routine the reference calls through
gdv_fn_dec_to_string) for the oracle AND for the product's device function compiled for the host; the GPU
tests then hold the kernels against the oracle."""
import ctypes as C
import decimal

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import gandiva_amd as gandiva
from gandiva_amd import workloads as W
from helpers import assert_bit_exact
from oracle import oracle
from test_device_lib_on_host import hostlib, _raw128  # noqa: F401  (fixture)

WIDE = decimal.Context(prec=80)
TYPES = [(38, 0), (10, 2), (38, 10), (38, 38), (20, 19), (15, 8), (38, 37), (5, 5), (12, 12), (19, 0), (20, 1), (7, 7)]


def decimals(p, s, seed, extra=300, null_every=11):
    rng = np.random.default_rng(seed)
    vals = [0, 1, -1, 7, -7, 10 ** p - 1, -(10 ** p - 1), 10 ** (p - 1), 123456789, -123456789012345678, 10 ** 19, 10 ** 19 - 1,
            -(10 ** 20), 5 * 10 ** 18, 10 ** 18, 99, -100, 1000000, 12345678901234567890123456789012345678]
    vals += [int(rng.integers(-10 ** 18, 10 ** 18)) * int(rng.integers(1, 10 ** 18)) for _ in range(extra)]
    vals += [int(rng.integers(-10 ** 6, 10 ** 6)) for _ in range(extra // 2)]
    vals += [int(rng.integers(-10 ** 18, 10 ** 18)) * 10 ** int(rng.integers(0, 20)) for _ in range(extra // 2)]
    vals = [v for v in vals if abs(v) < 10 ** p]
    py = [None if null_every and i % null_every == 3 else decimal.Decimal(v).scaleb(-s, context=WIDE) for i, v in enumerate(vals)]
    return pa.array(py, pa.decimal128(p, s))


def cast_expr(field, n):
    b = gandiva.TreeExprBuilder()
    return b.make_expression(b.make_function("castVARCHAR", [b.make_field(field), b.make_literal(n, pa.int64())], pa.string()),
                             pa.field("t", pa.string()))


def arrow_text(arr, n):
    full = pc.cast(arr, pa.string())
    return pc.utf8_slice_codeunits(full, 0, n) if n > 0 else pc.if_else(pc.is_valid(full), "", None)


@pytest.mark.parametrize("p,s", TYPES)
def test_oracle_text_of_a_decimal_is_arrows(p, s):
    arr = decimals(p, s, 100 * p + s)
    batch = pa.RecordBatch.from_arrays([arr], names=["d"])
    for n in (100, 44, 7, 1, 0):
        got = oracle.project([cast_expr(batch.schema.field(0), n)], batch)[0]
        assert got.equals(arrow_text(arr, n).cast(pa.string())), (p, s, n)


@pytest.mark.parametrize("p,s", TYPES)
def test_device_function_on_the_host_writes_arrows_text(hostlib, p, s):  # noqa: F811
    arr = decimals(p, s, 7 * p + s, null_every=0)
    raw = _raw128(arr)
    n = len(arr)
    for cut in (100, 20, 3):
        off = np.zeros(n + 1, dtype=np.int32)
        data = np.zeros(64 * n + 64, dtype=np.uint8)
        err = hostlib.host_cast_varchar_decimal(raw.ctypes.data_as(C.c_void_p), p, s, C.c_long(n), C.c_longlong(cut),
                                                off.ctypes.data_as(C.c_void_p), data.ctypes.data_as(C.c_void_p))
        assert err == 0
        got = [bytes(data[off[i]:off[i + 1]]).decode() for i in range(n)]
        assert got == arrow_text(arr, cut).to_pylist(), (p, s, cut)


def test_a_negative_length_is_an_error_and_the_signature_is_registered():
    sigs = [s for s in gandiva.get_registered_function_signatures() if s.name() == "castVARCHAR"]
    assert any(pa.types.is_decimal(s.param_types()[0]) for s in sigs)
    arr = decimals(10, 2, 5)
    batch = pa.RecordBatch.from_arrays([arr], names=["d"])
    with pytest.raises(Exception):
        oracle.project([cast_expr(batch.schema.field(0), -1)], batch)


@pytest.mark.gpu
@pytest.mark.parametrize("p,s", TYPES)
def test_cast_decimal_to_text_on_the_gpu(p, s):
    arr = decimals(p, s, 31 * p + s, extra=3000)
    batch = pa.RecordBatch.from_arrays([arr], names=["d"])
    for n in (100, 9):
        e = cast_expr(batch.schema.field(0), n)
        proj = gandiva.make_projector(batch.schema, [e], None)
        got = proj.evaluate(batch)[0]
        assert_bit_exact(got, oracle.project([e], batch)[0], f"decimal128({p},{s}) -> text, cut {n}")
        assert got.equals(arrow_text(arr, n).cast(pa.string()))
        dev = proj.evaluate_device(gandiva.DeviceBatch.from_arrow(batch))[0].to_arrow()
        assert_bit_exact(dev, got, "HBM-resident")


@pytest.mark.gpu
def test_text_of_a_decimal_feeds_other_string_functions_and_selection_mode():
    arr = decimals(20, 4, 77, extra=2000)
    k = pa.array(np.arange(len(arr)) % 7, pa.int64())
    batch = pa.RecordBatch.from_arrays([arr, k], names=["d", "k"])
    b = gandiva.TreeExprBuilder()
    fd, fk = b.make_field(batch.schema.field(0)), b.make_field(batch.schema.field(1))
    txt = b.make_function("castVARCHAR", [fd, b.make_literal(30, pa.int64())], pa.string())
    exprs = [b.make_expression(b.make_function("concat", [b.make_literal("[", pa.string()), txt, b.make_literal("]", pa.string())], pa.string()),
                               pa.field("c", pa.string())),
             b.make_expression(b.make_function("like", [txt, b.make_literal("%.12%", pa.string())], pa.bool_()), pa.field("l", pa.bool_())),
             b.make_expression(b.make_function("length", [txt], pa.int32()), pa.field("n", pa.int32())),
             b.make_expression(b.make_function("castVARCHAR", [b.make_function("multiply", [fd, fd], pa.decimal128(38, 6)), fk], pa.string()),
                               pa.field("sq", pa.string()))]
    proj = gandiva.make_projector(batch.schema, exprs, None)
    for g, w in zip(proj.evaluate(batch), oracle.project(exprs, batch)):
        assert_bit_exact(g, w, "two-stage consumers of the text")
    cond = b.make_condition(b.make_function("greater_than", [fk, b.make_literal(3, pa.int64())], pa.bool_()))
    sel = gandiva.make_filter(batch.schema, cond).evaluate(batch, None, "int32")
    psel = gandiva.make_projector(batch.schema, exprs, None, "UINT32")
    taken = oracle.take_rows(batch, sel.to_array().to_numpy())
    for g, w in zip(psel.evaluate(batch, sel), oracle.project(exprs, taken)):
        assert_bit_exact(g, w, "selection mode")
    with pytest.raises(Exception):
        gandiva.make_projector(batch.schema, [cast_expr(batch.schema.field(0), -2)], None).evaluate(batch)


# ------------------------------------------------------------------ date_trunc_*, extractWeek / weekofyear, last_day

UNITS = ["Second", "Minute", "Hour", "Day", "Week", "Month", "Quarter", "Year", "Decade", "Century", "Millennium"]


def instants(seed, n=4000):
    rng = np.random.default_rng(seed)
    fixed = [0, -1, 1, 86399999, 86400000, -86400000, -86400001, 951782400000, 951868800000, 4102444800000, -2208988800000,
             1609459199999, 1609459200000, 1230768000000, 1262217600000, 1293753600000, 978307200000 - 1, 978307200000,
             -62135596800000, 253402300799999]
    return np.concatenate([np.array(fixed), rng.integers(-62135596800000, 253402300799999, n),
                           rng.integers(-3 * 10 ** 12, 5 * 10 ** 12, n)]).astype(np.int64)


def independent_answer(unit, ms):
    """pyarrow.compute where it has the operation, the calendar by hand elsewhere."""
    arr = pa.array(ms, pa.timestamp("ms"))
    if unit in ("Second", "Minute", "Hour", "Day"):
        # upstream's DATE_TRUNC_FIXED_UNIT is (millis / N) * N with C++ division: towards ZERO, so instants before
        # 1970 go up.  pyarrow floors; mirrored around zero it is the same rule.
        up = -pc.floor_temporal(pa.array(-ms, pa.timestamp("ms")), unit=unit.lower()).cast(pa.int64()).to_numpy()
        down = pc.floor_temporal(arr, unit=unit.lower()).cast(pa.int64()).to_numpy()
        return np.where(ms < 0, up, down)
    if unit in ("Month", "Quarter", "Year"):
        return pc.floor_temporal(arr, unit=unit.lower()).cast(pa.int64()).to_numpy()
    if unit == "Week":
        return pc.floor_temporal(arr, unit="week", week_starts_monday=True).cast(pa.int64()).to_numpy()
    if unit == "IsoWeek":
        return pc.iso_week(arr).to_numpy()
    years = pc.year(arr).to_numpy()
    if unit == "Last":
        months = pc.month(arr).to_numpy()
        nxt = np.array([np.datetime64(f"{y + (m == 12):04d}-{m % 12 + 1:02d}-01", "D") for y, m in zip(years, months)])
        return (nxt - np.timedelta64(1, "D")).astype("datetime64[ms]").astype(np.int64)
    start = {"Decade": (years - 1) // 10 * 10 + 1, "Century": (years - 1) // 100 * 100 + 1, "Millennium": (years - 1) // 1000 * 1000 + 1}[unit]
    return np.array([np.datetime64(f"{y:04d}-01-01", "ms") for y in start]).astype(np.int64)


def date_expr(name, field, out_type):
    b = gandiva.TreeExprBuilder()
    return b.make_expression(b.make_function(name, [b.make_field(field)], out_type), pa.field("r", out_type))


def date_cases():
    return ([(f"date_trunc_{u}", u, None) for u in UNITS] + [("extractWeek", "IsoWeek", pa.int64()), ("weekofyear", "IsoWeek", pa.int64()),
                                                             ("last_day", "Last", pa.date64())])


@pytest.mark.parametrize("t", [pa.timestamp("ms"), pa.date64()])
def test_oracle_unit_starts_iso_weeks_and_month_ends_agree_with_pyarrow_and_the_calendar(t):
    ms = instants(5)
    if pa.types.is_date64(t):
        ms = ms // 86400000 * 86400000
    ms = ms[ms >= -62135596800000 + 86400000 * 400]          # (year 1 onwards: numpy / pyarrow calendars agree there)
    batch = pa.RecordBatch.from_arrays([pa.array(ms, pa.int64()).cast(t)], names=["t"])
    for name, unit, rt in date_cases():
        got = oracle.project([date_expr(name, batch.schema.field(0), rt or t)], batch)[0]
        assert got.cast(pa.int64()).to_numpy().tolist() == independent_answer(unit, ms).tolist(), (name, str(t))


def test_device_date_functions_on_the_host(hostlib):  # noqa: F811
    ms = instants(6)
    ms = ms[ms >= -62135596800000 + 86400000 * 400]
    out = np.zeros(len(ms), np.int64)
    for op, unit in enumerate(UNITS + ["IsoWeek", "Last"]):
        hostlib.host_date_trunc_timestamp(op, ms.ctypes.data_as(C.c_void_p), C.c_long(len(ms)), out.ctypes.data_as(C.c_void_p))
        assert out.tolist() == independent_answer(unit, ms).tolist(), unit


@pytest.mark.gpu
@pytest.mark.parametrize("t", [pa.timestamp("ms"), pa.date64()])
def test_date_trunc_week_and_last_day_on_the_gpu(t):
    ms = instants(7, n=30_000)
    if pa.types.is_date64(t):
        ms = ms // 86400000 * 86400000
    mask = np.arange(len(ms)) % 13 == 5
    batch = pa.RecordBatch.from_arrays([pa.array(ms, pa.int64(), mask=mask).cast(t)], names=["t"])
    exprs = [date_expr(name, batch.schema.field(0), rt or t) for name, _, rt in date_cases()]
    proj = gandiva.make_projector(batch.schema, exprs, None)
    for g, w, (name, _, _) in zip(proj.evaluate(batch), oracle.project(exprs, batch), date_cases()):
        assert_bit_exact(g, w, name)


# ------------------------------------------------------------------ round 5: initcap
# [recalled: string_ops.cc initcap_utf8 — "any character is considered as space, except if it is alphanumeric"]: the
# first letter of a word in upper case, the other letters in lower case, digits are word characters.  ASCII letters
# only on this backend (bytes >= 0x80: copied as they are, word characters — upstream maps them through utf8proc: a
# stated divergence, oracle header).  Second engines: a regular-expression restatement over bytes, and
# pyarrow.compute.utf8_title wherever the two rules coincide (ASCII text whose words hold no digit).

import re  # noqa: E402

STR = pa.string()
WORDS = ["hello", "WORLD", "mIxEd", "a", "Z", "x1y2", "42", "9lives", "o'neil", "snake_case", "kebab-case", "dotted.name",
         "tab\tsep", "two  spaces", " lead", "trail ", "", "ÉCOLE", "straße", "naïve café", "日本語 text", "aéb CÉD", "éx"]


from string_shapes import initcap as _initcap_by_regex  # noqa: E402  (the restatement lives in tests/string_shapes.py)


def _initcap_cases(seed, n):
    rng = np.random.default_rng(seed)
    seps = [" ", "  ", "-", "_", ".", ",", "'", "/", "\t", "1", ""]
    vals = []
    for _ in range(n):
        k = int(rng.integers(0, 6))
        t = "".join(str(rng.choice(WORDS)) + str(rng.choice(seps)) for _ in range(k))
        vals.append(None if rng.random() < 0.1 else t)
    return vals


def _initcap_exprs(b, s):
    f = lambda name, *a: b.make_function(name, list(a), STR)  # noqa: E731
    lit = lambda v, t=STR: b.make_literal(v, t)  # noqa: E731
    return [("initcap", f("initcap", s)), ("initcap(upper)", f("initcap", f("upper", s))),
            ("initcap(substr)", f("initcap", f("substr", s, lit(3, pa.int64()), lit(12, pa.int64())))),
            ("concat(initcap, '!')", f("concat", f("initcap", s), lit("!"))),
            ("upper(initcap) [two-stage]", f("upper", f("initcap", s)))]


def test_oracle_initcap_matches_the_regex_restatement_and_arrows_title_where_the_rules_coincide():
    vals = WORDS + _initcap_cases(3, 3000)
    batch = pa.RecordBatch.from_arrays([pa.array(vals, STR)], names=["s"])
    b = gandiva.TreeExprBuilder()
    s = b.make_field(batch.schema.field(0))
    e = b.make_expression(b.make_function("initcap", [s], STR), pa.field("r", STR))
    got = oracle.project([e], batch)[0].to_pylist()
    assert got == [_initcap_by_regex(v) for v in vals]
    # pyarrow.compute.utf8_title starts a new word after anything that is not a LETTER (digits included) and knows
    # Unicode: same answers on ASCII text whose words carry no digit
    same = [v for v in vals if v is not None and v.isascii() and not re.search(r"\d", v)]
    title = pc.utf8_title(pa.array(same, STR)).to_pylist()
    assert [_initcap_by_regex(v) for v in same] == title
    assert gandiva.get_registered_function_signatures and any(
        sig.name() == "initcap" for sig in gandiva.get_registered_function_signatures())


def test_device_initcap_on_the_host(hostlib):  # noqa: F811
    vals = [v for v in WORDS + _initcap_cases(4, 2000) if v is not None]
    arr = pa.array(vals, STR)
    off = np.frombuffer(arr.buffers()[1], np.int32)[: len(vals) + 1].copy()
    raw = np.frombuffer(arr.buffers()[2], np.uint8) if arr.buffers()[2] is not None else np.zeros(0, np.uint8)
    size = int(off[-1])
    data = np.concatenate([raw[:size], np.zeros(64, np.uint8)])
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for mp, pre in ((0, lambda t: t), (1, lambda t: t.encode().upper().decode()), (2, lambda t: t.encode().lower().decode())):
        out_off, out_data = np.zeros(len(vals) + 1, np.int32), np.zeros(size + 64, np.uint8)
        hostlib.host_str_initcap(p(off), p(data), C.c_long(size), C.c_long(len(vals)), mp, p(out_off), p(out_data))
        got = [bytes(out_data[out_off[i]:out_off[i + 1]]).decode() for i in range(len(vals))]
        assert got == [_initcap_by_regex(pre(v)) for v in vals], mp


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 64, 1000, 40_003])
def test_initcap_on_the_gpu(n):
    vals = (WORDS + _initcap_cases(n, n))[:n] if n >= len(WORDS) else _initcap_cases(n, n)
    batch = pa.RecordBatch.from_arrays([pa.array(vals, STR)], names=["s"])
    b = gandiva.TreeExprBuilder()
    s = b.make_field(batch.schema.field(0))
    exprs = [b.make_expression(node, pa.field(f"r{i}", STR)) for i, (_, node) in enumerate(_initcap_exprs(b, s))]
    proj = gandiva.make_projector(batch.schema, exprs, None)
    for g, w, (name, _) in zip(proj.evaluate(batch), oracle.project(exprs, batch), _initcap_exprs(b, s)):
        assert_bit_exact(g, w, name)
    # under a selection vector (the wave-shaped selection-mode kernels)
    keep = np.arange(0, n, 3, dtype=np.uint32)
    sel = gandiva.SelectionVector(2, keep, len(keep))
    psel = gandiva.make_projector(batch.schema, exprs[:4], None, "UINT32")
    for g, w in zip(psel.evaluate(batch, sel), oracle.project(exprs[:4], oracle.take_rows(batch, keep))):
        assert_bit_exact(g, w, "selection mode")


# ------------------------------------------------------------------ round 5: regular expressions, the literal subset
# [recalled: regexp_like / regexp_matches = RE2::PartialMatch, regexp_replace = RE2::GlobalReplace].  The tree builder
# rewrites the literal subset onto like / replace (gdv_node.h MakeFunctionNode); everything else is CodeGenError.
# Second engine: Python's re (search / sub), whose semantics on metacharacter-free patterns are RE2's.

REGEX_OK = ["spark", "^spark", "spark$", "^spark$", "a", "^a", "k$", "ar", "é", "^日本", "x-y", "it's"]
REGEX_REFUSED = ["sp.rk", "spa*", "(spark)", "[sp]ark", "a|b", "^", "$", "", "50%", "a_b", "back\\slash", "x{2}", "q?"]
REPLACEMENTS = [("spark", "flink"), ("ar", ""), ("é", "e"), ("a", "AAA"), ("x-y", "-")]


def _regex_batch(n, seed=9):
    rng = np.random.default_rng(seed)
    base = W.c5_batch(n, 0.1).column(0).to_pylist()
    extra = ["spark", "sparks fly", "a spark", "x-y", "it's", "é", "日本語", "", "park", "sparkspark", "café x-y ar"]
    vals = [extra[int(rng.integers(0, len(extra)))] if rng.random() < 0.2 else v for v in base]
    return pa.RecordBatch.from_arrays([pa.array(vals, STR)], names=["s"])


def _regex_exprs(b, s):
    out = []
    for k, pat in enumerate(REGEX_OK):
        for fn in ("regexp_like", "regexp_matches"):
            out.append((f"{fn}({pat!r})", b.make_expression(b.make_function(fn, [s, b.make_literal(pat, STR)], pa.bool_()),
                                                            pa.field(f"m{k}{fn[-1]}", pa.bool_())), ("search", pat, None)))
    for k, (pat, to) in enumerate(REPLACEMENTS):
        out.append((f"regexp_replace({pat!r}, {to!r})",
                    b.make_expression(b.make_function("regexp_replace", [s, b.make_literal(pat, STR), b.make_literal(to, STR)], STR),
                                      pa.field(f"r{k}", STR)), ("sub", pat, to)))
    return out


def test_oracle_regexp_subset_matches_pythons_re():
    batch = _regex_batch(4000)
    b = gandiva.TreeExprBuilder()
    s = b.make_field(batch.schema.field(0))
    cases = _regex_exprs(b, s)
    got = oracle.project([e for _, e, _ in cases], batch)
    vals = batch.column(0).to_pylist()
    for (name, _, (kind, pat, to)), g in zip(cases, got):
        rx = re.compile(pat)
        want = [None if v is None else (rx.search(v) is not None if kind == "search" else rx.sub(to, v)) for v in vals]
        assert g.to_pylist() == want, name


def test_regexps_beyond_the_literal_subset_are_refused_not_guessed(monkeypatch, tmp_path):
    """The rewritten forms compile for gfx950 (they ARE like / replace plans); a pattern with a metacharacter, a LIKE
    wildcard, nothing at all, or a replacement with a backslash reaches the planner as regexp_* and is refused there
    with CodeGenError — and the oracle refuses the same inputs."""
    from test_planner_cpu import _precompile
    batch = _regex_batch(64)
    b = gandiva.TreeExprBuilder()
    s = b.make_field(batch.schema.field(0))
    ok = [e for _, e, _ in _regex_exprs(b, s)]
    files = _precompile(monkeypatch, tmp_path, batch.schema, exprs=ok[:6] + ok[-2:])
    text = "".join(open(tmp_path / f).read() for f in files)
    assert "regexp_" not in text.split("#include")[1]        # nothing of the regexp names is left below the @expr header
    assert "gdv_like" in text or "gdv_range_any" in text
    from gandiva_amd import _capi, gandiva as gg
    # (regexp_like / regexp_matches take general patterns since late round 5 — further down; regexp_replace still does not)
    for pat in REGEX_REFUSED:
        e = b.make_expression(b.make_function("regexp_replace", [s, b.make_literal(pat, STR), b.make_literal("z", STR)], STR), pa.field("r", STR))
        sh = gg._make_schema(batch.schema)
        try:
            arr = (C.c_void_p * 1)(e._h)
            assert _capi.lib().gdv_precompile_projector(sh, arr, 1, 0) == 40, (pat, _capi.last_error())
            assert "regexp_replace with a literal pattern" in _capi.last_error()
        finally:
            _capi.lib().gdv_schema_free(sh)
        with pytest.raises(Exception):
            oracle.project([e], batch)
    e = b.make_expression(b.make_function("regexp_replace", [s, b.make_literal("a", STR), b.make_literal("\\1", STR)], STR), pa.field("r", STR))
    with pytest.raises(Exception):
        oracle.project([e], batch)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 1000, 50_003])
def test_regexp_subset_on_the_gpu(n):
    batch = _regex_batch(n, seed=n)
    b = gandiva.TreeExprBuilder()
    s = b.make_field(batch.schema.field(0))
    cases = _regex_exprs(b, s)
    exprs = [e for _, e, _ in cases]
    # (one projector per group: a kernel takes one swept replace() needle and a few '%needle%' hooks)
    for lo in range(0, len(exprs), 6):
        part = exprs[lo:lo + 6]
        got = gandiva.make_projector(batch.schema, part, None).evaluate(batch)
        for g, w, (name, _, _) in zip(got, oracle.project(part, batch), cases[lo:lo + 6]):
            assert_bit_exact(g, w, name)
    cond = b.make_condition(b.make_function("regexp_like", [s, b.make_literal("^spark", STR)], pa.bool_()))
    sel = gandiva.make_filter(batch.schema, cond).evaluate(batch, None, "int32")
    assert sel.to_array().equals(oracle.filter_indices(cond, batch, "int32"))


# ------------------------------------------------------------------ round 5: hashSHA256 / hashSHA1 / hashMD5
# The digests are public standards: pinned against Python's hashlib.  [recalled] a number is hashed as the 8 bytes of
# (double)value, a NULL as the empty message, the result is lower-case hex and never null.

import hashlib  # noqa: E402
import struct  # noqa: E402

DIGESTS = [("hashSHA256", "sha256", hashlib.sha256, 0), ("hashSHA1", "sha1", hashlib.sha1, 1), ("hashMD5", "md5", hashlib.md5, 2)]
DIGEST_TEXTS = ["", "a", "abc", "message digest", "x" * 55, "y" * 56, "z" * 63, "w" * 64, "v" * 65, "u" * 119, "t" * 120, "s" * 1000,
                "The quick brown fox jumps over the lazy dog", "日本語テキスト", "é" * 40]


def _digest_batch(n, seed=5):
    rng = np.random.default_rng(seed)
    base = W.c5_batch(n, 0.1).column(0).to_pylist()
    vals = [(DIGEST_TEXTS[int(rng.integers(0, len(DIGEST_TEXTS)))] if rng.random() < 0.3 else v) for v in base]
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 12, n)
    x[:min(4, n)] = [0.0, -0.0, 1.0, -1.5][:n]
    k = rng.integers(-2 ** 40, 2 ** 40, n)
    m = rng.random(n) < 0.1
    return pa.RecordBatch.from_arrays([pa.array(vals, STR), pa.array(x, pa.float64(), mask=m), pa.array(k, pa.int64(), mask=m),
                                       pa.array((k % 1000).astype(np.int32), pa.int32())], names=["s", "x", "k", "i"])


def _digest_exprs(b, batch):
    s, x, k, i32 = (b.make_field(batch.schema.field(j)) for j in range(4))
    out = []
    for name, alias, fn, _ in DIGESTS:
        out += [(f"{name}(s)", b.make_function(name, [s], STR), ("s", fn)), (f"{alias}(upper(s))", b.make_function(alias, [b.make_function("upper", [s], STR)], STR), ("S", fn)),
                (f"{name}(x)", b.make_function(name, [x], STR), ("x", fn)), (f"{alias}(k)", b.make_function(alias, [k], STR), ("k", fn)),
                (f"{name}(i)", b.make_function(name, [i32], STR), ("i", fn))]
    return out


def _digest_want(batch, what, fn):
    col = {"s": 0, "S": 0, "x": 1, "k": 2, "i": 3}[what]
    want = []
    for v in batch.column(col).to_pylist():
        if v is None:
            msg = b""
        elif what == "s":
            msg = v.encode()
        elif what == "S":
            msg = v.encode().upper()
        else:
            msg = struct.pack("<d", float(v))
        want.append(fn(msg).hexdigest())
    return want


def test_oracle_digests_match_hashlib():
    batch = _digest_batch(1500)
    b = gandiva.TreeExprBuilder()
    cases = _digest_exprs(b, batch)
    exprs = [b.make_expression(node, pa.field(f"h{j}", STR)) for j, (_, node, _) in enumerate(cases)]
    for (name, _, (what, fn)), g in zip(cases, oracle.project(exprs, batch)):
        assert g.null_count == 0 and g.to_pylist() == _digest_want(batch, what, fn), name


def test_device_digests_on_the_host(hostlib):  # noqa: F811
    batch = _digest_batch(600, seed=8)
    arr = batch.column(0)
    vals = arr.to_pylist()
    filled = pa.array([v if v is not None else "" for v in vals], STR)
    off = np.frombuffer(filled.buffers()[1], np.int32)[: len(vals) + 1].copy()
    size = int(off[-1])
    data = np.concatenate([np.frombuffer(filled.buffers()[2], np.uint8)[:size], np.zeros(64, np.uint8)])
    valid = np.array([v is not None for v in vals], np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for _, _, fn, algo in DIGESTS:
        nhex = fn(b"").digest_size * 2
        for mp, what in ((0, "s"), (1, "S")):
            out = np.zeros(64 * len(vals), np.uint8)
            hostlib.host_str_digest(algo, p(off), p(data), C.c_long(size), C.c_long(len(vals)), p(valid), mp, p(out))
            got = [bytes(out[64 * i:64 * i + nhex]).decode() for i in range(len(vals))]
            assert got == _digest_want(batch, what, fn), (algo, mp)
        x = np.asarray(batch.column(1).fill_null(0.0), np.float64)
        xv = np.array([v is not None for v in batch.column(1).to_pylist()], np.uint8)
        out = np.zeros(64 * len(x), np.uint8)
        hostlib.host_f64_digest(algo, p(x), C.c_long(len(x)), p(xv), p(out))
        got = [bytes(out[64 * i:64 * i + nhex]).decode() for i in range(len(x))]
        assert got == _digest_want(batch, "x", fn), algo


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 64, 1000, 20_011])
def test_digests_on_the_gpu(n):
    batch = _digest_batch(n, seed=n)
    b = gandiva.TreeExprBuilder()
    cases = _digest_exprs(b, batch)
    for lo in range(0, len(cases), 5):     # one projector per algorithm (a wave's LDS staging windows are three)
        part = cases[lo:lo + 5]
        for j in range(0, len(part), 3):
            exprs = [b.make_expression(node, pa.field(f"h{q}", STR)) for q, (_, node, _) in enumerate(part[j:j + 3])]
            got = gandiva.make_projector(batch.schema, exprs, None).evaluate(batch)
            for g, w, (name, _, _) in zip(got, oracle.project(exprs, batch), part[j:j + 3]):
                assert_bit_exact(g, w, name)
    # a digest as the argument of another function: two stages
    s = b.make_field(batch.schema.field(0))
    e = b.make_expression(b.make_function("upper", [b.make_function("substr", [b.make_function("hashMD5", [s], STR), b.make_literal(1, pa.int64()),
                                                                             b.make_literal(8, pa.int64())], STR)], STR), pa.field("u", STR))
    got = gandiva.make_projector(batch.schema, [e], None).evaluate(batch)
    assert_bit_exact(got[0], oracle.project([e], batch)[0], "upper(substr(hashMD5(s), 1, 8))")


# ------------------------------------------------------------------------------------------------
# round 5: castVARCHAR(float32 / float64, n) — shortest round-trip digits, Java-compatible layout.
#   engine 1 (oracle): the C library's "%.{p}e" with growing p until strtod / strtof reads the value back
#   engine 2 (device library, host build and GPU): Burger-Dybvig free-format over exact big integers
#   engine 3 (here): numpy's Dragon4 "unique" digits / Python's repr
import math  # noqa: E402


def _java_layout(digits, k, neg):
    """digits without trailing zeros, value = 0.digits * 10^k"""
    x, nd = k - 1, len(digits)
    if -3 <= x < 7:
        t = "0." + "0" * (-k) + digits if k <= 0 else digits + "0" * (k - nd) + ".0" if nd <= k else digits[:k] + "." + digits[k:]
    else:
        t = digits[0] + "." + (digits[1:] or "0") + "E" + str(x)
    return ("-" if neg else "") + t


def _real_text(v, t):
    if v is None:
        return None
    if math.isnan(v):
        return "NaN"
    if math.isinf(v):
        return "-Infinity" if v < 0 else "Infinity"
    neg = math.copysign(1.0, v) < 0
    if v == 0:
        return "-0.0" if neg else "0.0"
    s = np.format_float_scientific(np.float32(v) if t == pa.float32() else np.float64(v), unique=True, trim="-")
    m, e = s.lstrip("-").split("e")
    return _java_layout(m.replace(".", "").rstrip("0") or "0", int(e) + 1, neg)


REAL_SPECIALS = [0.0, -0.0, 1.0, 1.5, 100.0, 1e7, 9999999.0, 0.001, 0.00099999, 1e-5, 1.0e10, 123456.789, float("inf"), float("-inf"), float("nan"),
                 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, 2.0 ** 52, 2.0 ** -1022, 9007199254740993.0, 0.1, 1 / 3, 4.567, -3.4567, 1e22,
                 1e23, 8.41e21, 1.4e-45, 1.17549435e-38, 3.4028235e38, 16777216.0, 1.2345679, 10.0, 0.00001, 1234567.0, 12345678.0]


def _real_values(n, t, seed):
    rng = np.random.default_rng(seed)
    with np.errstate(all="ignore"):
        if t == pa.float32():
            bits = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32).astype(np.float64)
        else:
            bits = rng.integers(0, 2 ** 64, n, dtype=np.uint64).view(np.float64)
    mid = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 12, n)
    pick = rng.integers(0, 4, n)
    with np.errstate(all="ignore"):
        x = np.where(pick == 0, bits, np.where(pick == 1, mid, np.where(pick == 2, np.round(mid, 2), 2.0 ** rng.integers(-140, 120, n))))
        x[:min(n, len(REAL_SPECIALS))] = REAL_SPECIALS[:n]
        return x.astype(np.float32 if t == pa.float32() else np.float64)


def _real_batch(n, t, seed):
    x = _real_values(n, t, seed)
    m = np.random.default_rng(seed + 1).random(n) < 0.1
    m[:min(n, len(REAL_SPECIALS))] = False
    return pa.RecordBatch.from_arrays([pa.array(x, t, mask=m)], names=["x"])


def _real_exprs(b, batch, cuts=(40, 6, 0)):
    x = b.make_field(batch.schema.field(0))
    return [b.make_expression(b.make_function("castVARCHAR", [x, b.make_literal(c, pa.int64())], STR), pa.field(f"t{c}", STR)) for c in cuts]


@pytest.mark.parametrize("t", [pa.float64(), pa.float32()])
def test_oracle_text_of_a_real_is_the_shortest_digits_in_the_java_layout(t):
    batch = _real_batch(6000, t, seed=3)
    b = gandiva.TreeExprBuilder()
    want = [_real_text(v, t) for v in batch.column(0).to_pylist()]
    for cut, g in zip((40, 6, 0), oracle.project(_real_exprs(b, batch), batch)):
        assert g.to_pylist() == [None if w is None else w[:cut] for w in want], cut
    # the handful the lineage's own test names [gdv_function_stubs_test.cc TestCastVarcharFromFloat / Double, as recalled]
    for v, text in ((4.567, "4.567"), (-3.4567, "-3.4567"), (0.00001, "1.0E-5"), (0.00099999, "9.9999E-4"), (0.0, "0.0"), (10.0, "10.0"), (1.2345679, "1.2345679")):
        assert _real_text(float(np.float32(v)), pa.float32()) == text


@pytest.mark.parametrize("is32", [0, 1])
def test_device_real_text_on_the_host(hostlib, is32):  # noqa: F811
    t = pa.float32() if is32 else pa.float64()
    x = _real_values(120_000, t, seed=11)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for cut in (40, 5):
        out, ln = np.zeros(32 * len(x), np.uint8), np.zeros(len(x), np.int32)
        assert hostlib.host_real_text(is32, p(x), C.c_long(len(x)), C.c_long(cut), p(out), p(ln)) == 0
        got = [bytes(out[32 * i:32 * i + ln[i]]).decode() for i in range(len(x))]
        assert got == [_real_text(float(v), t)[:cut] for v in x], cut
    assert hostlib.host_real_text(is32, p(x), C.c_long(4), C.c_long(-1), p(out), p(ln)) != 0   # n < 0 raises


@pytest.mark.gpu
@pytest.mark.parametrize("t", [pa.float64(), pa.float32()])
@pytest.mark.parametrize("n", [1, 64, 1000, 30_011])
def test_cast_real_to_text_on_the_gpu(n, t):
    batch = _real_batch(n, t, seed=n)
    b = gandiva.TreeExprBuilder()
    exprs = _real_exprs(b, batch)
    got = gandiva.make_projector(batch.schema, exprs, None).evaluate(batch)
    for g, w, c in zip(got, oracle.project(exprs, batch), (40, 6, 0)):
        assert_bit_exact(g, w, f"castVARCHAR(x, {c})")
    assert got[0].to_pylist() == [_real_text(v, t) for v in batch.column(0).to_pylist()]


@pytest.mark.gpu
def test_text_of_a_real_feeds_concat_other_functions_and_selection_mode():
    batch = _real_batch(5000, pa.float64(), seed=2)
    b = gandiva.TreeExprBuilder()
    x = b.make_field(batch.schema.field(0))
    text = b.make_function("castVARCHAR", [x, b.make_literal(40, pa.int64())], STR)
    e = [b.make_expression(b.make_function("concat", [b.make_literal("v=", STR), text], STR), pa.field("c", STR)),
         b.make_expression(b.make_function("upper", [b.make_function("substr", [text, b.make_literal(1, pa.int64()), b.make_literal(4, pa.int64())], STR)], STR),
                           pa.field("u", STR))]
    got = gandiva.make_projector(batch.schema, e, None).evaluate(batch)
    for g, w in zip(got, oracle.project(e, batch)):
        assert_bit_exact(g, w, "castVARCHAR(x, 40) inside concat / upper(substr())")
    cond = b.make_condition(b.make_function("greater_than", [x, b.make_literal(0.0, pa.float64())], pa.bool_()))
    sel = gandiva.make_filter(batch.schema, cond).evaluate(batch)
    got = gandiva.make_projector(batch.schema, e[:1], None, "UINT32").evaluate(batch, sel)
    rows = sel.to_array().to_numpy()
    assert got[0].to_pylist() == [oracle.project(e[:1], batch)[0][int(r)].as_py() for r in rows]
    with pytest.raises(Exception):
        neg = b.make_expression(b.make_function("castVARCHAR", [x, b.make_literal(-1, pa.int64())], STR), pa.field("n", STR))
        gandiva.make_projector(batch.schema, [neg], None).evaluate(batch)


# ------------------------------------------------------------------------------------------------
# round 5: to_date(text, 'pattern'[, suppress_errors]), to_timestamp / to_time over numbers.
#   engine 1 (oracle): glibc's strptime itself (what the lineage calls) on the converted pattern
#   engine 2 (device library, host build and GPU): its own interpreter of the planner's compiled pattern
#   engine 3 (here): Python's datetime.strptime on well-formed texts
import datetime  # noqa: E402
from gandiva_amd import _capi as gandiva_capi  # noqa: E402

DATE_PATTERNS = [("YYYY-MM-DD", "%Y-%m-%d"), ("YYYY-MM-DD HH24:MI:SS", "%Y-%m-%d %H:%M:%S"), ("DD/MM/YYYY", "%d/%m/%Y"), ("MON DD, YYYY", "%b %d, %Y"),
                 ("DD MONTH YYYY", "%d %B %Y"), ("yyyymmdd", "%Y%m%d"), ("DY, DD MON YY HH12:MI:SS AM", "%a, %d %b %y %I:%M:%S %p"), ("YYYY.DDD", "%Y.%j"),
                 ('YYYY-MM-DD"T"HH24:MI', "%Y-%m-%dT%H:%M")]
_DATE_TOKENS = [("YYYY", "Y"), ("HH24", "H"), ("HH12", "I"), ("MONTH", "b"), ("MON", "b"), ("DDD", "j"), ("DAY", "a"), ("YY", "y"), ("MM", "m"), ("DD", "d"),
                ("DY", "a"), ("HH", "I"), ("MI", "M"), ("SS", "S"), ("AM", "p"), ("PM", "p")]


def _compile_date_pattern(p):
    """the planner's CompileDateFormat, restated: one byte per directive, 'L' c for a literal, ' ' for white space"""
    ops, i, quoted = b"", 0, False
    while i < len(p):
        c = p[i]
        if c == '"':
            quoted, i = not quoted, i + 1
        elif quoted:
            ops, i = ops + b"L" + c.encode(), i + 1
        elif c.isspace():
            ops += b" " if not ops.endswith(b" ") else b""
            i += 1
        elif not c.isalpha():
            ops += b"L" + c.encode()
            i += 1
        else:
            tok = next((t for t in _DATE_TOKENS if p[i:i + len(t[0])].upper() == t[0]), None)
            assert tok is not None, p[i:]
            ops += tok[1].encode()
            i += len(tok[0])
    return ops


def _date_texts(pyfmt, n, seed, mutate):
    rng = np.random.default_rng(seed)
    days = rng.integers(-20000, 30000, n)
    secs = rng.integers(0, 86400, n)
    out, want = [], []
    for d, s in zip(days, secs):
        t = datetime.datetime(1970, 1, 1) + datetime.timedelta(days=int(d), seconds=int(s))
        if "%y" in pyfmt:
            t = t.replace(year=1969 + int(d) % 100, day=min(t.day, 28))     # the two-digit window 1969 .. 2068
        text = t.strftime(pyfmt)
        if "%Y" in pyfmt and t.year < 1000:
            text = text.replace(str(t.year), f"{t.year:04d}", 1)
        w = datetime.datetime(t.year, t.month, t.day)   # (a day of the year gives month and day as well: glibc fills them in)
        if mutate and rng.random() < 0.5:
            k = int(rng.integers(0, 5))
            pos = int(rng.integers(0, len(text) + 1))
            if k == 0:
                text = text[:pos]
            elif k == 1:
                text = text[:pos] + "xX9 -:/"[int(rng.integers(0, 7))] + text[pos + 1:]
            elif k == 2:
                text = text[:pos] + " " * int(rng.integers(1, 3)) + text[pos:]
            elif k == 3:
                text = text + " trailing"
            else:
                text = text.upper() if rng.random() < 0.5 else text.lower()
            w = None
        out.append(text)
        want.append(w)
    return out, want


def _to_date_exprs(b, s, pattern, suppress):
    args = [s, b.make_literal(pattern, STR)] + ([b.make_literal(suppress, pa.int32())] if suppress is not None else [])
    return b.make_expression(b.make_function("to_date", args, pa.date64()), pa.field("d", pa.date64()))


@pytest.mark.parametrize("pattern,pyfmt", DATE_PATTERNS)
def test_oracle_to_date_is_strptime_and_agrees_with_pythons_on_well_formed_texts(pattern, pyfmt):
    texts, want = _date_texts(pyfmt, 800, seed=len(pattern), mutate=False)
    batch = pa.RecordBatch.from_arrays([pa.array(texts + [None], STR)], names=["s"])
    b = gandiva.TreeExprBuilder()
    s = b.make_field(batch.schema.field(0))
    got = oracle.project([_to_date_exprs(b, s, pattern, None)], batch)[0]
    assert got.to_pylist() == [w.date() for w in want] + [None], pattern
    # ... and Arrow's own strptime kernel (the primitive the lineage's holder calls; it keeps the time of day: cut to the date here)
    arrow = pc.strptime(batch.column(0), format=pyfmt, unit="s", error_is_null=True).cast(pa.int64())
    assert [None if v is None else (v // 86400) * 86400000 for v in arrow.to_pylist()] == got.cast(pa.int64()).to_pylist(), pattern
    # texts that do not parse: null with suppress_errors = 1, an error without
    bad = pa.RecordBatch.from_arrays([pa.array(["not a date", texts[0], ""], STR)], names=["s"])
    got = oracle.project([_to_date_exprs(b, s, pattern, 1)], bad)[0].to_pylist()
    assert got[0] is None and got[2] is None and got[1] == want[0].date()
    for flag in (None, 0):
        with pytest.raises(Exception):
            oracle.project([_to_date_exprs(b, s, pattern, flag)], bad)


@pytest.mark.parametrize("pattern,pyfmt", DATE_PATTERNS)
def test_device_to_date_interpreter_on_the_host_agrees_with_strptime_on_mutated_texts(hostlib, pattern, pyfmt):  # noqa: F811
    texts, _ = _date_texts(pyfmt, 4000, seed=7 + len(pattern), mutate=True)
    texts += ["", " ", "0", "9999-12-31", "1-1-1", "  2020-1-2", "2020-02-30", "2020-13-01", "69-01-01", "Feb", "Sunday", "12:00:61 PM", "2020.366", "2019.365", "2020.60", "2019.060"]
    arr = pa.array(texts, STR)
    batch = pa.RecordBatch.from_arrays([arr], names=["s"])
    b = gandiva.TreeExprBuilder()
    want = oracle.project([_to_date_exprs(b, b.make_field(batch.schema.field(0)), pattern, 1)], batch)[0]
    off = np.frombuffer(arr.buffers()[1], np.int32)[: len(texts) + 1].copy()
    size = int(off[-1])
    data = np.concatenate([np.frombuffer(arr.buffers()[2], np.uint8)[:size], np.zeros(64, np.uint8)])
    # the planner's own compiler (gdv_compile_date_format) — and this file's restatement of it agrees
    raw, buf, cnt = pattern.encode(), np.zeros(256, np.uint8), C.c_int64(0)
    assert gandiva_capi.lib().gdv_compile_date_format(raw, len(raw), buf.ctypes.data_as(C.c_void_p), 248, C.byref(cnt)) == 0
    assert bytes(buf[:cnt.value]) == _compile_date_pattern(pattern)
    ops = buf[:cnt.value + 8].copy()
    out, ov = np.zeros(len(texts), np.int64), np.zeros(len(texts), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert hostlib.host_parse_date(p(off), p(data), C.c_long(size), C.c_long(len(texts)), p(ops), len(ops) - 8, 1, p(out), p(ov)) == 0
    got = [int(v) if ok else None for v, ok in zip(out, ov)]
    assert got == want.cast(pa.int64()).to_pylist(), pattern
    if any(g is None for g in got):   # without suppress_errors the same rows raise
        assert hostlib.host_parse_date(p(off), p(data), C.c_long(size), C.c_long(len(texts)), p(ops), len(ops) - 8, 0, p(out), p(ov)) == 4


def _seconds_batch(n, seed=1):
    rng = np.random.default_rng(seed)
    k = rng.integers(-2 ** 33, 2 ** 33, n)
    x = rng.standard_normal(n) * 10.0 ** rng.integers(0, 11, n)
    return pa.RecordBatch.from_arrays([pa.array((k % 2 ** 31).astype(np.int32)), pa.array(k, pa.int64(), mask=rng.random(n) < 0.1), pa.array(x.astype(np.float32)),
                                       pa.array(x, pa.float64())], names=["i", "k", "f", "x"])


def _seconds_exprs(b, batch):
    out = []
    for j in range(4):
        fld = b.make_field(batch.schema.field(j))
        out += [b.make_expression(b.make_function("to_timestamp", [fld], pa.timestamp("ms")), pa.field(f"ts{j}", pa.timestamp("ms"))),
                b.make_expression(b.make_function("to_time", [fld], pa.time32("ms")), pa.field(f"tm{j}", pa.time32("ms")))]
    return out


def test_oracle_and_device_seconds_to_millis(hostlib):  # noqa: F811
    batch = _seconds_batch(3000)
    b = gandiva.TreeExprBuilder()
    got = oracle.project(_seconds_exprs(b, batch), batch)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for j, dt in enumerate((np.int32, np.int64, np.float32, np.float64)):
        col = batch.column(j)
        v = np.asarray(col.fill_null(0), dt)
        ms = (v.astype(np.float32) * np.float32(1000.0)).astype(np.float64) if dt == np.float32 else v * 1000.0 if dt == np.float64 else None
        want = (v.astype(np.int64) * 1000) if ms is None else np.trunc(ms).astype(np.int64)
        ok = np.array([x is not None for x in col.to_pylist()])
        ts = np.asarray(got[2 * j].cast(pa.int64()).fill_null(0))
        tm = np.asarray(got[2 * j + 1].cast(pa.int32()).fill_null(0))
        assert (ts[ok] == want[ok]).all() and (tm[ok] == np.fmod(want[ok], 86400000)).all(), dt
        hts, htm = np.zeros(len(v), np.int64), np.zeros(len(v), np.int32)
        hostlib.host_to_timestamp(j, p(v), C.c_long(len(v)), p(hts), p(htm))
        assert (hts[ok] == ts[ok]).all() and (htm[ok] == tm[ok]).all(), dt


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 64, 5000])
def test_to_date_and_seconds_to_millis_on_the_gpu(n):
    b = gandiva.TreeExprBuilder()
    for pattern, pyfmt in DATE_PATTERNS:
        texts, _ = _date_texts(pyfmt, n, seed=n + len(pattern), mutate=True)
        batch = pa.RecordBatch.from_arrays([pa.array(texts, STR, mask=np.random.default_rng(n).random(n) < 0.1)], names=["s"])
        s = b.make_field(batch.schema.field(0))
        e = [_to_date_exprs(b, s, pattern, 1), _to_date_exprs(b, b.make_function("upper", [s], STR), pattern, 1)]
        got = gandiva.make_projector(batch.schema, e, None).evaluate(batch)
        for g, w in zip(got, oracle.project(e, batch)):
            assert_bit_exact(g, w, f"to_date(s, '{pattern}', 1)")
        clean, want = _date_texts(pyfmt, n, seed=n, mutate=False)
        cb = pa.RecordBatch.from_arrays([pa.array(clean, STR)], names=["s"])
        got = gandiva.make_projector(cb.schema, [_to_date_exprs(b, s, pattern, None)], None).evaluate(cb)
        assert got[0].to_pylist() == [w.date() for w in want], pattern
        if any(v is None for v in oracle.project(e[:1], batch)[0].to_pylist()) and batch.column(0).null_count < n:
            with pytest.raises(Exception):
                gandiva.make_projector(batch.schema, [_to_date_exprs(b, s, pattern, 0)], None).evaluate(batch)
    batch = _seconds_batch(n, seed=n)
    e = _seconds_exprs(b, batch)
    for g, w in zip(gandiva.make_projector(batch.schema, e, None).evaluate(batch), oracle.project(e, batch)):
        assert_bit_exact(g, w, "to_timestamp / to_time")


def test_to_date_wants_literal_arguments_and_known_tokens():
    b = gandiva.TreeExprBuilder()
    sch = pa.schema([pa.field("s", STR), pa.field("p", STR)])
    s, p = b.make_field(sch.field(0)), b.make_field(sch.field(1))
    with pytest.raises(Exception, match="literal as the second parameter"):
        gandiva.make_projector(sch, [b.make_expression(b.make_function("to_date", [s, p], pa.date64()), pa.field("d", pa.date64()))], None)


# ------------------------------------------------------------------------------------------------
# round 5: replace / lpad / rpad with arguments that are NOT literals (columns, expressions): engine 1 the oracle (always took
# them per row), engine 2 the device functions (host build, GPU), engine 3 Python's str.replace / ljust / rjust restated per character
def _row_args_batch(n, seed=13):
    rng = np.random.default_rng(seed)
    words = ["ab", "a", "abc", "é", "日本", "x", "", "ba", "aa", "spark", "-", "0"]
    text, frm, to, fill = [], [], [], []
    for _ in range(n):
        k = int(rng.integers(0, 12))
        t = "".join(words[int(rng.integers(0, len(words)))] for _ in range(k))
        text.append(t)
        frm.append(words[int(rng.integers(0, len(words)))] if rng.random() < 0.8 or not t else t[int(rng.integers(0, len(t))):][:3])
        to.append(words[int(rng.integers(0, len(words)))] * int(rng.integers(0, 3)))
        fill.append(words[int(rng.integers(0, len(words)))] + ("é" if rng.random() < 0.2 else ""))
    want = rng.integers(-2, 24, n).astype(np.int32)
    m = lambda: rng.random(n) < 0.08  # noqa: E731
    return pa.RecordBatch.from_arrays([pa.array(text, STR, mask=m()), pa.array(frm, STR, mask=m()), pa.array(to, STR, mask=m()), pa.array(fill, STR, mask=m()),
                                       pa.array(want, pa.int32(), mask=m())], names=["t", "f", "r", "p", "n"])


def _py_replace(t, f, r):
    return t if not t or not f else t.replace(f, r)


def _py_pad(t, n, p, right):
    if not t or n <= 0:
        return ""
    if n <= len(t) or not p:
        return t[:n] if n < len(t) else t
    pad = (p * (n // len(p) + 1))[: n - len(t)]
    return t + pad if right else pad + t


def _row_args_exprs(b, batch):
    t, f, r, p, n = (b.make_field(batch.schema.field(j)) for j in range(5))
    lit = lambda s: b.make_literal(s, STR)  # noqa: E731
    return [("replace(t, f, r)", b.make_function("replace", [t, f, r], STR), lambda v: None if None in (v[0], v[1], v[2]) else _py_replace(v[0], v[1], v[2])),
            ("replace(t, 'a', r)", b.make_function("replace", [t, lit("a"), r], STR), lambda v: None if None in (v[0], v[2]) else _py_replace(v[0], "a", v[2])),
            ("replace(upper(t), f, '_')", b.make_function("replace", [b.make_function("upper", [t], STR), f, lit("_")], STR),
             lambda v: None if None in (v[0], v[1]) else _py_replace("".join(c.upper() if "a" <= c <= "z" else c for c in v[0]), v[1], "_")),
            ("lpad(t, n, p)", b.make_function("lpad", [t, n, p], STR), lambda v: None if None in (v[0], v[3], v[4]) else _py_pad(v[0], v[4], v[3], False)),
            ("rpad(t, n, p)", b.make_function("rpad", [t, n, p], STR), lambda v: None if None in (v[0], v[3], v[4]) else _py_pad(v[0], v[4], v[3], True)),
            ("lpad(t, n)", b.make_function("lpad", [t, n], STR), lambda v: None if None in (v[0], v[4]) else _py_pad(v[0], v[4], " ", False)),
            ("rpad(t, 9, p)", b.make_function("rpad", [t, b.make_literal(9, pa.int32()), p], STR), lambda v: None if None in (v[0], v[3]) else _py_pad(v[0], 9, v[3], True)),
            ("lpad(t, n, 'é-')", b.make_function("lpad", [t, n, lit("é-")], STR), lambda v: None if None in (v[0], v[4]) else _py_pad(v[0], v[4], "é-", False))]


def test_oracle_replace_and_pad_with_per_row_arguments_match_python():
    batch = _row_args_batch(3000)
    rows = list(zip(*[c.to_pylist() for c in batch.columns]))
    b = gandiva.TreeExprBuilder()
    cases = _row_args_exprs(b, batch)
    exprs = [b.make_expression(node, pa.field(f"o{j}", STR)) for j, (_, node, _) in enumerate(cases)]
    for (name, _, py), g in zip(cases, oracle.project(exprs, batch)):
        assert g.to_pylist() == [py(v) for v in rows], name


def test_device_replace_and_pad_with_per_row_arguments_on_the_host(hostlib):  # noqa: F811
    batch = _row_args_batch(4000, seed=17)
    cols = []
    for j in range(4):
        filled = pa.array([v if v is not None else "" for v in batch.column(j).to_pylist()], STR)
        off = np.frombuffer(filled.buffers()[1], np.int32)[: len(filled) + 1].copy()
        size = int(off[-1])
        data = np.concatenate([np.frombuffer(filled.buffers()[2], np.uint8)[:size] if size else np.zeros(0, np.uint8), np.zeros(64, np.uint8)])
        cols.append((off, data, size, filled.to_pylist()))
    want_n = np.asarray(batch.column(4).fill_null(0), np.int32)
    n = batch.num_rows
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    out_off, out = np.zeros(n + 1, np.int32), np.zeros(1 << 22, np.uint8)
    err = C.c_int(0)
    (o0, d0, s0, t), (o1, d1, s1, f), (o2, d2, s2, r), (o3, d3, s3, fill) = cols
    for mp in (0, 1):
        hostlib.host_replace_row.restype = C.c_long
        hostlib.host_replace_row(p(o0), p(d0), C.c_long(s0), p(o1), p(d1), C.c_long(s1), p(o2), p(d2), C.c_long(s2), C.c_long(n), mp, p(out_off), p(out), C.byref(err))
        got = [bytes(out[out_off[i]:out_off[i + 1]]).decode() for i in range(n)]
        up = (lambda s: "".join(c.upper() if "a" <= c <= "z" else c for c in s)) if mp else (lambda s: s)
        assert err.value == 0 and got == [_py_replace(up(a), b_, c) for a, b_, c in zip(t, f, r)], mp
    for right in (0, 1):
        hostlib.host_pad_row(right, p(o0), p(d0), C.c_long(s0), p(want_n), p(o3), p(d3), C.c_long(s3), C.c_long(n), p(out_off), p(out), C.byref(err))
        got = [bytes(out[out_off[i]:out_off[i + 1]]).decode() for i in range(n)]
        assert err.value == 0 and got == [_py_pad(a, int(k), q, bool(right)) for a, k, q in zip(t, want_n, fill)], right


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 64, 1000, 20_011])
def test_replace_and_pad_with_per_row_arguments_on_the_gpu(n):
    batch = _row_args_batch(n, seed=n)
    b = gandiva.TreeExprBuilder()
    cases = _row_args_exprs(b, batch)
    for lo in range(0, len(cases), 3):
        exprs = [b.make_expression(node, pa.field(f"o{j}", STR)) for j, (_, node, _) in enumerate(cases[lo:lo + 3])]
        got = gandiva.make_projector(batch.schema, exprs, None).evaluate(batch)
        for g, w, (name, _, _) in zip(got, oracle.project(exprs, batch), cases[lo:lo + 3]):
            assert_bit_exact(g, w, name)
    # under a selection vector, and a per-row replace feeding another function (two stages)
    t, f, r = (b.make_field(batch.schema.field(j)) for j in range(3))
    e = [b.make_expression(b.make_function("upper", [b.make_function("replace", [t, f, r], STR)], STR), pa.field("u", STR))]
    got = gandiva.make_projector(batch.schema, e, None).evaluate(batch)
    assert_bit_exact(got[0], oracle.project(e, batch)[0], "upper(replace(t, f, r))")
    cond = b.make_condition(b.make_function("isnotnull", [t], pa.bool_()))
    sel = gandiva.make_filter(batch.schema, cond).evaluate(batch)
    e2 = [b.make_expression(cases[0][1], pa.field("o", STR)), b.make_expression(cases[3][1], pa.field("q", STR))]
    got = gandiva.make_projector(batch.schema, e2, None, "UINT32").evaluate(batch, sel)
    rows = sel.to_array().to_numpy()
    for g, w in zip(got, oracle.project(e2, batch)):
        assert g.to_pylist() == [w[int(i)].as_py() for i in rows]


# ------------------------------------------------------------------------------------------------
# round 5, late: regexp_like / regexp_matches beyond the literal subset.
#   engine 1 (oracle): Thompson program over code points, thread list
#   engine 2 (device library, host build and GPU): byte-level position automaton compiled by the planner (gdv_compile_regex)
#   engine 3 (here): Python's re (ASCII classes; '$' written as \Z: Python's own '$' also matches before a final newline)
REGEX_PATTERNS = [r"\d+", r"^a.*3$", r"a.b", r"^$", r"[^a-z]+", r"(foo|bar)\.ba?r", r"x(yz)+y", r"é{2}", r"^\d{4}-\d{2}-\d{2}$", r"a{2,3}", r"日.語",
                  r"^(ab|abc)$", r"\w+\s\w+", r"[\d.]+$", r"z*", r"sp.rk\d?", r"^[A-Z][a-z]+$", r"(a|b)*c", r"\S+@\S+\.com", r"[^\d\s]{3,}", r"^.{3}$",
                  r"colou?r", r"\W", r"^\D*$", r"(?:ab){2,}", r"a+?b", r"[a-c-]+x", r"[]x]+y", r"\x41\x2e", r"^(\d+|[a-f]+)(\.\d*)?$", r".\n.", r"é+$",
                  r"(?i)spark", r"(?i)^[a-c]+\d?$", r"(?i)colou?r|HELLO", r"(?i)[^a]b", r"[é語x]+", r"^[日é][本é]", r"(?i)\W[A-Z]",
                  r"\bab\b", r"\Bb", r"^a|c$", r"(^|-)a", r"a(b|$)", r"\Aab", r"r\z", r"(?s)a.b", r"(?is)A.B", r"(?P<w>[a-z]+)\.(?P<x>b)", r"[[:alpha:]]+\d",
                  r"^[[:upper:]][[:lower:]]+$", r"[[:punct:][:space:]]{2}", r"\b\d+\b", r"x\b.", r"(\b|z)z", r"^$|^-$", r"é\b", r"\bé", r"^\bx", r"\B$", r"^\b\w+\b$", r"\B", r".\B", r"\Bx?", r"(?i)[^a]?\S\B",
                  # round 6 (advisor): \s / \S are Perl's (no vertical tab; [[:space:]] has it); (?i) folds U+212A onto k and U+017F onto s
                  r"\s", r"^\S+$", r"[[:space:]]", r"[\s]x?$", r"(?i)k", r"(?i)s", r"(?i)^[^k]$", r"(?i)^[^s]+$", r"(?i)\w", r"(?i)^\W$", r"(?i)spar[k]", r"(?i)[j-l]\b", r"k", r"[^k]"]
REGEX_WORDS = ["ab", "abc", "a", "3", "2021-03-04", "foo.bar", "bar.br", "xyzyzy", "é", "éé", "日本語", "日x語", " ", "\n", "spark", "sperk7", "Color", "colour",
               "x@y.com", "A.", "-", "]", "c", "zz", "Hello", "0.5", "ff.", "aab", "b-a-x", "]]xy", "\t", "c日x語a", "\x0b", "\u212a", "\u017f", "spar\u212a", "\u017fpark"]


def _regex_texts(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        k = int(rng.integers(0, 4))
        out.append("".join(REGEX_WORDS[int(rng.integers(0, len(REGEX_WORDS)))] for _ in range(k)))
    return out


def _py_regex(p):
    """the pattern in Python's dialect: '$' and \\z -> \\Z (Python's own '$' also matches before a final newline), (?P<n>..) as is;
    None where Python has no equivalent (POSIX classes) — RE2 alone is the reference there"""
    if "[:" in p:
        return None
    out, i, in_class = "", 0, False
    while i < len(p):
        c = p[i]
        if c == "\\" and i + 1 < len(p):
            out += "\\Z" if p[i + 1] == "z" and not in_class else p[i:i + 2]
            i += 2
            continue
        if in_class:
            in_class = c != "]" or out.endswith("[") or out.endswith("[^")
        elif c == "[":
            in_class = True
        elif c == "$":
            out, i = out + "\\Z", i + 1
            continue
        out += c
        i += 1
    return re.compile(out, re.ASCII)


def _regex_want(p, texts):
    """RE2 itself (the lineage's engine, as linked into this image's libarrow: PartialMatch with default options), cross-checked
    against Python's re where Python can express the pattern"""
    want = pc.match_substring_regex(pa.array(texts, STR), p).to_pylist()
    rx = _py_regex(p)
    if rx is not None:
        # (RE2 is the reference where the two differ on \\B: Python's does not match in an empty text; RE2 evaluates assertions between
        # BYTES and may begin a match inside a multi-byte character, where the gap is "not a word boundary")
        # (round 6: Python's \s holds the vertical tab, RE2's does not; under re.ASCII Python's (?i) does not fold U+212A / U+017F, RE2's does)
        keep = [i for i, t in enumerate(texts) if ("\\B" not in p or (t and t.isascii())) and not any(c in t for c in "\x0b\u212a\u017f")]
        assert [want[i] for i in keep] == [rx.search(texts[i]) is not None for i in keep], f"RE2 and Python's re disagree on {p!r}"
    return want


def _regex_expr(b, s, p, name="regexp_like"):
    return b.make_expression(b.make_function(name, [s, b.make_literal(p, STR)], pa.bool_()), pa.field("m", pa.bool_()))


def test_oracle_regular_expressions_match_pythons_re():
    texts = _regex_texts(1500, seed=4) + REGEX_WORDS
    batch = pa.RecordBatch.from_arrays([pa.array(texts + [None], STR)], names=["s"])
    b = gandiva.TreeExprBuilder()
    s = b.make_field(batch.schema.field(0))
    for p in REGEX_PATTERNS:
        got = oracle.project([_regex_expr(b, s, p)], batch)[0].to_pylist()
        assert got == _regex_want(p, texts) + [None], p


def test_device_regular_expressions_on_the_host_match_pythons_re(hostlib):  # noqa: F811
    texts = _regex_texts(4000, seed=6) + REGEX_WORDS
    arr = pa.array(texts, STR)
    off = np.frombuffer(arr.buffers()[1], np.int32)[: len(texts) + 1].copy()
    size = int(off[-1])
    data = np.concatenate([np.frombuffer(arr.buffers()[2], np.uint8)[:size], np.zeros(64, np.uint8)])
    lib = gandiva._capi.lib() if hasattr(gandiva, "_capi") else __import__("gandiva_amd._capi", fromlist=["lib"]).lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for pat in REGEX_PATTERNS:
        table = np.zeros(6352 + 8, np.uint8)
        raw = pat.encode()
        assert lib.gdv_compile_regex(raw, C.c_int64(len(raw)), p(table)) == 0, pat
        for mp in (0, 1):
            out = np.zeros(len(texts), np.uint8)
            hostlib.host_regex_search(p(off), p(data), C.c_long(size), C.c_long(len(texts)), p(table), mp, p(out))
            up = (lambda t: "".join(c.upper() if "a" <= c <= "z" else c for c in t)) if mp else (lambda t: t)
            assert out.astype(bool).tolist() == _regex_want(pat, [up(t) for t in texts]), (pat, mp)


def test_regular_expressions_outside_the_syntax_are_refused_with_a_reason():
    lib = __import__("gandiva_amd._capi", fromlist=["lib", "last_error"])
    table = np.zeros(6360, np.uint8)
    for pat, why in ((r"(a)\1", "escape"), (r"\pL", "escape"), (r"a(?i)b", "group flags"),
                     (r"[^é]", "non-ASCII"), (r"[à-ÿ]", "non-ASCII"), (r"(?i)é", "non-ASCII"), (r"(?m)^a", "group flags"), (r"(ab", "unmatched"),
                     (r"a{3,2}", "n < m"), (r"(abcdefgh){9}", "63"), ("a." * 20000, "longer than"), ("(" * 3000, "nested deeper"), ("a." * 40, "63"),
                     ("()" * 600, "atoms"), ("a" + "*" * 600, "atoms"), ("^" * 600, "atoms"), (r"a*+", "possessive"), (r"(?=x)", "look-around"), (r"[[:foo:]]", "POSIX")):
        raw = pat.encode()
        assert lib.lib().gdv_compile_regex(raw, C.c_int64(len(raw)), table.ctypes.data_as(C.c_void_p)) != 0, pat
        assert why in lib.last_error(), (pat, lib.last_error())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 64, 3000])
def test_regular_expressions_on_the_gpu(n):
    texts = (_regex_texts(n, seed=n) + REGEX_WORDS)[:max(n, 1)]
    batch = pa.RecordBatch.from_arrays([pa.array(texts, STR, mask=np.random.default_rng(n).random(len(texts)) < 0.1)], names=["s"])
    b = gandiva.TreeExprBuilder()
    s = b.make_field(batch.schema.field(0))
    for lo in range(0, len(REGEX_PATTERNS), 8):
        e = [_regex_expr(b, s, p, "regexp_like" if j % 2 else "regexp_matches") for j, p in enumerate(REGEX_PATTERNS[lo:lo + 8])]
        got = gandiva.make_projector(batch.schema, e, None).evaluate(batch)
        for g, w, p in zip(got, oracle.project(e, batch), REGEX_PATTERNS[lo:lo + 8]):
            assert_bit_exact(g, w, p)
    # as a filter condition, and over upper(s)
    cond = b.make_condition(b.make_function("regexp_like", [b.make_function("upper", [s], STR), b.make_literal(r"^[A-Z]+\d*$", STR)], pa.bool_()))
    sel = gandiva.make_filter(batch.schema, cond).evaluate(batch).to_array().to_pylist()
    rx = re.compile(r"^[A-Z]+\d*\Z", re.ASCII)
    assert sel == [i for i, t in enumerate(batch.column(0).to_pylist()) if t is not None and rx.search(t.upper() if t.isascii() else "".join(c.upper() if "a" <= c <= "z" else c for c in t))]


def test_random_patterns_three_engines_agree(hostlib):  # noqa: F811
    """patterns drawn from a small grammar (atoms x quantifiers, anchors, a top-level alternation): the oracle's thread list, the
    device library's position automaton (host build) and Python's re give the same answer on every text"""
    lib = __import__("gandiva_amd._capi", fromlist=["lib"]).lib()
    rng = np.random.default_rng(3)
    atoms = ["a", "b", "c", ".", "\\d", "\\w", "\\s", "[ab]", "[^a]", "[a-c]", "é", "x", "\\.", "(ab|c)", "(a|b)", "(?:bc)", "\\b", "\\B", "(^|-)", "($|b)"]
    quants = ["", "", "", "*", "+", "?", "{2}", "{1,3}", "{2,}", "*?"]
    texts = _regex_texts(500, seed=9) + REGEX_WORDS + ["abcabc", "aab", "ccc", "a.c", "bcbc", "é.é"]
    arr = pa.array(texts, STR)
    off = np.frombuffer(arr.buffers()[1], np.int32)[: len(texts) + 1].copy()
    size = int(off[-1])
    data = np.concatenate([np.frombuffer(arr.buffers()[2], np.uint8)[:size], np.zeros(64, np.uint8)])
    batch = pa.RecordBatch.from_arrays([arr], names=["s"])
    b = gandiva.TreeExprBuilder()
    s = b.make_field(batch.schema.field(0))
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    tried = 0
    for _ in range(160):
        k = int(rng.integers(1, 5))
        pick = [atoms[int(rng.integers(0, len(atoms)))] for _ in range(k)]
        pat = "".join(a + ("" if a in ("\\b", "\\B") else quants[int(rng.integers(0, len(quants)))]) for a in pick)   # (Python refuses a quantified \b)
        pat = ("^" if rng.random() < 0.3 else "") + pat + ("$" if rng.random() < 0.3 else "")
        if rng.random() < 0.2:
            pat = "(" + pat.strip("^$") + ")|zz"
        if "é" not in pat and rng.random() < 0.25:
            pat = "(?i)" + pat
        raw, table = pat.encode(), np.zeros(6360, np.uint8)
        if lib.gdv_compile_regex(raw, C.c_int64(len(raw)), p(table)) != 0:
            continue   # (more than 63 positions)
        tried += 1
        out = np.zeros(len(texts), np.uint8)
        hostlib.host_regex_search(p(off), p(data), C.c_long(size), C.c_long(len(texts)), p(table), 0, p(out))
        want = _regex_want(pat, texts)
        assert out.astype(bool).tolist() == want, pat
        assert oracle.project([_regex_expr(b, s, pat)], batch)[0].to_pylist() == want, pat
    assert tried > 100


def test_random_to_date_patterns_device_interpreter_agrees_with_strptime(hostlib):  # noqa: F811
    """token sequences drawn at random (a day of the year with and without a year, names, 12-hour clocks, quoted text): the
    interpreter of the device library follows glibc's strptime — including when glibc turns a day of the year into month
    and day (only if a year / month / day directive asked for a calendar date) — on rendered and mutated texts"""
    rng = np.random.default_rng(31)
    tokens = [("YYYY", "%Y"), ("YY", "%y"), ("MM", "%m"), ("MON", "%b"), ("MONTH", "%B"), ("DD", "%d"), ("DDD", "%j"), ("DY", "%a"), ("DAY", "%A"),
              ("HH24", "%H"), ("HH", "%I"), ("HH12", "%I"), ("MI", "%M"), ("SS", "%S"), ("AM", "%p"), ("PM", "%p")]
    seps = ["-", "/", " ", ":", ", ", ".", "T", " - ", ""]
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    b = gandiva.TreeExprBuilder()
    tried = 0
    for _ in range(120):
        k = int(rng.integers(1, 6))
        pattern = pyfmt = ""
        for j in range(k):
            sql, py = tokens[int(rng.integers(0, len(tokens)))]
            sep = seps[int(rng.integers(0, len(seps)))] if j < k - 1 else ""
            pattern += sql + ('"T"' if sep == "T" else sep)
            pyfmt += py + sep
        texts = []
        for _ in range(60):
            t = datetime.datetime(1970, 1, 1) + datetime.timedelta(days=int(rng.integers(-20000, 30000)), seconds=int(rng.integers(0, 86400)))
            s = t.strftime(pyfmt)
            if rng.random() < 0.3:
                pos, kind = int(rng.integers(0, len(s) + 1)), int(rng.integers(0, 4))
                s = s[:pos] if kind == 0 else s[:pos] + "xX9 -:/"[int(rng.integers(0, 7))] + s[pos + 1:] if kind == 1 else s[:pos] + " " + s[pos:] if kind == 2 else s.upper()
            texts.append(s)
        raw, buf, cnt = pattern.encode(), np.zeros(256, np.uint8), C.c_int64(0)
        if gandiva_capi.lib().gdv_compile_date_format(raw, len(raw), p(buf), 248, C.byref(cnt)) != 0:
            continue      # (two tokens ran together into letters that are no token: both sides refuse)
        arr = pa.array(texts, STR)
        batch = pa.RecordBatch.from_arrays([arr], names=["s"])
        want = oracle.project([_to_date_exprs(b, b.make_field(batch.schema.field(0)), pattern, 1)], batch)[0].cast(pa.int64()).to_pylist()
        off = np.frombuffer(arr.buffers()[1], np.int32)[: len(texts) + 1].copy()
        size = int(off[-1])
        data = np.concatenate([np.frombuffer(arr.buffers()[2], np.uint8)[:size], np.zeros(64, np.uint8)])
        out, ov = np.zeros(len(texts), np.int64), np.zeros(len(texts), np.uint8)
        hostlib.host_parse_date(p(off), p(data), C.c_long(size), C.c_long(len(texts)), p(buf), C.c_int(cnt.value), 1, p(out), p(ov))
        assert [int(v) if ok else None for v, ok in zip(out, ov)] == want, pattern
        tried += 1
    assert tried > 100
