"""Text <-> date / time without a GPU: castDATE / castTIMESTAMP / castTIME of text, castVARCHAR of date32 / date64 /
timestamp / time32, castTIME(timestamp) and castTIMESTAMP(date32).

PARITY STATUS: recollection (PARITY.md, text <-> date / time).  The expected values come from the plain-Python
restatement below (the oracle does not know these functions); the restatement itself is checked against
datetime.fromisoformat, pyarrow's string -> timestamp cast and numpy's datetime64 text where their rules coincide.  This
file checks
  * the registry, through the Python mirror and through libgandiva.so's ExpressionRegistry (the rebuilt pyarrow.gandiva);
  * plans that use them, cross-compiled for gfx950 by hipRTC, and which copy entry their kernels take;
  * the product's device functions and the copy entry of castVARCHAR plans, compiled for the host
    (tests/host_devlib/host_temporal_text.cc), against the restatement on random rows."""
import ctypes as C
import datetime as dt
import os
import re
import subprocess

import numpy as np
import pyarrow as pa
import pytest

import gandiva_amd as gandiva
from gandiva_amd import _capi, gandiva as gg

HERE = os.path.dirname(os.path.abspath(__file__))
STR, I32, I64 = pa.string(), pa.int32(), pa.int64()
TS, D64, D32, T32 = pa.timestamp("ms"), pa.date64(), pa.date32(), pa.time32("ms")
DAY = 86_400_000
EPOCH_ORDINAL = dt.date(1970, 1, 1).toordinal()


class RowError(Exception):
    """the row raises "invalid argument" (an execution error of the whole evaluation)"""


# ------------------------------------------------------------------ the restatement (bytes in, value or RowError out)

def days_of(y, m, d):
    """days since 1970-01-01 of y-m-d, y in 0..9999 (the Gregorian calendar repeats every 400 years = 146097 days)"""
    if not 0 <= y <= 9999:
        raise RowError("year")
    q, r = divmod(y - 1, 400)
    try:
        return dt.date(r + 1, m, d).toordinal() - EPOCH_ORDINAL + 146097 * q
    except ValueError:
        raise RowError("no such date") from None


def civil(days):
    """(year, month, day) of a day number, any year"""
    q, r = divmod(days, 146097)
    c = dt.date.fromordinal(r + EPOCH_ORDINAL)
    return c.year + 400 * q, c.month, c.day


def expand_year(digits):
    y = int(digits or b"0")
    if y < 100 and len(digits) < 4:
        return 2000 + y if y < 70 else 1900 + y
    return y


DATE_RE = re.compile(rb"([0-9]*)(?:[^0-9]([0-9]*)(?:[^0-9]([0-9]*))?)?", re.S)


def cast_date(t):
    """castDATE(text) -> date64 milliseconds: three digit runs, each ended by one non-digit byte (or the text's end)"""
    y, m, d = DATE_RE.match(t).groups()
    if d is None:
        raise RowError("fewer than three fields")
    if max(len(y), len(m), len(d)) > 9:
        raise RowError("field longer than 9 digits")
    return days_of(expand_year(y), int(m or b"0"), int(d or b"0")) * DAY


CLOCK = rb"([0-9]{1,2}):([0-9]{1,2})(?::([0-9]{1,2})(?:\.([0-9]{1,3}))?)?"
TS_RE = re.compile(rb"([0-9]{1,4})-([0-9]{1,2})-([0-9]{1,2})(?:[ T]" + CLOCK + rb")?(?: ?([+-])([0-9]{2})(?::?([0-9]{2}))?)?")
TIME_RE = re.compile(CLOCK)


def _clock(h, mi, s, f):
    h, mi, s = int(h), int(mi), int(s or b"0")
    if h > 23 or mi > 59 or s > 59:
        raise RowError("time field out of range")
    return ((h * 60 + mi) * 60 + s) * 1000 + (int(f.ljust(3, b"0")) if f else 0)


def cast_timestamp(t):
    g = TS_RE.fullmatch(t)
    if g is None:
        raise RowError("not a timestamp")
    y, m, d, h, mi, s, f, sign, oh, om = g.groups()
    ms = days_of(expand_year(y), int(m), int(d)) * DAY + (_clock(h, mi, s, f) if h is not None else 0)
    if sign is not None:
        oh, om = int(oh), int(om or b"0")
        if oh > 23 or om > 59:
            raise RowError("offset out of range")
        ms -= (1 if sign == b"+" else -1) * (oh * 60 + om) * 60_000
    return ms


def cast_time(t):
    g = TIME_RE.fullmatch(t)
    if g is None:
        raise RowError("not a time")
    return _clock(*g.groups())


def text_of(v, kind):
    """the full text of castVARCHAR: kind 0 timestamp, 1 date (v in milliseconds), 2 time"""
    days, t = divmod(v, DAY)
    clock = f"{t // 3_600_000:02d}:{t // 60_000 % 60:02d}:{t // 1000 % 60:02d}.{t % 1000:03d}"
    if kind == 2:
        return clock.encode()
    y, m, d = civil(days)
    text = f"{'-' if y < 0 else ''}{abs(y):04d}-{m:02d}-{d:02d}"
    return (text if kind == 1 else text + " " + clock).encode()


def cast_varchar(v, kind, n):
    if n < 0:
        raise RowError("negative length")
    return text_of(v, kind)[:min(n, (23, 10, 12)[kind])]


def ascii_upper(t):
    return bytes(c - 32 if 0x61 <= c <= 0x7A else c for c in t)


def ascii_lower(t):
    return bytes(c + 32 if 0x41 <= c <= 0x5A else c for c in t)


def _mapped(t, m):
    return ascii_upper(t) if m == 1 else ascii_lower(t) if m == 2 else t


def _want(f, *args):
    try:
        return f(*args), 0
    except RowError:
        return None, 4


# ------------------------------------------------------------------ 1. the restatement against other engines

def test_restatement_examples():
    D = lambda y, m, d: days_of(y, m, d) * DAY  # noqa: E731
    assert cast_date(b"2024-01-15 10:20:30") == D(2024, 1, 15)
    assert cast_date(b"2024/1/5") == D(2024, 1, 5)
    assert cast_date(b"24-2-29") == D(2024, 2, 29) and cast_date(b"69.12.31") == D(2069, 12, 31)
    assert cast_date(b"70-1-1") == 0 and cast_date(b"0070-1-1") == D(70, 1, 1)
    for bad in (b"2024-01", b"2023-02-29", b"10000-01-01", b"2024-01-0000000015", b"", b"2024-13-01", b"2024-01-"):
        with pytest.raises(RowError):
            cast_date(bad)
    assert cast_timestamp(b"2024-01-15T10:20:30.5+05:30") == D(2024, 1, 15) + (10 * 3600 + 20 * 60 + 30) * 1000 + 500 - 19_800_000
    assert cast_timestamp(b"1969-12-31 23:59:59.999") == -1
    assert cast_timestamp(b"2024-01-15 -0100") == D(2024, 1, 15) + 3_600_000
    for bad in (b"2024-01-15 10:20:30.1234", b"2024-01-15 24:00", b"2024-01-15 10:20 UTC", b"2024-01-15 ", b"2024-01-15+5"):
        with pytest.raises(RowError):
            cast_timestamp(bad)
    assert cast_time(b"1:2:3.04") == 3_723_040 and cast_time(b"23:59") == 86_340_000
    assert cast_varchar(-1, 0, 100) == b"1969-12-31 23:59:59.999" and cast_varchar(-1, 2, 5) == b"23:59"
    assert text_of(days_of(0, 1, 1) * DAY - DAY, 1) == b"-0001-12-31" and cast_varchar(-62_167_305_600_000, 1, 100) == b"-0001-12-3"
    assert cast_varchar(days_of(9999, 12, 31) * DAY + 2 * DAY, 0, 100) == b"10000-01-02 00:00:00.00"


def _ms_of_datetime(x):
    delta = x.replace(tzinfo=None) - dt.datetime(1970, 1, 1) - (x.utcoffset() or dt.timedelta(0))
    return delta.days * DAY + delta.seconds * 1000 + delta.microseconds // 1000


def test_restatement_against_fromisoformat_and_arrow():
    rng = np.random.default_rng(11)
    lo, hi = days_of(1, 1, 1) * DAY, days_of(9999, 12, 31) * DAY + DAY
    vals = [int(v) for v in rng.integers(lo, hi, 20_000)] + [lo, hi - 1, 0, -1, 951_782_400_000]
    texts = [text_of(v, 0) for v in vals]
    for v, t in zip(vals, texts):
        assert _ms_of_datetime(dt.datetime.fromisoformat(t.decode())) == v == cast_timestamp(t)
        assert dt.date.fromisoformat(t[:10].decode()).toordinal() - EPOCH_ORDINAL == v // DAY == cast_date(t) // DAY
    # offsets: an aware datetime, converted to UTC
    for v, t in zip(vals[:2000], texts[:2000]):
        off = int(rng.integers(-23 * 60, 24 * 60))
        sign, a = ("+" if off >= 0 else "-"), abs(off)
        z = f"{sign}{a // 60:02d}:{a % 60:02d}".encode()
        want = _ms_of_datetime(dt.datetime.fromisoformat((t + z).decode()))
        assert cast_timestamp(t + z) == want == v - off * 60_000
    arrow = pa.array([t.decode() for t in texts] + [t[:10].decode() for t in texts]).cast(TS)
    assert arrow.cast(I64).to_pylist() == [cast_timestamp(t) for t in texts] + [cast_timestamp(t[:10]) for t in texts]


def test_formatting_against_numpy():
    rng = np.random.default_rng(12)
    lo, hi = days_of(0, 1, 1) * DAY, days_of(9999, 12, 31) * DAY + DAY
    vals = np.concatenate([rng.integers(lo, hi, 50_000), rng.integers(-10 * DAY, 10 * DAY, 5_000), [lo, hi - 1, -1, 0]])
    want = [s.replace("T", " ").encode() for s in np.datetime_as_string(vals.astype("datetime64[ms]"), unit="ms")]
    assert [text_of(int(v), 0) for v in vals] == want
    assert [text_of(int(v), 1) for v in vals] == [w[:10] for w in want]
    assert [text_of(int(v), 2) for v in vals] == [w[11:] for w in want]


# ------------------------------------------------------------------ 2. registry

WANT = [("castDATE", [STR], D64), ("castTIMESTAMP", [STR], TS), ("castTIME", [STR], T32),
        ("castVARCHAR", [D64, I64], STR), ("castVARCHAR", [D32, I64], STR), ("castVARCHAR", [TS, I64], STR),
        ("castVARCHAR", [T32, I64], STR), ("castTIME", [TS], T32), ("castTIMESTAMP", [D32], TS)]


def _signatures(sigs):
    return {(s.name(), tuple(s.param_types())): s.return_type() for s in sigs}


def test_registry_lists_the_temporal_casts():
    sigs = _signatures(gandiva.get_registered_function_signatures())
    for name, params, ret in WANT:
        assert sigs.get((name, tuple(params))) == ret, (name, params)


def test_registry_of_the_rebuilt_pyarrow_gandiva_lists_the_temporal_casts():
    from gandiva_amd import pyarrow_gandiva
    sigs = _signatures(pyarrow_gandiva.load().get_registered_function_signatures())
    for name, params, ret in WANT:
        assert sigs.get((name, tuple(params))) == ret, (name, params)


def test_other_timestamp_units_fail_at_make():
    sch = pa.schema([pa.field("t", pa.timestamp("us"))])
    b = gandiva.TreeExprBuilder()
    e = b.make_expression(b.make_function("castVARCHAR", [b.make_field(sch.field(0)), b.make_literal(23, I64)], STR),
                          pa.field("o", STR))
    with pytest.raises(Exception):
        gandiva.make_projector(sch, [e], pa.default_memory_pool())


# ------------------------------------------------------------------ 3. cross-compile (hipRTC, no GPU)

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


SCH = pa.schema([pa.field("s", STR), pa.field("ts", TS), pa.field("d64", D64), pa.field("d32", D32),
                 pa.field("t32", T32), pa.field("n", I64)])


class T:
    def __init__(self):
        self.b = gandiva.TreeExprBuilder()
        self.f = {f.name: self.b.make_field(f) for f in SCH}

    def fn(self, name, args, t=STR):
        return self.b.make_function(name, args, t)

    def lit(self, v, t=I64):
        return self.b.make_literal(v, t)

    def expr(self, node, name, t=STR):
        return self.b.make_expression(node, pa.field(name, t))


PARSERS = ("castDATE_utf8", "castTIMESTAMP_utf8", "castTIME_utf8")
FORMATTERS = ("castVARCHAR_timestamp_int64", "castVARCHAR_date64_int64", "castVARCHAR_date32_int64",
              "castVARCHAR_time32_int64")


def test_projection_with_every_new_function_cross_compiles(monkeypatch, tmp_path):
    t = T()
    f = t.f
    exprs = [t.expr(t.fn("castDATE", [f["s"]], D64), "a", D64), t.expr(t.fn("castTIMESTAMP", [f["s"]], TS), "b", TS),
             t.expr(t.fn("castTIME", [f["s"]], T32), "c", T32), t.expr(t.fn("castTIME", [f["ts"]], T32), "d", T32),
             t.expr(t.fn("castTIMESTAMP", [f["d32"]], TS), "e", TS),
             t.expr(t.fn("castVARCHAR", [f["ts"], t.lit(23)]), "g"), t.expr(t.fn("castVARCHAR", [f["d64"], f["n"]]), "h"),
             t.expr(t.fn("castVARCHAR", [f["d32"], t.lit(10)]), "i"), t.expr(t.fn("castVARCHAR", [f["t32"], t.lit(12)]), "j")]
    texts = _precompile(monkeypatch, tmp_path, SCH, exprs=exprs)
    for sym in PARSERS + FORMATTERS + ("castTIME_timestamp", "castTIMESTAMP_date32"):
        assert any(sym in x for x in texts), sym
    # the kernels that copy var-len outputs take the date / time copy entry, and only it
    main = [x for x in texts if "GDV_STAGE_COPY" in x]
    assert main and all(re.search(r"GDV_STAGE_COPY\(dst, v\) gdv_stage_copy(_mirh?)?_dt\(", x) for x in main)
    assert not any("_ext" in x for x in texts)


def test_plans_without_the_new_casts_keep_their_copy_entry(monkeypatch, tmp_path):
    t = T()
    s, n = t.f["s"], t.f["n"]
    plain = [t.expr(t.fn("upper", [s]), "u"), t.expr(t.fn("castVARCHAR", [n, t.lit(20)]), "v")]
    for x in _precompile(monkeypatch, tmp_path / "plain", SCH, exprs=plain):
        assert "_dt" not in x and "_ext" not in x and "GDV_MAP_DATETIME" not in x.split("gdv_device_lib")[0]
    tr = [t.expr(t.fn("translate", [s, t.lit("ab", STR), t.lit("x", STR)]), "w")]
    texts = _precompile(monkeypatch, tmp_path / "tr", SCH, exprs=tr)
    assert any("gdv_stage_copy_ext(" in x or "gdv_stage_copy_mir_ext(" in x for x in texts)
    assert not any("_ext_dt" in x or "_dt(" in x for x in texts)


def test_translate_and_castvarchar_in_one_plan_take_the_combined_entry(monkeypatch, tmp_path):
    t = T()
    exprs = [t.expr(t.fn("translate", [t.f["s"], t.lit("ab", STR), t.lit("x", STR)]), "w"),
             t.expr(t.fn("castVARCHAR", [t.f["ts"], t.lit(23)]), "g")]
    texts = _precompile(monkeypatch, tmp_path, SCH, exprs=exprs)
    assert any(re.search(r"gdv_stage_copy(_mirh?)?_ext_dt\(", x) for x in texts)


def test_filter_on_castdate_cross_compiles(monkeypatch, tmp_path):
    t = T()
    cond = t.b.make_condition(t.fn("greater_than", [t.fn("castDATE", [t.f["s"]], D64), t.lit(19_000 * DAY, D64)], pa.bool_()))
    assert any("castDATE_utf8" in x for x in _precompile(monkeypatch, tmp_path, SCH, cond=cond))


def test_like_over_castvarchar_runs_staged_and_cross_compiles(monkeypatch, tmp_path):
    t = T()
    e = t.fn("like", [t.fn("castVARCHAR", [t.f["ts"], t.lit(23)]), t.lit("2024-%", STR)], pa.bool_())
    texts = _precompile(monkeypatch, tmp_path, SCH, exprs=[t.expr(e, "m", pa.bool_())])
    stage1 = [x for x in texts if "castVARCHAR_timestamp_int64" in x]
    stage2 = [x for x in texts if "gdv_like_prefix" in x]
    assert stage1 and stage2 and not set(map(id, stage1)) & set(map(id, stage2))


def test_castvarchar_prepass_reads_no_byte(monkeypatch, tmp_path):
    """castVARCHAR of dates and times is byte-free: a plan restricted to byte-free pre-passes (GDV_WAVE_BYTEFREE_ONLY) keeps
    its wave shape, and no pre-pass holds a parser"""
    t = T()
    exprs = [t.expr(t.fn("castVARCHAR", [t.f["ts"], t.lit(23)]), "g"), t.expr(t.f["s"], "s")]
    monkeypatch.setenv("GDV_WAVE_BYTEFREE_ONLY", "1")
    pre = [x for x in _precompile(monkeypatch, tmp_path, SCH, exprs=exprs) if "// pre-pass:" in x]
    assert len(pre) == 1 and not any(p in pre[0] for p in PARSERS)


# ------------------------------------------------------------------ 4. the device functions on the host

SRC = os.path.join(HERE, "host_devlib", "host_temporal_text.cc")
LIB = os.path.join(HERE, "host_devlib", "libhost_temporal_text.so")


@pytest.fixture(scope="module")
def dtlib():
    hdr = os.path.join(HERE, "..", "gandiva_amd", "csrc", "gdv_device_lib.hpp")
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off",
                               "-Wno-unused-function", "-Wno-unused-variable", SRC, "-o", LIB])
    return C.CDLL(LIB)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _parse(lib, fn, texts, inbuf, text_map=0):
    n = len(texts)
    off = np.zeros(n + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(x) for x in texts])
    data = np.frombuffer(b"".join(texts) + b"\0" * 24, dtype=np.uint8).copy()
    out = np.zeros(n, dtype=np.int64)
    err = np.zeros(n, dtype=np.uint8)
    lib.host_temporal_parse(fn, _p(off), _p(data), C.c_long(int(off[-1])), C.c_long(n), inbuf, text_map, _p(out), _p(err))
    return out, err


def _format(lib, kind, vals, ns):
    n = len(vals)
    v = np.asarray(vals, dtype=np.int64)
    k = np.asarray(ns, dtype=np.int64)
    out_off = np.zeros(n + 1, dtype=np.int32)
    out = np.zeros(24 * n + 64, dtype=np.uint8)
    err = np.zeros(n, dtype=np.uint8)
    lib.host_temporal_format.restype = C.c_long
    total = lib.host_temporal_format(kind, _p(v), _p(k), C.c_long(n), _p(out_off), _p(out), _p(err))
    assert total <= 23 * n
    raw = out.tobytes()
    return [raw[out_off[i]:out_off[i + 1]] for i in range(n)], err


def _check(got, err, want, what):
    bad = [i for i, ((g, e), (w, we)) in enumerate(zip(zip(got, err), want)) if (e != 0) != (we != 0) or (not we and g != w)]
    if bad:
        i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} rows differ; row {i}: got {got[i]!r} error {err[i]}, want {want[i]}")


def _random_instants(rng, n, lo_year=0, hi_year=9999):
    lo, hi = days_of(lo_year, 1, 1) * DAY, days_of(hi_year, 12, 31) * DAY + DAY
    return [int(v) for v in rng.integers(lo, hi, n)]


def _variant(rng, t):
    """a text derived from a canonical 'yyyy-MM-dd hh:mm:ss.sss': shorter layouts, one-digit fields, two-digit years,
    'T', offsets, 1-3 (or 4) fraction digits, spaces, mutations"""
    y, mo, d, h, mi, s, f = t[0:4], t[5:7], t[8:10], t[11:13], t[14:16], t[17:19], t[20:23]
    r = rng.random()
    if r < 0.15:
        return t
    if r < 0.25:
        return t[:19]
    if r < 0.35:
        return t[:10]
    strip = lambda x: x.lstrip(b"0") or b"0" if rng.random() < 0.3 else x  # noqa: E731
    yy = y[2:] if rng.random() < 0.15 else strip(y)
    out = yy + b"-" + strip(mo) + b"-" + strip(d)
    k = rng.random()
    if k < 0.8:
        out += (b"T" if rng.random() < 0.2 else b" ") + strip(h) + b":" + strip(mi)
        if rng.random() < 0.8:
            out += b":" + strip(s)
            if rng.random() < 0.7:
                out += b"." + (f + b"7")[:int(rng.integers(1, 5)) if rng.random() < 0.1 else int(rng.integers(1, 4))]
    if rng.random() < 0.2:
        oh, om = int(rng.integers(0, 25)), int(rng.integers(0, 61))
        out += [b"", b" "][int(rng.integers(0, 2))] + [b"+", b"-"][int(rng.integers(0, 2))] + b"%02d" % oh + \
            [b"", b":%02d" % om, b"%02d" % om, b":", b"%d" % (om % 10)][int(rng.integers(0, 5))]
    if rng.random() < 0.05:
        out = [b" " + out, out + b" ", out + b"Z", out.replace(b"-", b"/")][int(rng.integers(0, 4))]
    if rng.random() < 0.08 and out:
        at = int(rng.integers(0, len(out)))
        out = out[:at] + bytes([int(rng.choice(list(b"0123456789-: .T+/xa\xc3")))]) + out[at + 1:]
    return out


EDGE_DATES = [b"2024-02-29", b"2023-02-29", b"1900-02-29", b"2000-02-29", b"0000-02-29", b"24-02-29", b"23-2-29", b"99-12-31",
              b"69-12-31", b"70-01-01", b"0-1-1", b"9999-12-31", b"10000-01-01", b"2024-00-10", b"2024-13-10", b"2024-04-31",
              b"2024-01-00", b"2024-01-32", b"2024-01", b"2024", b"", b"-", b"--", b"2024--01", b"2024-01-15-", b"2024-01-",
              b"1234567890-01-01", b"2024-0000000001-01", b"000000002-01-01", b"2024-01-15x9", b"2024-01-151",
              b" 2024-01-15", b"2024-01-15 ", b"2024-01-15T10:20:30", b"2024-01-15 99:99:99.9999", b"\xc3\xa9-1-1"]
EDGE_TIMES = [b"00:00:00", b"23:59:59.999", b"24:00:00", b"23:60:00", b"23:59:60", b"1:2", b"1:2:3", b"1:2:3.4", b"1:2:3.45",
              b"1:2:3.456", b"1:2:3.4567", b"123:00", b"12:345", b"12:", b":12", b"12:30:", b"12:30:15.", b"12-30", b"",
              b" 12:30", b"12:30 ", b"12:30:15.123Z"]


@pytest.mark.parametrize("seed", range(4))
def test_parsers_on_host_against_the_restatement(dtlib, seed):
    rng = np.random.default_rng(9500 + seed)
    n = 25_000
    canon = [text_of(v, 0) for v in _random_instants(rng, n)]
    texts = [_variant(rng, t) for t in canon] + EDGE_DATES + EDGE_TIMES
    dates = [t[:10] if rng.random() < 0.5 else t for t in canon] + [_variant(rng, t) for t in canon[:5000]] + EDGE_DATES
    times = [t[11:] if rng.random() < 0.5 else t[11:19] for t in canon] + [_variant(rng, t)[11:] for t in canon[:5000]] + EDGE_TIMES
    for fn, ref, rows in ((0, cast_date, dates + texts), (1, cast_timestamp, texts), (2, cast_time, times)):
        for text_map in (0, 1, 2):
            want = [_want(ref, _mapped(t, text_map)) for t in rows]
            for inbuf in (1, 0):
                got, err = _parse(dtlib, fn, rows, inbuf, text_map)
                _check(list(got), err, want, f"fn {fn} map {text_map} inbuf {inbuf}")


def test_parser_error_classes_on_host(dtlib):
    cases = {0: [b"2024-01", b"2023-02-29", b"2024-13-01", b"10000-01-01", b"1234567890-1-1", b""],
             1: [b"2024-01-15 10:20:30.1234", b"2024-01-15 24:00:00", b"2024-01-15 10:60", b"2024-01-15 10:20:60",
                 b"2024-01-15 10:20 PST", b"2024-01-15+24:00", b"2024-01-15+05:60", b"2023-02-29", b"20245-01-01",
                 b"2024-01-15 ", b"2024/01/15"],
             2: [b"24:00", b"10:60", b"10:20:60", b"10:20:30.1234", b"10", b"10:20:30 "]}
    for fn, rows in cases.items():
        for inbuf in (1, 0):
            _, err = _parse(dtlib, fn, rows, inbuf)
            assert all(e == 4 for e in err), (fn, inbuf, list(err))


def test_fast_path_and_scanner_agree_on_canonical_rows(dtlib):
    rng = np.random.default_rng(9600)
    canon = [text_of(v, 0) for v in _random_instants(rng, 30_000)] + [text_of(v, 0) for v in _random_instants(rng, 2000, 0, 99)]
    for fn, rows in ((0, [t[:10] for t in canon] + canon), (1, canon + [t[:19] for t in canon] + [t[:10] for t in canon]),
                     (2, [t[11:] for t in canon] + [t[11:19] for t in canon])):
        fast, e1 = _parse(dtlib, fn, rows, 1)
        slow, e2 = _parse(dtlib, fn, rows, 0)
        assert not e1.any() and not e2.any()
        assert (fast == slow).all()
        ref = (cast_date, cast_timestamp, cast_time)[fn]
        assert fast.tolist() == [ref(r) for r in rows]
        # the same rows behind a leading space or with a trailing one: the byte scanner, whatever it answers
        for pad in ((lambda r: b" " + r), (lambda r: r + b" ")):
            padded = [pad(r) for r in rows[:5000]]
            got, err = _parse(dtlib, fn, padded, 1)
            _check(list(got), err, [_want(ref, r) for r in padded], f"fn {fn} padded")


KINDS = [(0, "timestamp"), (1, "date64"), (2, "date32"), (3, "time32")]
NS = [-1, 0, 5, 10, 23, 100]


@pytest.mark.parametrize("kind,what", KINDS)
def test_formatters_on_host_against_the_restatement(dtlib, kind, what):
    rng = np.random.default_rng(9700 + kind)
    n = 100_000
    vals = _random_instants(rng, n - 6000) + [int(v) for v in rng.integers(-(2**62), 2**62, 2000)] + \
        [int(v) for v in rng.integers(253_402_300_800_000, 3_093_000_000_000_000, 2000)] + \
        [int(v) for v in rng.integers(-3 * DAY, 3 * DAY, 2000)]
    vals += [0, -1, 2**63 - 1, -2**63, days_of(0, 1, 1) * DAY - 1, days_of(9999, 12, 31) * DAY + DAY]
    if kind == 2:
        vals = [v // DAY if -2**31 <= v // DAY < 2**31 else int(rng.integers(-2**31, 2**31)) for v in vals]
    if kind == 3:
        vals = [v % DAY if i % 3 else (v % 2**32) - 2**31 for i, v in enumerate(vals)]
    ns = [NS[int(rng.integers(0, len(NS)))] if rng.random() < 0.7 else int(rng.integers(-3, 30)) for _ in vals]
    got, err = _format(dtlib, kind, vals, ns)
    k = (0, 1, 1, 2)[kind]
    ms = [v * DAY if kind == 2 else v for v in vals]
    _check(got, err, [_want(cast_varchar, m, k, x) for m, x in zip(ms, ns)], what)


def test_fixed_width_casts_on_host(dtlib):
    rng = np.random.default_rng(9800)
    v = np.concatenate([rng.integers(-(2**62), 2**62, 10_000), [0, -1, DAY, -DAY, 2**63 - 1, -2**63]]).astype(np.int64)
    out = np.zeros(len(v), dtype=np.int64)
    dtlib.host_temporal_fixed(0, _p(v), C.c_long(len(v)), _p(out))
    assert out.tolist() == [int(x) % DAY for x in v]
    d = np.concatenate([rng.integers(-2**31, 2**31, 10_000), [0, -1, 2**31 - 1, -2**31]]).astype(np.int64)
    dtlib.host_temporal_fixed(1, _p(d), C.c_long(len(d)), _p(out[:len(d)]))
    assert out[:len(d)].tolist() == [int(x) * DAY for x in d]
