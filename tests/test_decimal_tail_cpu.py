"""The decimal tail without a GPU: castDECIMAL of float32 / float64 / text, castDECIMALNullOnOverflow, nvl / greatest / least,
is_distinct_from / is_not_distinct_from and hash / hash32 / hash64 over decimal128.

PARITY STATUS (PARITY.md, decimal tail): recollection.  What other engines pin: the text grammar is the accept set of
arrow::Decimal128::FromString (libarrow, reached through a pyarrow cast) and exact values agree with it; the float rule
agrees with decimal.Decimal(x), the exact binary value, on floats of at most 15 significant digits; MurmurHash3 is public.
Decided here: an exponent of more than 9 digits raises, "1e+-5" is refused, a value beyond the declared precision is 0 (the
lineage raises where its parser "cannot represent" the text).

The expected values of every test here and in test_decimal_tail.py come from the plain-Python restatement below (Python
integers, the decimal module for reading digits, helpers.py's MurmurHash3).  This file checks
  * the restatement against libarrow and decimal.Decimal;
  * the product's device functions compiled for the host (tests/host_devlib/host_decimal_tail.cc), bit for bit;
  * the parser under AddressSanitizer / UBSan as a stand-alone program run as a child process (tests/cxx/decimal_parse_check.cc);
  * the registry through the Python mirror and the rebuilt pyarrow.gandiva, the trees through the C++ API, the same-type rule;
  * that C2's, C4's and C5's kernels keep their names, and that tier 0 still refuses decimal plans."""
import ctypes as C
import decimal
import math
import os
import re
import subprocess

import numpy as np
import pyarrow as pa
import pytest

import gandiva_amd as gandiva
from gandiva_amd import _capi, workloads as W
from helpers import full_range_values, py_murmur3_x64_128_h1

HERE = os.path.dirname(os.path.abspath(__file__))
D = pa.decimal128
DEC = D(38, 0)   # how the registry enumerates decimal128
F32, F64, STR, I32, I64, BOOL = pa.float32(), pa.float64(), pa.string(), pa.int32(), pa.int64(), pa.bool_()
TARGETS = [(38, 0), (38, 38), (15, 2), (5, 0), (1, 1)]
SOURCE_SCALES = [0, 2, 12, 38]


class RowError(Exception):
    """the row raises "invalid argument" (an execution error of the whole evaluation)"""


# ------------------------------------------------------------------ the restatement

P10 = [float("1e%d" % k) for k in range(39)]   # the double nearest to 10^k


def dec_of_float(x, op, os):
    """x (a Python float; a float32 is widened first, exactly) -> unscaled integer of decimal(op, os)"""
    u = x * P10[os]                  # ONE IEEE multiplication
    if u != u or math.isinf(u):
        return 0
    t = math.trunc(u)
    if abs(u - t) >= 0.5:            # (abs(u) + 0.5 is wrong just below one half: the sum rounds up)
        t += 1 if u > 0 else -1
    return 0 if abs(t) >= 10 ** op else t


TEXT = re.compile(rb"[+-]?(?:[0-9]+(?:\.[0-9]*)?|\.[0-9]+)(?:[eE][+-]?([0-9]+))?")


def parse_text(t):
    """bytes -> (negative, digits as an integer, exponent of the last digit), or RowError"""
    m = TEXT.fullmatch(t)
    if m is None or (m.group(1) is not None and len(m.group(1)) > 9):
        raise RowError(t)
    sign, digits, exp = decimal.Decimal(t.decode("ascii")).as_tuple()
    return bool(sign), int("".join(map(str, digits))), exp


def dec_of_parsed(parsed, op, os):
    """the exact value, rounded half away from zero to os fractional digits; more than op digits: 0"""
    neg, m, exp = parsed
    e = exp + os
    if m == 0:
        return 0
    if e >= 0:
        v = m * 10 ** e if e <= 80 else 10 ** 99
    else:
        k = -e
        if k > len(str(m)) + 1:
            return 0
        v, r = divmod(m, 10 ** k)
        if 2 * r >= 10 ** k:
            v += 1
    if v >= 10 ** op:
        return 0
    return -v if neg else v


def dec_of_text(t, op, os):
    return dec_of_parsed(parse_text(t), op, os)


def rescale_or_none(x, xs, op, os):
    """castDECIMALNullOnOverflow: None where the value does not fit op digits"""
    if os >= xs:
        r = x * 10 ** (os - xs)
    else:
        q, rem = divmod(abs(x), 10 ** (xs - os))
        q += 1 if 2 * rem >= 10 ** (xs - os) else 0
        r = -q if x < 0 else q
    return None if abs(r) >= 10 ** op else r


def is_distinct(a, sa, b, sb):
    """a, b: unscaled integers or None; by value"""
    if (a is None) != (b is None):
        return True
    if a is None:
        return False
    s = max(sa, sb)
    return a * 10 ** (s - sa) != b * 10 ** (s - sb)


def nvl_of(a, b):
    return a if a is not None else b


def both(fn):
    return lambda a, b: None if a is None or b is None else fn(a, b)


def le16(v):
    return (v & ((1 << 128) - 1)).to_bytes(16, "little")


def murmur3_32(data, seed):
    """MurmurHash3_x86_32 (signed)"""
    M = 0xFFFFFFFF
    h = seed & M

    def mix(k):
        k = k * 0xcc9e2d51 & M
        k = (k << 15 | k >> 17) & M
        return k * 0x1b873593 & M
    n = len(data) // 4
    for i in range(n):
        h ^= mix(int.from_bytes(data[4 * i:4 * i + 4], "little"))
        h = (h << 13 | h >> 19) & M
        h = (h * 5 + 0xe6546b64) & M
    tail = data[4 * n:]
    if tail:
        h ^= mix(int.from_bytes(tail, "little"))
    h ^= len(data)
    h ^= h >> 16
    h = h * 0x85ebca6b & M
    h ^= h >> 13
    h = h * 0xc2b2ae35 & M
    h ^= h >> 16
    return h - (1 << 32) if h >> 31 else h


def _i32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def hash32_of(v, seed=0):
    """v: unscaled integer or None; seed: int32 or None (a NULL seed is 0).  A NULL value hashes to the seed"""
    seed = 0 if seed is None else seed
    return seed if v is None else murmur3_32(le16(v), seed)


def hash64_of(v, seed=0):
    """seed: int64 or None; the hash starts from its low 32 bits, sign-extended, as the numeric variants do"""
    seed = 0 if seed is None else seed
    return seed if v is None else py_murmur3_x64_128_h1(le16(v), _i32(seed))


# ------------------------------------------------------------------ generators shared with test_decimal_tail.py

def _digits(rng, k):
    return bytes(rng.integers(0x30, 0x3A, k, dtype=np.uint8))


def text_corpus(rng, n, mutate=0.15, cut=0.05):
    """0-15 digits on each side of the point, one-digit exponents; `mutate` of the texts with one byte replaced, `cut` of
    them cut short"""
    palette = b"0123456789+-.eE ,x\t"
    out = []
    for _ in range(n):
        t = [b"", b"", b"+", b"-"][int(rng.integers(0, 4))] + _digits(rng, int(rng.integers(0, 16)))
        if rng.random() < 0.7:
            t += b"." + _digits(rng, int(rng.integers(0, 16)))
        if rng.random() < 0.4:
            t += [b"e", b"E"][int(rng.integers(0, 2))] + [b"", b"+", b"-"][int(rng.integers(0, 3))] + _digits(rng, 1)
        k = rng.random()
        if k < mutate and t:
            t = bytearray(t)
            t[int(rng.integers(0, len(t)))] = palette[int(rng.integers(0, len(palette)))] if rng.random() < 0.8 else int(rng.integers(0, 256))
            t = bytes(t)
        elif k < mutate + cut and t:
            t = t[:int(rng.integers(0, len(t)))]
        out.append(t)
    return out


def long_texts(rng, n):
    """39-80 digits, a point anywhere, exponents up to +-60: all valid"""
    out = []
    for _ in range(n):
        d = _digits(rng, int(rng.integers(39, 81)))
        at = int(rng.integers(0, len(d) + 1))
        t = [b"", b"-"][int(rng.integers(0, 2))] + d[:at] + (b"." + d[at:] if at < len(d) or rng.random() < 0.5 else b"")
        if at == 0:
            t = t.replace(b".", b"0.", 1) if rng.random() < 0.5 else t
        if rng.random() < 0.8:
            t += b"e%d" % int(rng.integers(-60, 61))
        out.append(t)
    return out


def valid_texts(rng, n, max_len=45):
    """valid texts of 1..max_len bytes whose values spread over every magnitude"""
    out = []
    while len(out) < n:
        for t in text_corpus(rng, n, mutate=0.0, cut=0.0) + long_texts(rng, n // 8 + 1):
            if len(t) <= max_len and TEXT.fullmatch(t):
                out.append(t)
    return out[:n]


def dense_decimals(rng, n, digits=38):
    """unscaled integers of 1..digits random digits, both signs (Python integers)"""
    out = []
    for _ in range(n):
        v = int(_digits(rng, int(rng.integers(1, digits + 1))))
        out.append(-v if rng.random() < 0.5 else v)
    return out


def decimal_array(vals, t, offset=0):
    """unscaled Python integers (None: null) -> decimal128 array, sliced `offset` rows in"""
    n = len(vals) + offset
    raw = np.zeros((n, 2), dtype=np.uint64)
    valid = np.zeros(n, dtype=bool)
    for i, v in enumerate(vals):
        if v is not None:
            u = v & ((1 << 128) - 1)
            raw[i + offset] = (u & 0xFFFFFFFFFFFFFFFF, u >> 64)
            valid[i + offset] = True
    arr = pa.Array.from_buffers(t, n, [pa.py_buffer(np.packbits(valid, bitorder="little")), pa.py_buffer(raw)])
    return arr.slice(offset)


def unscaled(arr):
    """decimal128 array -> unscaled Python integers (None: null)"""
    raw = np.frombuffer(arr.buffers()[1], dtype=np.uint64).reshape(-1, 2)[arr.offset:arr.offset + len(arr)]
    ok = arr.is_valid().to_pylist()
    out = []
    for (lo, hi), v in zip(raw.tolist(), ok):
        x = lo | hi << 64
        out.append(None if not v else x - (1 << 128) if x >> 127 else x)
    return out


# ------------------------------------------------------------------ 1. the restatement: pins, libarrow, decimal.Decimal

def test_restatement_pins():
    for t in (b"5.", b".5", b"+.5", b"-.5e1", b"1.e1", b"1e05", b"1e-0"):
        parse_text(t)
    for t in (b"", b" ", b".", b"+", b"1e", b"1e+", b".e5", b"1..", b"1e 5", b"1e5 ", b" 1.2", b"1,5", "١".encode(), b"1e+-5",
              b"1e1234567890", b"1_0", b"Infinity", b"nan", b"1e5\n"):
        with pytest.raises(RowError):
            parse_text(t)
    assert dec_of_text(b"1.005", 38, 2) == 101 and dec_of_text(b"-1.005", 38, 2) == -101 and dec_of_text(b"1.0049999", 38, 2) == 100
    assert dec_of_text(b"12e3", 15, 2) == 1200000 and dec_of_text(b"5e-1", 5, 0) == 1 and dec_of_text(b"5e-2", 5, 0) == 0
    assert dec_of_text(b"99999.5", 5, 0) == 0 and dec_of_text(b"99999.4", 5, 0) == 99999 and dec_of_text(b"-69e58", 38, 0) == 0
    assert dec_of_text(b"1e999999999", 38, 0) == 0 and dec_of_text(b"0e999999999", 38, 0) == 0 and dec_of_text(b"1", 1, 1) == 0
    assert dec_of_float(0.125, 15, 2) == 13 and dec_of_float(-0.125, 15, 2) == -13 and dec_of_float(0.49999999999999994, 5, 0) == 0
    assert dec_of_float(float("nan"), 38, 0) == 0 and dec_of_float(float("inf"), 38, 0) == 0
    # the double nearest to 10^38 lies below it and fits 38 digits; its upper neighbour does not
    assert dec_of_float(1e38, 38, 0) == int(1e38) < 10 ** 38 and dec_of_float(math.nextafter(1e38, math.inf), 38, 0) == 0
    assert dec_of_float(9.999999999999999e37, 38, 0) == int(9.999999999999999e37) and dec_of_float(99999.5, 5, 0) == 0
    assert rescale_or_none(0, 0, 1, 38) == 0 and rescale_or_none(1, 0, 38, 38) is None and rescale_or_none(99995, 1, 4, 0) is None
    assert rescale_or_none(-99994, 1, 4, 0) == -9999
    assert not is_distinct(10, 1, 1, 0) and is_distinct(10, 1, 1, 1) and is_distinct(None, 0, 0, 0) and not is_distinct(None, 0, None, 5)
    assert murmur3_32(b"", 0) == 0 and murmur3_32(b"", 1) == 0x514E28B7 and murmur3_32(b"abcd", 0x9747b28c) == _i32(0xF0478627)
    assert murmur3_32(b"Hello, world!", 0x9747b28c) == 0x24884CBA
    assert hash32_of(None) == 0 and hash32_of(None, 7) == 7 and hash64_of(None, -3) == -3 and hash32_of(5, None) == hash32_of(5)


def _libarrow(t, scale, safe):
    """('ok', unscaled) | ('invalid', message) | ('unrepresentable', message)"""
    try:
        arr = pa.array([t], type=pa.binary()).cast(STR).cast(D(38, scale), safe=safe)
    except pa.ArrowInvalid as e:
        return ("unrepresentable" if "cannot be represented" in str(e) else "invalid"), str(e)
    return "ok", unscaled(arr)[0]


def test_restatement_grammar_and_values_against_libarrow():
    """libarrow's parser is what the lineage calls.  Excluded: texts it "cannot represent" (a value beyond 38 digits: 0 here)
    and the "e+-" quirk of its exponent reader; texts that are not UTF-8 (a mutated byte >= 0x80) are refused by both, here
    without asking libarrow."""
    rng = np.random.default_rng(2024)
    texts = text_corpus(rng, 20_000)
    excluded = agree_ok = agree_bad = exact = 0
    for t in texts:
        try:
            parsed = parse_text(t)
        except RowError:
            parsed = None
        try:
            t.decode("utf-8")
        except UnicodeDecodeError:
            assert parsed is None
            agree_bad += 1
            continue
        verdict, what = _libarrow(t, 0, False)
        if verdict == "unrepresentable" or re.search(rb"[eE]\+-", t):
            excluded += 1
            continue
        assert (verdict == "ok") == (parsed is not None), (t, verdict, what)
        if parsed is None:
            agree_bad += 1
            continue
        agree_ok += 1
        for scale in (2, 20):
            verdict, value = _libarrow(t, scale, True)   # succeeds only when no digit is lost: the exact value
            # (libarrow does not check its scale-up for overflow: b"+3947008588E9" at scale 20 "succeeds" with a wrapped value;
            # a value is compared where its digits fit 38, which the text's own magnitude tells)
            fits = parsed[1] == 0 or len(str(parsed[1])) + parsed[2] + scale <= 38
            if verdict == "ok" and fits:
                exact += 1
                assert dec_of_parsed(parsed, 38, scale) == value, (t, scale)
    assert excluded / len(texts) < 0.005, excluded
    assert agree_ok > 10_000 and agree_bad > 2_000 and exact > 5_000, (agree_ok, agree_bad, exact)


def test_restatement_float_rule_against_the_exact_binary_value():
    """decimal.Decimal(x) is the exact binary value of x; scaled by 10^os and rounded half away from zero it is what a cast
    without any intermediate rounding gives.  The restatement rounds the PRODUCT x * 10^os once, to 53 bits, before it rounds
    to an integer, so the two may differ where the exact product lies within an ulp of a tie (the double 0.015 is
    0.01499999999999999944...: times 100 exactly that rounds to 1, yet the one multiplication gives 1.5: 2) and wherever the product has more than 53
    significant bits (beyond 15 significant digits its integer part itself is rounded).  Checked here: doubles nearest to a
    decimal of at most 15 significant digits whose scaled value stays below 10^15, ties of that tolerance left out."""
    rng = np.random.default_rng(7)
    ctx = decimal.Context(prec=400, rounding=decimal.ROUND_HALF_UP)
    checked = differ_near_ties = 0
    for _ in range(20_000):
        m = int(rng.integers(0, 10 ** int(rng.integers(1, 16))))
        os = int(rng.integers(0, 13))
        e = -os - int(rng.integers(0, 4))
        x = float("%de%d" % (m, e)) * (-1 if rng.random() < 0.5 else 1)
        exact = ctx.multiply(decimal.Decimal(x), decimal.Decimal(10) ** os)
        frac = abs(exact - exact.to_integral_value(rounding=decimal.ROUND_DOWN))
        want = int(exact.to_integral_value(rounding=decimal.ROUND_HALF_UP))
        if abs(frac - decimal.Decimal("0.5")) <= abs(exact) * decimal.Decimal(2) ** -50:
            differ_near_ties += dec_of_float(x, 38, os) != want
            continue
        assert dec_of_float(x, 38, os) == want, (x, os)
        checked += 1
    assert checked > 15_000
    assert dec_of_float(0.015, 15, 2) == 2 and dec_of_float(1.005, 15, 2) == 100 and differ_near_ties > 0


# ------------------------------------------------------------------ 2. the device functions on the host

SRC = os.path.join(HERE, "host_devlib", "host_decimal_tail.cc")
LIB = os.path.join(HERE, "host_devlib", "libhost_decimal_tail.so")


@pytest.fixture(scope="module")
def declib():
    hdr = os.path.join(HERE, "..", "gandiva_amd", "csrc", "gdv_device_lib.hpp")
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off",
                               "-Wno-unused-function", "-Wno-unused-variable", "-Wno-attributes", SRC, "-o", LIB])
    return C.CDLL(LIB)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _raw(vals):
    raw = np.zeros((len(vals), 2), dtype=np.uint64)
    for i, v in enumerate(vals):
        u = (v or 0) & ((1 << 128) - 1)
        raw[i] = (u & 0xFFFFFFFFFFFFFFFF, u >> 64)
    return raw


def _ints(raw):
    out = []
    for lo, hi in raw.reshape(-1, 2).tolist():
        x = lo | hi << 64
        out.append(x - (1 << 128) if x >> 127 else x)
    return out


def _flags(vals):
    return np.array([v is not None for v in vals], dtype=np.uint8)


def _host_text(lib, texts, valid, op, os, text_map=0):
    n = len(texts)
    off = np.zeros(n + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(t) for t in texts])
    data = np.frombuffer(b"".join(texts) + b"\0", dtype=np.uint8).copy()   # (one spare byte: numpy has no empty buffer)
    out = np.zeros((n, 2), dtype=np.uint64)
    err = np.zeros(n, dtype=np.uint8)
    lib.host_cast_text(_p(off), _p(data), C.c_long(int(off[-1])), _p(valid), C.c_long(n), text_map, op, os, _p(out), _p(err))
    return _ints(out), err


def test_host_text_cast_against_the_restatement(declib):
    rng = np.random.default_rng(11)
    texts = text_corpus(rng, 100_000) + long_texts(rng, 4_000)
    texts[:12] = [b"", b".", b"5.", b".5", b"1e+-5", b"1e1234567890", b"1e123456789", b"-0.0", b"+0e-9", b"99999.5", b"0.5", b"-69e58"]
    valid = (rng.random(len(texts)) >= 0.1).astype(np.uint8)
    parsed = []
    for t in texts:
        try:
            parsed.append(parse_text(t))
        except RowError:
            parsed.append(None)
    assert 0.1 < sum(p is None for p in parsed) / len(texts) < 0.3
    for op, os in TARGETS:
        got, err = _host_text(declib, texts, valid, op, os)
        assert set(err.tolist()) <= {0, 4}, "only GDV_ERR_BAD_ARG is raised"
        for i, (p, v) in enumerate(zip(parsed, valid)):
            if not v:
                assert err[i] == 0 and got[i] == 0, (texts[i], "a null row is not parsed")
            elif p is None:
                assert err[i] == 4, (texts[i], op, os)
            else:
                assert err[i] == 0 and got[i] == dec_of_parsed(p, op, os), (texts[i], op, os, got[i])
    # through the byte maps: 'E' and 'e' are one letter, digits and signs have no case
    sub, ones = texts[:20_000], np.ones(20_000, dtype=np.uint8)
    for text_map in (1, 2):
        got, err = _host_text(declib, sub, ones, 15, 2, text_map)
        for i, p in enumerate(parsed[:20_000]):
            if p is None:
                mapped = sub[i].upper() if text_map == 1 else sub[i].lower()
                assert (err[i] == 4) == (TEXT.fullmatch(mapped) is None or len(TEXT.fullmatch(mapped).group(1) or b"") > 9), sub[i]
            else:
                assert err[i] == 0 and got[i] == dec_of_parsed(p, 15, 2), sub[i]


def _float_cases(t, op, os):
    rng = np.random.default_rng(op * 100 + os)
    dt = np.float32 if t == F32 else np.float64
    fi = np.finfo(dt)
    with np.errstate(over="ignore"):
        edge = 10.0 ** (op - os)
        special = [0.0, -0.0, fi.smallest_subnormal, -fi.smallest_subnormal, fi.tiny / 2, fi.tiny, np.inf, -np.inf, np.nan, fi.max, -fi.max,
                   0.5, -0.5, 0.49999999999999994, -0.49999999999999994, 1.5, 2.5, -2.5, 0.125, 0.285, 1.005,
                   2.0 ** 52 - 0.5, 2.0 ** 52 - 1.5, 2.0 ** 52 + 1, 2.0 ** 52 + 2, 2.0 ** 51 + 0.5, 2.0 ** 53 + 2, -(2.0 ** 52 - 0.5),
                   -(2.0 ** 52 + 1), 2.0 ** 63, 2.0 ** 64, 2.0 ** 126, 2.0 ** 127, -(2.0 ** 127), 1e38, 9.999999999999999e37]
        special = np.array(special, dtype=dt)
        near = np.array([s * f(dt(edge * m)) for m in (1.0, 0.1, 10.0 ** -os if os else 1.0) for s in (1, -1)
                         for f in (lambda v: v, lambda v: np.nextafter(v, dt(0)), lambda v: np.nextafter(v, dt(np.inf)))], dtype=dt)
        scaled = (rng.integers(-10 ** 9, 10 ** 9, 4000) / 8.0).astype(dt)     # many exact halves and quarters
    return np.concatenate([special, near, scaled, full_range_values(rng, t, 20_000)])


@pytest.mark.parametrize("t", [F64, F32], ids=["float64", "float32"])
def test_host_float_casts_against_the_restatement(declib, t):
    for op, os in TARGETS:
        x = _float_cases(t, op, os)
        out = np.zeros((len(x), 2), dtype=np.uint64)
        (declib.host_cast_f64 if t == F64 else declib.host_cast_f32)(_p(x), C.c_long(len(x)), op, os, _p(out))
        got = _ints(out)
        want = [dec_of_float(float(v), op, os) for v in x]
        bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not bad, (op, os, x[bad[0]], got[bad[0]], want[bad[0]])
        assert sum(1 for w in want if w != 0) > 100 or op == os


def test_host_cast_null_on_overflow(declib):
    rng = np.random.default_rng(13)
    for xs in SOURCE_SCALES:
        vals = dense_decimals(rng, 3000) + [0, 1, -1, 10 ** 38 - 1, -(10 ** 38 - 1), 5 * 10 ** 37, 10 ** 37 - 1]
        vals = [None if rng.random() < 0.1 else v for v in vals]
        for op, os in TARGETS:
            out = np.zeros((len(vals), 2), dtype=np.uint64)
            ov = np.full(len(vals), 7, dtype=np.uint8)
            declib.host_cast_null_on_overflow(_p(_raw(vals)), _p(_flags(vals)), C.c_long(len(vals)), 38, xs, op, os, _p(out), _p(ov))
            want = [None if v is None else rescale_or_none(v, xs, op, os) for v in vals]
            got = [g if o else None for g, o in zip(_ints(out), ov)]
            assert got == want, (xs, op, os)
            assert set(ov.tolist()) <= {0, 1}
    # scaling up and down both meet overflow and both meet values that fit
    assert rescale_or_none(10 ** 37, 0, 38, 2) is None and rescale_or_none(10 ** 35, 0, 38, 2) == 10 ** 37


def test_host_is_distinct_from_across_scales(declib):
    rng = np.random.default_rng(17)
    for sa in SOURCE_SCALES:
        for sb in SOURCE_SCALES:
            a = dense_decimals(rng, 1500)
            b = dense_decimals(rng, 1500)
            # equal VALUES at the two scales, wherever both sides can hold them
            for i in range(0, 1500, 3):
                top = min(10 ** 6, 10 ** (38 - abs(sa - sb)) - 1)   # the wider side stays within 38 digits
                v = int(rng.integers(-top, top + 1))
                lo = min(sa, sb)
                a[i], b[i] = v * 10 ** (sa - lo), v * 10 ** (sb - lo)
            a = [None if rng.random() < 0.15 else v for v in a]
            b = [None if rng.random() < 0.15 else v for v in b]
            a[:2], b[:2] = ([10, 10], [1, None]) if (sa, sb) != (0, 0) else ([1, 1], [1, None])
            d = np.zeros(len(a), dtype=np.uint8)
            nd = np.zeros(len(a), dtype=np.uint8)
            declib.host_distinct(_p(_raw(a)), _p(_flags(a)), 38, sa, _p(_raw(b)), _p(_flags(b)), 38, sb, C.c_long(len(a)), _p(d), _p(nd))
            want = [is_distinct(x, sa, y, sb) for x, y in zip(a, b)]
            assert d.astype(bool).tolist() == want and nd.astype(bool).tolist() == [not w for w in want], (sa, sb)
            assert 0.2 < sum(want) / len(want) < 0.9
    # 10 @ scale 1 is 1 @ scale 0
    a, b = [10, 10, None], [1, 2, None]
    d, nd = np.zeros(3, dtype=np.uint8), np.zeros(3, dtype=np.uint8)
    declib.host_distinct(_p(_raw(a)), _p(_flags(a)), 5, 1, _p(_raw(b)), _p(_flags(b)), 5, 0, C.c_long(3), _p(d), _p(nd))
    assert d.tolist() == [0, 1, 0] and nd.tolist() == [1, 0, 1]


def test_host_nvl_greatest_least(declib):
    rng = np.random.default_rng(19)
    a = [None if rng.random() < 0.2 else v for v in dense_decimals(rng, 4000)]
    b = [None if rng.random() < 0.2 else v for v in dense_decimals(rng, 4000)]
    for fn, rule in ((0, nvl_of), (1, both(max)), (2, both(min))):
        out = np.zeros((len(a), 2), dtype=np.uint64)
        ov = np.zeros(len(a), dtype=np.uint8)
        declib.host_pick(fn, _p(_raw(a)), _p(_flags(a)), _p(_raw(b)), _p(_flags(b)), C.c_long(len(a)), 38, 4, _p(out), _p(ov))
        got = [g if o else None for g, o in zip(_ints(out), ov)]
        assert got == [rule(x, y) for x, y in zip(a, b)], fn


def test_host_hashes_against_pure_python_murmur3(declib):
    rng = np.random.default_rng(23)
    vals = dense_decimals(rng, 5000) + [0, 1, -1, 10 ** 38 - 1, -(10 ** 38 - 1), 1 << 64, -(1 << 64), (1 << 63) - 1]
    vals = [None if rng.random() < 0.1 else v for v in vals]
    n = len(vals)
    s32 = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)
    s64 = rng.integers(-2 ** 63, 2 ** 63 - 1, n).astype(np.int64)
    sv = (rng.random(n) >= 0.1).astype(np.uint8)
    h32, h32s = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    h64, h64s = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    declib.host_hash(_p(_raw(vals)), _p(_flags(vals)), _p(s32), _p(s64), _p(sv), C.c_long(n), _p(h32), _p(h32s), _p(h64), _p(h64s))
    assert h32.tolist() == [hash32_of(v) for v in vals]
    assert h64.tolist() == [hash64_of(v) for v in vals]
    assert h32s.tolist() == [hash32_of(v, int(s) if k else None) for v, s, k in zip(vals, s32, sv)]
    assert h64s.tolist() == [hash64_of(v, int(s) if k else None) for v, s, k in zip(vals, s64, sv)]


# ------------------------------------------------------------------ 3. the parser under sanitizers, as a child process

@pytest.mark.parametrize("name,extra", [("plain", []), ("asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"])])
def test_parser_reads_nothing_past_its_text(name, extra):
    inc = os.path.join(HERE, "..", "gandiva_amd", "csrc")
    out = os.path.join(inc, "build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "decimal_parse_check_" + name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-unused-function", "-Wno-unused-variable", "-Wno-attributes"] +
                          extra + ["-I", inc, os.path.join(HERE, "cxx", "decimal_parse_check.cc"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, f"exit {run.returncode}\n{run.stdout}\n{run.stderr}"
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    assert "decimal_parse_check: ok" in run.stdout


# ------------------------------------------------------------------ 4. front doors

WANT = ([("castDECIMAL", (t,), DEC) for t in (F64, F32, STR)] + [("castDECIMALNullOnOverflow", (DEC,), DEC)] +
        [(f, (DEC, DEC), DEC) for f in ("nvl", "greatest", "least")] +
        [(f, (DEC, DEC), BOOL) for f in ("is_distinct_from", "is_not_distinct_from")] +
        [("hash", (DEC,), I32), ("hash32", (DEC,), I32), ("hash64", (DEC,), I64), ("hash32", (DEC, I32), I32), ("hash64", (DEC, I64), I64)])


def _signatures(sigs):
    return {(s.name(), tuple(s.param_types())): s.return_type() for s in sigs}


def _check_registry(sigs):
    assert len(WANT) == 14
    for name, params, ret in WANT:
        assert sigs.get((name, params)) == ret, (name, params)
    for name in ("hash32AsDouble", "hash64AsDouble"):   # decided: not added for decimals
        assert not [k for k in sigs if k[0] == name and pa.types.is_decimal(k[1][0])]


def test_registry_lists_the_fourteen_signatures():
    _check_registry(_signatures(gandiva.get_registered_function_signatures()))


def test_registry_of_the_rebuilt_pyarrow_gandiva_lists_them():
    from gandiva_amd import pyarrow_gandiva
    _check_registry(_signatures(pyarrow_gandiva.load().get_registered_function_signatures()))


def test_cxx_trees_host_only():
    cxx = os.path.join(HERE, "..", "gandiva_amd", "cxx")
    subprocess.check_call(["make", "-C", cxx, "all", "test_cxx"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(cxx, "tests", "test_decimal_tail_cxx"), "--host-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "OK (host-only)" in out.stdout, out.stdout + out.stderr


SCH = pa.schema([pa.field("s", STR), pa.field("x", F64), pa.field("f", F32), pa.field("d", D(15, 2)), pa.field("e", D(15, 2)),
                 pa.field("g", D(20, 5)), pa.field("i", I32), pa.field("l", I64)])


@pytest.mark.parametrize("name", ["nvl", "greatest", "least"])
def test_unequal_decimal_types_fail_at_make(name):
    b = gandiva.TreeExprBuilder()
    d, e, g = (b.make_field(SCH.field(k)) for k in ("d", "e", "g"))
    for args, ret in (([d, g], D(15, 2)), ([g, d], D(15, 2)), ([d, e], D(16, 2)), ([d, g], D(20, 5))):
        with pytest.raises(Exception) as err:
            gandiva.make_projector(SCH, [b.make_expression(b.make_function(name, args, ret), pa.field("o", ret))], None)
        assert "Validation" in type(err.value).__name__ + str(err.value) and "precision and scale" in str(err.value), err.value


def every_signature_exprs(b, schema=SCH):
    """one expression per signature over SCH's columns: [(expression, family)]"""
    f = {x.name: b.make_field(x) for x in schema}
    fn = b.make_function
    trees = [("cast", fn("castDECIMAL", [f["s"]], D(15, 2)), D(15, 2)), ("cast", fn("castDECIMAL", [f["x"]], D(15, 2)), D(15, 2)),
             ("cast", fn("castDECIMAL", [f["f"]], D(38, 10)), D(38, 10)), ("cast", fn("castDECIMALNullOnOverflow", [f["g"]], D(10, 2)), D(10, 2)),
             ("pick", fn("nvl", [f["d"], f["e"]], D(15, 2)), D(15, 2)), ("pick", fn("greatest", [f["d"], f["e"]], D(15, 2)), D(15, 2)),
             ("pick", fn("least", [f["d"], f["e"]], D(15, 2)), D(15, 2)),
             ("distinct", fn("is_distinct_from", [f["d"], f["g"]], BOOL), BOOL), ("distinct", fn("is_not_distinct_from", [f["d"], f["g"]], BOOL), BOOL),
             ("hash", fn("hash", [f["d"]], I32), I32), ("hash", fn("hash32", [f["d"]], I32), I32), ("hash", fn("hash64", [f["d"]], I64), I64),
             ("hash", fn("hash32", [f["d"], f["i"]], I32), I32), ("hash", fn("hash64", [f["d"], f["l"]], I64), I64)]
    return [(b.make_expression(node, pa.field("o%d" % k, t)), fam) for k, (fam, node, t) in enumerate(trees)]


def test_make_of_every_signature_cross_compiles(monkeypatch, tmp_path):
    """Make resolves and plans the fourteen signatures; their kernel compiles for gfx950 (on the parent: "not supported yet")"""
    from test_planner_cpu import _precompile
    b = gandiva.TreeExprBuilder()
    files = _precompile(monkeypatch, tmp_path, SCH, exprs=[e for e, _ in every_signature_exprs(b)])
    text = "".join(open(tmp_path / f).read().split('#include "gdv_device_lib.hpp"')[-1] for f in files)
    for sym in ("castDECIMAL_utf8(ctx, ", "castDECIMAL_float64(", "castDECIMAL_float32(", "castDECIMALNullOnOverflow_decimal128(",
                "nvl_decimal128_decimal128(", "greatest_decimal128_decimal128(", "least_decimal128_decimal128(",
                "is_distinct_from_decimal128_decimal128(", "is_not_distinct_from_decimal128_decimal128(", "hash32_decimal128(",
                "hash64_decimal128(", "hash32_decimal128_int32(", "hash64_decimal128_int64("):
        assert sym in text, sym
    # the raising cast runs only on live rows whose text is valid
    assert re.search(r"\(live && \w+\) \? castDECIMAL_utf8\(", text)


# ------------------------------------------------------------------ 5. kernel names of the baseline workloads, tier 0

# generated from the PARENT commit's library: every gdv_k_ name in the sources its planner dumps for the workload
PARENT_KERNELS = {
    "c2": ["gdv_k_d879db475de55ede"],
    "c4": ["gdv_k_3ca691c558a0d28c"],
    "c5": ["gdv_k_176cc168aed1acc5", "gdv_k_3bda2d4e01914b46", "gdv_k_3d60977eeda8feb4", "gdv_k_7ae13ad74296c1a6", "gdv_k_a641098839dd324a"],
}


@pytest.mark.parametrize("which", sorted(PARENT_KERNELS))
def test_baseline_kernels_keep_their_names(monkeypatch, tmp_path, which):
    from test_planner_cpu import _precompile
    schema, exprs = {"c2": (W.c2_schema, W.c2_expressions), "c4": (W.c4_schema, W.c4_expressions), "c5": (W.c5_schema, W.c5_expressions)}[which]
    files = _precompile(monkeypatch, tmp_path, schema(), exprs=exprs())
    names = set()
    for f in files:
        names |= set(re.findall(r"gdv_k_[0-9a-f]{16}", open(tmp_path / f).read()))
    assert sorted(names) == PARENT_KERNELS[which]


def test_tier0_still_refuses_a_decimal_plan():
    from test_tier0_coverage_cpu import _program
    b = gandiva.TreeExprBuilder()
    x = b.make_field(SCH.field("x"))
    prog, why = _program(SCH, [b.make_expression(b.make_function("castDECIMAL", [x], D(15, 2)), pa.field("o", D(15, 2)))])
    assert prog is None and "decimal128" in why, why
    d = b.make_field(SCH.field("d"))
    prog, why = _program(SCH, [b.make_expression(b.make_function("hash64", [d], I64), pa.field("o", I64))])
    assert prog is None and "decimal128" in why, why
