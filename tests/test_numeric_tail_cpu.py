"""The numeric tail without a GPU: sin cos tan asin acos atan sinh cosh tanh cot degrees radians atan2, sign, pmod, round /
truncate to a scale, shift_left / shift_right / shift_right_unsigned, gcd / lcm.

PARITY STATUS (PARITY.md, numeric tail): 2 engines for the arithmetic — the device functions and the independent reference of
tests/numeric_tail_reference.py (mpmath, Python integers, numpy float64) — and recollection + decisions for the rules.

This file checks
  * the reference's own sanity: math.* on exactly representable cases and the hand vectors of the issue;
  * the product's device functions compiled for the host (tests/host_devlib/host_numeric_tail.cc) against the reference on the
    4099-row batch: bit for bit, the libm-backed ones by class and ulp distance (the host's libm is glibc's, measured apart
    from the device's: numeric_tail_reference.HOST_MEASURED_ULPS);
  * the integer functions under AddressSanitizer / UBSan as a stand-alone child process (tests/cxx/numeric_tail_check.cc);
  * the registry (gandiva_amd and the rebuilt pyarrow.gandiva list the signatures);
  * Make: every signature cross-compiles for gfx950, with a per-row and with a literal second argument;
  * tier 0: every signature has a program in row mode and in selection mode;
  * plans without these functions mention none of the new symbols;
  * that the C++ test builds and its trees build."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pyarrow as pa
import pytest

import gandiva_amd as gandiva
import numeric_tail_reference as R
from helpers import assert_bit_exact
from test_tier0_coverage_cpu import _program, _program_selection

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "gandiva_amd", "csrc")
I32, I64, F32, F64 = pa.int32(), pa.int64(), pa.float32(), pa.float64()
FOUR = (I32, I64, F32, F64)
SUFFIX = {I32: "int32", I64: "int64", F32: "float32", F64: "float64"}
UNARY_F64 = ("sin", "cos", "tan", "asin", "acos", "atan", "sinh", "cosh", "tanh", "cot", "degrees", "radians")
# (name, parameter types, result type): the 84 signatures of the family
WANT = [(f, (t,), F64) for f in UNARY_F64 for t in FOUR] + [("atan2", (F64, F64), F64)] + [("sign", (t,), t) for t in FOUR] + \
       [(f, (t, t), t) for f in ("pmod",) for t in (I32, I64)] + [("round", (t,), t) for t in (I32, I64)] + \
       [(f, (t, I32), t) for f in ("round", "truncate", "shift_left", "shift_right", "shift_right_unsigned") for t in (I32, I64)] + \
       [("round", (F32, I32), F32), ("round", (F64, I32), F64), ("gcd", (I64, I64), I64), ("lcm", (I64, I64), I64)]
assert len(WANT) == 48 + 1 + 4 + 2 + 2 + 10 + 2 + 2


def _symbol(name, params):
    return name + "".join("_" + SUFFIX[p] for p in params)


# ------------------------------------------------------------------ 1. the reference's own sanity

def test_reference_on_exactly_representable_cases_and_against_math():
    one = R.libm_one
    assert one("sin", 0.0) == 0.0 and math.copysign(1, one("sin", -0.0)) == -1 and one("cos", 0.0) == 1.0 and one("tan", 0.0) == 0.0
    assert one("asin", 1.0) == math.pi / 2 and one("acos", 1.0) == 0.0 and one("acos", -1.0) == math.pi and one("atan", math.inf) == math.pi / 2
    assert one("asin", 0.5) == 0.5235987755982989 and one("acos", 0.5) == 1.0471975511965979      # pi/6 and pi/3, correctly rounded
    assert math.isnan(one("asin", 1.0000000000000002)) and math.isnan(one("acos", -2.0)) and math.isnan(one("sin", math.inf))
    assert one("sinh", 0.0) == 0.0 and one("cosh", 0.0) == 1.0 and one("tanh", 0.0) == 0.0 and one("tanh", 50.0) == 1.0 and one("tanh", -math.inf) == -1.0
    assert one("sinh", 711.0) == math.inf and one("sinh", -720.0) == -math.inf and one("cosh", -1e308) == math.inf
    assert 1.797e308 < one("sinh", 710.4758600739439) < math.inf and one("sinh", 710.475860073944) == math.inf
    assert one("sin", 5e-324) == 5e-324 and one("atan", -5e-324) == -5e-324 and one("tan", 2.2250738585072014e-308) == 2.2250738585072014e-308
    assert one("cot", 0.0) == one("tan", math.pi / 2) == 1.633123935319537e16               # cot(0): tan of the double pi/2
    assert one("sin", 1e22) == -0.8522008497671888                                            # the classic huge-argument case
    # within one ulp of the host's libm on ordinary arguments (math.* is not the reference: it only has to be near)
    rng = np.random.default_rng(3)
    for fn, lo, hi in (("sin", -10, 10), ("cos", -10, 10), ("tan", -1.5, 1.5), ("asin", -1, 1), ("acos", -1, 1), ("atan", -50, 50),
                       ("sinh", -20, 20), ("cosh", -20, 20), ("tanh", -5, 5)):
        x = rng.uniform(lo, hi, 200)
        got = np.array([one(fn, float(v)) for v in x])
        assert R.ulp_distances(got, np.array([getattr(math, fn)(float(v)) for v in x])).max() <= 2, fn
    a2 = R.atan2_one
    assert a2(0.0, 1.0) == 0.0 and a2(-0.0, -1.0) == -math.pi and a2(0.0, -0.0) == math.pi and math.copysign(1, a2(-0.0, 0.0)) == -1
    assert a2(1.0, 0.0) == math.pi / 2 and a2(math.inf, -math.inf) == 2.356194490192345 and a2(-1.0, math.inf) == 0.0 and a2(1.0, 1.0) == math.pi / 4
    assert math.isnan(a2(math.nan, 1.0)) and a2(5e-324, 1.0) == 5e-324 and a2(1.0, -0.125) == 1.695151321341658


def test_reference_on_the_hand_vectors_of_the_issue():
    assert R.pmod(-7, 3, "i32") == 2 and R.pmod(7, -3, "i32") == -2 and R.pmod(5, 0, "i32") == 5 and R.pmod(R.INT32_MIN, -1, "i32") == 0
    assert R.int_to_scale(125, -1, "i32", True) == 130 and R.int_to_scale(-125, -1, "i32", True) == -130
    assert R.int_to_scale(-125, -1, "i32", False) == -120
    assert R.int_to_scale(2147483647, -1, "i32", True) == R.wrap(2147483650, "i32") == -2147483646          # wraps, decided
    assert R.int_to_scale(7, -10, "i32", True) == 0 and R.int_to_scale(5 * 10 ** 18, -18, "i64", True) == 5 * 10 ** 18 and R.int_to_scale(7, -19, "i64", True) == 0
    f = lambda x, s: float(R.float_to_scale(np.array([x]), [s])[0])
    assert f(2.5, 0) == 3.0 and f(-0.125, 2) == -0.13 and f(1e308, 10) == 1e308 and f(1.5, 309) == 1.5
    assert f(-1.5, -309) == 0.0 and math.copysign(1, f(-1.5, -309)) == -1 and f(math.inf, 2) == math.inf and math.isnan(f(math.nan, -2))
    assert R.shift("shift_left", 1, 33, "i32") == 2 and R.shift("shift_right_unsigned", -1, 28, "i32") == 15
    assert R.shift("shift_right", -8, 1, "i64") == -4 and R.shift("shift_left", 1, -1, "i64") == -2 ** 63 and R.shift("shift_right", -8, 64, "i64") == -8
    assert R.gcd(-2 ** 63, 0) == -2 ** 63 and R.lcm(4, 6) == 12 and R.gcd(0, 0) == 0 and R.lcm(0, 9) == 0 and R.gcd(12, -18) == 6
    s = R.sign_float(np.array([-0.0, 0.0, -3.5, 7.0, np.nan]))
    assert s[0] == 0 and not np.signbit(s[0]) and list(s[1:4]) == [0.0, -1.0, 1.0] and np.isnan(s[4])
    assert [R.sign_int(v) for v in (-5, 0, 9)] == [-1, 0, 1]
    assert 180.0 * R.RAD == math.pi and R.DEG == 57.29577951308232


# ------------------------------------------------------------------ 2. the device functions on the host

@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_numeric_tail") / "libhost_numeric_tail.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unused-function", "-Wno-unused-variable",
                           "-Wno-attributes", os.path.join(HERE, "host_devlib", "host_numeric_tail.cc"), "-o", out])
    lib = C.CDLL(out)
    lib.host_call.restype = C.c_int
    return lib


def host_call(lib, name, arrays, ret):
    """the device function of a registry call over whole pyarrow arrays (no nulls) -> a pyarrow array"""
    cols = [np.ascontiguousarray(np.asarray(a)) for a in arrays]
    out = np.zeros(len(cols[0]), dtype=np.dtype(ret.to_pandas_dtype()))
    p = [c.ctypes.data_as(C.c_void_p) for c in cols] + [None]
    rc = lib.host_call(_symbol(name, [a.type for a in arrays]).encode(), p[0], p[1], out.ctypes.data_as(C.c_void_p), C.c_long(len(out)))
    assert rc == 0, "no device function " + _symbol(name, [a.type for a in arrays])
    return pa.array(out, ret)


@pytest.mark.parametrize("family", R.FAMILIES)
def test_host_build_matches_the_reference(hostlib, family):
    b = R.batch(0.0)
    for sp, want in zip(R.family_specs(family), R.expected_columns(family, 0.0)):
        got = host_call(hostlib, sp["fn"], [b.column(a) for a in sp["args"]], R.TYPES[sp["ret"]])
        if sp["ulps"] is None:
            assert_bit_exact(got, want, sp["label"])
        else:
            print("HOST ULP %s: %d" % (sp["label"], R.max_ulp_on_ordinary_rows(got, want)))
            R.assert_class_and_ulp(got, want, sp["host_ulps"], sp["label"])


def test_hand_vectors_on_the_host_build(hostlib):
    def one(name, args, types, ret):
        return host_call(hostlib, name, [pa.array([a], t) for a, t in zip(args, types)], ret)[0].as_py()
    assert one("pmod", (-7, 3), (I32, I32), I32) == 2 and one("pmod", (7, -3), (I32, I32), I32) == -2 and one("pmod", (5, 0), (I32, I32), I32) == 5
    assert one("pmod", (-2 ** 63, -1), (I64, I64), I64) == 0
    assert one("round", (125, -1), (I32, I32), I32) == 130 and one("round", (-125, -1), (I32, I32), I32) == -130
    assert one("truncate", (-125, -1), (I32, I32), I32) == -120 and one("round", (2147483647, -1), (I32, I32), I32) == -2147483646
    assert one("round", (2.5, 0), (F64, I32), F64) == 3.0 and one("round", (-0.125, 2), (F64, I32), F64) == -0.13
    assert one("round", (1e308, 10), (F64, I32), F64) == 1e308
    assert one("shift_left", (1, 33), (I32, I32), I32) == 2 and one("shift_right_unsigned", (-1, 28), (I32, I32), I32) == 15
    assert one("gcd", (-2 ** 63, 0), (I64, I64), I64) == -2 ** 63 and one("lcm", (4, 6), (I64, I64), I64) == 12
    s = one("sign", (-0.0,), (F64,), F64)
    assert s == 0.0 and math.copysign(1, s) == 1
    assert abs(one("cot", (0.0,), (F64,), F64) - math.tan(math.pi / 2)) <= 4.0            # two ulps of 1.6e16


# ------------------------------------------------------------------ 3. under sanitizers, as a child process

@pytest.mark.parametrize("name,extra", [("plain", []), ("asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"])])
def test_integer_functions_have_no_overflow_or_shift_ub(tmp_path, name, extra):
    exe = str(tmp_path / ("numeric_tail_check_" + name))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-unused-function", "-Wno-unused-variable", "-Wno-attributes"] +
                          extra + ["-I", CSRC, os.path.join(HERE, "cxx", "numeric_tail_check.cc"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, f"exit {run.returncode}\n{run.stdout}\n{run.stderr}"
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    assert "numeric_tail_check: ok" in run.stdout


# ------------------------------------------------------------------ 4. registry

def _check_registry(signatures):
    sigs = {(s.name(), tuple(s.param_types())): s.return_type() for s in signatures}
    for name, params, ret in WANT:
        assert sigs.get((name, params)) == ret, (name, params)
    names = {n for n, _, _ in WANT} - {"round", "truncate"}
    assert sum(1 for (name, _) in sigs if name in names) == sum(1 for n, _, _ in WANT if n in names)


def test_registry_lists_the_numeric_tail():
    _check_registry(gandiva.get_registered_function_signatures())


def test_registry_of_the_rebuilt_pyarrow_gandiva_lists_the_numeric_tail():
    from gandiva_amd import pyarrow_gandiva
    _check_registry(pyarrow_gandiva.load().get_registered_function_signatures())


# ------------------------------------------------------------------ 5. Make and tier 0

def _tree(b, name, params, ret, schema, literal_second=False):
    args = [b.make_field(schema.field(i)) for i in range(len(params))]
    if literal_second:
        args[1] = b.make_literal(-2 if name != "pmod" else 7, params[1])
    return b.make_function(name, args, ret)


@pytest.mark.parametrize("literal_second", [False, True], ids=["per_row", "literal"])
def test_every_signature_cross_compiles_for_gfx950(monkeypatch, tmp_path, literal_second):
    """one projector per parameter list (so that every signature sits in a plan), compiled for gfx950 by gdv_precompile_projector"""
    from test_planner_cpu import _precompile
    b = gandiva.TreeExprBuilder()
    by_params = {}
    for name, params, ret in WANT:
        if literal_second and (len(params) != 2 or name in ("atan2", "gcd", "lcm")):
            continue
        by_params.setdefault(params, []).append((name, ret))
    for k, (params, fns) in enumerate(sorted(by_params.items(), key=str)):
        schema = pa.schema([(f"c{i}", p) for i, p in enumerate(params)])
        exprs = [b.make_expression(_tree(b, name, params, ret, schema, literal_second), pa.field(f"r{j}", ret)) for j, (name, ret) in enumerate(fns)]
        d = tmp_path / str(k)
        d.mkdir()
        files = _precompile(monkeypatch, d, schema, exprs=exprs)
        text = "".join(open(d / f).read() for f in files).split('#include "gdv_device_lib.hpp"')[-1]
        for name, _ in fns:
            assert _symbol(name, params) + "(" in text, (name, params)


def test_every_signature_has_a_tier0_program_in_row_mode_and_selection_mode():
    b = gandiva.TreeExprBuilder()
    for name, params, ret in WANT:
        schema = pa.schema([(f"c{i}", p) for i, p in enumerate(params)])
        for literal_second in ([False, True] if len(params) == 2 and name not in ("atan2", "gcd", "lcm") else [False]):
            exprs = [b.make_expression(_tree(b, name, params, ret, schema, literal_second), pa.field("r", ret))]
            prog, why = _program(schema, exprs)
            assert prog is not None and "call " + _symbol(name, params) in prog, (name, params, why)
            assert len(prog) == len(params) + 2
            for mode, width in ((1, 16), (2, 32), (3, 64)):
                sel, why = _program_selection(schema, exprs, mode)
                assert sel == [f"select uint{width}"] + prog, (name, params, why)
    # the filter of the issue: sign(pmod(a, 7) - 3) = 1
    schema = pa.schema([("a", I32)])
    a = b.make_field(schema.field(0))
    cond = b.make_condition(b.make_function("equal", [b.make_function("sign", [b.make_function("subtract", [
        b.make_function("pmod", [a, b.make_literal(7, I32)], I32), b.make_literal(3, I32)], I32)], I32), b.make_literal(1, I32)], pa.bool_()))
    prog, why = _program(schema, [cond], 1)
    assert prog == ["load in0 int32", "lit #0 = 0x7", "call pmod_int32_int32", "lit #1 = 0x3", "subtract int32", "call sign_int32", "lit #2 = 0x1",
                    "compare eq int32", "filter"], (prog, why)


NEW_SYMBOLS = tuple(sorted({_symbol(n, p) + "(" for n, p, _ in WANT})) + ("gdv_cot", "gdv_pow10", "gdv_to_scale", "gdv_gcd_u64", "atan2")


def test_a_plan_without_these_functions_mentions_none_of_the_new_symbols(monkeypatch, tmp_path):
    from gandiva_amd import workloads as W
    from test_planner_cpu import _precompile
    b = gandiva.TreeExprBuilder()
    schema = pa.schema([("a", I32), ("l", I64), ("x", F64)])
    a, l, x = (b.make_field(schema.field(i)) for i in range(3))
    mixed = [b.make_expression(b.make_function("round", [x], F64), pa.field("r", F64)),
             b.make_expression(b.make_function("truncate", [x], F64), pa.field("t", F64)),
             b.make_expression(b.make_function("mod", [l, a], I32), pa.field("m", I32)),
             b.make_expression(b.make_function("power", [x, x], F64), pa.field("p", F64)),
             b.make_expression(b.make_function("bitwise_and", [a, a], I32), pa.field("b", I32))]
    for k, (sch, exprs) in enumerate(((schema, mixed), (W.c2_schema(), W.c2_expressions()))):
        d = tmp_path / str(k)
        d.mkdir()
        files = _precompile(monkeypatch, d, sch, exprs=exprs)
        assert files
        for f in files:
            assert re.fullmatch(r"gdv_k_[0-9a-f]{16}\.hip", f)
            body = open(d / f).read().split('#include "gdv_device_lib.hpp"')[-1]
            assert not any(sym in body for sym in NEW_SYMBOLS), [sym for sym in NEW_SYMBOLS if sym in body]


# ------------------------------------------------------------------ 6. the C++ API

def test_cxx_numeric_tail_builds_its_trees_host_only():
    """gandiva_amd/cxx/tests/test_numeric_tail_cxx.cc: it builds, the trees build, gandiva::ExpressionRegistry lists the family"""
    cxx = os.path.join(HERE, "..", "gandiva_amd", "cxx")
    subprocess.check_call(["make", "-C", cxx, "all", "test_cxx"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(cxx, "tests", "test_numeric_tail_cxx"), "--host-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "OK (host-only)" in out.stdout, out.stdout + out.stderr
