"""The calendar tail without a GPU: months_between, next_day, add_months, date_trunc('unit', t) and the extractor names
year month day dayofmonth dayofyear dayofweek quarter hour minute second.

PARITY STATUS (PARITY.md, calendar tail): 2 engines for the arithmetic — the device functions and the independent reference
of tests/calendar_tail_reference.py (Python integers and floats over temporal_reference's exact calendar) — and
recollection + decisions for the rules.

This file checks
  * the reference's own sanity: next_day against datetime.date.weekday() over years 1..9999, months_between against the hand
    vector of Hive's documentation and against dateutil.relativedelta for the whole-month cases;
  * the left-out share of every expression, on the reference alone: a row is left out only where the exact result leaves
    int64, nothing for months_between and the extractor names, at most temporal_reference.MAX_LEFT_OUT anywhere;
  * the product's device functions compiled for the host (tests/host_devlib/host_calendar_tail.cc) against the reference on
    the 4099-row batches, bit for bit, float64 results included;
  * the functions under AddressSanitizer / UBSan as a stand-alone child process (tests/cxx/calendar_tail_check.cc);
  * the registry; the tier-0 program text: one `call` per signature, date_trunc('MoNtH', ts) gives date_trunc_Month(ts)'s
    program, next_day(t, 'name') gives next_day(t, number)'s, each alias its target's, in row mode and selection mode;
  * Make: every signature cross-compiles for gfx950; the generated text of a rewritten node is that of its target;
  * the Make errors and their wording: unknown and per-row day names and units; NULL literals;
  * that the C++ test builds, its trees build and Make refuses a per-row name through gandiva::Projector;
  * that no function of the tier-0 kernel's translation unit comes near 128 KiB of code (the call switch stays in parts)."""
import ctypes as C
import datetime as dt
import os
import subprocess

import numpy as np
import pyarrow as pa
import pytest

import calendar_tail_reference as R
import gandiva_amd as gandiva
import temporal_reference as T
from helpers import assert_bit_exact_where
from test_tier0_coverage_cpu import _program, _program_selection

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "gandiva_amd", "csrc")
MS = R.MS
I32, I64, F64, STR = pa.int32(), pa.int64(), pa.float64(), pa.string()
D32, D64, TS, T32 = pa.date32(), pa.date64(), pa.timestamp("ms"), pa.time32("ms")
SUFFIX = {I32: "int32", I64: "int64", D32: "date32", D64: "date64", TS: "timestamp", T32: "time32"}
# (name, parameter types, result type, the symbol of the device function): the 41 signatures of the family
WANT = [("months_between", (t, t), F64, None) for t in (D64, TS)] + [("next_day", (t, I32), D64, None) for t in (D64, TS)] + \
       [("add_months", (t, n), t, None) for t in (D64, TS) for n in (I32, I64)] + \
       [(alias, (t,), I64, target) for alias, target in R.ALIASES.items() for t in (D32, D64, TS, T32) if t != T32 or alias in R.TIME_ALIASES]
assert len(WANT) == 2 + 2 + 4 + 7 * 3 + 3 * 4


def _symbol(name, params, target=None):
    return (target or name) + "".join("_" + SUFFIX[p] for p in params)


def _ms(y, m, d, tod=0):
    return T.day_of(y, m, d) * MS + tod


# ------------------------------------------------------------------ 1. the reference's own sanity

def test_reference_next_day_against_datetime_over_years_1_to_9999():
    first, last = dt.date(1, 1, 1).toordinal(), dt.date(9999, 12, 31).toordinal() - 7
    epoch = dt.date(1970, 1, 1).toordinal()
    for k, o in enumerate(range(first, last, 37)):      # every 37th day: each weekday in turn, each wanted day in turn
        dow = k % 9 - 1                                  # -1 .. 7: below and at the ends of 1..7 too
        r = R.next_day((o - epoch) * MS + (k * 7919) % MS, dow)
        assert r % MS == 0
        got = dt.date.fromordinal(r // MS + epoch)
        assert 1 <= got.toordinal() - o <= 7 and (got.weekday() + 1) % 7 + 1 == (dow - 1) % 7 + 1, (o, dow, got)
    assert R.next_day(_ms(2015, 1, 14), 3) == _ms(2015, 1, 20)                      # the hand vector: a Wednesday's next Tuesday
    assert R.next_day(_ms(2015, 1, 20, MS - 1), 3) == _ms(2015, 1, 27)              # strictly later
    assert R.next_day(_ms(2015, 1, 14), 3 + 7 * 1000) == R.next_day(_ms(2015, 1, 14), 3 - 7 * 1000) == _ms(2015, 1, 20)
    assert R.next_day(T.I64_MAX, 1) is None and R.next_day(T.I64_MAX - 8 * MS, 1) is not None
    for v in (T.I64_MIN, T.I64_MAX - 8 * MS, -1, 0):                                # the ends of int64: extractDow's reference agrees
        for dow in range(1, 8):
            r = R.next_day(v, dow)
            assert T.extract("Dow", "ts", r) == dow and r % MS == 0 and 1 <= r // MS - v // MS <= 7


def test_reference_months_between_on_the_hand_vector_and_against_relativedelta():
    from dateutil.relativedelta import relativedelta
    hand = R.months_between(_ms(1997, 2, 28, 37800000), _ms(1996, 10, 30))
    assert hand == 4 + (-2 + 0.4375) / 31 and abs(hand - 3.94959677) < 1e-8
    assert R.months_between(_ms(2015, 2, 28, 5), _ms(2015, 1, 31, 999)) == 1.0       # both the last of their months
    assert R.months_between(_ms(2015, 3, 30), _ms(2015, 2, 28)) == 1 + 2 / 31        # only one is
    assert R.months_between(T.I64_MAX, T.I64_MIN) == -R.months_between(T.I64_MIN, T.I64_MAX)
    rng = np.random.default_rng(7)
    epoch = dt.datetime(1970, 1, 1)
    to_ms = lambda t: (t - epoch) // dt.timedelta(milliseconds=1)
    whole = 0
    for _ in range(4000):
        start = dt.datetime(2000, 1, 1) + dt.timedelta(milliseconds=int(rng.integers(0, T.CYCLE * MS)))
        k = int(rng.integers(-5000, 5001))
        if not 1 <= start.year + k // 12 <= 9990:
            continue
        end = start + relativedelta(months=k) + dt.timedelta(milliseconds=int(rng.integers(-3600000, 3600000)))
        if end.day != start.day and not (T.last_dom(end.year, end.month) == end.day and T.last_dom(start.year, start.month) == start.day):
            continue
        whole += 1
        assert R.months_between(to_ms(end), to_ms(start)) == float(k) and R.months_between(to_ms(start), to_ms(end)) == float(-k)
    assert whole > 3000


# ------------------------------------------------------------------ 2. the left-out share, on the reference alone

@pytest.mark.parametrize("family", R.FAMILIES)
def test_rows_are_left_out_only_where_the_exact_result_leaves_int64(family):
    for nulls in (0.0, 0.1):
        b = R.batch(nulls)
        for sp, left_out in zip(R.family_specs(family), R.left_out_columns(family, nulls)):
            valid = np.logical_and.reduce([np.asarray(b.column(a).is_valid()) for a in sp["args"] if isinstance(a, str)])
            share = left_out.sum() / max(valid.sum(), 1)
            assert share <= T.MAX_LEFT_OUT, (sp["label"], share)
            if family == "months_between" or sp["fn"] in R.ALIASES:
                assert not left_out.any(), sp["label"]
            if sp["fn"] == "next_day":           # exactly the inputs within 7 days of INT64_MAX whose exact result is past it
                v = np.array(T.column_values(b.column(sp["args"][0]), R.arg_type(sp["args"][0])), dtype=object)
                assert all(int(x) // MS + 7 > T.I64_MAX // MS for x in v[left_out]), sp["label"]
            if sp["fn"] == "add_months":         # timestampaddMonth's rule, by its own reference
                twin = T._spec("timestampaddMonth", [sp["args"][1] if isinstance(sp["args"][1], str) else T._lit(sp["args"][1]["lit"], "i64"), sp["args"][0]],
                               sp["ret"])
                if R.arg_type(sp["args"][1]) == "i64":
                    assert np.array_equal(T.expected_of(twin, b)[1], left_out), sp["label"]


# ------------------------------------------------------------------ 3. the device functions on the host

@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_calendar_tail") / "libhost_calendar_tail.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unused-function", "-Wno-unused-variable",
                           "-Wno-attributes", os.path.join(HERE, "host_devlib", "host_calendar_tail.cc"), "-o", out])
    lib = C.CDLL(out)
    lib.host_call.restype = C.c_int
    return lib


def host_call(lib, symbol, columns, ret):
    """a device function by its symbol over dense numpy columns -> a numpy array of the storage type of `ret`"""
    cols = [np.ascontiguousarray(c) for c in columns]
    out = np.zeros(len(cols[0]), dtype=np.dtype(T.STORAGE[ret].to_pandas_dtype()))
    p = [c.ctypes.data_as(C.c_void_p) for c in cols] + [None]
    assert lib.host_call(symbol.encode(), p[0], p[1], out.ctypes.data_as(C.c_void_p), C.c_long(len(out))) == 0, "no device function " + symbol
    return out


@pytest.mark.parametrize("family", R.FAMILIES)
def test_host_build_matches_the_reference_bit_for_bit(hostlib, family):
    b = R.batch(0.0)
    n = b.num_rows
    for sp, (want, left_out) in zip(R.family_specs(family), R.expected_pairs(family, 0.0)):
        cols = []
        for a in sp["host"]["args"]:
            tn = R.arg_type(a)
            dtype = np.dtype(T.STORAGE[tn].to_pandas_dtype())
            cols.append(np.asarray(b.column(a).view(T.STORAGE[tn])) if isinstance(a, str) else np.full(n, a["lit"], dtype=dtype))
        got = host_call(hostlib, sp["host"]["symbol"], cols, sp["ret"])
        assert_bit_exact_where(pa.array(got, T.STORAGE[sp["ret"]]).view(R.TYPES[sp["ret"]]), want, ~left_out, sp["label"])


def test_hand_vectors_on_the_host_build(hostlib):
    one = lambda symbol, a, b, ret, tb=np.int64: host_call(hostlib, symbol, [np.array([a], dtype=np.int64), np.array([b], dtype=tb)], ret)[0]
    assert one("months_between_timestamp_timestamp", _ms(1997, 2, 28, 37800000), _ms(1996, 10, 30), "f64") == 4 + (-2 + 0.4375) / 31
    assert one("next_day_date64_int32", _ms(2015, 1, 14), 3, "d64", np.int32) == _ms(2015, 1, 20)
    assert one("next_day_timestamp_int32", _ms(2015, 1, 14, 5), -(1 << 31), "d64", np.int32) == R.next_day(_ms(2015, 1, 14), -(1 << 31))
    assert one("add_months_date64_int32", _ms(2023, 1, 31, 7), 1, "d64", np.int32) == _ms(2023, 2, 28, 7)
    assert one("add_months_timestamp_int64", _ms(2024, 2, 29), -12, "ts") == _ms(2023, 2, 28)


# ------------------------------------------------------------------ 4. under sanitizers, as a child process

@pytest.mark.parametrize("name,extra", [("plain", []), ("asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"])])
def test_no_overflow_or_other_undefined_behaviour_on_the_edge_rows(tmp_path, name, extra):
    exe = str(tmp_path / ("calendar_tail_check_" + name))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-unused-function", "-Wno-unused-variable", "-Wno-attributes"] +
                          extra + ["-I", CSRC, os.path.join(HERE, "cxx", "calendar_tail_check.cc"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, f"exit {run.returncode}\n{run.stdout}\n{run.stderr}"
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    assert "calendar_tail_check: ok" in run.stdout


# ------------------------------------------------------------------ 5. registry

def _check_registry(signatures):
    sigs = {(s.name(), tuple(s.param_types())): s.return_type() for s in signatures}
    for name, params, ret, _ in WANT:
        assert sigs.get((name, params)) == ret, (name, params)
    names = {n for n, _, _, _ in WANT}
    assert sum(1 for (name, _) in sigs if name in names) == len(WANT)
    assert not any(name == "date_trunc" for name, _ in sigs)        # a rewrite, not a signature (a text one would need a kernel)


def test_registry_lists_the_calendar_tail():
    _check_registry(gandiva.get_registered_function_signatures())


def test_registry_of_the_rebuilt_pyarrow_gandiva_lists_the_calendar_tail():
    from gandiva_amd import pyarrow_gandiva
    _check_registry(pyarrow_gandiva.load().get_registered_function_signatures())


# ------------------------------------------------------------------ 6. tier 0 and Make

def _one(b, node, t):
    return [b.make_expression(node, pa.field("r", t))]


def test_every_signature_is_one_call_in_row_mode_and_selection_mode():
    b = gandiva.TreeExprBuilder()
    for name, params, ret, target in WANT:
        schema = pa.schema([(f"c{i}", p) for i, p in enumerate(params)])
        for literal_second in ([False, True] if name in ("next_day", "add_months") else [False]):
            args = [b.make_field(schema.field(i)) for i in range(len(params))]
            if literal_second:
                args[1] = b.make_literal(-13, params[1])
            exprs = _one(b, b.make_function(name, args, ret), ret)
            prog, why = _program(schema, exprs)
            assert prog is not None and prog.count("call " + _symbol(name, params, target)) == 1, (name, params, why)
            assert len(prog) == len(params) + 2 and sum(p.startswith("call ") for p in prog) == 1
            for mode, width in ((1, 16), (2, 32), (3, 64)):
                sel, why = _program_selection(schema, exprs, mode)
                assert sel == [f"select uint{width}"] + prog, (name, params, why)


def test_each_alias_gives_its_targets_program():
    b = gandiva.TreeExprBuilder()
    for alias, params, ret, target in WANT:
        if target is None:
            continue
        schema = pa.schema([("c0", params[0])])
        c = b.make_field(schema.field(0))
        assert _program(schema, _one(b, b.make_function(alias, [c], ret), ret))[0] == _program(schema, _one(b, b.make_function(target, [c], ret), ret))[0] \
            == ["load in0 " + ("int32" if params[0] in (D32, T32) else "int64"), "call " + _symbol(target, params), "out0 int64"]


def test_a_literal_unit_and_a_literal_day_name_give_the_programs_of_their_targets():
    b = gandiva.TreeExprBuilder()
    for t in (D64, TS):
        schema = pa.schema([("t", t)])
        c = b.make_field(schema.field(0))
        want = _program(schema, _one(b, b.make_function("date_trunc_Month", [c], t), t))[0]
        assert want == ["load in0 int64", "call date_trunc_Month_" + SUFFIX[t], "out0 int64"]
        assert _program(schema, _one(b, b.make_function("date_trunc", [b.make_literal("MoNtH", STR), c], t), t))[0] == want
        for unit in T.TRUNC_UNITS:
            for text in (unit, unit.lower(), unit.upper()):
                prog, why = _program(schema, _one(b, b.make_function("date_trunc", [b.make_literal(text, STR), c], t), t))
                assert prog == ["load in0 int64", "call date_trunc_%s_%s" % (unit, SUFFIX[t]), "out0 int64"], (text, why)
        for n, names in R.DAY_NAMES.items():
            want = _program(schema, _one(b, b.make_function("next_day", [c, b.make_literal(n, I32)], D64), D64))[0]
            assert want == ["load in0 int64", "lit #0 = 0x%x" % n, "call next_day_%s_int32" % SUFFIX[t], "out0 int64"]
            for name in names:
                for text in (name, name.lower(), name.capitalize()):
                    assert _program(schema, _one(b, b.make_function("next_day", [c, b.make_literal(text, STR)], D64), D64))[0] == want, text


def _generated(monkeypatch, d, schema, exprs):
    from test_planner_cpu import _precompile
    d.mkdir()
    files = _precompile(monkeypatch, d, schema, exprs=exprs)
    assert files
    return files, "".join(open(d / f).read() for f in files).split('#include "gdv_device_lib.hpp"')[-1]


def test_every_signature_cross_compiles_for_gfx950(monkeypatch, tmp_path):
    """one projector per parameter list (so that every signature sits in a plan), compiled for gfx950 by gdv_precompile_projector"""
    b = gandiva.TreeExprBuilder()
    by_params = {}
    for name, params, ret, target in WANT:
        by_params.setdefault(params, []).append((name, ret, target))
    for k, (params, fns) in enumerate(sorted(by_params.items(), key=str)):
        schema = pa.schema([(f"c{i}", p) for i, p in enumerate(params)])
        exprs = [b.make_expression(b.make_function(name, [b.make_field(schema.field(i)) for i in range(len(params))], ret), pa.field(f"r{j}", ret))
                 for j, (name, ret, _) in enumerate(fns)]
        _, text = _generated(monkeypatch, tmp_path / str(k), schema, exprs)
        for name, _, target in fns:
            assert _symbol(name, params, target) + "(" in text, (name, params)


def test_a_rewritten_node_generates_the_kernel_of_its_target(monkeypatch, tmp_path):
    b = gandiva.TreeExprBuilder()
    schema = pa.schema([("t", TS)])
    c = b.make_field(schema.field(0))
    pairs = [(b.make_function("date_trunc", [b.make_literal("qUARTER", STR), c], TS), b.make_function("date_trunc_Quarter", [c], TS), TS),
             (b.make_function("next_day", [c, b.make_literal("Sat", STR)], D64), b.make_function("next_day", [c, b.make_literal(7, I32)], D64), D64),
             (b.make_function("dayofweek", [c], I64), b.make_function("extractDow", [c], I64), I64)]
    for k, (written, target, ret) in enumerate(pairs):
        files_w, text_w = _generated(monkeypatch, tmp_path / ("w%d" % k), schema, _one(b, written, ret))
        files_t, text_t = _generated(monkeypatch, tmp_path / ("t%d" % k), schema, _one(b, target, ret))
        assert files_w == files_t and text_w == text_t, k        # the same kernel under the same cache key


# ------------------------------------------------------------------ 7. what Make refuses, and NULL literals

DAY_FORMS = "SU MO TU WE TH FR SA, SUN MON TUE WED THU FRI SAT, SUNDAY MONDAY TUESDAY WEDNESDAY THURSDAY FRIDAY SATURDAY"
UNIT_FORMS = "second minute hour day week month quarter year decade century millennium"


@pytest.mark.parametrize("t", [D64, TS], ids=["date64", "timestamp"])
def test_make_refuses_unknown_and_per_row_names_and_units_and_says_what_it_takes(t):
    schema = pa.schema([("t", t), ("w", STR)])
    b = gandiva.TreeExprBuilder()
    c, w = b.make_field(schema.field(0)), b.make_field(schema.field(1))
    lit = lambda s: b.make_literal(s, STR)
    refused = [(b.make_function("next_day", [c, arg], D64), D64, "next_day", DAY_FORMS) for arg in (w, lit("Tuesdays"), lit(" tue"), lit("tue "), lit(""), lit("T"), lit("3"))] + \
              [(b.make_function("date_trunc", [arg, c], t), t, "date_trunc", UNIT_FORMS) for arg in (w, lit("months"), lit(" month"), lit("month "), lit(""), lit("fortnight"))]
    for node, ret, name, forms in refused:
        for make in (lambda e: gandiva.make_projector(schema, e, pa.default_memory_pool()),
                     lambda e: gandiva.make_projector(schema, e, pa.default_memory_pool(), "UINT32")):
            with pytest.raises(Exception) as err:
                make(_one(b, node, ret))
            text = str(err.value)
            assert "CodeGenError" in type(err.value).__name__ + text and name + "(" in text and forms in text and "LITERAL" in text, text
        assert _program(schema, _one(b, node, ret))[0] is None
    # (a filter over one of them is refused in the same words)
    cond = b.make_condition(b.make_function("less_than", [b.make_function("next_day", [c, w], D64), b.make_function("castDATE", [c], D64) if t == TS else c], pa.bool_()))
    with pytest.raises(Exception, match="next_day.*LITERAL day name"):
        gandiva.make_filter(schema, cond)


def test_null_literals_give_calls_whose_every_row_is_null():
    b = gandiva.TreeExprBuilder()
    for t in (D64, TS):
        schema = pa.schema([("t", t)])
        c = b.make_field(schema.field(0))
        for node, ret in ((b.make_function("next_day", [c, b.make_null(STR)], D64), D64), (b.make_function("date_trunc", [b.make_null(STR), c], t), t),
                          (b.make_function("next_day", [c, b.make_null(I32)], D64), D64), (b.make_function("add_months", [c, b.make_null(I64)], t), t)):
            prog, why = _program(schema, _one(b, node, ret))
            assert prog is not None and len(prog) == 4 and prog[0] == "load in0 int64" and "null" in prog[1] and prog[2].startswith("call "), (prog, why)


# ------------------------------------------------------------------ 8. the C++ API

def test_cxx_calendar_tail_builds_its_trees_host_only():
    """gandiva_amd/cxx/tests/test_calendar_tail_cxx.cc: it builds, the trees build, gandiva::ExpressionRegistry lists the family and
    gandiva::Projector::Make refuses a per-row day name"""
    cxx = os.path.join(HERE, "..", "gandiva_amd", "cxx")
    subprocess.check_call(["make", "-C", cxx, "all", "test_cxx"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(cxx, "tests", "test_calendar_tail_cxx"), "--host-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "OK (host-only)" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------ 9. the interpreter's out-of-line call switch stays in parts

def test_no_part_of_the_tier0_call_switch_comes_near_the_reach_of_a_short_branch(tmp_path):
    """gdv_tier0.hip: past 128 KiB of code in one function the compiler expands long branches through s[30:31], which hold a
    leaf function's return address; the call then never returns.  The one switch over every function id reached 140 760 bytes
    with this family's eight cases and hung every interpreted call of a low id, so the switch is cut into parts: every function
    of the translation unit stays below 96 KiB and no long branch is expanded anywhere."""
    import re
    asm = str(tmp_path / "gdv_tier0.s")
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")      # (as gandiva_amd/csrc/Makefile finds it)
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off",
                           "-fhip-fp32-correctly-rounded-divide-sqrt", "--cuda-device-only", "-S", os.path.join(CSRC, "gdv_tier0.hip"), "-o", asm],
                          stderr=subprocess.DEVNULL)
    text = open(asm).read()
    sizes = [int(m) for m in re.findall(r"; codeLenInByte = (\d+)", text)]
    assert len(sizes) >= 5 and text.count("CallPart") >= 4, sizes          # the parts and the four kernel instantiations
    assert max(sizes) < 96 * 1024, sizes
    assert "s_getpc_b64 s[30:31]" not in text
