"""The numeric tail on the GPU: trigonometry and angles, sign, pmod, round / truncate to a scale, shifts, gcd / lcm against
the independent reference of tests/numeric_tail_reference.py — bit for bit, the libm-backed functions by class and ulp
distance from the correctly rounded value.

Every family runs over the 4099-row batches (null share 0 and 0.1) in ONE fresh child process per path, with the machinery
of tests/full_range_child.py: with GDV_NO_TIER0=1 on the specialised kernels and with GDV_FORCE_TIER0=1 on the interpreter,
where every evaluation must raise gdv_tier0_launches() by one; the two paths' results are then held to each other bit for
bit.  The remaining tests run in this process: a projector of mixed functions on short and sliced batches, selection mode
behind the filter sign(pmod(a, 7) - 3) = 1 on host and device batches, a literal against a per-row scale, the hand vectors
and the C++ API.

Measured on an MI355X (profiles/numeric_tail.txt): every libm-backed function of the family stays within 1 ulp of the
correctly rounded value on every domain column, on both paths."""
import os
import subprocess

import numpy as np
import pyarrow as pa
import pytest

import gandiva_amd as gandiva
import numeric_tail_reference as R
from full_range_child import NULLS, run_child, write_case
from helpers import assert_bit_exact

pytestmark = pytest.mark.gpu
I32, I64, F32, F64, BOOL = pa.int32(), pa.int64(), pa.float32(), pa.float64(), pa.bool_()


@pytest.fixture(scope="module")
def case_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("numeric_tail")


@pytest.mark.parametrize("family", R.FAMILIES)
def test_family_matches_the_reference_on_both_paths_and_the_paths_agree(case_dir, family):
    case = write_case(R, case_dir, family, R.family_specs(family), {nulls: R.expected_columns(family, nulls) for nulls in NULLS})
    run_child("numeric_tail_child", case, interpreted=False)
    run_child("numeric_tail_child", case, interpreted=True)
    for nulls in NULLS:
        path = str(case_dir / ("%s_%s.arrow" % (family, nulls)))
        spec = pa.ipc.open_file(path + ".specialised").read_all().combine_chunks()
        tier0 = pa.ipc.open_file(path + ".tier0").read_all().combine_chunks()
        assert spec.column_names == tier0.column_names == [sp["label"] for sp in R.family_specs(family)]
        for name in spec.column_names:
            assert_bit_exact(tier0.column(name).chunk(0), spec.column(name).chunk(0), "interpreter against specialised kernel: %s nulls=%s" % (name, nulls))


MIXED = [R._spec("sin", ["t_dense"], "f64", ulps=R.BAR), R._spec("atan2", ["f64_a", "f64_b"], "f64", ulps=R.BAR), R._spec("degrees", ["i64_a"], "f64"),
         R._spec("sign", ["f32_a"], "f32"), R._spec("pmod", ["i64_a", "i64_b"], "i64"), R._spec("round", ["s_f64", "sc"], "f64"),
         R._spec("truncate", ["s_i32", "sc"], "i32"), R._spec("shift_right", ["s_i64", "sc"], "i64"), R._spec("gcd", ["i64_a", "i64_b"], "i64"),
         R._spec("cot", ["i32_a"], "f64", ulps=R.BAR)]


@pytest.fixture(scope="module")
def mixed():
    return gandiva.make_projector(R.SCHEMA, R.build_expressions(gandiva, MIXED), pa.default_memory_pool())


@pytest.mark.parametrize("offset", [1, 65])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 1025])
def test_one_projector_of_mixed_functions_on_short_and_sliced_batches(mixed, rows, offset):
    part = R.batch(0.1).slice(offset, rows)
    got = mixed.evaluate(part)
    for sp, g in zip(MIXED, got):
        want = R.expected_of(sp, part)
        what = "%s offset=%d rows=%d" % (sp["label"], offset, rows)
        if sp["ulps"] is None:
            assert_bit_exact(g, want, what)
        else:
            R.assert_class_and_ulp(g, want, sp["ulps"], what)


def _predicate(b, a):
    """sign(pmod(a, 7) - 3) = 1"""
    return b.make_function("equal", [b.make_function("sign", [b.make_function("subtract", [
        b.make_function("pmod", [a, b.make_literal(7, I32)], I32), b.make_literal(3, I32)], I32)], I32), b.make_literal(1, I32)], BOOL)


def _selected(batch):
    a = batch.column("i32_a")
    return np.array([i for i, v in enumerate(a.to_pylist()) if v is not None and v % 7 - 3 > 0], dtype=np.int64)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("mode,dtype", [("UINT16", "int16"), ("UINT32", "int32")])
def test_filter_and_selection_mode_behind_it(mode, dtype, where):
    batch = R.batch(0.1)
    b = gandiva.TreeExprBuilder()
    flt = gandiva.make_filter(R.SCHEMA, b.make_condition(_predicate(b, b.make_field(R.SCHEMA.field("i32_a")))))
    proj = gandiva.make_projector(R.SCHEMA, R.build_expressions(gandiva, MIXED), pa.default_memory_pool(), mode)
    want_idx = _selected(batch)
    assert 0 < len(want_idx) < len(batch)
    if where == "host":
        sel = flt.evaluate(batch, pa.default_memory_pool(), dtype)
        assert np.array_equal(sel.to_array().to_numpy().astype(np.int64), want_idx)
        got = proj.evaluate(batch, sel)
    else:
        db = gandiva.DeviceBatch.from_arrow(batch)
        sel = flt.evaluate_device(db, dtype)
        assert np.array_equal(sel.to_array().to_numpy().astype(np.int64), want_idx)
        got = [o.to_arrow() for o in proj.evaluate_device(db, selection=sel)]
    taken = batch.take(pa.array(want_idx))
    for sp, g in zip(MIXED, got):
        want = R.expected_of(sp, taken)
        if sp["ulps"] is None:
            assert_bit_exact(g, want, "%s %s %s" % (sp["label"], mode, where))
        else:
            R.assert_class_and_ulp(g, want, sp["ulps"], "%s %s %s" % (sp["label"], mode, where))


def test_a_literal_and_a_per_row_scale_give_identical_bits():
    batch = R.batch(0.1)
    b = gandiva.TreeExprBuilder()
    for k in (2, -1, 31):
        const = pa.array(np.full(len(batch), k, dtype=np.int32))
        full = pa.RecordBatch.from_arrays(batch.columns + [const], schema=R.SCHEMA.append(pa.field("k", I32)))
        kcol = b.make_field(full.schema.field("k"))
        exprs = []
        for fn, col, t in (("round", "s_f64", F64), ("round", "f32_a", F32), ("round", "i32_a", I32), ("truncate", "i64_a", I64), ("shift_left", "i32_a", I32),
                           ("shift_right", "i64_a", I64), ("shift_right_unsigned", "i64_a", I64)):
            x = b.make_field(full.schema.field(col))
            exprs += [b.make_expression(b.make_function(fn, [x, b.make_literal(k, I32)], t), pa.field("lit_%s_%s" % (fn, col), t)),
                      b.make_expression(b.make_function(fn, [x, kcol], t), pa.field("row_%s_%s" % (fn, col), t))]
        got = gandiva.make_projector(full.schema, exprs, pa.default_memory_pool()).evaluate(full)
        for i in range(0, len(got), 2):
            assert_bit_exact(got[i], got[i + 1], "literal against per-row %d: expression %d" % (k, i // 2))


def test_hand_vectors():
    sch = pa.schema([("a", I32), ("n", I32), ("l", I64), ("m", I64), ("x", F64), ("s", I32)])
    batch = pa.RecordBatch.from_arrays([pa.array([-7, 7, 5, 125, -125, 1, -1, 2147483647], I32), pa.array([3, -3, 0, -1, -1, 33, 28, -1], I32),
                                        pa.array([-2 ** 63, 4, 0, 12, -2 ** 63, 7, 0, 9], I64), pa.array([0, 6, 0, -18, -1, 0, 5, 9], I64),
                                        pa.array([2.5, -0.125, 1e308, -0.0, 0.0, np.nan, -3.0, 0.0], F64), pa.array([0, 2, 10, 0, 0, 0, 0, 0], I32)], schema=sch)
    b = gandiva.TreeExprBuilder()
    f = {x.name: b.make_field(x) for x in sch}
    exprs = [("pmod", ["a", "n"], I32, [2, -2, 5, 0, 0, 1, 27, 0]), ("round", ["a", "n"], I32, [-7, 0, 5, 130, -130, 1, -1, -2147483646]),
             ("truncate", ["a", "n"], I32, [-7, 0, 5, 120, -120, 1, -1, 2147483640]), ("shift_left", ["a", "n"], I32, [-56, -536870912, 5, -2 ** 31, -2 ** 31, 2, -2 ** 28, -2 ** 31]),
             ("shift_right_unsigned", ["a", "n"], I32, [(2 ** 32 - 7) >> 3, 0, 5, 0, 1, 0, 15, 0]),
             ("gcd", ["l", "m"], I64, [-2 ** 63, 2, 0, 6, 1, 7, 5, 9]), ("lcm", ["l", "m"], I64, [0, 12, 0, 36, -2 ** 63, 0, 0, 9]),
             ("round", ["x", "s"], F64, [3.0, -0.13, 1e308, 0.0, 0.0, np.nan, -3.0, 0.0]), ("sign", ["x"], F64, [1.0, -1.0, 1.0, 0.0, 0.0, np.nan, -1.0, 0.0])]
    got = gandiva.make_projector(sch, [b.make_expression(b.make_function(fn, [f[a] for a in args], t), pa.field("r%d" % i, t))
                                       for i, (fn, args, t, _) in enumerate(exprs)], pa.default_memory_pool()).evaluate(batch)
    for (fn, args, t, want), g in zip(exprs, got):
        assert_bit_exact(g, pa.array(want, t), "%s(%s)" % (fn, ", ".join(args)))
    cot = gandiva.make_projector(sch, [b.make_expression(b.make_function("cot", [f["x"]], F64), pa.field("c", F64))], pa.default_memory_pool()).evaluate(batch)[0]
    R.assert_class_and_ulp(cot.slice(7, 1), pa.array([R.libm_one("tan", R.HALF_PI)], F64), R.BAR, "cot(0) = tan of the double pi/2")


def test_numeric_tail_through_the_cxx_api():
    cxx = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gandiva_amd", "cxx")
    subprocess.check_call(["make", "-C", cxx, "all", "test_cxx"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(cxx, "tests", "test_numeric_tail_cxx")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
