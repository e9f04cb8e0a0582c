"""The calendar tail on the GPU: months_between, next_day, add_months, date_trunc('unit', t) and the extractor names year
month day dayofmonth dayofyear dayofweek quarter hour minute second against the independent reference of
tests/calendar_tail_reference.py, bit for bit — the float64 results of months_between included: every step of its rule is one
IEEE double operation and the kernels are compiled without contraction.

Every family runs over the 4099-row batches (null share 0 and 0.1) and the machinery's slices (1, 63, 64, 65 rows, offset
37) in ONE fresh child process per path, with tests/full_range_child.py: with GDV_NO_TIER0=1 on the specialised kernels and
with GDV_FORCE_TIER0=1 on the interpreter, where every evaluation must raise gdv_tier0_launches() by one; each child then
runs every projector once more behind a UINT16 selection vector (calendar_tail_reference.child_extra_passes).  A row is left
out of the value comparison only where the exact result leaves int64.  The remaining tests run in this process: the hand
vectors, NULL literals and the C++ API."""
import os
import subprocess

import pyarrow as pa
import pytest

import calendar_tail_reference as R
import gandiva_amd as gandiva
import temporal_reference as T
from full_range_child import NULLS, run_child, write_case
from helpers import assert_bit_exact

pytestmark = pytest.mark.gpu
MS = R.MS
I32, I64, F64, STR, D64, TS = pa.int32(), pa.int64(), pa.float64(), pa.string(), pa.date64(), pa.timestamp("ms")


@pytest.fixture(scope="module")
def case_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("calendar_tail")


@pytest.mark.parametrize("interpreted", [False, True], ids=["specialised", "interpreted"])
@pytest.mark.parametrize("family", R.FAMILIES)
def test_family_matches_the_reference(case_dir, family, interpreted):
    case = write_case(R, case_dir, family, R.family_specs(family), {nulls: R.expected_columns(family, nulls) for nulls in NULLS},
                      {nulls: R.left_out_columns(family, nulls) for nulls in NULLS})
    run_child("calendar_tail_reference", case, interpreted=interpreted)


def _ms(y, m, d, tod=0):
    return T.day_of(y, m, d) * MS + tod


def test_hand_vectors_and_null_literals():
    sch = pa.schema([("e", TS), ("s", TS), ("d", D64), ("n", I32)])
    batch = pa.RecordBatch.from_arrays([
        pa.array([_ms(1997, 2, 28, 37800000), _ms(2015, 1, 14), _ms(2015, 2, 28, 5), None], pa.int64()).view(TS),
        pa.array([_ms(1996, 10, 30), _ms(2015, 1, 14, 77), _ms(2015, 1, 31, 9), _ms(2015, 1, 31)], pa.int64()).view(TS),
        pa.array([_ms(2015, 1, 14), _ms(2015, 1, 20), _ms(2023, 1, 31), _ms(2024, 2, 29)], pa.int64()).view(D64),
        pa.array([3, 3, 1, -12], I32)], schema=sch)
    b = gandiva.TreeExprBuilder()
    e, s, d, n = (b.make_field(f) for f in sch)
    lit = lambda v: b.make_literal(v, STR)
    exprs = [("months_between", [e, s], F64, pa.array([4 + (-2 + 0.4375) / 31, 0.0, 1.0, None], F64)),
             ("next_day", [d, n], D64, pa.array([_ms(2015, 1, 20), _ms(2015, 1, 27), _ms(2023, 2, 5), _ms(2024, 3, 4)], pa.int64()).view(D64)),
             ("next_day", [d, lit("tUe")], D64, pa.array([_ms(2015, 1, 20), _ms(2015, 1, 27), _ms(2023, 2, 7), _ms(2024, 3, 5)], pa.int64()).view(D64)),
             ("add_months", [d, n], D64, pa.array([_ms(2015, 4, 14), _ms(2015, 4, 20), _ms(2023, 2, 28), _ms(2023, 2, 28)], pa.int64()).view(D64)),
             ("date_trunc", [lit("MoNtH"), s], TS, pa.array([_ms(1996, 10, 1), _ms(2015, 1, 1), _ms(2015, 1, 1), _ms(2015, 1, 1)], pa.int64()).view(TS)),
             ("dayofweek", [d], I64, pa.array([4, 3, 3, 5], I64)),
             ("next_day", [d, b.make_null(STR)], D64, pa.array([None] * 4, pa.int64()).view(D64)),
             ("date_trunc", [b.make_null(STR), s], TS, pa.array([None] * 4, pa.int64()).view(TS))]
    proj = gandiva.make_projector(sch, [b.make_expression(b.make_function(fn, args, t), pa.field("r%d" % i, t)) for i, (fn, args, t, _) in enumerate(exprs)],
                                  pa.default_memory_pool())
    for (fn, _, _, want), g in zip(exprs, proj.evaluate(batch)):
        assert_bit_exact(g, want, fn)


def test_calendar_tail_through_the_cxx_api():
    cxx = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gandiva_amd", "cxx")
    subprocess.check_call(["make", "-C", cxx, "all", "test_cxx"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(cxx, "tests", "test_calendar_tail_cxx")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
