"""The date and time functions on full-range operands, on the GPU: the extractors over date32 / date64 / timestamp /
time32, date_trunc_* / extractWeek / weekofyear / last_day, timestampadd* / date_add / date_sub with per-row and literal
counts, timestampdiff* / datediff / date_diff, the fixed-width casts and to_timestamp / to_time over numbers — over
4099-row batches of edge cross products (the type's ends, year 0 and below, era boundaries, month ends, ISO-week
corners) and exponent-uniform random rows that reach +-5.8 million years in date32 and +-292 million in milliseconds,
against the independent reference of tests/temporal_reference.py, bit for bit.  A row whose exact result or
intermediate leaves int64 is left out of the value comparison (signed overflow is undefined in the device library);
its validity is still compared.

Every family runs twice, each time in ONE fresh child process with a timeout of its own (tests/full_range_child.py):
with GDV_NO_TIER0=1 on the specialised hipRTC kernels and with GDV_FORCE_TIER0=1 on the interpreter, which calls the
same device functions by id and where every evaluation must raise gdv_tier0_launches() by one."""
import pytest

import temporal_reference as R
from full_range_child import NULLS, run_child, write_case


@pytest.fixture(scope="module")
def case_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("full_range_temporal")


def _family_case(case_dir, family):
    return write_case(R, case_dir, family, R.family_specs(family), {nulls: R.expected_columns(family, nulls) for nulls in NULLS},
                      {nulls: R.left_out_columns(family, nulls) for nulls in NULLS})


@pytest.mark.gpu
@pytest.mark.parametrize("family", R.FAMILIES)
def test_specialised_kernels_match_the_reference_on_full_range_dates_and_times(case_dir, family):
    """Every expression of the family on hipRTC-compiled kernels: civil dates of day counts far below year 0 and near the
    ends of date32 and of int64 milliseconds, truncation toward zero before 1970, month-end clamping millions of years
    out, month counts beyond 2^31 divided before they are narrowed, differences narrowed modulo 2^32, seconds times 1000
    modulo 2^64 and saturating from floats."""
    run_child("temporal_reference", _family_case(case_dir, family), interpreted=False)


@pytest.mark.gpu
@pytest.mark.parametrize("family", R.FAMILIES)
def test_interpreter_matches_the_reference_on_full_range_dates_and_times(case_dir, family):
    """The same expressions on the tier-0 interpreter (kCall1 / kCall2 into the same device functions, values in 64-bit
    slots, literal counts as constants); every evaluation counted as a tier-0 launch."""
    run_child("temporal_reference", _family_case(case_dir, family), interpreted=True)
