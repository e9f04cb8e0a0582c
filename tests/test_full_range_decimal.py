"""The decimal128 core on full-range operands, on the GPU: add subtract multiply divide mod, the six compares, greatest /
least, castDECIMAL between decimals and from integers, castBIGINT, castFLOAT8, castVARCHAR, abs, negative and round
truncate ceil floor over 4099-row batches — per type pair the anchor cross product, constructed ties of the half-away
rounding with their neighbours, results at +-(10^38 - 1) and one past it, equal values written at two scales, seeded
picks from the edge lists — against the independent reference of tests/decimal_reference.py, bit for bit on every row
(castFLOAT8 included: float(x) / p).

Precision and scale are plan constants, so hipRTC folds the device functions to different code per type pair; each pair
of decimal_reference.PAIRS names the branch it is there for.  One fresh child process per family (tests/full_range_child.py:
the whole batch, slices of 1, 63, 64, 65 rows and one at offset 37, both null fractions) with the default time limit;
tier 0 refuses decimal plans (tests/test_decimal_tail_cpu.py), so only the specialised kernels run.  The parent computes
the reference once per family.  That divide by zero raises and a null row does not is tests/test_decimal.py's."""
import json

import pytest

import decimal_reference as R
from full_range_child import NULLS, run_child, write_case


@pytest.fixture(scope="module")
def case_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("full_range_decimal")


def _case(case_dir, name, specs, groups=None):
    path = write_case(R, case_dir, name, specs, {nulls: R.expected_columns(name, nulls) for nulls in NULLS})
    if groups is not None:
        with open(path) as f:
            case = json.load(f)
        case["groups"] = groups
        with open(path, "w") as f:
            json.dump(case, f)
    return path


@pytest.mark.gpu
@pytest.mark.parametrize("family", R.FAMILIES)
def test_decimal_kernels_match_the_reference_on_full_range_operands(case_dir, family):
    """Every expression of the family on hipRTC-compiled kernels: the 128-bit fast paths and the 256-bit ones on either
    side of their thresholds, rounding at exact ties, overflow -> 0 at 10^38, 128-bit division by powers of ten up to
    10^38, the per-row k of round / truncate at the scale, one past it, -38, -39 and the int32 extremes."""
    run_child("decimal_reference", _case(case_dir, family, R.family_specs(family), R.family_groups(family)), interpreted=False)


@pytest.mark.gpu
def test_decimal_filter_and_selection_vectors_match_the_reference(case_dir):
    """less_than(a, b) across scales as a Filter against the reference's row numbers; multiply and castDECIMAL behind a
    UINT16 and a UINT32 selection vector (decimal_reference.child_extra_passes)."""
    run_child("decimal_reference", _case(case_dir, "extra", R.extra_specs()), interpreted=False)
