"""The numeric core on full-range operands, on the GPU: arithmetic, compares, divide / mod, casts, greatest / least /
negative / abs, bitwise, exact and libm-backed math and the hashes over 4099-row batches of edge cross products and
exponent-uniform random rows (tests/helpers.py: edge_values, edge_pair_values), against the independent reference of
tests/numeric_reference.py — bit for bit on valid rows, the libm-backed functions by class and ulp distance.

The arithmetic exists three times (the device library under hipRTC, under the ahead-of-time flags, and re-implemented
around 64-bit slots in the tier-0 interpreter), so every family runs twice, each time in ONE fresh child process with a
timeout of its own: with GDV_NO_TIER0=1 on the specialised kernels and with GDV_FORCE_TIER0=1 on the interpreter, where
every evaluation must raise gdv_tier0_launches() by one.  Expressions are packed up to 36 to a projector.  The parent
computes the reference once per family and hands batches and expected columns to the children in Arrow files; shape
coverage belongs to the other GPU tests, here only slices of 1, 63, 64, 65 rows and one at offset 37 run in addition.
The child-process machinery is tests/full_range_child.py's, shared with tests/test_full_range_temporal.py."""
import pytest

import numeric_reference as R
from full_range_child import NULLS, run_child, write_case


@pytest.fixture(scope="module")
def case_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("full_range")


def _family_case(case_dir, family):
    return write_case(R, case_dir, family, R.family_specs(family), {nulls: R.expected_columns(family, nulls) for nulls in NULLS})


@pytest.mark.gpu
@pytest.mark.parametrize("family", R.FAMILIES)
def test_specialised_kernels_match_the_reference_on_full_range_operands(case_dir, family):
    """Every expression of the family on hipRTC-compiled kernels: integer wrap-around, uint64 / uint32 above the sign bit,
    64-bit and float division at extreme operands, narrowing mod, casts that must round once, denormal results, the
    double image that the hashes take, libm over its whole domain."""
    run_child("numeric_reference", _family_case(case_dir, family), interpreted=False)


@pytest.mark.gpu
@pytest.mark.parametrize("family", [f for f in R.FAMILIES if f != "hash"])
def test_interpreter_matches_the_reference_on_full_range_operands(case_dir, family):
    """The same expressions (but divide and float mod, which have no tier-0 program) on the interpreter, whose Arith,
    Compare, Cast, Normalise and Generic1/2 are written around 64-bit slots; every evaluation counted as a tier-0 launch."""
    assert any(sp["tier0"] for sp in R.family_specs(family))
    run_child("numeric_reference", _family_case(case_dir, family), interpreted=True)


@pytest.mark.gpu
def test_seed_chains_of_hash64_and_hash32_match_the_oracle_on_full_range_operands(case_dir):
    """hash64(float64, int64) and hash32(int64, int32): the two-argument forms on full-range values and seeds, against
    the oracle (which tests/test_full_range_numeric_cpu.py holds to the reference)."""
    import gandiva_amd as gandiva
    from oracle import oracle
    exprs = R.build_expressions(gandiva, R.HASH_CHAINS)
    expected = {nulls: oracle.project(exprs, R.batch(nulls)) for nulls in NULLS}
    run_child("numeric_reference", write_case(R, case_dir, "hash_chains", R.HASH_CHAINS, expected), interpreted=False)
