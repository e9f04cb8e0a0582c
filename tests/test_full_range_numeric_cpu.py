"""The numeric core on full-range operands, without a GPU: the independent reference (tests/numeric_reference.py) against
the oracle and against the host build of the device library, on the 4099-row batches of edge cross products and
exponent-uniform random rows that tests/test_full_range_numeric.py runs on the GPU.  A wrong reference, a wrong oracle
or a wrong device function is found here first."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pytest

import gandiva_amd as gandiva
from oracle import oracle
import numeric_reference as R
from helpers import assert_bit_exact, edge_pair_values, edge_values, full_range_array, nonzero_divisors, validity_np
from test_device_lib_on_host import hostlib  # noqa: F401  (the fixture that builds tests/host_devlib)

def test_generators_cover_the_edges_and_every_magnitude():
    rng = np.random.default_rng(1)
    for tn in R.NUMERIC:
        t = R.TYPES[tn]
        e = edge_values(t)
        a, b = edge_pair_values(rng, t, R.ROWS)
        k = min(32, len(e))
        assert len(a) == len(b) == R.ROWS and R.ROWS - k * k >= 3000, "fewer than 3000 random rows"
        ea = np.array(e, dtype=a.dtype)
        assert a[:k * k].tobytes() == np.repeat(ea[:k], k).tobytes() and b[:k * k].tobytes() == np.tile(ea[:k], k).tobytes()
        img = {np.array([v], dtype=a.dtype).tobytes() for v in e}
        assert len(img) == len(e), "edge values are not deduplicated"
        seen = {a[i:i + 1].tobytes() for i in range(R.ROWS)} | {b[i:i + 1].tobytes() for i in range(R.ROWS)}
        assert img <= seen, "an edge value is in neither column"
        d = nonzero_divisors(b)
        assert not (d == 0).any() and np.array_equal(d[b != 0], b[b != 0], equal_nan=True)
        arr = full_range_array(rng, t, 20000, 0.1)
        v = np.asarray(arr.fill_null(1))
        assert 0.05 < arr.null_count / len(arr) < 0.15
        if pa.types.is_integer(t):
            info = np.iinfo(a.dtype)
            assert info.min in e and info.max in e and 0 in e and (v == 0).any()
            bits = np.array([abs(int(x)).bit_length() for x in v[:4000]])
            assert set(range(1, t.bit_width - (1 if info.min < 0 else 0) + 1)) <= set(bits.tolist()), "a magnitude never occurs"
            if info.min < 0:
                assert 0.3 < (v < 0).mean() < 0.7
        else:
            fi = np.finfo(a.dtype)
            assert np.isnan(v).sum() <= len(v) // 100 + 1
            tiny = np.abs(v[np.isfinite(v)])
            assert ((tiny > 0) & (tiny < fi.tiny)).any() and (tiny > fi.max / 4).any()
            assert fi.smallest_subnormal in e and np.isnan(e).sum() == 1 and np.signbit(e[e == 0]).tolist() == [False, True]


def test_integer_to_float_rounding_is_written_out_correctly():
    """The reference's integer -> float conversion against exact rational arithmetic at the ties."""
    assert R.int_to_float((1 << 24) + 1, 24, 128) == float(1 << 24)            # tie, even below
    assert R.int_to_float((1 << 24) + 3, 24, 128) == float((1 << 24) + 4)      # tie, even above
    assert R.int_to_float((1 << 54) + (1 << 30) + 1, 24, 128) == float((1 << 54) + (1 << 31))   # above the tie: up ...
    assert np.float32(np.float64((1 << 54) + (1 << 30) + 1)) == np.float32(1 << 54)             # ... but down through float64
    assert R.int_to_float(-(1 << 53) - 1, 53, 1024) == -float(1 << 53)
    assert R.int_to_float((1 << 64) - 1, 53, 1024) == 2.0 ** 64 and R.int_to_float((1 << 63) - 1, 24, 128) == 2.0 ** 63
    assert R.wrap(1 << 31, "i32") == -(1 << 31) and R.wrap(-1, "u8") == 255 and R.wrap(-(1 << 63) * -1, "i64") == -(1 << 63)


def test_pure_python_murmur3_32_matches_sklearn():
    from sklearn.utils import murmurhash3_32
    rng = np.random.default_rng(3)
    for seed in (0, 17, 0x7fffffff):
        for raw in [bytes(rng.integers(0, 256, 8, dtype=np.uint8)) for _ in range(50)]:
            assert R._murmur3_32(raw, seed) == murmurhash3_32(raw, seed=seed, positive=False)


@pytest.mark.parametrize("nulls", [0.0, 0.1])
@pytest.mark.parametrize("family", R.FAMILIES)
def test_oracle_matches_the_reference_on_full_range_operands(family, nulls):
    batch = R.batch(nulls)
    specs = R.family_specs(family)
    got = oracle.project(R.build_expressions(gandiva, specs), batch)
    for sp, g, w in zip(specs, got, R.expected_columns(family, nulls)):
        what = "oracle %s nulls=%s" % (sp["label"], nulls)
        if sp["ulps"] is None:
            assert_bit_exact(g, w, what)
        else:       # the host's libm: 1 ulp, but cbrt, pinned at its measured 3 (numeric_reference.ORACLE_MEASURED_ULPS)
            print("ULP %s: %d" % (what, R.max_ulp_on_ordinary_rows(g, w)))
            R.assert_class_and_ulp(g, w, sp["oracle_ulps"], what)


@pytest.mark.parametrize("nulls", [0.0, 0.1])
def test_oracle_seed_chains_match_the_reference(nulls):
    """hash64(float64, int64) and hash32(int64, int32): the value's hash seeded by the second column (an int64 seed
    narrowed to 32 bits and sign-extended), a NULL seed 0, a NULL value -> the seed as it stands."""
    batch = R.batch(nulls)
    got = oracle.project(R.build_expressions(gandiva, R.HASH_CHAINS), batch)
    for sp, g in zip(R.HASH_CHAINS, got):
        assert_bit_exact(g, R.expected_of(sp, batch), "oracle " + sp["label"])


def _host_result(hostlib, sp, batch):
    entry, k, op = sp["host"]
    args = [np.ascontiguousarray(np.asarray(batch.column(a).fill_null(1))) for a in sp["args"]]
    n = len(args[0])
    ptr = [a.ctypes.data_as(C.c_void_p) for a in args]
    rdt = np.uint8 if sp["ret"] == "bool" else np.dtype(R.TYPES[sp["ret"]].to_pandas_dtype())
    out = np.zeros(n, dtype=rdt)
    o = out.ctypes.data_as(C.c_void_p)
    if entry in ("int_binary", "float_binary", "compare", "minmax"):
        getattr(hostlib, "host_" + entry)(k, op, ptr[0], ptr[1], o, C.c_long(n))
    elif entry == "mod":
        hostlib.host_mod(k, ptr[0], ptr[1], o, C.c_long(n))
    elif entry == "cast":
        hostlib.host_cast(k, ptr[0], o, C.c_long(n))
    elif entry == "unary":
        hostlib.host_unary(k, op, ptr[0], o, C.c_long(n))
    else:
        hostlib.host_hash_numeric(k, op, ptr[0], o, C.c_long(n))
    return out


@pytest.mark.parametrize("family", ["arith", "divmod", "casts", "minmax_bitwise", "hash"])
def test_host_build_of_the_device_library_matches_the_reference(hostlib, family):
    """Every expression with a host entry point, per row through the device library's own function compiled for the
    host; compared on the rows where the expression is valid (the plain loop computes under nulls too: on 1)."""
    ran = 0
    for nulls in (0.0, 0.1):
        batch = R.batch(nulls)
        for sp, want in zip(R.family_specs(family), R.expected_columns(family, nulls)):
            if sp["host"] is None:
                continue
            raw = _host_result(hostlib, sp, batch)
            ok = validity_np(want) & np.logical_and.reduce([validity_np(batch.column(a)) for a in sp["args"]])
            got = pa.array(raw.astype(bool) if sp["ret"] == "bool" else raw, R.TYPES[sp["ret"]], mask=~validity_np(want))
            if sp["host"][0] == "hash":      # the expression hashes a NULL to 0; the host loop hashed the fill value
                got = pa.array(np.where(ok, raw, 0).astype(raw.dtype), R.TYPES[sp["ret"]])
            assert_bit_exact(got, want, "host build %s nulls=%s" % (sp["label"], nulls))
            ran += 1
    assert ran >= 12
