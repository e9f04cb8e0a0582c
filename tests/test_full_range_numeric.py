"""The numeric core on full-range operands, on the GPU: arithmetic, compares, divide / mod, casts, greatest / least /
negative / abs, bitwise, exact and libm-backed math and the hashes over 4099-row batches of edge cross products and
exponent-uniform random rows (tests/helpers.py: edge_values, edge_pair_values), against the independent reference of
tests/numeric_reference.py — bit for bit on valid rows, the libm-backed functions by class and ulp distance.

The arithmetic exists three times (the device library under hipRTC, under the ahead-of-time flags, and re-implemented
around 64-bit slots in the tier-0 interpreter), so every family runs twice, each time in ONE fresh child process with a
timeout of its own: with GDV_NO_TIER0=1 on the specialised kernels and with GDV_FORCE_TIER0=1 on the interpreter, where
every evaluation must raise gdv_tier0_launches() by one.  Expressions are packed up to 36 to a projector.  The parent
computes the reference once per family and hands batches and expected columns to the children in Arrow files; shape
coverage belongs to the other GPU tests, here only slices of 1, 63, 64, 65 rows and one at offset 37 run in addition."""
import json
import os
import subprocess
import sys
import textwrap

import pyarrow as pa
import pytest

import numeric_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULLS = (0.0, 0.1)

# ---- the child: python -c _CHILD <case.json>; GDV_FORCE_TIER0 / GDV_NO_TIER0 are read once per process -----------------
_CHILD = textwrap.dedent("""
    import os, sys, json, ctypes as C
    sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
    import numpy as np, pyarrow as pa
    import gandiva_amd as gandiva
    from gandiva_amd import _capi, gandiva as gg
    from helpers import assert_bit_exact
    import numeric_reference as R
    lib = _capi.lib()
    with open(sys.argv[1]) as f:
        case = json.load(f)
    specs = case["specs"]
    interpreted = os.environ.get("GDV_FORCE_TIER0") is not None
    exprs = R.build_expressions(gandiva, specs)

    def program_of(group):
        sh = gg._make_schema(R.SCHEMA)
        try:
            arr = (C.c_void_p * len(group))(*[exprs[i]._h for i in group])
            p = lib.gdv_tier0_program(sh, arr, len(group), 0)
            if p:
                lib.gdv_free_string(p)
            return bool(p)
        finally:
            lib.gdv_schema_free(sh)

    # packed many to a projector: at most 36 outputs, and on the interpreter as many as one program takes
    groups = [[]]
    for i in range(len(exprs)):
        if len(groups[-1]) == 36 or (interpreted and groups[-1] and not program_of(groups[-1] + [i])):
            groups.append([])
        groups[-1].append(i)
    projs = []
    for group in groups:
        if interpreted:
            assert program_of(group), "no tier-0 program for %s: %s" % ([specs[i]["label"] for i in group], _capi.last_error())
        projs.append(gandiva.make_projector(R.SCHEMA, [exprs[i] for i in group], None))

    failures, evaluations = [], 0
    for nulls, path in case["files"]:
        table = pa.ipc.open_file(path).read_all().combine_chunks()
        for off, rows in ((0, len(table)), (0, 1), (0, 63), (0, 64), (0, 65), (37, 2000)):
            part = table.slice(off, rows)
            batch = pa.RecordBatch.from_arrays([part.column(n).chunk(0) for n in R.SCHEMA.names], schema=R.SCHEMA)
            for group, proj in zip(groups, projs):
                before = lib.gdv_tier0_launches()
                got = proj.evaluate(batch)
                evaluations += 1
                if interpreted:
                    assert lib.gdv_tier0_launches() - before == 1, "the evaluation was not interpreted (exactly once)"
                else:
                    assert lib.gdv_tier0_launches() == before, "the evaluation ran on the interpreter"
                for i, g in zip(group, got):
                    want = part.column("e%d" % specs[i]["column"]).chunk(0)
                    what = "%s nulls=%s offset=%d rows=%d" % (specs[i]["label"], nulls, off, rows)
                    try:
                        if specs[i]["ulps"] is None:
                            assert_bit_exact(g, want, what)
                        else:
                            if rows == len(table):
                                print("ULP %s nulls=%s: %d" % (specs[i]["label"], nulls, R.max_ulp_on_ordinary_rows(g, want)))
                            R.assert_class_and_ulp(g, want, specs[i]["ulps"], what)
                    except AssertionError as e:
                        failures.append(str(e))
    assert not failures, "%d comparisons failed:\\n%s" % (len(failures), "\\n".join(failures[:40]))
    print("FAMILY OK %s: %d expressions, %d projectors, %d evaluations" % (case["family"], len(specs), len(projs), evaluations))
""")


@pytest.fixture(scope="module")
def case_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("full_range")


def _write_case(case_dir, name, specs, expected_by_nulls):
    """Batches and expected columns as Arrow files, the expressions as JSON: written once, read by both children."""
    path = case_dir / (name + ".json")
    if path.exists():
        return str(path)
    files = []
    for nulls in NULLS:
        batch = R.batch(nulls)
        cols = {n: batch.column(n) for n in R.SCHEMA.names}
        cols.update({"e%d" % i: e for i, e in enumerate(expected_by_nulls[nulls])})
        table = pa.table(cols)
        f = str(case_dir / ("%s_%s.arrow" % (name, nulls)))
        with pa.ipc.new_file(f, table.schema) as w:
            w.write_table(table)
        files.append((nulls, f))
    path.write_text(json.dumps({"family": name, "specs": [dict(sp, column=i) for i, sp in enumerate(specs)], "files": files}))
    return str(path)


# set by the first child that ends by a signal or at its time limit: no later test of this file starts another GPU process
_ENDED_BADLY = []


def _run_child(case_path, interpreted, timeout=240):
    assert not _ENDED_BADLY, "not started: an earlier child process of this file " + _ENDED_BADLY[0]
    with open(case_path) as f:
        case = json.load(f)
    if interpreted:      # the expressions without a tier-0 program (divide, float mod, the hashes) run specialised only
        case["specs"] = [sp for sp in case["specs"] if sp["tier0"]]
        case_path = case_path[:-5] + "_tier0.json"
        with open(case_path, "w") as f:
            json.dump(case, f)
    env = dict(os.environ)
    env.pop("GDV_FORCE_TIER0", None)
    env.pop("GDV_NO_TIER0", None)
    env["GDV_FORCE_TIER0" if interpreted else "GDV_NO_TIER0"] = "1"
    try:
        r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT), case_path], env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _ENDED_BADLY.append("ran into its time limit of %d s (%s)" % (timeout, case["family"]))
        raise
    if r.returncode < 0 or r.returncode in (134, 139):
        _ENDED_BADLY.append("ended with exit status %d (%s)" % (r.returncode, case["family"]))
    print("\n".join(line for line in r.stdout.splitlines() if line.startswith(("ULP ", "FAMILY OK "))))
    assert r.returncode == 0, "child exit %d\n" % r.returncode + r.stdout[-3000:] + r.stderr[-6000:]
    assert "FAMILY OK " + case["family"] in r.stdout


def _family_case(case_dir, family):
    return _write_case(case_dir, family, R.family_specs(family), {nulls: R.expected_columns(family, nulls) for nulls in NULLS})


@pytest.mark.gpu
@pytest.mark.parametrize("family", R.FAMILIES)
def test_specialised_kernels_match_the_reference_on_full_range_operands(case_dir, family):
    """Every expression of the family on hipRTC-compiled kernels: integer wrap-around, uint64 / uint32 above the sign bit,
    64-bit and float division at extreme operands, narrowing mod, casts that must round once, denormal results, the
    double image that the hashes take, libm over its whole domain."""
    _run_child(_family_case(case_dir, family), interpreted=False)


@pytest.mark.gpu
@pytest.mark.parametrize("family", [f for f in R.FAMILIES if f != "hash"])
def test_interpreter_matches_the_reference_on_full_range_operands(case_dir, family):
    """The same expressions (but divide and float mod, which have no tier-0 program) on the interpreter, whose Arith,
    Compare, Cast, Normalise and Generic1/2 are written around 64-bit slots; every evaluation counted as a tier-0 launch."""
    assert any(sp["tier0"] for sp in R.family_specs(family))
    _run_child(_family_case(case_dir, family), interpreted=True)


@pytest.mark.gpu
def test_seed_chains_of_hash64_and_hash32_match_the_oracle_on_full_range_operands(case_dir):
    """hash64(float64, int64) and hash32(int64, int32): the two-argument forms on full-range values and seeds, against
    the oracle (which tests/test_full_range_numeric_cpu.py holds to the reference)."""
    import gandiva_amd as gandiva
    from oracle import oracle
    exprs = R.build_expressions(gandiva, R.HASH_CHAINS)
    expected = {nulls: oracle.project(exprs, R.batch(nulls)) for nulls in NULLS}
    _run_child(_write_case(case_dir, "hash_chains", R.HASH_CHAINS, expected), interpreted=False)
