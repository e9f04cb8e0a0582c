"""The child-process machinery of the full-range GPU tests (tests/test_full_range_numeric.py over numeric_reference,
tests/test_full_range_temporal.py over temporal_reference): the parent writes batches and expected columns to Arrow
files and the expressions to JSON; one fresh child process per family and path evaluates them, packed up to 36 to a
projector, on the whole batch and on slices of 1, 63, 64, 65 rows and one at offset 37, and compares bit for bit (the
libm-backed functions by class and ulp distance).  With GDV_NO_TIER0=1 the specialised kernels run and
gdv_tier0_launches() must not move; with GDV_FORCE_TIER0=1 the interpreter runs and every evaluation raises it by one.
An expected column e<i> may come with a bool column x<i> of rows that are left out of the value comparison (their
validity is still compared)."""
import json
import os
import subprocess
import sys
import textwrap

import pyarrow as pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULLS = (0.0, 0.1)

# ---- the child: python -c CHILD <case.json>; GDV_FORCE_TIER0 / GDV_NO_TIER0 are read once per process -----------------
CHILD = textwrap.dedent("""
    import os, sys, json, ctypes as C
    sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
    import numpy as np, pyarrow as pa
    import gandiva_amd as gandiva
    from gandiva_amd import _capi, gandiva as gg
    from helpers import assert_bit_exact, assert_bit_exact_where
    import {module} as R
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

    # packed many to a projector: at most 36 outputs, and on the interpreter as many as one program takes (a case may
    # name its projectors itself: "groups", lists of expression numbers)
    groups = [[]]
    for i in range(len(exprs)):
        if len(groups[-1]) == 36 or (interpreted and groups[-1] and not program_of(groups[-1] + [i])):
            groups.append([])
        groups[-1].append(i)
    groups = case.get("groups", groups)
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
            if hasattr(R, "child_batch"):          # a reference whose inputs have a buffer layout that a file does not keep
                batch = R.child_batch(nulls, batch, off, rows)
            for group, proj in zip(groups, projs):
                before = lib.gdv_tier0_launches()
                got = proj.evaluate(batch)
                evaluations += 1
                if hasattr(R, "child_after_evaluate"):      # a reference's own assertions on the path the evaluation took
                    R.child_after_evaluate(case, nulls, group, proj, rows == len(table))
                if interpreted:
                    assert lib.gdv_tier0_launches() - before == 1, "the evaluation was not interpreted (exactly once)"
                else:
                    assert lib.gdv_tier0_launches() == before, "the evaluation ran on the interpreter"
                for i, g in zip(group, got):
                    want = part.column("e%d" % specs[i]["column"]).chunk(0)
                    what = "%s nulls=%s offset=%d rows=%d" % (specs[i]["label"], nulls, off, rows)
                    try:
                        if getattr(R, "VALIDATE_OUTPUTS", False):      # (not for date64: full-range values are no whole days)
                            g.validate(full=True)
                        if "x%d" % specs[i]["column"] in part.column_names:
                            assert_bit_exact_where(g, want, ~np.asarray(part.column("x%d" % specs[i]["column"]).chunk(0)), what)
                        elif specs[i]["ulps"] is None:
                            assert_bit_exact(g, want, what)
                        else:
                            if rows == len(table):
                                print("ULP %s nulls=%s: %d" % (specs[i]["label"], nulls, R.max_ulp_on_ordinary_rows(g, want)))
                            R.assert_class_and_ulp(g, want, specs[i]["ulps"], what)
                    except AssertionError as e:
                        failures.append(str(e))
    if hasattr(R, "child_extra_passes"):      # further passes of a reference's own (device-resident inputs, selection vectors)
        evaluations += R.child_extra_passes(gandiva, case, exprs, groups, projs, failures)
    assert not failures, "%d comparisons failed:\\n%s" % (len(failures), "\\n".join(failures[:40]))
    print("FAMILY OK %s: %d expressions, %d projectors, %d evaluations" % (case["family"], len(specs), len(projs), evaluations))
""")


def write_case(R, case_dir, name, specs, expected_by_nulls, left_out_by_nulls=None):
    """Batches and expected columns as Arrow files, the expressions as JSON: written once, read by both children."""
    path = case_dir / (name + ".json")
    if path.exists():
        return str(path)
    files = []
    for nulls in NULLS:
        batch = R.batch(nulls)
        cols = {n: batch.column(n) for n in R.SCHEMA.names}
        cols.update({"e%d" % i: e for i, e in enumerate(expected_by_nulls[nulls])})
        if left_out_by_nulls is not None:
            cols.update({"x%d" % i: pa.array(x) for i, x in enumerate(left_out_by_nulls[nulls]) if x.any()})
        table = pa.table(cols)
        f = str(case_dir / ("%s_%s.arrow" % (name, nulls)))
        with pa.ipc.new_file(f, table.schema) as w:
            w.write_table(table)
        files.append((nulls, f))
    path.write_text(json.dumps({"family": name, "specs": [dict(sp, column=i) for i, sp in enumerate(specs)], "files": files}))
    return str(path)


# set by the first child that ends by a signal or at its time limit: no later full-range test starts another GPU process
ENDED_BADLY = []


def run_child(module, case_path, interpreted, timeout=240, extra_env=None):
    """One fresh child process over a case; `extra_env` is added to the child's environment."""
    assert not ENDED_BADLY, "not started: an earlier child process of the full-range tests " + ENDED_BADLY[0]
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
    env.update(extra_env or {})
    try:
        r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, module=module), case_path], env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        ENDED_BADLY.append("ran into its time limit of %d s (%s)" % (timeout, case["family"]))
        raise
    if r.returncode < 0 or r.returncode in (134, 139):
        ENDED_BADLY.append("ended with exit status %d (%s)" % (r.returncode, case["family"]))
    print("\n".join(line for line in r.stdout.splitlines() if line.startswith(("ULP ", "FAMILY OK "))))
    assert r.returncode == 0, "child exit %d\n" % r.returncode + r.stdout[-3000:] + r.stderr[-6000:]
    assert "FAMILY OK " + case["family"] in r.stdout
