"""Tier 0 over the rest of the fixed-width registry and over selection vectors, on the GPU.

GDV_FORCE_TIER0 is read once per process, so every test runs ONE child process with it set (the child has its own
timeout).  Inside, a family's expressions are packed many to a projector — a handful of launches of the ahead-of-time
interpreter kernel, no hipRTC — and every evaluation must raise gdv_tier0_launches() by exactly one.  Results are
compared with the oracle bit for bit on valid rows (helpers.assert_bit_exact); the libm-backed math functions by the
rule of test_parity_gpu.py::test_math_functions_within_one_ulp, and bit for bit with the specialised kernel."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the child: python -c _CHILD <family> [<directory for the math family's outputs>] --------------------------------
_CHILD = textwrap.dedent("""
    import os, sys, json, time, ctypes as C
    sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
    import numpy as np, pyarrow as pa
    import gandiva_amd as gandiva
    from gandiva_amd import _capi, gandiva as gg
    from oracle import oracle
    from helpers import assert_bit_exact, random_array, validity_np, ulp_distance
    lib = _capi.lib()
    family = sys.argv[1]
    b = gandiva.TreeExprBuilder()
    I8, I16, I32, I64, U16, U32, U64 = pa.int8(), pa.int16(), pa.int32(), pa.int64(), pa.uint16(), pa.uint32(), pa.uint64()
    F32, F64, BOOL = pa.float32(), pa.float64(), pa.bool_()
    D32, D64, TS, TM = pa.date32(), pa.date64(), pa.timestamp("ms"), pa.time32("ms")
    DAY = 86400000

    def days(y, m, d):
        return int((np.datetime64("%04d-%02d-%02d" % (y, m, d)) - np.datetime64("1970-01-01")) / np.timedelta64(1, "D"))
    # instants before 1970, month ends, leap days, year boundaries (and the millisecond on either side of a midnight)
    SPECIAL_DAYS = [days(*t) for t in ((1969, 12, 31), (1970, 1, 1), (2000, 2, 29), (2024, 2, 29), (1900, 2, 28), (1900, 3, 1),
                                       (2023, 12, 31), (2024, 1, 1), (1999, 12, 31), (2021, 1, 31), (2021, 3, 31), (2021, 4, 30),
                                       (1600, 2, 29), (1583, 1, 1), (2100, 2, 28), (2001, 1, 1), (1901, 1, 1), (1960, 2, 29))]
    SPECIAL_MS = [d * DAY + o for d in SPECIAL_DAYS for o in (0, DAY - 1)] + [-1, 0, 1, -DAY, -DAY - 1, 951827696789, -2208988800001]

    def with_specials(arr, specials, t):
        # the specials go to the front, so that the short batches hold some too
        raw = np.array(arr.cast(I32 if t in (D32, TM) else I64).fill_null(0))
        k = min(len(specials), len(raw))
        raw[:k] = np.array(specials[:k], dtype=raw.dtype)
        return pa.array(raw, type=I32 if t in (D32, TM) else I64, mask=np.array(~validity_np(arr))).cast(t)

    COLS = [("a", I32), ("b", I32), ("l", I64), ("m", I64), ("p", F32), ("q", F32), ("x", F64), ("y", F64), ("u", U32), ("v", U32),
            ("w", U64), ("z", U64), ("f", BOOL), ("g", BOOL), ("c8", I8), ("c16", I16), ("h", U16), ("k32", I32), ("k64", I64),
            ("d32", D32), ("e32", D32), ("d64", D64), ("e64", D64), ("t1", TS), ("t2", TS), ("tm", TM), ("s32", I32), ("s64", I64),
            ("sf", F32), ("sx", F64), ("px", F64), ("py", F64)]
    SCHEMA = pa.schema(COLS)
    FLD = {{n: b.make_field(SCHEMA.field(n)) for n, _ in COLS}}

    def make_batch(n, nulls, seed):
        rng = np.random.default_rng(seed)
        arrs = []
        for name, t in COLS:
            if name in ("k32", "k64"):          # counts of timestampadd / date_add: small, so that no sum overflows
                arrs.append(random_array(rng, t, n, nulls, special=False))
            elif name in ("s32", "s64"):        # seconds since the epoch
                k = rng.integers(-2 ** 33, 2 ** 33, n)
                arrs.append(pa.array((k % 2 ** 31).astype(np.int32) if t == I32 else k, t, mask=None if nulls <= 0 else rng.random(n) < nulls))
            elif name in ("sf", "sx"):
                v = rng.standard_normal(n) * 10.0 ** rng.integers(0, 11, n)
                arrs.append(pa.array(v.astype(np.float32) if t == F32 else v, t, mask=None if nulls <= 0 else rng.random(n) < nulls))
            elif name in ("px", "py"):          # the domain of the libm comparison (test_math_functions_within_one_ulp)
                v = rng.random(n) * 100 + 0.01 if name == "px" else rng.random(n) * 3
                arrs.append(pa.array(v, t, mask=None if nulls <= 0 else rng.random(n) < nulls))
            elif t == TM:
                arrs.append(pa.array(rng.integers(0, DAY, n).astype(np.int32), I32, mask=None if nulls <= 0 else rng.random(n) < nulls).cast(TM))
            elif t in (D32, D64, TS):
                arr = random_array(rng, t, n, nulls)
                sp = SPECIAL_DAYS if t == D32 else [d * DAY for d in SPECIAL_DAYS] if t == D64 else SPECIAL_MS
                if name[0] == "e" or name == "t2":
                    sp = sp[::-1]
                arrs.append(with_specials(arr, sp, t))
            else:
                arrs.append(random_array(rng, t, n, nulls))
        return pa.RecordBatch.from_arrays(arrs, schema=SCHEMA)

    # castTIMESTAMP(date32) and castTIME(timestamp) are the two signatures the oracle has no case for (its generic integer
    # cast hands the argument back): their definitions, as tests/test_temporal_text.py states them — days x 86 400 000 and
    # the millisecond of the day (floored modulo)
    def by_definition(col, storage, t, f):
        def want(batch):
            arr = batch.column(col)
            raw = np.asarray(arr.cast(storage).fill_null(0))
            return pa.array(f(raw), mask=np.array(~validity_np(arr))).cast(t)
        return want
    NOT_IN_ORACLE = {{"castTIMESTAMP(d32)": by_definition("d32", I32, TS, lambda v: v.astype(np.int64) * DAY),
                     "castTIME(t1)": by_definition("t1", I64, TM, lambda v: (v % DAY).astype(np.int32))}}

    def fn(name, args, t):
        return (name + "(" + ",".join(args) + ")", b.make_function(name, [FLD[a] for a in args], t), t)

    def family_exprs(family):
        e = []
        if family == "arith":
            for t, (c0, c1) in ((I32, "ab"), (I64, "lm"), (F32, "pq"), (F64, "xy")):
                e += [fn("negative", [c0], t), fn("abs", [c0], t), fn("greatest", [c0, c1], t), fn("least", [c0, c1], t)]
            e += [fn("mod", ["l", "a"], I32), fn("mod", ["l", "m"], I64), fn("mod", ["a", "b"], I32),
                  fn("modulo", ["l", "a"], I32), fn("modulo", ["l", "m"], I64), fn("modulo", ["a", "b"], I32)]
            for t, (c0, c1) in ((I32, "ab"), (I64, "lm"), (U32, "uv"), (U64, "wz")):
                e += [fn("bitwise_and", [c0, c1], t), fn("bitwise_or", [c0, c1], t), fn("bitwise_xor", [c0, c1], t), fn("bitwise_not", [c0], t)]
        elif family == "nulls":
            pairs = (("a", "b", I32), ("l", "m", I64), ("p", "q", F32), ("x", "y", F64), ("u", "v", U32), ("w", "z", U64), ("f", "g", BOOL),
                     ("c8", "c8", I8), ("h", "h", U16), ("d32", "e32", D32), ("d64", "e64", D64), ("t1", "t2", TS), ("tm", "tm", TM))
            for c0, c1, t in pairs:
                e += [fn("nvl", [c0, c1], t), fn("is_distinct_from", [c0, c1], BOOL), fn("is_not_distinct_from", [c0, c1], BOOL)]
            e += [fn(f, ["f"], BOOL) for f in ("istrue", "isfalse", "isnottrue", "isnotfalse")]
            e += [fn("isnumeric", [c], BOOL) for c in ("a", "l", "p", "x", "u", "w", "c8", "h")]
            # a literal and a NULL literal as nvl's second argument; distinctness against a NULL
            e += [("nvl(a,7)", b.make_function("nvl", [FLD["a"], b.make_literal(7, I32)], I32), I32),
                  ("nvl(x,null)", b.make_function("nvl", [FLD["x"], b.make_null(F64)], F64), F64),
                  ("is_distinct_from(c16,null)", b.make_function("is_distinct_from", [FLD["c16"], b.make_null(I16)], BOOL), BOOL)]
        elif family == "dates":
            e += [fn("castDATE", ["l"], D64), fn("castDATE", ["d32"], D64), fn("castDATE", ["t1"], D64), fn("castDATE32", ["d64"], D32),
                  fn("castTIMESTAMP", ["l"], TS), fn("castTIMESTAMP", ["d64"], TS), fn("castTIMESTAMP", ["d32"], TS),
                  fn("castBIGINT", ["d64"], I64), fn("castBIGINT", ["t1"], I64), fn("castTIME", ["t1"], TM)]
            for c in ("d32", "d64", "t1"):
                e += [fn("extract" + u, [c], I64) for u in ("Year", "Month", "Day", "Quarter", "Doy", "Dow", "Hour", "Minute", "Second",
                                                             "Epoch", "Decade", "Century", "Millennium")]
            e += [fn("extract" + u, ["tm"], I64) for u in ("Hour", "Minute", "Second")]
        elif family == "trunc":
            for c, t in (("d64", D64), ("t1", TS)):
                e += [fn("date_trunc_" + u, [c], t) for u in ("Second", "Minute", "Hour", "Day", "Week", "Month", "Quarter", "Year",
                                                               "Decade", "Century", "Millennium")]
                e += [fn("extractWeek", [c], I64), fn("weekofyear", [c], I64), fn("last_day", [c], D64)]
        elif family == "adddiff":
            for c, c2, t in (("d64", "e64", D64), ("t1", "t2", TS)):
                e += [fn("timestampadd" + u, ["k64", c], t) for u in ("Second", "Minute", "Hour", "Day", "Week", "Month", "Quarter", "Year")]
                e += [fn("date_add", [c, "k64"], t), fn("date_sub", [c, "k64"], t), fn("date_add", [c, "k32"], t), fn("date_sub", [c, "k32"], t)]
                e += [fn("timestampdiff" + u, [c, c2], I32) for u in ("Second", "Minute", "Hour", "Day", "Week", "Month", "Quarter", "Year")]
                e += [fn("datediff", [c, c2], I32), fn("date_diff", [c, c2], I32)]
            e += [fn("datediff", ["d32", "e32"], I32), fn("date_diff", ["d32", "e32"], I32)]
        elif family == "seconds":
            for c in ("s32", "s64", "sf", "sx"):
                e += [fn("to_timestamp", [c], TS), fn("to_time", [c], TM)]
        elif family == "in":
            def inx(col, values, t):
                return ("in(" + col + ")", b.make_in_expression(FLD[col], values, t), BOOL)
            e += [inx("a", [0, 1, -1, 7, 999, -1000, 2147483647, -2147483648], I32), inx("a", list(range(-40, 40)), I32), inx("a", [], I32),
                  inx("l", [5, -5, 0, 2 ** 40, -2 ** 63], I64), inx("c8", [-128, -1, 3, 127], I8), inx("h", [0, 65535, 300], U16),
                  inx("u", [0, 4294967295, 17], U32), inx("w", [0, 2 ** 64 - 1, 1], U64),
                  inx("x", [0.0, 1.0, float("nan"), float("inf")], F64), inx("p", [-0.0, 1.0, float("-inf")], F32),
                  inx("d64", [d * DAY for d in SPECIAL_DAYS[:6]], D64), inx("d32", SPECIAL_DAYS[:6], D32), inx("t1", SPECIAL_MS[:9], TS)]
            # inside a tree: under NOT, AND with a comparison, as an if's condition
            e += [("not in", b.make_function("not", [b.make_in_expression(FLD["a"], [1, 2, 3], I32)], BOOL), BOOL),
                  ("in and cmp", b.make_and([b.make_in_expression(FLD["c8"], [1, 2, 3, -4], I8),
                                             b.make_function("greater_than", [FLD["l"], b.make_literal(0, I64)], BOOL)]), BOOL),
                  ("if in", b.make_if(b.make_in_expression(FLD["h"], [1, 2, 500], U16), FLD["a"], FLD["b"], I32), I32)]
        elif family == "math":
            e += [fn(f, ["px"], F64) for f in ("cbrt", "log", "log10", "sqrt")] + [fn("exp", ["py"], F64), fn("power", ["px", "py"], F64),
                                                                                  fn("pow", ["px", "py"], F64)]
            e += [fn(f, ["x"], F64) for f in ("floor", "ceil", "round", "truncate", "sqrt", "cbrt")]
        return e

    def program_of(exprs):
        sh = gg._make_schema(SCHEMA)
        try:
            arr = (C.c_void_p * len(exprs))(*[x._h for x in exprs])
            p = lib.gdv_tier0_program(sh, arr, len(exprs), 0)
            if not p:
                return None
            lib.gdv_free_string(p)
            return True
        finally:
            lib.gdv_schema_free(sh)

    def counted(call):
        before = lib.gdv_tier0_launches()
        out = call()
        assert lib.gdv_tier0_launches() - before == 1, "the evaluation was not interpreted (exactly once)"
        return out

    def run_family(family, save_dir=None):
        triples = family_exprs(family)
        exprs = [b.make_expression(node, pa.field("r%d" % i, t)) for i, (_, node, t) in enumerate(triples)]
        interpreted = os.environ.get("GDV_FORCE_TIER0") is not None
        # packed many to a projector: as many outputs as the interpreter's argument block and program take (at most 36)
        groups = [[]]
        for i in range(len(exprs)):
            if len(groups[-1]) == 36 or (groups[-1] and not program_of([exprs[j] for j in groups[-1] + [i]])):
                groups.append([])
            groups[-1].append(i)
        projs = []
        for gidx in groups:
            ge = [exprs[i] for i in gidx]
            assert program_of(ge), "no tier-0 program: " + _capi.last_error()
            projs.append(gandiva.make_projector(SCHEMA, ge, None))
        saved = {{}}
        def check(batch, what):
            for gidx, proj in zip(groups, projs):
                ge = [exprs[i] for i in gidx]
                got = counted(lambda: proj.evaluate(batch)) if interpreted else proj.evaluate(batch)
                want = oracle.project(ge, batch)
                for i, g, w in zip(gidx, got, want):
                    label = "%s %s" % (triples[i][0], what)
                    if triples[i][0] in NOT_IN_ORACLE:
                        w = NOT_IN_ORACLE[triples[i][0]](batch)
                    if family == "math":
                        check_math(triples[i][0], batch, g, w, label)
                        if save_dir:
                            ok = validity_np(w)
                            assert np.array_equal(validity_np(g), ok), label
                            saved["%s|%s" % (label, "values")] = np.asarray(g.fill_null(0.0))[ok]
                    else:
                        assert_bit_exact(g, w, label)
        for nulls in (0.0, 0.1, 1.0):
            full = make_batch(70001 + 65, nulls, seed=int(nulls * 10) + 3)
            for n in (1, 63, 64, 65, 1000, 70001):
                check(full.slice(0, n), "rows=%d nulls=%s" % (n, nulls))
            if nulls == 0.1:
                for off in (1, 63, 65):      # a sliced batch: bitmaps and bit-packed values misaligned
                    check(full.slice(off, 1000), "offset=%d" % off)
        if save_dir:
            np.savez(os.path.join(save_dir, "interpreted.npz" if interpreted else "specialised.npz"), **saved)

    def check_math(name, batch, g, w, label):
        ok = validity_np(w)
        assert np.array_equal(validity_np(g), ok), label
        f = name.split("(")[0]
        if f in ("floor", "ceil", "round", "truncate") or "(x" in name:
            if f in ("floor", "ceil", "round", "truncate"):
                assert_bit_exact(g, w, label)       # exact functions
            return                                   # (sqrt / cbrt over the full range: against the specialised kernel only)
        # within 1 ulp of the correctly rounded value (x87 extended precision, rounded once); the oracle's libm within 4
        lx = np.asarray(batch.column("px").fill_null(1.0)).astype(np.longdouble)
        ly = np.asarray(batch.column("py").fill_null(1.0)).astype(np.longdouble)
        exact = {{"cbrt": lambda: np.cbrt(lx), "log": lambda: np.log(lx), "log10": lambda: np.log10(lx), "sqrt": lambda: np.sqrt(lx),
                  "exp": lambda: np.exp(ly), "power": lambda: np.power(lx, ly), "pow": lambda: np.power(lx, ly)}}[f]().astype(np.float64)
        gv, wv = np.asarray(g.fill_null(0.0)), np.asarray(w.fill_null(0.0))
        hip_ulp, cpu_ulp = ulp_distance(gv[ok], exact[ok]), ulp_distance(wv[ok], exact[ok])
        assert hip_ulp <= 1, "%s: interpreted result %d ulp from the correctly rounded value" % (label, hip_ulp)
        assert cpu_ulp <= 4, "%s: oracle result %d ulp from the correctly rounded value" % (label, cpu_ulp)

    def run_selection():
        n = 70001
        batch = make_batch(n, 0.1, seed=11)
        cond = b.make_condition(b.make_function("greater_than", [b.make_function("extractYear", [FLD["t1"]], I64), b.make_literal(2000, I64)], BOOL))
        flt = gandiva.make_filter(SCHEMA, cond)
        sel = counted(lambda: flt.evaluate(batch, dtype="int32"))
        want_idx = oracle.filter_indices(cond, batch, "int32")
        assert sel.to_array().equals(want_idx)
        idx = np.asarray(want_idx)
        assert len(idx) > 1000 and idx[999] < 65536
        triples = [fn("date_trunc_Month", ["t1"], TS), fn("nvl", ["h", "h"], U16), fn("add", ["c8", "c8"], I8), fn("extractDay", ["d32"], I64),
                   ("nvl(c8,lit)", b.make_function("nvl", [FLD["c8"], b.make_literal(-3, I8)], I8), I8),
                   ("f and notnull(c8)", b.make_and([FLD["f"], b.make_function("isnotnull", [FLD["c8"]], BOOL)]), BOOL),
                   ("if f h", b.make_if(FLD["f"], FLD["h"], b.make_literal(9, U16), U16), U16),
                   ("istrue(g)", b.make_function("istrue", [FLD["g"]], BOOL), BOOL), fn("multiply", ["x", "y"], F64),
                   ("in(h)", b.make_in_expression(FLD["h"], [1, 2, 500, 1000], U16), BOOL)]
        exprs = [b.make_expression(node, pa.field("r%d" % i, t)) for i, (_, node, t) in enumerate(triples)]
        import torch
        dbatch = gandiva.DeviceBatch.from_arrow(batch)
        for mode, name, npdt, tdt in ((1, "UINT16", np.uint16, torch.int16), (2, "UINT32", np.uint32, torch.int32), (3, "UINT64", np.uint64, torch.int64)):
            proj = gandiva.make_projector(SCHEMA, exprs, None, selection_mode=name)
            for k in (1, 64, 65, 1000):
                want = oracle.project(exprs, oracle.take_rows(batch, idx[:k]))
                host_sel = gandiva.SelectionVector(mode, idx[:k].astype(npdt), k)
                got = counted(lambda: proj.evaluate(batch, selection=host_sel))
                for t3, g, w in zip(triples, got, want):
                    assert_bit_exact(g, w, "%s %s host slots=%d" % (t3[0], name, k))
                signed = idx[:k].astype(npdt).view({{np.uint16: np.int16, np.uint32: np.int32, np.uint64: np.int64}}[npdt])
                dev_sel = gandiva.SelectionVector(mode, torch.from_numpy(signed.copy()).to("cuda"), k, device=True)
                got = counted(lambda: proj.evaluate_device(dbatch, selection=dev_sel))
                for t3, g, w in zip(triples, got, want):
                    assert_bit_exact(g.to_arrow(), w, "%s %s device slots=%d" % (t3[0], name, k))
            # the slot count in device memory: buffers and grid sized for 1000 slots, 65 of them real
            signed = idx[:1000].astype(npdt).view({{np.uint16: np.int16, np.uint32: np.int32, np.uint64: np.int64}}[npdt])
            pending = gandiva.SelectionVector(mode, torch.from_numpy(signed.copy()).to("cuda"), None, device=True,
                                              count_tensor=torch.tensor([65], dtype=torch.int64, device="cuda"))
            got = counted(lambda: proj.evaluate_device(dbatch, selection=pending))
            for t3, g, w in zip(triples, got, oracle.project(exprs, oracle.take_rows(batch, idx[:65]))):
                assert_bit_exact(g.to_arrow(), w, "%s %s device-resident slot count" % (t3[0], name))
            # a sliced batch under a selection vector: rows and their validity bits gathered through shifted bitmaps
            sliced = batch.slice(37, 30000)
            sidx = np.asarray(oracle.filter_indices(cond, sliced, "int32"))
            sdev = gandiva.DeviceBatch.from_arrow(sliced)
            for k in (65, 1000):
                want = oracle.project(exprs, oracle.take_rows(sliced, sidx[:k]))
                host_sel = gandiva.SelectionVector(mode, sidx[:k].astype(npdt), k)
                got = counted(lambda: proj.evaluate(sliced, selection=host_sel))
                for t3, g, w in zip(triples, got, want):
                    assert_bit_exact(g, w, "%s %s sliced host slots=%d" % (t3[0], name, k))
                signed = sidx[:k].astype(npdt).view({{np.uint16: np.int16, np.uint32: np.int32, np.uint64: np.int64}}[npdt])
                dev_sel = gandiva.SelectionVector(mode, torch.from_numpy(signed.copy()).to("cuda"), k, device=True)
                got = counted(lambda: proj.evaluate_device(sdev, selection=dev_sel))
                for t3, g, w in zip(triples, got, want):
                    assert_bit_exact(g.to_arrow(), w, "%s %s sliced device slots=%d" % (t3[0], name, k))

    if family == "selection":
        run_selection()
    else:
        run_family(family, sys.argv[2] if len(sys.argv) > 2 else None)
    print("FAMILY OK " + family)
""")


def _run_child(family, *args, force=True, timeout=240):
    env = dict(os.environ)
    env.pop("GDV_FORCE_TIER0", None)
    env.pop("GDV_NO_TIER0", None)
    env["GDV_FORCE_TIER0" if force else "GDV_NO_TIER0"] = "1"
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT), family, *args], env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "FAMILY OK " + family in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["arith", "nulls", "dates", "trunc", "adddiff", "seconds", "in"])
def test_family_interpreted_matches_the_oracle(family):
    """arithmetic tail and bitwise / null handling / date casts and extraction / date_trunc, last_day, week / add and diff /
    to_timestamp, to_time / IN — rows 1, 63, 64, 65, 1000, 70 001 at null densities 0, 0.1, 1.0 and a sliced batch at
    offsets 1, 63, 65; dates before 1970, month ends, leap days, year boundaries among the inputs."""
    _run_child(family)


@pytest.mark.gpu
def test_libm_backed_math_interpreted_within_one_ulp_and_bit_equal_to_the_specialised_kernel(tmp_path):
    """cbrt, exp, log, log10, sqrt, power: within 1 ulp of the correctly rounded value, like the specialised kernel's
    (test_parity_gpu.py::test_math_functions_within_one_ulp); floor / ceil / round / truncate: the oracle's bits.  And
    every one of them bit for bit what the specialised kernel gives (the same script run again with GDV_NO_TIER0=1)."""
    _run_child("math", str(tmp_path))
    _run_child("math", str(tmp_path), force=False)
    a, s = np.load(tmp_path / "interpreted.npz"), np.load(tmp_path / "specialised.npz")
    assert sorted(a.files) == sorted(s.files) and len(a.files) > 0
    for key in a.files:
        assert np.array_equal(a[key].view(np.uint64), s[key].view(np.uint64)), f"{key}: the interpreter and the specialised kernel differ"


@pytest.mark.gpu
def test_filter_and_selection_mode_projector_both_interpreted():
    """extractYear(ts) > 2000 as a filter, then selection-mode projectors (uint16 / uint32 / uint64 indices; 1, 64, 65, 1000
    slots out of 70 001 rows; nulls at 0.1; host batches and device-resident ones with the slot count as a number, once with
    the count in device memory, and over a sliced batch) over bool, int8, uint16 and wider columns: the oracle's results,
    and every evaluation counted as a tier-0 launch."""
    _run_child("selection")


_COLD = textwrap.dedent("""
    import os, sys, time, json
    sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
    import numpy as np, pyarrow as pa
    import gandiva_amd as gandiva
    from gandiva_amd import _capi
    from oracle import oracle
    from helpers import assert_bit_exact, random_array
    lib = _capi.lib()
    out = {{}}
    n = 70001
    rng = np.random.default_rng(2)
    TS, U16, I64, BOOL = pa.timestamp("ms"), pa.uint16(), pa.int64(), pa.bool_()
    schema = pa.schema([("ts", TS), ("h", U16), ("k", U16)])
    batch = pa.RecordBatch.from_arrays([random_array(rng, TS, n, 0.1), random_array(rng, U16, n, 0.3), random_array(rng, U16, n, 0.3)], schema=schema)
    b = gandiva.TreeExprBuilder()
    ts, h, k = (b.make_field(schema.field(i)) for i in range(3))
    cond = b.make_condition(b.make_function("greater_than", [b.make_function("extractYear", [ts], I64), b.make_literal(1999, I64)], BOOL))
    exprs = [b.make_expression(b.make_function("date_trunc_Month", [ts], TS), pa.field("m", TS)),
             b.make_expression(b.make_function("nvl", [h, k], U16), pa.field("n", U16))]
    import torch
    torch.cuda.init(); torch.zeros(1, device="cuda"); gandiva.physical_device_count()   # (HIP start-up is not Make's time)
    t0 = time.perf_counter()
    flt = gandiva.make_filter(schema, cond)
    out["make_ms_filter"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    proj = gandiva.make_projector(schema, exprs, None, selection_mode="UINT32")
    out["make_ms_projector"] = (time.perf_counter() - t0) * 1e3
    want_idx = oracle.filter_indices(cond, batch, "int32")
    want = oracle.project(exprs, oracle.take_rows(batch, np.asarray(want_idx)))
    before = lib.gdv_tier0_launches()
    sel = flt.evaluate(batch, dtype="int32")
    out["tier0_filter"] = lib.gdv_tier0_launches() - before
    before = lib.gdv_tier0_launches()
    got = proj.evaluate(batch, selection=sel)
    out["tier0_projector"] = lib.gdv_tier0_launches() - before
    assert sel.to_array().equals(want_idx)
    for g, w in zip(got, want):
        assert_bit_exact(g, w, "selection-mode projector on tier 0")
    # the specialised code objects arrive from the background compiler: evaluations move over, results stay
    deadline = time.time() + 60
    while time.time() < deadline:
        before = lib.gdv_tier0_launches()
        sel = flt.evaluate(batch, dtype="int32"); got = proj.evaluate(batch, selection=sel)
        if lib.gdv_tier0_launches() == before:
            break
        time.sleep(0.05)
    out["moved_to_specialised"] = lib.gdv_tier0_launches() == before
    assert sel.to_array().equals(want_idx)
    for g, w in zip(got, want):
        assert_bit_exact(g, w, "selection-mode projector on the specialised kernel")
    print("RESULT " + json.dumps(out))
""")


@pytest.mark.gpu
def test_cold_make_of_a_date_filter_and_a_selection_mode_projector_returns_at_once(tmp_path):
    """A cold code-object cache and neither switch: make_filter on extractYear(ts) > literal and a selection-mode
    make_projector (date_trunc_Month, nvl) return in milliseconds, their first evaluations run interpreted — the
    oracle's results — and later ones on the specialised kernels the background compiler delivered."""
    env = dict(os.environ, GANDIVA_AMD_CACHE_DIR=str(tmp_path))
    env.pop("GDV_FORCE_TIER0", None)
    env.pop("GDV_NO_TIER0", None)
    r = subprocess.run([sys.executable, "-c", _COLD.format(root=ROOT)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][0][7:])
    assert res["tier0_filter"] == 1 and res["tier0_projector"] == 1, res
    assert res["moved_to_specialised"], res
    assert res["make_ms_filter"] < 100 and res["make_ms_projector"] < 100, res
