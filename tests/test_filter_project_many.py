"""gdv_filter_project_evaluate_many / FilterProject.evaluate_device_many: a list of small HBM-resident batches filtered
and projected in ONE launch, every batch by one workgroup (the plan's SMALL shape: the windowed body with a running
total in LDS instead of the look-back; the workgroup zeroes its own bitmaps).

The reference is FilterProject.evaluate_device on each batch ALONE (the look-back kernels of the one-batch call):
per batch the data rows [0, count), the validity / boolean words [0, ceil(count / 64)), the indices and the count
must be equal bit for bit — and, once, equal to the oracle's Filter -> take -> Projector chain.  Outputs and index
buffers always arrive filled with 0xFF and are followed by 64 guard bytes.

Three plans: test_filter_project's threshold plan (a boolean output, nullable inputs; the threshold is a literal, i.e.
a kernel ARGUMENT: every selectivity runs the same kernels), its first three expressions (cannot raise: truly
asynchronous) and a bare division (raises on selected rows only).
"""
import re

import numpy as np
import pyarrow as pa
import pytest

import gandiva_amd as gandiva
from gandiva_amd import gandiva as gg
from helpers import assert_bit_exact
from test_filter_project import _batch, _chain, _plan

I64, BOOL = pa.int64(), pa.bool_()
GUARD = 64
THRESHOLDS = [5000, -1, 499, 998]     # none / every row (every wave tile overflows the window) / half / ~0.1 %
MAX_ROWS = 1 << 17                    # no plan's cap is above 2^17 rows

_cache = {}


def _source(nulls):
    """ONE host batch and its device copy per null density; every batch of the tests is its first n rows."""
    key = ("source", nulls)
    if key not in _cache:
        batch = _batch(np.random.default_rng(1234 + int(nulls * 100)), MAX_ROWS + 1, nulls)
        _cache[key] = (batch, gandiva.DeviceBatch.from_arrow(batch))
    return _cache[key]


def _first_rows(db, n):
    cols = [gg.DeviceColumn(c.type, n, c.validity, c.data, None, 0) for c in db.columns]
    return gandiva.DeviceBatch(db.schema, cols, n)


def _fp(kind, threshold, dtype, nulls=0.0):
    key = ("fp", kind, threshold, dtype)
    if key not in _cache:
        schema = _source(nulls)[0].schema
        cond, exprs = _plan(schema, threshold)
        if kind == "no-raise":
            exprs = exprs[:3]
        fp = gandiva.make_filter_project(schema, cond, exprs, dtype)
        assert fp.fused and fp.small_batch_rows > 0
        _cache[key] = (fp, cond, exprs)
    return _cache[key]


def _tiles(fp):
    """(rows of a wave tile, rows of a workgroup tile, GDV_FP_CAP) from the plan's own text"""
    ir = fp.llvm_ir
    u, waves, k, cap = (int(re.search(rf"#define {name} (\d+)", ir).group(1))
                        for name in ("GDV_U", "GDV_WAVES", "GDV_FP_K", "GDV_FP_CAP"))
    return 64 * u * k, 64 * u * k * waves, cap


def _cap(fp, nb=1):
    """rows per batch up to which a list of nb batches is one launch: the plan's rows for one workgroup, times nb"""
    return min(MAX_ROWS, nb * fp.small_batch_rows)


def _row_counts(fp):
    wave, wg, window = _tiles(fp)
    cap = _cap(fp)
    assert 0 < cap <= MAX_ROWS and window < wave
    return [1, 63, 64, 65, wave - 1, wave, wave + 1, wg - 1, wg, wg + 1, 3 * wg + 77, cap], cap


def _dirty(nbytes):
    """nbytes + GUARD bytes of 0xFF; the first nbytes are what the library is told about"""
    import torch
    full = torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    return full, full[:nbytes]


class _Buffers:
    """dirty outputs + index buffer of one batch, each followed by guard bytes"""

    def __init__(self, fp, n, short_validity=0, drop_outputs=0, short_index=0):
        import torch
        self.fulls, self.columns = [], []
        words = (n + 63) // 64
        for t in fp._out_types[:len(fp._out_types) - drop_outputs]:
            vfull, v = _dirty(max(words * 8 - short_validity, 0))
            dfull, d = _dirty(words * 8 if pa.types.is_boolean(t) else n * t.bit_width // 8)
            self.fulls += [vfull, dfull]
            self.columns.append(gg.DeviceColumn(t, n, v, d))
        self.indices = None
        if fp._mode:
            width = {1: 2, 2: 4, 3: 8}[fp._mode]
            ifull, i = _dirty(max(n - short_index, 0) * width)
            self.fulls.append(ifull)
            self.indices = i.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[width])

    def guards_intact(self):
        return all(bool((f[-GUARD:] == 0xFF).all()) for f in self.fulls)

    def untouched(self):
        return all(bool((f == 0xFF).all()) for f in self.fulls)


def _reference(fp, key, db):
    """the one-batch call on this batch alone, once: (count, per output (validity words, data bytes), index bytes)"""
    import torch
    key = ("ref",) + key
    if key not in _cache:
        outs, sel = fp.evaluate_device(db)
        torch.cuda.synchronize()
        k = outs[0].num_rows if db.num_rows else 0
        _cache[key] = (k, [_used(o, k) for o in outs], None if sel is None else _used_indices(sel.indices, k))
    return _cache[key]


def _used(col, k):
    words = (k + 63) // 64
    data = col.data[:words * 8] if pa.types.is_boolean(col.type) else col.data[:k * col.type.bit_width // 8]
    return col.validity[:words * 8].clone(), data.clone()


def _used_indices(indices, k):
    import torch
    return indices[:k].clone().view(torch.uint8)


def _assert_equals_reference(got, ref, what):
    import torch
    (outs, sel), (k, ref_outs, ref_idx) = got, ref
    for e, (o, (rv, rd)) in enumerate(zip(outs, ref_outs)):
        assert o.num_rows == k, f"{what}: count {o.num_rows}, alone {k}"
        gv, gd = _used(o, k)
        assert torch.equal(gv, rv), f"{what}: validity words of output {e}"
        assert torch.equal(gd, rd), f"{what}: data of output {e}"
    if ref_idx is None:
        assert sel is None
    else:
        assert sel.num_slots == k, f"{what}: slots {sel.num_slots}, alone {k}"
        assert torch.equal(_used_indices(sel.indices, k), ref_idx), f"{what}: indices"


def _run(fp, dbs, sync=True):
    bufs = [_Buffers(fp, db.num_rows) for db in dbs]
    res = fp.evaluate_device_many(dbs, outputs=[b.columns for b in bufs], indices=[b.indices for b in bufs], sync=sync)
    return res, bufs


# ------------------------------------------------------------------------------------------ equality

@pytest.mark.gpu
@pytest.mark.parametrize("nulls", [0.0, 0.15])
@pytest.mark.parametrize("dtype", [None, "int16", "int32", "int64"])
def test_every_batch_equals_the_one_batch_call(dtype, nulls):
    """Every row count in ONE call (one workgroup each, one launch: twelve batches may have twelve times the rows one
    batch may), then the cap and cap + 1 in calls of their own (the by-value entry; the fallback), at four
    selectivities; compared with evaluate_device on the batch alone."""
    import torch
    _, src = _source(nulls)
    for thr in THRESHOLDS:
        fp, _, _ = _fp("threshold", thr, dtype)
        sizes, cap = _row_counts(fp)
        assert max(sizes) <= _cap(fp, len(sizes))     # the list is one launch
        dbs = [_first_rows(src, n) for n in sizes]
        res, bufs = _run(fp, dbs)
        torch.cuda.synchronize()
        for n, db, r, b in zip(sizes, dbs, res, bufs):
            _assert_equals_reference(r, _reference(fp, (thr, dtype, nulls, n), db), f"{n} rows, threshold {thr}")
            assert b.guards_intact(), f"{n} rows: guard bytes"
        for n in (cap, cap + 1):
            db = _first_rows(src, n)
            res, bufs = _run(fp, [db])
            torch.cuda.synchronize()
            _assert_equals_reference(res[0], _reference(fp, (thr, dtype, nulls, n), db), f"{n} rows alone, threshold {thr}")
            assert bufs[0].guards_intact()


@pytest.mark.gpu
def test_the_results_are_the_oracle_chain():
    """once against Filter -> take -> Projector as the oracle states it (values, validity, bool output, indices)"""
    host, src = _source(0.15)
    fp, cond, exprs = _fp("threshold", 499, "int32")
    wave, wg, _ = _tiles(fp)
    sizes = [65, wg + 1, _cap(fp)]
    assert max(sizes) <= _cap(fp, 3)
    res, _ = _run(fp, [_first_rows(src, n) for n in sizes])
    for n, (outs, sel) in zip(sizes, res):
        want_sel, want = _chain(cond, exprs, host.slice(0, n), "int32")
        assert sel.to_array().equals(want_sel), n
        for e, (o, w) in enumerate(zip(outs, want)):
            assert_bit_exact(o.to_arrow(), w, f"{n} rows, expression {e}")
    # ... and as the library's own two operators give it: Filter, then a selection-mode Projector over its vector
    flt = gandiva.make_filter(host.schema, cond)
    proj = gandiva.make_projector(host.schema, exprs, None, "UINT32")
    for n, (outs, sel) in zip(sizes, res):
        db = _first_rows(src, n)
        chain_sel = flt.evaluate_device(db, "int32")
        chain_outs = proj.evaluate_device(db, selection=chain_sel)
        assert sel.to_array().equals(chain_sel.to_array()), n
        for e, (o, c) in enumerate(zip(outs, chain_outs)):
            assert_bit_exact(o.to_arrow(), c.to_arrow(), f"{n} rows, expression {e}, Filter + Projector")


# ------------------------------------------------------------------------------------------ batch lists

def _list_sizes(nb, fp):
    wave, wg, _ = _tiles(fp)
    if nb == 1:
        return [min(wg + 1, _cap(fp))]
    if nb == 3:
        return [wave - 1, wg + 77, 65]
    return [1 + (37 * b) % (wave + 130) for b in range(nb)]


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [1, 3, 257])
def test_batch_lists_and_the_forced_fallback(nb):
    """one batch (its argument block travels by value), three sizes in one call, 257 batches; the same list with "small" = 0
    (batch by batch through the one-batch path) gives identical results"""
    import torch
    _, src = _source(0.15)
    fp, _, _ = _fp("threshold", 499, "int32")
    sizes = _list_sizes(nb, fp)
    assert max(sizes) <= _cap(fp, nb)
    dbs = [_first_rows(src, n) for n in sizes]
    res, bufs = _run(fp, dbs)
    fp.set_tuning("small", 0)
    try:
        res0, bufs0 = _run(fp, dbs)
    finally:
        fp.set_tuning("small", 1)
    torch.cuda.synchronize()
    for b, (n, db) in enumerate(zip(sizes, dbs)):
        ref = _reference(fp, (499, "int32", 0.15, n), db)
        _assert_equals_reference(res[b], ref, f"batch {b} of {nb} ({n} rows)")
        _assert_equals_reference(res0[b], ref, f"batch {b} of {nb} ({n} rows), small = 0")
        assert bufs[b].guards_intact() and bufs0[b].guards_intact()


@pytest.mark.gpu
def test_a_batch_of_no_rows_is_not_touched():
    import torch
    _, src = _source(0.0)
    fp, _, _ = _fp("threshold", 499, "int32")
    dbs = [_first_rows(src, 1000), _first_rows(src, 0), _first_rows(src, 65)]
    for small in (1, 0):
        fp.set_tuning("small", small)
        try:
            bufs = [_Buffers(fp, 1000), _Buffers(fp, 64), _Buffers(fp, 65)]   # (the empty batch brings real buffers)
            res = fp.evaluate_device_many(dbs, outputs=[b.columns for b in bufs], indices=[b.indices for b in bufs])
        finally:
            fp.set_tuning("small", 1)
        torch.cuda.synchronize()
        assert res[1][1].num_slots == 0 and all(o.num_rows == 0 for o in res[1][0])
        assert bufs[1].untouched(), f"small = {small}: a 0-row batch's buffers were written"
        for b in (0, 2):
            _assert_equals_reference(res[b], _reference(fp, (499, "int32", 0.0, dbs[b].num_rows), dbs[b]), f"batch {b}")
            assert bufs[b].guards_intact()
    assert fp.evaluate_device_many([]) == []


@pytest.mark.gpu
def test_a_list_is_one_launch_and_the_fallback_is_one_per_batch():
    """GDV_TRACE (read once per process: a subprocess) prints one line per evaluation: a list of three small batches is ONE
    "filter-project-small" evaluation over 3 batches — not three of the one-batch kind —, the same list with "small" = 0, or
    with a batch above the cap, is three "filter-project" evaluations and no small one."""
    import os, subprocess, sys, textwrap
    code = textwrap.dedent("""
        import sys
        sys.path.insert(0, %r); sys.path.insert(0, %r)
        import test_filter_project_many as T
        _, src = T._source(0.0)
        fp, _, _ = T._fp("threshold", 499, "int32")
        dbs = [T._first_rows(src, n) for n in (1000, 65, 3000)]
        print("MARK one launch", file=sys.stderr, flush=True)
        T._run(fp, dbs)
        print("MARK by value", file=sys.stderr, flush=True)
        T._run(fp, dbs[:1])
        print("MARK small = 0", file=sys.stderr, flush=True)
        fp.set_tuning("small", 0)
        T._run(fp, dbs)
        fp.set_tuning("small", 1)
        print("MARK above the cap", file=sys.stderr, flush=True)
        T._run(fp, dbs[:2] + [T._first_rows(src, T._cap(fp, 3) + 1)])
        print("MARK one batch above the cap", file=sys.stderr, flush=True)
        T._run(fp, [T._first_rows(src, T._cap(fp) + 1)])
        print("MARK end", file=sys.stderr, flush=True)
    """) % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GDV_TRACE="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    parts = r.stderr.split("MARK ")
    section = {p.split("\n", 1)[0]: [ln for ln in p.split("\n")[1:] if ln.startswith("[gdv] filter-project")] for p in parts[1:]}
    assert len(section["one launch"]) == 1 and "[gdv] filter-project-small " in section["one launch"][0] and " rows=3 " in section["one launch"][0]
    assert "_small " in section["one launch"][0]                       # the small kernel's own name
    assert len(section["by value"]) == 1 and "_small1 " in section["by value"][0] and " rows=1 " in section["by value"][0]
    for name, lines in (("small = 0", 3), ("above the cap", 3), ("one batch above the cap", 1)):
        assert len(section[name]) == lines and all(ln.startswith("[gdv] filter-project ") for ln in section[name]), section[name]


# ------------------------------------------------------------------------------------------ asynchronous

@pytest.mark.gpu
def test_asynchronous_counts_stay_on_the_device():
    import torch
    _, src = _source(0.15)
    fp, _, _ = _fp("no-raise", 499, "int32")
    wave, wg, _ = _tiles(fp)
    sizes = [wave + 1, 65, wg + 77]
    assert max(sizes) <= _cap(fp, 3)
    dbs = [_first_rows(src, n) for n in sizes]
    sync_res, _ = _run(fp, dbs)
    res, bufs = _run(fp, dbs, sync=False)
    for n, (outs, sel) in zip(sizes, res):
        assert sel.pending and all(o.count_tensor is not None and o.length == n for o in outs)   # host counts were -1
    torch.cuda.synchronize()
    counts = fp.last_count_tensor.cpu().tolist()
    for b, n in enumerate(sizes):
        k = sync_res[b][1].num_slots
        assert counts[b] == k
        ref = (k, [_used(o, k) for o in sync_res[b][0]], _used_indices(sync_res[b][1].indices, k))
        _assert_equals_reference(res[b], ref, f"batch {b}, asynchronous")
        assert bufs[b].guards_intact()


# ------------------------------------------------------------------------------------------ raising

@pytest.mark.gpu
def test_a_division_raises_on_selected_rows_only():
    import torch
    n = 5000
    a = np.arange(n, dtype=np.int64)
    b = np.where(a % 2 == 0, 0, 3).astype(np.int64)          # every even row would divide by zero
    schema = pa.schema([pa.field("a", I64), pa.field("b", I64)])
    bld = gandiva.TreeExprBuilder()
    fa, fb = bld.make_field(schema.field(0)), bld.make_field(schema.field(1))
    div = bld.make_expression(bld.make_function("divide", [fa, fb], I64), pa.field("q", I64))
    odd = bld.make_condition(bld.make_function("equal", [bld.make_function("mod", [fa, bld.make_literal(2, I64)], I64),
                                                         bld.make_literal(1, I64)], BOOL))
    fp = gandiva.make_filter_project(schema, odd, [div], "int32")
    assert fp.fused and _cap(fp, 3) >= n
    good = pa.RecordBatch.from_arrays([pa.array(a), pa.array(b)], schema=schema)
    bad_b = b.copy()
    bad_b[4001] = 0                                           # a zero in a SELECTED row
    bad = pa.RecordBatch.from_arrays([pa.array(a), pa.array(bad_b)], schema=schema)
    dgood, dbad = gandiva.DeviceBatch.from_arrow(good), gandiva.DeviceBatch.from_arrow(bad)
    lists = [_first_rows(dgood, 5000), _first_rows(dgood, 777), _first_rows(dgood, 4000)]
    res, bufs = _run(fp, lists)
    torch.cuda.synchronize()
    for db, (outs, sel) in zip(lists, res):
        want_sel, want = _chain(odd, [div], good.slice(0, db.num_rows), "int32")
        assert sel.to_array().equals(want_sel)
        assert_bit_exact(outs[0].to_arrow(), want[0])
    assert all(x.guards_intact() for x in bufs)
    with pytest.raises(pa.lib.ArrowException, match="divide by zero"):
        _run(fp, [_first_rows(dgood, 5000), _first_rows(dbad, 5000), _first_rows(dgood, 4000)])   # batch 2 of 3 raises
    with pytest.raises(pa.lib.ArrowException, match="divide by zero"):                           # asked not to wait: waits anyway
        _run(fp, [_first_rows(dgood, 5000), _first_rows(dbad, 5000), _first_rows(dgood, 4000)], sync=False)


# ------------------------------------------------------------------------------------------ argument checks

@pytest.mark.gpu
@pytest.mark.parametrize("fault", ["num_outs", "short validity", "max_slots", "uint16 rows"])
def test_argument_checks_name_the_batch_and_enqueue_nothing(fault):
    import torch
    _, src = _source(0.0)
    dtype = "int16" if fault == "uint16 rows" else "int32"
    fp, _, _ = _fp("threshold", 499, dtype)
    n_bad = 65537 if fault == "uint16 rows" else 1000
    dbs = [_first_rows(src, 1000), _first_rows(src, n_bad), _first_rows(src, 65)]
    bad = {"num_outs": dict(drop_outputs=1), "short validity": dict(short_validity=8), "max_slots": dict(short_index=1),
           "uint16 rows": {}}[fault]
    message = {"num_outs": "batch 1: number of output buffers does not match", "short validity": "batch 1: output buffer 0 too small",
               "max_slots": "batch 1: Selection vector too small", "uint16 rows": "batch 1: uint16 selection vector cannot address 65537"}[fault]
    for small in (1, 0):
        bufs = [_Buffers(fp, 1000), _Buffers(fp, n_bad, **bad), _Buffers(fp, 65)]
        fp.set_tuning("small", small)
        try:
            with pytest.raises(pa.lib.ArrowInvalid, match=message):
                fp.evaluate_device_many(dbs, outputs=[b.columns for b in bufs], indices=[b.indices for b in bufs])
        finally:
            fp.set_tuning("small", 1)
        torch.cuda.synchronize()
        assert all(b.untouched() for b in bufs), f"{fault}: something was enqueued before the check failed"


@pytest.mark.gpu
def test_the_c_entry_point_takes_an_empty_and_refuses_a_null_list():
    import ctypes as C
    from gandiva_amd import _capi
    lib = _capi.lib()
    fp, _, _ = _fp("threshold", 499, "int32")
    assert lib.gdv_filter_project_evaluate_many(fp._h, None, 0, None, None, None, 0) == 0
    rc = lib.gdv_filter_project_evaluate_many(fp._h, None, 2, None, None, None, 0)
    assert rc != 0 and "null batch list" in _capi.last_error()
    with pytest.raises(pa.lib.ArrowException, match="unknown key or value out of range"):
        fp.set_tuning("small", 2)
