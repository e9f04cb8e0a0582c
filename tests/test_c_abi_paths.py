"""Every door of the C ABI into Projector::Evaluate and Filter::Evaluate hands the engine the same buffers: one batch,
one set of operators, every entry point called directly and compared with the oracle."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pytest

import gandiva_amd as gandiva
from gandiva_amd import _capi, shard
from gandiva_amd._capi import (ArrowArray, ArrowDeviceArray, ArrowSchema, gdv_batch_t, gdv_column_t, gdv_filter_batch_t,
                               gdv_out_column_t, gdv_shard_t, release_c_struct)
from gandiva_amd.gandiva import _column_of_array
from oracle import oracle
from helpers import assert_bit_exact

ROWS = 2049  # one past 2048: the host-sharded calls split; crosses validity words and the 1024-row shard alignment
DEVICE, HOST = 1, 0
UINT32 = 2


def _batch():
    rng = np.random.default_rng(7)
    x = pa.array(rng.integers(-1000, 1000, ROWS).astype(np.int32), mask=rng.random(ROWS) < 0.1)
    words = ["".join(chr(97 + c) for c in rng.integers(0, 26, rng.integers(0, 12))) for _ in range(ROWS)]
    s = pa.array(words, type=pa.string(), mask=rng.random(ROWS) < 0.1)
    return pa.RecordBatch.from_arrays([x, s], names=["x", "s"])


def _is_varlen(t):
    return pa.types.is_string(t) or pa.types.is_binary(t)


class _DeviceOuts:
    """Output buffers in HBM for `types` over `rows` rows (var-len data: `data_bytes`), as the C structs and back."""

    def __init__(self, types, rows, data_bytes):
        import torch
        self.types, self.rows = types, rows
        self.c = (gdv_out_column_t * len(types))()
        self.t = []
        words = (rows + 63) // 64 * 8
        for i, t in enumerate(types):
            v = torch.zeros(words + 64, dtype=torch.uint8, device="cuda")
            o = torch.zeros((rows + 1) * 4 + 64, dtype=torch.uint8, device="cuda") if _is_varlen(t) else None
            d = torch.zeros(max(data_bytes if _is_varlen(t) else rows * t.bit_width // 8, 1) + 64, dtype=torch.uint8, device="cuda")
            self.t.append((v, o, d))
            self.c[i].validity, self.c[i].validity_size = v.data_ptr(), v.numel()
            self.c[i].data, self.c[i].data_size = d.data_ptr(), (data_bytes if _is_varlen(t) else d.numel())
            if o is not None:
                self.c[i].offsets, self.c[i].offsets_size = o.data_ptr(), o.numel()

    def arrays(self):
        out = []
        for t, (v, o, d) in zip(self.types, self.t):
            bufs = [pa.py_buffer(v.cpu().numpy())] + ([pa.py_buffer(o.cpu().numpy())] if o is not None else [])
            out.append(pa.Array.from_buffers(t, self.rows, bufs + [pa.py_buffer(d.cpu().numpy())]))
        return out


def _device_cols(dbatch):
    return (gdv_column_t * len(dbatch.columns))(*[c._c() for c in dbatch.columns])


def _rocm_array(dbatch, keep):
    """ARROW_DEVICE_ROCM struct array over the tensors of a DeviceBatch"""
    n = dbatch.num_rows
    children = (C.POINTER(ArrowArray) * len(dbatch.columns))()
    for i, col in enumerate(dbatch.columns):
        ptrs = [col.validity.data_ptr() if col.validity is not None else None]
        ptrs += [col.offsets.data_ptr()] if col.offsets is not None else []
        bufs = (C.c_void_p * len(ptrs + [0]))(*ptrs, col.data.data_ptr())
        child = ArrowArray(n, -1, 0, len(bufs), 0, bufs, None, None, C.c_void_p(1), None)
        keep += [bufs, child]
        children[i] = C.pointer(child)
    top = (C.c_void_p * 1)(None)
    dev = ArrowDeviceArray()
    dev.array = ArrowArray(n, 0, 0, 1, len(dbatch.columns), top, children, None, C.c_void_p(1), None)
    dev.device_id, dev.device_type, dev.sync_event = 0, 10, None
    keep += [top, children, dev]
    return C.addressof(dev)


def _flat_inputs(batch):
    addrs, sizes = [], []
    for col in batch.columns:
        for b in col.buffers():
            addrs.append(b.address if b is not None else 0)
            sizes.append(b.size if b is not None else 0)
    return (C.c_int64 * len(addrs))(*addrs), (C.c_int64 * len(addrs))(*sizes), len(addrs)


def _fetch(ptr, nbytes):
    buf = pa.allocate_buffer(max(nbytes, 1))
    if nbytes:
        assert _capi.lib().gdv_memcpy_d2h(C.c_void_p(buf.address), C.c_void_p(ptr), nbytes) == 0
    return buf


@pytest.mark.gpu
def test_every_door_hands_the_engine_the_same_buffers():
    """Projector (x + x: int32, upper(s): utf8), byte-equal to the oracle through gdv_projector_evaluate (device and host
    buffers), _evaluate_many (1024 + 1025 rows), _evaluate_async, _evaluate_flat, _evaluate_device_array, _evaluate_export
    and, for the fixed-width output alone, _evaluate_sharded / _evaluate_host_sharded over two virtual contexts; the
    var-len plan also goes through _evaluate_host_sharded, which then takes one device.  Every one of these entry points
    accepts var-len outputs; left out for var-len are only the two sharded calls over two contexts (the issue asks for a
    fixed-width plan there: byte positions of a var-len output depend on the shards before it) and
    _evaluate_selected (a device-resident slot count needs fixed-width outputs).  A var-len data buffer that is too
    small gives the same status and the same needed byte count through the plain, flat and device-array calls.
    Filter (x < 7): the same uint32 vector and count through the plain call, async, _evaluate_many, flat, device_array,
    _evaluate_sharded with global indices + gdv_filter_gather_sharded, and _evaluate_host_sharded.  FilterProject: one
    call against the chain of the two operators."""
    import torch
    lib = _capi.lib()
    batch = _batch()
    b = gandiva.TreeExprBuilder()
    fx, fs = b.make_field(batch.schema.field(0)), b.make_field(batch.schema.field(1))
    exprs = [b.make_expression(b.make_function("add", [fx, fx], pa.int32()), pa.field("x2", pa.int32())),
             b.make_expression(b.make_function("upper", [fs], pa.string()), pa.field("u", pa.string()))]
    cond = b.make_condition(b.make_function("less_than", [fx, b.make_literal(7, pa.int32())], pa.bool_()))
    types = [pa.int32(), pa.string()]
    proj = gandiva.make_projector(batch.schema, exprs, None)
    fixed = gandiva.make_projector(batch.schema, exprs[:1], None)
    flt = gandiva.make_filter(batch.schema, cond)
    want = oracle.project(exprs, batch)
    want_sel = oracle.filter_indices(cond, batch, "int32")
    want_idx = want_sel.to_numpy().astype(np.uint32)
    need = int(np.frombuffer(want[1].buffers()[1], dtype=np.int32)[ROWS])  # bytes of upper(s): the oracle's closing offset
    roomy = need + 256
    dbatch = gandiva.DeviceBatch.from_arrow(batch)
    cols = _device_cols(dbatch)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep = []
    before_devices = lib.gdv_device_count()

    def check(got, what, wanted=want):
        for g, w, t in zip(got, wanted, types):
            assert_bit_exact(g, w, f"{what}: {t}")

    try:
        # ---- projector: plain, device buffers
        o = _DeviceOuts(types, ROWS, roomy)
        assert lib.gdv_projector_evaluate(proj._h, ROWS, cols, 2, None, o.c, 2, DEVICE, stream, 0) == 0, _capi.last_error()
        assert o.c[1].data_size == need
        check(o.arrays(), "evaluate, device")
        # ---- plain, host buffers
        hcols = (gdv_column_t * 2)(*[_column_of_array(a) for a in batch.columns])
        hv = [np.zeros((ROWS + 7) // 8, np.uint8) for _ in types]
        hx, hoff, hdata = np.zeros(ROWS, np.int32), np.zeros(ROWS + 1, np.int32), np.zeros(roomy, np.uint8)
        houts = (gdv_out_column_t * 2)()
        houts[0].validity, houts[0].validity_size, houts[0].data, houts[0].data_size = hv[0].ctypes.data, hv[0].nbytes, hx.ctypes.data, hx.nbytes
        houts[1].validity, houts[1].validity_size, houts[1].data, houts[1].data_size = hv[1].ctypes.data, hv[1].nbytes, hdata.ctypes.data, hdata.nbytes
        houts[1].offsets, houts[1].offsets_size = hoff.ctypes.data, hoff.nbytes

        def host_arrays():
            return [pa.Array.from_buffers(types[0], ROWS, [pa.py_buffer(hv[0]), pa.py_buffer(hx)]),
                    pa.Array.from_buffers(types[1], ROWS, [pa.py_buffer(hv[1]), pa.py_buffer(hoff), pa.py_buffer(hdata)])]
        assert lib.gdv_projector_evaluate(proj._h, ROWS, hcols, 2, None, houts, 2, HOST, None, 0) == 0, _capi.last_error()
        assert houts[1].data_size == need
        check(host_arrays(), "evaluate, host")
        # ---- the one-device branch of host_sharded (var-len output)
        for a in hv + [hx, hoff, hdata]:
            a[:] = 0
        houts[1].data_size = hdata.nbytes
        two = (C.c_int32 * 2)(0, 1)
        assert lib.gdv_set_virtual_devices(2) == 0
        assert lib.gdv_projector_evaluate_host_sharded(proj._h, ROWS, hcols, 2, houts, 2, two, 2) == 0, _capi.last_error()
        assert houts[1].data_size == need
        check(host_arrays(), "evaluate_host_sharded, var-len plan")
        # ---- many: 1024 + 1025 rows
        parts = [batch.slice(0, 1024), batch.slice(1024, 1025)]
        parts = [pa.RecordBatch.from_arrays([pa.concat_arrays([c]) for c in p.columns], schema=p.schema) for p in parts]
        dparts = [gandiva.DeviceBatch.from_arrow(p) for p in parts]
        pouts = [_DeviceOuts(types, p.num_rows, roomy) for p in parts]
        pcols = [_device_cols(d) for d in dparts]
        many = (gdv_batch_t * 2)(*[gdv_batch_t(p.num_rows, pcols[i], 2, pouts[i].c, 2) for i, p in enumerate(parts)])
        assert lib.gdv_projector_evaluate_many(proj._h, many, 2, stream, 0) == 0, _capi.last_error()
        for i, p in enumerate(parts):
            pw = oracle.project(exprs, p)
            assert pouts[i].c[1].data_size == int(np.frombuffer(pw[1].buffers()[1], dtype=np.int32)[p.num_rows])
            check(pouts[i].arrays(), f"evaluate_many, batch {i}", pw)
        # ---- async
        o = _DeviceOuts(types, ROWS, roomy)
        result = torch.zeros(3, dtype=torch.int64, device="cuda")
        assert lib.gdv_projector_evaluate_async(proj._h, ROWS, cols, 2, None, None, o.c, 2, stream,
                                                C.c_void_p(result.data_ptr())) == 0, _capi.last_error()
        torch.cuda.synchronize()
        status = result.cpu().tolist()  # [0] device status, [1 + e] bytes output e produced
        assert status[0] == 0 and status[2] == need, status
        check(o.arrays(), "evaluate_async")
        # ---- flat, host buffers
        addrs, sizes, nb = _flat_inputs(batch)
        for a in hv + [hx, hoff, hdata]:
            a[:] = 0
        flat = [hv[0], hx, hv[1], hoff, hdata]
        oa = (C.c_int64 * 5)(*[a.ctypes.data for a in flat])
        osz = (C.c_int64 * 5)(*[a.nbytes for a in flat])
        assert lib.gdv_projector_evaluate_flat(proj._h, ROWS, addrs, sizes, nb, 0, 0, 0, oa, osz, 5, HOST) == 0, _capi.last_error()
        assert osz[4] == need
        check(host_arrays(), "evaluate_flat")
        # ---- device_array
        o = _DeviceOuts(types, ROWS, roomy)
        dev_arr = _rocm_array(dbatch, keep)
        assert lib.gdv_projector_evaluate_device_array(proj._h, dev_arr, None, o.c, 2, stream, 0) == 0, _capi.last_error()
        assert o.c[1].data_size == need
        check(o.arrays(), "evaluate_device_array")
        # ---- export
        exported, schema = ArrowDeviceArray(), ArrowSchema()
        assert lib.gdv_projector_evaluate_export(proj._h, dev_arr, None, stream, C.addressof(exported),
                                                 C.addressof(schema)) == 0, _capi.last_error()
        try:
            torch.cuda.synchronize()
            assert exported.array.n_children == 2 and exported.array.length == ROWS and exported.device_type == 10
            c0, c1 = exported.array.children[0].contents, exported.array.children[1].contents
            offs = _fetch(c1.buffers[1], (ROWS + 1) * 4)
            assert int(np.frombuffer(offs, dtype=np.int32)[ROWS]) == need
            got = [pa.Array.from_buffers(types[0], ROWS, [_fetch(c0.buffers[0], (ROWS + 7) // 8), _fetch(c0.buffers[1], ROWS * 4)]),
                   pa.Array.from_buffers(types[1], ROWS, [_fetch(c1.buffers[0], (ROWS + 7) // 8), offs, _fetch(c1.buffers[2], need)])]
            check(got, "evaluate_export")
        finally:
            release_c_struct(exported)
            release_c_struct(schema)
        # ---- sharded over two virtual contexts, fixed-width plan
        shards = []
        for s in range(2):
            part, _ = shard.shard_record_batch(batch, 2, s)
            part = pa.RecordBatch.from_arrays([pa.concat_arrays([c]) for c in part.columns], schema=part.schema)
            shards.append(gandiva.DeviceBatch.from_arrow(part))
        assert [d.num_rows for d in shards] == [2048, 1]  # three 1024-row tiles over two shards
        souts = [_DeviceOuts(types[:1], d.num_rows, 0) for d in shards]
        scols = [_device_cols(d) for d in shards]
        arr = (gdv_shard_t * 2)()
        for s in range(2):
            arr[s].device, arr[s].cols, arr[s].outs = s, scols[s], souts[s].c
        assert lib.gdv_projector_evaluate_sharded(fixed._h, ROWS, 2, 1, arr, 2, 0) == 0, _capi.last_error()
        got = pa.concat_arrays([souts[s].arrays()[0] for s in range(2)])
        assert_bit_exact(got, want[0], "evaluate_sharded")
        # ---- host_sharded over the same two contexts
        hv[0][:] = 0
        hx[:] = 0
        assert lib.gdv_projector_evaluate_host_sharded(fixed._h, ROWS, hcols, 2, houts, 1, two, 2) == 0, _capi.last_error()
        assert_bit_exact(host_arrays()[0], want[0], "evaluate_host_sharded")

        # ---- a var-len data buffer that is too small: same status, same needed byte count
        small = 16
        o = _DeviceOuts(types, ROWS, small)
        plain = (lib.gdv_projector_evaluate(proj._h, ROWS, cols, 2, None, o.c, 2, DEVICE, stream, 0), o.c[1].data_size)
        osz = (C.c_int64 * 5)(*[a.nbytes for a in flat[:4]], small)
        flat_rc = lib.gdv_projector_evaluate_flat(proj._h, ROWS, addrs, sizes, nb, 0, 0, 0, oa, osz, 5, HOST)
        o = _DeviceOuts(types, ROWS, small)
        darr = (lib.gdv_projector_evaluate_device_array(proj._h, dev_arr, None, o.c, 2, stream, 0), o.c[1].data_size)
        print("too small: plain", plain, "flat", (flat_rc, osz[4]), "device_array", darr, "oracle bytes", need)
        assert plain == (flat_rc, osz[4]) == darr
        assert plain[0] != 0 and plain[1] == need

        # ---- filter
        def device_vector():
            return torch.zeros(ROWS, dtype=torch.int32, device="cuda")

        def same(idx, count, what):
            got = idx[:count].cpu().numpy() if isinstance(idx, torch.Tensor) else idx[:count]
            assert count == len(want_idx), f"{what}: count {count} != {len(want_idx)}"
            assert np.array_equal(got.view(np.uint32), want_idx), what
        count = C.c_int64()
        idx = device_vector()
        assert lib.gdv_filter_evaluate(flt._h, ROWS, cols, 2, UINT32, C.c_void_p(idx.data_ptr()), ROWS, C.byref(count), DEVICE,
                                       stream) == 0, _capi.last_error()
        same(idx, count.value, "filter_evaluate")
        idx, dcount = device_vector(), torch.zeros(1, dtype=torch.int64, device="cuda")
        assert lib.gdv_filter_evaluate_async(flt._h, ROWS, cols, 2, UINT32, C.c_void_p(idx.data_ptr()), ROWS,
                                             C.c_void_p(dcount.data_ptr()), stream) == 0, _capi.last_error()
        torch.cuda.synchronize()
        same(idx, int(dcount.item()), "filter_evaluate_async")
        pidx = [device_vector(), device_vector()]
        fmany = (gdv_filter_batch_t * 2)(*[gdv_filter_batch_t(p.num_rows, pcols[i], 2, pidx[i].data_ptr(), ROWS)
                                          for i, p in enumerate(parts)])
        counts = (C.c_int64 * 2)()
        assert lib.gdv_filter_evaluate_many(flt._h, fmany, 2, UINT32, counts, None, stream, 0) == 0, _capi.last_error()
        joined = torch.cat([pidx[0][:counts[0]], pidx[1][:counts[1]] + 1024])
        same(joined, counts[0] + counts[1], "filter_evaluate_many")
        hidx = np.zeros(ROWS, np.uint32)
        assert lib.gdv_filter_evaluate_flat(flt._h, ROWS, addrs, sizes, nb, UINT32, hidx.ctypes.data, hidx.nbytes,
                                            C.byref(count), HOST) == 0, _capi.last_error()
        same(hidx, count.value, "filter_evaluate_flat")
        idx = device_vector()
        assert lib.gdv_filter_evaluate_device_array(flt._h, dev_arr, UINT32, C.c_void_p(idx.data_ptr()), ROWS, C.byref(count),
                                                    stream) == 0, _capi.last_error()
        same(idx, count.value, "filter_evaluate_device_array")
        sidx = [device_vector(), device_vector()]
        farr = (gdv_shard_t * 2)()
        for s in range(2):
            farr[s].device, farr[s].cols = s, scols[s]
            farr[s].out_indices, farr[s].max_slots = sidx[s].data_ptr(), shards[s].num_rows
        total = C.c_int64()
        assert lib.gdv_filter_evaluate_sharded(flt._h, ROWS, 2, UINT32, farr, 2, 2, C.byref(total)) == 0, _capi.last_error()
        idx = device_vector()
        assert lib.gdv_filter_gather_sharded(farr, 2, UINT32, 0, C.c_void_p(idx.data_ptr()), ROWS) == 0, _capi.last_error()
        same(idx, total.value, "filter_evaluate_sharded + gather")
        hidx[:] = 0
        assert lib.gdv_filter_evaluate_host_sharded(flt._h, ROWS, hcols, 2, UINT32, hidx.ctypes.data, ROWS, C.byref(count),
                                                    two, 2) == 0, _capi.last_error()
        same(hidx, count.value, "filter_evaluate_host_sharded")

        # ---- filter-project against the chain filter -> projector in selection mode
        fp = gandiva.make_filter_project(batch.schema, cond, exprs[:1], "int32")
        o = _DeviceOuts(types[:1], ROWS, 0)
        idx = device_vector()
        assert lib.gdv_filter_project_evaluate(fp._h, ROWS, cols, 2, o.c, 1, C.c_void_p(idx.data_ptr()), ROWS, C.byref(count),
                                               None, DEVICE, stream, 0) == 0, _capi.last_error()
        same(idx, count.value, "filter_project_evaluate")
        chained = gandiva.make_projector(batch.schema, exprs[:1], None, "UINT32")
        sel = _capi.gdv_selection_t(UINT32, idx.data_ptr(), count.value)
        co = _DeviceOuts(types[:1], count.value, 0)
        assert lib.gdv_projector_evaluate(chained._h, ROWS, cols, 2, C.byref(sel), co.c, 1, DEVICE, stream, 0) == 0, _capi.last_error()
        assert_bit_exact(o.arrays()[0].slice(0, count.value), co.arrays()[0], "filter_project_evaluate against the chain")
        assert_bit_exact(co.arrays()[0], oracle.take_rows(want[0], want_sel), "the chain against the oracle")
    finally:
        torch.cuda.synchronize()
        gandiva.set_virtual_devices(0 if before_devices == lib.gdv_physical_device_count() else before_devices)
