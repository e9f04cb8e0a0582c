"""The refusals of the C ABI, pinned: for a bad argument every entry point returns the same status code and leaves
the same gdv_last_error() text as the library did before gdv_c_api.cc was split into units and its marshalling folded
(the EXPECTED tables were written by running these cases against a library built from the commit before the split).

Every case returns before the library makes a HIP call.  The first table needs no device at all: a null handle, or no
handle.  The second table sits behind a `null handle` check, and an operator handle exists only where Make finds a
device (there is no CPU fallback), so those cases are marked gpu; they still launch nothing."""
import ctypes as C
import threading

import numpy as np
import pyarrow as pa
import pytest

import gandiva_amd as gandiva
from gandiva_amd import _capi, gandiva as gg
from gandiva_amd._capi import (ArrowArray, ArrowDeviceArray, gdv_batch_t, gdv_column_t, gdv_filter_batch_t,
                               gdv_out_column_t, gdv_selection_t, gdv_shard_t)
import proto_encode as P

NULL_PTR = "NULL"  # what a pointer-returning entry point gives back on failure


def _outcome(ret):
    """(code or NULL_PTR, last error) of a failed call"""
    lib = _capi.lib()
    if ret is None or isinstance(ret, int) and not isinstance(ret, bool):
        code = NULL_PTR if ret is None else ret
    else:
        raise AssertionError(f"unexpected return {ret!r}")
    return code, lib.gdv_last_error().decode()


# ------------------------------------------------------------------ fixtures the cases share (built once, host only)

class _Trees:
    def __init__(self):
        b = gandiva.TreeExprBuilder()
        self.schema = pa.schema([pa.field("x", pa.int32()), pa.field("s", pa.string())])
        x, s = b.make_field(self.schema.field(0)), b.make_field(self.schema.field(1))
        self.exprs = [b.make_expression(b.make_function("add", [x, x], pa.int32()), pa.field("x2", pa.int32())),
                      b.make_expression(b.make_function("upper", [s], pa.string()), pa.field("u", pa.string()))]
        self.fixed = [self.exprs[0]]
        self.cond = b.make_condition(b.make_function("less_than", [x, b.make_literal(7, pa.int32())], pa.bool_()))
        self.sh = gg._make_schema(self.schema)
        self.keep = b

    def handles(self, exprs):
        return (C.c_void_p * len(exprs))(*[e._h for e in exprs])


@pytest.fixture(scope="module")
def trees():
    return _Trees()


ONE_COL = (gdv_column_t * 1)()
ONE_OUT = (gdv_out_column_t * 1)()
ONE_SHARD = (gdv_shard_t * 1)()
ONE_DEV = (C.c_int32 * 1)(0)
I64 = C.c_int64()
SOME = C.c_void_p(64)  # a non-null address that is never dereferenced


def _sel(mode):
    return C.byref(gdv_selection_t(mode, None, 0))


def _gather_shards(counts):
    arr = (gdv_shard_t * len(counts))()
    for i, n in enumerate(counts):
        arr[i].num_selected = n
    return arr


def _truncated(t):
    eb = P.expression_list(t.exprs)
    return eb[:len(eb) - 3]


# ------------------------------------------------------------------ no device needed

CPU_CASES = {
    # null handles, every evaluate variant
    "projector_evaluate/null": lambda lib, t: lib.gdv_projector_evaluate(None, 8, ONE_COL, 1, None, ONE_OUT, 1, 0, None, 0),
    "projector_evaluate_selected/null": lambda lib, t: lib.gdv_projector_evaluate_selected(None, 8, ONE_COL, 1, _sel(2), SOME, ONE_OUT, 1, None, 0),
    "projector_evaluate_async/null": lambda lib, t: lib.gdv_projector_evaluate_async(None, 8, ONE_COL, 1, None, None, ONE_OUT, 1, None, SOME),
    "projector_evaluate_many/null": lambda lib, t: lib.gdv_projector_evaluate_many(None, (gdv_batch_t * 1)(), 1, None, 0),
    "projector_evaluate_flat/null": lambda lib, t: lib.gdv_projector_evaluate_flat(None, 8, None, None, 0, 0, 0, 0, None, None, 0, 0),
    "projector_evaluate_device_array/null": lambda lib, t: lib.gdv_projector_evaluate_device_array(None, None, None, ONE_OUT, 1, None, 0),
    "projector_evaluate_export/null": lambda lib, t: lib.gdv_projector_evaluate_export(None, None, None, None, None, None),
    "projector_evaluate_sharded/null": lambda lib, t: lib.gdv_projector_evaluate_sharded(None, 8, 1, 1, ONE_SHARD, 1, 0),
    "projector_evaluate_host_sharded/null": lambda lib, t: lib.gdv_projector_evaluate_host_sharded(None, 8, ONE_COL, 1, ONE_OUT, 1, ONE_DEV, 1),
    "filter_evaluate/null": lambda lib, t: lib.gdv_filter_evaluate(None, 8, ONE_COL, 1, 2, SOME, 8, C.byref(I64), 0, None),
    "filter_evaluate_async/null": lambda lib, t: lib.gdv_filter_evaluate_async(None, 8, ONE_COL, 1, 2, SOME, 8, SOME, None),
    "filter_evaluate_many/null": lambda lib, t: lib.gdv_filter_evaluate_many(None, (gdv_filter_batch_t * 1)(), 1, 2, C.byref(I64), None, None, 0),
    "filter_evaluate_flat/null": lambda lib, t: lib.gdv_filter_evaluate_flat(None, 8, None, None, 0, 2, 0, 0, C.byref(I64), 0),
    "filter_evaluate_device_array/null": lambda lib, t: lib.gdv_filter_evaluate_device_array(None, None, 2, SOME, 8, C.byref(I64), None),
    "filter_evaluate_sharded/null": lambda lib, t: lib.gdv_filter_evaluate_sharded(None, 8, 1, 2, ONE_SHARD, 1, 0, None),
    "filter_evaluate_host_sharded/null": lambda lib, t: lib.gdv_filter_evaluate_host_sharded(None, 8, ONE_COL, 1, 2, SOME, 8, C.byref(I64), ONE_DEV, 1),
    "filter_project_evaluate/null": lambda lib, t: lib.gdv_filter_project_evaluate(None, 8, ONE_COL, 1, ONE_OUT, 1, SOME, 8, C.byref(I64), None, 0, None, 0),
    # evaluate_selected wants both halves of the device-resident selection
    "projector_evaluate_selected/no_sel": lambda lib, t: lib.gdv_projector_evaluate_selected(None, 8, ONE_COL, 1, None, SOME, ONE_OUT, 1, None, 0),
    "projector_evaluate_selected/no_count": lambda lib, t: lib.gdv_projector_evaluate_selected(None, 8, ONE_COL, 1, _sel(2), None, ONE_OUT, 1, None, 0),
    # the gather needs no operator
    "filter_gather_sharded/mode-1": lambda lib, t: lib.gdv_filter_gather_sharded(_gather_shards([1]), 1, -1, 0, SOME, 8),
    "filter_gather_sharded/mode4": lambda lib, t: lib.gdv_filter_gather_sharded(_gather_shards([1]), 1, 4, 0, SOME, 8),
    "filter_gather_sharded/mode_none": lambda lib, t: lib.gdv_filter_gather_sharded(_gather_shards([1]), 1, 0, 0, SOME, 8),
    "filter_gather_sharded/no_shards": lambda lib, t: lib.gdv_filter_gather_sharded(_gather_shards([1]), 0, 2, 0, SOME, 8),
    "filter_gather_sharded/too_many": lambda lib, t: lib.gdv_filter_gather_sharded(_gather_shards([5, 6]), 2, 2, 0, SOME, 10),
    # make: the checks that come before the device is looked for
    "projector_make/mode-1": lambda lib, t: lib.gdv_projector_make(t.sh, t.handles(t.exprs), 2, -1, None, C.byref(C.c_void_p())),
    "projector_make/mode4": lambda lib, t: lib.gdv_projector_make(t.sh, t.handles(t.exprs), 2, 4, None, C.byref(C.c_void_p())),
    "projector_make/null_expr": lambda lib, t: lib.gdv_projector_make(t.sh, (C.c_void_p * 1)(None), 1, 0, None, C.byref(C.c_void_p())),
    "projector_make/null_schema": lambda lib, t: lib.gdv_projector_make(None, t.handles(t.exprs), 2, 0, None, C.byref(C.c_void_p())),
    "filter_make/null_condition": lambda lib, t: lib.gdv_filter_make(t.sh, None, None, C.byref(C.c_void_p())),
    "filter_project_make/mode4": lambda lib, t: lib.gdv_filter_project_make(t.sh, t.cond._h, t.handles(t.fixed), 1, 4, None, C.byref(C.c_void_p())),
    "filter_project_make/null_expr": lambda lib, t: lib.gdv_filter_project_make(t.sh, t.cond._h, (C.c_void_p * 1)(None), 1, 2, None, C.byref(C.c_void_p())),
    "filter_project_make/no_exprs": lambda lib, t: lib.gdv_filter_project_make(t.sh, t.cond._h, None, 0, 2, None, C.byref(C.c_void_p())),
    # protobuf
    "projector_make_from_proto/negative": lambda lib, t: lib.gdv_projector_make_from_proto(b"", -1, b"", 0, 0, None, C.byref(C.c_void_p())),
    "filter_make_from_proto/negative": lambda lib, t: lib.gdv_filter_make_from_proto(b"", 0, b"", -1, None, C.byref(C.c_void_p())),
    "filter_project_make_from_proto/negative": lambda lib, t: lib.gdv_filter_project_make_from_proto(b"", 0, b"", 0, b"", -1, 2, None, C.byref(C.c_void_p())),
    "filter_project_make_from_proto/mode4": lambda lib, t: lib.gdv_filter_project_make_from_proto(b"", 0, b"", 0, b"", 0, 4, None, C.byref(C.c_void_p())),
    "projector_make_from_proto/truncated": lambda lib, t: lib.gdv_projector_make_from_proto(P.schema(t.schema), len(P.schema(t.schema)), _truncated(t), len(_truncated(t)), 0, None, C.byref(C.c_void_p())),
    "projector_make_from_proto/truncated_schema": lambda lib, t: lib.gdv_projector_make_from_proto(P.schema(t.schema)[:-2], len(P.schema(t.schema)) - 2, b"", 0, 0, None, C.byref(C.c_void_p())),
    "filter_make_from_proto/truncated": lambda lib, t: lib.gdv_filter_make_from_proto(P.schema(t.schema), len(P.schema(t.schema)), P.condition(t.cond)[:-3], len(P.condition(t.cond)) - 3, None, C.byref(C.c_void_p())),
    "filter_project_make_from_proto/truncated": lambda lib, t: lib.gdv_filter_project_make_from_proto(P.schema(t.schema), len(P.schema(t.schema)), P.condition(t.cond), len(P.condition(t.cond)), _truncated(t), len(_truncated(t)), 2, None, C.byref(C.c_void_p())),
    "projector_make_from_proto/mode4": lambda lib, t: lib.gdv_projector_make_from_proto(P.schema(t.schema), len(P.schema(t.schema)), P.expression_list(t.exprs), len(P.expression_list(t.exprs)), 4, None, C.byref(C.c_void_p())),
    "proto_describe/null_message": lambda lib, t: lib.gdv_proto_describe(None, 4, b"", 0, 0),
    "proto_describe/truncated": lambda lib, t: lib.gdv_proto_describe(P.schema(t.schema), len(P.schema(t.schema)), _truncated(t), len(_truncated(t)), 0),
    "proto_describe/truncated_condition": lambda lib, t: lib.gdv_proto_describe(P.schema(t.schema), len(P.schema(t.schema)), P.condition(t.cond)[:-3], len(P.condition(t.cond)) - 3, 1),
    # build support
    "tier0_program/null_schema": lambda lib, t: lib.gdv_tier0_program(None, t.handles(t.fixed), 1, 0),
    "tier0_program/null_expr": lambda lib, t: lib.gdv_tier0_program(t.sh, (C.c_void_p * 1)(None), 1, 0),
    "tier0_program_selection/null_expr": lambda lib, t: lib.gdv_tier0_program_selection(t.sh, (C.c_void_p * 1)(None), 1, 2),
    "tier0_program_selection/mode4": lambda lib, t: lib.gdv_tier0_program_selection(t.sh, t.handles(t.fixed), 1, 4),
    "precompile_projector/null_schema": lambda lib, t: lib.gdv_precompile_projector(None, t.handles(t.fixed), 1, 0),
    "precompile_projector/null_expr": lambda lib, t: lib.gdv_precompile_projector(t.sh, (C.c_void_p * 1)(None), 1, 0),
    "precompile_projector/mode4": lambda lib, t: lib.gdv_precompile_projector(t.sh, t.handles(t.fixed), 1, 4),
    "precompile_filter/null": lambda lib, t: lib.gdv_precompile_filter(t.sh, None),
    "precompile_filter_project/null": lambda lib, t: lib.gdv_precompile_filter_project(t.sh, None, t.handles(t.fixed), 1, 2),
    "precompile_filter_project/null_expr": lambda lib, t: lib.gdv_precompile_filter_project(t.sh, t.cond._h, (C.c_void_p * 1)(None), 1, 2),
    "precompile_filter_project/mode-1": lambda lib, t: lib.gdv_precompile_filter_project(t.sh, t.cond._h, t.handles(t.fixed), 1, -1),
    "compile_date_format/cap": lambda lib, t: lib.gdv_compile_date_format(b"YYYY-MM-DD", 10, (C.c_uint8 * 1)(), 1, C.byref(I64)),
    "compile_date_format/null": lambda lib, t: lib.gdv_compile_date_format(None, 0, (C.c_uint8 * 1)(), 1, C.byref(I64)),
    # device unit
    "device_hbm_ceilings/small": lambda lib, t: lib.gdv_device_hbm_ceilings((1 << 20) - 1, C.byref(C.c_double()), C.byref(C.c_double()), C.byref(C.c_double())),
    "device_stream_ceiling/11_reads": lambda lib, t: lib.gdv_device_stream_ceiling(1 << 20, 11, 0, C.byref(C.c_double()), None, None),
    "device_stream_ceiling_on/null_streams": lambda lib, t: lib.gdv_device_stream_ceiling_on(None, 1, 1, 4096, C.byref(C.c_double()), None, None),
    "device_alloc/null": lambda lib, t: lib.gdv_device_alloc(16, None),
    "device_pool_alloc/null_pool": lambda lib, t: lib.gdv_device_pool_alloc(None, 16, C.byref(C.c_void_p())),
    "set_virtual_devices/negative": lambda lib, t: lib.gdv_set_virtual_devices(-1),
    "shard_bounds/bad": lambda lib, t: lib.gdv_shard_bounds(10, 2, 2, C.byref(I64), C.byref(I64)),
    # tuning
    "filter_set_tuning/null_key": lambda lib, t: lib.gdv_filter_set_tuning(None, None, 1),
    "filter_project_set_tuning/null_key": lambda lib, t: lib.gdv_filter_project_set_tuning(None, None, 1),
}

CPU_EXPECTED = {
    'compile_date_format/cap': (4, 'Invalid: ops buffer too small'),
    'compile_date_format/null': (4, 'Invalid: null argument'),
    'device_alloc/null': (4, 'Invalid: bad argument'),
    'device_hbm_ceilings/small': (4, 'Invalid: bad argument'),
    'device_pool_alloc/null_pool': (4, 'Invalid: null pool'),
    'device_stream_ceiling/11_reads': (4, 'Invalid: bad argument'),
    'device_stream_ceiling_on/null_streams': (4, 'Invalid: bad argument'),
    'filter_evaluate/null': (4, 'Invalid: null filter'),
    'filter_evaluate_async/null': (4, 'Invalid: null filter'),
    'filter_evaluate_device_array/null': (4, 'Invalid: null filter'),
    'filter_evaluate_flat/null': (4, 'Invalid: null filter'),
    'filter_evaluate_host_sharded/null': (4, 'Invalid: null filter'),
    'filter_evaluate_many/null': (4, 'Invalid: null filter'),
    'filter_evaluate_sharded/null': (4, 'Invalid: null filter'),
    'filter_gather_sharded/mode-1': (4, 'Invalid: bad selection mode'),
    'filter_gather_sharded/mode4': (4, 'Invalid: bad selection mode'),
    'filter_gather_sharded/mode_none': (4, 'Invalid: bad selection mode'),
    'filter_gather_sharded/no_shards': (4, 'Invalid: bad shard list'),
    'filter_gather_sharded/too_many': (4, 'Invalid: gathered selection vector needs 11 slots'),
    'filter_make/null_condition': (4, 'Invalid: Condition cannot be null'),
    'filter_make_from_proto/negative': (4, 'Invalid: bad argument'),
    'filter_make_from_proto/truncated': (4, 'Invalid: malformed protobuf message: TreeNode'),
    'filter_project_evaluate/null': (4, 'Invalid: null filter-project'),
    'filter_project_make/mode4': (4, 'Invalid: bad selection mode'),
    'filter_project_make/no_exprs': (4, 'Invalid: Expressions cannot be empty'),
    'filter_project_make/null_expr': (4, 'Invalid: Expression cannot be null'),
    'filter_project_make_from_proto/mode4': (4, 'Invalid: bad selection mode'),
    'filter_project_make_from_proto/negative': (4, 'Invalid: bad argument'),
    'filter_project_make_from_proto/truncated': (4, 'Invalid: malformed protobuf message: ExpressionRoot'),
    'filter_project_set_tuning/null_key': (4, 'Invalid: gdv_filter_project_set_tuning: null argument'),
    'filter_set_tuning/null_key': (4, 'Invalid: gdv_filter_set_tuning: null argument'),
    'precompile_filter/null': (4, 'Invalid: null argument'),
    'precompile_filter_project/mode-1': (4, 'Invalid: bad selection mode'),
    'precompile_filter_project/null': (4, 'Invalid: null argument'),
    'precompile_filter_project/null_expr': (4, 'Invalid: Expression cannot be null'),
    'precompile_projector/mode4': (4, 'Invalid: bad selection mode'),
    'precompile_projector/null_expr': (4, 'Invalid: null expression'),
    'precompile_projector/null_schema': (4, 'Invalid: null schema'),
    'projector_evaluate/null': (4, 'Invalid: null projector'),
    'projector_evaluate_async/null': (4, 'Invalid: null projector'),
    'projector_evaluate_device_array/null': (4, 'Invalid: null projector'),
    'projector_evaluate_export/null': (4, 'Invalid: null projector'),
    'projector_evaluate_flat/null': (4, 'Invalid: null projector'),
    'projector_evaluate_host_sharded/null': (4, 'Invalid: null projector'),
    'projector_evaluate_many/null': (4, 'Invalid: null projector'),
    'projector_evaluate_selected/no_count': (4, 'Invalid: selection vector and device slot count are required'),
    'projector_evaluate_selected/no_sel': (4, 'Invalid: selection vector and device slot count are required'),
    'projector_evaluate_selected/null': (4, 'Invalid: null projector'),
    'projector_evaluate_sharded/null': (4, 'Invalid: null projector'),
    'projector_make/mode-1': (4, 'Invalid: bad selection mode'),
    'projector_make/mode4': (4, 'Invalid: bad selection mode'),
    'projector_make/null_expr': (4, 'Invalid: null expression'),
    'projector_make/null_schema': (4, 'Invalid: null schema or output pointer'),
    'projector_make_from_proto/mode4': (4, 'Invalid: bad selection mode'),
    'projector_make_from_proto/negative': (4, 'Invalid: bad argument'),
    'projector_make_from_proto/truncated': (4, 'Invalid: malformed protobuf message: ExpressionRoot'),
    'projector_make_from_proto/truncated_schema': (4, 'Invalid: malformed protobuf message: Field'),
    'proto_describe/null_message': ('NULL', 'Invalid: gdv_proto_describe: negative length or null message'),
    'proto_describe/truncated': ('NULL', 'Invalid: malformed protobuf message: ExpressionRoot'),
    'proto_describe/truncated_condition': ('NULL', 'Invalid: malformed protobuf message: TreeNode'),
    'set_virtual_devices/negative': (4, 'Invalid: bad virtual device count'),
    'shard_bounds/bad': (4, 'Invalid: bad shard arguments'),
    'tier0_program/null_expr': ('NULL', 'Invalid: null expression'),
    'tier0_program/null_schema': ('NULL', 'Invalid: schema and expressions are required'),
    'tier0_program_selection/mode4': ('NULL', 'Invalid: selection mode must be 0 (none), 1 (uint16), 2 (uint32) or 3 (uint64)'),
    'tier0_program_selection/null_expr': ('NULL', 'Invalid: null expression'),
}


@pytest.mark.parametrize("case", sorted(CPU_CASES))
def test_refusal_without_a_device(trees, case):
    assert _outcome(CPU_CASES[case](_capi.lib(), trees)) == CPU_EXPECTED[case]


def test_last_error_is_per_thread_across_units():
    """Thread A fails in the eval unit, thread B in the device unit; after both have failed each reads its own text."""
    lib = _capi.lib()
    both_failed = threading.Barrier(2)
    seen = {}

    def run(name, call):
        rc = call()
        both_failed.wait(timeout=30)
        seen[name] = (rc, lib.gdv_last_error().decode())

    a = threading.Thread(target=run, args=("a", lambda: CPU_CASES["projector_evaluate/null"](lib, None)))
    b = threading.Thread(target=run, args=("b", lambda: CPU_CASES["device_hbm_ceilings/small"](lib, None)))
    a.start()
    b.start()
    a.join()
    b.join()
    assert seen["a"] == CPU_EXPECTED["projector_evaluate/null"]
    assert seen["b"] == CPU_EXPECTED["device_hbm_ceilings/small"]


# ------------------------------------------------------------------ behind a live handle (no launch all the same)

class _Operators:
    def __init__(self, t):
        self.proj = gandiva.make_projector(t.schema, t.exprs, None)           # x + x, upper(s)
        self.fixed = gandiva.make_projector(t.schema, t.fixed, None)
        self.selected = gandiva.make_projector(t.schema, t.fixed, None, "UINT32")
        self.flt = gandiva.make_filter(t.schema, t.cond)
        self.fp = gandiva.make_filter_project(t.schema, t.cond, t.fixed, None)
        self.keep = []

    def host_batch(self, n_children=2, offset=0, device_type=1, release=1):
        """an ArrowDeviceArray of 8 rows over host memory (x int32, s string), or a broken one"""
        x = np.arange(8, dtype=np.int32)
        offs = np.arange(9, dtype=np.int32)
        data = np.frombuffer(b"abcdefgh", dtype=np.uint8).copy()
        bx = (C.c_void_p * 2)(None, x.ctypes.data)
        bs = (C.c_void_p * 3)(None, offs.ctypes.data, data.ctypes.data)
        cx = ArrowArray(8, 0, 0, 2, 0, bx, None, None, C.c_void_p(1), None)
        cs = ArrowArray(8, 0, 0, 3, 0, bs, None, None, C.c_void_p(1), None)
        children = (C.POINTER(ArrowArray) * 2)(C.pointer(cx), C.pointer(cs))
        top = (C.c_void_p * 1)(None)
        dev = ArrowDeviceArray()
        dev.array = ArrowArray(8, 0, offset, 1, n_children, top, children, None, C.c_void_p(release) if release else None, None)
        dev.device_id, dev.device_type, dev.sync_event = -1, device_type, None
        self.keep += [x, offs, data, bx, bs, cx, cs, children, top, dev]
        return C.addressof(dev)


@pytest.fixture(scope="module")
def ops(trees):
    return _Operators(trees)


def _many(cols, outs):
    return (gdv_batch_t * 1)(gdv_batch_t(8, cols, 1, outs, 1))


GPU_CASES = {
    # null column array behind num_cols > 0
    "projector_evaluate/null_cols": lambda lib, o: lib.gdv_projector_evaluate(o.proj._h, 8, None, 2, None, ONE_OUT, 1, 0, None, 0),
    "projector_evaluate_async/null_cols": lambda lib, o: lib.gdv_projector_evaluate_async(o.fixed._h, 8, None, 2, None, None, ONE_OUT, 1, None, SOME),
    "projector_evaluate_host_sharded/null_cols": lambda lib, o: lib.gdv_projector_evaluate_host_sharded(o.fixed._h, 8, None, 2, ONE_OUT, 1, ONE_DEV, 1),
    "projector_evaluate_many/null_cols": lambda lib, o: lib.gdv_projector_evaluate_many(o.fixed._h, _many(None, ONE_OUT), 1, None, 0),
    "filter_evaluate/null_cols": lambda lib, o: lib.gdv_filter_evaluate(o.flt._h, 8, None, 2, 2, SOME, 8, C.byref(I64), 0, None),
    "filter_evaluate_async/null_cols": lambda lib, o: lib.gdv_filter_evaluate_async(o.flt._h, 8, None, 2, 2, SOME, 8, SOME, None),
    "filter_evaluate_host_sharded/null_cols": lambda lib, o: lib.gdv_filter_evaluate_host_sharded(o.flt._h, 8, None, 2, 2, SOME, 8, C.byref(I64), ONE_DEV, 1),
    "filter_project_evaluate/null_cols": lambda lib, o: lib.gdv_filter_project_evaluate(o.fp._h, 8, None, 2, ONE_OUT, 1, SOME, 8, C.byref(I64), None, 0, None, 0),
    # null outputs
    "projector_evaluate/null_outs": lambda lib, o: lib.gdv_projector_evaluate(o.proj._h, 8, ONE_COL, 1, None, None, 1, 0, None, 0),
    "projector_evaluate_selected/null_outs": lambda lib, o: lib.gdv_projector_evaluate_selected(o.selected._h, 8, ONE_COL, 1, _sel(2), SOME, None, 1, None, 0),
    "projector_evaluate_async/null_outs": lambda lib, o: lib.gdv_projector_evaluate_async(o.fixed._h, 8, ONE_COL, 1, None, None, None, 1, None, SOME),
    "projector_evaluate_async/null_result": lambda lib, o: lib.gdv_projector_evaluate_async(o.fixed._h, 8, ONE_COL, 1, None, None, ONE_OUT, 1, None, None),
    "projector_evaluate_device_array/null_outs": lambda lib, o: lib.gdv_projector_evaluate_device_array(o.proj._h, o.host_batch(), None, None, 1, None, 0),
    "projector_evaluate_export/null_out": lambda lib, o: lib.gdv_projector_evaluate_export(o.proj._h, o.host_batch(), None, None, None, None),
    "projector_evaluate_host_sharded/null_outs": lambda lib, o: lib.gdv_projector_evaluate_host_sharded(o.fixed._h, 8, ONE_COL, 1, None, 1, ONE_DEV, 1),
    "projector_evaluate_host_sharded/no_devices": lambda lib, o: lib.gdv_projector_evaluate_host_sharded(o.fixed._h, 8, ONE_COL, 1, ONE_OUT, 1, ONE_DEV, 0),
    "filter_evaluate_async/null_count": lambda lib, o: lib.gdv_filter_evaluate_async(o.flt._h, 8, ONE_COL, 1, 2, SOME, 8, None, None),
    "filter_evaluate_host_sharded/null_indices": lambda lib, o: lib.gdv_filter_evaluate_host_sharded(o.flt._h, 8, ONE_COL, 1, 2, None, 8, C.byref(I64), ONE_DEV, 1),
    # selection modes
    "projector_evaluate/sel-1": lambda lib, o: lib.gdv_projector_evaluate(o.selected._h, 8, ONE_COL, 1, _sel(-1), ONE_OUT, 1, 0, None, 0),
    "projector_evaluate/sel4": lambda lib, o: lib.gdv_projector_evaluate(o.selected._h, 8, ONE_COL, 1, _sel(4), ONE_OUT, 1, 0, None, 0),
    "projector_evaluate_selected/sel-1": lambda lib, o: lib.gdv_projector_evaluate_selected(o.selected._h, 8, ONE_COL, 1, _sel(-1), SOME, ONE_OUT, 1, None, 0),
    "projector_evaluate_selected/sel4": lambda lib, o: lib.gdv_projector_evaluate_selected(o.selected._h, 8, ONE_COL, 1, _sel(4), SOME, ONE_OUT, 1, None, 0),
    "projector_evaluate_async/sel-1": lambda lib, o: lib.gdv_projector_evaluate_async(o.selected._h, 8, ONE_COL, 1, _sel(-1), SOME, ONE_OUT, 1, None, SOME),
    "projector_evaluate_async/sel4": lambda lib, o: lib.gdv_projector_evaluate_async(o.selected._h, 8, ONE_COL, 1, _sel(4), SOME, ONE_OUT, 1, None, SOME),
    "projector_evaluate_flat/sel-1": lambda lib, o: lib.gdv_projector_evaluate_flat(o.fixed._h, 8, (C.c_int64 * 5)(), (C.c_int64 * 5)(), 5, -1, 0, 0, (C.c_int64 * 2)(), (C.c_int64 * 2)(), 2, 0),
    "projector_evaluate_flat/sel4": lambda lib, o: lib.gdv_projector_evaluate_flat(o.fixed._h, 8, (C.c_int64 * 5)(), (C.c_int64 * 5)(), 5, 4, 0, 0, (C.c_int64 * 2)(), (C.c_int64 * 2)(), 2, 0),
    "projector_evaluate_device_array/sel-1": lambda lib, o: lib.gdv_projector_evaluate_device_array(o.proj._h, o.host_batch(), _sel(-1), (gdv_out_column_t * 2)(), 2, None, 0),
    "projector_evaluate_device_array/sel4": lambda lib, o: lib.gdv_projector_evaluate_device_array(o.proj._h, o.host_batch(), _sel(4), (gdv_out_column_t * 2)(), 2, None, 0),
    "projector_evaluate_export/sel-1": lambda lib, o: lib.gdv_projector_evaluate_export(o.proj._h, o.host_batch(), _sel(-1), None, C.byref(ArrowDeviceArray()), None),
    "projector_evaluate_export/sel4": lambda lib, o: lib.gdv_projector_evaluate_export(o.proj._h, o.host_batch(), _sel(4), None, C.byref(ArrowDeviceArray()), None),
    "filter_evaluate/mode-1": lambda lib, o: lib.gdv_filter_evaluate(o.flt._h, 8, ONE_COL, 1, -1, SOME, 8, C.byref(I64), 0, None),
    "filter_evaluate/mode4": lambda lib, o: lib.gdv_filter_evaluate(o.flt._h, 8, ONE_COL, 1, 4, SOME, 8, C.byref(I64), 0, None),
    "filter_evaluate_async/mode-1": lambda lib, o: lib.gdv_filter_evaluate_async(o.flt._h, 8, ONE_COL, 1, -1, SOME, 8, SOME, None),
    "filter_evaluate_async/mode4": lambda lib, o: lib.gdv_filter_evaluate_async(o.flt._h, 8, ONE_COL, 1, 4, SOME, 8, SOME, None),
    "filter_evaluate_many/mode-1": lambda lib, o: lib.gdv_filter_evaluate_many(o.flt._h, (gdv_filter_batch_t * 1)(), 1, -1, C.byref(I64), None, None, 0),
    "filter_evaluate_many/mode4": lambda lib, o: lib.gdv_filter_evaluate_many(o.flt._h, (gdv_filter_batch_t * 1)(), 1, 4, C.byref(I64), None, None, 0),
    "filter_evaluate_flat/mode-1": lambda lib, o: lib.gdv_filter_evaluate_flat(o.flt._h, 8, None, None, 0, -1, 0, 0, C.byref(I64), 0),
    "filter_evaluate_flat/mode4": lambda lib, o: lib.gdv_filter_evaluate_flat(o.flt._h, 8, None, None, 0, 4, 0, 0, C.byref(I64), 0),
    "filter_evaluate_flat/mode_none": lambda lib, o: lib.gdv_filter_evaluate_flat(o.flt._h, 8, None, None, 0, 0, 0, 0, C.byref(I64), 0),
    "filter_evaluate_device_array/mode-1": lambda lib, o: lib.gdv_filter_evaluate_device_array(o.flt._h, o.host_batch(), -1, SOME, 8, C.byref(I64), None),
    "filter_evaluate_device_array/mode4": lambda lib, o: lib.gdv_filter_evaluate_device_array(o.flt._h, o.host_batch(), 4, SOME, 8, C.byref(I64), None),
    "filter_evaluate_sharded/mode-1": lambda lib, o: lib.gdv_filter_evaluate_sharded(o.flt._h, 8, 1, -1, ONE_SHARD, 1, 0, None),
    "filter_evaluate_sharded/mode4": lambda lib, o: lib.gdv_filter_evaluate_sharded(o.flt._h, 8, 1, 4, ONE_SHARD, 1, 0, None),
    "filter_evaluate_sharded/mode_none": lambda lib, o: lib.gdv_filter_evaluate_sharded(o.flt._h, 8, 1, 0, ONE_SHARD, 1, 0, None),
    "filter_evaluate_host_sharded/mode-1": lambda lib, o: lib.gdv_filter_evaluate_host_sharded(o.flt._h, 8, ONE_COL, 1, -1, SOME, 8, C.byref(I64), ONE_DEV, 1),
    "filter_evaluate_host_sharded/mode4": lambda lib, o: lib.gdv_filter_evaluate_host_sharded(o.flt._h, 8, ONE_COL, 1, 4, SOME, 8, C.byref(I64), ONE_DEV, 1),
    "filter_evaluate_host_sharded/mode_none": lambda lib, o: lib.gdv_filter_evaluate_host_sharded(o.flt._h, 8, ONE_COL, 1, 0, SOME, 8, C.byref(I64), ONE_DEV, 1),
    # batch lists
    "projector_evaluate_many/negative": lambda lib, o: lib.gdv_projector_evaluate_many(o.fixed._h, None, -1, None, 0),
    "projector_evaluate_many/null_list": lambda lib, o: lib.gdv_projector_evaluate_many(o.fixed._h, None, 2, None, 0),
    "filter_evaluate_many/negative": lambda lib, o: lib.gdv_filter_evaluate_many(o.flt._h, None, -1, 2, C.byref(I64), None, None, 0),
    "filter_evaluate_many/null_list": lambda lib, o: lib.gdv_filter_evaluate_many(o.flt._h, None, 2, 2, C.byref(I64), None, None, 0),
    # flat calls: both numbers are in the message
    "projector_evaluate_flat/input_count": lambda lib, o: lib.gdv_projector_evaluate_flat(o.proj._h, 8, (C.c_int64 * 4)(), (C.c_int64 * 4)(), 4, 0, 0, 0, (C.c_int64 * 5)(), (C.c_int64 * 5)(), 5, 0),
    "projector_evaluate_flat/output_count": lambda lib, o: lib.gdv_projector_evaluate_flat(o.proj._h, 8, (C.c_int64 * 5)(), (C.c_int64 * 5)(), 5, 0, 0, 0, (C.c_int64 * 4)(), (C.c_int64 * 4)(), 4, 0),
    "filter_evaluate_flat/input_count": lambda lib, o: lib.gdv_filter_evaluate_flat(o.flt._h, 8, (C.c_int64 * 6)(), (C.c_int64 * 6)(), 6, 2, 0, 0, C.byref(I64), 0),
    # sharded calls
    "projector_evaluate_sharded/selection_mode": lambda lib, o: lib.gdv_projector_evaluate_sharded(o.selected._h, 8, 1, 1, ONE_SHARD, 1, 0),
    "projector_evaluate_sharded/no_shards": lambda lib, o: lib.gdv_projector_evaluate_sharded(o.fixed._h, 8, 1, 1, ONE_SHARD, 0, 0),
    "projector_evaluate_sharded/shard_without_outs": lambda lib, o: lib.gdv_projector_evaluate_sharded(o.fixed._h, 8, 0, 1, ONE_SHARD, 1, 0),
    "filter_evaluate_sharded/shard_without_indices": lambda lib, o: lib.gdv_filter_evaluate_sharded(o.flt._h, 8, 0, 2, ONE_SHARD, 1, 0, None),
    "projector_evaluate_host_sharded/selection_mode": lambda lib, o: lib.gdv_projector_evaluate_host_sharded(o.selected._h, 8, ONE_COL, 1, ONE_OUT, 1, ONE_DEV, 1),
    "projector_evaluate_host_sharded/num_outs": lambda lib, o: lib.gdv_projector_evaluate_host_sharded(o.proj._h, 8, ONE_COL, 1, ONE_OUT, 1, ONE_DEV, 1),
    "filter_evaluate_host_sharded/max_slots": lambda lib, o: lib.gdv_filter_evaluate_host_sharded(o.flt._h, 8, ONE_COL, 1, 2, SOME, 7, C.byref(I64), ONE_DEV, 1),
    # device-array import
    "projector_evaluate_device_array/null_batch": lambda lib, o: lib.gdv_projector_evaluate_device_array(o.proj._h, None, None, (gdv_out_column_t * 2)(), 2, None, 0),
    "projector_evaluate_device_array/released": lambda lib, o: lib.gdv_projector_evaluate_device_array(o.proj._h, o.host_batch(release=0), None, (gdv_out_column_t * 2)(), 2, None, 0),
    "projector_evaluate_device_array/children": lambda lib, o: lib.gdv_projector_evaluate_device_array(o.proj._h, o.host_batch(n_children=1), None, (gdv_out_column_t * 2)(), 2, None, 0),
    "projector_evaluate_device_array/struct_offset": lambda lib, o: lib.gdv_projector_evaluate_device_array(o.proj._h, o.host_batch(offset=1), None, (gdv_out_column_t * 2)(), 2, None, 0),
    "projector_evaluate_device_array/device_type": lambda lib, o: lib.gdv_projector_evaluate_device_array(o.proj._h, o.host_batch(device_type=7), None, (gdv_out_column_t * 2)(), 2, None, 0),
    "filter_evaluate_device_array/null_batch": lambda lib, o: lib.gdv_filter_evaluate_device_array(o.flt._h, None, 2, SOME, 8, C.byref(I64), None),
    "filter_evaluate_device_array/children": lambda lib, o: lib.gdv_filter_evaluate_device_array(o.flt._h, o.host_batch(n_children=3), 2, SOME, 8, C.byref(I64), None),
    "projector_evaluate_export/released": lambda lib, o: lib.gdv_projector_evaluate_export(o.proj._h, o.host_batch(release=0), None, None, C.byref(ArrowDeviceArray()), None),
    "projector_evaluate_export/device_type": lambda lib, o: lib.gdv_projector_evaluate_export(o.proj._h, o.host_batch(device_type=7), None, None, C.byref(ArrowDeviceArray()), None),
    # tuning
    "filter_set_tuning/null_key": lambda lib, o: lib.gdv_filter_set_tuning(o.flt._h, None, 1),
    "filter_project_set_tuning/null_key": lambda lib, o: lib.gdv_filter_project_set_tuning(o.fp._h, None, 1),
    "projector_output_sizes/bad_index": lambda lib, o: lib.gdv_projector_output_sizes(o.proj._h, 2, 8, 0, None, None),
}

GPU_EXPECTED = {
    'filter_evaluate/mode-1': (4, 'Invalid: bad selection mode'),
    'filter_evaluate/mode4': (4, 'Invalid: bad selection mode'),
    'filter_evaluate/null_cols': (4, 'Invalid: null column array'),
    'filter_evaluate_async/mode-1': (4, 'Invalid: bad selection mode'),
    'filter_evaluate_async/mode4': (4, 'Invalid: bad selection mode'),
    'filter_evaluate_async/null_cols': (4, 'Invalid: null column array'),
    'filter_evaluate_async/null_count': (4, 'Invalid: null count pointer'),
    'filter_evaluate_device_array/children': (4, 'Invalid: ArrowDeviceArray has 3 children, the schema has 2 fields'),
    'filter_evaluate_device_array/mode-1': (4, 'Invalid: bad selection mode'),
    'filter_evaluate_device_array/mode4': (4, 'Invalid: bad selection mode'),
    'filter_evaluate_device_array/null_batch': (4, 'Invalid: null ArrowDeviceArray'),
    'filter_evaluate_flat/input_count': (4, 'Invalid: expected 5 input buffers (validity, [offsets,] data per field), got 6'),
    'filter_evaluate_flat/mode-1': (4, 'Invalid: bad selection mode'),
    'filter_evaluate_flat/mode4': (4, 'Invalid: bad selection mode'),
    'filter_evaluate_flat/mode_none': (4, 'Invalid: bad selection mode'),
    'filter_evaluate_host_sharded/max_slots': (4, 'Invalid: Selection vector too small: max slots 7 < rows 8'),
    'filter_evaluate_host_sharded/mode-1': (4, 'Invalid: bad selection mode'),
    'filter_evaluate_host_sharded/mode4': (4, 'Invalid: bad selection mode'),
    'filter_evaluate_host_sharded/mode_none': (4, 'Invalid: bad selection mode'),
    'filter_evaluate_host_sharded/null_cols': (4, 'Invalid: null column array'),
    'filter_evaluate_host_sharded/null_indices': (4, 'Invalid: Selection vector cannot be null'),
    'filter_evaluate_many/mode-1': (4, 'Invalid: bad selection mode'),
    'filter_evaluate_many/mode4': (4, 'Invalid: bad selection mode'),
    'filter_evaluate_many/negative': (4, 'Invalid: null batch list'),
    'filter_evaluate_many/null_list': (4, 'Invalid: null batch list'),
    'filter_evaluate_sharded/mode-1': (4, 'Invalid: bad selection mode'),
    'filter_evaluate_sharded/mode4': (4, 'Invalid: bad selection mode'),
    'filter_evaluate_sharded/mode_none': (4, 'Invalid: bad selection mode'),
    'filter_evaluate_sharded/shard_without_indices': (4, 'Invalid: shard without columns / indices'),
    'filter_project_evaluate/null_cols': (4, 'Invalid: null column array'),
    'filter_project_set_tuning/null_key': (4, 'Invalid: gdv_filter_project_set_tuning: null argument'),
    'filter_set_tuning/null_key': (4, 'Invalid: gdv_filter_set_tuning: null argument'),
    'projector_evaluate/null_cols': (4, 'Invalid: null column array'),
    'projector_evaluate/null_outs': (4, 'Invalid: Output array vector cannot be null'),
    'projector_evaluate/sel-1': (4, 'Invalid: bad selection mode'),
    'projector_evaluate/sel4': (4, 'Invalid: bad selection mode'),
    'projector_evaluate_async/null_cols': (4, 'Invalid: null column array'),
    'projector_evaluate_async/null_outs': (4, 'Invalid: Output array vector and result block cannot be null'),
    'projector_evaluate_async/null_result': (4, 'Invalid: Output array vector and result block cannot be null'),
    'projector_evaluate_async/sel-1': (4, 'Invalid: bad selection mode'),
    'projector_evaluate_async/sel4': (4, 'Invalid: bad selection mode'),
    'projector_evaluate_device_array/children': (4, 'Invalid: ArrowDeviceArray has 1 children, the schema has 2 fields'),
    'projector_evaluate_device_array/device_type': (4, 'Invalid: unsupported ArrowDeviceType 7'),
    'projector_evaluate_device_array/null_batch': (4, 'Invalid: null ArrowDeviceArray'),
    'projector_evaluate_device_array/null_outs': (4, 'Invalid: Output array vector cannot be null'),
    'projector_evaluate_device_array/released': (4, 'Invalid: ArrowDeviceArray was already released'),
    'projector_evaluate_device_array/sel-1': (4, 'Invalid: bad selection mode'),
    'projector_evaluate_device_array/sel4': (4, 'Invalid: bad selection mode'),
    'projector_evaluate_device_array/struct_offset': (4, 'Invalid: struct-level offset is not supported'),
    'projector_evaluate_export/device_type': (4, 'Invalid: unsupported ArrowDeviceType 7'),
    'projector_evaluate_export/null_out': (4, 'Invalid: null output ArrowDeviceArray'),
    'projector_evaluate_export/released': (4, 'Invalid: ArrowDeviceArray was already released'),
    'projector_evaluate_export/sel-1': (4, 'Invalid: bad selection mode'),
    'projector_evaluate_export/sel4': (4, 'Invalid: bad selection mode'),
    'projector_evaluate_flat/input_count': (4, 'Invalid: expected 5 input buffers (validity, [offsets,] data per field), got 4'),
    'projector_evaluate_flat/output_count': (4, 'Invalid: expected 5 output buffers, got 4'),
    'projector_evaluate_flat/sel-1': (4, 'Invalid: bad selection mode'),
    'projector_evaluate_flat/sel4': (4, 'Invalid: bad selection mode'),
    'projector_evaluate_host_sharded/no_devices': (4, 'Invalid: outputs and a device list are required'),
    'projector_evaluate_host_sharded/null_cols': (4, 'Invalid: null column array'),
    'projector_evaluate_host_sharded/null_outs': (4, 'Invalid: outputs and a device list are required'),
    'projector_evaluate_host_sharded/num_outs': (4, 'Invalid: number of outputs does not match the projector'),
    'projector_evaluate_host_sharded/selection_mode': (4, 'Invalid: sharded evaluation takes row-mode projectors'),
    'projector_evaluate_many/negative': (4, 'Invalid: null batch list'),
    'projector_evaluate_many/null_cols': (4, 'Invalid: null column array'),
    'projector_evaluate_many/null_list': (4, 'Invalid: null batch list'),
    'projector_evaluate_selected/null_outs': (4, 'Invalid: Output array vector cannot be null'),
    'projector_evaluate_selected/sel-1': (4, 'Invalid: bad selection mode'),
    'projector_evaluate_selected/sel4': (4, 'Invalid: bad selection mode'),
    'projector_evaluate_sharded/no_shards': (4, 'Invalid: bad shard list'),
    'projector_evaluate_sharded/selection_mode': (4, 'Invalid: sharded evaluation takes row-mode projectors'),
    'projector_evaluate_sharded/shard_without_outs': (4, 'Invalid: shard without columns / outputs'),
    'projector_output_sizes/bad_index': (4, 'Invalid: bad argument'),
}


@pytest.mark.gpu
def test_refusals_behind_a_live_handle(ops):
    """One test for the whole table (one set of operators, no launch): every case is compared, then all misses are shown."""
    lib = _capi.lib()
    got = {case: _outcome(GPU_CASES[case](lib, ops)) for case in sorted(GPU_CASES)}
    assert got == GPU_EXPECTED
