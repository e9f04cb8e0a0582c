"""gdv_filter_project_evaluate_many, the parts that need no device: the entry point is in the library and in the
ctypes binding; the fused plan has a third kernel text, the SMALL shape (one workgroup per batch: the windowed body
without look-back, ticket or granules), which compiles for gfx950; asking for it leaves the windowed and the direct
kernel's text — and so their names and disk-cache keys — byte for byte what they were; a plan that has the direct shape
only has no small shape.
"""
import ctypes as C
import re

import numpy as np
import pyarrow as pa
import pytest

import gandiva_amd as gandiva
from gandiva_amd import _capi, gandiva as gg
from test_filter_project import _batch, _plan

I64 = pa.int64()
MAIN, DIRECT, SMALL = 0, 1, 2


class _Planned:
    """schema + condition + expressions held as C handles for gdv_filter_project_plan_text"""

    def __init__(self, schema, cond, exprs):
        self.lib = _capi.lib()
        self.cond, self.exprs = cond, exprs
        self.sh = gg._make_schema(schema)
        self.arr = (C.c_void_p * len(exprs))(*[e._h for e in exprs])

    def text(self, mode, shape, request_small=1, compile=0):
        p = self.lib.gdv_filter_project_plan_text(self.sh, self.cond._h, self.arr, len(self.exprs), mode, shape,
                                                  request_small, compile)
        return _capi.take_string(p) if p else None

    def close(self):
        self.lib.gdv_schema_free(self.sh)


@pytest.fixture(scope="module")
def threshold_plan():
    batch = _batch(np.random.default_rng(0), 100, 0.1)
    cond, exprs = _plan(batch.schema, 500)
    p = _Planned(batch.schema, cond, exprs)
    yield p
    p.close()


def test_the_entry_point_is_in_the_library_and_in_the_binding():
    lib = _capi.lib()
    names = [p[0] for p in _capi.PROTOTYPES]
    for name in ("gdv_filter_project_evaluate_many", "gdv_filter_project_small_batch_rows", "gdv_filter_project_plan_text"):
        assert name in names
        assert getattr(lib, name) is not None
    fields = [f[0] for f in _capi.gdv_filter_project_batch_t._fields_]
    assert fields == ["num_rows", "cols", "num_cols", "outs", "num_outs", "out_indices", "max_slots"]
    assert C.sizeof(_capi.gdv_filter_project_batch_t) == 56
    assert hasattr(gandiva.gandiva.FilterProject, "evaluate_device_many")


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_the_small_plan_is_generated_and_compiles_for_gfx950(threshold_plan, mode):
    text = threshold_plan.text(mode, SMALL, compile=1)
    assert text is not None, _capi.last_error()
    name = re.search(r"(gdv_k_[0-9a-f]{16})_small\(const gdv_args\* __restrict__ table\)", text)
    assert name, "no table entry"
    assert f"{name.group(1)}_small1(const gdv_args A)" in text
    assert f" {name.group(1)}(" not in text                     # no one-batch entry: that call keeps its own kernels
    assert "table[blockIdx.y]" in text and "*(gdv_int64*)A.aux2" in text
    # the windowed body: the LDS window, the rounds, the re-read path of a wave tile that overflows the window
    assert "GDV_FP_CAP" in text and "for (int kb = 0; kb < GDV_FP_K; kb++)" in text and "gdv_one<" in text
    assert "gdv_bits_flush_local(" in text
    # the workgroup zeroes every output validity bitmap and the boolean output's data bitmap, then fences
    for e in range(5):
        assert f"A.out[{e}].valid[w] = 0;" in text
    assert "((gdv_uint64*)A.out[2].data)[w] = 0;" in text and "((gdv_uint64*)A.out[0].data)[w] = 0;" not in text
    assert text.index(".valid[w] = 0;") < text.index("__threadfence();") < text.index("for (gdv_int64 tile = 0; tile < ntiles; tile++)")


def test_the_small_plan_has_no_look_back_and_no_ticket(threshold_plan):
    for mode in (0, 2):
        small, windowed = threshold_plan.text(mode, SMALL), threshold_plan.text(mode, MAIN)
        assert "gdv_fp_lookback" in windowed and "__hip_atomic_fetch_add" in windowed and "wg_ticket" in windowed
        for needle in ("gdv_fp_lookback", "__hip_atomic_fetch_add", "wg_ticket", "A.mask", "A.counts", "gridDim"):
            assert needle not in small, needle
        assert "*wg_run = e + wg_total;" in small


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_windowed_and_direct_text_and_names_do_not_depend_on_the_small_plan(threshold_plan, mode):
    for shape in (MAIN, DIRECT):
        with_small, without = threshold_plan.text(mode, shape, 1), threshold_plan.text(mode, shape, 0)
        assert with_small is not None and with_small == without       # (the text carries the kernel's name)
    assert threshold_plan.text(mode, SMALL, 0) is None                # not requested: no small plan
    names = {re.search(r"gdv_k_[0-9a-f]{16}", threshold_plan.text(mode, s)).group(0) for s in (MAIN, DIRECT, SMALL)}
    assert len(names) == 3                                            # three kernels, three disk-cache keys


def test_a_plan_with_the_direct_shape_only_has_no_small_plan(threshold_plan):
    lib = _capi.lib()
    # rows too wide for the LDS window: eleven int64 outputs + the index are 92 bytes per row
    batch = _batch(np.random.default_rng(0), 100, 0.1)
    bld = gandiva.TreeExprBuilder()
    a, b = (bld.make_field(batch.schema.field(i)) for i in range(2))
    cond = bld.make_condition(bld.make_function("greater_than", [a, bld.make_literal(5, I64)], pa.bool_()))
    wide = [bld.make_expression(bld.make_function("add", [a, bld.make_function("multiply", [b, bld.make_literal(k, I64)], I64)], I64),
                                pa.field(f"o{k}", I64)) for k in range(11)]
    p = _Planned(batch.schema, cond, wide)
    try:
        main = p.text(2, MAIN)
        assert main is not None and "GDV_FP_CAP" not in main
        assert p.text(2, DIRECT) is None
        assert p.text(2, SMALL) is None
        assert "no small shape" in _capi.last_error()
    finally:
        p.close()
    # bool outputs only and no selection vector: nothing to window
    q = _Planned(batch.schema, threshold_plan.cond, threshold_plan.exprs[2:3])
    try:
        assert q.text(0, SMALL) is None and "no small shape" in _capi.last_error()
        assert q.text(2, SMALL) is not None       # with an index to window it has one
    finally:
        q.close()
    assert lib.gdv_filter_project_small_batch_rows(None) == 0
