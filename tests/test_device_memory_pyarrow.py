"""pyarrow.gandiva — the reference lineage's own binding, unmodified — over batches that live in HBM:
`batch.copy_to(pyarrow_gandiva.hip_memory_manager())`, `evaluate`, `result.copy_to(cpu)`.  The known answers are the
lineage's (pyarrow/tests/test_gandiva.py: test_table, test_regex, test_filter)."""
import pyarrow as pa
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gandiva():
    from gandiva_amd import pyarrow_gandiva
    return pyarrow_gandiva.load()   # (as tests/test_pyarrow_gandiva.py: a module that does not build or load is a failure)


@pytest.fixture(scope="module")
def mm(gandiva):
    from gandiva_amd import pyarrow_gandiva
    manager = pyarrow_gandiva.hip_memory_manager()
    assert isinstance(manager, pa.MemoryManager) and not manager.is_cpu
    assert manager.device.device_type == pa.DeviceAllocationType.ROCM and manager.device.device_id == 0
    return manager


def _cpu():
    return pa.default_cpu_memory_manager()


def test_add_float64_on_a_device_batch(gandiva, mm):
    table = pa.Table.from_arrays([pa.array([1.0, 2.0]), pa.array([3.0, 4.0])], ['a', 'b'])
    builder = gandiva.TreeExprBuilder()
    node_a = builder.make_field(table.schema.field("a"))
    node_b = builder.make_field(table.schema.field("b"))
    expr = builder.make_expression(builder.make_function("add", [node_a, node_b], pa.float64()), pa.field("c", pa.float64()))
    projector = gandiva.make_projector(table.schema, [expr], pa.default_memory_pool())
    batch = table.to_batches()[0]
    dbatch = batch.copy_to(mm)
    assert not dbatch.column(0).is_cpu
    r, = projector.evaluate(dbatch)
    assert r.is_cpu is False
    back = r.copy_to(_cpu())
    assert back.equals(pa.array([4.0, 6.0]))
    assert back.equals(projector.evaluate(batch)[0])


def test_like_on_a_device_batch(gandiva, mm):
    data = pa.array(["park", "sparkle", "bright spark and fire", "spark"], type=pa.string())
    table = pa.Table.from_arrays([data], names=['a'])
    builder = gandiva.TreeExprBuilder()
    node_a = builder.make_field(table.schema.field("a"))
    like = builder.make_function("like", [node_a, builder.make_literal("%spark%", pa.string())], pa.bool_())
    projector = gandiva.make_projector(table.schema, [builder.make_expression(like, pa.field("b", pa.bool_()))],
                                       pa.default_memory_pool())
    batch = table.to_batches()[0]
    r, = projector.evaluate(batch.copy_to(mm))
    assert r.is_cpu is False
    back = r.copy_to(_cpu())
    assert back.equals(pa.array([False, True, True, True], type=pa.bool_()))
    assert back.equals(projector.evaluate(batch)[0])


def test_filter_on_a_device_batch(gandiva, mm):
    """pyarrow's Filter.evaluate allocates its selection vector from a MemoryPool, so the vector is the host's: the
    indices are computed next to the batch and the selected ones are copied out."""
    table = pa.Table.from_arrays([pa.array([1.0 * i for i in range(10000)])], ['a'])
    builder = gandiva.TreeExprBuilder()
    node_a = builder.make_field(table.schema.field("a"))
    cond = builder.make_function("less_than", [node_a, builder.make_literal(1000.0, pa.float64())], pa.bool_())
    flt = gandiva.make_filter(table.schema, builder.make_condition(cond))
    batch = table.to_batches()[0]
    got = flt.evaluate(batch.copy_to(mm), pa.default_memory_pool())
    assert got.to_array().equals(pa.array(range(1000), type=pa.uint32()))
    assert got.to_array().equals(flt.evaluate(batch, pa.default_memory_pool()).to_array())


def test_the_pool_retains_and_trims(gandiva, mm):
    from gandiva_amd import pyarrow_gandiva
    batch = pa.RecordBatch.from_arrays([pa.array([1.0 * i for i in range(4097)])], names=['a'])
    dbatch = batch.copy_to(mm)
    total, in_use = pyarrow_gandiva.reserved_bytes()
    assert total >= in_use >= 4097 * 8
    del dbatch
    total, in_use = pyarrow_gandiva.reserved_bytes()
    assert total >= 4097 * 8 and in_use == 0      # dropped buffers stay in the pool ...
    pyarrow_gandiva.trim()
    assert pyarrow_gandiva.reserved_bytes() == (0, 0)   # ... until it is trimmed
