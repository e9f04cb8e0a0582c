"""An asynchronous caller may enqueue far ahead of the GPU: the library's scratch blocks must not grow with the run-ahead
(round 6: Runtime::Alloc waits for the oldest block of a size once eight of that size are waiting for their streams)."""
import pytest


@pytest.mark.gpu
def test_scratch_of_asynchronous_evaluations_is_bounded_by_the_run_ahead_cap():
    import torch
    import gandiva_amd as gandiva
    from gandiva_amd import workloads as W
    rows = 50_000_000
    batch = W.c5_device_batch_philox(rows)
    proj = gandiva.make_projector(W.c5_schema(), W.c5_expressions(), None)
    outs, result = proj.evaluate_device_async(batch)
    torch.cuda.synchronize()
    assert int(result[0].item()) == 0
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(100):          # ~0.5 ms of GPU work each, enqueued faster than that
        outs, result = proj.evaluate_device_async(batch, outputs=outs)
    free1, _ = torch.cuda.mem_get_info()
    torch.cuda.synchronize()
    assert int(result[0].item()) == 0
    # per call: head + counts + bases + chunks + state, ~1.6 MB at this size: eight calls' worth is ~13 MB, a run-ahead of
    # 50-100 calls would be 80-160 MB.  (torch's own allocations are cached and do not move mem_get_info inside the loop.)
    assert free0 - free1 < 48 << 20, f"scratch grew by {(free0 - free1) >> 20} MiB over 100 asynchronous calls"


@pytest.mark.gpu
def test_threads_running_ahead_on_one_context_share_the_deferred_blocks():
    """Four threads, one device context, one var-len projector, 40 asynchronous calls each on a 2049-row batch (one full
    2048-row tile and a one-row tail): every call allocates the same scratch sizes, so more than eight blocks of a size
    are pending across the threads and one thread waits for the oldest of them while the others reap.  Whoever takes an
    entry out of the queue is its only owner (gdv_reclaim.h): every thread's last result is the oracle's."""
    import threading
    import pyarrow as pa
    import torch
    import gandiva_amd as gandiva
    from gandiva_amd import workloads as W
    from oracle import oracle
    from helpers import assert_bit_exact
    rows, calls, nthreads = 2049, 40, 4
    exprs = W.c5_expressions()
    proj = gandiva.make_projector(W.c5_schema(), exprs, None)
    batches = []
    for i in range(nthreads):
        offsets, data, _ = W.c5_numpy(rows, seed=21 + i)
        arr = pa.Array.from_buffers(pa.string(), rows, [None, pa.py_buffer(offsets), pa.py_buffer(data)])
        batches.append(pa.RecordBatch.from_arrays([arr], schema=W.c5_schema()))
    want = [oracle.project(exprs, b) for b in batches]
    dbatches = [gandiva.DeviceBatch.from_arrow(b) for b in batches]
    streams = [torch.cuda.Stream() for _ in range(nthreads)]
    proj.evaluate_device(dbatches[0])   # (the kernels are loaded before the threads start)
    torch.cuda.synchronize()
    last, errors = [None] * nthreads, []

    def work(i):
        try:
            with torch.cuda.stream(streams[i]):
                # (substr and upper never produce more bytes than they read)
                outs, result = proj.evaluate_device_async(dbatches[i], capacity_bytes=batches[i].column(0).buffers()[2].size + 64)
                for _ in range(calls - 1):
                    outs, result = proj.evaluate_device_async(dbatches[i], outputs=outs)
                streams[i].synchronize()
                last[i] = (int(result[0].item()), [o.to_arrow() for o in outs])
        except Exception as e:  # noqa: BLE001
            errors.append((i, repr(e)))
    threads = [threading.Thread(target=work, args=(i,)) for i in range(nthreads)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(nthreads):
        status, got = last[i]
        assert status == 0, f"thread {i}: error word {status}"
        for g, w in zip(got, want[i]):
            assert_bit_exact(g, w, f"thread {i}")
