"""bench.py's CPU-side legs (no GPU): the argument parser, the per-workload tables and the short cpu_baseline of every
sub-workload of the driver's line — the oracle ("port") timed on a bounded sample, as the task's measurement contract asks."""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_defaults_are_the_drivers_invocation_and_every_workload_is_described(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = bench.parse()
    assert (a.gpus, a.workload, a.scaling, a.no_extras) == (1, "c2", "weak", False)
    assert a.extras.split(",") == ["c1", "c3", "k2f", "c5", "c4"] and a.pool_candidates == 8 and a.placements == 1
    for w in ["c2"] + a.extras.split(","):
        assert w in bench.WORKLOAD_TEXT and w in bench.DEFAULT_ROWS and w in bench.STRONG_ROWS and w in bench.CEILING_SHAPE
    assert bench.DEFAULT_ROWS["c2"] == 1 << 28 and bench.DEFAULT_ROWS["c3"] == 10**9 and bench.DEFAULT_ROWS["c5"] == 10**8
    assert bench.STRONG_ROWS["c4"] == 6 * 10**9 and bench.DEFAULT_ROWS["c4"] * 8 == bench.STRONG_ROWS["c4"]


def test_a_plain_run_checks_nothing_and_full_is_opt_in(monkeypatch):
    """Without --full the bench sets up, warms up, times, dumps and prints: its outputs are not checked (the workload is
    not even looked at); --full checks them unless --no-verify."""
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = bench.parse()
    assert a.full is False
    assert bench.verify(None, a)["ok"] is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-verify"])
    a = bench.parse()
    assert a.full is True and bench.verify(None, a) == {"ok": None, "what": "skipped (--no-verify)"}


def test_short_cpu_baselines_run_on_bounded_samples():
    bench = _bench()
    for name in ("c1", "c3", "k2f", "c4", "c5"):
        b = bench.short_cpu_baseline(name, 0.2)
        assert b["kind"] == "port" and b["unit"] == "million rows/s" and b["value"] > 0 and b["cores"] >= 1, (name, b)
        assert "passes x" in b["sample"]


def test_dump_outputs_writes_a_seeded_sample_of_what_the_last_step_left(tmp_path, monkeypatch):
    """--dump-outputs DIR: DIR/<name>.npy in float64 / float32, the same sampled rows on every run, values under a null
    written as 0, at most 64 MB (here: C2's ten outputs and C3's selection vector in host tensors, no device)."""
    import types
    import numpy as np
    import pyarrow as pa
    import pytest
    import torch
    from gandiva_amd.gandiva import DeviceColumn, SelectionVector
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--dump-outputs", str(tmp_path)])
    assert bench.parse().dump_outputs == str(tmp_path)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()
    n = 1 << 20
    rng = np.random.default_rng(5)
    valid = rng.random(n) >= 0.1
    vals = [rng.standard_normal(n) for _ in range(10)]
    outs = [DeviceColumn(pa.float64(), n, torch.from_numpy(np.packbits(valid, bitorder="little")),
                         torch.from_numpy(v).view(torch.uint8)) for v in vals]
    size = bench.dump_outputs(types.SimpleNamespace(name="c2", rows=n, outs=outs), str(tmp_path))
    assert 0 < size <= bench.DUMP_LIMIT_BYTES
    rows = np.load(tmp_path / "rows.npy")
    assert rows.dtype == np.float64 and np.array_equal(rows, bench.dump_sample(n, 1 << 18))
    r = rows.astype(np.int64)
    for e in range(10):
        got, ok = np.load(tmp_path / f"e{e}.npy"), np.load(tmp_path / f"e{e}_valid.npy")
        assert got.dtype == np.float64 and ok.dtype == np.float32
        assert np.array_equal(ok, valid[r]) and np.array_equal(got, np.where(valid[r], vals[e][r], 0.0))
    idx = np.flatnonzero(valid).astype(np.uint32)
    buf = torch.from_numpy(np.concatenate([idx, np.zeros(n - idx.size, np.uint32)]).view(np.int32))
    sel = SelectionVector(2, buf, None, device=True, count_tensor=torch.tensor([idx.size]))
    got = bench.dump_arrays(types.SimpleNamespace(name="c3", rows=n, last=sel))
    assert got["num_slots"][0] == idx.size
    assert np.array_equal(got["indices"], idx[got["positions"].astype(np.int64)].astype(np.float64))
    with pytest.raises(RuntimeError):
        bench.dump_outputs(types.SimpleNamespace(name="c3", rows=n, last=sel), str(tmp_path / "small"), budget=1024)
