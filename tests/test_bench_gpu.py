"""bench.py on the device: a plain run prints the headline line and leaves everything else to --full."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_plain_run_prints_the_headline_and_leaves_the_rest_to_full(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--rows", "1048576", "--steps", "5",
                        "--warmup", "2", "--data", "philox", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["metric"] == "million rows/sec, 10-expr float64 Projector (10% nulls)" and line["unit"] == "million rows/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f64" and line["steps"] == 5 and line["warmup"] == 2
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["roofline"]["kernel_ms"] > 0
    # nothing of --full: no check, no CPU baseline, no sub-lines, no ceilings or telemetry
    assert line["verified"] is None and line["verification"]["ok"] is None
    assert "cpu_baseline" not in line and "workloads" not in line
    assert "box" not in line["roofline"] and "measured_ceiling" not in line["roofline"]
    # --dump-outputs still writes the headline's arrays (a --rows run has no sub-workloads)
    names = sorted(os.listdir(tmp_path))
    assert "rows.npy" in names and "e9.npy" in names and "e9_valid.npy" in names
    assert not [n for n in names if n.split("_")[0] in ("c1", "c3", "k2f", "c5", "c4")]
