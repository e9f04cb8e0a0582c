"""Device time per Evaluate of sin(x), atan2(x, y), round(x, 2), pmod(a, b) and gcd(a, b) against three plans this family
does not touch — exp(x), power(x, y) and add(a, b) — all in one process, on the specialised kernels (GDV_NO_TIER0=1): 2^26
float64 / int64 rows, HBM-resident inputs and outputs, HIP events around evaluate_device, 5 warm-up calls, median of the
steps; no threshold.  The expectation to confirm or refute: round(x, 2) and pmod stay memory-bound like add, the libm ones sit
near exp, gcd's divergence is the outlier.  x, y: uniform in [-100, 100]; a: full-range int64, b: int64 below 2^31, no zeros.
The first 2000 rows of the bit-for-bit plans are checked against Python.  Prints its lines and, given a file, writes them.
Usage: python tools/numeric_tail_timing.py [rows=2^26] [steps=20] [output file] [only: a comma-separated list of plan names]"""
import json
import math
import os
import sys

os.environ.setdefault("GDV_NO_TIER0", "1")

import numpy as np  # noqa: E402
import pyarrow as pa  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gandiva_amd as gandiva  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 26
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
out_path = sys.argv[3] if len(sys.argv) > 3 else None
only = sys.argv[4].split(",") if len(sys.argv) > 4 else None
WARMUP, WIN = 5, 2000
F64, I64, I32 = pa.float64(), pa.int64(), pa.int32()

rng = np.random.default_rng(11)
cols = {"x": rng.uniform(-100.0, 100.0, n), "y": rng.uniform(-100.0, 100.0, n),
        "a": rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64), "b": rng.integers(1, 2 ** 31, n, dtype=np.int64)}
sch = pa.schema([("x", F64), ("y", F64), ("a", I64), ("b", I64)])
batch = pa.RecordBatch.from_arrays([pa.array(cols[f.name], f.type) for f in sch], schema=sch)
b = gandiva.TreeExprBuilder()
x, y, a, bb = (b.make_field(f) for f in sch)


def timed(call):
    for _ in range(WARMUP):
        out = call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = call()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), out


def half_away(v):
    m = v * 100.0
    return math.trunc(m + (0.5 if v >= 0 else -0.5)) / 100.0


# name, tree, result type, bytes read per row, the check of the first rows (None: a libm result, held to 1e-14 relative)
plans = [("sin", b.make_function("sin", [x], F64), F64, 8, None),
         ("atan2", b.make_function("atan2", [x, y], F64), F64, 16, None),
         ("round_2", b.make_function("round", [x, b.make_literal(2, I32)], F64), F64, 8, lambda r: half_away(r["x"])),
         ("pmod", b.make_function("pmod", [a, bb], I64), I64, 16, lambda r: r["a"] % r["b"]),
         ("gcd", b.make_function("gcd", [a, bb], I64), I64, 16, lambda r: math.gcd(abs(r["a"]), r["b"])),
         ("exp", b.make_function("exp", [x], F64), F64, 8, None),
         ("power", b.make_function("power", [x, y], F64), F64, 16, None),
         ("add", b.make_function("add", [a, bb], I64), I64, 16, lambda r: (r["a"] + r["b"] + 2 ** 63) % 2 ** 64 - 2 ** 63)]
libm = {"sin": lambda r: math.sin(r["x"]), "atan2": lambda r: math.atan2(r["x"], r["y"]), "exp": lambda r: math.exp(r["x"]),
        "power": lambda r: math.pow(r["x"], r["y"]) if r["x"] > 0 or r["y"] == int(r["y"]) else math.nan}
plans = [p for p in plans if only is None or p[0] in only]

db = gandiva.DeviceBatch.from_arrow(batch)
head = [dict(zip(sch.names, vals)) for vals in zip(*[batch.column(i).slice(0, WIN).to_pylist() for i in range(4)])]
lines, results = [], {}
for name, node, t, read, check in plans:
    proj = gandiva.make_projector(sch, [b.make_expression(node, pa.field("o", t))], None)
    ms, outs = timed(lambda: proj.evaluate_device(db))
    got = outs[0].to_arrow().slice(0, WIN).to_pylist()
    if check is not None:
        assert got == [check(r) for r in head], name
    else:
        for g, r in zip(got, head):
            w = libm[name](r)
            assert (g != g and w != w) or abs(g - w) <= 1e-14 * abs(w), (name, r, g, w)
    gbs = n * (read + 8) / ms / 1e6
    results[name] = {"ms": round(ms, 4), "bytes_per_row": read + 8, "GB_per_s": round(gbs, 1)}
    lines.append(f"{name}: {ms:.3f} ms per Evaluate, {read + 8} B/row moved, {gbs:.0f} GB/s")
    print(lines[-1], flush=True)
    del outs, proj
for name in ("sin", "atan2", "round_2", "pmod", "gcd"):
    if name in results:
        results[name]["vs"] = {k: round(results[name]["ms"] / results[k]["ms"], 2) for k in ("exp", "power", "add") if k in results}
        lines.append(f"{name} against " + ", ".join(f"{k}: {v:.2f}x" for k, v in results[name]["vs"].items()))
        print(lines[-1])
lines.append(json.dumps({"rows": n, "steps": steps, "warmup": WARMUP, "rows_checked": WIN, "device": torch.cuda.get_device_name(0), "results": results}))
print(lines[-1])
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("# tools/numeric_tail_timing.py %d %d: device time per Evaluate (HIP events around evaluate_device, median of the steps)\n" % (n, steps))
        f.write("\n".join(lines) + "\n")
