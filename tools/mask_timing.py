"""Device time per Evaluate of mask(s), mask_first_n(s, 4) and mask_show_last_n(s, 4) (values of their own kind: a pre-pass over
the offsets that reads no byte, the scan, a main kernel whose copy classifies eight bytes per step) against three plans this
family does not touch: the identity projection of the column, upper(s) on the flat path and translate(s, 'abc', 'xyz') (the
nearest value of the same shape with a byte loop in its copy), all in one process: on C5's column (utf8, lengths 4..20, ASCII)
and on the same column with 'é' planted into 1 % and into 30 % of the rows.  HBM-resident inputs and outputs, HIP events around
evaluate_device, 5 warm-up calls, median of the steps; no threshold.  The first 20000 rows of every result are checked against
re.sub / str slicing.  Writes profiles/mask.txt (and prints the same lines).
Usage: python tools/mask_timing.py [rows=5*10^7] [steps=20] [output file] [only: a comma-separated list of plan names]"""
import json
import os
import re
import sys

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gandiva_amd as gandiva  # noqa: E402
from gandiva_amd import workloads as W  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 50_000_000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "mask.txt")
only = sys.argv[4].split(",") if len(sys.argv) > 4 else None
WARMUP, WIN = 5, 20_000
STR, I32 = pa.string(), pa.int32()


def column(share):
    """C5's column; `share` of the rows get U+00E9 (two bytes) over their second and third byte"""
    offsets, data, _ = W.c5_numpy(n)
    if share > 0:
        rows = np.flatnonzero(np.random.default_rng(3).random(n) < share)
        at = offsets[rows].astype(np.int64) + 1
        data[at] = 0xC3
        data[at + 1] = 0xA9
    arr = pa.Array.from_buffers(STR, n, [None, pa.py_buffer(offsets), pa.py_buffer(data)])
    return pa.RecordBatch.from_arrays([arr], names=["s"])


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


def resub(v):
    return re.sub("[0-9]", "n", re.sub("[a-z]", "x", re.sub("[A-Z]", "X", v)))


sch = W.c5_schema()
b = gandiva.TreeExprBuilder()
s = b.make_field(sch.field(0))


def make(node):
    return gandiva.make_projector(sch, [b.make_expression(node, pa.field("o", STR))], None)


def strings(f, a):
    return pa.array([f(v) for v in a.to_pylist()], STR)


plans = [("mask", lambda: make(b.make_function("mask", [s], STR)), lambda a: strings(resub, a)),
         ("mask_first_n", lambda: make(b.make_function("mask_first_n", [s, b.make_literal(4, I32)], STR)),
          lambda a: strings(lambda v: resub(v[:4]) + v[4:], a)),
         ("mask_show_last_n", lambda: make(b.make_function("mask_show_last_n", [s, b.make_literal(4, I32)], STR)),
          lambda a: strings(lambda v: resub(v[:max(len(v) - 4, 0)]) + v[max(len(v) - 4, 0):], a)),
         ("identity", lambda: make(s), lambda a: a),
         ("upper_flat", lambda: make(b.make_function("upper", [s], STR)), pc.ascii_upper),
         ("translate", lambda: make(b.make_function("translate", [s, b.make_literal("abc", STR), b.make_literal("xyz", STR)], STR)),
          lambda a: strings(lambda v: v.translate(str.maketrans("abc", "xyz")), a))]
plans = [(name, mk(), want) for name, mk, want in plans if only is None or name in only]
lines = []
results = {}
for name, share in (("c5", 0.0), ("c5_1pct", 0.01), ("c5_30pct", 0.30)):
    batch = column(share)
    db = gandiva.DeviceBatch.from_arrow(batch)
    head = batch.column(0).slice(0, WIN)
    in_bytes = int(batch.column(0).buffers()[1].size + batch.column(0).buffers()[2].size)
    row = {"rows": n, "input_bytes": in_bytes, "rows_with_a_two_byte_letter": share}
    for pname, proj, want in plans:
        ms, outs = timed(lambda: proj.evaluate_device(db))
        got = outs[0].to_arrow().slice(0, WIN)
        assert got.to_pylist() == want(head).to_pylist(), (name, pname)
        row[pname + "_ms"] = round(ms, 4)
        del outs
    text = f"{name}: {n} rows, {share:.0%} with a two-byte letter;"
    for pname, _, _ in plans:
        text += f" {pname} {row[pname + '_ms']:.3f} ms"
        if pname.startswith("mask"):
            ratios = {k: round(row[pname + "_ms"] / row[k + "_ms"], 2) for k in ("identity", "upper_flat", "translate") if k + "_ms" in row}
            row[pname + "_vs"] = ratios
            text += " (" + ", ".join(f"{v:.2f}x {k}" for k, v in ratios.items()) + ")" if ratios else ""
        text += ";"
    results[name] = row
    lines.append(text)
    print(lines[-1], flush=True)
    del db, batch
lines.append(json.dumps({"steps": steps, "warmup": WARMUP, "rows_checked": WIN, "device": torch.cuda.get_device_name(0), "results": results}))
print(lines[-1])
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("# tools/mask_timing.py %d %d: device time per Evaluate (HIP events around evaluate_device, median of the steps)\n" % (n, steps))
    f.write("\n".join(lines) + "\n")
