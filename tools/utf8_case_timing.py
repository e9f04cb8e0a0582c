"""Device time per Evaluate of upper(s) under GDV_UTF8_CASE=1 (utf8proc's map: a value of its own kind, pre-pass + scan + main
kernel) against the same expression with the option unset (the flat ASCII byte map over the column's own offsets), against the
identity projection of the column and against translate(s, 'abc', 'xyz') (the nearest value of the same shape: a row function
that returns the length, a copy that only writes), all in one process: on C5's column (utf8, lengths 4..20, ASCII) and on the
same column with 'é' planted into 1 % and into 30 % of the rows.  HBM-resident inputs and outputs, HIP events around
evaluate_device, 5 warm-up calls, median of the steps; measured once, no threshold.  The first 20000 rows of every result are
checked against pyarrow.compute.  Writes profiles/utf8_case.txt (and prints the same lines).
Usage: python tools/utf8_case_timing.py [rows=5*10^7] [steps=20] [output file]"""
import json
import os
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
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "utf8_case.txt")
WARMUP, WIN = 5, 20_000
STR = pa.string()


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


sch = W.c5_schema()
b = gandiva.TreeExprBuilder()
s = b.make_field(sch.field(0))
upper = b.make_expression(b.make_function("upper", [s], STR), pa.field("o", STR))


def make(expr, option):
    """the option is read at Make only"""
    if option:
        os.environ["GDV_UTF8_CASE"] = "1"
    else:
        os.environ.pop("GDV_UTF8_CASE", None)
    try:
        return gandiva.make_projector(sch, [expr], None)
    finally:
        os.environ.pop("GDV_UTF8_CASE", None)


plans = [("upper_utf8_case", make(upper, True), pc.utf8_upper),
         ("upper_flat", make(upper, False), pc.ascii_upper),
         ("identity", make(b.make_expression(s, pa.field("o", STR)), False), lambda a: a),
         ("translate", make(b.make_expression(b.make_function("translate", [s, b.make_literal("abc", STR), b.make_literal("xyz", STR)], STR),
                                              pa.field("o", STR)), False),
          lambda a: pa.array([v.translate(str.maketrans("abc", "xyz")) for v in a.to_pylist()], STR))]
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
    u = row["upper_utf8_case_ms"]
    row["vs_flat"], row["vs_identity"], row["vs_translate"] = (round(u / row[k], 2) for k in ("upper_flat_ms", "identity_ms", "translate_ms"))
    results[name] = row
    lines.append(f"{name}: {n} rows, {share:.0%} with a two-byte cased letter; upper(s) GDV_UTF8_CASE=1 {u:.3f} ms, flat {row['upper_flat_ms']:.3f} ms "
                 f"({row['vs_flat']:.2f}x), identity {row['identity_ms']:.3f} ms ({row['vs_identity']:.2f}x), translate {row['translate_ms']:.3f} ms "
                 f"({row['vs_translate']:.2f}x)")
    print(lines[-1], flush=True)
    del db, batch
lines.append(json.dumps({"steps": steps, "warmup": WARMUP, "rows_checked_against_pyarrow": WIN, "device": torch.cuda.get_device_name(0),
                         "results": results}))
print(lines[-1])
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("# tools/utf8_case_timing.py %d %d: device time per Evaluate (HIP events around evaluate_device, median of the steps)\n" % (n, steps))
    f.write("\n".join(lines) + "\n")
