"""Device time per Evaluate of C4's arithmetic fed from text: castDECIMAL(utf8) of the three price columns rendered as text
("1234.56", "0.05"), next to C4's own kernel on the same values as decimal128 columns, same process, same row count.
HBM-resident inputs and outputs: HIP events around evaluate_device, 5 warm-up calls, median of `steps` calls (and their
min / max).  Prints, per plan, ms, algorithmic bytes (each input byte read once, each output byte written once) and the fraction
of 8 TB/s; the two plans' outputs are compared bit for bit on the device.  Kernel times come from a separate run of this
script under `rocprofv3 --kernel-trace --stats` (kernel names: the gdv_k_ lines this script prints).
Usage: python tools/decimal_tail_timing.py [rows=10^7] [steps=30]"""
import json
import os
import re
import sys

import numpy as np
import pyarrow as pa
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import gandiva_amd as gandiva  # noqa: E402
from gandiva_amd import workloads as W  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
WARMUP = 5

host = W.c4_batch(n)
text_schema = pa.schema([pa.field(f.name, pa.string()) for f in list(host.schema)[:3]] + [host.schema.field(3)])
text_host = pa.RecordBatch.from_arrays([host.column(k).cast(pa.string()) for k in range(3)] + [host.column(3)], schema=text_schema)
text_bytes = [int(text_host.column(k).buffers()[2].size) for k in range(3)]
dec_dev, text_dev = gandiva.DeviceBatch.from_arrow(host), gandiva.DeviceBatch.from_arrow(text_host)


def plan(schema, cast):
    b = gandiva.TreeExprBuilder()
    d152 = pa.decimal128(15, 2)
    ep, disc, tax = ((b.make_function("castDECIMAL", [b.make_field(schema.field(k))], d152) if cast else b.make_field(schema.field(k)))
                     for k in range(3))
    one = b.make_literal(100, d152)
    disc_price = b.make_function("multiply", [ep, b.make_function("subtract", [one, disc], pa.decimal128(16, 2))], pa.decimal128(32, 4))
    charge = b.make_function("multiply", [disc_price, b.make_function("add", [one, tax], pa.decimal128(16, 2))], pa.decimal128(38, 6))
    days = b.make_function("datediff", [b.make_literal(W.C4_DATE_1998_12_01, pa.date32()), b.make_field(schema.field(3))], pa.int32())
    return gandiva.make_projector(schema, [b.make_expression(disc_price, pa.field("disc_price", pa.decimal128(32, 4))),
                                           b.make_expression(charge, pa.field("charge", pa.decimal128(38, 6))),
                                           b.make_expression(days, pa.field("days", pa.int32()))], None)


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
    return float(np.median(ts)), float(min(ts)), float(max(ts)), out


out_bytes = (16 + 16 + 4) * n            # no input has nulls: no validity is read, none has to be written
plans = {"c4": ("C4 on decimal128 columns", plan(host.schema, False), dec_dev, 3 * 16 * n + 4 * n + out_bytes),
         "text": ("C4 on castDECIMAL(utf8) of three text columns (%.1f / %.1f / %.1f bytes a row)" % tuple(t / n for t in text_bytes),
                  plan(text_schema, True), text_dev, 3 * 4 * (n + 1) + sum(text_bytes) + 4 * n + out_bytes)}
results, outs = {}, {}
for key, (name, proj, db, algo) in plans.items():
    ms, lo, hi, outs[key] = timed(lambda: proj.evaluate_device(db))
    kernels = sorted(set(re.findall(r"gdv_k_[0-9a-f]{16}", proj.llvm_ir)))
    results[key] = {"plan": name, "rows": n, "ms": round(ms, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4), "algorithmic_bytes": algo,
                    "fraction_of_8TBps": round(algo / (ms * 1e-3) / 8e12, 4), "kernels": kernels}
    print(f"({key}) {name}: {n} rows, {ms:.3f} ms (min {lo:.3f}, max {hi:.3f}), {algo / 1e9:.3f} GB algorithmic, "
          f"{100 * results[key]['fraction_of_8TBps']:.1f} % of 8 TB/s, kernels {' '.join(kernels)}")
for a, b in zip(outs["c4"], outs["text"]):
    assert torch.equal(a.data, b.data), "the two plans' outputs differ"
print(f"text / c4: {results['text']['ms'] / results['c4']['ms']:.2f}x; outputs bit-equal")
print(json.dumps({"rows": n, "steps": steps, "warmup": WARMUP, "device": torch.cuda.get_device_name(0), "results": results}))
