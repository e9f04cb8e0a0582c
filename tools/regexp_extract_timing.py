"""Device time per Evaluate of regexp_extract(s, '(\\w+)@(\\w+)', 2) against regexp_like(s, '(\\w+)@(\\w+)') — the floor: it
reads the same bytes and keeps one 64-bit set where extraction keeps an ordered list with extents — on C5's column (utf8,
lengths 4..20, ASCII letters: no row holds an '@', so no row matches) and on the same column with an '@' planted inside
every second row.  HBM-resident inputs and outputs, HIP events around evaluate_device, 5 warm-up calls, median of the
steps.  The first 20000 rows of every result are checked against RE2 (pyarrow.compute).
Usage: python tools/regexp_extract_timing.py [rows=10^6] [steps=30]"""
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

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
WARMUP, WIN = 5, 20_000
PATTERN = "(\\w+)@(\\w+)"
STR, I32 = pa.string(), pa.int32()


def column(with_at):
    offsets, data, _ = W.c5_numpy(n)
    if with_at:
        rows = np.arange(0, n, 2)
        data[(offsets[rows] + (offsets[rows + 1] - offsets[rows]) // 2).astype(np.int64)] = ord("@")
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
extract = gandiva.make_projector(sch, [b.make_expression(b.make_function(
    "regexp_extract", [s, b.make_literal(PATTERN, STR), b.make_literal(2, I32)], STR), pa.field("o", STR))], None)
like = gandiva.make_projector(sch, [b.make_expression(b.make_function(
    "regexp_like", [s, b.make_literal(PATTERN, STR)], pa.bool_()), pa.field("o", pa.bool_()))], None)
results = {}
for name, with_at in (("c5", False), ("c5_with_at", True)):
    batch = column(with_at)
    db = gandiva.DeviceBatch.from_arrow(batch)
    head = batch.column(0).slice(0, WIN)
    ms_x, outs = timed(lambda: extract.evaluate_device(db))
    got = outs[0].to_arrow().slice(0, WIN)
    want = pc.struct_field(pc.extract_regex(head, pattern="(?P<a>\\w+)@(?P<b>\\w+)"), [1]).fill_null("")
    assert got.to_pylist() == want.to_pylist(), name
    ms_l, outs = timed(lambda: like.evaluate_device(db))
    assert outs[0].to_arrow().slice(0, WIN).to_pylist() == pc.match_substring_regex(head, pattern=PATTERN).to_pylist(), name
    in_bytes = int(batch.column(0).buffers()[1].size + batch.column(0).buffers()[2].size)
    results[name] = {"rows": n, "input_bytes": in_bytes, "matching_rows": int(pc.sum(pc.match_substring_regex(batch.column(0), pattern=PATTERN)).as_py()),
                     "regexp_extract_ms": round(ms_x, 4), "regexp_like_ms": round(ms_l, 4), "ratio": round(ms_x / ms_l, 2)}
    print(f"{name}: {n} rows, {results[name]['matching_rows']} match; regexp_extract {ms_x:.3f} ms, regexp_like {ms_l:.3f} ms, "
          f"ratio {ms_x / ms_l:.2f}x")
print(json.dumps({"pattern": PATTERN, "group": 2, "steps": steps, "warmup": WARMUP, "rows_checked_against_re2": WIN,
                  "device": torch.cuda.get_device_name(0), "results": results}))
