"""Device time per Evaluate of the string-tail functions on C5's column (utf8, lengths 4..20, letters only), HBM-resident
inputs and outputs: HIP events around evaluate_device, 5 warm-up calls, median of 30 steps.  Prints, per plan, ms,
algorithmic bytes (each input byte read once, each output byte written once), the fraction of 8 TB/s and the ratio to the
identity projection (a).  repeat(s, 2) (d) would exceed the 2 GiB of one var-len output at 10^8 rows: it runs on the
first half of the column, and its ratio is to the identity projection of that same half (a/2).  Two windows of every output are checked against the restatement of
tests/test_string_tail_cpu.py.  Usage: python tools/string_tail_timing.py [rows=10^8] [steps=30]"""
import json
import os
import sys

import numpy as np
import pyarrow as pa
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import gandiva_amd as gandiva  # noqa: E402
from gandiva_amd import workloads as W  # noqa: E402
import test_string_tail_cpu as R  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
WARMUP, WIN = 5, 20_000
db = W.c5_device_batch(n)
sch = W.c5_schema()
b = gandiva.TreeExprBuilder()
s = b.make_field(sch.field(0))
STR, I32 = pa.string(), pa.int32()
lit = lambda v, t=STR: b.make_literal(v, t)  # noqa: E731
fn = lambda name, args: b.make_function(name, args, STR)  # noqa: E731
col = db.columns[0]
in_off = col.offsets[: 4 * (n + 1)].view(torch.int32)
in_bytes = int(in_off[n].item())


def rows(off_t, data_t, lo, cnt):
    off = off_t[lo: lo + cnt + 1].cpu().numpy().astype(np.int64)
    raw = data_t[int(off[0]): int(off[-1])].cpu().numpy().tobytes()
    return [raw[off[i] - off[0]: off[i + 1] - off[0]] for i in range(cnt)]


PLANS = {
    "a": ("identity s", [s], lambda t: t),
    "b": ("split_part(s, ' ', 2)", [fn("split_part", [s, lit(" "), lit(2, I32)])], lambda t: R.split_part(t, b" ", 2)),
    "c": ("filter equal(substring_index(s, ' ', 1), 'spark')", None, lambda t: R.substring_index(t, b" ", 1) == b"spark"),
    "a/2": ("identity s, first half of the rows", [s], lambda t: t),
    "d": ("repeat(s, 2), first half of the rows", [fn("repeat", [s, lit(2, I32)])], lambda t: R.repeat(t, 2)),
    "e": ("translate(s, 'abc', 'xyz')", [fn("translate", [s, lit("abc"), lit("xyz")])], lambda t: R.translate(t, b"abc", b"xyz")),
}


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


results = {}
full = db
for key, (name, nodes, ref) in PLANS.items():
    db = gandiva.DeviceBatch(sch, full.columns, n // 2) if key in ("a/2", "d") else full
    m = db.num_rows
    WINDOWS = (0, m - WIN)
    if nodes is None:
        cond = b.make_condition(b.make_function("equal", [b.make_function("substring_index", [s, lit(" "), lit(1, I32)], STR),
                                                          lit("spark")], pa.bool_()))
        flt = gandiva.make_filter(sch, cond)
        ms, sel = timed(lambda: flt.evaluate_device(db, "int32"))
        idx = sel.indices[: sel.num_slots].cpu().numpy().astype(np.int64)
        for lo in WINDOWS:
            want = [lo + i for i, t in enumerate(rows(in_off, col.data, lo, WIN)) if ref(t)]
            got = idx[(idx >= lo) & (idx < lo + WIN)].tolist()
            assert got == want, f"{name}: window {lo}"
        algo = 4 * (n + 1) + in_bytes + 4 * sel.num_slots
    else:
        proj = gandiva.make_projector(sch, [b.make_expression(nd, pa.field("o", STR)) for nd in nodes], None)
        ms, outs = timed(lambda: proj.evaluate_device(db))
        o = outs[0]
        o_off = o.offsets[: 4 * (m + 1)].view(torch.int32)
        for lo in WINDOWS:
            assert rows(o_off, o.data, lo, WIN) == [ref(t) for t in rows(in_off, col.data, lo, WIN)], f"{name}: window {lo}"
        algo = 2 * 4 * (m + 1) + int(in_off[m].item()) + int(o_off[m].item())
    results[key] = {"plan": name, "rows": m, "ms": round(ms, 4), "algorithmic_bytes": algo, "fraction_of_8TBps": round(algo / (ms * 1e-3) / 8e12, 4)}
    torch.cuda.synchronize()

for key, r in results.items():
    base = "a/2" if key in ("a/2", "d") else "a"
    r["ratio_to"] = base
    r["ratio"] = round(r["ms"] / results[base]["ms"], 3)
    print(f"({key}) {r['plan']}: {r['rows']} rows, {r['ms']:.3f} ms, {r['algorithmic_bytes'] / 1e9:.2f} GB algorithmic, "
          f"{100 * r['fraction_of_8TBps']:.1f} % of 8 TB/s, {r['ratio']:.2f}x ({base})")
print(json.dumps({"rows": n, "steps": steps, "warmup": WARMUP, "windows_checked": "first and last 20000 rows of each plan", "window_rows": WIN,
                  "device": torch.cuda.get_device_name(0), "results": results}))
