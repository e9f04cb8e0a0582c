"""Device time per Evaluate of months_between(ts, ts), next_day(ts, 3) and add_months(ts, n), each beside the neighbour that
does the same civil-date work — timestampdiffMonth(ts, ts), date_trunc_Week(ts) and timestampaddMonth(n, ts) — all in one
process, on the specialised kernels (GDV_NO_TIER0=1): 2^26 rows, HBM-resident inputs and outputs, HIP events around
evaluate_device, 5 warm-up calls, median of the steps; no threshold.  The expectation to confirm or refute: each is near its
neighbour.  The instants are uniform over years 1..9999, n over +-1200 months.  The first 2000 rows are checked against
Python (tests/calendar_tail_reference.py).  Prints its lines and, given a file, writes them.
Usage: python tools/calendar_tail_timing.py [rows=2^26] [steps=20] [output file]"""
import json
import os
import sys

os.environ.setdefault("GDV_NO_TIER0", "1")

import numpy as np  # noqa: E402
import pyarrow as pa  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gandiva_amd as gandiva  # noqa: E402
import calendar_tail_reference as R  # noqa: E402
import temporal_reference as T  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 26
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
out_path = sys.argv[3] if len(sys.argv) > 3 else None
WARMUP, WIN = 5, 2000
TS, I64, I32, F64, D64 = pa.timestamp("ms"), pa.int64(), pa.int32(), pa.float64(), pa.date64()

rng = np.random.default_rng(13)
lo, hi = T.day_of(1, 1, 1) * T.MS, T.day_of(9999, 12, 31) * T.MS
cols = {"e": rng.integers(lo, hi, n, dtype=np.int64), "s": rng.integers(lo, hi, n, dtype=np.int64), "n": rng.integers(-1200, 1201, n, dtype=np.int64)}
sch = pa.schema([("e", TS), ("s", TS), ("n", I64)])
batch = pa.RecordBatch.from_arrays([pa.array(cols[f.name], I64).view(f.type) for f in sch], schema=sch)
b = gandiva.TreeExprBuilder()
e, s, cnt = (b.make_field(f) for f in sch)


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


# name, tree, result type, bytes read per row, result bytes, the rule of the first rows
plans = [("months_between", b.make_function("months_between", [e, s], F64), F64, 16, 8, lambda r: R.months_between(r["e"], r["s"])),
         ("timestampdiffMonth", b.make_function("timestampdiffMonth", [s, e], I32), I32, 16, 4, lambda r: T.timestampdiff("Month", r["s"], r["e"])),
         ("next_day", b.make_function("next_day", [e, b.make_literal(3, I32)], D64), D64, 8, 8, lambda r: R.next_day(r["e"], 3)),
         ("date_trunc_Week", b.make_function("date_trunc_Week", [e], TS), TS, 8, 8, lambda r: T.date_trunc("Week", r["e"])),
         ("add_months", b.make_function("add_months", [e, cnt], TS), TS, 16, 8, lambda r: R.add_months(r["e"], r["n"])),
         ("timestampaddMonth", b.make_function("timestampaddMonth", [cnt, e], TS), TS, 16, 8, lambda r: T.timestampadd("Month", r["n"], r["e"]))]

db = gandiva.DeviceBatch.from_arrow(batch)
head = [dict(zip(sch.names, vals)) for vals in zip(*[cols[name][:WIN].tolist() for name in sch.names])]
lines, results = [], {}
for name, node, t, read, wrote, rule in plans:
    proj = gandiva.make_projector(sch, [b.make_expression(node, pa.field("o", t))], None)
    ms, outs = timed(lambda: proj.evaluate_device(db))
    got = outs[0].to_arrow().slice(0, WIN)
    got = got.to_pylist() if t in (F64, I32) else got.view(I64).to_pylist()
    assert got == [rule(r) for r in head], name
    gbs = n * (read + wrote) / ms / 1e6
    results[name] = {"ms": round(ms, 4), "bytes_per_row": read + wrote, "GB_per_s": round(gbs, 1)}
    lines.append(f"{name}: {ms:.3f} ms per Evaluate, {read + wrote} B/row moved, {gbs:.0f} GB/s")
    print(lines[-1], flush=True)
    del outs, proj
for name, neighbour in (("months_between", "timestampdiffMonth"), ("next_day", "date_trunc_Week"), ("add_months", "timestampaddMonth")):
    results[name]["vs_" + neighbour] = round(results[name]["ms"] / results[neighbour]["ms"], 2)
    lines.append(f"{name} against {neighbour}: {results[name]['vs_' + neighbour]:.2f}x")
    print(lines[-1])
lines.append(json.dumps({"rows": n, "steps": steps, "warmup": WARMUP, "rows_checked": WIN, "device": torch.cuda.get_device_name(0), "results": results}))
print(lines[-1])
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("# tools/calendar_tail_timing.py %d %d: device time per Evaluate (HIP events around evaluate_device, median of the steps)\n" % (n, steps))
        f.write("\n".join(lines) + "\n")
