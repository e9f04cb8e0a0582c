"""Device time per Evaluate of the text <-> date / time casts, HBM-resident inputs and outputs: HIP events around
evaluate_device, 5 warm-up calls, median of 30 steps.  Columns: ts (timestamp(ms), uniform over 1900..2100, so a quarter
of the instants is negative), its canonical text "yyyy-MM-dd hh:mm:ss.sss" (23 bytes a row, made by castVARCHAR(ts, 23)
itself and checked), the same text with the 'T' separator in 10 % of the rows (not canonical: the byte scanner), and the
10-byte text of the dates.  Prints, per plan, ms, algorithmic bytes (each input byte read once, each output byte written
once), the fraction of 8 TB/s and the ratio to its yardstick: (b)-(d) to the identity projection of the 23-byte text (a),
(e) castVARCHAR(ts, 23) to castVARCHAR(int64, 20) over the same 8-byte values (f).  Two windows of every output are checked
against the restatement of tests/test_temporal_text_cpu.py.  9 * 10^7 rows by default: 10^8 rows of 23-byte text would
exceed the 2 GiB one utf8 column addresses.  Usage: python tools/temporal_text_timing.py [rows=9*10^7] [steps=30]"""
import json
import os
import sys

import numpy as np
import pyarrow as pa
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import gandiva_amd as gandiva  # noqa: E402
import test_temporal_text_cpu as R  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 90_000_000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
WARMUP, WIN = 5, 20_000
STR, I64, TS, D64 = pa.string(), pa.int64(), R.TS, R.D64
DAY = R.DAY


def pad(t):
    return torch.cat([t, torch.zeros((-t.numel()) % 64 + 64, dtype=torch.uint8, device=t.device)])


def fixed(typ, values):
    return gandiva.DeviceColumn(typ, n, None, pad(values.view(torch.uint8)))


def text(col):
    """a var-len output as an input column (its buffers padded like an uploaded one)"""
    m = col.length
    return gandiva.DeviceColumn(STR, m, None, pad(col.data[: col.data_used]), pad(col.offsets[: 4 * (m + 1)]))


def rows(c, lo, cnt):
    off = c.offsets[4 * lo: 4 * (lo + cnt + 1)].view(torch.int32).cpu().numpy().astype(np.int64)
    raw = c.data[int(off[0]): int(off[-1])].cpu().numpy().tobytes()
    return [raw[off[i] - off[0]: off[i + 1] - off[0]] for i in range(cnt)]


def values(c, lo, cnt, width=8):
    return c.data[width * lo: width * (lo + cnt)].view(torch.int64 if width == 8 else torch.int32).cpu().tolist()


g = torch.Generator(device="cuda")
g.manual_seed(41)
lo_ms, hi_ms = R.days_of(1900, 1, 1) * DAY, R.days_of(2100, 12, 31) * DAY + DAY
ts = torch.randint(lo_ms, hi_ms, (n,), generator=g, device="cuda", dtype=torch.int64)
d64 = torch.div(ts, DAY, rounding_mode="floor") * DAY
base_sch = pa.schema([pa.field("ts", TS), pa.field("d", D64), pa.field("v", I64)])
base = gandiva.DeviceBatch(base_sch, [fixed(TS, ts), fixed(D64, d64), fixed(I64, ts)], n)
b = gandiva.TreeExprBuilder()
f = {x.name: b.make_field(x) for x in base_sch}
lit = lambda v: b.make_literal(v, I64)  # noqa: E731
cv = lambda x, k: b.make_function("castVARCHAR", [x, lit(k)], STR)  # noqa: E731
mk = gandiva.make_projector(base_sch, [b.make_expression(cv(f["ts"], 23), pa.field("s", STR)),
                                       b.make_expression(cv(f["d"], 10), pa.field("d", STR))], None)
s_out, d_out = mk.evaluate_device(base)
s_col, d_col = text(s_out), text(d_out)
assert s_out.data_used == 23 * n and d_out.data_used == 10 * n
# 10 % of the rows with 'T' instead of ' ' at byte 10: not canonical
mixed = s_col.data.clone()
pick = torch.nonzero(torch.rand(n, generator=g, device="cuda") < 0.1).flatten()
mixed[pick * 23 + 10] = ord("T")
m_col = gandiva.DeviceColumn(STR, n, None, mixed, s_col.offsets)
text_sch = pa.schema([pa.field("s", STR), pa.field("m", STR), pa.field("d", STR)])
texts = gandiva.DeviceBatch(text_sch, [s_col, m_col, d_col], n)
tf = {x.name: b.make_field(x) for x in text_sch}

PLANS = {  # key: (plan, batch, node, output type, expected(window lo))
    "a": ("identity s (23-byte timestamp text)", texts, tf["s"], STR, lambda lo: rows(s_col, lo, WIN)),
    "b": ("castTIMESTAMP(s)", texts, b.make_function("castTIMESTAMP", [tf["s"]], TS), TS,
          lambda lo: [R.cast_timestamp(x) for x in rows(s_col, lo, WIN)]),
    "c": ("castTIMESTAMP(m), 10 % of the rows with 'T'", texts, b.make_function("castTIMESTAMP", [tf["m"]], TS), TS,
          lambda lo: [R.cast_timestamp(x) for x in rows(m_col, lo, WIN)]),
    "d": ("castDATE(d) (10-byte date text)", texts, b.make_function("castDATE", [tf["d"]], D64), D64,
          lambda lo: [R.cast_date(x) for x in rows(d_col, lo, WIN)]),
    "e": ("castVARCHAR(ts, 23)", base, cv(f["ts"], 23), STR, lambda lo: [R.cast_varchar(v, 0, 23) for v in values(base.columns[0], lo, WIN)]),
    "f": ("castVARCHAR(int64, 20)", base, cv(f["v"], 20), STR, lambda lo: [str(v).encode() for v in values(base.columns[2], lo, WIN)]),
}
BASE = {"a": "a", "b": "a", "c": "a", "d": "a", "e": "f", "f": "f"}


def timed(call):
    for _ in range(WARMUP):
        out = call()
    torch.cuda.synchronize()
    ts_ = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = call()
        e1.record()
        torch.cuda.synchronize()
        ts_.append(e0.elapsed_time(e1))
    return float(np.median(ts_)), out


results = {}
for key, (name, db, node, typ, want) in PLANS.items():
    proj = gandiva.make_projector(db.schema, [b.make_expression(node, pa.field("o", typ))], None)
    ms, outs = timed(lambda: proj.evaluate_device(db))
    o = outs[0]
    for lo in (0, n - WIN):
        got = rows(o, lo, WIN) if typ == STR else values(o, lo, WIN)
        assert got == want(lo), f"{name}: window {lo}"
    in_bytes = {"a": 4 * (n + 1) + 23 * n, "b": 4 * (n + 1) + 23 * n, "c": 4 * (n + 1) + 23 * n, "d": 4 * (n + 1) + 10 * n}.get(key, 8 * n)
    out_bytes = (o.data_used + 4 * (n + 1)) if typ == STR else 8 * n
    algo = in_bytes + out_bytes
    results[key] = {"plan": name, "rows": n, "ms": round(ms, 4), "algorithmic_bytes": algo,
                    "fraction_of_8TBps": round(algo / (ms * 1e-3) / 8e12, 4)}
    del outs, o
    torch.cuda.synchronize()

for key, r in results.items():
    r["ratio_to"] = BASE[key]
    r["ratio"] = round(r["ms"] / results[BASE[key]]["ms"], 3)
    print(f"({key}) {r['plan']}: {r['rows']} rows, {r['ms']:.3f} ms, {r['algorithmic_bytes'] / 1e9:.2f} GB algorithmic, "
          f"{100 * r['fraction_of_8TBps']:.1f} % of 8 TB/s, {r['ratio']:.2f}x ({BASE[key]})")
print(json.dumps({"rows": n, "steps": steps, "warmup": WARMUP, "windows_checked": "first and last 20000 rows of each plan",
                  "window_rows": WIN, "device": torch.cuda.get_device_name(0), "results": results}))
