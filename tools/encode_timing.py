"""Device time per Evaluate of hex / base64 / unhex / unbase64 / crc32 on C5's column (utf8, lengths 4..20, letters only),
HBM-resident inputs and outputs: HIP events around evaluate_device, 5 warm-up calls, median of 30 steps (and their min / max:
the run-to-run spread).  Prints, per plan, ms, algorithmic bytes (each input byte read once, each output byte written
once), the fraction of 8 TB/s and the ratio to the identity projection of the same rows.  Comparators from code these
functions do not touch, in the same run: repeat(s, 2) (reads and writes exactly the bytes hex(s) does), hash32(s) (one
var-len column in, one fixed-width column out, like crc32(s)) and hashMD5(s).  Outputs that would pass the 2 GiB of one var-len
column at the full row count (hex, repeat, hashMD5: 2 x or 32 bytes a row) run on the first half of the column, and their
ratios are to the identity projection of that half (a/2); unhex / unbase64 run over the hex / base64 text of that half,
produced on the device.  Two windows of every output but hash32's are checked against the restatement of tests/test_encode_cpu.py.
Usage: python tools/encode_timing.py [rows=10^8] [steps=30]"""
import hashlib
import json
import os
import sys
import zlib

import numpy as np
import pyarrow as pa
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import gandiva_amd as gandiva  # noqa: E402
from gandiva_amd import workloads as W  # noqa: E402
import test_encode_cpu as R  # noqa: E402
import test_string_tail_cpu as RT  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
WARMUP, WIN = 5, 20_000
full = W.c5_device_batch(n)
sch = W.c5_schema()
STR, BIN, I32, I64 = pa.string(), pa.binary(), pa.int32(), pa.int64()
half = gandiva.DeviceBatch(sch, full.columns, n // 2)


def rows(off_t, data_t, lo, cnt):
    off = off_t[lo: lo + cnt + 1].cpu().numpy().astype(np.int64)
    raw = data_t[int(off[0]): int(off[-1])].cpu().numpy().tobytes()
    return [raw[off[i] - off[0]: off[i + 1] - off[0]] for i in range(cnt)]


def offsets_of(col, m):
    return col.offsets[: 4 * (m + 1)].view(torch.int32)


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


def run(key, name, db, schema, fname, typ, ref, args=None):
    """one projection `fname(column 0 [, args])` (fname None: the column itself) over db; returns its output column"""
    b = gandiva.TreeExprBuilder()
    s = b.make_field(schema.field(0))
    node = s if fname is None else b.make_function(fname, [s] + [b.make_literal(v, t) for v, t in (args or [])], typ)
    proj = gandiva.make_projector(schema, [b.make_expression(node, pa.field("o", typ))], None)
    ms, lo_ms, hi_ms, outs = timed(lambda: proj.evaluate_device(db))
    m, o, col = db.num_rows, outs[0], db.columns[0]
    in_off = offsets_of(col, m)
    varlen = typ in (STR, BIN)
    for lo in (0, m - WIN) if ref is not None else ():
        want = [ref(t) for t in rows(in_off, col.data, lo, WIN)]
        if varlen:
            got = rows(offsets_of(o, m), o.data, lo, WIN)
        else:
            width = 8 if typ == I64 else 4
            got = o.data[width * lo: width * (lo + WIN)].view(torch.int64 if typ == I64 else torch.int32).cpu().numpy().tolist()
        assert got == want, f"{name}: window {lo}"
    out_bytes = 4 * (m + 1) + int(offsets_of(o, m)[m].item()) if varlen else (8 if typ == I64 else 4) * m
    algo = 4 * (m + 1) + int(in_off[m].item()) + out_bytes
    results[key] = {"plan": name, "rows": m, "ms": round(ms, 4), "min_ms": round(lo_ms, 4), "max_ms": round(hi_ms, 4),
                    "algorithmic_bytes": algo, "fraction_of_8TBps": round(algo / (ms * 1e-3) / 8e12, 4)}
    torch.cuda.synchronize()
    return o


def as_batch(col, typ, m, name):
    schema = pa.schema([pa.field(name, typ)])
    return gandiva.DeviceBatch(schema, [gandiva.DeviceColumn(typ, m, None, col.data, col.offsets)], m), schema


results = {}
h = n // 2
run("a", "identity s", full, sch, None, STR, lambda t: t)
run("a/2", "identity s, first half of the rows", half, sch, None, STR, lambda t: t)
hexed = run("hex", "hex(s), first half of the rows", half, sch, "hex", STR, R.hex_of)
run("repeat", "repeat(s, 2), first half of the rows", half, sch, "repeat", STR, lambda t: RT.repeat(t, 2), [(2, I32)])
b64 = run("base64", "base64(s), first half of the rows", half, sch, "base64", STR, R.base64_of)
hb, hs = as_batch(hexed, STR, h, "h")
run("unhex", "unhex(h), h = hex of the first half", hb, hs, "unhex", BIN, R.unhex_of)
bb, bs = as_batch(b64, STR, h, "e")
run("unbase64", "unbase64(e), e = base64 of the first half", bb, bs, "unbase64", BIN, R.unbase64_of)
del hexed, b64, hb, bb
run("crc32", "crc32(s)", full, sch, "crc32", I64, zlib.crc32)
run("hash32", "hash32(s) (checked by the suite, not here)", full, sch, "hash32", I32, None)
run("md5", "hashMD5(s), first half of the rows", half, sch, "hashMD5", STR, lambda t: hashlib.md5(t).hexdigest().encode())

BASE = {"a": "a", "crc32": "a", "hash32": "a"}
for key, r in results.items():
    base = BASE.get(key, "a/2")
    r["ratio_to"] = base
    r["ratio"] = round(r["ms"] / results[base]["ms"], 3)
    print(f"({key}) {r['plan']}: {r['rows']} rows, {r['ms']:.3f} ms (min {r['min_ms']:.3f}, max {r['max_ms']:.3f}), "
          f"{r['algorithmic_bytes'] / 1e9:.2f} GB algorithmic, {100 * r['fraction_of_8TBps']:.1f} % of 8 TB/s, {r['ratio']:.2f}x ({base})")
print(f"hex(s) / repeat(s, 2): {results['hex']['ms'] / results['repeat']['ms']:.3f}   crc32(s) / hash32(s): "
      f"{results['crc32']['ms'] / results['hash32']['ms']:.3f}")
print(json.dumps({"rows": n, "steps": steps, "warmup": WARMUP, "windows_checked": "first and last 20000 rows of each plan", "window_rows": WIN,
                  "device": torch.cuda.get_device_name(0), "results": results}))
