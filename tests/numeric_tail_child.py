"""What the child processes of tests/test_numeric_tail.py import (tests/full_range_child.py: `import <module> as R`): the
reference module's cases, plus one further pass that keeps the results of the whole batches in an Arrow file next to the
case's inputs — `<batch file>.tier0` from the interpreter, `<batch file>.specialised` from the hipRTC kernels — so that
the parent can hold the two paths to each other bit for bit."""
import os

import pyarrow as pa

from numeric_tail_reference import *  # noqa: F401,F403
from numeric_tail_reference import SCHEMA


def child_extra_passes(gandiva, case, exprs, groups, projs, failures):
    suffix = ".tier0" if os.environ.get("GDV_FORCE_TIER0") is not None else ".specialised"
    evaluations = 0
    for nulls, path in case["files"]:
        table = pa.ipc.open_file(path).read_all().combine_chunks()
        batch = pa.RecordBatch.from_arrays([table.column(n).chunk(0) for n in SCHEMA.names], schema=SCHEMA)
        cols = {}
        for group, proj in zip(groups, projs):
            for i, g in zip(group, proj.evaluate(batch)):
                cols[case["specs"][i]["label"]] = g
            evaluations += 1
        out = pa.table(cols)
        with pa.ipc.new_file(path + suffix, out.schema) as w:
            w.write_table(out)
    return evaluations
