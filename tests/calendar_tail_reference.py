"""An independent reference for the calendar tail — months_between, next_day, add_months, date_trunc('unit', t) and the
extractor names year month day dayofmonth dayofyear dayofweek quarter hour minute second — on full-range operands.  Python
integers and floats only; the exact calendar (civil, last_dom, add_months, date_trunc, extract), the 4099-row batches, their
edge rows and the left-out rule are those of tests/temporal_reference.py, which shares no code with the product.

A result is None ("left out") only where the exact result leaves int64: next_day within 7 days of INT64_MAX, add_months by
timestampaddMonth's rule, date_trunc by date_trunc_<Unit>'s.  Nothing is left out for months_between and the extractor
names.  A float64 result is compared bit for bit: every step of the rule is one IEEE double operation.

The module has the interface tests/full_range_child.py expects (family_specs, expected_columns, left_out_columns,
build_expressions, SCHEMA, batch) and one further pass of its own: selection vectors (child_extra_passes)."""
import functools

import numpy as np
import pyarrow as pa

import temporal_reference as T
from helpers import assert_bit_exact_where, validity_np
from temporal_reference import COLUMNS, MAX_LEFT_OUT, MS, SCHEMA, batch  # noqa: F401

FAMILIES = ["months_between", "next_day", "add_months", "aliases_and_units"]
TYPES = dict(T.TYPES, str=pa.string())
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1

# 1 = Sunday ... 7 = Saturday (extractDow's numbering); every accepted spelling of a day
DAY_NAMES = {1: ("SU", "SUN", "SUNDAY"), 2: ("MO", "MON", "MONDAY"), 3: ("TU", "TUE", "TUESDAY"), 4: ("WE", "WED", "WEDNESDAY"),
             5: ("TH", "THU", "THURSDAY"), 6: ("FR", "FRI", "FRIDAY"), 7: ("SA", "SAT", "SATURDAY")}
DAY_NUMBER = {name: n for n, names in DAY_NAMES.items() for name in names}
UNITS = [u.lower() for u in T.TRUNC_UNITS]
ALIASES = {"year": "extractYear", "month": "extractMonth", "day": "extractDay", "dayofmonth": "extractDay", "dayofyear": "extractDoy",
           "dayofweek": "extractDow", "quarter": "extractQuarter", "hour": "extractHour", "minute": "extractMinute", "second": "extractSecond"}
TIME_ALIASES = ("hour", "minute", "second")
DOW_EDGES = [3, 1, 7, 0, 8, -1, -6, -7, 14, I32_MAX, I32_MIN]


def _mixed_case(s, k):
    """`s` with the letters at positions i where bit (i + k) % 3 == 0 in lower case, the others in upper case"""
    return "".join(c.lower() if (i + k) % 3 == 0 else c.upper() for i, c in enumerate(s))


# ---- the rules -----------------------------------------------------------------------------------------------------------
def months_between(e, s):
    (eday, te), (sday, ts) = divmod(e, MS), divmod(s, MS)
    ye, me, de, _ = T.civil(eday)
    ys, ms, ds, _ = T.civil(sday)
    n = (ye - ys) * 12 + (me - ms)
    if de == ds or (de == T.last_dom(ye, me) and ds == T.last_dom(ys, ms)):
        return float(n)
    return float(n) + (float(de - ds) + float(te - ts) / 86400000.0) / 31.0


def next_day(v, dow):
    day = v // MS
    want = (dow - 1) % 7 + 1
    cur = T.civil(day)[3].isoweekday() % 7 + 1
    r = (day + ((want - cur) % 7 or 7)) * MS
    return r if T._in64(r) else None


def add_months(v, n):
    return T.add_months(v, n)


def row_function(sp, tns):
    fn = sp["fn"]
    if fn == "months_between":
        return months_between
    if fn == "next_day":
        return (lambda v, name: next_day(v, DAY_NUMBER[name.upper()])) if tns[1] == "str" else next_day
    if fn == "add_months":
        return add_months
    if fn == "date_trunc":
        return lambda unit, v: T.date_trunc(unit.capitalize(), v)
    return T.row_function(ALIASES[fn], tns)


# ---- the cases -----------------------------------------------------------------------------------------------------------
def _lit(v, tn):
    return {"lit": v, "type": tn}


def _spec(fn, args, ret, symbol, host_args=None):
    """An expression: `args` are column names or literals.  `symbol` is the device function that computes it and
    `host_args` its arguments where they differ from `args` (a day name resolved, a unit dropped)."""
    label = "%s(%s)" % (fn, ",".join(a if isinstance(a, str) else repr(a["lit"]) for a in args))
    return {"label": label, "fn": fn, "args": list(args), "ret": ret, "tier0": True, "ulps": None,
            "host": {"symbol": symbol, "args": list(args if host_args is None else host_args)}}


def arg_type(a):
    return dict(COLUMNS)[a] if isinstance(a, str) else a["type"]


@functools.lru_cache(maxsize=None)
def family_specs(family):
    s = []
    for tn in ("d64", "ts"):
        name = T.TYPE_NAMES[tn]
        a, b = tn + "_a", tn + "_b"
        if family == "months_between":
            sym = "months_between_%s_%s" % (name, name)
            s += [_spec("months_between", [a, b], "f64", sym), _spec("months_between", [b, a], "f64", sym), _spec("months_between", [a, a], "f64", sym)]
        elif family == "next_day":
            sym = "next_day_%s_int32" % name
            s += [_spec("next_day", [a, "c_i32"], "d64", sym), _spec("next_day", [a, "s_i32"], "d64", sym), _spec("next_day", [b, "s_i32"], "d64", sym)]
            s += [_spec("next_day", [b, _lit(d, "i32")], "d64", sym) for d in DOW_EDGES]
            k = 0
            for n, names in DAY_NAMES.items():      # each accepted name once per type, in a letter case of its own
                for form in names:
                    k += 1
                    s.append(_spec("next_day", [a if k % 2 else b, _lit(_mixed_case(form, k), "str")], "d64", sym, [a if k % 2 else b, _lit(n, "i32")]))
        elif family == "add_months":
            for cn in ("i32", "i64"):
                sym = "add_months_%s_%s" % (name, T.TYPE_NAMES[cn])
                s.append(_spec("add_months", [a, "c_" + cn], tn, sym))
                s += [_spec("add_months", [b, _lit(c, cn)], tn, sym) for c in T.COUNT_EDGES]
        elif family == "aliases_and_units":
            for k, u in enumerate(UNITS):
                col = a if k % 2 else b
                s.append(_spec("date_trunc", [_lit(_mixed_case(u, k), "str"), col], tn, "date_trunc_%s_%s" % (u.capitalize(), name), [col]))
        else:
            raise KeyError(family)
    if family == "aliases_and_units":
        for tn in ("d32", "d64", "ts", "t32"):
            for alias, target in ALIASES.items():
                if tn != "t32" or alias in TIME_ALIASES:
                    s.append(_spec(alias, [tn + "_a"], "i64", "%s_%s" % (target, T.TYPE_NAMES[tn])))
    return s


def expected_of(sp, b):
    """(expected pyarrow array, left-out bool numpy array) of one spec over a batch: NULL where an argument is NULL; a row
    that is left out holds 0 and is compared for validity only."""
    n = b.num_rows
    tns = [arg_type(a) for a in sp["args"]]
    vals = [T.column_values(b.column(a), tn) if isinstance(a, str) else [a["lit"]] * n for a, tn in zip(sp["args"], tns)]
    valid = np.logical_and.reduce([validity_np(b.column(a)) for a in sp["args"] if isinstance(a, str)])
    f = row_function(sp, tns)
    res = [f(*row) for row in zip(*vals)]
    left_out = np.array([r is None for r in res]) & valid
    out = np.array([0 if r is None else r for r in res], dtype=np.dtype(T.STORAGE[sp["ret"]].to_pandas_dtype()))
    share = left_out.sum() / max(valid.sum(), 1)
    assert share <= MAX_LEFT_OUT, "%s leaves out %.1f %% of its valid rows" % (sp["label"], 100 * share)
    return pa.array(out, T.STORAGE[sp["ret"]], mask=~valid).view(TYPES[sp["ret"]]), left_out


@functools.lru_cache(maxsize=None)
def expected_pairs(family, nulls):
    """(expected, left out) for every expression of a family over batch(nulls): computed once, shared, never changed."""
    b = batch(nulls)
    return [expected_of(sp, b) for sp in family_specs(family)]


def expected_columns(family, nulls):
    return [e for e, _ in expected_pairs(family, nulls)]


def left_out_columns(family, nulls):
    return [x for _, x in expected_pairs(family, nulls)]


def build_expressions(gandiva, specs):
    """gandiva expressions for a list of specs, over SCHEMA."""
    b = gandiva.TreeExprBuilder()
    out = []
    for i, sp in enumerate(specs):
        args = [b.make_field(SCHEMA.field(a)) if isinstance(a, str) else b.make_literal(a["lit"], TYPES[a["type"]]) for a in sp["args"]]
        out.append(b.make_expression(b.make_function(sp["fn"], args, TYPES[sp["ret"]]), pa.field("r%d" % i, TYPES[sp["ret"]])))
    return out


# ---- the child's further pass: every projector once more behind a selection vector ----------------------------------------
def child_extra_passes(gandiva, case, exprs, groups, projs, failures):
    """Selection mode: rows 0, 1, 37, 63, 64, 65, the last and every 41st of the whole batches through projectors made
    with a UINT16 selection vector, against the same rows of the expected columns."""
    import os
    from gandiva_amd import _capi, gandiva as gg
    lib, interpreted = _capi.lib(), os.environ.get("GDV_FORCE_TIER0") is not None
    specs = case["specs"]
    evaluations = 0
    for nulls, path in case["files"]:
        table = pa.ipc.open_file(path).read_all().combine_chunks()
        rows = np.array(sorted({0, 1, 37, 63, 64, 65, len(table) - 1} | set(range(2, len(table), 41))), dtype=np.uint16)
        full = pa.RecordBatch.from_arrays([table.column(n).chunk(0) for n in SCHEMA.names], schema=SCHEMA)
        sel = gg.SelectionVector(1, rows, len(rows))
        for group in groups:
            proj = gandiva.make_projector(SCHEMA, [exprs[i] for i in group], pa.default_memory_pool(), "UINT16")
            before = lib.gdv_tier0_launches()
            got = proj.evaluate(full, sel)
            evaluations += 1
            assert lib.gdv_tier0_launches() - before == (1 if interpreted else 0), "the selection pass took the other path"
            for i, g in zip(group, got):
                col = specs[i]["column"]
                want = table.column("e%d" % col).chunk(0).take(pa.array(rows))
                keep = np.ones(len(rows), dtype=bool)
                if "x%d" % col in table.column_names:
                    keep = ~np.asarray(table.column("x%d" % col).chunk(0).take(pa.array(rows)))
                try:
                    assert_bit_exact_where(g, want, keep, "%s nulls=%s behind a selection vector" % (specs[i]["label"], nulls))
                except AssertionError as e:
                    failures.append(str(e))
    return evaluations
