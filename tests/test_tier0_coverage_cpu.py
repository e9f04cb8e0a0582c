"""Tier 0 covers the fixed-width registry: every signature whose parameters and result are fixed-width and not decimal,
that cannot raise and is not a hash, has a program for the interpreter kernel (gandiva_amd/csrc/gdv_tier0.*) — in row
mode and, for projectors, in selection mode.  No GPU: the programs are built and read as text."""
import ctypes as C

import pyarrow as pa

import gandiva_amd as gandiva
from gandiva_amd import _capi, gandiva as gg
from gandiva_amd._capi import gdv_type_t

HASHES = {"hash", "hash32", "hash64", "hash32AsDouble", "hash64AsDouble"}
NUMERIC = [pa.int8(), pa.int16(), pa.int32(), pa.int64(), pa.uint8(), pa.uint16(), pa.uint32(), pa.uint64(), pa.float32(), pa.float64()]
# the signatures that can raise: outside tier 0 by design
RAISING = {("divide", (t, t)) for t in NUMERIC} | {("mod", (pa.float64(), pa.float64())), ("modulo", (pa.float64(), pa.float64())),
                                                   ("log", (pa.float64(), pa.float64()))}
MAX_LITS = 92   # tier0::kMaxLits


def _text(call):
    lib = _capi.lib()
    p = call(lib)
    if not p:
        return None, _capi.last_error()
    text = C.string_at(p).decode()
    lib.gdv_free_string(p)
    return text.splitlines(), None


def _program(schema, exprs, is_condition=0):
    sh = gg._make_schema(schema)
    try:
        arr = (C.c_void_p * len(exprs))(*[e._h for e in exprs])
        return _text(lambda lib: lib.gdv_tier0_program(sh, arr, len(exprs), is_condition))
    finally:
        _capi.lib().gdv_schema_free(sh)


def _program_selection(schema, exprs, mode):
    sh = gg._make_schema(schema)
    try:
        arr = (C.c_void_p * len(exprs))(*[e._h for e in exprs])
        return _text(lambda lib: lib.gdv_tier0_program_selection(sh, arr, len(exprs), mode))
    finally:
        _capi.lib().gdv_schema_free(sh)


def _fixed(t):
    return (pa.types.is_boolean(t) or pa.types.is_integer(t) or pa.types.is_floating(t) or pa.types.is_date(t) or
            pa.types.is_timestamp(t) or pa.types.is_time(t))


def _kind(t):
    """how the program text names a type: its storage"""
    if pa.types.is_boolean(t):
        return "bool"
    if pa.types.is_date32(t) or pa.types.is_time32(t):
        return "int32"
    if pa.types.is_date64(t) or pa.types.is_timestamp(t) or pa.types.is_time64(t):
        return "int64"
    return {"float": "float32", "double": "float64"}.get(str(t), str(t))


def _registry():
    """(name, return type, parameter types) of every registered signature, through the C ABI"""
    lib = _capi.lib()
    out = []
    for i in range(lib.gdv_registry_size()):
        name, ret, params, n = C.c_char_p(), gdv_type_t(), (gdv_type_t * 8)(), C.c_int()
        assert lib.gdv_registry_get(i, C.byref(name), C.byref(ret), params, 8, C.byref(n)) == 0
        out.append((name.value.decode(), gg.from_gdv_type(ret), tuple(gg.from_gdv_type(params[j]) for j in range(n.value))))
    return out


def test_every_fixed_width_signature_that_cannot_raise_and_is_no_hash_has_a_program():
    b = gandiva.TreeExprBuilder()
    covered, missing = 0, []
    for name, ret, params in _registry():
        if not (_fixed(ret) and all(_fixed(p) for p in params)) or name in HASHES or (name, params) in RAISING:
            continue
        schema = pa.schema([(f"c{i}", p) for i, p in enumerate(params)])
        call = b.make_function(name, [b.make_field(schema.field(i)) for i in range(len(params))], ret)
        prog, why = _program(schema, [b.make_expression(call, pa.field("r", ret))])
        sig = f"{name}({', '.join(map(str, params))})"
        if prog is None:
            missing.append(f"{sig}: {why}")
            continue
        assert prog[-1] == f"out0 {_kind(ret)}", (sig, prog)
        loads = [p for p in prog if p.startswith("load in")]
        assert len(loads) == len(params), (sig, prog)
        for i, p in enumerate(params):
            assert loads[i].startswith(f"load in{i} {_kind(p)}"), (sig, prog)
        assert len(prog) == len(params) + 2, (sig, prog)     # loads, ONE instruction for the call, the output
        covered += 1
    assert not missing, "\n".join(missing)
    assert covered > 150, covered


SCHEMA = pa.schema([("a", pa.int32()), ("x", pa.float64()), ("f", pa.bool_()), ("d", pa.date64()), ("ts", pa.timestamp("ms")),
                    ("u", pa.uint16()), ("i8", pa.int8()), ("l", pa.int64())])


def _fields(b):
    return [b.make_field(SCHEMA.field(i)) for i in range(len(SCHEMA))]


def _one(b, node, t):
    return [b.make_expression(node, pa.field("r", t))]


def test_program_text_of_one_tree_per_new_kind_of_instruction():
    b = gandiva.TreeExprBuilder()
    a, x, f, d, ts, u, i8, l = _fields(b)
    i32, i64, f64, bl = pa.int32(), pa.int64(), pa.float64(), pa.bool_()
    prog, _ = _program(SCHEMA, _one(b, b.make_function("extractYear", [ts], i64), i64))                     # a unary call
    assert prog == ["load in0 int64", "call extractYear_timestamp", "out0 int64"]
    prog, _ = _program(SCHEMA, _one(b, b.make_function("timestampaddMonth", [l, ts], pa.timestamp("ms")), pa.timestamp("ms")))  # a binary call
    assert prog == ["load in0 int64", "load in1 int64", "call timestampaddMonth_int64_timestamp", "out0 int64"]
    prog, _ = _program(SCHEMA, _one(b, b.make_function("negative", [x], f64), f64))                         # type-generic, one operand
    assert prog == ["load in0 float64", "negative float64", "out0 float64"]
    prog, _ = _program(SCHEMA, _one(b, b.make_function("bitwise_xor", [a, b.make_literal(0x0f0f, i32)], i32), i32))
    assert prog == ["load in0 int32", "lit #0 = 0xf0f", "bitwise_xor int32", "out0 int32"]
    prog, _ = _program(SCHEMA, _one(b, b.make_function("nvl", [i8, b.make_literal(-1, pa.int8())], pa.int8()), pa.int8()))
    assert prog == ["load in0 int8", "lit #0 = 0xffffffffffffffff", "nvl int8", "out0 int8"]
    prog, _ = _program(SCHEMA, _one(b, b.make_function("is_distinct_from", [x, b.make_null(f64)], bl), bl))
    assert prog == ["load in0 float64", "lit #0 null", "is_distinct_from float64", "out0 bool"]
    prog, _ = _program(SCHEMA, _one(b, b.make_function("is_not_distinct_from", [u, u], bl), bl))
    assert prog == ["load in0 uint16", "load in0 uint16", "is_not_distinct_from uint16", "out0 bool"]
    prog, _ = _program(SCHEMA, _one(b, b.make_function("isnotfalse", [f], bl), bl))
    assert prog == ["load in0 bool", "isnotfalse", "out0 bool"]
    # IN: one instruction over a run of literal slots (the values' bit images, sorted, duplicates dropped)
    prog, _ = _program(SCHEMA, [b.make_condition(b.make_in_expression(a, [7, -2, 7, 3], i32))], 1)
    assert prog == ["load in0 int32", "in int32 #0..#2", "filter"]
    prog, _ = _program(SCHEMA, _one(b, b.make_and([b.make_function("greater_than", [l, b.make_literal(5, i64)], bl),
                                                  b.make_in_expression(d, [86400000, 0], pa.date64())]), bl))
    assert prog == ["load in0 int64", "lit #0 = 0x5", "compare gt int64", "load in1 int64", "in int64 #1..#2", "and", "out0 bool"]


def test_an_alias_and_its_target_give_the_same_program():
    b = gandiva.TreeExprBuilder()
    a, x, f, d, ts, u, i8, l = _fields(b)
    i32, i64, f64, bl = pa.int32(), pa.int64(), pa.float64(), pa.bool_()
    for alias, target, args, t in (("pow", "power", [x, x], f64), ("modulo", "mod", [l, a], i32), ("weekofyear", "extractWeek", [ts], i64),
                                   ("date_diff", "datediff", [d, d], i32), ("eq", "equal", [u, u], bl), ("same", "equal", [x, x], bl),
                                   ("isnumeric", "isnotnull", [x], bl)):
        p1, w1 = _program(SCHEMA, _one(b, b.make_function(alias, args, t), t))
        p2, w2 = _program(SCHEMA, _one(b, b.make_function(target, args, t), t))
        assert p1 is not None and p1 == p2, (alias, p1, w1, p2, w2)
    prog, _ = _program(SCHEMA, _one(b, b.make_function("pow", [x, x], f64), f64))
    assert "call power_float64_float64" in prog


def test_program_of_a_selection_mode_projector():
    b = gandiva.TreeExprBuilder()
    a, x, f, d, ts, u, i8, l = _fields(b)
    exprs = [b.make_expression(b.make_function("date_trunc_Month", [ts], pa.timestamp("ms")), pa.field("m", pa.timestamp("ms"))),
             b.make_expression(b.make_function("nvl", [u, b.make_literal(9, pa.uint16())], pa.uint16()), pa.field("n", pa.uint16())),
             b.make_expression(b.make_and([f, b.make_function("isnotnull", [i8], pa.bool_())]), pa.field("g", pa.bool_()))]
    body = ["load in0 int64", "call date_trunc_Month_timestamp", "out0 int64", "load in1 uint16", "lit #0 = 0x9", "nvl uint16",
            "out1 uint16", "load in2 bool", "load in3 int8", "isnotnull", "and", "out2 bool"]
    for mode, width in ((1, 16), (2, 32), (3, 64)):
        prog, why = _program_selection(SCHEMA, exprs, mode)
        assert prog == [f"select uint{width}"] + body, (prog, why)
    prog, _ = _program_selection(SCHEMA, exprs, 0)            # mode 0: the row-mode program
    assert prog == body
    assert _program(SCHEMA, exprs)[0] == body
    prog, why = _program_selection(SCHEMA, exprs, 7)
    assert prog is None and "selection mode" in why


def test_an_in_list_longer_than_the_literal_table_is_refused_and_says_so():
    b = gandiva.TreeExprBuilder()
    a = _fields(b)[0]
    prog, why = _program(SCHEMA, [b.make_condition(b.make_in_expression(a, list(range(MAX_LITS)), pa.int32()))], 1)
    assert prog == ["load in0 int32", f"in int32 #0..#{MAX_LITS - 1}", "filter"], why
    prog, why = _program(SCHEMA, [b.make_condition(b.make_in_expression(a, list(range(MAX_LITS + 1)), pa.int32()))], 1)
    assert prog is None and "IN list" in why and "literal table" in why
    # the table is shared with the plan's other literals
    cond = b.make_and([b.make_function("less_than", [a, b.make_literal(1000, pa.int32())], pa.bool_()),
                       b.make_in_expression(a, list(range(MAX_LITS)), pa.int32())])
    prog, why = _program(SCHEMA, [b.make_condition(cond)], 1)
    assert prog is None and "literal table" in why


def test_what_stays_outside_is_refused_with_its_cause():
    from gandiva_amd import workloads as W
    b = gandiva.TreeExprBuilder()
    a, x, f, d, ts, u, i8, l = _fields(b)
    i32, f64 = pa.int32(), pa.float64()
    for name, args, t in (("divide", [a, a], i32), ("divide", [x, x], f64), ("mod", [x, x], f64), ("modulo", [x, x], f64),
                          ("log", [x, x], f64)):
        prog, why = _program(SCHEMA, _one(b, b.make_function(name, args, t), t))
        assert prog is None and name in why and "raise" in why, (name, why)
    for name, args, t in (("hash32", [a], i32), ("hash64", [x], pa.int64()), ("hash", [ts], i32), ("hash64AsDouble", [a, l], pa.int64())):
        prog, why = _program(SCHEMA, _one(b, b.make_function(name, args, t), t))
        assert prog is None and f"function {name} is a hash" in why, (name, why)
    prog, why = _program(W.c4_schema(), W.c4_expressions())
    assert prog is None and "decimal128" in why
    prog, why = _program(W.c5_schema(), W.c5_expressions())
    assert prog is None and "var-len" in why
    prog, why = _program_selection(W.c5_schema(), W.c5_expressions(), 2)
    assert prog is None and "var-len" in why
    deep = a
    for _ in range(14):
        deep = b.make_function("greatest", [a, deep], i32)
    prog, why = _program(SCHEMA, _one(b, deep, i32))
    assert prog is None and "stack" in why


def test_the_plan_options_outside_tier_0_are_refused_by_name(monkeypatch):
    """cast_x86_indefinite is read from the environment at every Make (CodegenOptions::FromEnv): with it set, a plan that has
    a program otherwise has none, in row mode and in selection mode, and the reason names the option.  rows_word is set
    for the second stage of a two-stage plan only, and such a plan never reaches the builder: it is refused before, as a
    plan that materialises values in a first stage."""
    b = gandiva.TreeExprBuilder()
    a, x, f, d, ts, u, i8, l = _fields(b)
    exprs = _one(b, b.make_function("castINT", [x], pa.int32()), pa.int32())
    assert _program(SCHEMA, exprs)[0] == ["load in0 float64", "cast float64 -> int32", "out0 int32"]
    monkeypatch.setenv("GDV_CAST_X86_INDEFINITE", "1")
    for prog, why in (_program(SCHEMA, exprs), _program_selection(SCHEMA, exprs, 2),
                      _program(SCHEMA, [b.make_condition(b.make_function("greater_than", [a, b.make_literal(1, pa.int32())], pa.bool_()))], 1)):
        assert prog is None and "cast_x86_indefinite" in why, why
    monkeypatch.delenv("GDV_CAST_X86_INDEFINITE")
    assert _program(SCHEMA, exprs)[0] is not None
    # a two-stage plan (upper over a concat result: the concat is materialised by a first stage)
    schema = pa.schema([("s", pa.string())])
    s = b.make_field(schema.field(0))
    two_stage = b.make_function("upper", [b.make_function("concat", [s, s], pa.string())], pa.string())
    for prog, why in (_program(schema, [b.make_expression(two_stage, pa.field("r", pa.string()))]),
                      _program_selection(schema, [b.make_expression(two_stage, pa.field("r", pa.string()))], 2)):
        assert prog is None and "first stage" in why, why
