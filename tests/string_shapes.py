"""The core string functions on rows that cross every boundary of the wave-shaped string kernels: the corpus, the
expressions and an independent reference (plain Python over str / bytes; nothing here reads oracle/ or
gdv_device_lib.hpp).  tests/test_string_shapes_cpu.py holds the reference against pyarrow.compute, the oracle and the
host build of the device library against the reference, and the corpus's ladders against the thresholds of the
generated kernels; tests/test_string_shapes.py runs every group of GROUPS on the GPU.

What the kernels do depends on the shape of the rows: a 64-row sub-tile whose bytes fit the sweep's LDS mirror is
answered from match bitmaps, a longer one by the per-row search; a wave tile (64 x 4 or 64 x 8 rows) has a limit on the
span its match bitmaps cover and a limit on the bytes one LDS output window stages; the sweep moves 16 bytes per lane
and 1024 per step.  SPAN_LADDERS names every (threshold T, rows of the unit it applies to) the corpus stands on with
totals of T - 1, T and T + 1 bytes; the CPU test reads the thresholds of the kernels it generates and fails when one of
them is not in that list."""
import functools
import re

import numpy as np
import pyarrow as pa

from helpers import py_murmur3_x64_128_h1, py_murmur3_x86_32

VARIANTS = ("ascii", "multibyte")
NULLS = (0.0, 0.1)
SCHEMA = pa.schema([("s", pa.string()), ("t", pa.string()), ("b", pa.binary()), ("k", pa.int32())])
TYPES = {"bool": pa.bool_(), "i32": pa.int32(), "i64": pa.int64(), "str": pa.string(), "bin": pa.binary()}

SUB = 64                       # rows of a sub-tile
TILE = 512                     # rows of the largest wave tile (64 x 8); a run aligned to it is aligned to 64 x 4 too
LENGTH_LADDER = list(range(41)) + [55, 56, 57, 63, 64, 65, 119, 120, 127, 128, 129, 255, 256, 257] + \
    [t + d for t in (1024, 2048, 4096, 8192, 16384) for d in (-1, 0, 1)] + [65536 + 77]
# (threshold in bytes, rows of the unit): the sweep's mirror per sub-tile; the match bitmaps' span per wave tile of
# 4 / 8 sub-tiles; one output window per wave tile of 4 / 8 sub-tiles
SPAN_LADDERS = [(2048, 64), (8192, 256), (16384, 512), (2048, 256), (4096, 512)]
NEEDLES = ["k", "sp", "spark", "sparkles", "sparkling"]      # 1, 2, 5, 8 and 9 bytes


# ---- the reference: one plain function per registry function (None = NULL is handled by evaluate()) --------------------
def ascii_upper(v):
    return "".join(chr(ord(c) - 32) if "a" <= c <= "z" else c for c in v)


def ascii_lower(v):
    return "".join(chr(ord(c) + 32) if "A" <= c <= "Z" else c for c in v)


def substr(v, start, count=0x7fffffff):
    """Characters start.. (1-based; negative: from the end; 0 as 1), at most count of them; "" when out of range."""
    if count <= 0 or not v:
        return ""
    n = len(v)
    s = start - 1 if start > 0 else (n + start if start < 0 else 0)
    if s < 0 or s >= n:
        return ""
    return v[s:s + count]


def like(v, pat, escape=None):
    rx, i = [], 0
    while i < len(pat):
        c = pat[i]
        if escape and c == escape and i + 1 < len(pat):
            i += 1
            rx.append(re.escape(pat[i]))
        else:
            rx.append(".*" if c == "%" else "." if c == "_" else re.escape(c))
        i += 1
    return re.fullmatch("".join(rx), v, re.DOTALL) is not None


def left(v, k):
    return "" if k == 0 else (v[:k] if k > 0 else v[:max(len(v) + k, 0)])


def right(v, k):
    return "" if k == 0 else (v[max(len(v) - k, 0):] if k > 0 else v[min(-k, len(v)):])


def locate(sub, v, start=1):
    """1-based character position of sub in v at or after character `start`; 0 when absent or either is empty."""
    return 0 if not v or not sub else v.find(sub, start - 1) + 1


def ascii_of(v):
    return 0 if not v else int(np.int8(np.uint8(v.encode()[0])))


def pad(v, n, fill, right):
    if v is None:
        return None
    if v == "" or n <= 0:
        return ""
    if len(v) >= n or fill == "":
        return v[:n] if len(v) > n else v
    p = (fill * n)[:n - len(v)]
    return v + p if right else p + v


def initcap(t):
    """First letter of a word in upper case, the others in lower; words are runs of ASCII alphanumerics and bytes >= 0x80,
    and only ASCII letters change."""
    if t is None:
        return None

    def word(m):
        w = m.group(0)
        head = w[:1].upper() if w[0] < 0x80 else w[:1]
        return head + w[1:].lower()          # bytes.lower() / .upper() touch ASCII letters only
    return re.sub(rb"[A-Za-z0-9\x80-\xff]+", word, t.encode()).decode()


def replace(v, frm, to):
    return v.replace(frm, to) if frm else v


def _raw(v):
    return v if isinstance(v, bytes) else v.encode()


def _i32(v):
    return ((v + (1 << 31)) & 0xffffffff) - (1 << 31)


def hash32(v, seed=0):
    return _i32(seed) if v is None else py_murmur3_x86_32(_raw(v), seed)


def hash64(v, seed=0):      # the seed is narrowed to int32 and sign-extended into both lanes
    return _i32(seed) if v is None else py_murmur3_x64_128_h1(_raw(v), _i32(seed))


def python_positions(vals, subs):
    """tests/test_strings.py's _position_exprs in plain Python (str = sequence of characters)."""
    cols = []

    def col(fn):
        cols.append([None if v is None else fn(v) for v in vals])
    for k in (0, 1, 3, 100, -1, -4, -100):
        col(lambda v, k=k: left(v, k))
        col(lambda v, k=k: right(v, k))
    for k in (0, 2, 7, 1000):
        col(lambda v, k=k: v[:k])
    for sub in ("spark", "a", "é", "日本", ""):
        col(lambda v, sub=sub: locate(sub, v))
        col(lambda v, sub=sub: locate(sub, v))
    col(lambda v: locate("a", v, 3))
    cols.append([None if v is None or t is None else locate(t, v) for v, t in zip(vals, subs)])
    col(ascii_of)
    col(lambda v: ascii_of(ascii_upper(v)))
    return cols


def python_concat(ss, ts):
    """tests/test_strings.py's _concat_exprs in plain Python."""
    e = lambda v: "" if v is None else v  # noqa: E731
    return [[e(s) + e(t) for s, t in zip(ss, ts)],
            [None if s is None or t is None else s + t for s, t in zip(ss, ts)],
            [e(s) + " - " + ("" if t is None else ascii_upper(t)) for s, t in zip(ss, ts)],
            [None if s is None else s[1:4] + "|" + ascii_lower(s) for s in ss],
            [("" if s is None or t is None else s + t) + "." + e(t) + e(t) for s, t in zip(ss, ts)],
            [e(s) + e(t) + e(s) + e(t) + "日本" for s, t in zip(ss, ts)]]


REGEX = "s[a-z]a+rk|[0-9][0-9]x|^Fl"
_COMPARES = {"equal": lambda x, y: x == y, "not_equal": lambda x, y: x != y, "less_than": lambda x, y: x < y,
             "less_than_or_equal_to": lambda x, y: x <= y, "greater_than": lambda x, y: x > y,
             "greater_than_or_equal_to": lambda x, y: x >= y}
_NULL_NEVER = {"isnull": lambda v: v is None, "isnotnull": lambda v: v is not None,
               "concat": lambda *a: "".join("" if x is None else x for x in a),
               "hash": hash32, "hash32": hash32, "hash32AsDouble": hash32, "hash64": hash64, "hash64AsDouble": hash64}
_NULL_IF_NULL = {
    "like": like, "ilike": lambda v, p: like(ascii_lower(v), ascii_lower(p)),
    "regexp_like": lambda v, p: re.search(p, v) is not None, "regexp_matches": lambda v, p: re.search(p, v) is not None,
    "starts_with": lambda v, p: v.startswith(p), "ends_with": lambda v, p: v.endswith(p),
    "octet_length": lambda v: len(_raw(v)), "bit_length": lambda v: 8 * len(_raw(v)),
    "char_length": len, "length": len, "lengthUtf8": lambda v: len(v.decode()),
    "locate": locate, "position": locate, "strpos": lambda v, sub: locate(sub, v), "ascii": ascii_of,
    "substr": substr, "substring": substr, "left": left, "right": right,
    "ltrim": lambda v: v.lstrip(" "), "rtrim": lambda v: v.rstrip(" "), "btrim": lambda v: v.strip(" "), "trim": lambda v: v.strip(" "),
    "castVARCHAR": lambda v, n: v[:n], "upper": ascii_upper, "lower": ascii_lower, "initcap": initcap, "reverse": lambda v: v[::-1],
    "replace": replace, "lpad": lambda v, n, fill=" ": pad(v, n, fill, False), "rpad": lambda v, n, fill=" ": pad(v, n, fill, True),
    "concatOperator": lambda *a: "".join(a),
}
for _name, _op in _COMPARES.items():
    _NULL_IF_NULL[_name] = lambda x, y, _op=_op: _op(_raw(x), _raw(y))


def evaluate(node, row):
    """The value of a spec's tree on one row (dict column -> Python value, None = NULL), by each function's registry
    policy: isnull / isnotnull, concat and the hashes are never NULL, everything else is NULL if an argument is."""
    if isinstance(node, str):
        return row[node]
    if "lit" in node:
        return node["lit"].encode() if node["type"] == "bin" else node["lit"]
    if "if" in node:
        return evaluate(node["then"], row) if evaluate(node["if"], row) else evaluate(node["else"], row)
    if "in" in node:
        v = evaluate(node["in"], row)
        return None if v is None else v in node["values"]
    a = [evaluate(x, row) for x in node["args"]]
    f = _NULL_NEVER.get(node["fn"])
    if f is not None:
        return f(*a)
    return None if any(x is None for x in a) else _NULL_IF_NULL[node["fn"]](*a)


# ---- expressions ------------------------------------------------------------------------------------------------------
def L(v, tn="str"):
    return {"lit": v, "type": tn}


def F(fn, ret, *args):
    return {"fn": fn, "args": list(args), "ret": ret}


def _label(node):
    if isinstance(node, str):
        return node
    if "lit" in node:
        return repr(node["lit"])
    if "if" in node:
        return "if(%s,%s,%s)" % (_label(node["if"]), _label(node["then"]), _label(node["else"]))
    if "in" in node:
        return "in(%s,%r)" % (_label(node["in"]), node["values"])
    return "%s(%s)" % (node["fn"], ",".join(_label(a) for a in node["args"]))


def _fields(node, out):
    if isinstance(node, str):
        out.add(node)
    elif "if" in node:
        for x in (node["if"], node["then"], node["else"]):
            _fields(x, out)
    elif "in" in node:
        _fields(node["in"], out)
    elif "args" in node:
        for x in node["args"]:
            _fields(x, out)
    return out


def signatures_of(node, out=None):
    """(name, parameter type names) of every registry function a tree calls."""
    out = set() if out is None else out
    if isinstance(node, dict) and "if" in node:
        for x in (node["if"], node["then"], node["else"]):
            signatures_of(x, out)
    elif isinstance(node, dict) and "in" in node:
        signatures_of(node["in"], out)
    elif isinstance(node, dict) and "args" in node:
        out.add((node["fn"], tuple(_ret(a) for a in node["args"])))
        for x in node["args"]:
            signatures_of(x, out)
    return out


def _ret(node):
    if isinstance(node, str):
        return {"s": "str", "t": "str", "b": "bin", "k": "i32"}[node]
    return node["type"] if "lit" in node else "bool" if "in" in node else node["ret"]


CARRIER = F("substr", "str", "s", L(2, "i64"), L(5, "i64"))     # one var-len output keeps a group of numbers on the wave shape
I32, I64 = (lambda v: L(v, "i32")), (lambda v: L(v, "i64"))


def _predicates_like():
    out = [F("like", "bool", "s", L(p)) for p in ("%spark%", "spark%", "%spark", "%k%", "%sp%", "%sparkles%", "%sparkling%",
                                                    "s_ark%", "%a%b%", "_%_", "", "%", "%sparkles", "sparkling%")]
    out += [F("like", "bool", "s", L("100#%%"), L("#")), F("like", "bool", "s", L("%a\\_b\\%c%"), L("\\"))]
    out += [F("ilike", "bool", "s", L("%SpArK%")), F("ilike", "bool", "s", L("mixed c_se%")), F("regexp_like", "bool", "s", L(REGEX))]
    out += [F("starts_with", "bool", "s", L(n)) for n in ("spa", "sparkling")] + [F("ends_with", "bool", "s", L(n)) for n in ("k", "sparkles")]
    out += [F("starts_with", "bool", "s", "t"), F("ends_with", "bool", "s", "t")]
    return out


def _predicates_compare():
    out = []
    for name in _COMPARES:
        out += [F(name, "bool", "s", L("spark")), F(name, "bool", "s", "t"), F(name, "bool", "b", L("sparkles", "bin"))]
    out += [{"in": "s", "values": ["spark", "k", "", "sparkling", "日本語テキスト", " " * 8]}]
    out += [F(fn, "bool", c) for fn in ("isnull", "isnotnull") for c in ("s", "b")]
    return out


def _numbers_lengths():
    out = [F(fn, "i32", c) for fn in ("octet_length", "bit_length") for c in ("s", "b")]
    out += [F("char_length", "i32", "s"), F("length", "i32", "s"), F("lengthUtf8", "i32", "b"), F("ascii", "i32", "s")]
    out += [F("locate", "i32", L(n), "s") for n in NEEDLES] + [F("strpos", "i32", "s", L(n)) for n in ("sp", "sparkles")]
    out += [F("locate", "i32", L("spark"), "s", I32(k)) for k in (1, 2, 8, 9, 16, 17, 100000)]
    out += [F("position", "i32", L("sparkling"), "s"), F("position", "i32", L("k"), "s", I32(9)), F("locate", "i32", "t", "s"), F("strpos", "i32", "s", "t")]
    return out


def _numbers_hashes():
    out = []
    for c in ("s", "b"):
        out += [F("hash", "i32", c), F("hash32", "i32", c), F("hash32AsDouble", "i32", c), F("hash64", "i64", c), F("hash64AsDouble", "i64", c),
                F("hash32", "i32", c, I32(17)), F("hash32AsDouble", "i32", c, I32(-5)), F("hash64", "i64", c, I64(-1234567)), F("hash64AsDouble", "i64", c, I64(99))]
    return out


def _views():
    g1 = [F("substr", "str", "s", I64(a), I64(c)) for a, c in ((1, 1), (2, 8), (8, 9), (9, 16), (16, 17), (17, 2), (-1, 2), (-8, 8))]
    g2 = [F("substr", "str", "s", I64(a), I64(c)) for a, c in ((-9, 9), (0, 16), (100000, 2), (2, 0))] + \
         [F("substr", "str", "s", I64(a)) for a in (2, 9, -8)] + [F("substring", "str", "s", I64(9), I64(8))]
    g3 = [F("substring", "str", "s", I64(17))] + [F("left", "str", "s", I32(k)) for k in (1, 8, 9, -1)] + [F("right", "str", "s", I32(k)) for k in (1, 8, 9)]
    g4 = [F("left", "str", "s", I32(k)) for k in (16, 17, -8, 0, 100000)] + [F("right", "str", "s", I32(k)) for k in (16, -9, 100000)]
    g5 = [F(fn, "str", "s") for fn in ("ltrim", "rtrim", "btrim", "trim")] + [F("castVARCHAR", "str", "s", I64(n)) for n in (0, 8, 9, 100000)]
    g6 = [F("castVARCHAR", "str", "s", I64(n)) for n in (1, 16, 17)] + [F("left", "str", "s", "k"), F("right", "str", "s", "k"), F("right", "str", "s", I32(17))]
    return [g1, g2, g3, g4, g5, g6]


def _materialised():
    g1 = [F("initcap", "str", "s"), F("reverse", "str", "s")] + \
         [F("replace", "str", "s", L(f), L(t)) for f, t in (("k", "kkkkk"), ("sp", "SP!"), ("spark", "flink"), ("sparkles", "x"), ("sparkling", "sparkling!!"))] + \
         [F("upper", "str", F("substr", "str", "s", I64(2), I64(9)))]
    g2 = [F("lpad", "str", "s", I32(n), L(f)) for n, f in ((0, "*"), (8, "*"), (17, "abc"), (40, "12345678"))] + \
         [F("rpad", "str", "s", I32(n), L(f)) for n, f in ((1, "*"), (9, "abc"), (16, "12345678"), (300, "é日"))]
    g3 = [F("lpad", "str", "s", I32(16)), F("rpad", "str", "s", I32(17)), F("lpad", "str", "s", "k"), F("rpad", "str", "s", "k", "t"),
          F("concat", "str", "s", "t"), F("concatOperator", "str", "s", "t"), F("concat", "str", "s", L(" - "), "t"), F("concatOperator", "str", "t", L("|"), "s")]
    g4 = [F("concat", "str", "s", "t", "s", L(""), "t", L("日本")), F("concatOperator", "str", "t", L("1"), "t", L("22"), "s", L("333")),
          {"if": F("starts_with", "bool", "s", L("s")), "then": "s", "else": L("other"), "ret": "str"},
          {"if": F("like", "bool", "s", L("%spark%")), "then": F("upper", "str", "s"), "else": "t", "ret": "str"},
          F("concat", "str", "t", L("-"), "s", "t"), F("concatOperator", "str", "s", "t", L("é"), "t", "s"),
          F("lower", "str", F("left", "str", "s", I32(9)))]
    # predicates over a mapped value, next to the outputs they would gate
    g4 += [F("like", "bool", F("upper", "str", "s"), L("%SPARK%"))]
    # concat() under another function is hoisted into a first stage of its own: two wave-shaped plans, one after the other
    g5 = [F("substr", "str", F("concat", "str", "s", "t"), I64(8), I64(9)), F("concatOperator", "str", "s", L("1"), "t", L("22")),
          F("concat", "str", "s", "s", "t", "t", L("55555"))]
    return [g1, g2, g3, g4, g5]


# name -> (family, shape the group is meant to run on, trees).  "wave": a wave-shaped main kernel and its pre-pass;
# "stages": two such plans, the first writing the concat() that the second reads; "flat": upper(s) / lower(s) alone,
# stored from the sweep's registers.  A group of predicates or numbers carries one
# substr() output: a projector without a var-len output is planned on the scanner shape.
@functools.lru_cache(maxsize=None)
def groups():
    g = {"predicates_like": ("predicates", "wave", _predicates_like() + [CARRIER]),
         "predicates_compare": ("predicates", "wave", _predicates_compare() + [CARRIER]),
         "numbers_lengths": ("numbers", "wave", _numbers_lengths() + [CARRIER]),
         "numbers_hashes": ("numbers", "wave", _numbers_hashes() + [CARRIER])}
    for i, trees in enumerate(_views()):
        g["views_%d" % (i + 1)] = ("views", "wave", trees)
    for i, trees in enumerate(_materialised()):
        g["materialised_%d" % (i + 1)] = ("materialised", "stages" if i == 4 else "wave", trees)
    g["flat_upper"] = ("flat", "flat", [F("upper", "str", "s")])
    g["flat_lower"] = ("flat", "flat", [F("lower", "str", "s")])
    return g


FAMILIES = ("predicates", "numbers", "views", "materialised", "flat")


def family_groups(family):
    return [name for name, (fam, _, _) in groups().items() if fam == family]


def group_specs(name):
    return [{"label": _label(t), "tree": t, "ret": _ret(t), "group": name} for t in groups()[name][2]]


def family_specs(family):
    return [sp for name in family_groups(family) for sp in group_specs(name)]


def build_expressions(gandiva, specs):
    b = gandiva.TreeExprBuilder()

    def node(t):
        if isinstance(t, str):
            return b.make_field(SCHEMA.field(t))
        if "lit" in t:
            return b.make_literal(t["lit"].encode() if t["type"] == "bin" else t["lit"], TYPES[t["type"]])
        if "if" in t:
            return b.make_if(node(t["if"]), node(t["then"]), node(t["else"]), TYPES[t["ret"]])
        if "in" in t:
            return b.make_in_expression(node(t["in"]), t["values"], pa.string())
        return b.make_function(t["fn"], [node(a) for a in t["args"]], TYPES[t["ret"]])
    return [b.make_expression(node(sp["tree"]), pa.field("r%d" % i, TYPES[sp["ret"]])) for i, sp in enumerate(specs)]


# ---- the corpus -------------------------------------------------------------------------------------------------------
_WORDS = ["spark", "Flink", "a_b%c", " ", "sparkles", "x", "MiXeD CaSe", "100%", "ar", "  ", "sparkling", "k", "07x", "sp", "park", "Sp"]
_MB = ["é", "日", "𝄞", "ß", "語", "€"]


def text(n, seed, variant):
    """n bytes of words (needles, their prefixes, spaces, cased letters, digits, LIKE's wildcards); the multibyte variant
    puts a 2-, 3- or 4-byte character after every word, so characters fall on every kind of boundary.  A row above 65535
    bytes holds neither "k" nor "sp", so no needle: replace() raises on a result of more than 65535 bytes (a stated rule),
    and nothing in these families is meant to raise."""
    words = _WORDS if n <= 65535 else [w for w in _WORDS if "k" not in w and "sp" not in w]
    out, size, i = [], 0, seed
    while size < n:
        w = words[(i * 7 + seed) % len(words)]
        if variant == "multibyte":
            w += _MB[(i + seed) % len(_MB)]
        i += 1
        for c in w:
            cl = len(c.encode())
            if size + cl > n:
                c, cl = "x", 1
            out.append(c)
            size += cl
            if size == n:
                break
    return "".join(out)


def _fill(n, variant):
    """n bytes that hold no letter of a needle: dots, in the multibyte variant with a 3-byte character before each."""
    if variant == "ascii":
        return "." * n
    head = ("日." * n).encode()[:n].decode(errors="ignore")
    return head + "." * (n - len(head.encode()))


class _Corpus:
    def __init__(self, variant):
        self.variant, self.rows, self.forced_null, self.anchor, self.runs = variant, [], set(), set(), {}

    def align(self, rows):
        while len(self.rows) % rows:
            self.rows.append("")

    def run(self, name, rows, align=SUB, anchor=False):
        self.align(align)
        self.runs.setdefault(name, []).append((len(self.rows), len(rows)))
        if anchor:     # rows whose bytes make up a ladder's total: the random NULLs of nulls = 0.1 leave them alone
            self.anchor.update(range(len(self.rows), len(self.rows) + len(rows)))
        self.rows += rows


def _equal_rows(c, unit_rows, each, delta, seed):
    rows = [text(each, seed + i % 16, c.variant) for i in range(unit_rows)]
    rows[unit_rows // 3] = text(each + delta, seed + 17, c.variant)
    return rows


@functools.lru_cache(maxsize=None)
def corpus(variant):
    """(rows of s as str, forced-NULL row numbers, anchor row numbers, runs: name -> [(first row, rows)])."""
    c = _Corpus(variant)
    v = variant
    # the needle as the first bytes of the data buffer, then the row-length ladder
    c.run("lengths", ["sparkling" + text(20, 1, v)] + [text(n, 3 + n, v) for n in LENGTH_LADDER], anchor=True)
    # span ladders.  Equal rows of 32 bytes: a sub-tile holds 2048, a tile of 4 sub-tiles 8192, of 8 sub-tiles 16384;
    # equal rows of 8 bytes: 2048 / 4096 per tile of 4 / 8 sub-tiles.  One row of each run is a byte shorter or longer.
    for each in (32, 8):
        for delta in (-1, 0, 1):
            c.run("equal_%d%+d" % (each, delta), _equal_rows(c, TILE, each, delta, 100 * each + delta), align=TILE, anchor=True)
    # one long row among empty ones: T + delta in the first tile of 4 sub-tiles and T in the second, 2 T + delta in the
    # tile of 8 (8192 -> 16384: the match bitmaps; 2048 -> 4096: a window; and 2048 + delta alone in its sub-tile)
    for t in (8192, 2048):
        for delta in (-1, 0, 1):
            rows = [""] * TILE
            rows[5], rows[256 + 70] = text(t + delta, t + delta, v), text(t, t + 7, v)
            c.run("long_%d%+d" % (t, delta), rows, align=TILE, anchor=True)
    # output totals.  Rows of 4 bytes ("sp.k") with 4-byte second operands and counts of 8: concat(s, t), lpad(s, k),
    # rpad(s, k, t) and replace('k' -> 'kkkkk') write 8 bytes per row where they read 4; rows of 16 bytes: substr(s, 9) and
    # right(s, 8) write 8 where they read 16.  The OUTPUT's total stands at 2048 / 4096 per tile of 4 / 8 sub-tiles.
    for delta in (-1, 0, 1):
        rows = ["sp" + ".x"[i % 2] + "k" for i in range(TILE)]
        rows[100] = "spk" if delta < 0 else rows[100] + "z" * delta
        c.run("out_grow%+d" % delta, rows, align=TILE, anchor=True)
        rows = [text(16, 900 + i % 16, "ascii") for i in range(TILE)]
        rows[100] = text(16 + delta, 917, "ascii")
        c.run("out_shrink%+d" % delta, rows, align=TILE, anchor=True)
    # needle placement: sub-tiles of exactly 2048 bytes whose first byte is at a multiple of 1024 of the data buffer
    for needle in NEEDLES[1:]:
        c.align(SUB)
        used = sum(len(r.encode()) for r in c.rows)
        c.run("pad", [_fill(-used % 1024, v)])
        c.run("placed_" + needle, _placed_subtile(needle, v, False) + _placed_subtile(needle, v, True))
    # needles split over rows, which must not match: adjacent rows, the last row of a sub-tile and the first of the next,
    # likewise over the boundaries of wave tiles of 4 and of 8 sub-tiles, and around a NULL row
    rows = [_fill(24, v) for _ in range(2 * TILE)]
    pairs = [(10 + 4 * i, n) for i, n in enumerate(NEEDLES[1:])] + [(SUB * (2 * i + 1) - 1, n) for i, n in enumerate(NEEDLES[1:])] + \
            [(255, "spark"), (511, "sparkles"), (767, "sparkling")]
    for r, needle in pairs:
        h = len(needle) // 2
        rows[r], rows[r + 1] = _fill(20, v) + needle[:h], needle[h:] + _fill(20, v)
    nul = 40
    rows[nul - 1], rows[nul], rows[nul + 1] = _fill(20, v) + "spar", "k", "k" + _fill(20, v)
    first = len(c.rows) + (-len(c.rows) % TILE)
    c.forced_null.add(first + nul)
    c.run("split", rows, align=TILE)
    # degenerate runs
    c.run("empty_tile", [""] * TILE, align=TILE)
    first = len(c.rows) + (-len(c.rows) % TILE)
    c.forced_null.update(range(first, first + TILE))
    c.run("null_tile", ["x"] * TILE, align=TILE)
    c.run("alternating", [text(13, i, v) if i % 2 else "" for i in range(2 * SUB)])
    c.run("spaces", [" " * n for n in (1, 6, 7, 8, 9, 10, 15, 16, 17, 18, 24, 31, 32, 33)] +
          [" " * a + m + " " * z for a in (0, 7, 8, 9, 16) for z in (0, 7, 8, 9, 17) for m in ("x", "sp ark", "é" if v == "multibyte" else "ee")])
    c.run("long_then_short", [text(70001, 9, v)] + ["spark"[i % 5] for i in range(TILE)])
    # near misses: every needle with its last or its first byte changed or missing, as the first bytes, the last bytes and
    # in the middle of a row (a compare that drops a byte at either end of the needle answers these wrongly)
    rows = []
    for needle in NEEDLES:
        for miss in (needle[:-1] + "x", "x" + needle[1:], needle[:-1], needle[1:], needle):
            rows += [miss + _fill(11, v), _fill(11, v) + miss, _fill(7, v) + miss + _fill(9, v), miss]
    c.run("near_misses", rows)
    # the needle as the last bytes of the data buffer
    c.run("last", [text(30, 5, v), text(11, 6, v) + "spark"])
    return c.rows, frozenset(c.forced_null), frozenset(c.anchor), c.runs


def _placed_subtile(needle, variant, straddle):
    """64 rows of 2048 bytes in all that hold `needle` ending at byte 32, starting at byte 80 and straddling byte 128 (16 k:
    the pieces of three lanes), as the last bytes of the span, and either ending at and starting at byte 1024 (the sweep's
    step) or straddling it.  The rows are cut at the first or the last byte of a needle, never inside one."""
    n = len(needle)
    span = bytearray(b"." * 2048)
    pos = [32 - n, 80, 128 - (n + 1) // 2, 2048 - n] + ([1024 - (n + 1) // 2] if straddle else [1024 - n, 1024])
    for p in pos:
        span[p:p + n] = needle.encode()
    cuts = {0, 2048} | set(pos[0::2]) | {p + n for p in pos[1::2]}
    for p in range(150, 2040, 29):
        if len(cuts) < SUB + 1 and not any(m < p < m + n for m in pos):
            cuts.add(p)
    cuts = sorted(cuts)
    assert len(cuts) == SUB + 1
    rows = [span[a:z].decode() for a, z in zip(cuts, cuts[1:])]
    if variant == "multibyte":      # same lengths: two filler bytes become one 2-byte character, three times a row
        rows = [re.sub(r"\.\.(?=\.)", "é", r, count=3) for r in rows]
    return rows


_T_VALUES = ["k", "sp", "spark", "sparkles", "sparkling", "", "..", "x", " ", "sp.k", "z" * 4, "Flink", "é", "日本"]


@functools.lru_cache(maxsize=None)
def columns(variant, nulls):
    """The four columns as Python lists (None = NULL): s, t, b (the bytes of s), k."""
    rows, forced, anchor, _ = corpus(variant)
    n = len(rows)
    rng = np.random.default_rng(20 + int(nulls * 100))
    ascii_only = variant == "ascii"
    tv = [x for x in _T_VALUES if not ascii_only or x.isascii()]
    t = [tv[int(i)] for i in rng.integers(0, len(tv), n)]
    counts = [1, 2, 8, 9, 16, 17, -1, -8, -9, 0, 40, 300]      # (a per-row pad to more than 65536 characters raises)
    k = [counts[int(i)] for i in rng.integers(0, len(counts), n)]
    _, _, _, runs = corpus(variant)
    for delta in (-1, 0, 1):
        first, cnt = runs["out_grow%+d" % delta][0]
        for i in range(first, first + cnt):      # 4-byte second operands and a count of 8: 8 bytes out per row
            t[i], k[i] = "t.k" + "sp"[i % 2], 8
        k[first + 100] = 8 + delta               # (the row that is a byte shorter or longer, for the pads too)
    s = [None if i in forced else r for i, r in enumerate(rows)]
    if nulls > 0:
        for col, keep in ((s, anchor), (t, anchor), (k, anchor)):
            for i in np.flatnonzero(rng.random(n) < nulls).tolist():
                if i not in keep:
                    col[i] = None
    b = [None if x is None else x.encode() for x in s]
    return s, t, b, k


def _utf8_array(vals, typ):
    """A var-len array over a data buffer of exactly the bytes (a numpy array of that size, nothing behind the last row)."""
    raw = [b"" if v is None else (v if isinstance(v, bytes) else v.encode()) for v in vals]
    off = np.zeros(len(raw) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(r) for r in raw])
    data = np.frombuffer(b"".join(raw), dtype=np.uint8).copy()
    valid = np.array([v is not None for v in vals])
    bits = None if valid.all() else pa.py_buffer(np.packbits(valid, bitorder="little"))
    return pa.Array.from_buffers(typ, len(raw), [bits, pa.py_buffer(off), pa.py_buffer(data)], null_count=int((~valid).sum()))


@functools.lru_cache(maxsize=None)
def batch(variant, nulls):
    """One deterministic RecordBatch over SCHEMA; runs start at multiples of 64 (512 where a wave tile matters)."""
    s, t, b, k = columns(variant, nulls)
    return pa.RecordBatch.from_arrays([_utf8_array(s, pa.string()), pa.array(t, pa.string()), _utf8_array(b, pa.binary()),
                                       pa.array(k, pa.int32())], schema=SCHEMA)


# ---- layouts (pa.Array.from_buffers) -----------------------------------------------------------------------------------
LAYOUTS = ("sliced", "exact_end", "null_bytes")
_LAYOUT_ROWS = 3 * SUB + 9


@functools.lru_cache(maxsize=None)
def layout_columns(layout, variant):
    rows = [text(n % 37, n, variant) for n in range(_LAYOUT_ROWS - 9)] + [text(n, 50 + n, variant) for n in (9, 8, 7, 6, 5, 4, 3, 2, 1)]
    rows[0], rows[-10] = "k" + rows[0], rows[-10] + "spar"
    rng = np.random.default_rng(31)
    t = [_T_VALUES[int(i)] for i in rng.integers(0, 5, len(rows))]
    k = [[1, 8, 9, -1, 17][int(i)] for i in rng.integers(0, 5, len(rows))]
    s = list(rows)
    if layout == "null_bytes":
        for i in np.flatnonzero(rng.random(len(rows)) < 0.1).tolist():
            s[i] = None
    return s, t, [None if x is None else x.encode() for x in s], k, rows


@functools.lru_cache(maxsize=None)
def layout_batch(layout, variant):
    """sliced: the first offset of s and b is 7 and the bytes before and behind the rows hold needle halves, spaces and
    upper-case letters; exact_end: the data buffer ends at the last byte of the last row and the last rows hold 9..1
    bytes; null_bytes: the NULL rows of s keep their bytes (the flat store cannot serve such a batch)."""
    s, t, b, k, rows = layout_columns(layout, variant)
    if layout == "exact_end":
        sa, ba = _utf8_array(s, pa.string()), _utf8_array(b, pa.binary())
    else:
        before, behind = (b"SPA spar", b"k sparkling  SPARK") if layout == "sliced" else (b"", b"")
        before = before[:7] if layout == "sliced" else before
        raw = [r.encode() for r in rows]
        off = np.zeros(len(raw) + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(r) for r in raw])
        off += len(before)
        data = np.frombuffer(before + b"".join(raw) + behind, dtype=np.uint8).copy()
        valid = np.array([v is not None for v in s])
        bits = None if valid.all() else pa.py_buffer(np.packbits(valid, bitorder="little"))
        sa, ba = (pa.Array.from_buffers(typ, len(raw), [bits, pa.py_buffer(off), pa.py_buffer(data)], null_count=int((~valid).sum()))
                  for typ in (pa.string(), pa.binary()))
    return pa.RecordBatch.from_arrays([sa, pa.array(t, pa.string()), ba, pa.array(k, pa.int32())], schema=SCHEMA)


# ---- expected columns --------------------------------------------------------------------------------------------------
def expected_of(specs, cols):
    """One expected pyarrow array per spec over the columns (s, t, b, k as Python lists); a tree's value is computed once
    per distinct tuple of the columns it reads."""
    s, t, b, k = cols[:4]
    by_name = {"s": s, "t": t, "b": b, "k": k}
    out = []
    for sp in specs:
        names = sorted(_fields(sp["tree"], set()))
        memo = {}
        vals = []
        for key in zip(*[by_name[c] for c in names]):
            if key not in memo:
                memo[key] = evaluate(sp["tree"], dict(zip(names, key)))
            vals.append(memo[key])
        out.append(pa.array(vals, TYPES[sp["ret"]]))
    return out


@functools.lru_cache(maxsize=None)
def expected_columns(group, variant, nulls):
    return expected_of(group_specs(group), columns(variant, nulls))


@functools.lru_cache(maxsize=None)
def expected_layout_columns(group, layout, variant):
    return expected_of(group_specs(group), layout_columns(layout, variant))


# ---- the groups' kernel shapes, and what the GPU child asserts about the path of every evaluation ------------------------
# group -> (kernels of the row-mode plan; its optimistic kernels assume ASCII, so an exact variant exists; outputs staged
# through LDS windows, at least; a NULL row that carries bytes sends the batch to the general kernel).
# tests/test_string_shapes_cpu.py holds every entry against the generated text.
GROUP_SHAPES = {
    "predicates_like": ("wave", True, 1, False), "predicates_compare": ("wave", True, 1, False),
    "numbers_lengths": ("wave", True, 1, False), "numbers_hashes": ("wave", True, 1, False),
    "views_1": ("wave", True, 3, False), "views_2": ("wave", True, 3, False), "views_3": ("wave", True, 3, False),
    "views_4": ("wave", True, 3, False), "views_5": ("wave", True, 3, False), "views_6": ("wave", True, 3, False),
    "materialised_1": ("wave", True, 3, False), "materialised_2": ("wave", True, 3, False), "materialised_3": ("wave", True, 3, False),
    "materialised_4": ("wave", True, 3, False), "materialised_5": ("stages", True, 3, False),
    "flat_upper": ("flat", False, 0, True), "flat_lower": ("flat", False, 0, True),
}
MAIN_FILES = [("ascii", 0.0), ("ascii", 0.1), ("multibyte", 0.0), ("multibyte", 0.1), ("ascii", 0.0)]   # there, and back
VALIDATE_OUTPUTS = True      # the child validates every output in full (offsets, UTF-8) before it compares
CHILD_MODES = {"wave": {}, "scanner": {"GDV_NO_WAVE_SHAPE": "1"}, "selection": {}}


def _tagged(tag):
    parts = tag.split("/")      # "layout/<layout>/<variant>" or "<variant>/<nulls>"
    return (layout_batch(parts[1], parts[2]), parts[2]) if parts[0] == "layout" else (batch(parts[0], float(parts[1])), parts[0])


def _holds_non_ascii(arr):
    if len(arr) == 0:
        return False
    off = np.frombuffer(arr.buffers()[1], dtype=np.int32)[arr.offset: arr.offset + len(arr) + 1]
    data = np.frombuffer(arr.buffers()[2], dtype=np.uint8)[off[0]:off[-1]]
    return bool((data >= 0x80).any())


def child_batch(tag, from_file, off, rows):
    """The inputs with the buffer layout that matters (an exact-size data buffer, a first offset of 7, NULL rows with
    bytes): built again in the child, and equal to what the parent wrote."""
    b = _tagged(tag)[0].slice(off, rows)
    assert b.equals(from_file), "the child's batch %s differs from the parent's" % tag
    return b


def child_after_evaluate(case, tag, group, proj, whole):
    """path_hint after an evaluation: 0 on the optimistic kernels, 1 on the exact variant (text with a byte >= 0x80 under
    kernels that assume ASCII, and again on the next call; ASCII text brings 0 back), 2 on the scanner-shaped general
    kernel (NULL rows that carry bytes under a flat output).  With GDV_NO_WAVE_SHAPE=1 there is nothing to choose."""
    name = case["group_names"][case["groups"].index(group)]
    _, exact, _, notflat = GROUP_SHAPES[name]
    hint = proj.path_hint
    what = "%s %s: path_hint %d" % (name, tag, hint)
    if case["mode"] == "scanner":
        assert hint == 0, what
        return
    full, variant = _tagged(tag)
    if tag.startswith("layout/null_bytes") and notflat:
        assert not whole or hint == 2, what
    elif exact and whole:
        assert hint == (1 if variant == "multibyte" else 0), what
    elif exact and variant == "ascii":
        assert hint == 0, what
    elif not exact:
        assert hint == 0, what


def _selections(n, runs):
    edges = sorted({r for spans in runs.values() for first, rows in spans for r in (first, first + rows - 1)})
    return [("every row", np.arange(n)), ("every third row", np.arange(0, n, 3)), ("first and last row of each run", np.array(edges)),
            ("no row", np.arange(0))]


def child_extra_passes(gandiva, case, exprs, groups, projs, failures):
    """wave / scanner: every whole batch once more through DeviceBatch.from_arrow and evaluate_device.  selection: every
    group as a UINT16 and a UINT32 projector over four selections of the ASCII batches (on the wave pair: path_hint 0),
    then over a selection of ASCII rows and ONE multi-byte row, which reaches the general kernel through NOTASCII."""
    import torch
    from gandiva_amd import gandiva as gg
    from helpers import assert_bit_exact
    specs, evaluations = case["specs"], 0

    def compare(got, group, want_of, what):
        for i, g in zip(group, got):
            try:
                g.validate(full=True)
                assert_bit_exact(g, want_of(i), "%s %s" % (specs[i]["label"], what))
            except AssertionError as e:
                failures.append(str(e))
    if case["mode"] != "selection":
        for tag, path in dict(case["files"]).items():
            if tag.startswith("layout/"):
                continue
            table = pa.ipc.open_file(path).read_all().combine_chunks()
            db = gandiva.DeviceBatch.from_arrow(_tagged(tag)[0])
            for group, proj in zip(groups, projs):
                outs = proj.evaluate_device(db)
                torch.cuda.synchronize()
                evaluations += 1
                compare([o.to_arrow() for o in outs], group, lambda i: table.column("e%d" % specs[i]["column"]).chunk(0), "device-resident " + tag)
        # last, because it leaves a projector with a flat output on the general kernel: NULL rows that carry bytes
        for tag, path in case.get("null_bytes_files", []):
            table = pa.ipc.open_file(path).read_all().combine_chunks()
            for name, group, proj in zip(case["group_names"], groups, projs):
                got = proj.evaluate(_tagged(tag)[0])
                evaluations += 1
                compare(got, group, lambda i: table.column("e%d" % specs[i]["column"]).chunk(0), tag)
                child_after_evaluate(case, tag, group, proj, True)
        return evaluations
    for mode_name, mode, dtype in (("UINT16", 1, np.uint16), ("UINT32", 2, np.uint32)):
        sel_projs = [gandiva.make_projector(SCHEMA, [exprs[i] for i in group], None, mode_name) for group in groups]
        for tag, path in case["selection_files"]:
            table = pa.ipc.open_file(path).read_all().combine_chunks()
            full, variant = _tagged(tag)
            runs = corpus(variant)[3]
            if variant == "ascii":
                selections = _selections(full.num_rows, runs)
            else:      # rows of the empty tile, and one row of the length ladder that holds multi-byte characters
                e0, row = runs["empty_tile"][0][0], 30
                t = full.column("t").to_pylist()
                plain = [r for r in range(e0, e0 + TILE) if t[r] is None or t[r].isascii()][:40]
                assert _holds_non_ascii(full.column("s").slice(row, 1)) and len(plain) == 40
                selections = [("ASCII rows and one multi-byte row", np.array([row] + plain))]
            for sel_name, idx in selections:
                sel = gg.SelectionVector(mode, np.ascontiguousarray(idx.astype(dtype) if len(idx) else np.zeros(1, dtype)), len(idx))
                take = pa.array(idx, pa.int64())
                for name, group, proj in zip(case["group_names"], groups, sel_projs):
                    got = proj.evaluate(full, sel)
                    evaluations += 1
                    what = "%s %s %s" % (mode_name, tag, sel_name)
                    compare(got, group, lambda i: table.column("e%d" % specs[i]["column"]).chunk(0).take(take), what)
                    want_hint = 0 if variant == "ascii" or not GROUP_SHAPES[name][1] or len(idx) == 0 else 2
                    if proj.path_hint != want_hint:
                        failures.append("%s %s: path_hint %d, not %d" % (name, what, proj.path_hint, want_hint))
    return evaluations
