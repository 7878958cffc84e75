"""An independent reference for the device projection (databend_amd/csrc/expr.hpp, expr.hip): the
reference's rules for plus / minus / multiply over numbers and Decimal128, in plain Python integers.

Types are `DataType`s; an integer or decimal value is a Python int (a decimal: the value scaled by
10^scale), a float value a Python float (a double), NULL is None.  An expression is a tuple:
    ("col", i) | ("lit", value, DataType) | (op, a, b)   with op one of "+", "-", "*"

The rules (FUNCS = src/query/functions/src/scalars of the reference):
 * numbers (FUNCS/arithmetic.rs:91-175): plus / multiply -> an integer of min(64, 2 x the wider
   operand) bits, signed if either operand is; minus -> that width, always signed; a float operand
   -> Float64.  64-bit integer results wrap.
 * Decimal128 (EXP/types/decimal.rs:1000-1067, FUNCS/decimal/arithmetic.rs:75-172): see
   `result_type` and `apply`.
 * NULLs (EXP/function.rs:562-571, 660-710): nullable if any operand is; NULL if any operand is;
   a NULL row raises nothing.
"""
import struct

from databend_amd import abi
from databend_amd.column import DataType, Decimal128

INTS = (abi.INT8, abi.INT16, abi.INT32, abi.INT64, abi.UINT8, abi.UINT16, abi.UINT32, abi.UINT64)
FLOATS = (abi.FLOAT32, abi.FLOAT64)
NUMBERS = INTS + FLOATS
BITS = {abi.INT8: 8, abi.INT16: 16, abi.INT32: 32, abi.INT64: 64, abi.UINT8: 8, abi.UINT16: 16, abi.UINT32: 32, abi.UINT64: 64}
SIGNED = (abi.INT8, abi.INT16, abi.INT32, abi.INT64)
INT_OF = {(8, True): abi.INT8, (16, True): abi.INT16, (32, True): abi.INT32, (64, True): abi.INT64,
          (8, False): abi.UINT8, (16, False): abi.UINT16, (32, False): abi.UINT32, (64, False): abi.UINT64}
# get_decimal_properties (EXP/types/number.rs:475-484): the digits of an integer type
INT_DIGITS = {abi.INT8: 3, abi.UINT8: 3, abi.INT16: 5, abi.UINT16: 5, abi.INT32: 10, abi.UINT32: 10, abi.INT64: 19, abi.UINT64: 20}
OP_NAME = {"+": "plus", "-": "minus", "*": "multiply"}
I128_MIN, I128_MAX = -(1 << 127), (1 << 127) - 1


class Unsupported(Exception):
    pass


class Overflow(Exception):
    """An operator failed on a valid row; `.op` is its name."""

    def __init__(self, op):
        super().__init__(op)
        self.op = op


def int_range(t):
    b = BITS[t]
    return (-(1 << (b - 1)), (1 << (b - 1)) - 1) if t in SIGNED else (0, (1 << b) - 1)


def wrap_int(v, t):
    b = BITS[t]
    v &= (1 << b) - 1
    return v - (1 << b) if t in SIGNED and v >> (b - 1) else v


def refuse(t: DataType):
    names = {abi.DECIMAL256: "Decimal256", abi.STRING: "String", abi.BOOLEAN: "Boolean", abi.DATE: "Date", abi.TIMESTAMP: "Timestamp"}
    if t.type_id in names:
        raise Unsupported(names[t.type_id])


def dec_props(t: DataType):
    if t.type_id == abi.DECIMAL128:
        return t.precision, t.scale
    return INT_DIGITS[t.type_id], 0


def result_type(op: str, a: DataType, b: DataType) -> DataType:
    refuse(a)
    refuse(b)
    nullable = a.nullable or b.nullable
    da, db = a.type_id == abi.DECIMAL128, b.type_id == abi.DECIMAL128
    if not da and not db:
        if a.type_id in FLOATS or b.type_id in FLOATS:
            return DataType(abi.FLOAT64, 0, 0, nullable)
        w = min(64, 2 * max(BITS[a.type_id], BITS[b.type_id]))
        signed = op == "-" or a.type_id in SIGNED or b.type_id in SIGNED
        return DataType(INT_OF[(w, signed)], 0, 0, nullable)
    if a.type_id in FLOATS or b.type_id in FLOATS:
        raise Unsupported("Decimal mixed with Float")
    (pa, sa), (pb, sb) = dec_props(a), dec_props(b)
    la, lb = pa - sa, pb - sb
    if op == "*":
        s = min(sa + sb, max(sa, sb, 12))
        p = min(38, la + lb + s)
    else:
        s = max(sa, sb)
        p = min(38, max(la, lb) + s + 1)
    return DataType(abi.DECIMAL128, p, s, nullable)


def to_f64(v, t: DataType) -> float:
    return float(v)  # an integer rounds to the nearest double as Rust's `as f64` does; a Float32 widens exactly


def div_trunc(a: int, b: int) -> int:
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def apply(op: str, ta: DataType, tb: DataType, x, y):
    """x op y for non-NULL operands: the value, or Overflow."""
    rt = result_type(op, ta, tb)
    if rt.type_id == abi.FLOAT64:
        fx, fy = to_f64(x, ta), to_f64(y, tb)
        return fx + fy if op == "+" else (fx - fy if op == "-" else fx * fy)
    if rt.type_id != abi.DECIMAL128:
        r = x + y if op == "+" else (x - y if op == "-" else x * y)
        return wrap_int(r, rt.type_id)
    (_, sa), (_, sb) = dec_props(ta), dec_props(tb)
    p, s = rt.precision, rt.scale
    lim = 10 ** p - 1
    if op == "*":
        # do_round_mul (decimal.rs:465-478): half the divisor away from zero, truncating division,
        # an error only outside i128
        div = 10 ** (sa + sb - s)
        prod = x * y
        r = div_trunc(prod + div // 2, div) if (x < 0) == (y < 0) else div_trunc(prod - div // 2, div)
        if not I128_MIN <= r <= I128_MAX:
            raise Overflow("multiply")
        return r
    vals = []
    for v, sv, t in ((x, sa, ta), (y, sb, tb)):
        # the cast to (p, s): raising the scale (and every integer operand) multiplies and checks
        # the precision's range (cast.rs:489-525, 686-707); the same scale copies
        if sv < s or t.type_id != abi.DECIMAL128:
            v = v * 10 ** (s - sv)
            if not -lim <= v <= lim:
                raise Overflow(OP_NAME[op])
        vals.append(v)
    r = vals[0] + vals[1] if op == "+" else vals[0] - vals[1]
    r = ((r - I128_MIN) % (1 << 128)) + I128_MIN  # i128 arithmetic wraps in a release build
    if p == 38 and not -lim <= r <= lim:
        raise Overflow(OP_NAME[op])
    return r


def type_of(e, col_types) -> DataType:
    if e[0] == "col":
        t = col_types[e[1]]
        refuse(t)
        return t
    if e[0] == "lit":
        refuse(e[2])
        return e[2]
    return result_type(e[0], type_of(e[1], col_types), type_of(e[2], col_types))


def eval_row(e, col_types, row, raise_errors=True):
    """Value of e on one row (None = NULL)."""
    if e[0] == "col":
        return row[e[1]]
    if e[0] == "lit":
        return e[1]
    a = eval_row(e[1], col_types, row, raise_errors)
    b = eval_row(e[2], col_types, row, raise_errors)
    if a is None or b is None:
        return None
    return apply(e[0], type_of(e[1], col_types), type_of(e[2], col_types), a, b)


def evaluate(e, col_types, col_values, selected=None):
    """(type, values, error): values[i] is None for NULL; error is the name of the operator that
    failed on a valid, selected row (the values are then meaningless), else None.  A row that is
    not selected is not evaluated: its value is reported as the string "unselected"."""
    t = type_of(e, col_types)
    n = len(col_values[0]) if col_values else 0
    out, err = [], None
    for i in range(n):
        if selected is not None and not selected[i]:
            out.append("unselected")
            continue
        try:
            out.append(eval_row(e, col_types, [c[i] for c in col_values]))
        except Overflow as o:
            err = err or o.op
            out.append("error")
    return t, out, err


def f64_bits(v: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def same_value(t: DataType, a, b) -> bool:
    if a is None or b is None:
        return a is None and b is None
    if t.type_id in FLOATS:
        if a != a or b != b:
            return a != a and b != b
        return f64_bits(float(a)) == f64_bits(float(b))
    return int(a) == int(b)


def to_lib_expr(e):
    """The tuple form as a databend_amd.expr tree."""
    from decimal import Decimal

    from databend_amd import expr as X
    if e[0] == "col":
        return X.col(e[1])
    if e[0] == "lit":
        v, t = e[1], e[2]
        if t.type_id == abi.DECIMAL128:
            return X.lit(int(v), t)  # an int for a decimal type is the scaled value
        return X.lit(v, t)
    a, b = to_lib_expr(e[1]), to_lib_expr(e[2])
    return a + b if e[0] == "+" else (a - b if e[0] == "-" else a * b)


def Dec(p, s, nullable=False) -> DataType:
    t = Decimal128(p, s)
    return t.wrap_nullable() if nullable else t


# ---- binary cases for the host build and the device kernels --------------------------------------
F32_MAX = struct.unpack("<f", struct.pack("<I", 0x7F7FFFFF))[0]


def extremes(t: DataType):
    """The type's extremes, 0 and +-1, and a few values in between."""
    k = t.type_id
    if k in INTS:
        lo, hi = int_range(k)
        vals = [lo, hi, 0, 1, hi - 1, lo + 1, hi // 3]
        if k in SIGNED:
            vals += [-1, -(hi // 3)]
        return vals
    if k == abi.FLOAT32:
        tenth = struct.unpack("<f", struct.pack("<f", 0.1))[0]
        return [0.0, -0.0, 1.0, -1.0, F32_MAX, -F32_MAX, struct.unpack("<f", struct.pack("<I", 1))[0], tenth, float("inf"), float("nan")]
    if k == abi.FLOAT64:
        return [0.0, -0.0, 1.0, -1.0, 1.7976931348623157e308, -1.7976931348623157e308, 5e-324, 0.1, 1.0 / 3.0, float(2 ** 53),
                float("inf"), float("-inf"), float("nan")]
    m = 10 ** t.precision - 1
    return [0, 1, -1, m, -m, m // 2 + 1, -(m // 3), 10 ** max(0, t.precision - 1), 5 * 10 ** max(0, t.scale - 1)]


def canon(v, t: DataType):
    """(lo, hi): the value as the evaluator holds it."""
    if t.type_id in FLOATS:
        return f64_bits(float(v)), 0
    u = int(v) & ((1 << 128) - 1)
    return u & ((1 << 64) - 1), u >> 64


def uncanon(lo, hi, t: DataType):
    if t.type_id in FLOATS:
        return struct.unpack("<d", struct.pack("<Q", lo))[0]
    if t.type_id == abi.DECIMAL128:
        u = lo | (hi << 64)
        return u - (1 << 128) if u >> 127 else u
    return wrap_int(lo, t.type_id)


def pack_cases(cases) -> bytes:
    """cases: (op, ta, tb, x, y) — the case file of tests/csrc/expr_host_main.cpp."""
    parts = [struct.pack("<I", len(cases))]
    for op, ta, tb, x, y in cases:
        (alo, ahi), (blo, bhi) = canon(x, ta), canon(y, tb)
        parts.append(struct.pack("<8B4Q", "+-*".index(op), ta.type_id, ta.precision, ta.scale, tb.type_id, tb.precision, tb.scale, 0,
                                 alo, ahi, blo, bhi))
    return b"".join(parts)


NUMBER_TYPES = [DataType(t) for t in NUMBERS]
# decimal (p, s) pairs: small, the scale cap of 12, the clamp at 38, divisors 10^0 / 10^8 / 10^30 / 10^38
DECIMAL_GRID = [(1, 0), (1, 1), (10, 1), (15, 2), (16, 2), (18, 9), (20, 10), (31, 4), (38, 0), (38, 6), (38, 10), (38, 19),
                (38, 30), (38, 38)]


def number_cases():
    out = []
    for op in "+-*":
        for ta in NUMBER_TYPES:
            for tb in NUMBER_TYPES:
                xs, ys = extremes(ta), extremes(tb)
                n = max(len(xs), len(ys))
                out += [(op, ta, tb, xs[i % len(xs)], ys[(i * 3 + 1) % len(ys)]) for i in range(n)]
                out += [(op, ta, tb, xs[0], ys[0]), (op, ta, tb, xs[1], ys[1]), (op, ta, tb, xs[0], ys[1])]
    return out


def decimal_cases():
    """Decimal x decimal over the grid and integer x decimal, with values at the rules' edges: the
    precision's extremes, exact halves of the multiply divisor, results around 10^38 and 2^127."""
    out = []
    ints = [DataType(t) for t in INTS]
    for op in "+-*":
        for pa, sa in DECIMAL_GRID:
            for pb, sb in DECIMAL_GRID:
                ta, tb = Dec(pa, sa), Dec(pb, sb)
                xs, ys = extremes(ta), extremes(tb)
                out += [(op, ta, tb, xs[i % len(xs)], ys[(i * 2 + 1) % len(ys)]) for i in range(len(xs))]
                if op == "*":
                    rt = result_type(op, ta, tb)
                    k = sa + sb - rt.scale
                    if k:
                        h = 10 ** k // 2  # products exactly at, just below and just above half the divisor
                        out += [(op, ta, tb, h, 1), (op, ta, tb, -h, 1), (op, ta, tb, h, -1), (op, ta, tb, -h, -1),
                                (op, ta, tb, h - 1, 1), (op, ta, tb, 1 - h, 1), (op, ta, tb, 3 * h, 1), (op, ta, tb, -3 * h, 1)]
            for ti in ints:
                ta = Dec(pa, sa)
                xs, ys = extremes(ta), extremes(ti)
                out += [(op, ta, ti, xs[i % len(xs)], ys[i % len(ys)]) for i in range(len(xs))]
                out += [(op, ti, ta, ys[i % len(ys)], xs[(i + 2) % len(xs)]) for i in range(len(ys))]
    D = Dec(38, 0)
    out += [("*", D, D, 10 ** 19, 10 ** 19 + 7), ("*", D, D, 1 << 64, 1 << 63), ("*", D, D, -(1 << 64), 1 << 63),
            ("*", D, D, (1 << 64), (1 << 63) - 1), ("*", D, D, I128_MIN, 1), ("*", D, D, I128_MIN, -1), ("*", D, D, I128_MAX, I128_MAX),
            ("+", D, D, I128_MAX, I128_MAX), ("-", D, D, I128_MIN, 1), ("+", D, D, 10 ** 38 - 1, 1), ("+", D, D, 10 ** 38 - 2, 1),
            ("-", D, D, -(10 ** 38 - 1), 1)]
    E = Dec(38, 30)
    out += [("*", E, E, 10 ** 37, 10 ** 37), ("*", E, E, 5 * 10 ** 29, 1), ("*", E, E, -5 * 10 ** 29, 1), ("*", E, E, 5 * 10 ** 29 - 1, 1),
            ("*", E, E, I128_MAX, I128_MAX), ("*", E, E, I128_MIN, I128_MIN), ("*", E, E, I128_MIN, I128_MAX)]
    return out


def expected(case):
    """(type, value or None, error 0/1) of one binary case."""
    op, ta, tb, x, y = case
    t = result_type(op, ta, tb)
    try:
        return t, apply(op, ta, tb, x, y), 0
    except Overflow:
        return t, None, 1


# ---- whole programs: number operators whose results feed decimal operators ---------------------------
def postfix_of(e, out=None):
    """The tuple form as postfix nodes: ("col", i) | ("lit", value, type) | (op,)."""
    out = [] if out is None else out
    if e[0] in ("col", "lit"):
        out.append(e)
    else:
        postfix_of(e[1], out)
        postfix_of(e[2], out)
        out.append((e[0],))
    return out


def _spread(vals, n, step):
    return [vals[(i * step + i // len(vals)) % len(vals)] for i in range(n)]


def mixed_programs(rows=67):
    """(expression, column types, column values): integer intermediates — negative, wrapped at 64
    bits, unsigned with the top bit set — as either operand of a decimal operator, NULLs included."""
    T = lambda t, nullable=False: DataType(t, 0, 0, nullable)
    I8, I16, I32, I64 = T(abi.INT8), T(abi.INT16), T(abi.INT32, True), T(abi.INT64, True)
    U8, U32, U64 = T(abi.UINT8), T(abi.UINT32), T(abi.UINT64)
    i32, i64, u64, u32 = extremes(I32), extremes(I64), extremes(U64), extremes(U32)
    d152 = [0, 1, -1, 100, -100, 123456789012345, -999999999999999, 50, -50]
    d204 = [0, 1, -1, 10 ** 19, -(10 ** 19), 12345, -5 * 10 ** 3, 10 ** 20 - 1]
    d101 = [0, 5, -5, 10 ** 10 - 1, -(10 ** 10 - 1), 31]
    d380 = [0, 1, -1, 10 ** 30, -(10 ** 30), 10 ** 37, -(10 ** 37)]
    nulls = lambda vals, k: [None if i % k == k - 1 else v for i, v in enumerate(vals)]
    n = rows
    return [
        (("*", ("-", ("col", 0), ("col", 1)), ("col", 2)), [I32, U8, Dec(15, 2)],
         [nulls(_spread(i32, n, 1), 7), _spread(extremes(U8), n, 2), _spread(d152, n, 3)]),
        (("*", ("-", ("col", 0), ("lit", 7, U8)), ("lit", 100, Dec(3, 2))), [I32], [nulls(_spread([3, 7, 8, -5] + i32, n, 1), 5)]),
        (("+", ("+", ("col", 0), ("col", 1)), ("col", 2)), [I64, I64, Dec(20, 4, True)],
         [nulls(_spread(i64 + [-7], n, 1), 11), _spread(i64 + [5], n, 2), nulls(_spread(d204, n, 3), 9)]),
        (("-", ("-", ("col", 0), ("col", 1)), ("col", 2)), [U64, U64, Dec(10, 1)],
         [_spread(u64, n, 1), _spread(u64, n, 3), _spread(d101, n, 2)]),
        (("-", ("*", ("col", 0), ("col", 1)), ("col", 2)), [U32, U32, Dec(38, 0)],
         [_spread(u32, n, 1), _spread(u32, n, 2), _spread(d380, n, 3)]),
        (("+", ("col", 2), ("*", ("col", 0), ("col", 1))), [I16, I8, Dec(15, 2, True)],
         [_spread(extremes(I16), n, 1), _spread(extremes(I8), n, 2), nulls(_spread(d152, n, 3), 6)]),
        (("*", ("col", 1), ("-", ("+", ("col", 0), ("lit", -9, I8)), ("lit", 3, U8))), [I64, Dec(10, 1)],
         [nulls(_spread([4, 12, 13, -1] + i64, n, 1), 8), _spread(d101, n, 2)]),
    ]


def pack_programs(progs) -> bytes:
    """The program file of tests/csrc/expr_host_main.cpp (--programs): one output per program."""
    parts = [struct.pack("<I", len(progs))]
    for e, types, values in progs:
        nodes = postfix_of(e)
        n_rows = len(values[0])
        parts.append(struct.pack("<HHI", len(types), len(nodes), n_rows))
        for t in types:
            parts.append(struct.pack("<4B", t.type_id, t.precision, t.scale, 1 if t.nullable else 0))
        for nd in nodes:
            if nd[0] == "col":
                parts.append(struct.pack("<8B2Q", 0, nd[1], 0, 0, 0, 0, 0, 0, 0, 0))
            elif nd[0] == "lit":
                t = nd[2]
                lo, hi = canon(nd[1], t)
                parts.append(struct.pack("<8B2Q", 1, 0, t.type_id, t.precision, t.scale, 0, 0, 0, lo, hi))
            else:
                parts.append(struct.pack("<8B2Q", 2 + "+-*".index(nd[0]), 0, 0, 0, 0, 0, 0, 0, 0, 0))
        for i in range(n_rows):
            for t, col_vals in zip(types, values):
                v = col_vals[i]
                lo, hi = canon(0 if v is None else v, t)
                parts.append(struct.pack("<Q2Q", 0 if v is None else 1, lo, hi))
    return b"".join(parts)
