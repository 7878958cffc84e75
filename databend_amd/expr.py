"""Scalar expressions for the projection in front of the aggregate (mirror of the `Expr` trees that
`BlockOperator::Map` evaluates, SQL/evaluator/block_operator.rs:50-80).

`plus`, `minus` and `multiply` over number and Decimal128 columns and typed constants, the date /
time functions over Date and Timestamp columns (session timezone UTC) and `length` over String
columns, evaluated on the device by dbg_expr_eval; the result columns stay in HBM and go into
`add_groups` as arguments or group keys as they are.

    price, disc, tax = col(0), col(1), col(2)
    disc_price = price * (lit(1) - disc)
    charge = disc_price * (lit(1) + tax)
    prog = ExprProgram([disc_price, charge], [extprice_col, discount_col, tax_col])
    prog.result_types()        # [Decimal(31, 4), Decimal(38, 6)]
    a, b = prog.eval(rows)     # DeviceColumns

    minute = extract("minute", col(0))             # to_minute(EventTime): UInt8
    bucket = date_trunc("minute", col(0))          # to_start_of_minute(EventTime): Timestamp
    yyyymm = to_year(col(1)) * 100 + to_month(col(1))
    url_len = length(col(2))                       # UInt64, NULL where the URL is
"""
from __future__ import annotations

import ctypes as C
from decimal import Decimal
from typing import List, Optional, Sequence

from . import abi
from .column import DataType, Decimal128

_OPS = {"+": abi.EXPR_PLUS, "-": abi.EXPR_MINUS, "*": abi.EXPR_MULTIPLY}
_UNSIGNED = ((abi.UINT8, 8), (abi.UINT16, 16), (abi.UINT32, 32), (abi.UINT64, 64))
_SIGNED = ((abi.INT8, 8), (abi.INT16, 16), (abi.INT32, 32), (abi.INT64, 64))


class Expr:
    def key(self) -> tuple:
        """Structural identity: equal subtrees share one evaluation."""
        raise NotImplementedError

    def children(self) -> Sequence["Expr"]:
        return ()

    def __add__(self, o):
        return _Bin("+", self, _wrap(o))

    def __radd__(self, o):
        return _Bin("+", _wrap(o), self)

    def __sub__(self, o):
        return _Bin("-", self, _wrap(o))

    def __rsub__(self, o):
        return _Bin("-", _wrap(o), self)

    def __mul__(self, o):
        return _Bin("*", self, _wrap(o))

    def __rmul__(self, o):
        return _Bin("*", _wrap(o), self)

    def func(self, name: str) -> "Expr":
        """`name(self)` for a function of abi.EXPR_FUNC_NAMES; every one is also a method and a
        module function of its own name: `e.to_year()`, `to_year(e)`."""
        return _Func(name, self)


class _Col(Expr):
    def __init__(self, index: int):
        self.index = int(index)

    def key(self):
        return ("col", self.index)


class _Lit(Expr):
    def __init__(self, value, dtype: DataType):
        self.value, self.dtype = value, dtype

    def key(self):
        return ("lit", repr(self.value), self.dtype)


class _Bin(Expr):
    def __init__(self, op: str, a: Expr, b: Expr):
        self.op, self.a, self.b = op, a, b
        self._key = ("bin", op, a.key(), b.key())

    def key(self):
        return self._key

    def children(self):
        return (self.a, self.b)


class _Func(Expr):
    def __init__(self, name: str, a: Expr):
        if name not in abi.EXPR_FUNCS:
            raise ValueError(f"no function {name!r}")
        self.name, self.a = name, a
        self._key = ("func", name, a.key())

    def key(self):
        return self._key

    def children(self):
        return (self.a,)


def _define_functions():
    for name in abi.EXPR_FUNC_NAMES:
        def method(self, _name=name):
            return _Func(_name, self)

        def function(e, _name=name):
            return _Func(_name, _wrap(e))
        method.__name__ = function.__name__ = name
        method.__doc__ = function.__doc__ = f"The reference's `{name}`."
        setattr(Expr, name, method)
        globals()[name] = function


_define_functions()

# date_trunc(unit, e): the to_start_of_* function the reference's rewrite picks; year, quarter and
# month give a Date, the others a Timestamp
_DATE_TRUNC = {"year": "to_start_of_year", "quarter": "to_start_of_quarter", "month": "to_start_of_month",
               "day": "to_start_of_day", "hour": "to_start_of_hour", "minute": "to_start_of_minute",
               "second": "to_start_of_second"}
# extract(unit FROM e) / date_part: the to_* number function
_EXTRACT = {"year": "to_year", "quarter": "to_quarter", "month": "to_month", "day": "to_day_of_month", "dow": "to_day_of_week",
            "doy": "to_day_of_year", "week": "to_week_of_year", "hour": "to_hour", "minute": "to_minute", "second": "to_second",
            "epoch": "to_unix_timestamp", "yyyymm": "to_yyyymm", "yyyymmdd": "to_yyyymmdd", "yyyymmddhh": "to_yyyymmddhh",
            "yyyymmddhhmmss": "to_yyyymmddhhmmss"}


def date_trunc(unit: str, e) -> Expr:
    """`DATE_TRUNC(unit, e)`: sugar for the function the reference rewrites it to."""
    u = unit.lower()
    if u not in _DATE_TRUNC:
        raise ValueError(f"date_trunc: no unit {unit!r}; one of {sorted(_DATE_TRUNC)}")
    return _Func(_DATE_TRUNC[u], _wrap(e))


def extract(unit: str, e) -> Expr:
    """`EXTRACT(unit FROM e)`: sugar for the reference's `to_*` number function."""
    u = unit.lower()
    if u not in _EXTRACT:
        raise ValueError(f"extract: no unit {unit!r}; one of {sorted(_EXTRACT)}")
    return _Func(_EXTRACT[u], _wrap(e))


def _wrap(v) -> Expr:
    return v if isinstance(v, Expr) else lit(v)


def col(index: int) -> Expr:
    """Column `index` of the program's columns."""
    return _Col(index)


def literal_type(v) -> DataType:
    """The type the reference gives a literal: the smallest unsigned integer that holds it, the
    smallest signed one for a negative value, Float64 for a float, and for a decimal
    Decimal(digits, fraction digits) — `0.5` is Decimal(1, 1)."""
    if isinstance(v, bool):
        raise TypeError("Boolean literals are not supported")
    if isinstance(v, int):
        if v >= 0:
            for t, bits in _UNSIGNED:
                if v < (1 << bits):
                    return DataType(t)
        else:
            for t, bits in _SIGNED:
                if v >= -(1 << (bits - 1)):
                    return DataType(t)
        raise OverflowError(f"integer literal {v} does not fit 64 bits")
    if isinstance(v, float):
        return DataType(abi.FLOAT64)
    if isinstance(v, Decimal):
        scale = max(0, -int(v.as_tuple().exponent))
        whole = abs(int(v.scaleb(scale))) // 10 ** scale
        int_digits = len(str(whole)) if whole else 0  # a zero integer part does not count: 0.5 has one digit
        return Decimal128(max(int_digits + scale, 1), scale)
    raise TypeError(f"no literal type for {type(v).__name__}")


def lit(v, dtype: Optional[DataType] = None) -> Expr:
    """A typed constant; `dtype` defaults to `literal_type(v)`."""
    return _Lit(v, dtype if dtype is not None else literal_type(v))


def _set_const(n: abi.dbg_expr_node, v, dt: DataType):
    n.dt = dt.to_abi()
    t = dt.type_id
    if t in (abi.FLOAT32, abi.FLOAT64):
        n.f64 = float(v)
    elif t == abi.DECIMAL128:
        x = int(Decimal(v).scaleb(dt.scale)) if isinstance(v, Decimal) else int(v)  # an int is the scaled value
        u = x & ((1 << 128) - 1)
        n.i128_lo = u & ((1 << 64) - 1)
        hi = u >> 64
        n.i128_hi = hi - (1 << 64) if hi >= (1 << 63) else hi
    else:
        u = int(v) & ((1 << 64) - 1)
        n.i64 = u - (1 << 64) if u >= (1 << 63) else u


def postfix(exprs: Sequence[Expr]) -> List[dict]:
    """The outputs as one postfix program.  An output that is a subtree of another is stored on the
    way (STORE leaves the value on the stack), so it is evaluated once."""
    keys = [e.key() for e in exprs]
    first = {}
    for i, k in enumerate(keys):
        first.setdefault(k, []).append(i)
    stored = set()
    out: List[dict] = []

    def emit(e: Expr):
        if isinstance(e, _Col):
            out.append(dict(op=abi.EXPR_COLUMN, index=e.index))
        elif isinstance(e, _Lit):
            out.append(dict(op=abi.EXPR_CONST, value=e.value, dtype=e.dtype))
        elif isinstance(e, _Func):
            emit(e.a)
            out.append(dict(op=abi.EXPR_FUNC, index=abi.EXPR_FUNCS[e.name]))
        else:
            emit(e.a)
            emit(e.b)
            out.append(dict(op=_OPS[e.op]))
        for i in first.get(e.key(), ()):
            if i not in stored:
                stored.add(i)
                out.append(dict(op=abi.EXPR_STORE, index=i))

    def contains(e: Expr, k: tuple) -> bool:
        return e.key() == k or any(contains(c, k) for c in e.children())

    for i, e in enumerate(exprs):
        if i in stored:
            continue
        # an output inside a later, larger output is stored when that one is emitted
        if any(j != i and j not in stored and keys[j] != keys[i] and contains(exprs[j], keys[i]) for j in range(len(exprs))):
            continue
        emit(e)
    return out


class ExprProgram:
    """Expressions bound to their columns, marshalled as `dbg_expr_program` (kept alive by this
    object).  `cols` holds `dbg_column` structs or column objects (DeviceColumn; Date, Timestamp
    and String columns for the functions that take them): objects are kept referenced here, as
    FilterProgram keeps its own.  The program's `reserved` word is 0: the session timezone is UTC."""

    def __init__(self, exprs: Sequence[Expr], cols: Sequence):
        self.exprs = list(exprs)
        self._owners = [c for c in cols if hasattr(c, "to_abi")]
        self.cols = [c.to_abi() if hasattr(c, "to_abi") else c for c in cols]
        post = postfix(self.exprs)
        self.nodes = (abi.dbg_expr_node * max(1, len(post)))()
        for i, d in enumerate(post):
            n = self.nodes[i]
            n.op = d["op"]
            n.index = d.get("index", 0)
            if d["op"] == abi.EXPR_CONST:
                _set_const(n, d["value"], d["dtype"])
        self.col_arr = (abi.dbg_column * max(1, len(self.cols)))(*self.cols)
        self.struct = abi.dbg_expr_program(self.nodes, len(post), len(self.cols), self.col_arr, len(self.exprs), 0)

    def ptr(self):
        return C.byref(self.struct)

    def result_types(self) -> List[DataType]:
        from .ffi import check, lib
        out = []
        for k in range(len(self.exprs)):
            dt = abi.dbg_datatype()
            check(lib().dbg_expr_result_type(self.ptr(), k, C.byref(dt)))
            out.append(DataType.from_abi(dt))
        return out

    def eval(self, rows: int, filter_program=None, stream=None) -> list:
        """Evaluate over `rows` rows; returns one DeviceColumn per expression.  With a
        FilterProgram, rows it does not select cannot raise and their outputs are unspecified."""
        from . import device
        from .ffi import check, lib
        types = self.result_types()
        dev = "cuda"
        for c in self._owners:
            if getattr(c, "data", None) is not None and hasattr(c.data, "device"):
                dev = c.data.device
                break
        outs = [device.empty(t, rows, device=dev) for t in types]
        arr = (abi.dbg_out_column * max(1, len(outs)))()
        for i, o in enumerate(outs):
            arr[i].data = o.data.data_ptr()
            if o.validity is not None:
                arr[i].validity = o.validity.data_ptr()
        fp = filter_program.ptr() if filter_program is not None else None
        check(lib().dbg_expr_eval(self.ptr(), fp, rows, arr, stream))
        return outs
