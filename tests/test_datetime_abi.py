"""dbg_expr_result_type on the host (no device) for DBG_EXPR_FUNC: the result type of every function
over Date, Timestamp and String, nullable and not, against tests/datetime_ref.py; every refusal by
code and by message; a non-zero `reserved` (a session timezone other than UTC).  Then the Python
mirror's functions, date_trunc and extract."""
import ctypes as C

import pytest

from databend_amd import abi
from databend_amd import column as col
from databend_amd import expr as X
from databend_amd.column import DataType
from databend_amd.ffi import lib
from tests import datetime_ref as D


def column_of(t: DataType) -> abi.dbg_column:
    c = abi.dbg_column()
    c.dt = t.to_abi()
    return c


def node(op, index=0, dt=None, i64=0):
    n = abi.dbg_expr_node()
    n.op, n.index, n.i64 = op, index, i64
    if dt is not None:
        n.dt = dt.to_abi()
    return n


def program(nodes, types, n_outputs=1, reserved=0):
    na = (abi.dbg_expr_node * max(1, len(nodes)))(*nodes)
    ca = (abi.dbg_column * max(1, len(types)))(*[column_of(t) for t in types])
    p = abi.dbg_expr_program(na, len(nodes), len(types), ca, n_outputs, reserved)
    p._keep = (na, ca)
    return p


def result_type(p, k=0):
    dt = abi.dbg_datatype()
    rc = lib().dbg_expr_result_type(C.byref(p), k, C.byref(dt))
    return rc, DataType.from_abi(dt), lib().dbg_last_error().decode(errors="replace")


COL0, STORE0 = node(abi.EXPR_COLUMN, 0), node(abi.EXPR_STORE, 0)


def func(name):
    return node(abi.EXPR_FUNC, abi.EXPR_FUNCS[name])


def unary(name, t):
    return program([COL0, func(name), STORE0], [t])


def test_ids_follow_the_header():
    assert abi.EXPR_FUNC == 6 and abi.EXPR_STORE == 5
    assert abi.EXPR_FUNCS["to_yyyymm"] == 1 and abi.EXPR_FUNCS["to_second"] == 15 and abi.EXPR_FUNCS["to_start_of_second"] == 16
    assert abi.EXPR_FUNCS["to_start_of_day"] == 23 and abi.EXPR_FUNCS["to_monday"] == 24 and abi.EXPR_FUNCS["length"] == 30
    assert C.sizeof(abi.dbg_expr_node) == 48 and C.sizeof(abi.dbg_expr_program) == 32  # additive only


@pytest.mark.parametrize("name", abi.EXPR_FUNC_NAMES)
def test_result_types_and_wrong_operand_types(name):
    """Every function x Date, Timestamp, String, nullable and not: the reference's result type where
    the reference registers the overload, DBG_ERR_INVALID naming the function where it does not."""
    n_ok = 0
    for base in (col.Date, col.Timestamp, col.String, col.Int32, col.UInt64, col.Float64, col.Decimal128(10, 2)):
        for t in (base, base.wrap_nullable()):
            rc, got, msg = result_type(unary(name, t))
            if D.takes(name, t):
                assert rc == abi.DBG_OK, msg
                assert got == D.result_type(name, t), (name, t, got)
                assert got.nullable == t.nullable
                n_ok += 1
            else:
                assert rc == abi.DBG_ERR_INVALID and name in msg and "does not take" in msg, (name, t, rc, msg)
    assert n_ok == (2 if name == "length" or name not in D.DATE_FUNCS else 4)


def test_exact_result_types():
    want = {"to_yyyymm": col.UInt32, "to_yyyymmdd": col.UInt32, "to_yyyymmddhh": col.UInt64, "to_yyyymmddhhmmss": col.UInt64,
            "to_year": col.UInt16, "to_quarter": col.UInt8, "to_month": col.UInt8, "to_day_of_month": col.UInt8,
            "to_day_of_week": col.UInt8, "to_day_of_year": col.UInt16, "to_week_of_year": col.UInt32, "to_unix_timestamp": col.Int64,
            "to_hour": col.UInt8, "to_minute": col.UInt8, "to_second": col.UInt8, "to_monday": col.Date, "to_start_of_week": col.Date,
            "to_start_of_month": col.Date, "to_start_of_quarter": col.Date, "to_start_of_year": col.Date,
            "to_start_of_iso_year": col.Date, "time_slot": col.Timestamp, "to_start_of_day": col.Timestamp,
            "to_start_of_second": col.Timestamp, "to_start_of_minute": col.Timestamp, "to_start_of_five_minutes": col.Timestamp,
            "to_start_of_ten_minutes": col.Timestamp, "to_start_of_fifteen_minutes": col.Timestamp, "to_start_of_hour": col.Timestamp}
    assert set(want) | {"length"} == set(abi.EXPR_FUNC_NAMES)
    for name, t in want.items():
        assert result_type(unary(name, col.Timestamp))[:2] == (abi.DBG_OK, t), name
    assert result_type(unary("length", col.String))[:2] == (abi.DBG_OK, col.UInt64)


def test_number_results_feed_the_operators():
    # to_year(d) * 100 + to_month(d): UInt16 * UInt8 -> UInt32, + UInt8 -> UInt64
    hundred = node(abi.EXPR_CONST, dt=DataType(abi.UINT8), i64=100)
    p = program([COL0, func("to_year"), hundred, node(abi.EXPR_MULTIPLY), COL0, func("to_month"), node(abi.EXPR_PLUS), STORE0],
                [col.Date.wrap_nullable()])
    assert result_type(p)[:2] == (abi.DBG_OK, col.UInt64.wrap_nullable())
    # a function of a function's Date result, and a bare Date column stored
    p = program([COL0, func("to_start_of_month"), func("to_day_of_week"), STORE0, COL0, node(abi.EXPR_STORE, 1)], [col.Timestamp], 2)
    assert result_type(p, 0)[:2] == (abi.DBG_OK, col.UInt8) and result_type(p, 1)[:2] == (abi.DBG_OK, col.Timestamp)
    # length + 1 with a Decimal beside it (the 128-bit instantiation)
    p = program([COL0, func("length"), node(abi.EXPR_COLUMN, 1), node(abi.EXPR_PLUS), STORE0], [col.String, col.Decimal128(10, 2)])
    assert result_type(p)[:2] == (abi.DBG_OK, col.Decimal128(23, 2))


@pytest.mark.parametrize("t,word", [(col.Date, "Date"), (col.Timestamp, "Timestamp"), (col.String, "String")])
def test_date_timestamp_string_values_are_no_operands_of_the_operators(t, word):
    for op, name in ((abi.EXPR_PLUS, "plus"), (abi.EXPR_MINUS, "minus"), (abi.EXPR_MULTIPLY, "multiply")):
        for nodes in ([COL0, node(abi.EXPR_COLUMN, 1), node(op), STORE0], [node(abi.EXPR_COLUMN, 1), COL0, node(op), STORE0]):
            rc, _, msg = result_type(program(nodes, [t, col.Int32]))
            assert rc == abi.DBG_ERR_UNSUPPORTED and word in msg and name in msg, (rc, msg)
    # ... nor is a function's Date / Timestamp result
    if t.type_id != abi.STRING:
        f = "to_start_of_month" if t.type_id == abi.DATE else "to_start_of_hour"
        rc, _, msg = result_type(program([COL0, func(f), node(abi.EXPR_COLUMN, 1), node(abi.EXPR_PLUS), STORE0], [col.Timestamp, col.Int64]))
        assert rc == abi.DBG_ERR_UNSUPPORTED and word in msg and "plus" in msg, (rc, msg)
    # constants of these types stay refused
    rc, _, msg = result_type(program([node(abi.EXPR_CONST, dt=t), func("length" if t.type_id == abi.STRING else "to_year"), STORE0], []))
    assert rc == abi.DBG_ERR_UNSUPPORTED and word in msg and "constant" in msg, (rc, msg)


def test_string_results_are_refused():
    rc, _, msg = result_type(program([COL0, STORE0], [col.String]))
    assert rc == abi.DBG_ERR_UNSUPPORTED and "String results" in msg


def test_unknown_function_ids():
    for bad in (0, -1, 31, 1000):
        rc, _, msg = result_type(program([COL0, node(abi.EXPR_FUNC, bad), STORE0], [col.Date]))
        assert rc == abi.DBG_ERR_INVALID and "function id" in msg and str(bad) in msg, (bad, rc, msg)
    rc, _, msg = result_type(program([COL0, node(7), STORE0], [col.Date]))
    assert rc == abi.DBG_ERR_INVALID and "unknown op" in msg


def test_function_stack_underflow():
    rc, _, msg = result_type(program([func("to_year"), STORE0], [col.Date]))
    assert rc == abi.DBG_ERR_INVALID and "underflow" in msg and "to_year" in msg


def test_reserved_must_be_zero():
    for r in (1, -1, 480):
        rc, _, msg = result_type(program([COL0, func("to_year"), STORE0], [col.Date], reserved=r))
        assert rc == abi.DBG_ERR_INVALID and "reserved" in msg and "UTC" in msg, (r, rc, msg)
        rc, _, msg = result_type(program([COL0, STORE0], [col.Int32], reserved=r))
        assert rc == abi.DBG_ERR_INVALID and "reserved" in msg
    assert result_type(program([COL0, func("to_year"), STORE0], [col.Date], reserved=0))[0] == abi.DBG_OK


def test_functions_do_not_count_as_live_values():
    # four live values with a function on each still fit the stack of four
    nodes = []
    for _ in range(4):
        nodes += [COL0, func("to_year")]
    nodes += [node(abi.EXPR_PLUS)] * 3 + [STORE0]
    assert result_type(program(nodes, [col.Date]))[:2] == (abi.DBG_OK, col.UInt64)


# ---- the Python mirror ------------------------------------------------------------------------------
def test_python_functions_methods_and_sugar():
    e = X.col(0)
    for name in abi.EXPR_FUNC_NAMES:
        a, b, c = getattr(X, name)(e), getattr(e, name)(), e.func(name)
        assert a.key() == b.key() == c.key() == ("func", name, ("col", 0))
    units = {"year": "to_start_of_year", "quarter": "to_start_of_quarter", "month": "to_start_of_month", "day": "to_start_of_day",
             "hour": "to_start_of_hour", "minute": "to_start_of_minute", "second": "to_start_of_second"}
    for u, f in units.items():
        assert X.date_trunc(u, e).name == f and X.date_trunc(u.upper(), e).name == f
    for u, f in (("year", "to_year"), ("quarter", "to_quarter"), ("month", "to_month"), ("day", "to_day_of_month"), ("hour", "to_hour"),
                 ("minute", "to_minute"), ("second", "to_second"), ("week", "to_week_of_year"), ("dow", "to_day_of_week"),
                 ("doy", "to_day_of_year"), ("epoch", "to_unix_timestamp")):
        assert X.extract(u, e).name == f
    for bad in (lambda: X.date_trunc("week", e), lambda: X.extract("century", e), lambda: e.func("to_date")):
        with pytest.raises(ValueError):
            bad()


def test_python_program_marshalling():
    d = X.col(0)
    prog = X.ExprProgram([X.to_year(d) * 100 + X.to_month(d), X.to_yyyymm(d), X.length(X.col(1)), X.date_trunc("month", d)],
                         [column_of(col.Date), column_of(col.String.wrap_nullable())])
    assert prog.struct.reserved == 0
    ops = [(n.op, n.index) for n in prog.nodes]
    assert (abi.EXPR_FUNC, abi.EXPR_FUNCS["to_year"]) in ops and (abi.EXPR_FUNC, abi.EXPR_FUNCS["length"]) in ops
    assert prog.result_types() == [col.UInt64, col.UInt32, col.UInt64.wrap_nullable(), col.Date]
    # equal subtrees share one evaluation
    prog = X.ExprProgram([X.to_year(d), X.to_year(d) * 2], [column_of(col.Date)])
    assert [n.op for n in prog.nodes].count(abi.EXPR_FUNC) == 1
