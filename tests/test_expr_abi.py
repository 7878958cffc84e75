"""dbg_expr_result_type on the host (no device): the types of every number pair, a grid of decimal
(precision, scale) pairs with the clamp at 38 and the scale cap at 12, integer x decimal — all
against tests/expr_ref.py — and every refusal by code and by message: the caps, Decimal256, String,
Boolean, Decimal with Float, and malformed programs.  Then the Python mirror's marshalling."""
import ctypes as C
from decimal import Decimal

import pytest

from databend_amd import abi
from databend_amd import column as col
from databend_amd import expr as X
from databend_amd.column import DataType
from databend_amd.ffi import lib
from tests import expr_ref as R

OPS = {"+": abi.EXPR_PLUS, "-": abi.EXPR_MINUS, "*": abi.EXPR_MULTIPLY}


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


def program(nodes, types, n_outputs=1):
    na = (abi.dbg_expr_node * max(1, len(nodes)))(*nodes)
    ca = (abi.dbg_column * max(1, len(types)))(*[column_of(t) for t in types])
    p = abi.dbg_expr_program(na, len(nodes), len(types), ca, n_outputs, 0)
    p._keep = (na, ca)
    return p


def result_type(p, k=0):
    dt = abi.dbg_datatype()
    rc = lib().dbg_expr_result_type(C.byref(p), k, C.byref(dt))
    return rc, DataType.from_abi(dt), lib().dbg_last_error().decode(errors="replace")


def binary(op, ta, tb):
    return program([node(abi.EXPR_COLUMN, 0), node(abi.EXPR_COLUMN, 1), node(OPS[op]), node(abi.EXPR_STORE, 0)], [ta, tb])


def test_symbols_exist():
    assert hasattr(lib(), "dbg_expr_result_type") and hasattr(lib(), "dbg_expr_eval")
    assert C.sizeof(abi.dbg_expr_node) == 48 and C.sizeof(abi.dbg_expr_program) == 32


@pytest.mark.parametrize("op", "+-*")
def test_number_pairs(op):
    for ta in R.NUMBER_TYPES:
        for tb in R.NUMBER_TYPES:
            for na, nb in ((False, False), (True, False), (False, True)):
                a = ta.wrap_nullable() if na else ta
                b = tb.wrap_nullable() if nb else tb
                rc, t, msg = result_type(binary(op, a, b))
                assert rc == abi.DBG_OK, msg
                assert t == R.result_type(op, a, b), (op, a, b, t)


@pytest.mark.parametrize("op", "+-*")
def test_decimal_grid(op):
    seen_clamp = seen_cap = False
    for pa, sa in R.DECIMAL_GRID:
        for pb, sb in R.DECIMAL_GRID:
            a, b = R.Dec(pa, sa), R.Dec(pb, sb, nullable=True)
            rc, t, msg = result_type(binary(op, a, b))
            assert rc == abi.DBG_OK, msg
            want = R.result_type(op, a, b)
            assert t == want, (op, a, b, t, want)
            seen_clamp |= t.precision == 38
            seen_cap |= op == "*" and sa + sb > 12 and t.scale == max(sa, sb, 12)
        for ti in R.INTS:
            for a, b in ((R.Dec(pa, sa), DataType(ti)), (DataType(ti), R.Dec(pa, sa))):
                rc, t, msg = result_type(binary(op, a, b))
                assert rc == abi.DBG_OK, msg
                assert t == R.result_type(op, a, b), (op, a, b, t)
    assert seen_clamp and (seen_cap or op != "*")


def test_q1_types():
    D = R.Dec(15, 2)
    one = node(abi.EXPR_CONST, dt=DataType(abi.UINT8), i64=1)
    nodes = [node(abi.EXPR_COLUMN, 0), one, node(abi.EXPR_COLUMN, 1), node(abi.EXPR_MINUS), node(abi.EXPR_MULTIPLY),
             node(abi.EXPR_STORE, 0), one, node(abi.EXPR_COLUMN, 2), node(abi.EXPR_PLUS), node(abi.EXPR_MULTIPLY), node(abi.EXPR_STORE, 1)]
    p = program(nodes, [D, D, D], 2)
    assert result_type(p, 0)[:2] == (abi.DBG_OK, R.Dec(31, 4))
    assert result_type(p, 1)[:2] == (abi.DBG_OK, R.Dec(38, 6))
    rc, _, msg = result_type(p, 2)
    assert rc == abi.DBG_ERR_INVALID and "output index" in msg


REFUSED_TYPES = [(col.Decimal256(40, 2), "Decimal256"), (col.String, "String"), (col.Boolean, "Boolean"), (col.Date, "Date"),
                 (col.Timestamp, "Timestamp")]


@pytest.mark.parametrize("t,name", REFUSED_TYPES, ids=[n for _, n in REFUSED_TYPES])
def test_unsupported_operand_types(t, name):
    for p in (binary("+", t, col.Int32), binary("*", col.Int32, t),
              program([node(abi.EXPR_COLUMN, 0), node(abi.EXPR_CONST, dt=t), node(abi.EXPR_PLUS), node(abi.EXPR_STORE, 0)], [col.Int32])):
        rc, _, msg = result_type(p)
        assert rc == abi.DBG_ERR_UNSUPPORTED and name in msg, (rc, msg)


@pytest.mark.parametrize("op", "+-*")
def test_decimal_with_float_is_refused(op):
    for f in (col.Float32, col.Float64):
        for a, b in ((R.Dec(10, 1), f), (f, R.Dec(10, 1))):
            rc, _, msg = result_type(binary(op, a, b))
            assert rc == abi.DBG_ERR_UNSUPPORTED and "Decimal mixed with Float" in msg and R.OP_NAME[op] in msg, msg


def test_null_constant_is_refused():
    p = program([node(abi.EXPR_COLUMN, 0), node(abi.EXPR_CONST, dt=col.Int32.wrap_nullable()), node(abi.EXPR_PLUS), node(abi.EXPR_STORE, 0)],
                [col.Int32])
    rc, _, msg = result_type(p)
    assert rc == abi.DBG_ERR_UNSUPPORTED and "NULL constants" in msg


def test_caps():
    c0, st = node(abi.EXPR_COLUMN, 0), node(abi.EXPR_STORE, 0)
    one = node(abi.EXPR_CONST, dt=DataType(abi.UINT8), i64=1)
    # 64 nodes pass, 65 do not: c0 (1 +)*31 STORE = 1 + 62 + 1
    chain = [c0] + [one, node(abi.EXPR_PLUS)] * 31 + [st]
    assert len(chain) == abi.EXPR_MAX_NODES
    rc, t, msg = result_type(program(chain, [col.Int64]))
    assert rc == abi.DBG_OK and t == col.Int64, msg
    rc, _, msg = result_type(program([c0, one, node(abi.EXPR_PLUS)] + chain[1:], [col.Int64]))
    assert rc == abi.DBG_ERR_UNSUPPORTED and str(abi.EXPR_MAX_NODES) in msg and "nodes" in msg
    # 4 live values pass, 5 do not
    deep = [c0] * 4 + [node(abi.EXPR_PLUS)] * 3 + [st]
    assert result_type(program(deep, [col.Int8]))[0] == abi.DBG_OK
    rc, _, msg = result_type(program([c0] * 5 + [node(abi.EXPR_PLUS)] * 4 + [st], [col.Int8]))
    assert rc == abi.DBG_ERR_UNSUPPORTED and "live values" in msg and str(abi.EXPR_MAX_STACK) in msg
    # 8 independent outputs pass (a stored value nothing takes is not live), 9 do not
    outs = []
    for k in range(abi.EXPR_MAX_OUTPUTS):
        outs += [c0, node(abi.EXPR_CONST, dt=DataType(abi.UINT8), i64=k), node(abi.EXPR_PLUS), node(abi.EXPR_STORE, k)]
    p = program(outs, [col.Int16], abi.EXPR_MAX_OUTPUTS)
    assert [result_type(p, k)[:2] for k in range(abi.EXPR_MAX_OUTPUTS)] == [(abi.DBG_OK, col.Int32)] * abi.EXPR_MAX_OUTPUTS
    rc, _, msg = result_type(program(outs + [c0, node(abi.EXPR_STORE, 8)], [col.Int16], 9))
    assert rc == abi.DBG_ERR_UNSUPPORTED and "outputs" in msg and str(abi.EXPR_MAX_OUTPUTS) in msg
    # 16 columns pass, 17 do not
    assert result_type(program([node(abi.EXPR_COLUMN, 15), st], [col.Int8] * 16))[0] == abi.DBG_OK
    rc, _, msg = result_type(program([c0, st], [col.Int8] * 17))
    assert rc == abi.DBG_ERR_UNSUPPORTED and "columns" in msg and str(abi.EXPR_MAX_COLUMNS) in msg


MALFORMED = [
    ("underflow_operator", [node(abi.EXPR_COLUMN, 0), node(abi.EXPR_PLUS), node(abi.EXPR_STORE, 0)], 1, "underflow"),
    ("underflow_store", [node(abi.EXPR_STORE, 0)], 1, "underflow"),
    ("value_left_over", [node(abi.EXPR_COLUMN, 0), node(abi.EXPR_COLUMN, 0), node(abi.EXPR_STORE, 0)], 1, "left over"),
    ("stored_twice", [node(abi.EXPR_COLUMN, 0), node(abi.EXPR_STORE, 0), node(abi.EXPR_STORE, 0)], 1, "stored twice"),
    ("never_stored", [node(abi.EXPR_COLUMN, 0), node(abi.EXPR_STORE, 0)], 2, "never stored"),
    ("bad_column", [node(abi.EXPR_COLUMN, 1), node(abi.EXPR_STORE, 0)], 1, "column index"),
    ("negative_column", [node(abi.EXPR_COLUMN, -1), node(abi.EXPR_STORE, 0)], 1, "column index"),
    ("bad_output", [node(abi.EXPR_COLUMN, 0), node(abi.EXPR_STORE, 1)], 1, "output index"),
    ("unknown_op", [node(abi.EXPR_COLUMN, 0), node(6), node(abi.EXPR_STORE, 0)], 1, "unknown op"),
    ("no_outputs", [node(abi.EXPR_COLUMN, 0)], 0, "no outputs"),
    ("bad_decimal", [node(abi.EXPR_CONST, dt=DataType(abi.DECIMAL128, 39, 0)), node(abi.EXPR_STORE, 0)], 1, "precision"),
]


@pytest.mark.parametrize("name,nodes,n_out,word", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_malformed_programs(name, nodes, n_out, word):
    rc, _, msg = result_type(program(nodes, [col.Int32], n_out))
    assert rc == abi.DBG_ERR_INVALID and word in msg, (rc, msg)


def test_null_arguments():
    dt = abi.dbg_datatype()
    assert lib().dbg_expr_result_type(None, 0, C.byref(dt)) == abi.DBG_ERR_INVALID
    assert lib().dbg_expr_eval(None, None, 0, None, None) == abi.DBG_ERR_INVALID


# ---- the Python mirror ------------------------------------------------------------------------------
def test_literal_types():
    lt = X.literal_type
    assert [lt(v).type_id for v in (0, 255, 256, 65535, 65536, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1)] == \
        [abi.UINT8, abi.UINT8, abi.UINT16, abi.UINT16, abi.UINT32, abi.UINT32, abi.UINT64, abi.UINT64]
    assert [lt(v).type_id for v in (-1, -128, -129, -32768, -32769, -2 ** 31, -2 ** 31 - 1, -2 ** 63)] == \
        [abi.INT8, abi.INT8, abi.INT16, abi.INT16, abi.INT32, abi.INT32, abi.INT64, abi.INT64]
    assert lt(0.5) == col.Float64
    assert lt(Decimal("0.5")) == R.Dec(1, 1) and lt(Decimal("12.34")) == R.Dec(4, 2) and lt(Decimal("0.05")) == R.Dec(2, 2)
    assert lt(Decimal("7")) == R.Dec(1, 0)
    with pytest.raises(OverflowError):
        lt(2 ** 64)


def test_program_shares_a_stored_subtree():
    price, disc, tax = X.col(0), X.col(1), X.col(2)
    disc_price = price * (1 - disc)
    charge = disc_price * (1 + tax)
    D = R.Dec(15, 2)
    for order in ([disc_price, charge], [charge, disc_price]):
        prog = X.ExprProgram(order, [column_of(D)] * 3)
        ops = [n.op for n in prog.nodes]
        assert ops.count(abi.EXPR_MULTIPLY) == 2 and ops.count(abi.EXPR_STORE) == 2 and len(ops) == 11  # disc_price once
        types = prog.result_types()
        assert types == ([R.Dec(31, 4), R.Dec(38, 6)] if order[0] is disc_price else [R.Dec(38, 6), R.Dec(31, 4)])
    # independent outputs, and the same expression twice
    prog = X.ExprProgram([X.col(0) + k for k in range(4)] + [X.col(0) + 1], [column_of(col.Int16)])
    assert prog.result_types() == [col.Int32] * 5
    assert [n.op for n in prog.nodes].count(abi.EXPR_PLUS) == 4
    # constants: the typed fields
    prog = X.ExprProgram([X.col(0) * X.lit(Decimal("0.5")) + X.lit(-3) * X.lit(2.5, col.Float32)], [column_of(R.Dec(10, 1))])
    consts = [n for n in prog.nodes if n.op == abi.EXPR_CONST]
    assert (consts[0].dt.type, consts[0].dt.precision, consts[0].dt.scale, consts[0].i128_lo) == (abi.DECIMAL128, 1, 1, 5)
    assert (consts[1].dt.type, consts[1].i64) == (abi.INT8, -3) and (consts[2].dt.type, consts[2].f64) == (abi.FLOAT32, 2.5)
    with pytest.raises(Exception) as e:
        prog.result_types()
    assert e.value.code == abi.DBG_ERR_UNSUPPORTED  # Decimal with Float
