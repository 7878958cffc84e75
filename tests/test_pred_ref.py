"""CPU tests of the predicate conformance suite: the reference (tests/pred_ref.py) against
hand-computed answers, the case matrix (tests/pred_cases.py) against its own condition, the
oracle against the reference over the whole matrix, and the library's refusals of malformed
programs — all of which return before the library touches a device."""
import ctypes as C
from decimal import Decimal

import numpy as np
import pytest

from databend_amd import abi
from databend_amd import column as col
from databend_amd.aggregates import AggregateFunctionFactory
from databend_amd.column import Column
from databend_amd.ffi import DbgError, lib
from databend_amd.filter import FilterProgram, and_, cmp, cmp_cols, is_not_null, is_null, not_, or_, true_
from oracle import oracle
from tests import pred_cases as pc
from tests import pred_ref

F, T, N_ = pred_ref.FALSE, pred_ref.TRUE, pred_ref.NULL
FN = AggregateFunctionFactory.instance()


# ---- the reference against answers worked out by hand -----------------------------------
def _tri_column(states):
    return Column.from_bools([s == T for s in states], validity=[s != N_ for s in states])


def test_truth_tables():
    a = _tri_column([F, F, F, T, T, T, N_, N_, N_])
    b = _tri_column([F, T, N_, F, T, N_, F, T, N_])
    A, B = cmp(0, "=", 1), cmp(1, "=", 1)
    ev = lambda p: list(pred_ref.evaluate(p, [a, b], 9))
    assert ev(A) == [F, F, F, T, T, T, N_, N_, N_]
    assert ev(and_(A, B)) == [F, F, F, F, T, N_, F, N_, N_]
    assert ev(or_(A, B)) == [F, T, N_, T, T, T, N_, T, N_]
    assert ev(not_(A)) == [T, T, T, F, F, F, N_, N_, N_]
    assert ev(is_null(0)) == [F, F, F, F, F, F, T, T, T]
    assert ev(is_not_null(0)) == [T, T, T, T, T, T, F, F, F]
    assert ev(true_()) == [T] * 9
    assert list(pred_ref.select(or_(A, B), [a, b], 9)) == [1, 3, 4, 5, 7]


def _one(column, op, const):
    return list(pred_ref.evaluate(cmp(0, op, const), [column], len(column)))


def test_nan_family():
    nan, inf = float("nan"), float("inf")
    neg_nan = np.array([0xFFF8000000000001], np.uint64).view(np.float64)[0]
    c = Column.from_numbers(col.Float64, [nan, neg_nan, inf, -inf, 0.0, -0.0, 5e-324, 1.5])
    assert _one(c, "=", nan) == [T, T, F, F, F, F, F, F]
    assert _one(c, "<", nan) == [F, F, T, T, T, T, T, T]
    assert _one(c, ">=", nan) == [T, T, F, F, F, F, F, F]
    assert _one(c, ">", inf) == [T, T, F, F, F, F, F, F]
    assert _one(c, "<=", inf) == [F, F, T, T, T, T, T, T]
    assert _one(c, "=", 0.0) == [F, F, F, F, T, T, F, F]
    assert _one(c, "=", -0.0) == [F, F, F, F, T, T, F, F]
    assert _one(c, "<", 0.0) == [F, F, F, T, F, F, F, F]
    assert _one(c, ">", -0.0) == [T, T, T, F, F, F, T, T]
    assert _one(c, "<>", nan) == [F, F, T, T, T, T, T, T]
    assert _one(c, "<=", -inf) == [F, F, F, T, F, F, F, F]
    f32 = Column.from_numbers(col.Float32, [np.float32(0.1), np.float32(1e-45), np.float32(nan)])
    assert _one(f32, "=", float(np.float32(0.1))) == [T, F, F]
    assert _one(f32, "<", 0.1) == [F, T, F]  # float32(0.1) widens to a double above 0.1
    assert _one(f32, ">", 0.0) == [T, T, T]


def test_uint64_high_bit_family():
    c = Column.from_numbers(col.UInt64, np.array([0, 1, 2**63 - 1, 2**63, 2**63 + 1, 2**64 - 1], dtype=np.uint64))
    assert _one(c, "<", 2**63) == [T, T, T, F, F, F]
    assert _one(c, ">=", 2**63) == [F, F, F, T, T, T]
    assert _one(c, ">", 2**63 - 1) == [F, F, F, T, T, T]
    assert _one(c, "=", 2**64 - 1) == [F, F, F, F, F, T]
    assert _one(c, "<", 2**64 - 1) == [T, T, T, T, T, F]
    assert _one(c, ">", 0) == [F, T, T, T, T, T]
    assert _one(c, "<=", 0) == [T, F, F, F, F, F]
    assert _one(c, "<>", 2**63) == [T, T, T, F, T, T]
    assert _one(c, "<=", 2**63) == [T, T, T, T, F, F]
    assert _one(c, ">", 2**63) == [F, F, F, F, T, T]
    assert _one(c, ">=", 1) == [F, T, T, T, T, T]
    assert _one(c, "=", 2**63 - 1) == [F, F, T, F, F, F]
    d = Column.from_numbers(col.UInt64, np.array([2**64 - 1, 1, 2**63, 5], dtype=np.uint64))
    e = Column.from_numbers(col.UInt64, np.array([1, 2**64 - 1, 2**63 - 1, 5], dtype=np.uint64))
    assert list(pred_ref.evaluate(cmp_cols(0, ">", 1), [d, e], 4)) == [T, F, T, F]


def test_decimal128_sign_and_low_word_family():
    hi = 5 << 64
    vals = [-10**38 + 1, -hi + 2**63, -2**64, -2**63, -1, 0, 2**63 - 1, 2**63, hi + 2**63 - 1, hi + 2**63, 10**38 - 1]
    c = Column.from_decimals(38, 6, vals)
    assert _one(c, "<", 0) == [T, T, T, T, T, F, F, F, F, F, F]
    assert _one(c, ">", -1) == [F, F, F, F, F, T, T, T, T, T, T]
    assert _one(c, "=", -1) == [F, F, F, F, T, F, F, F, F, F, F]
    assert _one(c, "<", 2**63) == [T, T, T, T, T, T, T, F, F, F, F]  # low word's top bit: not a sign
    assert _one(c, ">=", 2**63) == [F, F, F, F, F, F, F, T, T, T, T]
    assert _one(c, "<", hi + 2**63) == [T, T, T, T, T, T, T, T, T, F, F]  # equal high words
    assert _one(c, ">", hi + 2**63 - 1) == [F, F, F, F, F, F, F, F, F, T, T]
    assert _one(c, "<=", -hi + 2**63) == [T, T, F, F, F, F, F, F, F, F, F]  # negative high word
    assert _one(c, ">", -2**64) == [F, F, F, T, T, T, T, T, T, T, T]
    assert _one(c, "<", -2**63) == [T, T, T, F, F, F, F, F, F, F, F]
    assert _one(c, "=", 10**38 - 1) == [F] * 10 + [T]
    assert _one(c, "<>", -10**38 + 1) == [F] + [T] * 10
    money = Column.from_decimals(15, 2, [-150, 0, 149, 150, 151])
    assert _one(money, "<", Decimal("1.50")) == [T, T, T, F, F]  # a Decimal constant is scaled by the column
    assert _one(money, "<", 150) == [T, T, T, F, F]  # an int constant is already unscaled


def test_string_prefix_and_high_byte_family():
    c = Column.from_strings([b"", b"a", b"a\x00", b"ab", b"a\x7f", b"a\x80", b"a\xff", b"b", b"prefix__", b"prefix__x"])
    assert _one(c, "=", b"") == [T] + [F] * 9
    assert _one(c, ">", b"") == [F] + [T] * 9
    assert _one(c, "<", b"a") == [T] + [F] * 9
    assert _one(c, ">", b"a") == [F, F] + [T] * 8  # "a" is a proper prefix of everything after it
    assert _one(c, "<", b"a\x00") == [T, T] + [F] * 8
    assert _one(c, "<", b"a\x80") == [T, T, T, T, T, F, F, F, F, F]  # 0x80 sorts above 0x7f and 'b': unsigned bytes
    assert _one(c, ">", b"a\x7f") == [F, F, F, F, F, T, T, T, T, T]
    assert _one(c, ">=", b"a\xff") == [F, F, F, F, F, F, T, T, T, T]
    assert _one(c, "<", b"b") == [T] * 7 + [F] * 3
    assert _one(c, "<", b"prefix__x") == [T] * 9 + [F]
    assert _one(c, "<=", b"prefix__") == [T] * 9 + [F]
    assert _one(c, "<", b"prefix__") == [T] * 8 + [F, F]
    assert _one(c, ">", b"prefix_") == [F] * 8 + [T, T]
    n = Column.from_strings([b"a", b"", b"b"], validity=[True, False, True])
    assert _one(n, "=", b"") == [F, N_, F]
    assert _one(n, "<>", b"") == [T, N_, T]


def test_signed_widths_and_out_of_range_constants():
    c = Column.from_numbers(col.Int8, [-128, -1, 0, 127])
    assert _one(c, "<", 0) == [T, T, F, F]
    assert _one(c, ">", -129) == [T, T, T, T]
    assert _one(c, "<", 128) == [T, T, T, T]
    assert _one(c, "=", 128) == [F, F, F, F]
    assert _one(c, "<=", -128) == [T, F, F, F]
    u = Column.from_numbers(col.UInt8, [0, 127, 128, 255])
    assert _one(u, ">", 127) == [F, F, T, T]
    assert _one(u, "<", 256) == [T, T, T, T]
    b = Column.from_bools([False, True, True], validity=[True, True, False])
    assert _one(b, "=", 1) == [F, T, N_]
    assert _one(b, "<", 1) == [T, F, N_]


def test_group_reference_by_hand():
    k1 = Column.from_numbers(col.Int32, [1, 1, 2, 2, 1])
    k2 = Column.from_strings([b"x", b"x", b"", b"y", b"x"], validity=[True, True, False, True, True])
    v = Column.from_numbers(col.Int64, [10, 20, 30, 40, 50], validity=[True, False, False, True, True])
    got = pred_ref.group_reference(np.array([True, True, True, False, True]), [k1, k2], [v])
    assert got == {(1, b"x"): (3, 60), (2, None): (1, None)}
    assert pred_ref.group_min(np.array([True, True, True, False, True]), [k1, k2], v) == {(1, b"x"): 10, (2, None): None}
    assert pred_ref.group_reference(np.zeros(5, bool), [k1], [v]) == {}


# ---- the matrix ------------------------------------------------------------------------------


def test_matrix_condition():
    """Every (type, operator) has a constant case and a column-against-column case whose
    selection is neither empty nor everything; the random programs reach the program limits."""
    for name in pc.TYPES:
        for maker in (lambda: pc.const_cases(name, False) + pc.const_cases(name, True), lambda: pc.colcol_cases(name)):
            partial = set()
            for _, cols, p in maker():
                k = len(pred_ref.select(p, cols, pc.N))
                if 0 < k < pc.N:
                    partial.add(p.op)
            assert partial == set(pc.OPS), (name, set(pc.OPS) - partial)
    rnd = pc.random_cases()
    assert len(rnd) == 200
    sizes = [pc.count_nodes(p) for _, _, p in rnd]
    assert max(sizes) == pc.MAX_NODES and sum(s == pc.MAX_NODES for s in sizes) >= 10
    assert any(len(pc.columns_used(p)) == pc.MAX_COLS for _, _, p in rnd)
    for name in pc.TYPES:  # one null in the first and in the last row of every nullable column
        v = pc.column(name, True).validity
        assert not v[0] and not v[-1] and 0.05 < 1 - v.mean() < 0.15


def test_matrix_pool_values_are_present():
    for name in pc.INT_TYPES:
        lo, hi = pc._INT_RANGE[name]
        vals = set(pc.column(name, False).values())
        assert {lo, hi, 0, 1, pc.PRESENT} <= vals and pc.ABSENT not in vals, name
    u = set(pc.column("UInt64", False).values())
    assert {2**63 - 1, 2**63, 2**64 - 1} <= u
    for name in ("Float32", "Float64"):
        d = pc.column(name, False).data
        assert np.isnan(d).any() and np.isinf(d).any() and (np.signbit(d) & (d == 0)).any() and (~np.signbit(d) & (d == 0)).any()
        assert (d == np.finfo(d.dtype).smallest_subnormal).any()
    assert set(pc.column("String", False).values()) == set(pc.STRING_POOL)
    assert set(pc.column("Decimal128(38,6)", False).values()) == set(pc.DECIMAL_POOLS["Decimal128(38,6)"])
    for c in pc.float_constants("Float32"):
        assert np.isnan(c) or float(np.float32(c)) == c  # exactly float32 values


def test_de_morgan_holds_in_the_reference():
    by_id = {i: (cols, p) for i, cols, p in pc.logic_cases()}
    for lhs, rhs in pc.DEMORGAN:
        (cols, p), (_, q) = by_id["logic " + lhs], by_id["logic " + rhs]
        assert np.array_equal(pred_ref.evaluate(p, cols, pc.N), pred_ref.evaluate(q, cols, pc.N))


PARTS = 10  # the matrix is built when the first of these runs, not at collection


@pytest.mark.parametrize("part", range(PARTS))
def test_oracle_matches_reference(part):
    """pred_ref.select == oracle.filter_select, exactly, over the whole matrix."""
    for cid, cols, p in pc.all_cases()[part::PARTS]:
        got = oracle.filter_select(FilterProgram(p, [c.to_abi() for c in cols]), pc.N)
        assert np.array_equal(got, pred_ref.select(p, cols, pc.N)), cid


def test_oracle_aggregate_matches_group_reference():
    c = pc.agg_inputs()
    keys = [c["k_i32"], c["k_str"]]
    specs = [(FN.get("count").to_abi(), None), (FN.get("sum", [], [col.Int64]).to_abi(), c["v"])]
    for cid, fcols, p in pc.generic_agg_cases():
        ok, oa = oracle.aggregate(keys, specs, filter_program=FilterProgram(p, [x.to_abi() for x in fcols]), threads=2)
        mask = pred_ref.evaluate(p, fcols, pc.N_AGG) == T
        assert pred_ref.result_dict(ok, oa) == pred_ref.group_reference(mask, keys, [c["v"]]), cid


# ---- refusals: every one returns before the library touches a device or a column pointer -----
def _abi_col(dt: col.DataType, n=4) -> abi.dbg_column:
    c = abi.dbg_column()
    c.dt = dt.to_abi()
    c.len = n  # data / offsets / validity stay null: a refusal never reads them
    return c


def _select_rc(nodes, cols, n_cols=None):
    """dbg_filter_select on a raw program: (status, message)."""
    arr = (abi.dbg_pred_node * max(1, len(nodes)))()
    for i, d in enumerate(nodes):
        for k, v in d.items():
            setattr(arr[i], k, v)
    carr = (abi.dbg_column * max(1, len(cols)))(*cols)
    f = abi.dbg_filter(arr, len(nodes), len(cols) if n_cols is None else n_cols, carr)
    sel = (C.c_uint32 * 4)()
    n = C.c_uint64()
    rc = lib().dbg_filter_select(C.byref(f), 4, sel, C.byref(n), None)
    return rc, lib().dbg_last_error().decode()


def _orc_rc(nodes, cols):
    arr = (abi.dbg_pred_node * len(nodes))()
    for i, d in enumerate(nodes):
        for k, v in d.items():
            setattr(arr[i], k, v)
    carr = (abi.dbg_column * len(cols))(*cols)
    f = abi.dbg_filter(arr, len(nodes), len(cols), carr)
    sel = (C.c_uint32 * 4)()
    n = C.c_uint64()
    return oracle.lib().orc_filter_select(C.byref(f), 4, sel, C.byref(n)), oracle.lib().orc_last_error().decode()


LEAF = dict(op=abi.PRED_IS_NULL, col=0)
MISMATCHES = [("type", col.String, col.Int32), ("type", col.Int64, col.UInt64), ("type", col.Int32, col.Date),
              ("scale", col.Decimal128(38, 6), col.Decimal128(38, 2))]


@pytest.mark.parametrize("what,a,b", MISMATCHES, ids=lambda v: str(v))
def test_column_comparison_of_unlike_columns_is_refused(what, a, b):
    cols = [_abi_col(a), _abi_col(b)]
    node = dict(op=abi.PRED_CMP_COLS, cmp=abi.CMP_LT, col=0, col2=1)
    rc, msg = _select_rc([node], cols)
    assert rc == abi.DBG_ERR_INVALID and what in msg, (rc, msg)
    rc, msg = _select_rc([LEAF, node, dict(op=abi.PRED_AND)], cols)  # not only as the first node
    assert rc == abi.DBG_ERR_INVALID and what in msg, (rc, msg)
    orc, omsg = _orc_rc([node], cols)
    assert orc == abi.DBG_ERR_INVALID and omsg == msg
    with pytest.raises(DbgError) as e:
        FilterProgram(cmp_cols(0, "<", 1), cols)
    assert e.value.code == abi.DBG_ERR_INVALID and msg in str(e.value)


def test_oracle_aggregate_refuses_unlike_columns():
    k = Column.from_numbers(col.Int32, [1, 2, 3, 4])
    a, b = _abi_col(col.Int64), _abi_col(col.UInt64)
    node = (abi.dbg_pred_node * 1)()
    node[0].op, node[0].cmp, node[0].col, node[0].col2 = abi.PRED_CMP_COLS, abi.CMP_EQ, 0, 1

    class Raw:  # what oracle.aggregate needs of a FilterProgram
        def __init__(self):
            self.carr = (abi.dbg_column * 2)(a, b)
            self.f = abi.dbg_filter(node, 1, 2, self.carr)

        def ptr(self):
            return C.byref(self.f)

    with pytest.raises(oracle.OracleError) as e:
        oracle.aggregate([k], [(FN.get("count").to_abi(), None)], filter_program=Raw())
    assert e.value.code == abi.DBG_ERR_INVALID and "type" in str(e.value)


def test_same_type_column_comparison_is_accepted_by_filter_program():
    FilterProgram(cmp_cols(0, "<", 1), [_abi_col(col.Decimal128(38, 6)), _abi_col(col.Decimal128(15, 6))])
    FilterProgram(cmp_cols(0, "=", 1), [_abi_col(col.String), _abi_col(col.String.wrap_nullable())])


def test_malformed_programs_are_refused():
    i32 = _abi_col(col.Int32)
    rc, msg = _select_rc([LEAF] * 13 + [dict(op=abi.PRED_AND)] * 12, [i32])  # 25 nodes
    assert rc == abi.DBG_ERR_UNSUPPORTED and "too large" in msg
    rc, msg = _select_rc([LEAF], [i32] * 9)  # 9 columns
    assert rc == abi.DBG_ERR_UNSUPPORTED and "too large" in msg
    for bad in (dict(op=abi.PRED_CMP_CONST, col=1), dict(op=abi.PRED_CMP_CONST, col=-1), dict(op=abi.PRED_IS_NULL, col=3),
                dict(op=abi.PRED_CMP_COLS, col=0, col2=1), dict(op=abi.PRED_CMP_COLS, col=0, col2=-1)):
        rc, msg = _select_rc([bad], [i32])
        assert rc == abi.DBG_ERR_INVALID and "out of range" in msg, bad
    rc, msg = _select_rc([LEAF, dict(op=abi.PRED_AND)], [i32])  # AND with one operand
    assert rc == abi.DBG_ERR_INVALID and "malformed" in msg
    rc, msg = _select_rc([dict(op=abi.PRED_NOT)], [i32])  # NOT with none
    assert rc == abi.DBG_ERR_INVALID and "malformed" in msg
    rc, msg = _select_rc([LEAF, LEAF], [i32])  # ends two deep
    assert rc == abi.DBG_ERR_INVALID and "malformed" in msg
    rc, msg = _select_rc([dict(op=8)], [i32])
    assert rc == abi.DBG_ERR_INVALID and "unknown" in msg
    rc, msg = _select_rc([dict(op=-1)], [i32])
    assert rc == abi.DBG_ERR_INVALID and "unknown" in msg
