"""An independent reference for predicate programs: SQL three-valued logic over host Columns.

Written from SQL's rules and the contract of include/dbgpu_agg.h, not from the kernels or the
oracle: it walks the `Pred` tree itself (never the postfix program) and compares cells as plain
Python values.

  * a comparison with a NULL operand is NULL; AND / OR / NOT are Kleene's; IS [NOT] NULL is never NULL
  * integers, Date, Timestamp and Decimal128 compare as Python ints (Decimal128 unscaled: column
    and constant are at the column's scale), Boolean as 0 / 1
  * strings compare as Python `bytes`: unsigned bytewise, a proper prefix sorts first
  * floats compare in the header's total order: NaN equals NaN and is greater than everything
    else, -0.0 equals 0.0; a Float32 cell widens exactly to a Python float (a double)
  * a row is selected only when the predicate is TRUE
"""
import math
import operator
from decimal import Decimal

import numpy as np

from databend_amd import abi
from databend_amd.filter import _Bin, _Cmp, _CmpCols, _Un

FALSE, TRUE, NULL = 0, 1, 2

_OPS = {"=": operator.eq, "==": operator.eq, "<>": operator.ne, "!=": operator.ne, "<": operator.lt,
        "<=": operator.le, ">": operator.gt, ">=": operator.ge}
_FLOATS = (abi.FLOAT32, abi.FLOAT64)
# every value of these fits an int64, so numpy compares them exactly
_I64_EXACT = (abi.INT8, abi.INT16, abi.INT32, abi.INT64, abi.UINT8, abi.UINT16, abi.UINT32, abi.DATE,
              abi.TIMESTAMP, abi.BOOLEAN)


def _float_key(x: float):
    """Total order: every NaN is one value above all others; -0.0 == 0.0 as Python compares them."""
    return (1, 0.0) if math.isnan(x) else (0, x)


def validity(col, n: int) -> np.ndarray:
    if col.validity is None or not col.dtype.nullable:
        return np.ones(n, dtype=bool)
    return np.asarray(col.validity[:n], dtype=bool)


_KEYS = {}  # id(col) -> (col, order keys): the per-row Python values are made once per column


def _order_keys(col) -> list:
    """One comparable Python value per row (the cells of NULL rows are placeholders)."""
    hit = _KEYS.get(id(col))
    if hit is not None and hit[0] is col:
        return hit[1]
    t = col.dtype.type_id
    if t == abi.STRING:
        raw = bytes(np.asarray(col.data, np.uint8))
        o = [int(x) for x in col.offsets]
        keys = [raw[o[i]:o[i + 1]] for i in range(len(o) - 1)]
    elif t == abi.DECIMAL128:
        raw = bytes(np.asarray(col.data, np.uint8))
        keys = [int.from_bytes(raw[16 * i:16 * i + 16], "little", signed=True) for i in range(len(raw) // 16)]
    elif t in _FLOATS:
        keys = [_float_key(float(x)) for x in col.data]  # float(np.float32) widens exactly
    elif t == abi.BOOLEAN:
        keys = [1 if x else 0 for x in col.data]
    else:
        keys = [int(x) for x in col.data]
    _KEYS[id(col)] = (col, keys)
    return keys


def _const_key(col, const):
    t = col.dtype.type_id
    if t == abi.STRING:
        return const.encode() if isinstance(const, str) else bytes(const)
    if t in _FLOATS:
        return _float_key(float(const))
    if t == abi.DECIMAL128 and isinstance(const, Decimal):
        return int(const.scaleb(col.dtype.scale))
    return int(const)


def _tri(truth: np.ndarray, valid: np.ndarray) -> np.ndarray:
    return np.where(valid, np.where(truth, TRUE, FALSE), NULL).astype(np.uint8)


def _cmp_const(col, op: str, const, n: int) -> np.ndarray:
    f = _OPS[op]
    ck = _const_key(col, const)
    if col.dtype.type_id in _I64_EXACT and -(1 << 63) <= ck < (1 << 63):
        truth = f(np.asarray(col.data[:n]).astype(np.int64), np.int64(ck))
    else:
        keys = _order_keys(col)
        truth = np.fromiter((f(keys[i], ck) for i in range(n)), dtype=bool, count=n)
    return _tri(truth, validity(col, n))


def _cmp_cols(a, op: str, b, n: int) -> np.ndarray:
    assert a.dtype.type_id == b.dtype.type_id and a.dtype.scale == b.dtype.scale, "columns of one type only"
    f = _OPS[op]
    if a.dtype.type_id in _I64_EXACT:
        truth = f(np.asarray(a.data[:n]).astype(np.int64), np.asarray(b.data[:n]).astype(np.int64))
    else:
        ka, kb = _order_keys(a), _order_keys(b)
        truth = np.fromiter((f(ka[i], kb[i]) for i in range(n)), dtype=bool, count=n)
    return _tri(truth, validity(a, n) & validity(b, n))


def evaluate(pred, cols, n: int) -> np.ndarray:
    """Per-row value of the predicate tree in {FALSE, TRUE, NULL} (uint8)."""
    if isinstance(pred, _Cmp):
        return _cmp_const(cols[pred.col], pred.op, pred.const, n)
    if isinstance(pred, _CmpCols):
        return _cmp_cols(cols[pred.a], pred.op, cols[pred.b], n)
    if isinstance(pred, _Bin):
        a, b = evaluate(pred.a, cols, n), evaluate(pred.b, cols, n)
        if pred.op == abi.PRED_AND:  # FALSE wins, then NULL
            return np.where((a == FALSE) | (b == FALSE), FALSE, np.where((a == NULL) | (b == NULL), NULL, TRUE)).astype(np.uint8)
        assert pred.op == abi.PRED_OR  # TRUE wins, then NULL
        return np.where((a == TRUE) | (b == TRUE), TRUE, np.where((a == NULL) | (b == NULL), NULL, FALSE)).astype(np.uint8)
    assert isinstance(pred, _Un)
    if pred.op == abi.PRED_NOT:
        a = evaluate(pred.a, cols, n)
        return np.where(a == NULL, NULL, np.where(a == TRUE, FALSE, TRUE)).astype(np.uint8)
    if pred.op == abi.PRED_TRUE:
        return np.full(n, TRUE, dtype=np.uint8)
    v = validity(cols[pred.col], n)
    if pred.op == abi.PRED_IS_NULL:
        return np.where(v, FALSE, TRUE).astype(np.uint8)
    assert pred.op == abi.PRED_IS_NOT_NULL
    return np.where(v, TRUE, FALSE).astype(np.uint8)


def select(pred, cols, n: int) -> np.ndarray:
    return np.flatnonzero(evaluate(pred, cols, n) == TRUE).astype(np.uint32)


_GROUPS = {}  # ids of the key columns -> (key columns, group code per row, key tuple per code)


def _group_codes(keys):
    """Per-row group number and the key tuple (None for NULL) of each group, made once per key set."""
    ident = tuple(id(k) for k in keys)
    hit = _GROUPS.get(ident)
    if hit is not None and all(a is b for a, b in zip(hit[0], keys)):
        return hit[1], hit[2]
    index = {}
    codes = np.fromiter((index.setdefault(t, len(index)) for t in zip(*[k.values() for k in keys])), dtype=np.int64)
    _GROUPS[ident] = (list(keys), codes, list(index))
    return codes, list(index)


def _int_arg(col, n_rows: int):
    """An integer argument column as int64 values + validity; its sums cannot leave int64."""
    v = np.asarray(col.data).astype(np.int64)
    assert np.issubdtype(np.asarray(col.data).dtype, np.integer) and int(np.abs(v).max(initial=0)) * max(1, n_rows) < 2**63
    return v, validity(col, len(v))


def group_reference(mask, keys, args) -> dict:
    """GROUP BY keys over the rows where mask is true: key tuple (None for NULL) ->
    (COUNT(*), SUM(args[0])).  SUM skips NULL arguments and is None (NULL) for a group with none
    left; without args it is None."""
    codes, uniq = _group_codes(keys)
    rows = np.flatnonzero(np.asarray(mask, dtype=bool))
    counts = np.bincount(codes[rows], minlength=len(uniq))
    sums = present = None
    if args:
        v, ok = _int_arg(args[0], len(codes))
        rows_ok = rows[ok[rows]]
        sums = np.zeros(len(uniq), dtype=np.int64)
        np.add.at(sums, codes[rows_ok], v[rows_ok])
        present = np.bincount(codes[rows_ok], minlength=len(uniq))
    return {uniq[g]: (int(counts[g]), int(sums[g]) if args and present[g] else None)
            for g in np.flatnonzero(counts)}


def group_min(mask, keys, arg) -> dict:
    """key tuple -> MIN(arg) over the rows where mask is true (None when every argument is NULL)."""
    codes, uniq = _group_codes(keys)
    rows = np.flatnonzero(np.asarray(mask, dtype=bool))
    v, ok = _int_arg(arg, 1)
    rows_ok = rows[ok[rows]]
    mins = np.full(len(uniq), np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(mins, codes[rows_ok], v[rows_ok])
    present = np.bincount(codes[rows_ok], minlength=len(uniq))
    return {uniq[g]: int(mins[g]) if present[g] else None for g in np.flatnonzero(np.bincount(codes[rows], minlength=len(uniq)))}


def result_dict(keys, aggs) -> dict:
    """Result columns of an aggregate (key columns, aggregate columns) -> key tuple -> tuple of
    the aggregates' values, in Python values (None for NULL)."""
    kv = [k.values() for k in keys]
    av = [a.values() for a in aggs]
    n = len(kv[0]) if kv else 0
    out = {tuple(k[i] for k in kv): tuple(a[i] for a in av) for i in range(n)}
    assert len(out) == n, "a group appears twice"
    return out
