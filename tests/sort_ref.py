"""ORDER BY ... LIMIT k by definition: the order stated as a comparator over Python values
(functools.cmp_to_key), for one or several sort columns.  It shares nothing with the kernel's or
the oracle's key encoding: no sign flips, no XOR on raw bits, no byte strings.

  * Columns are compared left to right.
  * Per column NULLs go first or last as `nulls_first` says; DESC does not move them.  Two NULLs
    are equal.
  * Values compare by type, reversed for DESC: integers, Date, Timestamp and Decimal128 as Python
    ints, Boolean False < True, String as Python bytes, floats by IEEE 754 totalOrder.
  * Rows equal on every column come out in ascending row order.

totalOrder is written out as classes, sign and payload read with struct from the stored bytes (a
Float32 never passes through a Python float unless it is finite, so no payload is quietened):

  -NaN (larger payload first) < -inf < negative finite < -0 < +0 < positive finite < +inf
  < +NaN (smaller payload first)
"""
import functools
import struct

import numpy as np

from databend_amd import abi

_FLOAT = {abi.FLOAT32: (4, "<I", "<f", 8, 23), abi.FLOAT64: (8, "<Q", "<d", 11, 52)}


def float_class(raw: bytes, type_id: int):
    """The totalOrder position of one stored float as a tuple that Python compares: (class, rank
    within the class)."""
    width, ifmt, ffmt, ebits, mbits = _FLOAT[type_id]
    bits = struct.unpack(ifmt, raw)[0]
    negative = bits >> (width * 8 - 1) == 1
    exponent = (bits >> mbits) & ((1 << ebits) - 1)
    mantissa = bits & ((1 << mbits) - 1)
    if exponent == (1 << ebits) - 1:
        if mantissa:  # NaN: by payload, away from zero
            return (0, -mantissa) if negative else (7, mantissa)
        return (1, 0) if negative else (6, 0)
    if exponent == 0 and mantissa == 0:
        return (3, 0) if negative else (4, 0)
    value = struct.unpack(ffmt, raw)[0]  # finite and non-zero: exact as a Python float
    return (2, value) if negative else (5, value)


def row_values(column) -> list:
    """One comparable Python value per row, None for NULL."""
    t = column.dtype.type_id
    n = len(column)
    if t in _FLOAT:
        w = _FLOAT[t][0]
        raw = np.ascontiguousarray(column.data).tobytes()
        out = [float_class(raw[i * w:(i + 1) * w], t) for i in range(n)]
    elif t == abi.STRING:
        o = [int(x) for x in column.offsets]
        raw = np.ascontiguousarray(column.data).tobytes()
        out = [raw[o[i]:o[i + 1]] for i in range(n)]
    elif t == abi.DECIMAL128:
        raw = np.ascontiguousarray(column.data).tobytes()
        out = [int.from_bytes(raw[16 * i:16 * i + 16], "little", signed=True) for i in range(n)]
    elif t == abi.BOOLEAN:
        out = [bool(x) for x in column.data]
    else:
        out = [int(x) for x in column.data]
    if column.validity is not None and column.dtype.nullable:
        out = [x if ok else None for x, ok in zip(out, column.validity)]
    return out


def full_order(columns, asc, nulls_first) -> list:
    """Every row index in the stated order."""
    cols = [(row_values(c), bool(a), bool(f)) for c, a, f in zip(columns, asc, nulls_first)]

    def compare(i, j):
        for values, ascending, first in cols:
            x, y = values[i], values[j]
            if x is None or y is None:
                if x is None and y is None:
                    continue
                return -1 if (x is None) == first else 1
            if x == y:
                continue
            less = x < y
            return -1 if less == ascending else 1
        return -1 if i < j else (1 if i > j else 0)

    return sorted(range(len(columns[0])), key=functools.cmp_to_key(compare))


def sort_limit(columns, asc, nulls_first, limit) -> list:
    """The first min(limit, n) row indices (limit None: all)."""
    order = full_order(columns, asc, nulls_first)
    return order if limit is None else order[:max(0, int(limit))]
