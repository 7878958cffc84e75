"""An exact reference for GROUP BY with COUNT / SUM / AVG / sql_avg / MIN / MAX, in plain Python
(int, fractions.Fraction, struct) over lists of rows: independent of the oracle and of the library.

Values: integers, Date, Timestamp and Decimal128 (the scaled integer) are Python ints; Float32 and
Float64 are their raw bit patterns as ints (so a NaN's sign and payload and the sign of a zero
survive); String keys are bytes; NULL is None.  Types are databend_amd.column.DataType values,
used as descriptors only.

Semantics, from the reference sources (paths as in oracle/dbagg_oracle.cpp: FUN =
src/query/functions/src/aggregates, EXP = src/query/expression/src, EAGG = EXP/aggregate):

  integers   SUM is a wrapping `+=` on i64 / u64 (FUN/aggregate_sum.rs:64-113; release builds have
             overflow checks off); AVG is `value as f64 / count as f64` (FUN/aggregate_avg.rs:38-99).
  Decimal128 SUM is an i128 `+=` (wrapping), range-checked against +-(10^38 - 1) when the input
             precision is <= 18 (FUN/aggregate_sum.rs:115-170, 203-222).  AVG checks the same range
             when the precision is > 18, then value.checked_mul(10^scale_add).checked_div(count),
             truncating (FUN/aggregate_avg.rs:113-201, 235).  sql_avg is the planner's
             sum / count with do_round_div: (sum * 10^k +- count / 2) / count truncated, low 128
             bits (EXP/types/decimal.rs:480-489).
  floats     SUM / AVG accumulate in f64 from +0.0 (NumberSumState<f64>::default,
             FUN/aggregate_sum.rs:64-113); AVG is the IEEE quotient by the count.
             MIN / MAX replace the state when `l.partial_cmp(r)` is Greater / Less over
             OrderedFloat (FUN/aggregate_scalar_state.rs:78-93): every NaN is one value above all
             others, -0.0 equals +0.0 — so which zero a group holding both keeps depends on the
             row order (:183-186 keep the left operand when nothing changes).
  float keys the group hash canonicalises NaN and hashes every other value by its bits
             (EAGG/group_hash.rs:238-258): every NaN is one group, -0.0 and +0.0 are two.
  NULLs      a nullable argument's NULL rows are skipped and a group without a valid row gives
             NULL (FUN/adaptors/aggregate_null_unary_adaptor.rs); COUNT(arg) counts valid rows.

A float SUM here is exact: aggregate() asserts for every all-finite group that the addends share
a quantum 2^e with sum(|v|) / 2^e < 2^53, so every partial sum in every order is representable and
the expected bits are unique.  A case that breaks the condition is a bug in the case.
"""
import struct
from fractions import Fraction
from types import SimpleNamespace
from typing import List, Optional, Sequence, Tuple

from databend_amd import abi
from tests.pp_edges import result_dtype

OVERFLOW = "overflow"      # a result the reference reports as ErrorCode::Overflow (DecimalOverflow)


class _EitherZero:
    """Expected MIN / MAX of a group holding both zeros whose winner is a zero: -0.0 or +0.0."""
    def __repr__(self):
        return "EITHER_ZERO"


EITHER_ZERO = _EitherZero()

F64_NAN, F32_NAN = 0x7FF8000000000000, 0x7FC00000
I128_MAX, I128_MIN = 2**127 - 1, -2**127
DEC_MAX = 10**38 - 1
INT_TYPES = (abi.INT8, abi.INT16, abi.INT32, abi.INT64, abi.UINT8, abi.UINT16, abi.UINT32, abi.UINT64, abi.DATE, abi.TIMESTAMP)
UNSIGNED = (abi.UINT8, abi.UINT16, abi.UINT32, abi.UINT64)
FLOATS = (abi.FLOAT32, abi.FLOAT64)


# ---- float bit patterns ---------------------------------------------------------------------
def is_float(dt) -> bool:
    return dt.type_id in FLOATS


def f64_bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def bits_f64(b: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def is_nan_bits(dt, b: int) -> bool:
    if dt.type_id == abi.FLOAT32:
        return (b & 0x7F800000) == 0x7F800000 and (b & 0x007FFFFF) != 0
    return (b & 0x7FF0000000000000) == 0x7FF0000000000000 and (b & 0x000FFFFFFFFFFFFF) != 0


def is_zero_bits(dt, b: int) -> bool:
    return (b & (0x7FFFFFFF if dt.type_id == abi.FLOAT32 else 0x7FFFFFFFFFFFFFFF)) == 0


def to_f64(dt, b: int) -> float:
    """The f64 a non-NaN Float32 / Float64 bit pattern widens to (exact)."""
    if dt.type_id == abi.FLOAT32:
        return struct.unpack("<f", struct.pack("<I", b))[0]
    return bits_f64(b)


def canonical_key(dt, v):
    """What identifies a key value's group: canonical bits for floats (EAGG/group_hash.rs:238-258)."""
    if v is not None and is_float(dt) and is_nan_bits(dt, v):
        return F32_NAN if dt.type_id == abi.FLOAT32 else F64_NAN
    return v


def wrap(v: int, bits: int, signed: bool) -> int:
    v &= (1 << bits) - 1
    return v - (1 << bits) if signed and v >> (bits - 1) else v


def trunc_div(a: int, b: int) -> int:
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


# ---- one group's state -> result ------------------------------------------------------------
def float_sum(dt, values: Sequence[int]) -> float:
    """The f64 every order of IEEE additions from +0.0 gives for these addends (module docstring)."""
    if any(is_nan_bits(dt, b) for b in values):
        return bits_f64(F64_NAN)
    xs = [to_f64(dt, b) for b in values]
    inf = {x for x in xs if x in (float("inf"), float("-inf"))}
    fin = [Fraction(x) for x in xs if x not in inf]
    if len(inf) == 2:
        return bits_f64(F64_NAN)
    total, mag = sum(fin, Fraction(0)), sum((abs(f) for f in fin), Fraction(0))
    if inf:
        assert mag < Fraction(2)**1023, "finite partial sums could reach the other infinity"
        return inf.pop()
    nz = [f for f in fin if f != 0]
    if not nz:
        # +0.0 + -0.0 = +0.0 in round-to-nearest, and the state starts at +0.0
        return 0.0
    # the largest 2^e dividing every addend: numerator's trailing zeros minus log2(denominator)
    e = min((f.numerator & -f.numerator).bit_length() - 1 - (f.denominator.bit_length() - 1) for f in nz)
    q = Fraction(2)**e
    assert e >= -1074 and mag / q < 2**53, "float SUM case is not exact in every order"
    if abs(total) >= Fraction(2)**1024:
        assert all(f > 0 for f in nz) or all(f < 0 for f in nz), "overflow with mixed signs"
        return float("inf") if total > 0 else float("-inf")
    assert mag < Fraction(2)**1024, "a partial sum could overflow"
    out = float(total)
    assert Fraction(out) == total
    return out


def float_div(s: float, n: int) -> float:
    return s / float(n)  # IEEE binary64 division; n >= 1


def _minmax_float(dt, values, is_min):
    nn = [b for b in values if not is_nan_bits(dt, b)]
    if is_min:
        if not nn:
            return F32_NAN if dt.type_id == abi.FLOAT32 else F64_NAN
        best = min(to_f64(dt, b) for b in nn)
    else:
        if len(nn) < len(values):  # NaN is the greatest value
            return F32_NAN if dt.type_id == abi.FLOAT32 else F64_NAN
        best = max(to_f64(dt, b) for b in nn)
    winners = {b for b in nn if to_f64(dt, b) == best}
    if len(winners) == 2:  # -0.0 and +0.0 compare equal: the first in row order stays
        return EITHER_ZERO
    return winners.pop()


def _aggregate_group(name, dt, values: List[int]):
    """Result of one aggregate over one group's valid argument values (non-empty), as a plain
    value of the result type, or OVERFLOW."""
    n = len(values)
    t = dt.type_id
    if name in ("min", "max"):
        if is_float(dt):
            return _minmax_float(dt, values, name == "min")
        return min(values) if name == "min" else max(values)
    if is_float(dt):
        s = float_sum(dt, values)
        return f64_bits(s if name == "sum" else float_div(s, n))
    if t == abi.DECIMAL128:
        s = wrap(sum(values), 128, True)
        checked = dt.precision <= 18 if name in ("sum", "sql_avg") else dt.precision > 18
        if checked and not -DEC_MAX <= s <= DEC_MAX:
            return OVERFLOW
        if name == "sum":
            return s
        if name == "avg":
            prod = s * 10**(max(dt.scale, 4) - dt.scale)
            if not I128_MIN <= prod <= I128_MAX:
                return OVERFLOW  # checked_mul
            return trunc_div(prod, n)
        k = max(dt.scale, min(dt.scale + 6, 12)) - dt.scale
        half = n // 2
        return wrap(trunc_div(s * 10**k + (half if s >= 0 else -half), n), 128, True)
    assert t in INT_TYPES, dt
    s = wrap(sum(values), 64, t not in UNSIGNED)
    return s if name == "sum" else f64_bits(float(s) / float(n))


def finalize_state(name, dt, value: int, count: int):
    """merge_result of one SUM / AVG state {value, count} that no row produced (a serialized
    state may carry any count): integers and Decimal128.  Returns a plain value or OVERFLOW."""
    if dt.type_id == abi.DECIMAL128:
        checked = dt.precision <= 18 if name == "sum" else dt.precision > 18
        if checked and not -DEC_MAX <= value <= DEC_MAX:
            return OVERFLOW
        if name == "sum":
            return value
        prod = value * 10**(max(dt.scale, 4) - dt.scale)
        if not I128_MIN <= prod <= I128_MAX:
            return OVERFLOW
        return trunc_div(prod, count)
    return value if name == "sum" else f64_bits(float(value) / float(count))


# ---- GROUP BY -------------------------------------------------------------------------------
def aggregate(key_types, key_rows: Sequence[tuple], aggs: Sequence[Tuple[str, Optional[object], Optional[list]]]):
    """GROUP BY.  key_rows: one tuple of key values per row.  aggs: (function name, argument type
    or None, argument values or None), the type's `nullable` saying whether None may appear.
    Returns (group key tuples in first-appearance order — the first row's own values —,
    [(result type, values)]), a value being an int (float results: bits), None, EITHER_ZERO or
    OVERFLOW."""
    index, first = {}, []
    gid = []
    for r in key_rows:
        ck = tuple(canonical_key(t, v) for t, v in zip(key_types, r))
        if ck not in index:
            index[ck] = len(first)
            first.append(tuple(r))
        gid.append(index[ck])
    G = len(first)
    out = []
    for name, dt, vals in aggs:
        rt = result_dtype(name, None if dt is None else SimpleNamespace(dtype=dt))
        per = [[] for _ in range(G)]
        if vals is None:
            for g in gid:
                per[g].append(0)
        else:
            assert len(vals) == len(gid)
            for g, v in zip(gid, vals):
                assert v is not None or dt.nullable, "NULL in a non-nullable argument"
                if v is not None:
                    per[g].append(v)
        if name == "count":
            out.append((rt, [len(p) for p in per]))
        else:
            out.append((rt, [None if not p else _aggregate_group(name, dt.remove_nullable(), p) for p in per]))
    return first, out


def has_overflow(result_columns) -> bool:
    return any(v is OVERFLOW for _, vals in result_columns for v in vals)


# ---- comparison -----------------------------------------------------------------------------
def assert_exact(got, expected):
    """got, expected: (key types, key tuples, [(result type, values)]) in plain values.  Groups
    are matched by their canonical keys (the group order is not part of the contract).  Every
    value compares bit for bit, but for the two answers the reference itself does not fix:
      1. where a NaN is expected (a result, or a float key's NaN group — the payload row keeps
         the first row's own NaN, EAGG/payload_row.rs), any NaN passes;
      2. EITHER_ZERO — MIN / MAX of a group holding both zeros, the winner a zero: change_if
         (FUN/aggregate_scalar_state.rs:78-93) sees -0.0 == +0.0 and keeps the value that came
         first in row order (:183-186) — passes with either zero.
    There is no tolerance."""
    gt, gk, gc = got
    et, ek, ec = expected
    assert list(gt) == list(et), f"key types {gt} != {et}"
    assert len(gk) == len(ek), f"group count differs: got {len(gk)} expected {len(ek)}"
    assert [t for t, _ in gc] == [t for t, _ in ec], f"result types {[t for t, _ in gc]} != {[t for t, _ in ec]}"
    canon = lambda row: tuple(canonical_key(t, v) for t, v in zip(et, row))
    where = {canon(r): i for i, r in enumerate(gk)}
    assert len(where) == len(gk), "a group came back twice"
    for j, row in enumerate(ek):
        assert canon(row) in where, f"group {row} is missing"
        i = where[canon(row)]
        for t, x, y in zip(et, gk[i], row):
            if not (y is not None and is_float(t) and is_nan_bits(t, y)):
                assert x == y, f"group {row}: key came back as {x!r}"
        for a, ((t, gv), (_, ev)) in enumerate(zip(gc, ec)):
            x, y = gv[i], ev[j]
            if y is EITHER_ZERO:
                ok = x is not None and is_zero_bits(t, x)
            elif y is not None and is_float(t) and is_nan_bits(t, y):
                ok = x is not None and is_nan_bits(t, x)
            else:
                assert y is not OVERFLOW, "an overflowing case has no result to compare"
                ok = x == y
            fmt = (lambda v: hex(v) if isinstance(v, int) and is_float(t) else repr(v))
            assert ok, f"group {row} aggregate {a} ({t}): got {fmt(x)} expected {fmt(y)}"
