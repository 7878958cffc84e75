"""Inputs at the value extremes for every insert and merge path of the hash aggregate: small cases
of designed groups (in the style of pp_edges.arg_case), their keys chosen per route, plus crafted
serialized states.  tests/agg_ref.py gives the expected results; tests/test_agg_ref.py pins both
against the oracle on the CPU, tests/test_gpu_agg_values.py runs them on every GPU route.

A case is {"args": [argument types], "aggs": [(function, argument index | None)], "groups":
[{"n": rows, "args": [values per argument], "keys": [key tuple per row] (float-key cases only)}]}
in agg_ref's plain values (floats as bit patterns, decimals as scaled ints, NULL as None).  build()
gives a case the key columns of a key shape, interleaves the groups' rows round-robin (so the lanes
of a wave share a few slots) and returns Columns together with the plain rows.
"""
import functools
import struct
from types import SimpleNamespace

import numpy as np

from databend_amd import abi
from databend_amd import column as col
from databend_amd.column import Column
from tests import agg_ref as R
from tests import pp_edges as E


# ---- plain values <-> Columns ---------------------------------------------------------------
def to_column(dt, values) -> Column:
    t = dt.type_id
    valid = np.array([v is not None for v in values], dtype=bool) if dt.nullable else None
    assert dt.nullable or all(v is not None for v in values)
    filled = [0 if v is None else v for v in values]
    if t == abi.STRING:
        return Column.from_strings([b"" if v is None else v for v in values], validity=valid)
    if t == abi.DECIMAL128:
        c = Column.from_decimals(dt.precision, dt.scale, filled, validity=valid)
        assert c.dtype == dt
        return c
    if t in R.FLOATS:
        u = np.uint32 if t == abi.FLOAT32 else np.uint64
        return Column.from_numbers(dt.remove_nullable(), np.array(filled, dtype=u).view(dt.np_dtype), validity=valid)
    return Column.from_numbers(dt.remove_nullable(), np.array(filled, dtype=dt.np_dtype), validity=valid)


def from_column(c: Column) -> list:
    t = c.dtype.type_id
    if t in R.FLOATS:
        u = np.uint32 if t == abi.FLOAT32 else np.uint64
        out = [int(x) for x in np.ascontiguousarray(c.data).view(u)]
        if c.validity is not None and c.dtype.nullable:
            out = [x if ok else None for x, ok in zip(out, c.validity)]
        return out
    return c.values()


def plain_result(key_cols, agg_cols):
    """(key types, key tuples, [(result type, values)]) of result columns: assert_exact's operand."""
    keys = list(zip(*[from_column(k) for k in key_cols])) if key_cols else []
    return [k.dtype for k in key_cols], keys, [(a.dtype, from_column(a)) for a in agg_cols]


# ---- float pools ----------------------------------------------------------------------------
def _f32(x: float) -> int:
    return struct.unpack("<I", struct.pack("<f", x))[0]


class Pool:
    """Bit patterns of a float type's edge values."""
    def __init__(self, dt):
        f64 = dt.type_id == abi.FLOAT64
        self.dt = dt
        self.sign = 1 << (63 if f64 else 31)
        self.zero, self.nzero = 0, self.sign
        self.sub_min = 1
        self.sub_max = 0x000FFFFFFFFFFFFF if f64 else 0x007FFFFF
        self.norm_min = 0x0010000000000000 if f64 else 0x00800000
        self.v15 = 0x3FF8000000000000 if f64 else 0x3FC00000
        self.maxf = 0x7FEFFFFFFFFFFFFF if f64 else 0x7F7FFFFF
        self.inf = 0x7FF0000000000000 if f64 else 0x7F800000
        self.nan = R.F64_NAN if f64 else R.F32_NAN
        self.neg_nan = 0xFFF8000000000001 if f64 else 0xFFC00001   # negative, with a payload
        self.snan = 0x7FF0000000000001 if f64 else 0x7F800001      # signalling
        self.big = (1000 + 1023) << 52 if f64 else (100 + 127) << 23  # 2^1000 / 2^100
        self.top = 0x7FE0000000000000 if f64 else self.maxf            # 2^1023 / max finite f32
        self.of = (lambda x: R.f64_bits(float(x))) if f64 else _f32
        self.int_bits = 52 if f64 else 23

    def neg(self, b):
        return b | self.sign

    def all(self):
        pos = [self.zero, self.sub_min, self.sub_max, self.norm_min, self.v15, self.maxf, self.inf]
        return pos + [self.neg(b) for b in pos] + [self.nan, self.neg_nan, self.snan]


def _cycle(values, n):
    return [values[i % len(values)] for i in range(n)]


def _pad(values, n, pad):
    return list(values) + [pad] * (n - len(values))


def _holes(values, step, at):
    return [None if i % step == at else v for i, v in enumerate(values)]


def float_case(dt):
    """Arguments [mm, sm, nullable mm, nullable sm] of one float type: `mm` feeds MIN / MAX (any
    value), `sm` feeds SUM / AVG (values whose sum is exact in every order, agg_ref.float_sum)."""
    P = Pool(dt)
    neg = P.neg
    N = 48
    g = []

    def grp(mm, sm, n=N, pad=P.zero, mmn=None, smn=None):
        mm, sm = _cycle(mm, n), _pad(sm, n, pad)
        g.append({"n": n, "args": [mm, sm, _holes(mm, 3, 1) if mmn is None else mmn, _holes(sm, 4, 2) if smn is None else smn]})

    grp([neg(P.v15), neg(P.maxf), neg(P.norm_min), neg(P.sub_min)], [neg(P.v15)] * 7)        # only negatives
    grp([P.nan, P.neg_nan, P.snan], [P.nan, P.neg_nan, P.snan], pad=P.neg_nan)               # only NaN
    grp([P.nzero], [P.nzero], pad=P.nzero)                                                    # only -0.0
    grp([P.nzero, P.zero], [P.nzero, P.zero])                                                 # both zeros
    grp([P.inf, neg(P.inf), P.v15], [P.inf, neg(P.inf), P.v15])                               # both infinities
    grp([neg(P.inf), P.v15, neg(P.maxf)], [P.inf, P.v15, neg(P.v15), P.big])                  # one infinity + finite
    grp([P.sub_min, neg(P.sub_max), P.sub_max], [P.sub_min] * 5 + [neg(P.sub_min)] * 2)      # subnormal sum
    grp([P.sub_max, P.sub_min], [P.sub_max, P.sub_min])                                       # -> smallest normal
    ints = [P.of(2**P.int_bits), P.of(2**P.int_bits - 2), P.of(1)]
    grp(ints, ints)                                                                           # integers below 2^53 / 2^24
    grp([P.top] * 3, [P.top] * 3)                                                             # 3 x 2^1023 (f32: 3 x max)
    grp([neg(P.maxf)], [neg(P.maxf)], n=1, mmn=[neg(P.maxf)], smn=[neg(P.maxf)])              # one row
    grp(P.all(), [P.v15, neg(P.v15), P.v15])                                                  # the whole pool
    grp([P.v15], [P.v15], mmn=[None] * N, smn=[None] * N)                                     # all NULL
    only = [None] * 20 + [neg(P.maxf)] + [None] * (N - 21)
    grp([P.maxf, P.nan], [P.v15], mmn=only, smn=[None if v is None else P.maxf for v in only])  # one valid extreme
    n_dt = dt.wrap_nullable()
    aggs = [("count", None), ("min", 0), ("max", 0), ("sum", 1), ("avg", 1), ("sql_avg", 1),
            ("count", 2), ("min", 2), ("max", 2), ("sum", 3), ("avg", 3)]
    return {"args": [dt, dt, n_dt, n_dt], "aggs": aggs, "groups": g}


# ---- integers -------------------------------------------------------------------------------
INT_SETS = {"int_a": ("Int8", "UInt8", "Int16"), "int_b": ("UInt16", "Int32", "UInt32"), "int_c": ("Int64", "UInt64"),
            "int_d": ("Date", "Timestamp")}
_INT = dict(E.ARG_TYPES, Date=col.Date, Timestamp=col.Timestamp)


def _int_patterns(T):
    """pp_edges.arg_case's value set at a smaller size: only T.min, only T.max (each equal to a
    MIN / MAX state's identity), both, the values either side of the top bit, one row, uniform
    values, the four wrapping bit patterns; and a group whose early and late rows differ in sign."""
    rng = np.random.default_rng(31)
    lo, hi = E.limits(T)
    b = E.bits_of(T)
    below, above = (-1, 0) if E.is_signed(T) else ((1 << (b - 1)) - 1, 1 << (b - 1))
    return [[lo] * 40, [hi] * 45, [lo, hi, hi] * 14, [below, above] * 20, [lo], E._uniform(T, 30, rng),
            [E.as_type(T, p) for p in ((1 << (b - 1)) + 5, 3, (1 << b) - 1, (1 << (b - 1)) - 1)],
            # small positives first, top-bit-set values later: the two partials of a merge hold
            # MIN / MAX states of different sign
            [5] * 20 + [E.as_type(T, -3)] * 20]


def int_case(names):
    """[T, Nullable(T)] per type; groups: _int_patterns, an all-NULL group and groups whose only
    valid value is T.max / T.min."""
    types = [_INT[n] for n in names]
    pats = [_int_patterns(T) for T in types]
    groups = []
    for p in range(len(pats[0])):
        n = len(pats[0][p])
        args = []
        for k in range(len(types)):
            v = pats[k][p]
            args += [v, v if n == 1 else _holes(v, 3, 1)]
        groups.append({"n": n, "args": args})
    for which in (None, 1, 0):
        args = []
        for T in types:
            ext = None if which is None else E.limits(T)[which]
            args += [[0] * 11, [None] * 5 + [ext] + [None] * 5]
        groups.append({"n": 11, "args": args})
    arg_types, aggs = [], [("count", None)]
    for k, T in enumerate(types):
        arg_types += [T, T.wrap_nullable()]
        fns = ("min", "max") if T in (col.Date, col.Timestamp) else ("sum", "avg", "min", "max")  # no SUM of dates
        aggs += [(f, 2 * k) for f in fns] + [("count", 2 * k + 1)] + [(f, 2 * k + 1) for f in fns]
    return {"args": arg_types, "aggs": aggs, "groups": groups}


# ---- decimals -------------------------------------------------------------------------------
def _avg_groups():
    """Sums of -7, -5, 5, 7 over 2 and 3 rows (truncation toward zero, round half away from zero,
    odd and even counts), and the ties +-(k * count + count / 2) at count 2."""
    out = []
    for s in (-7, -5, 5, 7):
        out += [[s - 1, 1], [s - 2, 1, 1]]
    return out + [[10**6, 10**6 + 1], [-10**6, -10**6 - 1]]


def _dec_extreme(dt):
    """The largest value whose AVG survives checked_mul(10^scale_add): 10^p - 1, or at precision
    38 and scale < 4 the checked_mul boundary i128::MAX / 10^scale_add itself."""
    return min(10**dt.precision - 1, R.I128_MAX // 10**(max(dt.scale, 4) - dt.scale))


def decimal_case(types, sql_avg, nullable_of):
    """One argument per type plus a nullable copy of types[nullable_of]; sql_avg: indices that
    take sql_avg (where sum * 10^k stays inside i128)."""
    groups = []

    def add(pattern_of):
        args = [pattern_of(dt) for dt in types]
        m = max(len(a) for a in args)
        args = [_pad(a, m, 0) for a in args]
        nv = args[nullable_of]
        groups.append({"n": m, "args": args + [nv if m <= 3 else _holes(nv, 3, 1)]})

    M = _dec_extreme
    # many rows of the extreme where every partial sum stays in range (precision <= 19); one
    # extreme among zeros at precision 38 (AVG range-checks the sum there)
    add(lambda dt: [M(dt)] * 40 if dt.precision <= 19 else [M(dt)] + [0] * 39)
    add(lambda dt: [-M(dt)] * 40 if dt.precision <= 19 else [-M(dt)] + [0] * 39)
    add(lambda dt: [M(dt), -M(dt)] * (3 if dt.precision <= 19 else 1))  # no order passes +-(10^38 - 1)
    add(lambda dt: [0, -1] * 10)
    add(lambda dt: [M(dt)])
    # add128: carry into the high word, out of it (-1 + 1), and a borrow from it
    add(lambda dt: [2**64 - 1, 1] if dt.precision == 38 else [10**dt.precision - 1] * 2)
    add(lambda dt: [-1, 1])
    add(lambda dt: [-2**64, -1, 2**64 + 5] if dt.precision == 38 else [-(10**dt.precision - 1)] * 2 + [10**dt.precision - 1])
    for vals in _avg_groups():
        add(lambda dt, vals=vals: list(vals))
    n = 11
    groups.append({"n": n, "args": [[0] * n for _ in types] + [[None] * n]})
    for sign in (1, -1):
        groups.append({"n": n, "args": [[1] * n for _ in types] + [[None] * 5 + [sign * M(types[nullable_of])] + [None] * 5]})
    aggs = [("count", None)]
    for k, dt in enumerate(types):
        aggs += [(f, k) for f in ("sum", "avg", "min", "max")] + ([("sql_avg", k)] if k in sql_avg else [])
    k = len(types)
    aggs += [("count", k)] + [(f, k) for f in ("sum", "avg", "min", "max")]
    return {"args": list(types) + [types[nullable_of].wrap_nullable()], "aggs": aggs, "groups": groups}


def dec_wrap_case():
    """SUM over precision 38 leaves i128 and wraps (no range check above precision 18)."""
    dt = col.Decimal128(38, 4)
    M = 10**38 - 1
    groups = [{"n": len(v), "args": [v]} for v in ([M, M], [-M, -M], [M, M, -M, -M], [M] * 7, [-M] * 5 + [M])]
    return {"args": [dt], "aggs": [("count", None), ("sum", 0), ("min", 0), ("max", 0)], "groups": groups}


def dec_avg_overflow_case():
    """AVG over Decimal(38, 0): one past the checked_mul boundary is ErrorCode::Overflow."""
    dt = col.Decimal128(38, 0)
    groups = [{"n": 2, "args": [[5, 7]]}, {"n": 1, "args": [[_dec_extreme(dt) + 1]]}]
    return {"args": [dt], "aggs": [("avg", 0)], "groups": groups, "overflow": True}


def narrow_case(precision, rows, sign):
    """The short-key insert's narrow Decimal sum at its bound: one group, every value
    +-(10^p - 1), COUNT / SUM / AVG."""
    dt = col.Decimal128(precision, 2)
    v = [sign * (10**precision - 1)] * rows
    return {"args": [dt], "aggs": [("count", None), ("sum", 0), ("avg", 0)], "groups": [{"n": rows, "args": [v]}], "batches": 1}


def float_key_case(dt, with_int):
    """A float key holding both zeros, both infinities, three encodings of NaN and a few normals
    (alone, or beside an Int32 key); COUNT, SUM(Int64) and MIN / MAX of the key column itself."""
    P = Pool(dt)
    vals = [[P.zero], [P.nzero], [P.inf], [P.neg(P.inf)], [P.nan, P.neg_nan, P.snan], [P.v15], [P.neg(P.v15)], [P.maxf],
            [P.sub_min], [P.neg(P.sub_min)]]
    groups = []
    for i, enc in enumerate(vals):
        for second in ((7, -1) if with_int else (None,)):
            n = 12 + i
            ks = _cycle(enc, n)
            keys = [(k, second) if with_int else (k,) for k in ks]
            groups.append({"n": n, "keys": keys, "args": [[(i + 1) * (j - 3) for j in range(n)], ks]})
    return {"key_types": [dt, col.Int32] if with_int else [dt], "args": [col.Int64, dt],
            "aggs": [("count", None), ("sum", 0), ("min", 1), ("max", 1)], "groups": groups}


D = col.Decimal128
CASES = {
    "f64": lambda: float_case(col.Float64),
    "f32": lambda: float_case(col.Float32),
    **{k: functools.partial(int_case, v) for k, v in INT_SETS.items()},
    "dec64": lambda: decimal_case([D(4, 2), D(15, 2), D(16, 2), D(18, 2), D(15, 12)], sql_avg=(0, 1, 2, 3, 4), nullable_of=3),
    "dec128": lambda: decimal_case([D(19, 4), D(38, 4), D(38, 0), D(38, 12)], sql_avg=(0, 3), nullable_of=1),
    "dec_wrap": dec_wrap_case,
    "dec_avg_overflow": dec_avg_overflow_case,
    **{f"narrow_{n}_{s}": functools.partial(narrow_case, 16, n, sg) for n in (899, 900, 923) for s, sg in (("pos", 1), ("neg", -1))},
    **{f"narrow_3wg_{s}": functools.partial(narrow_case, 15, 12288, sg) for s, sg in (("pos", 1), ("neg", -1))},
    "fkey64": lambda: float_key_case(col.Float64, False),
    "fkey32": lambda: float_key_case(col.Float32, False),
    "fkey64_i32": lambda: float_key_case(col.Float64, True),
    "fkey32_i32": lambda: float_key_case(col.Float32, True),
}
NARROW = [c for c in CASES if c.startswith("narrow_")]
FLOAT_KEY = [c for c in CASES if c.startswith("fkey")]

# key shape -> (key types, key of group g, key of filler f)
KEY_SHAPES = {
    "i64": ([col.Int64], lambda g: (g - 1,), lambda f: (1000 + 7 * f,)),   # -1: the all-ones packed key
    "ni64": ([col.Int64.wrap_nullable()], lambda g: (None if g == 0 else g,), lambda f: (1000 + f,)),
    "i32_str": ([col.Int32, col.String], lambda g: (g - 1, b"key-%d" % g), lambda f: (f, b"fill")),
    "str": ([col.String], lambda g: (b"s%03d" % g,), lambda f: (b"filler-%d" % f,)),
    "str_str": ([col.String, col.String], lambda g: (b"a%d" % g, b"" if g % 2 else b"zz"), lambda f: (b"f", b"%d" % f)),
    "i64_i32": ([col.Int64, col.Int32], lambda g: (g - 1, -g), lambda f: (1000 + f, f)),
}


def state_words(aggs, arg_types) -> int:
    """State words of a slot holding these aggregates ("State words per function"):
    COUNT 1; SUM 1 (Decimal 2: lo / hi); AVG and sql_avg the sum's words + a count; MIN / MAX 1
    (Decimal above precision 18: sequence word + lo + hi); one shared flags word when a SUM, MIN or
    MAX has a nullable argument."""
    words, flags = 0, 0
    for name, a in aggs:
        dt = None if a is None else arg_types[a]
        dec = dt is not None and dt.type_id == abi.DECIMAL128
        if name == "count":
            words += 1
        elif name in ("min", "max"):
            words += 3 if dec and dt.precision > 18 else 1
        else:
            words += (2 if dec else 1) + (name != "sum")
        if name in ("sum", "min", "max") and dt.nullable:
            flags = 1
    return words + flags


def chunks_of(case_id: str, max_words: int):
    """The case's aggregates as tuples of indices, consecutive ones together while their state
    words stay within max_words (an aggregate wider than that stands alone)."""
    case = CASES[case_id]()
    out, cur = [], []
    for i in range(len(case["aggs"])):
        if cur and state_words([case["aggs"][j] for j in cur + [i]], case["args"]) > max_words:
            out.append(tuple(cur))
            cur = []
        cur.append(i)
    return out + [tuple(cur)]


@functools.lru_cache(maxsize=None)
def build(case_id: str, shape: str = "i64", *, fillers: int = 0, only: tuple = None, nonnull: bool = False, limit: int = None,
          pick: tuple = None):
    """The case's input with the keys of `shape` (float-key cases carry their own keys).
    fillers: extra one-row groups of zeros.  What a route takes of the case's aggregates:
    only — just these functions (a route without MIN / MAX); nonnull — none over a nullable
    argument; limit — the first `limit` of what is left; pick — exactly these indices.
    Returns a namespace: keys / aggs (Columns, gpu_aggregate's operands), key_types, key_rows,
    plain_aggs (agg_ref.aggregate's operands), expected (its result), overflow, batches, rows,
    words (state_words of the aggregates kept).  Cached: callers must not change it."""
    case = CASES[case_id]()
    if "key_types" in case:
        key_types, key_of, filler_of = case["key_types"], None, None
        assert not fillers
    else:
        key_types, key_of, filler_of = KEY_SHAPES[shape]
    arg_types = case["args"]
    rows = []  # (group, index in group)
    sizes = [g["n"] for g in case["groups"]]
    for j in range(max(sizes)):
        rows += [(gi, j) for gi, n in enumerate(sizes) if j < n]
    key_rows = [case["groups"][gi]["keys"][j] if key_of is None else key_of(gi) for gi, j in rows]
    arg_vals = [[case["groups"][gi]["args"][a][j] for gi, j in rows] for a in range(len(arg_types))]
    # fillers spread through the rows; every argument 0 (+0.0), valid
    if fillers:
        step = max(1, len(rows) // fillers)
        for f in range(fillers):
            at = min(len(key_rows), f * (step + 1))
            key_rows.insert(at, filler_of(f))
            for v in arg_vals:
                v.insert(at, 0)
    aggs = [case["aggs"][i] for i in pick] if pick is not None else list(case["aggs"])
    aggs = [(n, a) for n, a in aggs if only is None or n in only]
    if nonnull:
        aggs = [(n, a) for n, a in aggs if a is None or not arg_types[a].nullable]
    aggs = aggs[:limit]
    key_cols = [to_column(t, [r[i] for r in key_rows]) for i, t in enumerate(key_types)]
    arg_cols = [to_column(t, v) for t, v in zip(arg_types, arg_vals)]
    plain_aggs = [(n, None if a is None else arg_types[a], None if a is None else arg_vals[a]) for n, a in aggs]
    ek, ec = R.aggregate(key_types, key_rows, plain_aggs)
    overflow = R.has_overflow(ec)
    assert overflow == bool(case.get("overflow")) or pick is not None
    return SimpleNamespace(keys=key_cols, aggs=[(n, None if a is None else arg_cols[a]) for n, a in aggs], key_types=key_types,
                           key_rows=key_rows, plain_aggs=plain_aggs, expected=(key_types, ek, ec), overflow=overflow,
                           batches=case.get("batches", 2), rows=len(key_rows), words=state_words(aggs, arg_types))


# ---- crafted serialized states --------------------------------------------------------------
def _le(v: int, nbytes: int) -> bytes:
    return (v & ((1 << (8 * nbytes)) - 1)).to_bytes(nbytes, "little")


def state_bytes(name, dt, value, count=None) -> bytes:
    """borsh of one aggregate's state over a non-nullable argument, as the factory builds it
    (or_null): NumberSumState {value} / DecimalSumState {value: i128} / Number|DecimalAvgState
    {value, count: u64} / MinMaxAnyState {Option<T>} (FUN/aggregate_sum.rs:64-170,
    aggregate_avg.rs:38-201, aggregate_min_max_any.rs:46-56), then AggregateFunctionOrNullAdaptor's
    flag byte (FUN/adaptors/aggregate_ornull_adaptor.rs:175-187)."""
    wide = dt.type_id == abi.DECIMAL128
    if name == "sum":
        body = _le(value, 16 if wide else 8)
    elif name == "avg":
        body = _le(value, 16 if wide else 8) + _le(count, 8)
    else:
        body = b"\x01" + _le(value, dt.width)
    return body + b"\x01"


def _merged(name, dt, states):
    """Expected result of merging states [(value, count)] of one group."""
    if name in ("min", "max"):
        return R._aggregate_group(name, dt, [v for v, _ in states])
    wide = dt.type_id == abi.DECIMAL128
    signed = dt.type_id not in R.UNSIGNED
    value = R.wrap(sum(v for v, _ in states), 128 if wide else 64, signed)
    count = sum(c or 0 for _, c in states) & (2**64 - 1)
    return R.finalize_state(name, dt, value, count)


def crafted_cases():
    """id -> (function, argument type, {Int32 key: [(value, count)] states of that group}).
    Counts no row count reaches (the divides' branch for a count above 2^32), quotients with a
    non-zero high word, the SUM range check at +-(10^38 - 1) and +-10^38, wrapping Int64 sums,
    and every float pool value as a MIN / MAX state.  Two states of one key are merged."""
    d38, d18_0, d18_4 = D(38, 4), D(18, 0), D(18, 4)
    counts = [2**32 - 1, 2**32, 2**32 + 1, 2**40 + 3]
    big = [10**37 + 12345678901234567, -(10**37) - 987654321, 3 * 10**30 + 1, -(2**100) - 1]
    out = {
        "avg_d38_counts": ("avg", d38, {k: [(v, c)] for k, (v, c) in enumerate(zip(big, counts))}),
        "avg_d38_merge": ("avg", d38, {1: [(big[0], 2**32 - 5), (big[2], 7)], 2: [(-5, 2**31), (-2, 2**31 + 1)]}),
        "avg_i64_counts": ("avg", col.Int64, {k: [(v, c)] for k, (v, c) in
                                              enumerate(zip([2**63 - 1, -2**63, -7, 2**62 + 1], counts))}),
        "avg_i64_merge": ("avg", col.Int64, {1: [(2**63 - 1, 2**32), (5, 1)], 2: [(-2**63, 2**33), (-1, 2**33)]}),
        "avg_u64_counts": ("avg", col.UInt64, {1: [(2**64 - 1, 2**32 + 1)], 2: [(2**63 + 5, 3)], 3: [(2**63, 2**40 + 3)]}),
        "avg_d18_min": ("avg", d18_4, {1: [(R.I128_MIN, 3)], 2: [(R.I128_MAX, 2**32 + 1)], 3: [(R.I128_MIN, 2**40 + 3)]}),
        "avg_d18_mul_ok": ("avg", d18_0, {1: [(R.I128_MAX // 10**4, 7)], 2: [(-(R.I128_MAX // 10**4), 2**32 + 1)]}),
        "avg_d18_mul_overflow": ("avg", d18_0, {1: [(R.I128_MAX // 10**4 + 1, 7)], 2: [(5, 1)]}),
        "sum_d18_valid": ("sum", d18_0, {1: [(R.DEC_MAX, None)], 2: [(-R.DEC_MAX, None)], 3: [(R.DEC_MAX - 5, None), (5, None)]}),
        "sum_d18_overflow_pos": ("sum", d18_0, {1: [(10**38, None)], 2: [(1, None)]}),
        "sum_d18_overflow_neg": ("sum", d18_0, {1: [(5, None)], 2: [(-(10**38) + 1, None), (-1, None)]}),
        "sum_i64_wrap": ("sum", col.Int64, {1: [(2**63 - 1, None), (1, None)], 2: [(-2**63, None), (-1, None)],
                                           3: [(2**63 - 1, None), (-2**63, None)]}),
        "sum_u64_wrap": ("sum", col.UInt64, {1: [(2**64 - 1, None), (7, None)], 2: [(2**63, None)]}),
    }
    for name, dt in (("min", col.Int8), ("max", col.Int16), ("min", col.Int32), ("max", col.Date), ("max", col.UInt8)):
        lo, hi = E.limits(dt)  # narrow MIN / MAX states of either sign: ser_decode widens them itself
        out[f"{name}_{dt}_states".lower()] = (name, dt, {1: [(lo, None), (hi, None)], 2: [(5, None), (E.as_type(dt, -3), None)],
                                                          3: [(E.as_type(dt, -1), None)], 4: [(hi, None), (lo, None)],
                                                          5: [(E.as_type(dt, -3), None), (5, None)]})
    for name in ("min", "max"):
        for dt, tag in ((col.Float64, "f64"), (col.Float32, "f32")):
            P = Pool(dt)
            single = {k: [(b, None)] for k, b in enumerate(P.all())}
            pairs = {100: [(P.nzero, None), (P.nzero, None)], 101: [(P.nzero, None), (P.zero, None)],
                     102: [(P.neg_nan, None), (P.snan, None)], 103: [(P.neg_nan, None), (P.neg(P.inf), None)],
                     104: [(P.neg(P.maxf), None), (P.neg(P.inf), None)], 105: [(P.inf, None), (P.maxf, None)],
                     106: [(P.sub_min, None), (P.neg(P.sub_min), None)]}
            out[f"{name}_{tag}_states"] = (name, dt, {**single, **pairs})
    return out


@functools.lru_cache(maxsize=None)
def crafted(case_id: str):
    """Namespace of a crafted case: blocks — [(key Column, state Column)] of well-formed
    AggregateMeta::Serialized blocks, every key at most once per block —, name, dtype, expected
    (assert_exact's operand), overflow."""
    name, dt, groups = crafted_cases()[case_id]
    depth = max(len(s) for s in groups.values())
    blocks = []
    for j in range(depth):
        ks = [k for k, s in groups.items() if j < len(s)]
        data = [state_bytes(name, dt, *groups[k][j]) for k in ks]
        blocks.append((Column.from_numbers(col.Int32, ks), Column.from_strings(data)))
    rt = E.result_dtype(name, SimpleNamespace(dtype=dt))
    vals = [_merged(name, dt, s) for s in groups.values()]
    expected = ([col.Int32], [(k,) for k in groups], [(rt, vals)])
    return SimpleNamespace(name=name, dtype=dt, blocks=blocks, expected=expected, overflow=R.has_overflow(expected[2]))


@functools.lru_cache(maxsize=None)
def float_key_states(dt, second):
    """Two AggregateMeta::Serialized blocks [COUNT(*) state, SUM(Int64) state, float key (, second
    key)] whose float keys hold NaNs of different sign and payload within a block and across the
    two, both zeros, both infinities and +-1.5.  second: None, "i32" or "str".  Namespace of
    key_types, aggs (_gpu_final's operand), blocks, expected (seven groups)."""
    from databend_amd.column import DataBlock
    P = Pool(dt)
    fk = [[P.nan, P.neg_nan, P.snan, P.zero, P.nzero, P.inf, P.neg(P.inf), P.v15],
          [P.snan, P.neg(P.snan), P.nzero, P.zero, P.neg(P.inf), P.neg(P.v15), P.neg_nan]]
    extra = {None: [], "i32": [(col.Int32, -1)], "str": [(col.String, b"k")]}[second]
    key_types = [dt] + [t for t, _ in extra]
    blocks, groups = [], {}
    for bi, ks in enumerate(fk):
        vals = [(7 * bi + i + 1, (-1) ** i * (2**62 + i)) for i in range(len(ks))]  # (count, sum): the sums wrap
        blocks.append(DataBlock([Column.from_strings([_le(c, 8) for c, _ in vals]),
                                 Column.from_strings([state_bytes("sum", col.Int64, s) for _, s in vals]),
                                 to_column(dt, ks)] + [to_column(t, [v] * len(ks)) for t, v in extra]))
        for k, (c, s) in zip(ks, vals):
            key = (k,) + tuple(v for _, v in extra)
            ck = tuple(R.canonical_key(t, v) for t, v in zip(key_types, key))
            first, c0, s0 = groups.get(ck, (key, 0, 0))
            groups[ck] = (first, c0 + c, R.wrap(s0 + s, 64, True))
    assert len(groups) == 7  # NaN, +0.0, -0.0, +inf, -inf, 1.5, -1.5
    g = list(groups.values())
    expected = (key_types, [x[0] for x in g], [(col.UInt64, [x[1] for x in g]), (col.Int64.wrap_nullable(), [x[2] for x in g])])
    aggs = [("count", None), ("sum", Column(col.Int64, np.zeros(0, np.int64)))]
    return SimpleNamespace(key_types=key_types, aggs=aggs, blocks=blocks, expected=expected)
