"""Inputs and an exact reference for the partitioned specialised aggregation at its limits
(pp.hip pp_agg_spec_kernel / pp_agg_desc_kernel): groups of exactly the per-partition record
budget, argument and key extremes, and keys placed in chosen final partitions.

A record's final partition is the top `pp_bits` bits of its group hash (pp_mix is the identity).
The plan never uses fewer than MIN_BITS = PP_L1_BITS + 1 bits, so keys whose hashes differ in
their top MIN_BITS bits never share a final partition; with a specialised kernel it never uses
more than MAX_BITS = PP_L1_BITS + 10, so keys whose hashes agree in their top MAX_BITS bits always
do (abi_pp.hip pp_prepare).  The builders below place keys by those two facts; the tests recompute
every record's partition from the bits the finalize reports and check that the placement held.

exact_reference() is plain Python-integer arithmetic per group, independent of the oracle and
of the library; tests/test_pp_edges_ref.py pins it (and the builders) against the oracle on the
CPU, tests/test_gpu_pp_edges.py compares the kernels with both.
"""
import functools
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from databend_amd import abi
from databend_amd import column as col
from databend_amd.column import Column
from oracle import oracle

MIN_BITS = 9    # PP_L1_BITS + 1 (agg.hpp PP_L1_BITS = 8; abi_pp.hip pp_prepare: B and b2 start there)
MAX_BITS = 18   # PP_L1_BITS + 10 (abi_pp.hip pp_prepare: the specialised plan's b2 stops there)

# Records of one final partition the kernels aggregate themselves; one more and the partition goes
# to the generic kernel (`n > SNT * RPT`).  Written out on purpose: a retune of these constants
# must fail the cut tests and be updated here deliberately.
#   literal instances: PP_LIT_NT (1024) x PP_LIT_RPT (8)                         pp.hip:34-38
#   descriptor kernel: PP_SPEC_NT (1024) x ps_rpt(W), W = record words:          pp.hip:2137-2145
#                      8 at W <= 2, 4 at W <= 4, 2 beyond
CUT_LITERAL = 8192
CUT_DESC = {1: 8192, 2: 8192, 3: 4096, 4: 4096, 5: 2048, 6: 2048}


def limits(dt) -> Tuple[int, int]:
    i = np.iinfo(dt.np_dtype)
    return int(i.min), int(i.max)


def is_signed(dt) -> bool:
    return np.dtype(dt.np_dtype).kind == "i"


def bits_of(dt) -> int:
    return 8 * np.dtype(dt.np_dtype).itemsize


def as_type(dt, pattern: int) -> int:
    """The value of type dt whose two's-complement bits are `pattern` (mod 2^bits)."""
    b = bits_of(dt)
    v = pattern & ((1 << b) - 1)
    return v - (1 << b) if is_signed(dt) and v >> (b - 1) else v


def column_of(dt, values) -> Column:
    return Column.from_numbers(dt, np.array(list(values), dtype=dt.np_dtype))


def columns_of(dtypes, tuples) -> List[Column]:
    return [column_of(dt, [t[i] for t in tuples]) for i, dt in enumerate(dtypes)]


def random_columns(dtypes, n, rng) -> List[Column]:
    out = []
    for dt in dtypes:
        lo, hi = limits(dt)
        out.append(Column.from_numbers(dt, rng.integers(lo, hi, n, dtype=dt.np_dtype, endpoint=True)))
    return out


def tuples_of(cols: Sequence[Column]) -> List[tuple]:
    return list(zip(*[c.data.tolist() for c in cols]))


def prefixes(cols: Sequence[Column], bits: int) -> np.ndarray:
    """Final partition of every row under `bits` partition bits."""
    return (oracle.group_hash(cols) >> np.uint64(64 - bits)).astype(np.int64)


# ------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------
def result_dtype(name: str, arg: Optional[Column]):
    """AggregateFunction::return_type of the factory-built function (or_null wraps all but count)."""
    if name == "count":
        return col.UInt64
    if name not in ("sum", "avg", "sql_avg", "min", "max"):
        raise ValueError(name)
    t = arg.dtype
    if t.type_id == abi.DECIMAL128 and name not in ("min", "max"):
        # SUM: Decimal(38, s) (FUN/aggregate_sum.rs:203-222); AVG: Decimal(38, max(s, 4))
        # (FUN/aggregate_avg.rs:235-262); the SQL rewrite's divide: scale max(s, min(s + 6, 12))
        # (EXP/types/decimal.rs:1015-1018)
        s = t.scale
        scale = {"sum": s, "avg": max(s, 4), "sql_avg": max(s, min(s + 6, 12))}[name]
        return col.Decimal128(38, scale).wrap_nullable()
    if t.type_id in (abi.FLOAT32, abi.FLOAT64) and name not in ("min", "max"):
        return col.Float64.wrap_nullable()  # NumberSumState<f64> / NumberAvgState<_, f64>
    if name == "sum":
        return (col.Int64 if is_signed(arg.dtype) else col.UInt64).wrap_nullable()
    if name in ("avg", "sql_avg"):
        return col.Float64.wrap_nullable()
    if name in ("min", "max"):
        return arg.dtype.wrap_nullable()
    raise ValueError(name)


def exact_reference(keys: Sequence[Column], aggs: Sequence[Tuple[str, Optional[Column]]]):
    """GROUP BY keys with COUNT / SUM / MIN / MAX (and AVG) over non-nullable integer columns in
    Python integers.  SUM is reduced modulo 2^64 and reinterpreted as the result type (Int64 for
    signed arguments, UInt64 for unsigned); AVG is that wrapped sum divided by the count, in
    float64.  Returns (key columns, aggregate columns), groups in first-appearance order."""
    index: Dict[tuple, int] = {}
    gid = [index.setdefault(r, len(index)) for r in tuples_of(keys)]
    G = len(index)
    out_keys = columns_of([k.dtype for k in keys], list(index.keys()))
    counts = [0] * G
    for g in gid:
        counts[g] += 1
    out = []
    for name, c in aggs:
        rt = result_dtype(name, c)
        if name == "count":
            out.append(Column(rt, np.array(counts, dtype=np.uint64)))
            continue
        vals = c.data.tolist()
        if name in ("sum", "avg", "sql_avg"):
            acc = [0] * G
            for g, v in zip(gid, vals):
                acc[g] += v
            sum_t = col.Int64 if is_signed(c.dtype) else col.UInt64
            acc = [as_type(sum_t, s) for s in acc]
            if name == "sum":
                data = np.array(acc, dtype=sum_t.np_dtype)
            else:
                data = np.array([float(s) / float(n) for s, n in zip(acc, counts)], dtype=np.float64)
        else:
            pick = min if name == "min" else max
            acc = [None] * G
            for g, v in zip(gid, vals):
                acc[g] = v if acc[g] is None else pick(acc[g], v)
            data = np.array(acc, dtype=c.dtype.np_dtype)
        out.append(Column(rt, data, None, np.ones(G, dtype=bool)))
    return out_keys, out


# ------------------------------------------------------------------------------------------
# key placement
# ------------------------------------------------------------------------------------------
def keys_alone_in_partition(dtypes, g: int, include: Sequence[tuple] = (), seed: int = 1) -> List[tuple]:
    """g key tuples (starting with `include`) whose group hashes have pairwise distinct top
    MIN_BITS bits: they never share a final partition."""
    rng = np.random.default_rng(seed)
    cand = list(include) + tuples_of(random_columns(dtypes, 4000, rng))
    pre = prefixes(columns_of(dtypes, cand), MIN_BITS)
    out, seen = [], set()
    for i, t in enumerate(cand):
        if int(pre[i]) in seen:
            assert i >= len(include), f"keys to include share a partition: {t}"
            continue
        seen.add(int(pre[i]))
        out.append(t)
        if len(out) == g:
            return out
    raise AssertionError(f"only {len(out)} of {g} partition prefixes found")


def keys_sharing_partition(dtypes, key: tuple, n: int, seed: int = 2) -> List[tuple]:
    """n key tuples, different from `key` and from each other, whose group hashes share their
    top MAX_BITS bits with key's: they always land in key's final partition."""
    rng = np.random.default_rng(seed)
    want = int(prefixes(columns_of(dtypes, [key]), MAX_BITS)[0])
    cand = random_columns(dtypes, 1 << 22, rng)
    hit = np.nonzero(prefixes(cand, MAX_BITS) == want)[0]
    out = []
    for t in tuples_of([Column(c.dtype, c.data[hit]) for c in cand]):
        if t != tuple(key) and t not in out:
            out.append(t)
        if len(out) == n:
            return out
    raise AssertionError(f"only {len(out)} of {n} keys found in the partition of {key}")


def key_sharing_partition(dtypes, key: tuple) -> tuple:
    return keys_sharing_partition(dtypes, key, 1)[0]


def filler_keys(dtypes, n: int, avoid: Sequence[tuple], seed: int = 3) -> List[tuple]:
    """n distinct key tuples in none of the MIN_BITS-bit partitions of the keys in `avoid`."""
    rng = np.random.default_rng(seed)
    bad = np.unique(prefixes(columns_of(dtypes, list(avoid)), MIN_BITS)) if len(avoid) else np.zeros(0, np.int64)
    cand = random_columns(dtypes, 2 * n + 64, rng)
    ok = ~np.isin(prefixes(cand, MIN_BITS), bad)
    out = list(dict.fromkeys(tuples_of([Column(c.dtype, c.data[ok]) for c in cand])))
    assert len(out) >= n, f"{len(out)} filler keys of {n}"
    return out[:n]


# ------------------------------------------------------------------------------------------
# cases: {"keys": [Column], "aggs": [(name, Column | None)], + what the case's test needs}
# ------------------------------------------------------------------------------------------
def _assemble(dtypes, groups, fillers, arg_types, seed):
    """groups: [(key tuple, records, [value list per argument])]; fillers: key tuples with one
    record of uniform values each.  Rows shuffled.  Returns (key columns, argument columns)."""
    rng = np.random.default_rng(seed)
    ktup, args = [], [[] for _ in arg_types]
    for key, n, vals in groups:
        ktup += [key] * n
        for a, v in enumerate(vals):
            assert len(v) == n
            args[a] += list(v)
    ktup += list(fillers)
    for a, dt in enumerate(arg_types):
        lo, hi = limits(dt)
        args[a] += rng.integers(lo, hi, len(fillers), dtype=dt.np_dtype, endpoint=True).tolist()
    order = rng.permutation(len(ktup))
    keys = [Column(c.dtype, c.data[order]) for c in columns_of(dtypes, ktup)]
    acols = [Column.from_numbers(dt, np.array(v, dtype=dt.np_dtype)[order]) for dt, v in zip(arg_types, args)]
    return keys, acols


def _uniform(dt, n, rng) -> list:
    lo, hi = limits(dt)
    return rng.integers(lo, hi, n, dtype=dt.np_dtype, endpoint=True).tolist()


C4_KEYS = (col.Int64, col.Int32)
I64_MIN, I32_MIN = -2**63, -2**31


@functools.lru_cache(maxsize=None)
def narrow_cap_case():
    """(a) C4's shape; six hot keys, each alone in its partition with exactly 8192 records — the
    most a narrow (32-bit) slot is ever asked to hold — of Int16 extremes."""
    rng = np.random.default_rng(11)
    n = CUT_LITERAL
    lo, hi = limits(col.Int16)
    patterns = [[lo] * n, [hi] * n, [lo, hi] * (n // 2), [-1] * n, [0] * n, _uniform(col.Int16, n, rng)]
    hot = keys_alone_in_partition(C4_KEYS, 6, include=[(I64_MIN, I32_MIN), (-1, 0), (0, -1)])
    # SUM's argument takes pattern g, AVG's pattern 5 - g: both sum words see every pattern
    groups = [(hot[g], n, [patterns[g], patterns[5 - g]]) for g in range(6)]
    keys, (v, w) = _assemble(C4_KEYS, groups, filler_keys(C4_KEYS, 4000, hot), [col.Int16, col.Int16], 12)
    return {"keys": keys, "aggs": [("count", None), ("sum", v), ("sql_avg", w)], "hot": hot, "cut": n}


# (b) shape -> (key types, [(aggregate, argument type)], cut, descriptor kernel forced?)
CUT_SHAPES = {
    "i32_count_sum32": ((col.Int32,), [("count", None), ("sum", col.Int32)], CUT_DESC[1], False),
    "c4_literal": (C4_KEYS, [("count", None), ("sum", col.Int16), ("sql_avg", col.Int16)], CUT_LITERAL, False),
    "c4_desc": (C4_KEYS, [("count", None), ("sum", col.Int16), ("sql_avg", col.Int16)], CUT_DESC[2], True),
    "i64_sum_min": ((col.Int64,), [("sum", col.Int64), ("min", col.Int64)], CUT_DESC[3], False),
    "i64_i64_sum_min_max": ((col.Int64, col.Int64), [("sum", col.Int64), ("min", col.Int64), ("max", col.Int64)], CUT_DESC[5], False),
    "i64_count_sum_literal": ((col.Int64,), [("count", None), ("sum", col.Int64)], CUT_LITERAL, False),
    "i64_i64_count_literal": ((col.Int64, col.Int64), [("count", None)], CUT_LITERAL, False),
}
# variant -> (hot group size - cut, keys added to the hot partition with one record each, spills)
CUT_VARIANTS = {"below": (-1, 0, 0), "at": (0, 0, 0), "above": (1, 0, 1), "below_plus_key": (-1, 1, 0), "below_plus_2_keys": (-1, 2, 1)}


@functools.lru_cache(maxsize=None)
def cut_case(shape: str, variant: str):
    """(b) one hot group of cut - 1, cut or cut + 1 records of uniform values, alone in its final
    partition but for `extra` keys of one record each that share it; 2000 filler keys elsewhere."""
    dtypes, aggs, cut, _ = CUT_SHAPES[shape]
    d, extra, spills = CUT_VARIANTS[variant]
    rng = np.random.default_rng(21)
    arg_types = [t for _, t in aggs if t is not None]
    hot = keys_alone_in_partition(dtypes, 1, seed=22)[0]
    near = keys_sharing_partition(dtypes, hot, extra) if extra else []
    groups = [(hot, cut + d, [_uniform(t, cut + d, rng) for t in arg_types])]
    groups += [(k, 1, [_uniform(t, 1, rng) for t in arg_types]) for k in near]
    keys, acols = _assemble(dtypes, groups, filler_keys(dtypes, 2000, [hot]), arg_types, 23)
    it = iter(acols)
    return {"keys": keys, "aggs": [(name, next(it) if t is not None else None) for name, t in aggs], "hot": hot,
            "near": near, "cut": cut, "hot_partition_records": cut + d + extra, "spills": spills}


ARG_TYPES = {"Int8": col.Int8, "UInt8": col.UInt8, "Int16": col.Int16, "UInt16": col.UInt16, "Int32": col.Int32,
             "UInt32": col.UInt32, "Int64": col.Int64, "UInt64": col.UInt64}
ARG_AGGS = {"count_sum_min_max": ["count", "sum", "min", "max"], "avg_sum": ["avg", "sum"]}


@functools.lru_cache(maxsize=None)
def arg_case(tname: str, aggs: str):
    """(c) Int64 key, every aggregate over one column of type T; one group each of: only T.min,
    only T.max, both, the two values either side of the top bit, one record, uniform values, and
    the four bit patterns {2^(b-1) + 5, 3, 2^b - 1, 2^(b-1) - 1} (UInt64: SUM wraps to 6, AVG 1.5)."""
    T = ARG_TYPES[tname]
    rng = np.random.default_rng(31)
    lo, hi = limits(T)
    b = bits_of(T)
    # either side of the top bit: 2^(b-1) - 1 and 2^(b-1) unsigned, -1 and 0 signed
    below, above = (-1, 0) if is_signed(T) else ((1 << (b - 1)) - 1, 1 << (b - 1))
    values = [[lo] * 700, [hi] * 900, [lo, hi, hi] * 500, [below, above] * 1000, _uniform(T, 1, rng), _uniform(T, 300, rng),
              [as_type(T, p) for p in ((1 << (b - 1)) + 5, 3, (1 << b) - 1, (1 << (b - 1)) - 1)]]
    dtypes = (col.Int64,)
    gk = keys_alone_in_partition(dtypes, len(values), seed=32)
    keys, (v,) = _assemble(dtypes, [(k, len(x), [x]) for k, x in zip(gk, values)], filler_keys(dtypes, 3000, gk), [T], 33)
    return {"keys": keys, "aggs": [(name, None if name == "count" else v) for name in ARG_AGGS[aggs]], "group_keys": gk}


KEY_PAIRS = {"i8_i64": (col.Int8, col.Int64), "i32_i64": (col.Int32, col.Int64), "u16_u8": (col.UInt16, col.UInt8),
             "i16_i16": (col.Int16, col.Int16), "date_ts": (col.Date, col.Timestamp), "u64_u32": (col.UInt64, col.UInt32)}


def key_extremes(dt) -> List[int]:
    """{min, -1 or all-ones, 0, max} of a key type.  For an unsigned type these are two values (min
    is 0, all-ones is max); the two either side of its top bit make the set four again, so every
    pair of types yields 16 distinct groups."""
    lo, hi = limits(dt)
    if is_signed(dt):
        return [lo, -1, 0, hi]
    return [lo, hi, 1 << (bits_of(dt) - 1), (1 << (bits_of(dt) - 1)) - 1]


@functools.lru_cache(maxsize=None)
def key_case(pair: str):
    """(d) 16 groups: every combination of the extremes of the two key types, group i with
    5 + 7 i records; COUNT and SUM(Int32)."""
    dtypes = KEY_PAIRS[pair]
    rng = np.random.default_rng(41)
    combos = [(a, b) for a in key_extremes(dtypes[0]) for b in key_extremes(dtypes[1])]
    assert len(set(combos)) == 16
    sizes = [5 + 7 * i for i in range(16)]
    groups = [(k, n, [_uniform(col.Int32, n, rng)]) for k, n in zip(combos, sizes)]
    keys, (v,) = _assemble(dtypes, groups, filler_keys(dtypes, 3000, combos), [col.Int32], 43)
    return {"keys": keys, "aggs": [("count", None), ("sum", v)], "groups": dict(zip(combos, sizes))}


def all_cases():
    """(id, builder) of every case, for the CPU check of the reference and the builders."""
    out = [("narrow_cap", narrow_cap_case)]
    out += [(f"cut-{s}-{v}", functools.partial(cut_case, s, v)) for s in CUT_SHAPES for v in CUT_VARIANTS if s != "c4_desc"]
    out += [(f"arg-{t}-{a}", functools.partial(arg_case, t, a)) for t in ARG_TYPES for a in ARG_AGGS]
    out += [(f"key-{p}", functools.partial(key_case, p)) for p in KEY_PAIRS]
    return out


@functools.lru_cache(maxsize=None)
def references(case_id: str):
    """((keys, aggs) of exact_reference, (keys, aggs) of the oracle) of a case of all_cases(),
    or of "cut-c4_desc-*" (the input of "cut-c4_literal-*").  Computed once; callers must not
    change them."""
    from databend_amd.aggregates import AggregateFunctionFactory
    F = AggregateFunctionFactory.instance()
    case = dict(all_cases())[case_id.replace("c4_desc", "c4_literal")]()
    specs = [(F.get(n, [], [c.dtype] if c is not None else []).to_abi(), c) for n, c in case["aggs"]]
    return exact_reference(case["keys"], case["aggs"]), oracle.aggregate(case["keys"], specs, threads=4)
