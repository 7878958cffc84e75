"""The predicate conformance matrix: data shared by tests/test_pred_ref.py (reference against the
oracle, on the CPU) and tests/test_gpu_predicates.py (every kernel against the reference).

A case is (id, [host Columns], Pred).  Columns are drawn from a small pool per type that holds
the values at which comparisons go wrong (type limits, sign and high bits, NaN and signed zeros,
prefixes and high bytes), and every constant sits in the pool together with its neighbours, so
`<` / `<=` / `>` / `>=` differ from each other on some row.
"""
import functools

import numpy as np

from databend_amd import column as col
from databend_amd.column import Column
from databend_amd.filter import and_, cmp, cmp_cols, is_not_null, is_null, not_, or_, true_

N = 8209  # two 4096-row tiles of the standalone filter and a 17-row tail: the last strip is partial
OPS = ["=", "<>", "<", "<=", ">", ">="]

_INT_RANGE = {"Int8": (-2**7, 2**7 - 1), "Int16": (-2**15, 2**15 - 1), "Int32": (-2**31, 2**31 - 1),
              "Int64": (-2**63, 2**63 - 1), "UInt8": (0, 2**8 - 1), "UInt16": (0, 2**16 - 1),
              "UInt32": (0, 2**32 - 1), "UInt64": (0, 2**64 - 1), "Date": (-2**31, 2**31 - 1),
              "Timestamp": (-2**63, 2**63 - 1)}
_DTYPES = {"Int8": col.Int8, "Int16": col.Int16, "Int32": col.Int32, "Int64": col.Int64, "UInt8": col.UInt8,
           "UInt16": col.UInt16, "UInt32": col.UInt32, "UInt64": col.UInt64, "Date": col.Date,
           "Timestamp": col.Timestamp, "Float32": col.Float32, "Float64": col.Float64, "Boolean": col.Boolean,
           "Decimal128(38,6)": col.Decimal128(38, 6), "Decimal128(15,2)": col.Decimal128(15, 2), "String": col.String}
TYPES = list(_DTYPES)
INT_TYPES = list(_INT_RANGE)
PRESENT, ABSENT = 42, 77  # 76 and 78 are in every integer pool, 77 in none


def int_constants(name: str, in_range_only: bool = False) -> list:
    """tmin, tmin+1, -1, 0, 1, a present value, an absent one, tmax-1, tmax; UInt64's sign-bit
    neighbourhood; and for types of up to 32 bits one constant past each end of the range
    (unsigned constants travel as their 64-bit pattern, so a negative one would alias a huge
    value: unsigned types get the upper one only)."""
    lo, hi = _INT_RANGE[name]
    cs = [lo, lo + 1, 0, 1, PRESENT, ABSENT, hi - 1, hi]
    if lo < 0:
        cs.append(-1)
    if name == "UInt64":
        cs += [2**63 - 1, 2**63]
    if not in_range_only and hi < 2**32:
        cs.append(hi + 1)
        if lo < 0:
            cs.append(lo - 1)
    return sorted(set(cs))


def _int_pool(name: str) -> list:
    lo, hi = _INT_RANGE[name]
    pool = set()
    for c in int_constants(name, in_range_only=True):
        pool |= {v for v in (c - 1, c, c + 1) if lo <= v <= hi}
    pool.discard(ABSENT)
    return sorted(pool)


def _float_info(name: str):
    return (np.float32, np.uint32, 0xFFC00001) if name == "Float32" else (np.float64, np.uint64, 0xFFF8000000000001)


def float_constants(name: str) -> list:
    """Python floats.  The node carries a double in the column's domain, so every Float32 constant
    here is exactly a float32 value (built as np.float32, then widened)."""
    ft, _, _ = _float_info(name)
    fi = np.finfo(ft)
    vals = [np.nan, np.inf, -np.inf, 0.0, -0.0, float(fi.smallest_subnormal), 1.5, 2.25, -2.5, float(fi.max), float(fi.min)]
    return [float(ft(v)) for v in vals]  # 2.25 is absent from the pool


def _float_pool(name: str) -> np.ndarray:
    ft, ut, neg_nan_bits = _float_info(name)
    base = [ft(c) for c in float_constants(name) if c != 2.25]
    pool = list(base)
    for c in (ft(1.5), ft(2.25), ft(-2.5), ft(0.0)):  # neighbours of the finite constants
        pool += [np.nextafter(c, ft(np.inf)), np.nextafter(c, ft(-np.inf))]
    pool += [np.nextafter(ft(np.finfo(ft).max), ft(0)), ft(1.0), ft(-1.0)]
    pool.append(np.array([neg_nan_bits], dtype=ut).view(ft)[0])  # a NaN with the sign bit and a payload
    return np.array(pool, dtype=ft)


_D38 = 10**38 - 1
_HI5 = 5 << 64  # pairs below share a high word and differ in a low word whose top bit is set
DECIMAL_POOLS = {
    "Decimal128(38,6)": sorted({_D38, _D38 - 1, -_D38, -_D38 + 1, -2, -1, 0, 1, 2, PRESENT - 1, PRESENT, PRESENT + 1,
                                ABSENT - 1, ABSENT + 1,
                                2**63 - 1, 2**63, 2**63 + 1, -2**63 - 1, -2**63, -2**63 + 1, 2**64 - 1, 2**64, -2**64, -2**64 + 1,
                                _HI5 + 2**63 - 1, _HI5 + 2**63, _HI5 + 2**63 + 1, _HI5 + 2**64 - 1,
                                -_HI5 + 2**63 - 1, -_HI5 + 2**63, -_HI5 + 2**63 + 1, -_HI5 - 1, -_HI5}),
    "Decimal128(15,2)": sorted({10**15 - 1, 10**15 - 2, -10**15 + 1, -10**15 + 2, -2, -1, 0, 1, 2, PRESENT - 1, PRESENT,
                                PRESENT + 1, ABSENT - 1, ABSENT + 1, 2**32 - 1, 2**32, 2**32 + 1, -2**32 - 1, -2**32, -2**32 + 1}),
}
DECIMAL_CONSTANTS = {
    "Decimal128(38,6)": [_D38, -_D38, -1, 0, 1, PRESENT, ABSENT, 2**63, -2**63, 2**64, _HI5 + 2**63, -_HI5 + 2**63, -_HI5],
    "Decimal128(15,2)": [10**15 - 1, -10**15 + 1, -1, 0, 1, PRESENT, ABSENT, 2**32, -2**32],
}

_P8 = b"prefix__"
STRING_POOL = [b"", b"a", b"a\x00", b"ab", b"a\x80", b"a\xff", _P8[:7], _P8, _P8 + b"x", _P8 + b"12345678",
               _P8 + b"123456789", _P8 + b"z" * 62]
# "" (the least string), the greatest pool string, a present value that is also a proper prefix
# ("a" of "ab"), an absent proper prefix, a present 8-byte value, a present value with a byte
# >= 0x80, and two absent values
STRING_CONSTANTS = [b"", max(STRING_POOL), b"a", b"pref", _P8, b"a\x80", b"a\x7f", b"b", _P8 + b"1234567"]


def constants(name: str) -> list:
    if name in _INT_RANGE:
        return int_constants(name)
    if name in ("Float32", "Float64"):
        return float_constants(name)
    if name == "Boolean":
        return [0, 1]
    if name == "String":
        return STRING_CONSTANTS
    return DECIMAL_CONSTANTS[name]


def _validity(rng, n: int) -> np.ndarray:
    v = rng.random(n) >= 0.1
    v[0] = v[-1] = False
    return v


@functools.lru_cache(maxsize=None)
def column(name: str, nullable: bool, seed: int = 0, n: int = N) -> Column:
    """n rows of `name` drawn from its pool (the same column object for the same arguments)."""
    rng = np.random.default_rng([seed, TYPES.index(name), int(nullable), n])
    v = _validity(rng, n) if nullable else None
    if name in _INT_RANGE:
        pool = _int_pool(name)
        vals = np.array(pool, dtype=_DTYPES[name].np_dtype)[rng.integers(0, len(pool), n)]
        return Column.from_numbers(_DTYPES[name], vals, validity=v)
    if name in ("Float32", "Float64"):
        pool = _float_pool(name)
        return Column.from_numbers(_DTYPES[name], pool[rng.integers(0, len(pool), n)], validity=v)
    if name == "Boolean":
        return Column.from_bools(rng.random(n) < 0.5, validity=v)
    if name == "String":
        return Column.from_strings([STRING_POOL[i] for i in rng.integers(0, len(STRING_POOL), n)], validity=v)
    pool = DECIMAL_POOLS[name]
    dt = _DTYPES[name]
    return Column.from_decimals(dt.precision, dt.scale, [pool[i] for i in rng.integers(0, len(pool), n)], validity=v)


def _cid(c) -> str:
    if isinstance(c, bytes):
        return c[:12].hex() or "empty"
    return repr(c)


def const_cases(name: str, nullable: bool) -> list:
    c = column(name, nullable)
    return [(f"{name}{'?' if nullable else ''} {op} {_cid(k)}", [c], cmp(0, op, k)) for k in constants(name) for op in OPS]


def colcol_cases(name: str) -> list:
    out = []
    for na in (False, True):
        for nb in (False, True):
            a, b = column(name, na, seed=1), column(name, nb, seed=2)
            out += [(f"{name}{'?' if na else ''} {op} {name}{'?' if nb else ''}", [a, b], cmp_cols(0, op, 1)) for op in OPS]
    return out


# ---- three-valued logic ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def logic_columns(n: int = N) -> tuple:
    """Three nullable Boolean columns: rows 0..26 run through {F, T, NULL}^3, the rest are random."""
    rng = np.random.default_rng(27)
    cols = []
    for k in range(3):
        state = np.concatenate([(np.arange(27) // 3**k) % 3, rng.integers(0, 3, n - 27)])
        cols.append(Column.from_bools(state == 1, validity=state != 2))
    return tuple(cols)


def _leaf(i: int):
    return cmp(i, "=", 1)


@functools.lru_cache(maxsize=None)
def logic_cases() -> list:
    cols = list(logic_columns())
    level = [(f"c{i}", _leaf(i)) for i in range(3)]
    seen = list(level)
    for _ in range(2):  # nestings of depth 2, then 3, over everything shallower
        nxt = [(f"not({s})", not_(p)) for s, p in seen]
        nxt += [(f"{nm}({s},{t})", f(p, q)) for nm, f in (("and", and_), ("or", or_)) for s, p in seen for t, q in seen]
        seen = level + nxt
    a, b, c = _leaf(0), _leaf(1), _leaf(2)
    extra = [("demorgan_and_lhs", not_(and_(a, b))), ("demorgan_and_rhs", or_(not_(a), not_(b))),
             ("demorgan_or_lhs", not_(or_(a, b))), ("demorgan_or_rhs", and_(not_(a), not_(b))),
             ("true", true_()), ("not(true)", not_(true_())), ("and(true,c0)", and_(true_(), a)), ("or(c0,not(true))", or_(a, not_(true_()))),
             ("is_null(c0)", is_null(0)), ("is_not_null(c1)", is_not_null(1)), ("not(is_null(c2))", not_(is_null(2))),
             ("or(is_null(c0),c1)", or_(is_null(0), b)), ("and(is_not_null(c0),not(c0))", and_(is_not_null(0), not_(a))),
             ("and(not(c0),is_null(c1),true)", and_(not_(a), is_null(1), true_())), ("or(and(c0,is_null(c1)),not(c2))", or_(and_(a, is_null(1)), not_(c)))]
    return [(f"logic {s}", cols, p) for s, p in seen + extra]


DEMORGAN = [("demorgan_and_lhs", "demorgan_and_rhs"), ("demorgan_or_lhs", "demorgan_or_rhs")]

# ---- random programs ---------------------------------------------------------------------
RANDOM_TYPES = [("Int32", False), ("Int32", True), ("String", False), ("String", True), ("Float64", True), ("UInt64", False),
                ("Decimal128(38,6)", True), ("Boolean", True)]
MAX_NODES, MAX_COLS = 24, 8


@functools.lru_cache(maxsize=None)
def random_columns() -> tuple:
    return tuple(column(t, nl, seed=3 + i) for i, (t, nl) in enumerate(RANDOM_TYPES))


def count_nodes(p) -> int:
    return len(p.postfix())


def columns_used(p) -> set:
    return {d[k] for d in p.postfix() for k in ("col", "col2") if k in d}


def _random_tree(rng, budget: int):
    """A tree of exactly `budget` postfix nodes."""
    if budget == 1:
        kind = rng.integers(0, 10)
        i = int(rng.integers(0, MAX_COLS))
        name = RANDOM_TYPES[i][0]
        if kind == 0:
            return is_null(i)
        if kind == 1:
            return is_not_null(i)
        if kind == 2:
            return true_()
        if kind == 3:
            same = [j for j, (t, _) in enumerate(RANDOM_TYPES) if t == name and j != i]
            if same:
                return cmp_cols(i, OPS[rng.integers(0, 6)], same[0])
        cs = constants(name)
        return cmp(i, OPS[rng.integers(0, 6)], cs[rng.integers(0, len(cs))])
    if budget == 2 or rng.random() < 0.15:
        return not_(_random_tree(rng, budget - 1))
    left = int(rng.integers(1, budget - 1))
    f = and_ if rng.random() < 0.5 else or_
    return f(_random_tree(rng, left), _random_tree(rng, budget - 1 - left))


@functools.lru_cache(maxsize=None)
def random_cases() -> list:
    rng = np.random.default_rng(20250)
    cols = list(random_columns())
    trees = []
    while not trees:  # the first tree is full-size and reads every column
        t = _random_tree(rng, MAX_NODES)
        if len(columns_used(t)) == MAX_COLS:
            trees.append(t)
    while len(trees) < 12:
        trees.append(_random_tree(rng, MAX_NODES))
    while len(trees) < 200:
        trees.append(_random_tree(rng, int(rng.integers(1, MAX_NODES + 1))))
    return [(f"random {i} ({count_nodes(t)} nodes)", cols, t) for i, t in enumerate(trees)]


@functools.lru_cache(maxsize=None)
def all_cases() -> list:
    out = []
    for name in TYPES:
        for nullable in (False, True):
            out += const_cases(name, nullable)
        out += colcol_cases(name)
    return out + logic_cases() + random_cases()


# ---- aggregate shapes (the insert kernels evaluate the predicate themselves) ----------------
N_AGG = 65549  # 17 workgroups of the generic insert with a ragged tail


@functools.lru_cache(maxsize=None)
def agg_inputs(n: int = N_AGG) -> dict:
    """Two keys (Int32 + nullable String), a SUM argument, and filter columns apart from the keys."""
    rng = np.random.default_rng(65549)
    words = [b"", b"k", b"key-one", b"key-two-longer-than-16-bytes", b"\xf0\x9f\x98\x80"]
    pos = np.arange(n)
    return dict(
        k_i32=Column.from_numbers(col.Int32, rng.integers(-3, 4, n)),
        k_str=Column.from_strings([words[i] for i in rng.integers(0, len(words), n)], validity=_validity(rng, n)),
        v=Column.from_numbers(col.Int64, rng.integers(-2**40, 2**40, n)),
        pos=Column.from_numbers(col.Int32, pos),  # the row number: selectivity by position
        eighth=Column.from_numbers(col.UInt8, rng.integers(0, 8, n)),
        i16n=column("Int16", True, seed=9, n=n), u64=column("UInt64", False, seed=9, n=n),
        f32n=column("Float32", True, seed=9, n=n), dec=column("Decimal128(38,6)", True, seed=9, n=n),
        s=column("String", False, seed=9, n=n), sn=column("String", True, seed=9, n=n),
        bn=column("Boolean", True, seed=9, n=n),
    )


def generic_agg_cases(n: int = N_AGG) -> list:
    """(id, [filter columns], pred) over agg_inputs(): the selectivities that leave the kernel's LDS
    selection queue empty, full, wrapped and partly full at the end, then a slice of the matrix."""
    c = agg_inputs(n)
    parity = Column.from_numbers(col.UInt8, np.arange(n) % 2)
    sel = [("none", [c["pos"]], cmp(0, "<", 0)), ("all", [c["pos"]], cmp(0, ">=", 0)),
           ("eighth", [c["eighth"]], cmp(0, "=", 3)), ("alternating", [parity], cmp(0, "=", 1)),
           ("last_row", [c["pos"]], cmp(0, "=", n - 1)), ("first_row", [c["pos"]], cmp(0, "<=", 0))]
    mat = [("i16n<-1", [c["i16n"]], cmp(0, "<", -1)), ("u64>=2^63", [c["u64"]], cmp(0, ">=", 2**63)),
           ("f32n>=nan", [c["f32n"]], cmp(0, ">=", float("nan"))), ("f32n<-0.0", [c["f32n"]], cmp(0, "<", -0.0)),
           ("dec<-hi5", [c["dec"]], cmp(0, "<=", -_HI5 + 2**63)), ("dec>2^63", [c["dec"]], cmp(0, ">", 2**63)),
           ("s>=a80", [c["s"]], cmp(0, ">=", b"a\x80")), ("sn<prefix", [c["sn"]], cmp(0, "<", _P8)),
           ("s<sn", [c["s"], c["sn"]], cmp_cols(0, "<", 1)), ("not(bn)", [c["bn"]], not_(cmp(0, "=", 1))),
           ("mixed", [c["i16n"], c["sn"], c["bn"], c["u64"]],
            or_(and_(cmp(0, ">", 0), not_(cmp(1, "=", b""))), and_(is_null(2), cmp(3, "<>", 2**64 - 1)))),
           ("null_or_true", [c["bn"], c["i16n"]], or_(cmp(0, "=", 1), is_null(1))), ("true", [c["pos"]], true_())]
    return sel + mat
