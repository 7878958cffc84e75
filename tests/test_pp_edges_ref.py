"""CPU check of tests/pp_edges.py: on every case the GPU edge tests use, exact_reference (Python
integers) equals the oracle bit for bit, and the key builders' partition properties hold when
recomputed from oracle.group_hash.  Pins the reference and the inputs without a GPU."""
import numpy as np
import pytest

from databend_amd import abi
from databend_amd import column as col
from databend_amd.column import Column
from oracle import oracle
from tests import pp_edges as E
from tests.parity import assert_results_equal

CASES = dict(E.all_cases())


def _sorted_bits(keys, aggs):
    """Rows ordered by key; every column as raw bits (floats as their u64 patterns)."""
    order = np.lexsort([k.data for k in keys][::-1])
    cols = []
    for c in list(keys) + list(aggs):
        d = np.asarray(c.data)[order]
        cols.append(d.view(np.uint64) if d.dtype == np.float64 else d)
        if c.validity is not None:
            assert np.all(np.asarray(c.validity, bool))
    return cols


@pytest.mark.parametrize("case_id", list(CASES))
def test_exact_reference_equals_oracle(case_id):
    case = CASES[case_id]()
    (ek, ea), (ok, oa) = E.references(case_id)
    assert [c.dtype for c in ea] == [c.dtype for c in oa]
    assert_results_equal(ek, ea, ok, oa)
    # bit for bit on integer, count, MIN and MAX results (AVG: the project's float rule, above)
    integer = [i for i, (name, _) in enumerate(case["aggs"]) if name in ("count", "sum", "min", "max")]
    e, o = _sorted_bits(ek, [ea[i] for i in integer]), _sorted_bits(ok, [oa[i] for i in integer])
    for x, y in zip(e, o):
        assert x.dtype == y.dtype and np.array_equal(x, y)


def test_exact_reference_wraps_and_extends():
    """The figures the oracle gives for the narrow-slot and wrapping cases, from Python integers."""
    k = Column.from_numbers(col.Int64, np.array([1] * 8192 + [2] * 8192 + [3] * 4))
    lo, hi = E.limits(col.Int16)
    i16 = Column.from_numbers(col.Int16, np.array([lo] * 8192 + [hi] * 8192 + [0] * 4))
    u64 = Column.from_numbers(col.UInt64, np.array([0] * 16384 + [2**63 + 5, 3, 2**64 - 1, 2**63 - 1], dtype=np.uint64))
    _, (s16, a16, s64, a64, mn, mx) = E.exact_reference([k], [("sum", i16), ("avg", i16), ("sum", u64), ("avg", u64),
                                                                ("min", u64), ("max", u64)])
    assert s16.values() == [-268435456, 268427264, 0]
    assert a16.values() == [-32768.0, 32767.0, 0.0]
    assert s64.values()[2] == 6 and a64.values()[2] == 1.5
    assert (mn.values()[2], mx.values()[2]) == (3, 2**64 - 1)
    assert s64.dtype == col.UInt64.wrap_nullable() and s16.dtype == col.Int64.wrap_nullable()


def test_keys_alone_in_partition():
    for dtypes in [E.C4_KEYS, (col.Int64,), (col.Int32,), (col.UInt16, col.UInt8)]:
        keys = E.keys_alone_in_partition(dtypes, 40)
        pre = E.prefixes(E.columns_of(dtypes, keys), E.MIN_BITS)
        assert len(keys) == 40 and len(set(pre.tolist())) == 40
    hot = E.narrow_cap_case()["hot"]
    assert hot[:3] == [(E.I64_MIN, E.I32_MIN), (-1, 0), (0, -1)]
    assert len(set(E.prefixes(E.columns_of(E.C4_KEYS, hot), E.MIN_BITS).tolist())) == 6


@pytest.mark.parametrize("shape", [s for s in E.CUT_SHAPES if s != "c4_desc"])
def test_key_sharing_partition(shape):
    dtypes = E.CUT_SHAPES[shape][0]
    case = E.cut_case(shape, "below_plus_2_keys")
    hot, near = case["hot"], case["near"]
    assert len(near) == 2 and len({hot, *near}) == 3
    h = oracle.group_hash(E.columns_of(dtypes, [hot] + near)) >> np.uint64(64 - E.MAX_BITS)
    assert h[0] == h[1] == h[2]
    assert E.key_sharing_partition(dtypes, hot) == near[0]


@pytest.mark.parametrize("case_id", list(CASES))
def test_case_partitions(case_id):
    """What each case relies on, at every partition width the plan can choose: its special keys'
    partitions hold exactly their own records, and no other partition comes near a cut."""
    case = CASES[case_id]()
    keys = case["keys"]
    n = len(keys[0])
    assert n <= 100_000
    dtypes = [k.dtype for k in keys]
    if "hot_partition_records" in case:
        special, expect = [case["hot"]], [case["hot_partition_records"]]
    elif "hot" in case:
        special, expect = case["hot"], [case["cut"]] * 6
    elif "group_keys" in case:
        special = case["group_keys"]
        rows = E.tuples_of(keys)
        expect = [rows.count(k) for k in special]
    else:
        special, expect = [], []
    for bits in range(E.MIN_BITS, E.MAX_BITS + 1):
        counts = np.bincount(E.prefixes(keys, bits), minlength=1 << bits)
        sp = E.prefixes(E.columns_of(dtypes, special), bits) if special else np.zeros(0, np.int64)
        assert counts[sp].tolist() == expect
        rest = counts.copy()
        rest[sp] = 0
        assert rest.max() < 256
    if "groups" in case:  # the 16 extreme key pairs: distinct from every filler key
        uk = set(E.tuples_of(keys))
        assert len(uk) == 16 + 3000 and set(case["groups"]) <= uk
