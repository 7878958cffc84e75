"""MIN / MAX of a String argument on the GPU hash aggregate (MinMaxAnyState<StringType, CMP>).

The reference has no String MIN/MAX fixture and the oracle does not implement it, so the expected
values come from the plain Python reference below: per group the min / max of `bytes` objects,
which Python compares in &str order (unsigned bytewise lexicographic: a proper prefix sorts first,
0x80 sorts above 0x7f).  Comparison is exact.
"""
import ctypes as C

import numpy as np
import pytest

from databend_amd import abi
from databend_amd import column as col
from databend_amd.aggregates import AggregateFunctionFactory
from databend_amd.aggregator import AggregateHashTable, AggregatorParams, HashTableConfig
from databend_amd.column import Column
from databend_amd.ffi import Unsupported, check, lib
from databend_amd.filter import and_, cmp
from tests.test_gpu_parity import gpu_aggregate, slice_col

pytestmark = pytest.mark.gpu

F = AggregateFunctionFactory.instance()
ALPHABET = np.array([0x00, 0x2F, 0x61, 0x7A, 0x80, 0xFF], dtype=np.uint8)


def value_pool(rng, n_values, max_len=70, prefixes=(0, 19, 40)):
    """Strings over ALPHABET, lengths 0..max_len, sharing a prefix of one of `prefixes` bytes;
    always the empty string, and a string next to a proper prefix of it."""
    pre = {p: bytes(rng.choice(ALPHABET, p)) for p in prefixes}
    longest = pre[prefixes[-1]] + bytes(rng.choice(ALPHABET, max_len - prefixes[-1]))
    vals = [b"", longest, longest[:-3], longest[:prefixes[-1]]]
    while len(vals) < n_values:
        p = prefixes[int(rng.integers(len(prefixes)))]
        n = int(rng.integers(0, max_len + 1))
        vals.append(pre[p][:n] if n <= p else pre[p] + bytes(rng.choice(ALPHABET, n - p)))
    return vals


def strings(pool, idx, validity=None) -> Column:
    return Column.from_strings([pool[i] for i in idx], validity)


def reference(keys, aggs, selected=None):
    """{group key tuple: tuple of aggregate results}; aggs as gpu_aggregate takes them."""
    kv = [k.values() for k in keys]
    av = [None if c is None else c.values() for _, c in aggs]
    rows_of = {}
    for i in range(len(keys[0])):
        if selected is not None and not selected[i]:
            continue
        rows_of.setdefault(tuple(k[i] for k in kv), []).append(i)
    out = {}
    for g, rows in rows_of.items():
        res = []
        for (name, c), v in zip(aggs, av):
            if c is None:
                res.append(len(rows))
                continue
            vals = [v[i] for i in rows if v[i] is not None]
            if name == "count":
                res.append(len(vals))
            elif not vals:
                res.append(None)
            else:
                res.append({"min": min, "max": max, "sum": sum}[name](vals))
        out[g] = tuple(res)
    return out


def as_dict(gk, ga):
    kv = [c.values() for c in gk]
    av = [c.values() for c in ga]
    n = len(kv[0])
    out = {tuple(k[i] for k in kv): tuple(a[i] for a in av) for i in range(n)}
    assert len(out) == n, "a group appears twice"
    return out


def check_against_reference(keys, aggs, selected=None, **kw):
    gk, ga = gpu_aggregate(keys, aggs, **kw)
    for (name, c), r in zip(aggs, ga):
        if c is not None and c.dtype.type_id == abi.STRING:
            assert r.dtype.type_id == abi.STRING and r.dtype.nullable  # factory.get wraps or_null
    got = as_dict(gk, ga)
    exp = reference(keys, aggs, selected)
    assert got.keys() == exp.keys()
    bad = [(g, got[g], exp[g]) for g in exp if got[g] != exp[g]]
    assert not bad, bad[:3]
    return got


# ---- 1. order edge cases ------------------------------------------------------------------------
EDGE = [b"", b"a", b"a\x00", b"a\xff", b"ab", b"b", b"\x80"]


@pytest.mark.parametrize("with_empty", [True, False])
def test_order_edge_cases(with_empty):
    rng = np.random.default_rng(1)
    vals = EDGE if with_empty else EDGE[1:]
    idx = rng.permutation(np.repeat(np.arange(len(vals)), 3000))
    s = strings(vals, idx)
    key = Column.from_numbers(col.Int32, np.zeros(len(idx), np.int32))
    got = check_against_reference([key], [("min", s), ("max", s)])
    assert got[(0,)] == (b"" if with_empty else b"a", b"\x80")


# ---- 2. contention ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def contention():
    rng = np.random.default_rng(2)
    n = 200_000
    pool = value_pool(rng, 400)
    g = rng.integers(0, 7, n).astype(np.int32)
    s = strings(pool, rng.integers(0, len(pool), n))
    sn_valid = (rng.random(n) < 0.7) & (g != 3)  # group 3 holds only NULLs in sn
    sn = strings(pool, rng.integers(0, len(pool), n), sn_valid)
    x = Column.from_numbers(col.Int64, rng.integers(-1000, 1000, n))
    keys = [Column.from_numbers(col.Int32, g)]
    aggs = [("min", s), ("max", s), ("min", sn), ("max", sn), ("count", None), ("sum", x)]
    return keys, aggs


@pytest.mark.parametrize("on_device", [False, True])
def test_contention_few_groups(contention, on_device):
    keys, aggs = contention
    got = check_against_reference(keys, aggs, on_device=on_device)
    assert len(got) == 7 and got[(3,)][2] is None and got[(3,)][3] is None


# ---- 3. growth and rehash -----------------------------------------------------------------------
def test_growth_rehash_three_batches():
    rng = np.random.default_rng(3)
    n = 300_000
    pool = value_pool(rng, 5000)
    keys = [Column.from_numbers(col.Int64, rng.integers(0, 40_000, n) * 7919 - 12345)]
    s = strings(pool, rng.integers(0, len(pool), n))
    got = check_against_reference(keys, [("min", s), ("max", s), ("count", None)], batches=3)
    assert len(got) > 32768 / 1.5  # more groups than the default table holds at its load factor


# ---- 4. wide / ref keys -------------------------------------------------------------------------
def test_wide_ref_keys():
    rng = np.random.default_rng(4)
    n = 100_000
    pool = value_pool(rng, 2000)
    k0 = rng.integers(0, 1000, n) << 40
    k1 = rng.integers(0, 3, n).astype(np.int16)
    keys = [Column.from_numbers(col.Int64, k0), Column.from_numbers(col.Int16, k1, rng.random(n) < 0.8)]
    s = strings(pool, rng.integers(0, len(pool), n))
    sn = strings(pool, rng.integers(0, len(pool), n), rng.random(n) < 0.5)
    check_against_reference(keys, [("max", s), ("min", sn), ("count", None)], batches=2)


# ---- 5. one String key: the ClickBench shape ----------------------------------------------------
@pytest.mark.parametrize("distinct,hint", [(50_000, 100_000), (200, 0)])
def test_string_key_clickbench_shape(distinct, hint):
    rng = np.random.default_rng(5)
    n = 200_000
    phrases = [b"phrase %d " % i + b"x" * (i % 41) for i in range(distinct)]
    pool = value_pool(rng, 3000)
    keys = [strings(phrases, rng.integers(0, distinct, n))]
    url = strings(pool, rng.integers(0, len(pool), n))
    check_against_reference(keys, [("min", url), ("count", None)], capacity_hint=hint)


# ---- 6. fused filter ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["and", "length_only"])
def test_fused_filter(shape):
    rng = np.random.default_rng(6)
    n = 120_000
    pool = value_pool(rng, 300)
    g = rng.integers(0, 500, n)
    x = rng.integers(0, 100, n)
    x[g >= 450] = 0  # every row of these groups fails `x > 10`
    si = rng.integers(0, len(pool), n)
    si[(g >= 400) & (g < 450)] = 0  # ... and of these `s <> ''` (pool[0] is the empty string)
    s = strings(pool, si)
    xc = Column.from_numbers(col.Int64, x)
    keys = [Column.from_numbers(col.Int64, g)]
    nonempty = np.array([len(pool[i]) > 0 for i in si])
    if shape == "and":
        filt, sel = (and_(cmp(0, ">", 10), cmp(1, "<>", b"")), [xc, s]), (x > 10) & nonempty
    else:
        filt, sel = (cmp(0, "<>", b""), [s]), nonempty
    got = check_against_reference(keys, [("min", s), ("max", s), ("count", None)], selected=sel, filt=filt)
    assert all(g0 < 400 for (g0,) in got) if shape == "and" else all(not 400 <= g0 < 450 for (g0,) in got)


# ---- 7. long values -----------------------------------------------------------------------------
def test_long_values_shared_prefix():
    rng = np.random.default_rng(7)
    n = 30_000
    pool = value_pool(rng, 500, max_len=300, prefixes=(0, 19, 256))
    keys = [Column.from_numbers(col.Int32, rng.integers(0, 40, n).astype(np.int32))]
    s = strings(pool, rng.integers(0, len(pool), n))
    check_against_reference(keys, [("min", s), ("max", s)])


# ---- handles driven directly --------------------------------------------------------------------
def small_case(seed, n=60_000, groups=300):
    rng = np.random.default_rng(seed)
    pool = value_pool(rng, 800)
    keys = [Column.from_numbers(col.Int64, rng.integers(0, groups, n))]
    s = strings(pool, rng.integers(0, len(pool), n))
    sn = strings(pool, rng.integers(0, len(pool), n), rng.random(n) < 0.01)  # some groups all NULL
    return keys, [("min", s), ("max", sn), ("count", None)]


def make_table(keys, aggs, hint=0):
    fns = [F.get(n, [], [c.dtype] if c is not None else []) for n, c in aggs]
    return AggregateHashTable(AggregatorParams([k.dtype for k in keys], fns), HashTableConfig(True, hint))


def add_host(ht, keys, aggs, lo=0, hi=None):
    hi = len(keys[0]) if hi is None else hi
    ht.add_groups([slice_col(k, lo, hi) for k in keys], [None if c is None else slice_col(c, lo, hi) for _, c in aggs],
                  rows=hi - lo, on_device=False)


def result_dict(ht, n_aggs):
    cols = ht.merge_result().columns
    return as_dict(cols[n_aggs:], cols[:n_aggs])


# ---- 8. device result ---------------------------------------------------------------------------
def test_device_result_equals_host_result():
    keys, aggs = small_case(8)
    ht = make_table(keys, aggs)
    try:
        add_host(ht, keys, aggs)
        host = ht.merge_result().columns
        dev = [c.to_host() for c in ht.merge_result_device()]
        assert any(v is None for v in host[1].values())  # the NULL results are there to compare
        for h, d in zip(host, dev):
            assert h.dtype == d.dtype
            if h.offsets is not None:
                assert np.array_equal(h.offsets, d.offsets)
                nbytes = int(h.offsets[-1])
                assert np.array_equal(h.data[:nbytes], d.data[:nbytes])
            else:
                assert np.array_equal(h.data, d.data)
            assert (h.validity is None) == (d.validity is None)
            if h.validity is not None:
                assert np.array_equal(h.validity, d.validity)
        assert as_dict(host[3:], host[:3]) == reference(keys, aggs)
    finally:
        ht.close()


# ---- 9. reset and reuse -------------------------------------------------------------------------
def test_reset_and_reuse():
    keys_a, aggs_a = small_case(9)
    keys_b, aggs_b = small_case(10, n=20_000, groups=150)
    ht = make_table(keys_a, aggs_a)
    try:
        add_host(ht, keys_a, aggs_a)
        assert result_dict(ht, 3) == reference(keys_a, aggs_a)
        ht.reset()
        add_host(ht, keys_b, aggs_b)
        assert result_dict(ht, 3) == reference(keys_b, aggs_b)
    finally:
        ht.close()


# ---- 10. host staging and recycle mode ----------------------------------------------------------
def test_host_staging_blocks():
    keys, aggs = small_case(11, n=100_000)
    ht = make_table(keys, aggs)
    try:
        ht.set_host_staging(65536)
        for lo in range(0, 100_000, 10_000):
            add_host(ht, keys, aggs, lo, lo + 10_000)
        assert result_dict(ht, 3) == reference(keys, aggs)
    finally:
        ht.close()


def test_recycle_mode_device_batches(contention):
    from databend_amd.device import DeviceColumn
    keys, aggs = contention  # one Int32 key, 7 groups: the shape a recycling handle would fuse with its finalize
    ht = make_table(keys, aggs)
    try:
        check(lib().dbg_agg_set_recycle(ht.h, 1))
        n = len(keys[0])
        for lo, hi in ((0, n // 2), (n // 2, n)):
            ks = [DeviceColumn.from_host(slice_col(k, lo, hi)) for k in keys]
            ars = [None if c is None else DeviceColumn.from_host(slice_col(c, lo, hi)) for _, c in aggs]
            ht.add_groups(ks, ars, rows=hi - lo, on_device=True)
        assert result_dict(ht, len(aggs)) == reference(keys, aggs)
    finally:
        ht.close()


# ---- 11. refusals -------------------------------------------------------------------------------
def test_refusals_and_compact():
    keys, aggs = small_case(12, n=20_000, groups=100)
    ht = make_table(keys, aggs)
    L = lib()
    h = ht.h
    scratch = (C.c_uint64 * 4096)()  # a valid, zeroed buffer for every pointer argument
    p = C.cast(scratch, C.c_void_p)
    u64p = C.cast(scratch, C.POINTER(C.c_uint64))
    u32p = C.cast(scratch, C.POINTER(C.c_uint32))
    outc = (abi.dbg_out_column * 4)()
    incols = (abi.dbg_column * 4)()
    params, keep = ht.params.to_abi(True, 0, -1)
    layout = abi.dbg_record_layout()
    stats = abi.dbg_exchange_stats()
    ptrs = (C.c_void_p * 1)(p.value)
    calls = {
        "set_strategy(PARTITIONED)": lambda: L.dbg_agg_set_strategy(h, abi.STRATEGY_PARTITIONED),
        "partition": lambda: L.dbg_agg_partition(h, 4, 0, u64p, u64p),
        "export_records": lambda: L.dbg_agg_export_records(h, p, p),
        "merge_records": lambda: L.dbg_agg_merge_records(h, p, p, 1, u64p, u64p),
        "export_fixed": lambda: L.dbg_agg_export_fixed(h, p, 16),
        "merge_fixed": lambda: L.dbg_agg_merge_fixed(h, p, 1, 16),
        "payload_counts": lambda: L.dbg_agg_payload_counts(h, u64p, u32p),
        "payload_counts_from": lambda: L.dbg_agg_payload_counts_from(h, u32p, u64p, u32p, u32p),
        "payload_export": lambda: L.dbg_agg_payload_export(h, 1, p),
        "payload_export_from": lambda: L.dbg_agg_payload_export_from(h, 1, u32p, p),
        "payload_import": lambda: L.dbg_agg_payload_import(h, 1, 0, u64p, p, p),
        "payload_import_chunks": lambda: L.dbg_agg_payload_import_chunks(h, 1, 0, 1, u64p, ptrs, ptrs),
        "exchange_payload": lambda: L.dbg_agg_exchange_payload(p, h, C.byref(stats)),
        "exchange_payload_chunk": lambda: L.dbg_agg_exchange_payload_chunk(p, h, 1, C.byref(stats)),
        "exchange": lambda: L.dbg_agg_exchange(p, h, h, C.byref(stats)),
        "payload_exchange_plan": lambda: L.dbg_payload_exchange_plan(C.byref(params), 1, 0, u64p, u32p, u64p, u64p),
        "merge_exchange_plan": lambda: L.dbg_merge_exchange_plan(C.byref(params), 1, 0, u64p, u32p, u64p, u64p, u64p),
        "serialized_stride": lambda: L.dbg_agg_serialized_stride(h, u32p),
        "result_serialized": lambda: L.dbg_agg_result_serialized(h, outc, outc, 0),
        "merge_serialized": lambda: L.dbg_agg_merge_serialized(h, incols, incols, 1, 0),
        "record_layout": lambda: L.dbg_agg_record_layout(C.byref(params), C.byref(layout)),
        "finalize_into": lambda: L.dbg_agg_finalize_into(h, outc, outc, 16, None, u64p, u64p),
        "finalize_into_async": lambda: L.dbg_agg_finalize_into_async(h, outc, outc, 16, None),
    }
    try:
        add_host(ht, keys, aggs)
        for name, call in calls.items():
            assert call() == abi.DBG_ERR_UNSUPPORTED, name
            assert b"String min/max" in L.dbg_last_error(), (name, L.dbg_last_error())
        with pytest.raises(Unsupported):
            ht.set_strategy(abi.STRATEGY_PARTITIONED)
        with pytest.raises(Unsupported):
            ht.partition(4)
        with pytest.raises(Unsupported):
            ht.serialized_strides()
        with pytest.raises(Unsupported):
            ht.params.record_layout()
        assert ht.strategy()[0] is False
        assert ht.compact() is False
        assert result_dict(ht, 3) == reference(keys, aggs)
    finally:
        ht.close()
