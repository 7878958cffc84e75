"""The partitioned payload's specialised aggregation (pp.hip pp_agg_spec_kernel, pp_agg_desc_kernel)
at its limits: groups of exactly the per-partition record budget in narrow 32-bit slots, the
spill cut at max - 1 / max / max + 1, argument and key extremes in the descriptor kernel, and the
state-record output — inputs of at most ~60 k rows from tests/pp_edges.py.

Every result is compared with exact_reference (Python integers) and with the oracle; integer,
count, MIN and MAX results bit for bit, AVG by the project's float rule (tests/parity.py).  Every
test asserts that the specialised kernel ran, how many final partitions it handed to the generic
kernel (dbg_agg_get_pp_stats), and — from the partition bits the finalize reports — that the
records sat in the partitions the case was built for.

Two finalize routes reach the kernels: gpu_aggregate's dbg_agg_finalize + dbg_agg_result builds
state records (MODE 1) and converts them to columns; the fused dbg_agg_finalize_into writes the
result columns from the slots directly (MODE 0).  Tests (a)-(d) run both.
"""
import ctypes as C

import numpy as np
import pytest

from databend_amd import abi
from databend_amd import column as col
from databend_amd.aggregator import AggregateHashTable, AggregatorParams, HashTableConfig
from databend_amd.column import Column
from databend_amd.ffi import check, lib
from oracle import oracle
from tests import pp_edges as E
from tests.parity import assert_results_equal
from tests.test_gpu_parity import F, _cat, gpu_aggregate, slice_col

pytestmark = pytest.mark.gpu
PP = abi.STRATEGY_PARTITIONED
ROUTES = ["records", "fused"]


def _functions(aggs):
    return [F.get(n, [], [c.dtype] if c is not None else []) for n, c in aggs]


def fused_aggregate(keys, aggs, on_device=True, batches=1, info=None, strategy=PP, capacity_hint=0, recycle=False):
    """gpu_aggregate's twin on the fused finalize (dbg_agg_finalize_into, device output columns).
    recycle: dbg_agg_set_recycle, under which an on-device fast insert the table can fuse is held
    back and launched together with the finalize; info then also receives "paths_before" (the
    insert counts before the finalize), "finalize_scopes" (the profiler scopes the finalize call
    opened) and "groups_after" (what a second finalize finds in the recycled table)."""
    from databend_amd import ffi
    from databend_amd.device import DeviceColumn, empty
    from databend_amd.workloads import _dev_to_host
    fns = _functions(aggs)
    ht = AggregateHashTable(AggregatorParams([k.dtype for k in keys], fns), HashTableConfig(True, capacity_hint))
    ht.set_strategy(strategy)
    if recycle:
        check(lib().dbg_agg_set_recycle(ht.h, 1))
    try:
        n = len(keys[0])
        bounds = np.linspace(0, n, batches + 1).astype(int)
        keep = []
        for b in range(batches):
            lo, hi = int(bounds[b]), int(bounds[b + 1])
            ks = [slice_col(k, lo, hi) for k in keys]
            ars = [None if c is None else slice_col(c, lo, hi) for _, c in aggs]
            if on_device:
                ks = [DeviceColumn.from_host(k) for k in ks]
                ars = [None if c is None else DeviceColumn.from_host(c) for c in ars]
            keep.append((ks, ars))
            ht.add_groups(ks, ars, rows=hi - lo, on_device=on_device)
        out_a = [empty(f.return_type(), n) for f in fns]
        out_k = [empty(k.dtype, n) for k in keys]
        oa = (abi.dbg_out_column * len(out_a))()
        ok = (abi.dbg_out_column * len(out_k))()
        for arr, cols in ((oa, out_a), (ok, out_k)):
            for j, c in enumerate(cols):
                arr[j].data = c.data.data_ptr()
                arr[j].validity = c.validity.data_ptr() if c.validity is not None else None
        groups = C.c_uint64()
        sb = (C.c_uint64 * len(keys))()
        scap = (C.c_uint64 * len(keys))()
        watch = info is not None and recycle
        if watch:
            info["paths_before"] = ht.insert_paths()
            ffi.prof_reset()
            ffi.prof_enable(True)
        try:
            check(lib().dbg_agg_finalize_into(ht.h, oa, ok, n, scap, C.byref(groups), sb))
        finally:
            if watch:
                ffi.prof_enable(False)
                info["finalize_scopes"] = set(ffi.prof_read())
        if info is not None:
            info["partitioned"], info["extra_rounds"] = ht.strategy()
            info["specialised"] = ht.pp_specialised()
            info["pp_bits"], info["spilled"] = ht.pp_stats()
            info["insert_paths"] = ht.insert_paths()
        result = [_dev_to_host(c, groups.value) for c in out_k], [_dev_to_host(c, groups.value) for c in out_a]
        if watch:
            after = C.c_uint64()
            check(lib().dbg_agg_finalize_into(ht.h, oa, ok, n, scap, C.byref(after), sb))
            info["groups_after"] = after.value
        return result
    finally:
        ht.close()


def run_pp(case_id, case, route, on_device=True, batches=1):
    """One partitioned aggregate of a case on one finalize route, compared with both references.
    Returns (keys, aggs, info, records per final partition)."""
    info = {}
    if route == "fused":
        gk, ga = fused_aggregate(case["keys"], case["aggs"], on_device=on_device, batches=batches, info=info)
    else:
        gk, ga = gpu_aggregate(case["keys"], case["aggs"], strategy=PP, on_device=on_device, batches=batches, info=info)
    assert info["partitioned"] and info["specialised"]
    (ek, ea), (ok, oa) = E.references(case_id)
    assert_results_equal(gk, ga, ek, ea)
    assert_results_equal(gk, ga, ok, oa)
    bits = info["pp_bits"]
    assert E.MIN_BITS <= bits <= E.MAX_BITS
    return gk, ga, info, np.bincount(E.prefixes(case["keys"], bits), minlength=1 << bits)


def partitions_of(dtypes, key_tuples, bits):
    return E.prefixes(E.columns_of(dtypes, key_tuples), bits)


# ---- (a) narrow slots at the cap -----------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("batches", [1, 3])
@pytest.mark.parametrize("kernel", ["literal", "desc"])
def test_narrow_slots_at_the_cap(kernel, batches, on_device, route, monkeypatch):
    """Six groups of exactly 8192 records (PP_LIT_NT x PP_LIT_RPT, the bound of pp.hip's narrow
    slots: 32-bit count and Int16 sums) of Int16 extremes, each alone in its final partition, on
    C4's literal instance and on the descriptor kernel.  No partition may spill: only then did the
    32-bit words aggregate them."""
    if kernel == "desc":
        monkeypatch.setenv("DBG_X_PPSPEC_DESC", "1")
    case = E.narrow_cap_case()
    gk, ga, info, counts = run_pp("narrow_cap", case, route, on_device=on_device, batches=batches)
    assert info["spilled"] == 0
    hot_parts = partitions_of(E.C4_KEYS, case["hot"], info["pp_bits"])
    assert len(set(hot_parts.tolist())) == 6 and counts[hot_parts].tolist() == [case["cut"]] * 6
    rest = counts.copy()
    rest[hot_parts] = 0
    assert rest.max() <= case["cut"]
    rows = {r[:2]: r[2:] for r in zip(*[c.values() for c in list(gk) + list(ga)])}
    # all -32768 / all 32767 in SUM's argument; AVG's argument holds pattern 5 - g
    assert rows[case["hot"][0]][:2] == (8192, -268435456) and rows[case["hot"][1]][:2] == (8192, 268427264)
    assert rows[case["hot"][5]][2] == -32768.0 and rows[case["hot"][4]][2] == 32767.0


# ---- (b) the cut itself --------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("variant", list(E.CUT_VARIANTS))
@pytest.mark.parametrize("shape", list(E.CUT_SHAPES))
def test_spill_cut(shape, variant, route, monkeypatch):
    """A final partition of cut - 1, cut and cut + 1 records (one hot group; or cut - 1 of it plus
    one or two other keys of the same partition): the kernel keeps a partition of `cut` records
    (`n > SNT * RPT` spills) and hands one record more to the generic kernel.  Cuts: E.CUT_LITERAL,
    E.CUT_DESC (pp.hip ps_rpt, PP_LIT_NT x PP_LIT_RPT)."""
    dtypes, _, cut, desc = E.CUT_SHAPES[shape]
    if desc:
        monkeypatch.setenv("DBG_X_PPSPEC_DESC", "1")
    case = E.cut_case(shape, variant)
    gk, ga, info, counts = run_pp(f"cut-{shape}-{variant}", case, route, batches=2)
    bits = info["pp_bits"]
    hot_part = int(partitions_of(dtypes, [case["hot"]], bits)[0])
    assert counts[hot_part] == case["hot_partition_records"]
    assert np.all(partitions_of(dtypes, case["near"], bits) == hot_part) if case["near"] else True
    rest = counts.copy()
    rest[hot_part] = 0
    assert rest.max() <= cut
    assert info["spilled"] == case["spills"] == int(counts[hot_part] > cut)
    assert int(np.sum(E.prefixes(gk, bits) == hot_part)) == 1 + len(case["near"])


# ---- (c) argument extremes in the descriptor kernel ----------------------------------------
@pytest.mark.parametrize("route", ROUTES + ["table"])
@pytest.mark.parametrize("aggs", list(E.ARG_AGGS))
@pytest.mark.parametrize("tname", list(E.ARG_TYPES))
def test_argument_extremes(tname, aggs, route):
    """Groups of only T.min, only T.max, both, the values either side of the top bit, one record,
    uniform values and a wrapping 64-bit sum, for every integer argument type: the shift-pair
    extension (ps_arg), signed / unsigned MIN and MAX (ps_signed) and 64-bit wrap-around.  The same
    inputs through the HBM table pin that path at the same extremes."""
    case_id = f"arg-{tname}-{aggs}"
    case = E.arg_case(tname, aggs)
    if route == "table":
        gk, ga = gpu_aggregate(case["keys"], case["aggs"], strategy=abi.STRATEGY_TABLE, on_device=True, batches=2)
        (ek, ea), (ok, oa) = E.references(case_id)
        assert_results_equal(gk, ga, ek, ea)
        assert_results_equal(gk, ga, ok, oa)
        return
    gk, ga, info, counts = run_pp(case_id, case, route, batches=2)
    assert info["spilled"] == 0
    assert counts.max() <= min(E.CUT_DESC.values())  # no partition near any descriptor cut
    parts = partitions_of((col.Int64,), case["group_keys"], info["pp_bits"])
    assert len(set(parts.tolist())) == len(case["group_keys"])


# ---- (d) key masks and straddles -----------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("pair", list(E.KEY_PAIRS))
def test_key_masks_and_straddles(pair, route):
    """The 16 combinations of two key types' extremes (all ones beside zero, min beside max): a
    key mask, shift or straddle (km0, km1, k1s, klast) that leaked a bit would merge or split them.
    Exactly those groups come back, each with its own count."""
    case = E.key_case(pair)
    gk, ga, info, counts = run_pp(f"key-{pair}", case, route, batches=2)
    assert info["spilled"] == 0 and counts.max() <= min(E.CUT_DESC.values())
    got = dict(zip(zip(*[k.values() for k in gk]), ga[0].values()))
    assert len(got) == 16 + 3000
    assert {k: got[k] for k in case["groups"]} == case["groups"]


# ---- (e) state records ----------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["literal", "desc"])
def test_state_records_at_the_cap(kernel, monkeypatch):
    """The input of (a) as state records (MODE 1: narrow sums widened into 64-bit state words): a
    partitioned partial -> partition(4, 0) -> export_records -> merge_records into four partitioned
    finals.  Each final holds only keys with group_hash % 4 == p; the union equals the references."""
    import torch
    if kernel == "desc":
        monkeypatch.setenv("DBG_X_PPSPEC_DESC", "1")
    case = E.narrow_cap_case()
    keys, aggs = case["keys"], case["aggs"]
    params = AggregatorParams([k.dtype for k in keys], _functions(aggs))
    W = 4
    partial = AggregateHashTable(params, HashTableConfig(True))
    finals = [AggregateHashTable(params, HashTableConfig(False)) for _ in range(W)]
    try:
        for t in [partial] + finals:
            t.set_strategy(PP)
        partial.add_groups(keys, [c for _, c in aggs])
        counts, sbytes = partial.partition(W, 0)
        assert partial.pp_specialised()
        bits, spilled = partial.pp_stats()
        assert spilled == 0
        per_part = np.bincount(E.prefixes(keys, bits), minlength=1 << bits)
        hot_parts = partitions_of(E.C4_KEYS, case["hot"], bits)
        assert per_part[hot_parts].tolist() == [case["cut"]] * 6 and per_part.max() == case["cut"]
        w = partial.record_width()
        recs = torch.empty(max(1, sum(counts) * w), dtype=torch.uint8, device="cuda")
        strs = torch.empty(1, dtype=torch.uint8, device="cuda")
        partial.export_records(recs, strs)
        torch.cuda.synchronize()
        ro = 0
        for p in range(W):
            finals[p].merge_records(recs[ro * w:(ro + counts[p]) * w], strs[:1], [counts[p]], [0])
            ro += counts[p]
        nk, na = len(keys), len(aggs)
        all_k, all_a = [], []
        for p, f in enumerate(finals):
            blk = f.merge_result()
            ks, ags = blk.columns[na:], blk.columns[:na]
            assert len(ks[0]) == counts[p]
            assert np.all(oracle.group_hash(ks) % W == p)
            all_k.append(ks)
            all_a.append(ags)
        cat = lambda cols: Column(cols[0].dtype, *_cat(cols))
        gk = [cat([k[i] for k in all_k]) for i in range(nk)]
        ga = [cat([a[i] for a in all_a]) for i in range(na)]
        (ek, ea), (ok, oa) = E.references("narrow_cap")
        assert_results_equal(gk, ga, ek, ea)
        assert_results_equal(gk, ga, ok, oa)
    finally:
        for t in [partial] + finals:
            t.close()
