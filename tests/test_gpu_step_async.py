"""dbg_agg_step_async: one device batch into result columns in one call (dbg_agg_reset +
dbg_agg_add_groups(on_device = 1) + dbg_agg_finalize_into_async), completed by
dbg_agg_finalize_wait.

ClickBench Q8's shape (Int16 key, `key <> 0`, COUNT(*)) at the row counts where the fused launch
changes path — one workgroup round is 8 vectors x 1024 lanes x 2 = 16384 rows: below one 16-byte
vector and ragged (1, 7, 8, 9: one workgroup, no chain), the smallest chain (16384 is still one
workgroup, 16385 two), two groups of the chain with the second of size 1 (17 workgroups,
SCR_GROUP = 16), and the full grid over two rounds with a ragged end.  Every result equals the
oracle, and equals what the three calls give on a second handle bit for bit: the same groups with
the same key and count bits.  The order of result rows is free in this library (the count-only
finalize takes each row's position from an atomic counter), so both sides are put in key order
first.

Also: a shape that cannot fuse (Int64 key with SUM), output buffers shorter than the groups
(DBG_ERR_INVALID with the group count, table intact, the retry succeeds), a call while a finalize is
in flight (refused, nothing changes), and 40 consecutive steps on a fresh handle, which cross both
wraps of the chain's tags (a handle starts 32 finalizes below 2^24)."""
import ctypes as C

import numpy as np
import pytest

from databend_amd import abi
from databend_amd import column as col
from databend_amd.aggregates import AggregateFunctionFactory
from databend_amd.aggregator import AggregateHashTable, AggregatorParams, HashTableConfig
from databend_amd.column import Column, abi_array
from databend_amd.device import DeviceColumn, empty
from databend_amd.ffi import check, lib
from databend_amd.filter import FilterProgram, cmp
from tests.parity import assert_results_equal
from tests.test_gpu_parity import oracle_aggregate

pytestmark = pytest.mark.gpu
F = AggregateFunctionFactory.instance()

ROUND = 8 * 1024 * 2  # rows of one workgroup round
ROWS = [1, 7, 8, 9, ROUND, ROUND + 1, 17 * ROUND + 5, 256 * 2 * ROUND + 3]


class Handle:
    """One recycling handle with its output columns; `step` goes through the new entry, `three`
    through the three calls it stands for."""

    def __init__(self, ktype, fns):
        self.ktype, self.fns = ktype, fns
        self.params = AggregatorParams([ktype], fns)
        self.rtypes = [f.return_type() for f in fns]
        self.table = AggregateHashTable(self.params, HashTableConfig(True))
        self.h = self.table.h
        check(lib().dbg_agg_set_recycle(self.h, 1))
        self._keep = []  # argument structs of every call, alive as long as the handle
        self.alloc(1024)

    def alloc(self, cap):
        self.cap = cap
        self.kcol = empty(self.ktype, cap)
        self.acols = [empty(t, cap) for t in self.rtypes]
        self.ok = (abi.dbg_out_column * 1)()
        self.oa = (abi.dbg_out_column * len(self.acols))()
        self.ok[0].data = self.kcol.data.data_ptr()
        for j, c in enumerate(self.acols):
            self.oa[j].data = c.data.data_ptr()
            self.oa[j].validity = c.validity.data_ptr() if c.validity is not None else None
        self.scap = (C.c_uint64 * 1)(0)

    @staticmethod
    def marshal(dkey, dargs, pred):
        keys = abi_array([dkey.to_abi()])
        args = []
        for c in dargs:
            if c is None:
                d = abi.dbg_column()
                d.dt = abi.dbg_datatype(-1, 0, 0, 0, 0)
                args.append(d)
            else:
                args.append(c.to_abi())
        fp = FilterProgram(cmp(0, pred[0], pred[1]), [dkey]) if pred else None
        return keys, abi_array(args), fp

    def step_rc(self, dkey, dargs, pred, n):
        keys, args, fp = self.marshal(dkey, dargs, pred)
        self._keep.append((keys, args, fp))
        return lib().dbg_agg_step_async(self.h, keys, args, fp.ptr() if fp else None, n, self.oa, self.ok, self.cap, self.scap)

    def three_rc(self, dkey, dargs, pred, n):
        keys, args, fp = self.marshal(dkey, dargs, pred)
        self._keep.append((keys, args, fp))
        L = lib()
        check(L.dbg_agg_reset(self.h))
        check(L.dbg_agg_add_groups(self.h, keys, args, fp.ptr() if fp else None, n, 1))
        return L.dbg_agg_finalize_into_async(self.h, self.oa, self.ok, self.cap, self.scap)

    def wait_rc(self):
        ng = C.c_uint64()
        sb = (C.c_uint64 * 1)()
        rc = lib().dbg_agg_finalize_wait(self.h, C.byref(ng), sb)
        return rc, ng.value

    def wait(self):
        rc, m = self.wait_rc()
        check(rc)
        return self.host(m)

    def host(self, m):
        import torch
        torch.cuda.synchronize()
        kw = self.ktype.width
        kh = Column(self.ktype, self.kcol.data[: m * kw].cpu().numpy().view(self.ktype.np_dtype).copy())
        ah = [Column(t, c.data[: m * t.width].cpu().numpy().view(t.np_dtype).copy()) for t, c in zip(self.rtypes, self.acols)]
        return [kh], ah

    def close(self):
        self.table.close()


def same_bits(a, b):
    """Two results hold the same rows with the same bits (rows taken in key order: see above)."""
    (ka,), aa = a
    (kb,), ab = b
    assert len(ka.data) == len(kb.data)
    ia, ib = np.argsort(ka.data, kind="stable"), np.argsort(kb.data, kind="stable")
    assert ka.data[ia].tobytes() == kb.data[ib].tobytes()
    for x, y in zip(aa, ab):
        assert x.data[ia].tobytes() == y.data[ib].tobytes()


@pytest.fixture(scope="module")
def q8_keys():
    """Int16 values, 70 % zero, the rest 33 values that include both ends of the type; row 0 is
    selected, so even the 1-row prefix has a group."""
    rng = np.random.default_rng(8)
    n = max(ROWS)
    pool = np.concatenate([rng.integers(-32768, 32768, 31), [-32768, 32767]]).astype(np.int16)
    pool[pool == 0] = 5
    vals = np.where(rng.random(n) < 0.7, 0, pool[rng.integers(0, len(pool), n)]).astype(np.int16)
    vals[0] = 32767
    return vals


@pytest.fixture(scope="module")
def q8_handles():
    a = Handle(col.Int16, [F.get("count")])
    b = Handle(col.Int16, [F.get("count")])
    yield a, b
    a.close()
    b.close()


@pytest.mark.parametrize("n", ROWS)
def test_step_async_matches_oracle_and_three_calls(q8_keys, q8_handles, n):
    a, b = q8_handles
    key = Column.from_numbers(col.Int16, q8_keys[:n])
    dk = DeviceColumn.from_host(key)
    check(a.step_rc(dk, [None], ("<>", 0), n))
    got = a.wait()
    check(b.three_rc(dk, [None], ("<>", 0), n))
    ref = b.wait()
    ok, oa = oracle_aggregate([key], [("count", None)], (cmp(0, "<>", 0), [key]))
    assert_results_equal(got[0], got[1], ok, oa)
    same_bits(got, ref)


def test_step_async_unfusable_shape_gives_three_call_result():
    """Int64 key with SUM: the insert is not held back for a fused launch; the entry enqueues the
    insert and the table finalize as the three calls do."""
    rng = np.random.default_rng(9)
    n = 300_001
    key = Column.from_numbers(col.Int64, rng.integers(-50, 50, n) * (1 << 40))
    val = Column.from_numbers(col.Int64, rng.integers(-(1 << 40), 1 << 40, n))
    fns = [F.get("sum", [], [col.Int64])]
    a, b = Handle(col.Int64, fns), Handle(col.Int64, fns)
    try:
        dk, dv = DeviceColumn.from_host(key), DeviceColumn.from_host(val)
        for _ in range(2):  # the second step resets a table that holds groups
            check(a.step_rc(dk, [dv], None, n))
            got = a.wait()
            check(b.three_rc(dk, [dv], None, n))
            ref = b.wait()
            ok, oa = oracle_aggregate([key], [("sum", val)])
            assert_results_equal(got[0], got[1], ok, oa)
            same_bits(got, ref)
    finally:
        a.close()
        b.close()


def test_step_async_short_buffers_then_retry(q8_keys):
    n = 17 * ROUND + 5
    key = Column.from_numbers(col.Int16, q8_keys[:n])
    dk = DeviceColumn.from_host(key)
    ok, oa = oracle_aggregate([key], [("count", None)], (cmp(0, "<>", 0), [key]))
    groups = len(ok[0].data)
    assert groups > 8
    a = Handle(col.Int16, [F.get("count")])
    try:
        a.alloc(8)
        check(a.step_rc(dk, [None], ("<>", 0), n))
        rc, m = a.wait_rc()
        assert rc == abi.DBG_ERR_INVALID and m == groups
        # the table is intact: finalize it again into buffers that hold every group
        a.alloc(groups)
        ng = C.c_uint64()
        sb = (C.c_uint64 * 1)()
        check(lib().dbg_agg_finalize_into(a.h, a.oa, a.ok, a.cap, a.scap, C.byref(ng), sb))
        assert ng.value == groups
        got = a.host(groups)
        assert_results_equal(got[0], got[1], ok, oa)
        # and the handle steps on
        check(a.step_rc(dk, [None], ("<>", 0), n))
        got = a.wait()
        assert_results_equal(got[0], got[1], ok, oa)
    finally:
        a.close()


def test_step_async_refused_while_a_finalize_is_in_flight(q8_keys):
    n1, n2 = 17 * ROUND + 5, ROUND + 1
    k1, k2 = (Column.from_numbers(col.Int16, q8_keys[:m]) for m in (n1, n2))
    # another batch: were it accepted, the result would change
    k2 = Column.from_numbers(col.Int16, (k2.data.astype(np.int32) // 2 + 1).astype(np.int16))
    d1, d2 = DeviceColumn.from_host(k1), DeviceColumn.from_host(k2)
    a = Handle(col.Int16, [F.get("count")])
    try:
        check(a.step_rc(d1, [None], ("<>", 0), n1))
        assert a.step_rc(d2, [None], ("<>", 0), n2) == abi.DBG_ERR_INVALID
        assert b"in flight" in lib().dbg_last_error()
        got = a.wait()  # the finalize in flight is still there and delivers batch 1
        ok, oa = oracle_aggregate([k1], [("count", None)], (cmp(0, "<>", 0), [k1]))
        assert_results_equal(got[0], got[1], ok, oa)
        rc, _ = a.wait_rc()  # and only that one
        assert rc == abi.DBG_ERR_INVALID
        check(a.step_rc(d2, [None], ("<>", 0), n2))
        got = a.wait()
        ok, oa = oracle_aggregate([k2], [("count", None)], (cmp(0, "<>", 0), [k2]))
        assert_results_equal(got[0], got[1], ok, oa)
    finally:
        a.close()


def test_step_async_40_steps_cross_both_tag_wraps(q8_keys):
    """A fresh handle's sequence number starts 32 below 2^24: 40 steps of a chained launch pass the
    wrap of the 20-bit and of the 24-bit tag (the scratch is cleared there).  Two inputs alternate,
    so a result served from stale parked words would not match."""
    n = 17 * ROUND + 5
    ka = Column.from_numbers(col.Int16, q8_keys[:n])
    kb = Column.from_numbers(col.Int16, q8_keys[n:2 * n])
    cols = [ka, kb]
    dev = [DeviceColumn.from_host(c) for c in cols]
    exp = [oracle_aggregate([c], [("count", None)], (cmp(0, "<>", 0), [c])) for c in cols]
    a = Handle(col.Int16, [F.get("count")])
    try:
        for s in range(40):
            check(a.step_rc(dev[s % 2], [None], ("<>", 0), n))
            got = a.wait()
            assert_results_equal(got[0], got[1], exp[s % 2][0], exp[s % 2][1])
    finally:
        a.close()
