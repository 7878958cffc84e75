"""Predicate conformance on the GPU: every implementation of the filter against the independent
reference (tests/pred_ref.py), exactly, over the shared case matrix (tests/pred_cases.py).

  a. dbg_filter_select (eval_pred / cmp_const / cmp_cols), the whole matrix
  b. the two-pass compaction at its row-count and selectivity edges
  c. the generic insert (agg_insert_kernel), host and device input
  d. its `string <op> ''` queue (lenpred)
  e. the fast insert's predicate folded into a range on the host (launch_fast_t)
  f. the key-caching String insert with `key <op> ''`
  g. the short-key insert
  h. the partitioned payload: generic level-1 kernels, the specialised fixed-width predicate
     (pp_fast_pred) and the specialised String-key predicate
  i. take at the selection

The aggregate tests assert, through AggregateHashTable.insert_paths() or strategy(), that the
kernel they mean to test is the one that ran.
"""
import ctypes as C

import numpy as np
import pytest

from databend_amd import abi
from databend_amd import column as col
from databend_amd.aggregates import AggregateFunctionFactory
from databend_amd.aggregator import AggregateHashTable, AggregatorParams, HashTableConfig
from databend_amd.column import Column, pack_bits
from databend_amd.ffi import check, lib
from databend_amd.filter import FilterExecutor, FilterProgram, cmp
from tests import pred_cases as pc
from tests import pred_ref

pytestmark = pytest.mark.gpu

FN = AggregateFunctionFactory.instance()
TRUE = pred_ref.TRUE


def _torch():
    import torch
    return torch


# ---- device columns with bit offsets ---------------------------------------------------------
class DevCol:
    """A host Column in HBM as a dbg_column, its validity bitmap starting `voff` bits in and (for
    Boolean) its values `doff` bits in; the bits before them are set, so reading from bit 0 would
    show."""

    def __init__(self, c: Column, voff: int = 0, doff: int = 0):
        torch = _torch()
        self.host, self.length, self.dtype = c, len(c), c.dtype
        t = c.dtype.type_id
        if t == abi.BOOLEAN:
            data = pack_bits(np.concatenate([np.ones(doff, bool), np.asarray(c.data, bool)]))
        else:
            data = np.ascontiguousarray(c.data).view(np.uint8)
            doff = 0
        self.data = torch.from_numpy(np.concatenate([data, np.zeros(8, np.uint8)])).cuda()  # never empty
        self.offsets = torch.from_numpy(c.offsets.astype(np.uint64).view(np.int64).copy()).cuda() if c.offsets is not None else None
        self.validity = None
        if c.validity is not None and c.dtype.nullable:
            self.validity = torch.from_numpy(pack_bits(np.concatenate([np.ones(voff, bool), np.asarray(c.validity, bool)]))).cuda()
        else:
            voff = 0
        self.voff, self.doff = voff, doff

    def to_abi(self) -> abi.dbg_column:
        d = abi.dbg_column()
        d.dt = self.dtype.to_abi()
        d.data = self.data.data_ptr()
        if self.offsets is not None:
            d.offsets = self.offsets.data_ptr()
        if self.validity is not None:
            d.validity = self.validity.data_ptr()
        d.validity_offset, d.data_offset, d.len = self.voff, self.doff, self.length
        return d

    def __len__(self):
        return self.length


_DEV = {}


def dev(c: Column, shift: int = 0) -> DevCol:
    """The device copy of a host column (one per column and shift, made once per session)."""
    key = (id(c), shift)
    if key not in _DEV:
        _DEV[key] = (c, DevCol(c, voff=shift, doff=shift))
        _torch().cuda.synchronize()
    return _DEV[key][1]


_SEL = {}


def gpu_select(pred, dcols, n: int) -> np.ndarray:
    torch = _torch()
    if _SEL.get("n", -1) < n:
        _SEL["buf"], _SEL["n"] = torch.empty(max(1, n), dtype=torch.int32, device="cuda"), n
        torch.cuda.synchronize()
    prog = FilterProgram(pred, dcols)
    got = C.c_uint64()
    check(lib().dbg_filter_select(prog.ptr(), n, _SEL["buf"].data_ptr(), C.byref(got), None))
    assert got.value <= n
    return _SEL["buf"][:got.value].cpu().numpy().view(np.uint32)


def check_select_cases(cases, shift: int):
    for cid, cols, p in cases:
        got = gpu_select(p, [dev(c, shift) for c in cols], pc.N)
        assert np.array_equal(got, pred_ref.select(p, cols, pc.N)), cid


# ---- a. standalone select ---------------------------------------------------------------------
# shift: the bit offset of every validity bitmap and of Boolean values
@pytest.mark.parametrize("shift", [0, 5])
@pytest.mark.parametrize("name", pc.TYPES)
def test_select_constants_and_columns(name, shift):
    check_select_cases(pc.const_cases(name, False) + pc.const_cases(name, True) + pc.colcol_cases(name), shift)


@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("part", range(4))
def test_select_three_valued_logic(part, shift):
    check_select_cases(pc.logic_cases()[part::4], shift)


@pytest.mark.parametrize("shift", [0, 9])
def test_select_random_programs(shift):
    check_select_cases(pc.random_cases(), shift)


# ---- b. the compaction's edges ------------------------------------------------------------------
@pytest.mark.parametrize("rows", [0, 1, 15, 16, 17, 4095, 4096, 4097])
def test_select_row_count_edges(rows):
    patterns = {
        "none": (np.full(rows, 7), 7), "all": (np.full(rows, 7), 8), "every_other": (np.arange(rows) % 2, 1),
        "first_only": (np.where(np.arange(rows) == 0, 0, 5), 1), "last_only": (np.where(np.arange(rows) == rows - 1, 0, 5), 1),
    }
    for name, (vals, c) in patterns.items():
        column = Column.from_numbers(col.Int32, vals.astype(np.int32))
        p = cmp(0, "<", c)
        got = gpu_select(p, [DevCol(column)], rows)
        assert np.array_equal(got, pred_ref.select(p, [column], rows)), name


def test_select_more_than_1024_tiles():
    """1026 tiles: the single-workgroup scan of the tile counts runs two elements per thread."""
    rows = 1024 * 4096 + 4096 + 1
    rng = np.random.default_rng(1026)
    column = Column.from_numbers(col.Int32, rng.integers(-1000, 1000, rows).astype(np.int32))
    d = DevCol(column)
    for c in (-200, 999):
        p = cmp(0, "<", c)
        assert np.array_equal(gpu_select(p, [d], rows), pred_ref.select(p, [column], rows)), c


# ---- aggregates -------------------------------------------------------------------------------
class Table:
    """One handle, reset between cases."""

    def __init__(self, key_types, aggs, capacity_hint=0, strategy=abi.STRATEGY_AUTO):
        self.fns = [FN.get(n, [], [t] if t is not None else []) for n, t in aggs]
        self.strategy = strategy
        self.ht = AggregateHashTable(AggregatorParams(list(key_types), self.fns), HashTableConfig(True, capacity_hint))
        self.ht.set_strategy(strategy)
        self.n_aggs = len(aggs)

    def run(self, keys, args, pred, fcols, on_device=True) -> dict:
        """keys / args / fcols: DevCol (device) or Column (host).  -> key tuple -> aggregate values"""
        self.ht.reset()
        self.ht.set_strategy(self.strategy)
        fp = FilterProgram(pred, fcols)
        self.ht.add_groups(keys, args, rows=len(keys[0]), filter_program=fp, on_device=on_device)
        block = self.ht.merge_result()
        return pred_ref.result_dict(block.columns[self.n_aggs:], block.columns[:self.n_aggs])

    def paths(self) -> dict:
        return self.ht.insert_paths()

    def close(self):
        self.ht.close()


def expected_count_sum(pred, fcols, keys, v) -> dict:
    mask = pred_ref.evaluate(pred, fcols, len(keys[0])) == TRUE
    return pred_ref.group_reference(mask, keys, [v] if v is not None else [])


# ---- c. the generic insert ----------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [False, True])
def test_generic_insert(on_device):
    c = pc.agg_inputs()
    keys, v = [c["k_i32"], c["k_str"]], c["v"]
    t = Table([k.dtype for k in keys], [("count", None), ("sum", v.dtype)])
    place = dev if on_device else (lambda x: x)
    try:
        for cid, fcols, p in pc.generic_agg_cases():
            before = t.paths()["generic"]
            got = t.run([place(k) for k in keys], [None, place(v)], p, [place(f) for f in fcols], on_device=on_device)
            assert got == expected_count_sum(p, fcols, keys, v), cid
            assert t.paths()["generic"] > before, (cid, t.paths())
    finally:
        t.close()


# ---- d. `string <op> ''` from the offsets ----------------------------------------------------------
def test_generic_insert_lenpred():
    c = pc.agg_inputs()
    n = pc.N_AGG
    rng = np.random.default_rng(4)
    mixed = Column.from_strings([b"" if r < 0.4 else b"x" * int(1 + 40 * r) for r in rng.random(n)])
    all_empty = Column.from_strings([b""] * n)
    none_empty = Column.from_strings([b"y" * (1 + i % 3) for i in range(n)])
    key, v = c["k_i32"], c["v"]
    t = Table([key.dtype], [("count", None), ("sum", v.dtype)])
    try:
        for name, s in (("mixed", mixed), ("all_empty", all_empty), ("none_empty", none_empty)):
            for op in pc.OPS:
                p = cmp(0, op, b"")
                before = t.paths()["generic_lenpred"]
                got = t.run([dev(key)], [None, dev(v)], p, [dev(s)])
                assert got == expected_count_sum(p, [s], [key], v), (name, op)
                assert t.paths()["generic_lenpred"] > before, (name, op, t.paths())
    finally:
        t.close()


# ---- e. the fast insert's folded predicate --------------------------------------------------------
@pytest.mark.parametrize("name", pc.INT_TYPES)
def test_fast_insert_folded_predicate(name):
    """One non-null integer key filtered on itself (the same device column): `key <op> C` is
    folded on the host into a range test in the key's own type, with C - 1 / C + 1 at and past the
    type's limits."""
    key = pc.column(name, False, seed=9, n=pc.N_AGG)
    v = pc.agg_inputs()["v"]
    dk, dv = dev(key), dev(v)
    count_only = Table([key.dtype], [("count", None)])
    three = Table([key.dtype], [("count", None), ("sum", v.dtype), ("min", v.dtype)])
    try:
        for const in pc.int_constants(name):
            for op in pc.OPS:
                p = cmp(0, op, const)
                mask = pred_ref.evaluate(p, [key], pc.N_AGG) == TRUE
                exp = pred_ref.group_reference(mask, [key], [v])
                mins = pred_ref.group_min(mask, [key], v)
                before = count_only.paths()["fast_pred"], three.paths()["fast_pred"]
                got1 = count_only.run([dk], [None], p, [dk])
                got3 = three.run([dk], [None, dv, dv], p, [dk])
                assert got1 == {k: (cnt,) for k, (cnt, _) in exp.items()}, (op, const)
                assert got3 == {k: (cnt, s, mins[k]) for k, (cnt, s) in exp.items()}, (op, const)
                assert count_only.paths()["fast_pred"] > before[0] and three.paths()["fast_pred"] > before[1], (op, const)
    finally:
        count_only.close()
        three.close()


# ---- f. the key-caching String insert with `key <op> ''` -----------------------------------------
def test_str1_insert_with_predicate():
    rng = np.random.default_rng(48)
    n = pc.N_AGG
    words = sorted({bytes(rng.integers(32, 127, int(ln), dtype=np.uint8)) for ln in rng.integers(0, 49, 400)} | {b""})
    key = Column.from_strings([words[i] for i in rng.integers(0, len(words), n)])
    v = pc.agg_inputs()["v"]
    dk, dv = dev(key), dev(v)
    t = Table([key.dtype], [("count", None), ("sum", v.dtype)], capacity_hint=1 << 17)
    try:
        for op in pc.OPS:
            p = cmp(0, op, b"")
            before = t.paths()["str1_pred"]
            got = t.run([dk], [None, dv], p, [dk])
            assert got == expected_count_sum(p, [key], [key], v), op
            assert t.paths()["str1_pred"] > before, (op, t.paths())
    finally:
        t.close()


# ---- g. the short-key insert ------------------------------------------------------------------------
@pytest.mark.parametrize("n_keys", [1, 2])
def test_short_key_insert(n_keys):
    c = pc.agg_inputs()
    rng = np.random.default_rng(n_keys)
    words = [b"", b"k", b"key-one", b"0123456789abcdef", b"\xf0\x9f\x98\x80"]
    keys = [Column.from_strings([words[i] for i in rng.integers(0, len(words), pc.N_AGG)]) for _ in range(n_keys)]
    v = c["v"]
    t = Table([k.dtype for k in keys], [("count", None), ("sum", v.dtype)])
    try:
        for cid, fcols, p in pc.generic_agg_cases():
            before = t.paths()["short"]
            got = t.run([dev(k) for k in keys], [None, dev(v)], p, [dev(f) for f in fcols])
            assert got == expected_count_sum(p, fcols, keys, v), cid
            assert t.paths()["short"] > before, (cid, t.paths())
    finally:
        t.close()


# ---- h. the partitioned payload ------------------------------------------------------------------
def _partitioned(t: Table) -> bool:
    return t.ht.strategy()[0]


def _delta(before: dict, after: dict) -> dict:
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def test_partitioned_generic_predicates():
    """Nullable filter columns and multi-node programs: the generic level-1 kernels evaluate them."""
    c = pc.agg_inputs()
    keys, v = [c["k_i32"], c["k_str"]], c["v"]
    t = Table([k.dtype for k in keys], [("count", None), ("sum", v.dtype)], strategy=abi.STRATEGY_PARTITIONED)
    try:
        for cid, fcols, p in pc.generic_agg_cases():
            before = t.paths()
            got = t.run([dev(k) for k in keys], [None, dev(v)], p, [dev(f) for f in fcols])
            assert got == expected_count_sum(p, fcols, keys, v), cid
            assert _partitioned(t), cid
            assert _delta(before, t.paths()) == {"pp_generic": 1}, cid  # and no insert into the HBM table
    finally:
        t.close()


@pytest.mark.parametrize("name", pc.INT_TYPES)
def test_partitioned_specialised_fixed_predicate(name):
    """pp_fast_pred: a non-nullable fixed-width filter column against a constant, in the
    specialised level-1 scatter of fixed-width non-null keys and arguments.  That this level-1 form
    evaluated the predicate is what the "pp_fixed" count asserts.  pp_specialised() is about
    something else, the aggregation at finalize: it is asserted too, except where the predicate
    selects no row, since a payload without records is never aggregated."""
    n = pc.N_AGG
    f = pc.column(name, False, seed=9, n=n)
    key = Column.from_numbers(col.Int64, np.random.default_rng(7).integers(-150, 150, n) * (2**40 + 1))
    v = pc.agg_inputs()["v"]
    t = Table([key.dtype], [("count", None), ("sum", v.dtype)], strategy=abi.STRATEGY_PARTITIONED)
    try:
        for const in pc.int_constants(name):
            for op in pc.OPS:
                p = cmp(0, op, const)
                exp = expected_count_sum(p, [f], [key], v)
                before = t.paths()
                got = t.run([dev(key)], [None, dev(v)], p, [dev(f)])
                assert got == exp, (op, const)
                assert _partitioned(t) and _delta(before, t.paths()) == {"pp_fixed": 1}, (op, const, t.paths())
                assert t.ht.pp_specialised() or not exp, (op, const)  # no record, nothing to aggregate
    finally:
        t.close()


def test_partitioned_specialised_string_predicate():
    """One non-null String key filtered on itself (the same device column) with COUNT(*): the
    specialised String scatter compares each key with the constant bytewise."""
    n = pc.N_AGG
    rng = np.random.default_rng(13)
    pool = pc.STRING_POOL + [b"a\x80\x80", b"prefix__12", b"\xff", b"\x80abc"]
    key = Column.from_strings([pool[i] for i in rng.integers(0, len(pool), n)])
    dk = dev(key)
    longer = max(pool, key=len) + b"!"  # longer than every key
    t = Table([key.dtype], [("count", None)], strategy=abi.STRATEGY_PARTITIONED)
    try:
        for const in (b"", b"prefix__1", b"a\x80", longer, b"a", b"prefix__"):
            for op in pc.OPS:
                p = cmp(0, op, const)
                mask = pred_ref.evaluate(p, [key], n) == TRUE
                exp = {k: (cnt,) for k, (cnt, _) in pred_ref.group_reference(mask, [key], []).items()}
                before = t.paths()
                assert t.run([dk], [None], p, [dk]) == exp, (op, const)
                assert _partitioned(t) and _delta(before, t.paths()) == {"pp_str": 1}, (op, const, t.paths())
    finally:
        t.close()


# ---- i. take ------------------------------------------------------------------------------------------
def _take_inputs():
    n = pc.N
    rng = np.random.default_rng(17)
    strs = [bytes(rng.integers(97, 123, int(ln), dtype=np.uint8)) for ln in rng.integers(0, 18, n)]
    return dict(pos=Column.from_numbers(col.Int32, np.arange(n, dtype=np.int32)),
                s=Column.from_strings(strs), sn=Column.from_strings(strs[::-1], validity=rng.random(n) > 0.2),
                i16=pc.column("Int16", True, seed=11), dec=pc.column("Decimal128(38,6)", True, seed=11),
                b=pc.column("Boolean", False, seed=11), bn=pc.column("Boolean", True, seed=11))


def _host_take(c: Column, idx: np.ndarray):
    vals = c.values()
    return [vals[i] for i in idx]


def _check_take(cols: dict, idx_dev, idx: np.ndarray):
    from databend_amd.device import DeviceColumn
    names = [k for k in cols if k != "pos"]
    taken = FilterExecutor(None, []).take([DeviceColumn.from_host(cols[k]) for k in names], idx_dev)
    for k, out in zip(names, taken):
        assert out.to_host().values() == _host_take(cols[k], idx), k
    # a gathered Boolean column is a Boolean column like any other: gather it again, in reverse
    torch = _torch()
    back = np.arange(len(idx) - 1, -1, -1, dtype=np.int32)
    again = FilterExecutor(None, []).take([taken[names.index("b")], taken[names.index("bn")]], torch.from_numpy(back).cuda())
    for k, out in zip(("b", "bn"), again):
        assert out.to_host().values() == _host_take(cols[k], idx)[::-1], k


@pytest.mark.parametrize("n_sel", [0, 1, 1023, 1024, 1025, 2049])
def test_take_at_selection(n_sel):
    """The first n_sel rows pass the filter; every column is gathered at that selection."""
    from databend_amd.device import DeviceColumn
    cols = _take_inputs()
    p = cmp(0, "<", n_sel)
    sel = FilterExecutor(p, [0]).select([DeviceColumn.from_host(cols["pos"])], pc.N)
    idx = pred_ref.select(p, [cols["pos"]], pc.N)
    assert np.array_equal(sel.cpu().numpy().view(np.uint32), idx) and len(idx) == n_sel
    _check_take(cols, sel, idx)


def test_take_repeats_and_descending_runs():
    """An index vector as ORDER BY feeds it: repeats and descending runs, not a selection."""
    torch = _torch()
    cols = _take_inputs()
    rng = np.random.default_rng(23)
    idx = np.concatenate([np.arange(pc.N - 1, pc.N - 1500, -1), np.repeat(rng.integers(0, pc.N, 200), 3),
                          np.arange(40, 0, -1), [0, 0, pc.N - 1, pc.N - 1]]).astype(np.uint32)
    _check_take(cols, torch.from_numpy(idx.view(np.int32)).cuda(), idx)


@pytest.mark.parametrize("doff,voff", [(0, 0), (5, 3)])
def test_take_boolean_with_bit_offsets(doff, voff):
    """dbg_take_fixed itself, on a nullable Boolean column whose values and validity start inside
    a byte (a DeviceColumn cannot say that): one value byte per output row, validity bit-packed."""
    torch = _torch()
    c = pc.column("Boolean", True, seed=11)
    d = DevCol(c, voff=voff, doff=doff)
    idx = np.concatenate([np.arange(0, pc.N, 3), np.arange(pc.N - 1, pc.N - 50, -1)]).astype(np.uint32)
    sel = torch.from_numpy(idx.view(np.int32)).cuda()
    out = torch.zeros(len(idx), dtype=torch.uint8, device="cuda")
    vbits = torch.zeros((len(idx) + 7) // 8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    check(lib().dbg_take_fixed(C.byref(d.to_abi()), sel.data_ptr(), len(idx), out.data_ptr(), vbits.data_ptr(), None))
    valid = np.unpackbits(vbits.cpu().numpy(), bitorder="little")[:len(idx)].astype(bool)
    assert np.array_equal(valid, np.asarray(c.validity)[idx])
    assert np.array_equal(out.cpu().numpy().astype(bool)[valid], np.asarray(c.data)[idx][valid])
