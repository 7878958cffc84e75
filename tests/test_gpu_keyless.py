"""Aggregation without GROUP BY on the GPU: the keyless handle (include/dbgpu_agg.h), its reduce and
merge kernels (csrc/reduce.hip) and the single-state processor mirrors.

Expected values come from tests/agg_ref.py — the exact Python-integer / Fraction reference — over
one group of every selected row, with the rule for the empty input added here: COUNT = 0, everything
else NULL.  Comparison is bit for bit (agg_ref.assert_exact; NaN and the zeros' sign follow its two
rules).  Every run asserts through keyless_stats() that the reduce (or the state merge) ran.
"""
import ctypes as C
import math

import numpy as np
import pytest

from databend_amd import abi
from databend_amd import column as col
from databend_amd.aggregator import (AggregateHashTable, AggregatorParams, FinalSingleStateAggregator, HashTableConfig,
                                     PartialSingleStateAggregator)
from databend_amd.column import Column, DataBlock
from databend_amd.device import DeviceColumn
from databend_amd.ffi import DbgError, DecimalOverflow, Unsupported, lib
from databend_amd.filter import FilterProgram, and_, cmp, like, not_like
from tests import agg_cases as AC
from tests import agg_ref as R
from tests import like_ref, pred_cases, pred_ref
from tests.pp_edges import result_dtype
from tests.test_gpu_parity import F, gpu_aggregate, slice_col

pytestmark = pytest.mark.gpu
TILE, G = abi.KEYLESS_TILE, abi.KEYLESS_MAX_BLOCKS
D18, D38 = col.Decimal128(18, 2), col.Decimal128(38, 4)


# ---- running and expecting --------------------------------------------------------------------
def fn_of(name, c):
    return F.get(name, [], [c.dtype] if c is not None else [])


def table_of(aggs, partial=True):
    return AggregateHashTable(AggregatorParams([], [fn_of(n, c) for n, c in aggs]), HashTableConfig(partial))


def feed(ht, aggs, rows, filt=None, batches=1, on_device=False):
    """`rows` rows of the aggregates' argument Columns (and the filter's) in `batches` add_groups calls."""
    bounds = np.linspace(0, rows, batches + 1).astype(int)
    for b in range(batches):
        lo, hi = int(bounds[b]), int(bounds[b + 1])
        ars = [None if c is None else slice_col(c, lo, hi) for _, c in aggs]
        fcols = [slice_col(c, lo, hi) for c in filt[1]] if filt is not None else None
        if on_device:
            ars = [None if c is None else DeviceColumn.from_host(c) for c in ars]
            fcols = [DeviceColumn.from_host(c) for c in fcols] if fcols is not None else None
        fp = FilterProgram(filt[0], fcols) if filt is not None else None
        ht.add_groups([], ars, rows=hi - lo, filter_program=fp, on_device=on_device)


def run(aggs, rows, filt=None, batches=1, on_device=False, staging=0, serialized=False):
    """The one result row (Columns) of the aggregates over `rows` rows; with serialized also the row
    of states.  Asserts that a non-empty input took the reduce kernel."""
    ht = table_of(aggs)
    try:
        if staging:
            ht.set_host_staging(staging)
        feed(ht, aggs, rows, filt, batches, on_device)
        block = ht.merge_result()
        ser = ht.result_serialized() if serialized else None
        launches = ht.keyless_stats()["reduce_launches"]
        assert (launches > 0) == (rows > 0), (launches, rows)
        assert ht.insert_paths() == dict.fromkeys(abi.INSERT_PATHS, 0)  # no table insert of any kind
    finally:
        ht.close()
    assert block.num_rows() == 1 and block.num_columns() == len(aggs)
    return (block.columns, ser.columns) if serialized else block.columns


def expected(aggs, rows, keep=None):
    """agg_ref's result over one group of the kept rows (keep: bool per row, None = all)."""
    keep = np.ones(rows, bool) if keep is None else np.asarray(keep, bool)
    n = int(keep.sum())
    if n == 0:  # FinalSingleStateAggregator::on_finish over freshly initialised states
        return [], [()], [(result_dtype(name, c), [0 if name == "count" else None]) for name, c in aggs]
    plain = []
    for name, c in aggs:
        vals = None if c is None else [v for v, k in zip(AC.from_column(c), keep) if k]
        plain.append((name, None if c is None else c.dtype, vals))
    _, cols = R.aggregate([], [()] * n, plain)
    return [], [()], cols


def got_of(cols):
    return [], [()], [(c.dtype, AC.from_column(c)) for c in cols]


def check(aggs, rows, keep=None, **kw):
    R.assert_exact(got_of(run(aggs, rows, **kw)), expected(aggs, rows, keep))


# ---- columns ----------------------------------------------------------------------------------
def typed_column(dt, n, rng, nullable):
    v = (rng.random(n) > 0.2) if nullable else None
    t = dt.type_id
    if t == abi.BOOLEAN:
        return Column.from_bools(rng.random(n) < 0.5, validity=v)
    if t == abi.DECIMAL128:
        if dt.precision <= 18:
            vals = [int(x) for x in rng.integers(-10**17, 10**17, n)]
        else:  # magnitudes past 2^64: the high word carries
            vals = [int(x) * 37 for x in rng.integers(-2**62, 2**62, n)]
        return Column.from_decimals(dt.precision, dt.scale, vals, validity=v)
    if t in R.FLOATS:  # quarters: every order of addition is exact
        return Column.from_numbers(dt, rng.integers(-4000, 4001, n) / 4.0, validity=v)
    if t == abi.DATE:
        return Column.from_numbers(dt, rng.integers(-100000, 100000, n), validity=v)
    info = np.iinfo(dt.np_dtype)
    return Column.from_numbers(dt, rng.integers(info.min, info.max, n, dtype=dt.np_dtype, endpoint=True), validity=v)


def functions_of(dt):
    if dt.type_id in (abi.DATE, abi.TIMESTAMP, abi.BOOLEAN):
        return ["count", "min", "max"]
    return ["count", "sum", "min", "max", "avg", "sql_avg"]


WIDTH_TYPES = [col.Int8, col.Int16, col.Int32, col.Int64, col.Float32, col.Float64, D18, D38, col.Date, col.Timestamp, col.Boolean]
ROW_COUNTS = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17]


# ---- 1. row counts, per type width --------------------------------------------------------------
@pytest.mark.parametrize("n", ROW_COUNTS)
@pytest.mark.parametrize("dt", WIDTH_TYPES, ids=repr)
def test_row_counts_per_type(dt, n):
    rng = np.random.default_rng([n, WIDTH_TYPES.index(dt)])
    x, xn = typed_column(dt, n, rng, False), typed_column(dt, n, rng, True)
    aggs = [("count", None)] + [(f, c) for c in (x, xn) for f in functions_of(dt)]
    check(aggs, n, on_device=ROW_COUNTS.index(n) % 2 == 0)


def test_grid_stride_wraps():
    """G * TILE + 5 rows: workgroup 0 takes a second, partial tile."""
    n = G * TILE + 5
    rng = np.random.default_rng(5)
    x = Column.from_numbers(col.Int16, rng.integers(-2**15, 2**15, n))
    aggs = [("count", None), ("sum", x), ("min", x), ("max", x), ("avg", x)]
    cols = run(aggs, n, on_device=True)
    vals = x.data.astype(np.int64).tolist()
    want = [n] + [R._aggregate_group(f, col.Int16, vals) for f in ("sum", "min", "max", "avg")]
    assert [AC.from_column(c)[0] for c in cols] == want


# ---- 2. alignment -------------------------------------------------------------------------------
def _struct(dt, n, data=0, validity=0, validity_offset=0, data_offset=0):
    c = abi.dbg_column()
    c.dt = dt.to_abi()
    c.data, c.validity, c.validity_offset, c.data_offset, c.len = data, validity, validity_offset, data_offset, n
    return c


def _resident(arr, on_device):
    """(something to keep alive, address) of a numpy buffer on the host or copied to the device."""
    if not on_device:
        return arr, arr.ctypes.data
    import torch
    t = torch.from_numpy(arr.view(np.uint8).copy()).cuda()
    return t, t.data_ptr()


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("dt", [col.Int8, col.Int16, col.Int32, col.Int64, D38], ids=repr)
def test_data_starts_inside_a_larger_buffer(dt, on_device):
    """The column's data starts k elements into its buffer, k = 0 .. 16 / width: every alignment a
    lane's 16-byte loads can meet.  One handle, reset between the offsets."""
    n = TILE + 77
    w = dt.width
    rng = np.random.default_rng(w)
    big = typed_column(dt, n + 16 // w + 1, rng, False)
    raw = np.ascontiguousarray(big.data).view(np.uint8)
    keep, base = _resident(raw, on_device)
    aggs = [("sum", big), ("min", big), ("max", big)]
    ht = table_of(aggs)
    try:
        for k in range(16 // w + 1):
            ht.reset()
            ht.add_groups_abi([], [_struct(dt, n, data=base + k * w)] * 3, n, on_device=on_device)
            view = slice_col(big, k, k + n)
            R.assert_exact(got_of(ht.merge_result().columns), expected([(f, view) for f, _ in aggs], n))
        assert ht.keyless_stats()["reduce_launches"] == 16 // w + 1
    finally:
        ht.close()


BIT_OFFSETS = [0, 1, 7, 8, 9, 63]


def _bitmap(bits, off, junk):
    """`bits` packed from bit `off` on, the bits before and after them set to `junk`."""
    pad = np.full(off, junk, bool)
    return np.packbits(np.concatenate([pad, np.asarray(bits, bool), np.full(64, junk, bool)]), bitorder="little")


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("off", BIT_OFFSETS)
def test_validity_starts_at_a_bit_offset(off, on_device):
    n = TILE + 77
    rng = np.random.default_rng(off)
    x = typed_column(col.Int32, n, rng, True)
    data_keep, data = _resident(np.ascontiguousarray(x.data), on_device)
    aggs = [("count", None), ("count", x), ("sum", x), ("min", x)]
    ht = table_of(aggs)
    try:
        for junk in (False, True):  # a reader that strays off the row's bits sees the opposite value
            ht.reset()
            keep, bits = _resident(_bitmap(x.validity, off, junk), on_device)
            s = _struct(x.dtype, n, data=data, validity=bits, validity_offset=off)
            ht.add_groups_abi([], [_struct(x.dtype, 0), s, s, s], n, on_device=on_device)
            R.assert_exact(got_of(ht.merge_result().columns), expected(aggs, n))
        assert ht.keyless_stats()["reduce_launches"] == 2
    finally:
        ht.close()


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("off", BIT_OFFSETS)
def test_boolean_data_starts_at_a_bit_offset(off, on_device):
    """MIN / MAX see every bit of the rows and none beside them: uniform data inside opposite junk,
    and one differing row at the first row, a tile's last row and the last row."""
    n = TILE + 77
    proto = Column.from_bools(np.zeros(1, bool))
    aggs = [("min", proto), ("max", proto)]
    ht = table_of(aggs)
    try:
        runs = [(np.zeros(n, bool), True), (np.ones(n, bool), False)]
        for r in (0, TILE - 1, n - 1):
            one = np.zeros(n, bool)
            one[r] = True
            runs += [(one, False), (~one, True)]
        for data, junk in runs:
            ht.reset()
            keep, bits = _resident(_bitmap(data, off, junk), on_device)
            s = _struct(col.Boolean, n, data=bits, data_offset=off)
            ht.add_groups_abi([], [s, s], n, on_device=on_device)
            mn, mx = (c.values()[0] for c in ht.merge_result().columns)
            assert (mn, mx) == (bool(data.min()), bool(data.max())), (off, junk)
        assert ht.keyless_stats()["reduce_launches"] == len(runs)
    finally:
        ht.close()


# ---- 3. value extremes --------------------------------------------------------------------------
VALUE_CASES = ["f64", "f32", "int_a", "int_b", "int_c", "int_d", "dec64", "dec128", "dec_wrap", "dec_avg_overflow"]


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case_id", VALUE_CASES)
def test_value_extremes(case_id, on_device):
    """The cases of tests/agg_cases.py (integer wraps, 128-bit carries, the float pool, Decimal limits,
    sql_avg ties) with every row in the one group, in two batches.  Aggregates whose collapsed sum
    leaves the Decimal range must raise; the others are compared."""
    b = AC.build(case_id, "i64")
    _, _, cols = expected(b.aggs, b.rows)
    bad = [i for i, (_, vals) in enumerate(cols) if vals[0] is R.OVERFLOW]
    good = [a for i, a in enumerate(b.aggs) if i not in bad]
    if good:
        check(good, b.rows, batches=2, on_device=on_device)
    for i in bad:
        with pytest.raises(DecimalOverflow):
            run([b.aggs[i]], b.rows, batches=2, on_device=on_device)
    assert bad or case_id != "dec_avg_overflow"


# ---- 4. NULLs and empties -----------------------------------------------------------------------
def _null_empty_aggs(n, all_null):
    rng = np.random.default_rng(4)
    x = Column.from_numbers(col.Int64, rng.integers(-99, 99, n))
    v = np.zeros(n, bool) if all_null else rng.random(n) > 0.5
    xn = Column.from_numbers(col.Int64, rng.integers(-99, 99, n), validity=v)
    i32 = Column.from_numbers(col.Int32, rng.integers(-99, 99, n))
    return [("count", None), ("count", xn), ("sum", x), ("sum", xn), ("avg", x), ("avg", xn), ("min", i32), ("max", xn)]


def _flag_bytes(ser_cols, aggs):
    """(NullUnary byte | None, OrNull byte | None) of each serialized state."""
    out = []
    for (name, c), s in zip(aggs, ser_cols):
        b = s.values()[0]
        if name == "count":
            assert len(b) == 8
            out.append((None, None))
        elif c.dtype.nullable:
            out.append((b[-2], b[-1]))
        else:
            out.append((None, b[-1]))
    return out


@pytest.mark.parametrize("mode", ["all_null_argument", "no_rows_ever", "every_row_filtered"])
def test_nulls_and_empties(mode):
    n = 0 if mode == "no_rows_ever" else TILE + 5
    aggs = _null_empty_aggs(n, mode == "all_null_argument")
    filt, keep = None, None
    if mode == "every_row_filtered":
        pos = Column.from_numbers(col.Int32, np.arange(n))
        filt, keep = (cmp(0, "<", 0), [pos]), np.zeros(n, bool)
    cols, ser = run(aggs, n, filt=filt, serialized=True, on_device=True)
    R.assert_exact(got_of(cols), expected(aggs, n, keep))
    flags = _flag_bytes(ser, aggs)
    seen = 1 if mode == "all_null_argument" else 0  # a row reached accumulate
    for (name, c), (null_unary, or_null), s in zip(aggs, flags, ser):
        if name == "count":
            continue
        assert or_null == seen, (name, c.dtype)
        if null_unary is not None:  # a non-NULL value reached the state
            assert null_unary == 0, (name, c.dtype)
        if not seen:  # the initial state: zeros, or None
            body = s.values()[0][:-1 if null_unary is None else -2]
            assert body == (b"\x00" if name in ("min", "max") else bytes(len(body))), (name, body)
    if seen:
        vals = [c.values()[0] for c in cols]
        assert vals[0] == n and vals[1] == 0 and vals[3] is None and vals[5] is None and vals[7] is None
        assert vals[2] is not None and vals[6] is not None


# ---- 5. predicates ------------------------------------------------------------------------------
N_PRED = 3 * TILE + 17
PRED_CASES = pred_cases.generic_agg_cases(N_PRED)
# the hand-written tail of the logic cases (De Morgan pairs, TRUE, IS [NOT] NULL inside AND / OR / NOT) and four plain nestings
LOGIC = pred_cases.logic_cases()[-15:] + [c for c in pred_cases.logic_cases()
                                          if c[0] in ("logic not(c0)", "logic and(c0,c1)", "logic or(c1,c2)", "logic or(not(c0),and(c1,c2))")]
COLCOL = pred_cases.colcol_cases("Int32")[::5] + pred_cases.colcol_cases("Float64")[::7]


@pytest.mark.parametrize("case", PRED_CASES, ids=[c[0] for c in PRED_CASES])
def test_predicates_over_count_and_sum(case):
    _, fcols, pred = case
    v = pred_cases.agg_inputs(N_PRED)["v"]
    keep = pred_ref.evaluate(pred, fcols, N_PRED) == pred_ref.TRUE
    check([("count", None), ("sum", v)], N_PRED, keep, filt=(pred, fcols), on_device=PRED_CASES.index(case) % 2 == 0)


@pytest.mark.parametrize("case", LOGIC + COLCOL, ids=[c[0] for c in LOGIC + COLCOL])
def test_three_valued_logic_and_column_comparisons(case):
    _, fcols, pred = case
    n = pred_cases.N
    v = Column.from_numbers(col.Int64, np.arange(n) * 3 - 7)
    keep = pred_ref.evaluate(pred, fcols, n) == pred_ref.TRUE
    check([("count", None), ("sum", v)], n, keep, filt=(pred, list(fcols)), on_device=True)


def _urls(n):
    rng = np.random.default_rng(21)
    hosts = [b"http://example.com/", b"https://www.google.com/search?q=", b"http://goo.gl/", b"", b"http://maps.google.de/x"]
    rows = [hosts[i] + b"p%d" % j for j, i in enumerate(rng.integers(0, len(hosts), n))]
    return Column.from_strings(rows, validity=rng.random(n) > 0.1)


@pytest.mark.parametrize("on_device,staging", [(True, 0), (False, 0), (False, 1 << 20)], ids=["device", "host", "host_staged"])
@pytest.mark.parametrize("which", ["like", "not_like", "like_and_cmp"])
def test_like_predicates(which, on_device, staging):
    n = 2 * TILE + 100
    url = _urls(n)
    num = Column.from_numbers(col.Int32, np.arange(n) % 7)
    pred = {"like": like(0, b"%google%"), "not_like": not_like(0, b"%google%"),
            "like_and_cmp": and_(like(0, b"%google%"), cmp(1, "<", 3))}[which]
    fcols = [url, num]
    keep = like_ref.evaluate(pred, fcols, n) == pred_ref.TRUE
    assert 0 < keep.sum() < n
    check([("count", None), ("sum", num)], n, keep, filt=(pred, fcols), on_device=on_device, staging=staging, batches=2)


# ---- 6. batching and determinism ------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["host", "host_staged", "device"])
def test_same_rows_in_1_2_5_batches(mode):
    n = 2 * TILE + 333
    rng = np.random.default_rng(6)
    a, b, f = typed_column(col.Int64, n, rng, True), typed_column(D38, n, rng, False), typed_column(col.Float64, n, rng, True)
    aggs = [("count", None), ("sum", a), ("avg", a), ("sum", b), ("min", b), ("sum", f), ("max", f), ("sql_avg", b)]
    want = expected(aggs, n)
    for batches in (1, 2, 5):
        got = run(aggs, n, batches=batches, on_device=mode == "device", staging=1 << 12 if mode == "host_staged" else 0)
        R.assert_exact(got_of(got), want)


def _float_sum_bits(x, batches):
    c = Column.from_numbers(col.Float64, x)
    return AC.from_column(run([("sum", c)], len(x), batches=batches, on_device=True)[0])[0]


def test_float_sum_is_deterministic():
    """Same rows and same batching: the same bits on every run.  Against math.fsum the project's
    1e-12 relative holds where the sum is well-conditioned; an ill-conditioned sum is
    held to run-to-run identity only."""
    n = 3 * TILE + 17
    rng = np.random.default_rng(66)
    well = rng.random(n) + 0.5
    ill = rng.standard_normal(n) * 10.0 ** rng.integers(-12, 13, n)
    ill[1::2] = -ill[0::2][: len(ill[1::2])] * (1 + 1e-9)  # heavy cancellation
    for x in (well, ill):
        for batches in (1, 3):
            assert _float_sum_bits(x, batches) == _float_sum_bits(x, batches)
    exact = math.fsum(well)
    assert abs(R.bits_f64(_float_sum_bits(well, 1)) - exact) <= 1e-12 * abs(exact)


def test_reset_then_reuse():
    n = TILE + 9
    rng = np.random.default_rng(7)
    x, y = typed_column(col.Int32, n, rng, True), typed_column(col.Int32, 77, rng, True)
    ht = table_of([("count", None), ("sum", x), ("max", x)])
    try:
        feed(ht, [("count", None), ("sum", x), ("max", x)], n, on_device=True)
        R.assert_exact(got_of(ht.merge_result().columns), expected([("count", None), ("sum", x), ("max", x)], n))
        ht.reset()
        R.assert_exact(got_of(ht.merge_result().columns), expected([("count", None), ("sum", x), ("max", x)], 0))
        feed(ht, [("count", None), ("sum", y), ("max", y)], 77)
        R.assert_exact(got_of(ht.merge_result().columns), expected([("count", None), ("sum", y), ("max", y)], 77))
        assert ht.keyless_stats()["reduce_launches"] == 2 and ht.retained_bytes() > 0
        assert ht.compact() is False
    finally:
        ht.close()


# ---- 7. many aggregates, and each kind alone --------------------------------------------------------
def _kind_columns(n):
    rng = np.random.default_rng(32)
    return {"i16": typed_column(col.Int16, n, rng, False), "i64n": typed_column(col.Int64, n, rng, True),
            "u32": Column.from_numbers(col.UInt32, rng.integers(0, 2**32, n)), "f32n": typed_column(col.Float32, n, rng, True),
            "f64": typed_column(col.Float64, n, rng, False), "d18": typed_column(D18, n, rng, False),
            "d38n": typed_column(D38, n, rng, True), "date": typed_column(col.Date, n, rng, False),
            "bool": typed_column(col.Boolean, n, rng, True)}


KINDS = [("count", None), ("count", "i64n"), ("sum", "i16"), ("sum", "i64n"), ("sum", "u32"), ("sum", "f32n"), ("sum", "f64"),
         ("sum", "d18"), ("sum", "d38n"), ("avg", "i16"), ("avg", "f64"), ("avg", "d18"), ("avg", "d38n"), ("sql_avg", "d18"),
         ("sql_avg", "i64n"), ("min", "i16"), ("max", "i64n"), ("min", "u32"), ("max", "u32"), ("min", "f32n"), ("max", "f64"),
         ("min", "d18"), ("max", "d18"), ("min", "d38n"), ("max", "d38n"), ("min", "date"), ("max", "date"), ("min", "bool"),
         ("max", "bool"), ("count", "bool"), ("avg", "u32"), ("sum", "i16")]
N_KINDS = TILE + 41


def test_32_aggregates_in_one_handle():
    assert len(KINDS) == 32
    c = _kind_columns(N_KINDS)
    check([(f, None if k is None else c[k]) for f, k in KINDS], N_KINDS, on_device=True, batches=2)


@pytest.mark.parametrize("kind", KINDS[:-1], ids=[f"{f}_{k}" for f, k in KINDS[:-1]])
def test_each_kind_alone(kind):
    f, k = kind
    check([(f, None if k is None else _kind_columns(N_KINDS)[k])], N_KINDS, on_device=True)


# ---- 8. serialized round trips --------------------------------------------------------------------
def _final_of(aggs, blocks):
    """Result columns of a final handle after merging blocks of serialized states (all rows of each)."""
    final = table_of(aggs, partial=False)
    try:
        for cols in blocks:
            final.merge_serialized(cols, [], rows=len(cols[0]))
        assert final.keyless_stats() == {"reduce_launches": 0, "merged_states": sum(len(c[0]) for c in blocks)}
        return final.merge_result().columns
    finally:
        final.close()


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_partials_to_final(on_device):
    """Three partial handles over three row ranges, the middle one empty, through result_serialized
    and merge_serialized: equal to the direct result and to the reference."""
    n = 2 * TILE + 50
    rng = np.random.default_rng(8)
    a, an, d, f = (typed_column(col.Int32, n, rng, False), typed_column(col.Int64, n, rng, True), typed_column(D38, n, rng, True),
                   typed_column(col.Float32, n, rng, False))
    aggs = [("count", None), ("count", an), ("sum", a), ("avg", an), ("min", d), ("sum", d), ("max", f), ("avg", f), ("min", a)]
    blocks = []
    for lo, hi in ((0, TILE + 3), (TILE + 3, TILE + 3), (TILE + 3, n)):
        part = [(name, None if c is None else slice_col(c, lo, hi)) for name, c in aggs]
        _, ser = run(part, hi - lo, serialized=True, on_device=on_device)
        blocks.append(ser)
    got = _final_of(aggs, blocks)
    R.assert_exact(got_of(got), expected(aggs, n))
    R.assert_exact(got_of(got), got_of(run(aggs, n, on_device=on_device)))


CRAFTED = list(AC.crafted_cases())


@pytest.mark.parametrize("case_id", CRAFTED)
def test_crafted_states_merge(case_id):
    """agg_cases' crafted states (counts above 2^32, the SUM range check at +-(10^38 - 1) / +-10^38,
    wrapping sums, the float pool) as the rows of one block per group, into one reused final handle."""
    name, dt, groups = AC.crafted_cases()[case_id]
    proto = AC.to_column(dt, [])
    final = table_of([(name, proto)], partial=False)
    try:
        for key, states in groups.items():
            final.reset()
            block = Column.from_strings([AC.state_bytes(name, dt, *s) for s in states])
            final.merge_serialized([block], [], rows=len(states), on_device=False)
            want = AC._merged(name, dt, states)
            if want is R.OVERFLOW:
                with pytest.raises(DecimalOverflow):
                    final.merge_result()
                continue
            R.assert_exact(got_of(final.merge_result().columns), ([], [()], [(result_dtype(name, proto), [want])]))
        assert final.keyless_stats()["merged_states"] == sum(len(s) for s in groups.values())
    finally:
        final.close()


def test_flag_zero_states_merge_as_nothing_seen():
    dt = col.Int64
    proto = AC.to_column(dt, [])
    off = lambda b: b[:-1] + b"\x00"  # the OrNull adaptor's byte: no row reached the state
    aggs = [("sum", proto), ("avg", proto), ("min", proto)]
    real = [AC.state_bytes("sum", dt, 41), AC.state_bytes("avg", dt, 10, 4), AC.state_bytes("min", dt, -3)]
    empty = [off(AC.state_bytes("sum", dt, 0)), off(AC.state_bytes("avg", dt, 0, 0)), b"\x00\x00"]  # MinMaxAnyState None
    stale = [off(AC.state_bytes("sum", dt, 0)), off(AC.state_bytes("avg", dt, 99, 5)), b"\x00\x00"]  # flag 0 over a count
    block = lambda rows: [Column.from_strings([r[a] for r in rows]) for a in range(3)]
    vals = lambda cols: [c.values()[0] for c in cols]
    assert vals(_final_of(aggs, [block([empty, real, empty])])) == [41, 2.5, -3]
    assert vals(_final_of(aggs, [block([empty]), block([empty, empty])])) == [None, None, None]
    assert vals(_final_of(aggs, [block([stale, real])])) == [41, 2.5, -3]


def test_short_state_is_invalid():
    proto = AC.to_column(col.Int64, [])
    final = table_of([("sum", proto)], partial=False)
    try:
        good = AC.state_bytes("sum", col.Int64, 5)
        with pytest.raises(DbgError) as e:
            final.merge_serialized([Column.from_strings([good, good[1:]])], [], rows=2)
        assert e.value.code == abi.DBG_ERR_INVALID
        assert final.merge_result().columns[0].values() == [None]  # nothing was merged
    finally:
        final.close()


def test_serialized_bytes_of_non_nullable_arguments():
    n = TILE + 3
    rng = np.random.default_rng(88)
    i64, i32, f64, d = (typed_column(col.Int64, n, rng, False), typed_column(col.Int32, n, rng, False),
                        typed_column(col.Float64, n, rng, False), typed_column(D38, n, rng, False))
    aggs = [("sum", i64), ("avg", i64), ("min", i32), ("max", f64), ("sum", d), ("avg", d), ("count", None)]
    _, ser = run(aggs, n, serialized=True, on_device=True)
    vi, vd = AC.from_column(i64), AC.from_column(d)
    want = [AC.state_bytes("sum", col.Int64, R.wrap(sum(vi), 64, True)), AC.state_bytes("avg", col.Int64, R.wrap(sum(vi), 64, True), n),
            AC.state_bytes("min", col.Int32, min(AC.from_column(i32))),
            AC.state_bytes("max", col.Float64, R._aggregate_group("max", col.Float64, AC.from_column(f64))),
            AC.state_bytes("sum", D38, R.wrap(sum(vd), 128, True)), AC.state_bytes("avg", D38, R.wrap(sum(vd), 128, True), n),
            n.to_bytes(8, "little")]
    assert [s.values()[0] for s in ser] == want


# ---- 9. processor mirrors -------------------------------------------------------------------------
def test_single_state_processors():
    """Blocks of 65,536 rows through two partials into one final."""
    rows, nblocks = 65536, 4
    rng = np.random.default_rng(9)
    blocks = [DataBlock([typed_column(col.Int16, rows, rng, False), typed_column(col.Int64, rows, rng, True),
                         Column.from_numbers(col.Int32, rng.integers(0, 10, rows))]) for _ in range(nblocks)]
    fns = [F.get("count"), F.get("sum", [], [col.Int16]), F.get("avg", [], [col.Int16]), F.get("max", [], [col.Int64.wrap_nullable()])]
    params = AggregatorParams([], fns)
    arg_indices = [None, 0, 0, 1]
    final = FinalSingleStateAggregator(params)
    for half in (blocks[:2], blocks[2:]):
        p = PartialSingleStateAggregator(params)
        try:
            for b in half:
                assert p.transform(b, arg_indices, FilterProgram(cmp(0, "<>", 3), [b.columns[2]])) == []
            out = p.on_finish()
            assert len(out) == 1 and out[0].num_rows() == 1 and out[0].num_columns() == 4
            assert p.state.keyless_stats()["reduce_launches"] == 1  # host staging gathered the blocks
            final.transform(out[0])
        finally:
            p.close()
    whole = [Column.from_numbers(col.Int16, np.concatenate([b.columns[0].data for b in blocks])),
             Column.from_numbers(col.Int64, np.concatenate([b.columns[1].data for b in blocks]),
                                 validity=np.concatenate([b.columns[1].validity for b in blocks]))]
    keep = np.concatenate([b.columns[2].data for b in blocks]) != 3
    aggs = [("count", None), ("sum", whole[0]), ("avg", whole[0]), ("max", whole[1])]
    R.assert_exact(got_of(final.on_finish().columns), expected(aggs, rows * nblocks, keep))
    # a final that collected nothing still emits its one row
    R.assert_exact(got_of(FinalSingleStateAggregator(params).on_finish().columns), expected(aggs, 0))


# ---- 10. refusals ---------------------------------------------------------------------------------
def test_table_entry_points_are_refused_and_the_handle_lives_on():
    import torch
    n = TILE + 1
    x = Column.from_numbers(col.Int64, np.arange(n))
    aggs = [("count", None), ("sum", x)]
    ht = table_of(aggs)
    L, h = lib(), None
    u64 = lambda k: (C.c_uint64 * k)()
    u32 = lambda k: (C.c_uint32 * k)()
    dummy = torch.zeros(64, dtype=torch.uint8, device="cuda")
    ptr = dummy.data_ptr()
    try:
        feed(ht, aggs, n, on_device=True)
        h = ht.h
        out_a, out_k, groups = (abi.dbg_out_column * 2)(), (abi.dbg_out_column * 1)(), C.c_uint64()
        p, keep = ht.params.to_abi(True, 0, -1)
        arg = (abi.dbg_column * 2)()
        calls = {
            "set_strategy(PARTITIONED)": lambda: L.dbg_agg_set_strategy(h, abi.STRATEGY_PARTITIONED),
            "partition": lambda: L.dbg_agg_partition(h, 4, 0, u64(4), u64(4)),
            "export_records": lambda: L.dbg_agg_export_records(h, ptr, ptr),
            "merge_records": lambda: L.dbg_agg_merge_records(h, ptr, ptr, 0, u64(1), u64(1)),
            "export_fixed": lambda: L.dbg_agg_export_fixed(h, ptr, 16),
            "merge_fixed": lambda: L.dbg_agg_merge_fixed(h, ptr, 1, 16),
            "payload_counts": lambda: L.dbg_agg_payload_counts(h, u64(512), u32(2)),
            "payload_counts_from": lambda: L.dbg_agg_payload_counts_from(h, u32(2), u64(512), u32(2), u32(2)),
            "payload_export": lambda: L.dbg_agg_payload_export(h, 2, ptr),
            "payload_export_from": lambda: L.dbg_agg_payload_export_from(h, 2, u32(2), ptr),
            "payload_import": lambda: L.dbg_agg_payload_import(h, 2, 0, u64(1024), ptr, ptr),
            "payload_import_chunks": lambda: L.dbg_agg_payload_import_chunks(h, 2, 0, 1, u64(1024), (C.c_void_p * 1)(ptr),
                                                                             (C.c_void_p * 1)(ptr)),
            "exchange_payload": lambda: L.dbg_agg_exchange_payload(None, h, None),
            "exchange_payload_chunk": lambda: L.dbg_agg_exchange_payload_chunk(None, h, 1, None),
            "exchange": lambda: L.dbg_agg_exchange(None, h, h, None),
            "payload_exchange_plan": lambda: L.dbg_payload_exchange_plan(C.byref(p), 2, 0, u64(1024), u32(2), u64(2), u64(2)),
            "merge_exchange_plan": lambda: L.dbg_merge_exchange_plan(C.byref(p), 2, 0, u64(4), u32(1), u64(2), u64(2), u64(2)),
            "record_layout": lambda: L.dbg_agg_record_layout(C.byref(p), C.byref(abi.dbg_record_layout())),
            "record_width": lambda: L.dbg_agg_record_width(h, u32(1)),
            "set_partition_keys": lambda: L.dbg_agg_set_partition_keys(h, 0),
            "set_recycle(1)": lambda: L.dbg_agg_set_recycle(h, 1),
            "capacity": lambda: L.dbg_agg_capacity(h, u64(1)),
            "finalize_into": lambda: L.dbg_agg_finalize_into(h, out_a, out_k, 1, None, C.byref(groups), None),
            "finalize_into_async": lambda: L.dbg_agg_finalize_into_async(h, out_a, out_k, 1, None),
            "step_async": lambda: L.dbg_agg_step_async(h, None, arg, None, 1, out_a, out_k, 1, None),
        }
        for name, call in calls.items():
            assert call() == abi.DBG_ERR_UNSUPPORTED, name
            assert b"no group columns" in L.dbg_last_error(), (name, L.dbg_last_error())
        assert L.dbg_agg_set_recycle(h, 0) == abi.DBG_OK and L.dbg_agg_set_strategy(h, abi.STRATEGY_TABLE) == abi.DBG_OK
        R.assert_exact(got_of(ht.merge_result().columns), expected(aggs, n))
        assert ht.keyless_stats()["reduce_launches"] == 1
    finally:
        ht.close()


def test_specs_refused_at_create():
    s = Column.from_strings([b"a"])
    d256 = Column.from_decimals(50, 2, [1])
    x = Column.from_numbers(col.Int64, [1])
    for fns in ([F.get("min", [], [s.dtype])], [F.get("max", [], [s.dtype.wrap_nullable()])], [F.get("sum", [], [d256.dtype])],
                [F.get("count", [], [d256.dtype])], [F.get_or_null("sum", [], [x.dtype], False)], []):
        with pytest.raises(Unsupported, match="no group columns"):
            AggregateHashTable(AggregatorParams([], fns))
    ok = AggregateHashTable(AggregatorParams([], [F.get("count", [], [s.dtype.wrap_nullable()])]))  # COUNT(string) counts valid rows
    ok.close()


def test_keyed_handle_is_unaffected():
    """One small grouped parity case before and after a keyless handle lived on the same device; the
    keyless counters are the keyless handle's alone."""
    rng = np.random.default_rng(10)
    n = 5000
    k = Column.from_numbers(col.Int32, rng.integers(0, 37, n))
    v = typed_column(col.Int64, n, rng, True)
    aggs = [("count", None), ("sum", v), ("min", v)]
    plain = [(name, None if c is None else c.dtype, None if c is None else AC.from_column(c)) for name, c in aggs]
    ek, ec = R.aggregate([col.Int32], [(int(x),) for x in k.data], plain)

    def keyed():
        gk, ga = gpu_aggregate([k], aggs, on_device=True)
        R.assert_exact(AC.plain_result(gk, ga), ([col.Int32], ek, ec))

    keyed()
    check(aggs, n, on_device=True)
    keyed()
    ht = AggregateHashTable(AggregatorParams([col.Int32], [F.get("count")]))
    try:
        assert lib().dbg_agg_keyless_stats(ht.h, None, None) == abi.DBG_ERR_INVALID
    finally:
        ht.close()
