"""The date / time functions and length() of the device projection (dbg_expr_eval,
databend_amd/csrc/expr.hip) on the GPU: the function case of the node loop in the narrow and the
wide instantiation, and the length() pre-pass.

Expected values and types come from tests/datetime_ref.py (plain Python integers, pinned by the
reference's recorded results and by Python's datetime); the end-to-end cases compare with
tests/agg_ref.py.  Every comparison is exact and validity bits are exact; the data of NULL rows and
of rows the filter drops are not compared.  Outputs are written into buffers with guard bytes on
both sides, which must stay untouched."""
import numpy as np
import pytest

from databend_amd import abi
from databend_amd import column as col
from databend_amd import expr as X
from databend_amd.column import DataType
from databend_amd.ffi import check, lib
from databend_amd.filter import FilterProgram, cmp
from tests import agg_cases as AC
from tests import agg_ref as AR
from tests import datetime_ref as D

pytestmark = pytest.mark.gpu
GUARD = 64
ROW_COUNTS = [0, 1, 7, 8, 9, 63, 64, 65, 2047, 2048, 2049, 2 * 2048 * 4 + 5]  # test_gpu_expr.py's
# (element offset, validity bit offset) of the input views, and whether the outputs start one
# element past a 16-byte boundary
VIEWS = [(0, 0, False), (1, 1, True), (3, 7, True)]
GARBAGE = {abi.DATE: [-(1 << 31), (1 << 31) - 1, 0x55555555], abi.TIMESTAMP: [-(1 << 63), (1 << 63) - 1, 0x5555555555555555]}


def _torch():
    import torch
    return torch


def dev_col(t: DataType, values, elem_off=0, vbit_off=0):
    """A device view of Date / Timestamp / number `values` (None = NULL, stored as out-of-range
    garbage) that starts elem_off elements into its buffer and vbit_off bits into its bitmap."""
    torch = _torch()
    g = GARBAGE.get(t.type_id, [0])
    filled = [g[i % len(g)] if v is None else v for i, v in enumerate(values)]
    data = np.array(filled, dtype=t.np_dtype).view(np.uint8)
    buf = np.concatenate([np.full(elem_off * t.width, 0xEE, np.uint8), data, np.full(1, 0xEE, np.uint8)])
    d = torch.from_numpy(buf).cuda()
    c = abi.dbg_column()
    c.dt = t.to_abi()
    c.data = d.data_ptr() + elem_off * t.width
    c.len = len(values)
    keep = [d]
    if t.nullable:
        bits = np.concatenate([np.ones(vbit_off, bool), np.array([v is not None for v in values], bool)])
        v = torch.from_numpy(np.concatenate([np.packbits(bits, bitorder="little"), np.zeros(1, np.uint8)])).cuda()
        c.validity = v.data_ptr()
        c.validity_offset = vbit_off
        keep.append(v)
    return c, keep


def str_col(strings, first_row=0, nullable=False, vbit_off=0, lead=0):
    """A device String column of `strings` (bytes; None = NULL, stored as an empty cell) seen from
    row first_row on; `lead` bytes precede the first string in the blob."""
    torch = _torch()
    cells = [b"" if s is None else s for s in strings]
    blob = b"\xbf" * lead + b"".join(cells)
    offs = np.concatenate([[lead], lead + np.cumsum([len(s) for s in cells])]).astype(np.uint64)
    d = torch.from_numpy(np.frombuffer(blob + b"\xbf" * 32, dtype=np.uint8).copy()).cuda()
    o = torch.from_numpy(offs.view(np.int64).copy()).cuda()
    c = abi.dbg_column()
    c.dt = (col.String.wrap_nullable() if nullable else col.String).to_abi()
    c.data = d.data_ptr()
    c.offsets = o.data_ptr() + 8 * first_row
    c.len = len(strings) - first_row
    keep = [d, o]
    if nullable:
        bits = np.concatenate([np.ones(vbit_off, bool), np.array([s is not None for s in strings[first_row:]], bool)])
        v = torch.from_numpy(np.concatenate([np.packbits(bits, bitorder="little"), np.zeros(1, np.uint8)])).cuda()
        c.validity = v.data_ptr()
        c.validity_offset = vbit_off
        keep.append(v)
    return c, keep


def run(exprs, cols, rows, filt=None, odd_outputs=False):
    """exprs: library expressions; cols: [(dbg_column, keep)].  Returns [(type, values)] with None for
    NULL rows; checks the guard bytes and the validity bits past the last row."""
    torch = _torch()
    prog = X.ExprProgram(exprs, [c for c, _ in cols])
    types = prog.result_types()
    arr = (abi.dbg_out_column * len(types))()
    bufs = []
    for k, t in enumerate(types):
        lead = GUARD + (t.width if odd_outputs else 0)
        d = torch.full((lead + rows * t.width + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        v = torch.full((GUARD + (rows + 7) // 8 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda") if t.nullable else None
        arr[k].data = d.data_ptr() + lead
        if v is not None:
            arr[k].validity = v.data_ptr() + GUARD
        bufs.append((d, v, lead))
    fp = filt.ptr() if filt is not None else None
    check(lib().dbg_expr_eval(prog.ptr(), fp, rows, arr, torch.cuda.current_stream().cuda_stream))
    out = []
    for k, (t, (d, v, lead)) in enumerate(zip(types, bufs)):
        assert DataType.from_abi(arr[k].dt) == t
        raw = d.cpu().numpy()
        assert (raw[:lead] == 0xA5).all() and (raw[lead + rows * t.width:] == 0xA5).all(), "data guard bytes were written"
        cells = raw[lead:lead + rows * t.width].copy()
        vals = col.i128_from_bytes(cells) if t.type_id == abi.DECIMAL128 else [int(x) for x in cells.view(t.np_dtype)]
        if v is not None:
            vr = v.cpu().numpy()
            nb = (rows + 7) // 8
            assert (vr[:GUARD] == 0xA5).all() and (vr[GUARD + nb:] == 0xA5).all(), "validity guard bytes were written"
            bits = np.unpackbits(vr[GUARD:GUARD + nb], bitorder="little")
            assert not bits[rows:].any(), "validity bits past the last row are set"
            vals = [x if b else None for x, b in zip(vals, bits[:rows])]
        out.append((t, vals))
    return out


def want_of(name, t, values):
    return D.result_type(name, t), [None if v is None else D.evaluate(name, t, v) for v in values]


def assert_same(got, want, what=""):
    (gt, gv), (wt, wv) = got, want
    assert gt == wt, (what, gt, wt)
    assert len(gv) == len(wv)
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(gv, wv)) if w != "unselected" and g != w]
    assert not bad, (what, bad[:5], len(bad))


def cycle(vals, n, seed):
    rng = np.random.default_rng(seed)
    idx = np.concatenate([np.arange(len(vals)), rng.integers(0, len(vals), max(0, n - len(vals)))])[:n]
    return [vals[int(i)] for i in idx]


def with_nulls(vals, seed, frac=0.2):
    rng = np.random.default_rng(seed)
    return [None if rng.random() < frac else v for v in vals]


def yyyymm_by_operators(e):
    return X.to_year(e) * 100 + X.to_month(e)


# ---- row counts and views ----------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ROW_COUNTS)
def test_row_counts_and_views(rows):
    """The lane, wave, strip and tile edges, at three views; the nullable Timestamp's NULL rows hold
    out-of-range garbage: they must not raise and their validity must be 0."""
    tt, td = col.Timestamp.wrap_nullable(), col.Date
    ts = with_nulls(cycle(D.edge_timestamps(), rows, 1), 2)
    ds = cycle(D.edge_dates(), rows, 3)
    e_ts, e_d = X.col(0), X.col(1)
    exprs = [X.to_minute(e_ts), X.to_start_of_minute(e_ts), X.to_monday(e_ts), X.to_year(e_d), X.to_yyyymm(e_d), yyyymm_by_operators(e_d),
             X.to_start_of_iso_year(e_d)]
    want = [want_of("to_minute", tt, ts), want_of("to_start_of_minute", tt, ts), want_of("to_monday", tt, ts), want_of("to_year", td, ds),
            want_of("to_yyyymm", td, ds), (col.UInt64, want_of("to_yyyymm", td, ds)[1]), want_of("to_start_of_iso_year", td, ds)]
    for eo, vo, odd in VIEWS:
        got = run(exprs, [dev_col(tt, ts, eo, vo), dev_col(td, ds, eo, 0)], rows, odd_outputs=odd)
        for k, (g, w) in enumerate(zip(got, want)):
            assert_same(g, w, (k, rows, eo, vo, odd))
    if rows > 100:
        assert any(v is None for v in ts)


# ---- every function over the edge values ------------------------------------------------------------------
def function_groups(names, size=8):
    return [names[i:i + size] for i in range(0, len(names), size)]


@pytest.mark.parametrize("names", function_groups(D.DATE_FUNCS), ids=lambda n: n[0])
def test_every_function_over_dates(names):
    rows = 2048 + 300
    t = col.Date.wrap_nullable()
    vals = with_nulls(cycle(D.edge_dates() + D.sweep_dates(300, 31), rows, 4), 5, 0.1)
    vals[:len(D.edge_dates())] = D.edge_dates()
    got = run([X.col(0).func(n) for n in names], [dev_col(t, vals, 1, 3)], rows)
    for n, g in zip(names, got):
        assert_same(g, want_of(n, t, vals), n)
    got = run([X.col(0).func(n) for n in names], [dev_col(col.Date, D.edge_dates())], len(D.edge_dates()))
    for n, g in zip(names, got):
        assert_same(g, want_of(n, col.Date, D.edge_dates()), n)


@pytest.mark.parametrize("names", function_groups(D.TS_FUNCS), ids=lambda n: n[0])
def test_every_function_over_timestamps(names):
    rows = 2048 + 300
    t = col.Timestamp
    edges = D.edge_timestamps()
    vals = cycle(edges + D.sweep_timestamps(300, 32), rows, 6)
    assert vals[:len(edges)] == edges and {-100, -59999900, 0, 1, -1, D.TS_MIN, D.TS_MAX} <= set(edges)
    got = run([X.col(0).func(n) for n in names], [dev_col(t, vals)], rows)
    for n, g in zip(names, got):
        assert_same(g, want_of(n, t, vals), n)


def test_mixed_program_equals_to_yyyymm():
    """to_year(d) * 100 + to_month(d) = to_yyyymm(d): a function's number result feeds the operators."""
    rows = 4099
    for t, vals in ((col.Date, cycle(D.edge_dates() + D.sweep_dates(500, 33), rows, 7)),
                    (col.Timestamp.wrap_nullable(), with_nulls(cycle(D.edge_timestamps() + D.sweep_timestamps(500, 34), rows, 8), 9))):
        a, b = run([yyyymm_by_operators(X.col(0)), X.to_yyyymm(X.col(0))], [dev_col(t, vals)], rows)
        assert a[0].remove_nullable() == col.UInt64 and b[0].remove_nullable() == col.UInt32 and a[0].nullable == b[0].nullable == t.nullable
        assert a[1] == b[1] == want_of("to_yyyymm", t, vals)[1]


def test_functions_in_the_wide_instantiation():
    """A Decimal128 beside the function: to_year(d) * price (UInt16 x Decimal(10, 2)) and a function
    result stored from a 128-bit program, one row per lane."""
    P = col.Decimal128(10, 2)
    for rows in (1, 65, 2049 + 70):
        ds = with_nulls(cycle(D.edge_dates(), rows, 10), 11)
        ps = [(-1) ** i * (i * 7919 % 10 ** 9) for i in range(rows)]
        td = col.Date.wrap_nullable()
        data = torch_i128(ps)
        c = abi.dbg_column()
        c.dt = P.to_abi()
        c.data = data.data_ptr()
        c.len = rows
        got = run([X.to_year(X.col(0)) * X.col(1), X.to_start_of_month(X.col(0)), X.to_day_of_week(X.col(0))],
                  [dev_col(td, ds, 1, 5), (c, [data])], rows)
        years = want_of("to_year", td, ds)[1]
        assert got[0][0] == col.Decimal128(15, 2).wrap_nullable()
        assert_same((got[1][0], got[1][1]), want_of("to_start_of_month", td, ds))
        assert_same((got[2][0], got[2][1]), want_of("to_day_of_week", td, ds))
        assert got[0][1] == [None if y is None else y * p for y, p in zip(years, ps)]


def torch_i128(values):
    return _torch().from_numpy(col.i128_to_bytes(values).copy()).cuda()


# ---- length() --------------------------------------------------------------------------------------------
def lengths(cols, rows, exprs=None):
    return run(exprs or [X.length(X.col(0))], cols, rows)


def check_length(strings, first_row=0, nullable=False, vbit_off=0, lead=0):
    rows = len(strings) - first_row
    t = col.String.wrap_nullable() if nullable else col.String
    got = lengths([str_col(strings, first_row, nullable, vbit_off, lead)], rows)[0]
    want = [None if s is None else D.length(s) for s in strings[first_row:]]
    assert_same(got, (D.result_type("length", t), want), (rows, first_row, lead))


def test_length_of_small_columns():
    u = [s.encode("utf-8") for s in D.LENGTH_STRINGS]
    check_length([b""])
    check_length(u)
    check_length(u, lead=1)
    check_length(u, lead=13)
    # ends exactly on a 16-byte chunk boundary and one byte either side (the blob is 16-byte aligned)
    check_length([b"x" * 15, b"y", b"z", b"w" * 14, "é".encode(), b"q"])
    check_length([b"x" * 16, b"", b"y" * 16, b"", b"", "€".encode() * 5 + b"z"])
    # stray continuation bytes and bytes that are no UTF-8 at all: counted by the rule, nothing raised
    check_length([b"\x80\x80a\xbf", b"\xc3", b"\xff\xfe\x80", b"\xbf" * 40, bytes(range(256))])


def test_length_all_rows_empty():
    for rows in (1, 1023, 1024, 1025, 3000):
        check_length([b""] * rows)


def test_length_across_workgroups_and_tiles():
    """More rows than one workgroup takes (1024), strings of mixed widths so that the byte span of a
    workgroup begins and ends inside a 16-byte chunk, and enough bytes for several 4 KiB tiles."""
    rng = np.random.default_rng(41)
    alphabet = ["a", "é", "€", "\U0001f600", "z", "я", ""]
    strings = ["".join(alphabet[int(i)] for i in rng.integers(0, len(alphabet), int(n))).encode("utf-8")
               for n in rng.integers(0, 60, 1024 * 3 + 17)]
    offs = np.cumsum([0] + [len(s) for s in strings])
    assert offs[1024] % 16 == 13 and offs[1024] > 3 * 4096  # with five bytes in front, the second boundary is off a chunk edge too
    assert (offs[2048] + 5) % 16 == 5
    check_length(strings)
    check_length(strings, lead=5)
    # a row whose bytes straddle two workgroups' spans cannot exist (spans follow rows); the rows either
    # side of the boundary share a chunk instead, and a long row crosses the tile boundary inside one span
    strings[1023] = "€".encode() * 700
    strings[1024] = b"\xf0\x9f\x98\x80" * 600
    check_length(strings)
    # a view starting at row 3 of a larger column, and one starting in the second workgroup's rows
    check_length(strings, first_row=3)
    check_length(strings, first_row=1500)


def test_length_one_long_string_among_one_byte_strings():
    strings = [b"a"] * 2100
    strings[700] = ("x" * 1234 + "é" * 1883).encode("utf-8")
    assert len(strings[700]) == 5000
    check_length(strings)
    strings[700] = b"\x80" * 5000  # 5,000 continuation bytes: length 0
    check_length(strings)


def test_length_nullable_and_in_a_larger_program():
    rng = np.random.default_rng(42)
    rows = 2500
    strings = [None if rng.random() < 0.25 else ("ü" * int(n) + "k").encode("utf-8") for n in rng.integers(0, 30, rows)]
    for vbit_off in (0, 1, 7):
        check_length(strings, nullable=True, vbit_off=vbit_off)
    check_length(strings, first_row=3, nullable=True, vbit_off=5)
    # length feeding an operator, beside a number column; the String's validity passes through
    n = [int(x) for x in rng.integers(-1000, 1000, rows)]
    got = run([X.length(X.col(0)) * 2 + X.col(1), X.length(X.col(0))], [str_col(strings, nullable=True), dev_col(col.Int32, n)], rows)
    want = [None if s is None else D.length(s) for s in strings]
    assert got[0][0] == col.Int64.wrap_nullable() and got[1][0] == col.UInt64.wrap_nullable()
    assert got[1][1] == want and got[0][1] == [None if w is None else 2 * w + x for w, x in zip(want, n)]


# ---- end to end: the queries' shapes ----------------------------------------------------------------------
def group_by(key_cols, key_types, aggs, rows, filt=None):
    """aggs: [(name, DeviceColumn or None)].  Returns assert_exact's `got`."""
    from databend_amd.aggregates import AggregateFunctionFactory
    from databend_amd.aggregator import AggregateHashTable, AggregatorParams, HashTableConfig
    F = AggregateFunctionFactory.instance()
    fns = [F.get(name, [], [] if a is None else [a.dtype]) for name, a in aggs]
    ht = AggregateHashTable(AggregatorParams(list(key_types), fns), HashTableConfig())
    try:
        ht.add_groups(key_cols, [a for _, a in aggs], rows=rows, on_device=True, filter_program=filt)
        block = ht.merge_result()
    finally:
        ht.close()
    return AC.plain_result(block.columns[len(aggs):], block.columns[:len(aggs)])


def device_of(t, values):
    from databend_amd.device import DeviceColumn
    c, keep = dev_col(t, values)
    return DeviceColumn(t, keep[0][: len(values) * t.width], None, keep[1] if t.nullable else None, len(values))


def device_strings(strings):
    from databend_amd.device import DeviceColumn
    torch = _torch()
    offs = np.cumsum([0] + [len(s) for s in strings]).astype(np.int64)
    data = torch.from_numpy(np.frombuffer(b"".join(strings) + b"\0", dtype=np.uint8).copy()).cuda()
    return DeviceColumn(col.String, data, torch.from_numpy(offs).cuda(), None, len(strings))


def test_q19_shape_group_by_user_minute_phrase():
    """ClickBench Q19: GROUP BY UserID, extract(minute FROM EventTime), SearchPhrase; COUNT(*)."""
    rng = np.random.default_rng(51)
    rows = 6001
    users = [int(x) for x in rng.integers(0, 5, rows)]
    times = [1372636800000000 + int(x) * 1000003 for x in rng.integers(0, 3 * 3600, rows)]
    phrases = [[b"", b"gpu", "запрос".encode()][int(i)] for i in rng.integers(0, 3, rows)]
    u, t, p = device_of(col.UInt64, users), device_of(col.Timestamp, times), device_strings(phrases)
    (minute,) = X.ExprProgram([X.extract("minute", X.col(0))], [t]).eval(rows)
    assert minute.dtype == col.UInt8
    got = group_by([u, minute, p], [col.UInt64, col.UInt8, col.String], [("count", None)], rows)
    keys = [(a, D.evaluate("to_minute", col.Timestamp, b), c) for a, b, c in zip(users, times, phrases)]
    ek, ec = AR.aggregate([col.UInt64, col.UInt8, col.String], keys, [("count", None, None)])
    assert 300 < len(ek) < rows
    AR.assert_exact(got, ([col.UInt64, col.UInt8, col.String], ek, ec))


def test_q43_shape_group_by_start_of_minute():
    """ClickBench Q43: GROUP BY DATE_TRUNC('minute', EventTime), COUNT(*), rows within one hour."""
    rng = np.random.default_rng(52)
    rows = 5003
    times = [1372640400000000 + int(x) for x in rng.integers(0, 3600 * 10 ** 6, rows)]
    t = device_of(col.Timestamp, times)
    (key,) = X.ExprProgram([X.date_trunc("minute", X.col(0))], [t]).eval(rows)
    assert key.dtype == col.Timestamp
    got = group_by([key], [col.Timestamp], [("count", None)], rows)
    ek, ec = AR.aggregate([col.Timestamp], [(D.evaluate("to_start_of_minute", col.Timestamp, x),) for x in times], [("count", None, None)])
    assert len(ek) == 60
    AR.assert_exact(got, ([col.Timestamp], ek, ec))


def test_q28_shape_avg_of_length_per_counter():
    """ClickBench Q28: AVG(length(URL)) per CounterID (SQL's avg)."""
    rng = np.random.default_rng(53)
    rows = 5003
    counters = [int(x) for x in rng.integers(0, 41, rows)]
    urls = [("http://пример.example/" + "ы" * int(n) + "?q=" + "x" * int(m)).encode("utf-8")
            for n, m in zip(rng.integers(0, 40, rows), rng.integers(0, 90, rows))]
    c, s = device_of(col.Int32, counters), device_strings(urls)
    (ln,) = X.ExprProgram([X.length(X.col(0))], [s]).eval(rows)
    assert ln.dtype == col.UInt64
    got = group_by([c], [col.Int32], [("sql_avg", ln), ("count", None)], rows)
    ek, ec = AR.aggregate([col.Int32], [(x,) for x in counters], [("sql_avg", col.UInt64, [D.length(u) for u in urls]), ("count", None, None)])
    AR.assert_exact(got, ([col.Int32], ek, ec))


def test_group_by_year_of_date_with_sum_behind_a_filter():
    """TPC-H Q7 / Q8 / Q9's GROUP BY extract(year FROM date) with a SUM, once plain and once with a
    filter in front whose rejected rows hold out-of-range dates."""
    rng = np.random.default_rng(54)
    rows = 7001
    dates = [int(x) for x in rng.integers(D.days_from_civil(1992, 1, 1), D.days_from_civil(1998, 12, 31), rows)]
    vol = [int(x) for x in rng.integers(-10 ** 6, 10 ** 6, rows)]
    d, v = device_of(col.Date, dates), device_of(col.Int64, vol)
    (year,) = X.ExprProgram([X.extract("year", X.col(0))], [d]).eval(rows)
    got = group_by([year], [col.UInt16], [("sum", v), ("count", None)], rows)
    ek, ec = AR.aggregate([col.UInt16], [(D.Civil(x).year,) for x in dates], [("sum", col.Int64, vol), ("count", None, None)])
    assert len(ek) == 7
    AR.assert_exact(got, ([col.UInt16], ek, ec))
    # the filter: flag = 1 keeps a row; the others hold garbage dates
    flags = [int(x) for x in rng.integers(0, 2, rows)]
    dirty = [x if f else GARBAGE[abi.DATE][i % 3] for i, (x, f) in enumerate(zip(dates, flags))]
    dd, ff = device_of(col.Date, dirty), device_of(col.Int8, flags)
    fp = FilterProgram(cmp(0, "=", 1), [ff])
    (year,) = X.ExprProgram([X.to_year(X.col(0))], [dd]).eval(rows, filter_program=fp)
    got = group_by([year], [col.UInt16], [("sum", v), ("count", None)], rows, filt=fp)
    kept = [i for i, f in enumerate(flags) if f]
    ek, ec = AR.aggregate([col.UInt16], [(D.Civil(dates[i]).year,) for i in kept],
                          [("sum", col.Int64, [vol[i] for i in kept]), ("count", None, None)])
    AR.assert_exact(got, ([col.UInt16], ek, ec))
