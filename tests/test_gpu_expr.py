"""The device projection (dbg_expr_eval, databend_amd/csrc/expr.hip) on the GPU: plus / minus /
multiply over numbers and Decimal128, both kernel instantiations (narrow: 8 rows per lane; wide: a
Decimal128 somewhere, one row per lane).

Expected values, validity and errors come from tests/expr_ref.py (plain Python integers).  Every
comparison is exact and validity bits are exact; the data of NULL rows and of rows the filter drops
are not compared.  Outputs are written into buffers with guard bytes on both sides, which must
stay untouched."""
import numpy as np
import pytest

from databend_amd import abi
from databend_amd import column as col
from databend_amd import expr as X
from databend_amd.column import DataType
from databend_amd.ffi import DecimalOverflow, check, lib
from databend_amd.filter import FilterProgram, cmp
from tests import expr_ref as R

pytestmark = pytest.mark.gpu
GUARD = 64
ROW_COUNTS = [0, 1, 7, 8, 9, 63, 64, 65, 2047, 2048, 2049, 2 * 2048 * 4 + 5]
# (element offset, validity bit offset) of the input views, and whether the outputs start one element
# (a Decimal128: 8 bytes) past a 16-byte boundary, which takes the stores that are not 16 bytes wide
VIEWS = [(0, 0, False), (1, 1, True), (3, 7, True)]


def _torch():
    import torch
    return torch


def host_bytes(t: DataType, values) -> np.ndarray:
    if t.type_id == abi.DECIMAL128:
        return col.i128_to_bytes(values)
    if t.type_id in R.FLOATS:
        return np.asarray(values, dtype=t.np_dtype).view(np.uint8)
    return np.array([R.wrap_int(int(v), t.type_id) for v in values], dtype=t.np_dtype).view(np.uint8)


def dev_col(t: DataType, values, elem_off=0, vbit_off=0, null_fill=0):
    """A device view of `values` (None = NULL, stored as null_fill) that starts elem_off elements into
    its buffer and vbit_off bits into its bitmap.  Returns (dbg_column, what keeps it alive)."""
    torch = _torch()
    n, w = len(values), t.width
    data = host_bytes(t, [null_fill if v is None else v for v in values])
    buf = np.concatenate([np.full(elem_off * w, 0xEE, np.uint8), data, np.full(1, 0xEE, np.uint8)])
    d = torch.from_numpy(buf).cuda()
    c = abi.dbg_column()
    c.dt = t.to_abi()
    c.data = d.data_ptr() + elem_off * w
    c.len = n
    keep = [d]
    if t.nullable:
        bits = np.concatenate([np.ones(vbit_off, bool), np.array([v is not None for v in values], bool)])
        v = torch.from_numpy(np.concatenate([np.packbits(bits, bitorder="little"), np.zeros(1, np.uint8)])).cuda()
        c.validity = v.data_ptr()
        c.validity_offset = vbit_off
        keep.append(v)
    return c, keep


def decode(t: DataType, raw: np.ndarray, n: int):
    if t.type_id == abi.DECIMAL128:
        return col.i128_from_bytes(raw[: n * 16])
    a = raw[: n * t.width].view(t.np_dtype)
    return [float(x) for x in a] if t.type_id in R.FLOATS else [int(x) for x in a]


def run(exprs, cols, rows, filt=None, odd_outputs=False):
    """exprs: tuple-form expressions; cols: [(dbg_column, keep)].  Returns [(type, values)] with None
    for NULL rows.  Raises what dbg_expr_eval fails with.  odd_outputs: every output buffer starts
    one element (8 bytes for a Decimal128) past a 16-byte boundary."""
    torch = _torch()
    prog = X.ExprProgram([R.to_lib_expr(e) for e in exprs], [c for c, _ in cols])
    types = prog.result_types()
    arr = (abi.dbg_out_column * len(types))()
    bufs = []
    for k, t in enumerate(types):
        lead = GUARD + (min(t.width, 8) if odd_outputs else 0)  # torch buffers and GUARD are multiples of 16
        d = torch.full((lead + rows * t.width + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        assert d.data_ptr() % 16 == 0
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
        vals = decode(t, raw[lead:].copy(), rows)
        if v is not None:
            vr = v.cpu().numpy()
            nb = (rows + 7) // 8
            assert (vr[:GUARD] == 0xA5).all() and (vr[GUARD + nb:] == 0xA5).all(), "validity guard bytes were written"
            bits = np.unpackbits(vr[GUARD:GUARD + nb], bitorder="little")
            assert not bits[rows:].any(), "validity bits past the last row are set"
            vals = [x if b else None for x, b in zip(vals, bits[:rows])]
        out.append((t, vals))
    return out


def assert_same(got, want_t, want, what=""):
    t, vals = got
    assert t == want_t, (what, t, want_t)
    assert len(vals) == len(want)
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(vals, want)) if w != "unselected" and not R.same_value(t, g, w)]
    assert not bad, (what, bad[:5], len(bad))


def check_program(exprs, types, values, rows, views=((0, 0, False),), filt_rows=None):
    """Run the expressions over `values` at every view and compare with the reference."""
    want = [R.evaluate(e, types, values, filt_rows) for e in exprs]
    assert all(w[2] is None for w in want)
    for eo, vo, odd in views:
        cols = [dev_col(t, v, eo, vo if t.nullable else 0) for t, v in zip(types, values)]
        got = run(exprs, cols, rows, odd_outputs=odd)
        for k, (g, (wt, wv, _)) in enumerate(zip(got, want)):
            assert_same(g, wt, wv, (k, rows, eo, vo, odd))


def cycle(vals, n, seed):
    rng = np.random.default_rng(seed)
    idx = np.concatenate([np.arange(len(vals)), rng.integers(0, len(vals), max(0, n - len(vals)))])[:n]
    return [vals[int(i)] for i in idx]


def with_nulls(vals, seed, frac=0.2):
    rng = np.random.default_rng(seed)
    return [None if rng.random() < frac else v for v in vals]


# ---- row counts and views: the lane, wave, strip and tile edges of both instantiations ----------------
@pytest.mark.parametrize("rows", ROW_COUNTS)
def test_row_counts_narrow(rows):
    ta, tb, tc = col.Int16.wrap_nullable(), col.UInt32, col.Float64.wrap_nullable()
    a = with_nulls(cycle(R.extremes(ta), rows, 1), 2)
    b = cycle(R.extremes(tb), rows, 3)
    c = with_nulls(cycle([0.5, -1.25, 3.0, 1e300, -7.0], rows, 4), 5)
    three = ("lit", 3, DataType(abi.UINT8))
    exprs = [("+", ("col", 0), ("col", 1)), ("*", ("col", 0), three), ("-", ("col", 2), ("col", 1)), ("col", 0)]
    check_program(exprs, [ta, tb, tc], [a, b, c], rows, VIEWS)


@pytest.mark.parametrize("rows", ROW_COUNTS)
def test_row_counts_wide(rows):
    D = R.Dec(15, 2)
    ta, tb, tc = D.wrap_nullable(), D, col.Int32.wrap_nullable()
    a = with_nulls(cycle(R.extremes(D), rows, 6), 7)
    b = cycle(R.extremes(D), rows, 8)
    c = with_nulls(cycle(R.extremes(tc), rows, 9), 10)
    exprs = [("*", ("col", 0), ("col", 1)), ("+", ("col", 0), ("col", 2)), ("-", ("col", 2), ("lit", 7, DataType(abi.INT8)))]
    check_program(exprs, [ta, tb, tc], [a, b, c], rows, VIEWS)


# ---- numbers: every type pair x every operator --------------------------------------------------------
@pytest.mark.parametrize("op", "+-*")
def test_number_pairs(op):
    rows = 257
    for i, ta in enumerate(R.NUMBER_TYPES):
        for j, tb in enumerate(R.NUMBER_TYPES):
            a = cycle(R.extremes(ta), rows, 100 + i)
            b = cycle(list(reversed(R.extremes(tb))), rows, 200 + j)
            # the extremes against each other: 64-bit wrap included
            a[:3], b[:3] = [R.extremes(ta)[0], R.extremes(ta)[1], R.extremes(ta)[0]], [R.extremes(tb)[0], R.extremes(tb)[1], R.extremes(tb)[1]]
            check_program([(op, ("col", 0), ("col", 1))], [ta, tb], [a, b], rows)


def test_int64_wraps():
    I, U = col.Int64, col.UInt64
    hi, lo, um = (1 << 63) - 1, -(1 << 63), (1 << 64) - 1
    got = run([("+", ("col", 0), ("col", 1)), ("-", ("col", 0), ("col", 1)), ("*", ("col", 0), ("col", 1)), ("-", ("col", 2), ("col", 3)),
               ("*", ("col", 2), ("col", 3))],
              [dev_col(I, [hi, lo, hi]), dev_col(I, [1, 1, hi]), dev_col(U, [0, um, um]), dev_col(U, [1, 0, um])], 3)
    assert got[0] == (I, [lo, lo + 1, -2]) and got[1] == (I, [hi - 1, hi, 0]) and got[2] == (I, [hi, lo, 1])
    assert got[3] == (I, [-1, -1, 0]) and got[4] == (U, [0, 0, 1])


def test_float_multiply_add_is_not_fused():
    """a * b + c where the product rounds: (1 + 2^-30)(1 - 2^-30) = 1 - 2^-60 rounds to 1.0, so two
    roundings give 0.0 where a fused multiply-add gives -2^-60."""
    F = col.Float64
    a, b, c = [1.0 + 2.0 ** -30, 3.0, 1.0 + 2.0 ** -52], [1.0 - 2.0 ** -30, 1.0 / 3.0, 1.0 + 2.0 ** -52], [-1.0, -1.0, -1.0]
    e = ("+", ("*", ("col", 0), ("col", 1)), ("col", 2))
    _, want, _ = R.evaluate(e, [F, F, F], [a, b, c])
    assert want[0] == 0.0 and want[2] == 2.0 ** -51  # the fused results would be -2^-60 and 2^-51 + 2^-104
    rows = 2048 + 3
    vals = [cycle(v, rows, 1) for v in (a, b, c)]  # the same draw for all three: the triples stay together
    got = run([e], [dev_col(F, v) for v in vals], rows)[0]
    assert_same(got, F, R.evaluate(e, [F, F, F], vals)[1])
    assert got[1][:3] == [0.0, want[1], 2.0 ** -51]


# ---- number operators whose results feed decimal operators ------------------------------------------------
@pytest.mark.parametrize("k", range(len(R.mixed_programs(1))))
def test_integer_results_feed_decimal_operators(k):
    """(Int32 - UInt8) * Decimal, (Int64 + Int64) + Decimal, (UInt64 - UInt64) - Decimal and the like:
    the integer intermediate — negative, wrapped at 64 bits, unsigned with the top bit set, or NULL —
    must reach the decimal operator extended to 128 bits by its own result type, as either operand."""
    rows = 2049 + 70
    e, types, values = R.mixed_programs(rows)[k]
    _, want, _ = R.evaluate(e, types, values)
    assert any(w is not None and w < 0 for w in want)
    check_program([e], types, values, rows, VIEWS)
    inner = e[1] if e[1][0] in "+-*" else e[2]
    check_program([e, inner], types, [v[:9] for v in values], 9)  # the intermediate as an output of its own, stored on the way


# ---- decimals: the reference's case grid, grouped into columns ----------------------------------------
def grouped_decimal_cases(op):
    groups = {}
    for c in R.decimal_cases():
        if c[0] == op:
            groups.setdefault((c[1], c[2]), []).append(c)
    return groups


@pytest.mark.parametrize("op", "+-*")
def test_decimal_case_grid(op):
    """Every (type pair, operator) group of expr_ref.decimal_cases() as one two-column call.  A group
    with failing rows must fail with DBG_ERR_OVERFLOW naming the operation; with those rows made
    NULL (the same bytes underneath) it must pass and every other row must be exact."""
    n_err = n_ok = 0
    for (ta, tb), cases in grouped_decimal_cases(op).items():
        exp = [R.expected(c) for c in cases]
        rt = exp[0][0]
        xs, ys = [c[3] for c in cases], [c[4] for c in cases]
        e = (op, ("col", 0), ("col", 1))
        if any(x[2] for x in exp):
            with pytest.raises(DecimalOverflow) as err:
                run([e], [dev_col(ta, xs), dev_col(tb, ys)], len(cases))
            assert R.OP_NAME[op] in str(err.value), str(err.value)
            n_err += 1
        # the failing rows as NULLs: same data bytes, validity bit clear
        tn = ta.wrap_nullable()
        xn = [None if x[2] else v for v, x in zip(xs, exp)]
        fills = [v for v, x in zip(xs, exp) if x[2]]
        colA, keep = dev_col(tn, xn, 0, 3)
        if fills:  # put the overflowing operands back under the NULL rows
            raw = host_bytes(ta, xs)
            keep[0][: len(raw)].copy_(_torch().from_numpy(raw))
        got = run([e], [(colA, keep), dev_col(tb, ys)], len(cases))[0]
        assert_same(got, rt.wrap_nullable(), [None if x[2] else x[1] for x in exp], (op, ta, tb))
        n_ok += 1
    assert n_err > 20 and n_ok > 300


def test_decimal_multiply_divisors_and_rounding():
    """Divisor exponents 0, 8 and 30 (the last in two divisions), products exactly at +-half the
    divisor, a result beyond 10^38 that fits i128, and one beyond i128."""
    for (p, s), k in (((15, 2), 0), ((20, 10), 8), ((38, 30), 30)):
        D = R.Dec(p, s)
        rt = R.result_type("*", D, D)
        assert 2 * s - rt.scale == k
        h = 10 ** k // 2
        xs = [h, -h, h, -h, h - 1, 1 - h, h + 1, 3 * h, -3 * h, 10 ** (p - 1), -(10 ** (p - 1)), 7, 0, 0] if k else [3, -3, 10 ** 14, -7, 0]
        ys = [1, 1, -1, -1, 1, 1, 1, 1, 1, 10 ** 18 + 3, 10 ** 18 + 3, -9, -5, 5][: len(xs)] if k else [5, 5, -(10 ** 14), 0, -1]
        rows = 2049
        a, b = cycle(xs, rows, 1), cycle(ys, rows, 1)
        check_program([("*", ("col", 0), ("col", 1))], [D, D], [a, b], rows, [(0, 0, False), (1, 0, True)])
    D = R.Dec(38, 0)
    got = run([("*", ("col", 0), ("col", 1))], [dev_col(D, [10 ** 19, -(1 << 64)]), dev_col(D, [10 ** 19 + 7, 1 << 63])], 2)[0]
    assert got == (D, [10 ** 38 + 7 * 10 ** 19, -(1 << 127)])  # beyond the precision, inside i128: no error
    with pytest.raises(DecimalOverflow) as e:
        run([("*", ("col", 0), ("col", 1))], [dev_col(D, [1, 1 << 64]), dev_col(D, [1, 1 << 63])], 2)
    assert "multiply" in str(e.value)


def test_decimal_plus_minus_checks():
    D0, D10, small = R.Dec(38, 0), R.Dec(38, 10), R.Dec(10, 0)
    m = 10 ** 38 - 1
    # precision 38: the sum is range-checked
    for op, x, y in (("+", m, 1), ("-", -m, 1), ("+", m, m), ("-", m, -m)):
        with pytest.raises(DecimalOverflow) as e:
            run([(op, ("col", 0), ("col", 1))], [dev_col(D0, [0, x]), dev_col(D0, [0, y])], 2)
        assert R.OP_NAME[op] in str(e.value)
    assert run([("+", ("col", 0), ("col", 1))], [dev_col(D0, [m - 1, -m]), dev_col(D0, [1, 0])], 2)[0] == (D0, [m, -m])
    # the scale-up cast: 10^28 * 10^10 leaves precision 38
    with pytest.raises(DecimalOverflow):
        run([("+", ("col", 0), ("col", 1))], [dev_col(D0, [10 ** 28]), dev_col(D10, [0])], 1)
    assert run([("-", ("col", 0), ("col", 1))], [dev_col(D0, [10 ** 28 - 1]), dev_col(D10, [5])], 1)[0] == \
        (D10, [(10 ** 28 - 1) * 10 ** 10 - 5])
    # below 38 nothing is checked: values beyond the declared precision pass
    assert run([("+", ("col", 0), ("col", 1))], [dev_col(small, [10 ** 30]), dev_col(small, [1])], 1)[0] == (R.Dec(11, 0), [10 ** 30 + 1])


def test_errors_are_masked_by_null_and_by_the_filter():
    D = R.Dec(38, 0)
    m = 10 ** 38 - 1
    rows = 2049 + 64
    bad = [7, 300, 2048, rows - 1]  # rows whose operands overflow, in both kernels' edge positions
    x = [m if i in bad else i for i in range(rows)]
    y = [1] * rows
    key = [0 if i in bad else 1 for i in range(rows)]
    e = ("+", ("col", 0), ("col", 1))
    mul = ("*", ("col", 0), ("col", 0))  # m * m leaves i128
    with pytest.raises(DecimalOverflow):
        run([e], [dev_col(D, x), dev_col(D, y)], rows)
    with pytest.raises(DecimalOverflow):
        run([mul], [dev_col(D, x)], rows)
    # NULL rows (the overflowing bytes still under them)
    xn = [None if i in bad else v for i, v in enumerate(x)]
    got = run([e, mul], [dev_col(D.wrap_nullable(), xn, 1, 5, null_fill=m), dev_col(D, y)], rows)
    assert_same(got[0], D.wrap_nullable(), [None if i in bad else i + 1 for i in range(rows)])
    assert_same(got[1], D.wrap_nullable(), [None if i in bad else i * i for i in range(rows)])
    # rows the filter drops
    kc, kk = dev_col(col.Int8, key)
    fp = FilterProgram(cmp(0, "=", 1), [kc])
    got = run([e, mul], [dev_col(D, x), dev_col(D, y)], rows, fp)
    assert_same(got[0], D, ["unselected" if i in bad else i + 1 for i in range(rows)])
    assert_same(got[1], D, ["unselected" if i in bad else i * i for i in range(rows)])
    # ... and the filter does not hide an error on a row it keeps
    fp2 = FilterProgram(cmp(0, "=", 0), [kc])
    with pytest.raises(DecimalOverflow):
        run([e], [dev_col(D, x), dev_col(D, y)], rows, fp2)
    del kk


# ---- the queries -----------------------------------------------------------------------------------------
def q1_program(cols):
    price, disc, tax = X.col(0), X.col(1), X.col(2)
    disc_price = price * (1 - disc)
    return X.ExprProgram([disc_price, disc_price * (1 + tax)], [cols["l_extendedprice"], cols["l_discount"], cols["l_tax"]])


def test_q1_projection_equals_the_generators_columns():
    from databend_amd import workloads
    rows = 4099
    cols = workloads.generate_device(1, rows)
    prog = q1_program(cols)
    assert [n.op for n in prog.nodes].count(abi.EXPR_STORE) == 2 and [n.op for n in prog.nodes].count(abi.EXPR_MULTIPLY) == 2
    assert prog.result_types() == [cols["disc_price"].dtype, cols["charge"].dtype]
    disc_price, charge = prog.eval(rows)
    for got, name in ((disc_price, "disc_price"), (charge, "charge")):
        assert got.dtype == cols[name].dtype and got.length == rows
        assert bytes(got.data.cpu().numpy()[: rows * 16]) == bytes(cols[name].data.cpu().numpy()[: rows * 16]), name


def test_q1_end_to_end_with_projected_columns():
    from databend_amd import workloads
    from databend_amd.aggregator import AggregateHashTable
    rows = 4099
    cols = workloads.generate_device(1, rows)
    shape = workloads.SHAPES[1]
    projected = dict(cols)
    projected["disc_price"], projected["charge"] = q1_program(cols).eval(rows)
    blocks = []
    for src in (projected, cols):
        ht = AggregateHashTable(workloads.params_for(1, {k: v.dtype for k, v in src.items()}))
        try:
            c, op, k = shape.predicate
            fp = FilterProgram(cmp(0, op, k), [src[c]])
            ht.add_groups([src[k] for k in shape.keys], [src[a] if a else None for _, a in shape.aggs], rows=rows, filter_program=fp,
                          on_device=True)
            blocks.append(ht.merge_result())
        finally:
            ht.close()
    a, b = blocks
    assert a.num_rows() == b.num_rows() >= 3 and a.num_columns() == b.num_columns() == len(shape.aggs) + len(shape.keys)
    rows_a = sorted(zip(*[c.values() for c in a.columns]), key=lambda r: r[-2:])
    rows_b = sorted(zip(*[c.values() for c in b.columns]), key=lambda r: r[-2:])
    assert rows_a == rows_b
    assert [c.dtype for c in a.columns] == [c.dtype for c in b.columns]


def test_q30_keyless_sums_of_column_plus_constant():
    """ClickBench Q30's shape: SUM(ResolutionWidth + k), k = 0..3, without GROUP BY."""
    from databend_amd import workloads
    from databend_amd.aggregator import AggregateHashTable, AggregatorParams, HashTableConfig
    from databend_amd.aggregates import AggregateFunctionFactory
    F = AggregateFunctionFactory.instance()
    rows = 10_007
    cols = workloads.generate_device(4, rows)
    w = cols["ResolutionWidth"]
    prog = X.ExprProgram([X.col(0) + k for k in range(4)], [w])
    assert prog.result_types() == [col.Int32] * 4  # Int16 + UInt8
    outs = prog.eval(rows)
    ht = AggregateHashTable(AggregatorParams([], [F.get("sum", [], [col.Int32]) for _ in range(4)]), HashTableConfig())
    try:
        ht.add_groups([], outs, rows=rows, on_device=True)
        block = ht.merge_result()
    finally:
        ht.close()
    host = w.data.cpu().numpy()[: rows * 2].view(np.int16).astype(np.int64)
    assert [c.values()[0] for c in block.columns] == [int(host.sum()) + k * rows for k in range(4)]
    for k, o in enumerate(outs):
        assert (o.data.cpu().numpy()[: rows * 4].view(np.int32) == (host + k).astype(np.int32)).all()


def test_q36_group_by_column_minus_constant():
    """ClickBench Q36's shape: GROUP BY ClientIP - 1 (Int32 - UInt8 -> Int64), COUNT(*)."""
    from databend_amd import workloads
    from databend_amd.aggregator import AggregateHashTable, AggregatorParams, HashTableConfig
    from databend_amd.aggregates import AggregateFunctionFactory
    F = AggregateFunctionFactory.instance()
    rows = 10_007
    cols = workloads.generate_device(4, rows)
    ip = cols["ClientIP"]
    # fewer distinct keys than rows, so that groups hold several rows
    torch = _torch()
    folded = (ip.data[: rows * 4].view(torch.int32) % 257).contiguous().view(torch.uint8)
    from databend_amd.device import DeviceColumn
    ipc = DeviceColumn(col.Int32, folded, None, None, rows)
    prog = X.ExprProgram([X.col(0) - 1], [ipc])
    assert prog.result_types() == [col.Int64]
    (key,) = prog.eval(rows)
    ht = AggregateHashTable(AggregatorParams([col.Int64], [F.get("count", [], [])]), HashTableConfig())
    try:
        ht.add_groups([key], [None], rows=rows, on_device=True)
        block = ht.merge_result()
    finally:
        ht.close()
    host = folded.cpu().numpy().view(np.int32).astype(np.int64) - 1
    uniq, counts = np.unique(host, return_counts=True)
    got = dict(zip(block.columns[1].values(), block.columns[0].values()))
    assert got == dict(zip((int(u) for u in uniq), (int(c) for c in counts)))
