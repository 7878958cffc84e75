"""The ORDER BY ... LIMIT case table (tests/sort_cases.py) on the CPU: the reference by definition
(tests/sort_ref.py) against hand-written orders and against the oracle, the key model of the path
predictor against the reference, every case's claim about the path it reaches, the union of the
paths reached, and the argument checks of the two entry points that return before any launch.
The device run over the same table is tests/test_gpu_sort_paths.py."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

from databend_amd import abi
from databend_amd import column as col
from databend_amd.column import Column
from databend_amd.ffi import lib
from oracle import oracle
from tests import sort_cases as sc
from tests import sort_ref

NAMES = [c.name for c in sc.cases()]
BIG = "index-byte3"  # 2^24 + 300 rows: closed form, no comparator sort


@functools.lru_cache(maxsize=None)
def prediction(name):
    return sc.predict(sc.case(name))


# ---------------------------------------------------------------- the reference itself
def test_total_order_classes_f32():
    S = 1 << 31
    F = sc.F32
    ascending = [S | F["nan_ones"], S | F["nan_quiet"], S | F["nan_1"], S | F["inf"], S | F["big"], 0xBF800000, S | F["den_max"],
                 S | F["den_min"], S, 0, F["den_min"], F["den_max"], 0x3F800000, F["big"], F["inf"], F["nan_1"], F["nan_quiet"],
                 F["nan_ones"]]
    keys = [sort_ref.float_class(struct.pack("<I", b), abi.FLOAT32) for b in ascending]
    assert all(a < b for a, b in zip(keys, keys[1:]))
    c = Column(col.Float32, np.array(ascending[::-1], np.uint32).view(np.float32))
    n = len(ascending)
    assert sort_ref.sort_limit([c], [True], [False], None) == list(range(n))[::-1]
    assert sort_ref.sort_limit([c], [False], [False], 3) == [0, 1, 2]


def test_total_order_classes_f64():
    S = 1 << 63
    F = sc.F64
    one = struct.unpack("<Q", struct.pack("<d", 1.0))[0]
    ascending = [S | F["nan_ones"], S | F["nan_quiet"], S | F["nan_1"], S | F["inf"], S | F["big"], S | one, S | F["den_max"],
                 S | F["den_min"], S, 0, F["den_min"], F["den_max"], one, F["big"], F["inf"], F["nan_1"], F["nan_quiet"], F["nan_ones"]]
    keys = [sort_ref.float_class(struct.pack("<Q", b), abi.FLOAT64) for b in ascending]
    assert all(a < b for a, b in zip(keys, keys[1:]))


def test_reference_on_written_out_orders():
    ints = Column.from_numbers(col.Int64, [6, 4, 3, 2, 1, 1, 7])
    strs = Column.from_strings(["b1", "b2", "b3", "b4", "b5", "b6", "b7"])
    assert sort_ref.sort_limit([ints], [True], [False], None) == [4, 5, 3, 2, 1, 0, 6]
    assert sort_ref.sort_limit([ints], [True], [False], 4) == [4, 5, 3, 2]
    assert sort_ref.sort_limit([strs], [False], [False], None) == [6, 5, 4, 3, 2, 1, 0]
    assert sort_ref.sort_limit([ints, strs], [True, False], [False, False], None) == [5, 4, 3, 2, 1, 0, 6]
    # NULLs: placed by nulls_first whatever the direction, equal among themselves, then row order
    n = Column.from_numbers(col.Int32, [3, 9, 1, 9, 2], [True, False, True, False, True])
    assert sort_ref.sort_limit([n], [True], [False], None) == [2, 4, 0, 1, 3]
    assert sort_ref.sort_limit([n], [False], [False], None) == [0, 4, 2, 1, 3]
    assert sort_ref.sort_limit([n], [False], [True], None) == [1, 3, 0, 4, 2]
    assert sort_ref.sort_limit([n], [True], [True], 0) == []
    assert sort_ref.sort_limit([n], [True], [True], 99) == [1, 3, 2, 4, 0]
    # a NULL String before another column: the bytes under the NULLs say nothing
    s = Column.from_strings([b"x" * 20, b"y", b"", b"abc", b"q" * 9], validity=[False, False, True, False, False])
    i = Column.from_numbers(col.Int64, [5, 1, 0, 3, 2])
    assert sort_ref.sort_limit([s, i], [True, True], [False, False], None) == [2, 1, 4, 3, 0]
    # bytes: a prefix sorts first; Boolean False < True; Decimal128 beyond 64 bits
    b = Column.from_strings([b"ab", b"a", b"", b"a\x00", b"b"])
    assert sort_ref.sort_limit([b], [True], [False], None) == [2, 1, 3, 0, 4]
    assert sort_ref.sort_limit([Column.from_bools([True, False, True, False])], [True], [False], None) == [1, 3, 0, 2]
    d = Column.from_decimals(38, 0, [1 << 64, -(1 << 64), 2**127 - 1, -2**127, 0])
    assert sort_ref.sort_limit([d], [True], [False], None) == [3, 1, 4, 0, 2]


# ---------------------------------------------------------------- the table against the oracle
@pytest.mark.parametrize("name", [n for n in NAMES if n != BIG])
def test_reference_equals_oracle(name):
    c = sc.case(name)
    want = sc.reference(c)
    if c.entry == "single":
        got = oracle.sort_limit_indices(c.columns[0], c.asc[0], c.nulls_first[0], c.limit).tolist()
        assert got == want
    got = oracle.sort_multi_limit_indices(c.columns, c.asc, c.nulls_first, c.limit).tolist()
    assert got == want


def test_closed_form_of_the_large_case():
    c = sc.case(BIG)
    v = np.asarray(c.columns[0].data)
    assert len(v) == 2**24 + 300 and c.asc == (True,) and c.columns[0].validity is None
    assert c.expected == np.flatnonzero(v == v.min())[:c.limit].tolist()
    assert sum(1 for x in sc.cases() if len(x.columns[0]) > 70_000) == 1


# ---------------------------------------------------------------- the predictor
@pytest.mark.parametrize("name", [n for n in NAMES if n != BIG])
def test_model_key_orders_rows_like_the_reference(name):
    """The replay's composite key (the kernel's trick, NULL String = one zero group) gives the
    reference's order, so what the replay says about the key's bytes is about the right key."""
    c = sc.case(name)
    n = len(c.columns[0])
    if c.entry == "single":
        valid = sc.valid_mask(c.columns[0])
        ok = sc.order_key(c.columns[0])
        ok = np.where(valid, ok if c.asc[0] else ~ok, np.uint64(0))
        nr = valid == c.nulls_first[0]
        order = np.lexsort([np.arange(n), ok, nr]).tolist()
    else:
        keys, _ = sc.multi_keys(c.columns, c.asc, c.nulls_first)
        order = sorted(range(n), key=lambda i: (keys[i], i))
    assert (order if c.limit is None else order[:c.limit]) == sc.reference(c)


def _order_by_keys(keys, limit):
    W = (max(len(k) for k in keys) + 7) // 8
    order = sorted(range(len(keys)), key=lambda i: (keys[i] + bytes(8 * W - len(keys[i])), i))
    return order if limit is None else order[:limit]


def test_null_string_cases_tell_the_two_encodings_apart():
    """Every NULL-String case comes out wrong under the encoding that sized a NULL's part of the
    key by the bytes beneath it, so a kernel that did so fails each of them."""
    s = Column.from_strings([b"x" * 20, b"y", b"", b"abc", b"q" * 9], validity=[False, False, True, False, False])
    i = Column.from_numbers(col.Int64, [5, 1, 0, 3, 2])
    keys, _ = sc.multi_keys([s, i], [True, True], [False, False], null_string_by_length=True)
    assert _order_by_keys(keys, None) == [2, 0, 4, 1, 3]
    keys, _ = sc.multi_keys([s, i], [True, True], [False, False])
    assert _order_by_keys(keys, None) == [2, 1, 4, 3, 0]
    names = [n for n in NAMES if n.startswith("nullstr-")]
    assert len(names) == 10
    for name in names:
        c = sc.case(name)
        keys, _ = sc.multi_keys(c.columns, c.asc, c.nulls_first, null_string_by_length=True)
        assert _order_by_keys(keys, c.limit) != sc.reference(c), name


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_the_path_it_claims(name):
    c = sc.case(name)
    pred = prediction(name)
    assert c.raises == (pred["path"] == "unsupported")
    assert sc.check_claims(pred, c.claims) == [], pred


def test_every_path_is_reached():
    single = [prediction(c.name) for c in sc.cases() if c.entry == "single"]
    multi = [prediction(c.name) for c in sc.cases() if c.entry == "multi"]
    assert {"empty", "direct", "select", "unsupported"} <= {p["path"] for p in single}
    assert {"direct", "select"} <= {p["path"] for p in multi}
    steps = [p["steps"] for p in single if p["path"] == "select"]
    for level in range(1, 9):
        for kind in ("stop", "skipped", "hist"):
            assert any(s.get(level, ("",))[0] == kind for s in steps), (level, kind)
    assert any(s.get(0, ("",))[0] == "stop" for s in steps)
    for level in (10, 11, 12):
        assert any(level in s and s[level][2] > 1 for s in steps), level
    assert any(9 in s and s[9][1] != 0 for s in steps)
    sel = [p for p in multi if p["path"] == "select"]
    assert any(p["stop"][0] == 0 for p in sel)
    assert any(1 <= p["stop"][0] < p["W"] for p in sel)
    assert any(p["stop"][0] == p["W"] for p in sel)
    assert any(p["W"] >= 16 for p in sel)
    assert any(p["straddle"] for p in sel)
    assert any(len(c.columns) == sc.SORT_MAX_COLS for c in sc.cases())


def test_case_table_shape():
    by = {}
    for c in sc.cases():
        by.setdefault(c.name.split("-limit")[0], []).append(c)
    for n in (1, 2, 2047, 2048):
        assert {c.limit for c in by["cap-n%d" % n]} == {1, n - 1, n, n + 5, None}
    assert {(c.limit, c.raises) for c in by["cap-n2049"]} == {(1, False), (2048, False), (2049, True), (None, True)}
    for L in range(1, 9):
        for t in ("i64", "u64"):
            assert sorted(c.limit for c in by["level%d-%s" % (L, t)]) == [999, 1000, 1001]
    assert sorted(c.limit for c in by["all-equal"]) == [1, 255, 256, 257, 2048]
    for c in sc.cases():
        assert len(c.columns[0]) <= 5000 or len(c.columns[0]) == 70_000 or c.name == BIG, c.name
        assert all(len(x) == len(c.columns[0]) for x in c.columns)


# ---------------------------------------------------------------- argument checks, before any launch
def _call_single(c, rows, limit=1):
    n, idx = C.c_uint64(), (C.c_uint32 * 8)()
    return lib().dbg_sort_limit_indices(C.byref(c), rows, 1, 0, limit, idx, C.byref(n), None)


def _call_multi(cols, rows, limit=1):
    arr = (abi.dbg_column * max(1, len(cols)))(*cols)
    flags = (C.c_int * max(1, len(cols)))()
    n, idx = C.c_uint64(), (C.c_uint32 * 8)()
    return lib().dbg_sort_limit_multi(arr, len(cols), flags, flags, rows, limit, idx, C.byref(n), None)


def test_single_refuses_a_short_column():
    host = Column.from_numbers(col.Int64, [3, 1, 2])
    assert _call_single(host.to_abi(), 5) == abi.DBG_ERR_INVALID
    assert b"shorter" in lib().dbg_last_error()
    nullable = Column.from_numbers(col.Int32, [3, 1, 2], [True, False, True])
    assert _call_single(nullable.to_abi(), 4, limit=4) == abi.DBG_ERR_INVALID


def test_multi_argument_checks():
    host = Column.from_numbers(col.Int64, [3, 1, 2])
    a = host.to_abi()
    assert _call_multi([], 3) == abi.DBG_ERR_UNSUPPORTED
    assert _call_multi([a] * 9, 3) == abi.DBG_ERR_UNSUPPORTED
    assert _call_multi([a], 5) == abi.DBG_ERR_INVALID
    assert _call_multi([a, a], 4) == abi.DBG_ERR_INVALID
    strs = Column.from_strings(["a", "b", "c"])
    s = strs.to_abi()
    s.offsets = None
    assert _call_multi([a, s], 3) == abi.DBG_ERR_INVALID
    assert b"offsets" in lib().dbg_last_error()
    wide = Column.from_decimals(50, 2, [3, 1, 2])
    assert _call_multi([a, wide.to_abi()], 3) == abi.DBG_ERR_UNSUPPORTED
    assert b"Decimal256" in lib().dbg_last_error()
