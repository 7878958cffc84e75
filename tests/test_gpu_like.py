"""LIKE predicates on the device (DBG_PRED_LIKE): the standalone select, three-valued logic, the two
mask kernels at their boundaries, LIKE fused into GROUP BY on every insert family, masks per batch,
and the refusals.  Expected values come from tests/like_ref.py (plain Python bytes, written from the
reference's rules) composed with tests/pred_ref.py; the expected GROUP BY results from the Python
group references under that mask.  All comparisons are exact.

The mask of `%needle%` comes from like_scan_kernel or like_rows_kernel; dbg_like_force_kernel forces
one, and dbg_like_kernel_counts shows which ran."""
import ctypes as C
from contextlib import contextmanager

import numpy as np
import pytest

from databend_amd import abi
from databend_amd import column as col
from databend_amd.aggregates import AggregateFunctionFactory
from databend_amd.aggregator import AggregateHashTable, AggregatorParams, HashTableConfig
from databend_amd.column import Column
from databend_amd.ffi import DbgError, Unsupported, check, lib
from databend_amd.filter import FilterProgram, and_, cmp, is_null, like, not_, not_like, or_
from tests import like_ref, pred_ref
from tests.test_gpu_parity import gpu_aggregate
from tests.test_gpu_predicates import DevCol, Table, gpu_select
from tests.test_gpu_string_minmax import as_dict, reference

pytestmark = pytest.mark.gpu

FN = AggregateFunctionFactory.instance()
TRUE = pred_ref.TRUE
TILE = 16384  # like_scan_kernel's tile


def kernel_counts() -> dict:
    c = (C.c_uint64 * 3)()
    check(lib().dbg_like_kernel_counts(c, 3))
    return dict(fill=int(c[0]), rows=int(c[1]), scan=int(c[2]))


@contextmanager
def forced(kernel):
    """kernel: 'rows', 'scan' or None (the library's own dispatch)."""
    check(lib().dbg_like_force_kernel({None: 0, "rows": 1, "scan": 2}[kernel]))
    try:
        yield
    finally:
        check(lib().dbg_like_force_kernel(0))


class RawStr:
    """A String column in HBM whose blob starts `skew` bytes into a buffer (an unaligned data
    pointer) and whose offsets start at `first` (offsets[0] != 0); the bytes around the blob repeat
    `around`, so a read outside [offsets[0], offsets[rows]) would find matches that are not there."""

    def __init__(self, c: Column, skew=0, first=0, around=b"", voff=0):
        import torch
        blob = np.asarray(c.data, np.uint8)
        pad = np.frombuffer((around * (64 // max(1, len(around)) + 1))[:64] if around else bytes(64), np.uint8)
        lead = np.concatenate([pad, pad])[:skew + first] if skew + first else np.zeros(0, np.uint8)
        buf = np.concatenate([lead, blob, pad])
        self.buf = torch.from_numpy(buf.copy()).cuda()
        self.offsets = torch.from_numpy((c.offsets.astype(np.uint64) + np.uint64(first)).view(np.int64).copy()).cuda()
        self.validity = None
        if c.validity is not None and c.dtype.nullable:
            bits = np.concatenate([np.ones(voff, bool), np.asarray(c.validity, bool)])
            self.validity = torch.from_numpy(np.packbits(bits, bitorder="little")).cuda()
        self.skew, self.voff, self.dtype, self.length = skew, voff, c.dtype, len(c)
        torch.cuda.synchronize()

    def to_abi(self) -> abi.dbg_column:
        d = abi.dbg_column()
        d.dt = self.dtype.to_abi()
        d.data = self.buf.data_ptr() + self.skew
        d.offsets = self.offsets.data_ptr()
        if self.validity is not None:
            d.validity = self.validity.data_ptr()
            d.validity_offset = self.voff
        d.len = self.length
        return d

    def __len__(self):
        return self.length


def check_select(pred, hcols, dcols, n, kernel=None, what=None):
    before = kernel_counts()
    with forced(kernel):
        got = gpu_select(pred, dcols, n)
    exp = like_ref.select(pred, hcols, n)
    assert np.array_equal(got, exp), (what, kernel, got[:8], exp[:8], len(got), len(exp))
    return {k: v - before[k] for k, v in kernel_counts().items()}


# ---- a. select parity, every class -----------------------------------------------------------------
ALPHABET = [b"\x00", b"\x80", b"\xff", b"%", b"_", b"\\", b"a", b"b"]
SPECIAL = [b"", "é".encode(), b"v%xx", b"%", b"a\\b", b"ab", b"a", b"\\", b"a\\", b"_", b"a_b", b"aXb"]
PATTERNS = {
    "ordinal": [b"", b"a", b"ab", b"a\\b", b"\x00", b"\xff\x80"],
    "start_of_percent": [b"%", b"%a", b"%\x00\x80", b"%a\\b", b"%\\"],
    "end_of_percent": [b"a%", b"\xff%", b"a\\b%", b"\x00\x00%"],
    "surround": [b"%%", b"%a%", b"%ab%", b"%\x00%", b"%\xff\x80%", b"%a\\b%", b"%bbb%"],
    "simple": [b"%%%", b"a%b", b"%a%b", b"a%b%", b"%a%b%", b"a%%", b"%%a", b"\x80%\xff%a", b"%a%a%a%"],
    "complex": [b"_", b"__", b"a_", b"_%", b"%_a", b"\\%", b"_\\%%", b"%\\_%", b"\\\\", b"a\\%b", b"%a_b%", b"_\\", b"%\\%%\\\\%"],
}
KIND_OF = dict(ordinal=0, start_of_percent=1, end_of_percent=2, surround=3, simple=4, complex=5)


@pytest.fixture(scope="module")
def mixed():
    """~3000 short strings over ALPHABET (many empty), the quirk strings among them; a nullable twin."""
    rng = np.random.default_rng(11)
    vals = list(SPECIAL)
    while len(vals) < 3000:
        n = int(rng.choice([0, 1, 2, 3, 5, 8, 13]))
        vals.append(b"".join(ALPHABET[i] for i in rng.integers(0, len(ALPHABET), n)))
    order = rng.permutation(len(vals))
    vals = [vals[i] for i in order]
    valid = rng.random(len(vals)) < 0.8
    return Column.from_strings(vals), Column.from_strings(vals, valid)


@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("cls", list(PATTERNS))
def test_select_parity_every_class(mixed, cls, nullable):
    h = mixed[1 if nullable else 0]
    d = RawStr(h, voff=5 if nullable else 0)
    n = len(h)
    for pat in PATTERNS[cls]:
        assert like_ref.kind(pat) == KIND_OF[cls], pat
        ran = check_select(like(0, pat), [h], [d], n, what=pat)
        assert sum(ran.values()) == 1, (pat, ran)  # one pre-pass per LIKE node


def test_quirks_on_the_device():
    vals = [b"", "é".encode(), b"v%xx", b"%", b"a\\b", b"ab"]
    h = Column.from_strings(vals)
    d = DevCol(h)
    sel = lambda pat: [vals[i] for i in gpu_select(like(0, pat), [d], len(vals))]
    assert sel(b"%%%") == vals[1:]          # '' LIKE '%%%' is false
    assert sel(b"%%") == vals and sel(b"%") == vals
    assert sel(b"a\\b") == [b"a\\b"]        # raw compare, the backslash a byte
    assert sel(b"_") == [b"%"] and sel(b"__") == ["é".encode(), b"ab"]
    assert sel(b"\\%") == [b"%"] and sel(b"_\\%%") == [b"v%xx"]


# ---- b. three-valued logic ---------------------------------------------------------------------------
def test_three_valued_logic(mixed):
    _, h = mixed
    n = len(h)
    rng = np.random.default_rng(12)
    x = Column.from_numbers(col.Int32, rng.integers(0, 10, n).astype(np.int32), rng.random(n) < 0.9)
    dh, dx = DevCol(h, voff=3), DevCol(x, voff=7)
    preds = {
        "not_like": not_like(0, b"%a%"),
        "like_and_cmp": and_(like(0, b"%a%"), cmp(1, "<", 5)),
        "like_or_is_null": or_(like(0, b"a%b"), is_null(0)),
        "not_or_like_like": not_(or_(like(0, b"%a%"), like(0, b"_\\%%"))),
        "not_like_complex_and_not_null_cmp": and_(not_like(0, b"%_a"), not_(cmp(1, "=", 3))),
    }
    for name, p in preds.items():
        check_select(p, [h, x], [dh, dx], n, what=name)
    null_rows = set(np.flatnonzero(~np.asarray(h.validity, bool)).tolist())
    assert null_rows
    for p in (like(0, b"%a%"), not_like(0, b"%a%"), like(0, b"%%"), not_like(0, b"%%")):
        assert not null_rows & set(gpu_select(p, [dh, dx], n).tolist())


# ---- c. like_scan_kernel's boundaries, each case through both kernels -----------------------------------
def both_kernels(h: Column, needle: bytes, what, **raw):
    d = RawStr(h, **raw)
    pat = b"%" + needle + b"%"
    for kernel in ("scan", "rows"):
        ran = check_select(like(0, pat), [h], [d], len(h), kernel=kernel, what=what)
        assert ran == dict(fill=0, rows=int(kernel == "rows"), scan=int(kernel == "scan")), (what, kernel, ran)
    return len(like_ref.select(like(0, pat), [h], len(h)))


def implanted(rng, total, needle, positions, max_row=40, filler=b"xyz"):
    """A blob of `total` filler bytes cut into rows of 0..max_row bytes, the needle written at the
    given blob positions, each inside one row (a cut that would fall inside an occurrence is dropped)."""
    blob = bytearray(bytes(rng.choice(np.frombuffer(filler, np.uint8), total)))
    for p in positions:
        blob[p:p + len(needle)] = needle
    cuts = [0]
    while cuts[-1] < total:
        c = min(total, cuts[-1] + int(rng.integers(0, max_row + 1)))
        if any(p < c < p + len(needle) for p in positions):
            continue
        cuts.append(c)
    return Column.from_strings([bytes(blob[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])


def test_scan_occurrences_across_chunks_waves_and_tiles():
    rng = np.random.default_rng(31)
    needle = b"google"
    # starts that straddle a 16-byte lane chunk, a wave's 1 KiB span, a workgroup sweep (4 KiB) and a
    # tile edge — for a blob whose base is 16-byte aligned, and for bases 11 and 40 bytes off, where the
    # same rows straddle other chunks
    pos = [11, 61, 111, 144, 1019, 2047, 4093, 8192, TILE - 5, TILE + 4093, 2 * TILE - 1, 2 * TILE + 1021, 3 * TILE, 3 * TILE + 700]
    h = implanted(rng, 3 * TILE + 900, needle, pos)
    assert both_kernels(h, needle, "aligned") == len(pos)
    assert both_kernels(h, needle, "skewed", skew=11, first=0, around=needle) == len(pos)
    assert both_kernels(h, needle, "first!=0", skew=3, first=37, around=needle) == len(pos)


def test_scan_row_boundary_is_not_a_match():
    rows = [b"xxgoo", b"glexx", b"goo", b"gle", b"g", b"o", b"o", b"g", b"l", b"e", b"", b"google", b"goog", b"", b"le"]
    h = Column.from_strings(rows * 40)
    assert both_kernels(h, b"google", "row boundary") == 40


def test_scan_row_longer_than_two_tiles():
    rng = np.random.default_rng(32)
    long1 = bytearray(bytes(rng.choice(np.frombuffer(b"xyz", np.uint8), 2 * TILE + 5000)))
    for p in (3, TILE + 100, 2 * TILE + 4000):
        long1[p:p + 6] = b"google"
    long2 = bytearray(bytes(rng.choice(np.frombuffer(b"xyz", np.uint8), 2 * TILE + 3000)))
    long2[2 * TILE + 2990:2 * TILE + 2996] = b"google"  # only in the part its third tile covers
    long3 = bytes(rng.choice(np.frombuffer(b"xyz", np.uint8), 2 * TILE + 100))  # no occurrence
    rows = [b"ab", bytes(long1), b"", b"google", bytes(long2), b"x", long3, b"goo"]
    h = Column.from_strings(rows)
    assert both_kernels(h, b"google", "long rows") == 3
    assert both_kernels(h, b"google", "long rows, skewed", skew=9, first=21, around=b"google") == 3


def test_scan_runs_of_tiny_rows():
    rng = np.random.default_rng(33)
    tiny = [b"", b"a", b"aa", b"b", b"ab", b"ba"]
    vals = [tiny[i] for i in rng.integers(0, len(tiny), 1500)] + [b"xxabxx"] + [tiny[i] for i in rng.integers(0, len(tiny), 1500)]
    valid = rng.random(len(vals)) < 0.7
    h = Column.from_strings(vals, valid)
    for needle in (b"a", b"aa", b"ab", b"aba"):
        both_kernels(h, needle, ("tiny rows", needle), voff=13)


def test_scan_needle_lengths_and_overlaps():
    cap = abi.LIKE_MAX_PATTERN - 2  # the longest needle a '%needle%' pattern holds
    big = bytes((i * 7 + 1) % 251 + 1 for i in range(cap)).replace(b"%", b"!").replace(b"_", b"!").replace(b"\\", b"!")
    rows = [b"a", b"b", b"ab", b"aaaa", b"", b"abc", b"xabcx", big, big[:-1], b"q" + big, big + b"q", big[1:], b"aa", b"aaa"]
    h = Column.from_strings(rows * 3)
    assert both_kernels(h, b"a", "one byte") >= 3 * 7
    assert both_kernels(h, b"aa", "overlapping occurrences") == 3 * 3
    assert both_kernels(h, b"ab", "needle == row") == 3 * 3
    assert both_kernels(h, b"abc", "needle == row, row + 1") == 3 * 2
    assert both_kernels(h, b"abcd", "needle longer than every candidate") == 0
    assert both_kernels(h, big, "needle at the cap") == 3 * 3
    assert len(b"%" + big + b"%") == abi.LIKE_MAX_PATTERN


def test_scan_hit_in_the_last_bytes_and_small_batches():
    h = Column.from_strings([b"xyz"] * 700 + [b"xxgoogle"])
    assert both_kernels(h, b"google", "last bytes") == 1
    assert both_kernels(h, b"google", "last bytes, bytes beyond the blob", skew=7, first=5, around=b"google") == 1
    one = Column.from_strings([b"a google b"])
    assert both_kernels(one, b"google", "one row") == 1
    assert both_kernels(Column.from_strings([b"goog"]), b"google", "one row shorter than the needle") == 0
    assert both_kernels(Column.from_strings([b""]), b"g", "one empty row") == 0
    empty = Column.from_strings([])
    d = RawStr(empty)
    for kernel in ("scan", "rows"):
        with forced(kernel):
            assert len(gpu_select(like(0, b"%google%"), [d], 0)) == 0


# ---- d. fused into GROUP BY ------------------------------------------------------------------------------
N = 6000


@pytest.fixture(scope="module")
def urls():
    """URL-like strings sharing a 19-byte prefix, ~30 % holding 'google'; String and Int64 keys; a value."""
    rng = np.random.default_rng(41)
    alnum = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789/.-_%", np.uint8)
    out = []
    for i in range(N):
        tail = bytearray(bytes(rng.choice(alnum, int(rng.integers(21, 101)))))
        r = rng.random()
        if r < 0.3:
            p = int(rng.integers(0, len(tail) - 5))
            tail[p:p + 6] = b"google"
        elif r < 0.4:
            tail[0:6] = b"goo.gl"
        out.append(b"http://example.com/" + bytes(tail))
    url = Column.from_strings(out)
    words = [b"", b"phrase", b"another search phrase", b"k", b"\xff\x00", b"never google"] + [b"w%d" % i for i in range(60)]
    kidx = rng.integers(0, len(words), N)
    # the group 'never google' holds no matching row, the group 'k' only matching ones
    for i in range(N):
        hit = b"google" in out[i]
        if words[kidx[i]] == b"never google" and hit:
            kidx[i] = 1
        if words[kidx[i]] == b"k" and not hit:
            kidx[i] = 2
    skey = Column.from_strings([words[i] for i in kidx])
    ikey = Column.from_numbers(col.Int64, rng.integers(0, 50, N) * 1_000_003 - 7)
    v = Column.from_numbers(col.Int64, rng.integers(-1000, 1000, N))
    return dict(url=url, skey=skey, ikey=ikey, v=v)


def delta(before, after):
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def test_q22_shape_string_key_min_url(urls):
    """SELECT key, MIN(url), COUNT(*) WHERE url LIKE '%google%' AND key <> '' GROUP BY key: the
    String-key family's general-predicate kernel, not the `key <op> ''` specialisations."""
    url, key = urls["url"], urls["skey"]
    pred = and_(like(0, "%google%"), cmp(1, "<>", ""))
    mask = like_ref.evaluate(pred, [url, key], N) == TRUE
    exp = reference([key], [("min", url), ("count", None)], selected=mask)
    assert (b"never google",) not in exp and (b"",) not in exp and (b"k",) in exp
    for on_device in (True, False):
        info = {}
        gk, ga = gpu_aggregate([key], [("min", url), ("count", None)], filt=(pred, [url, key]), on_device=on_device,
                               share_filter_columns=True, capacity_hint=1 << 17, info=info)
        assert as_dict(gk, ga) == exp, on_device
        paths = {k: v for k, v in info["insert_paths"].items() if v}
        assert paths == {"generic": 1}, paths


def test_single_like_node_takes_no_specialised_predicate_path(urls):
    url, skey, ikey, v = urls["url"], urls["skey"], urls["ikey"], urls["v"]
    d_url, d_skey, d_ikey, d_v = DevCol(url), DevCol(skey), DevCol(ikey), DevCol(v)
    # Int64 key + SUM: the fast kernel folds `key <op> const` only; a LIKE program goes to the generic insert
    t = Table([ikey.dtype], [("count", None), ("sum", v.dtype)])
    try:
        for pred, fcols, dcols in ((like(0, "%google%"), [url], [d_url]),
                                   (and_(like(0, "%google%"), cmp(1, ">", 0)), [url, ikey], [d_url, d_ikey])):
            before = t.paths()
            got = t.run([d_ikey], [None, d_v], pred, dcols)
            mask = like_ref.evaluate(pred, fcols, N) == TRUE
            assert got == pred_ref.group_reference(mask, [ikey], [v])
            assert delta(before, t.paths()) == {"generic": 1}
    finally:
        t.close()
    # one String key in a large key-caching table, a lone LIKE node on the key's own column, the
    # empty pattern (str_len == 0) included: neither agg_insert_str1_kernel<true> nor the `''` queue
    t = Table([skey.dtype], [("count", None), ("sum", v.dtype)], capacity_hint=1 << 17)
    try:
        for pat in (b"", b"%a%", b"w1%", b"%_%"):
            before = t.paths()
            got = t.run([d_skey], [None, d_v], like(0, pat), [d_skey])
            mask = like_ref.evaluate(like(0, pat), [skey], N) == TRUE
            assert got == pred_ref.group_reference(mask, [skey], [v]), pat
            assert delta(before, t.paths()) == {"generic": 1}, pat
    finally:
        t.close()
    # the short-key kernel evaluates whole programs (eval_pred): a LIKE program stays on it
    t = Table([skey.dtype], [("count", None), ("sum", v.dtype)])
    try:
        before = t.paths()
        pred = and_(like(1, "%google%"), not_like(0, b"w_"))
        got = t.run([d_skey], [None, d_v], pred, [d_skey, d_url])
        mask = like_ref.evaluate(pred, [skey, url], N) == TRUE
        assert got == pred_ref.group_reference(mask, [skey], [v])
        assert delta(before, t.paths()) == {"short": 1}
    finally:
        t.close()


def test_partitioned_payload_takes_the_generic_level_1(urls):
    url, skey, ikey, v = urls["url"], urls["skey"], urls["ikey"], urls["v"]
    d_url, d_skey, d_ikey, d_v = DevCol(url), DevCol(skey), DevCol(ikey), DevCol(v)
    # fixed-width keys and arguments (pp_l1_fixed_kernel's shape) with a lone LIKE node
    t = Table([ikey.dtype], [("count", None), ("sum", v.dtype)], strategy=abi.STRATEGY_PARTITIONED)
    try:
        before = t.paths()
        got = t.run([d_ikey], [None, d_v], like(0, "%google%"), [d_url])
        mask = like_ref.evaluate(like(0, "%google%"), [url], N) == TRUE
        assert got == pred_ref.group_reference(mask, [ikey], [v])
        assert t.ht.strategy()[0] and delta(before, t.paths()) == {"pp_generic": 1}
    finally:
        t.close()
    # one String key, COUNT(*) only, the predicate on the key's own column (the String form's shape)
    t = Table([skey.dtype], [("count", None)], strategy=abi.STRATEGY_PARTITIONED)
    try:
        before = t.paths()
        got = t.run([d_skey], [None], like(0, b"w_"), [d_skey])
        mask = like_ref.evaluate(like(0, b"w_"), [skey], N) == TRUE
        exp = pred_ref.group_reference(mask, [skey], [])
        assert got == {k: (c,) for k, (c, _) in exp.items()} and len(got) == 10
        assert t.ht.strategy()[0] and delta(before, t.paths()) == {"pp_generic": 1}
    finally:
        t.close()


# ---- e. batches ----------------------------------------------------------------------------------------
def test_two_device_batches_keep_their_own_masks(urls):
    url, ikey, v = urls["url"], urls["ikey"], urls["v"]
    from tests.test_gpu_parity import slice_col
    half = N // 2
    parts = [(0, half, b"%google%"), (half, N, b"%goo.gl%")]
    fns = [FN.get("count", [], []), FN.get("sum", [], [v.dtype])]
    ht = AggregateHashTable(AggregatorParams([ikey.dtype], fns), HashTableConfig(True, 0))
    try:
        mask = np.zeros(N, bool)
        before = kernel_counts()
        for lo, hi, pat in parts:
            k, a, u = (DevCol(slice_col(c, lo, hi)) for c in (ikey, v, url))
            ht.add_groups([k], [None, a], rows=hi - lo, filter_program=FilterProgram(like(0, pat), [u]), on_device=True)
            mask[lo:hi] = like_ref.evaluate(like(0, pat), [slice_col(url, lo, hi)], hi - lo) == TRUE
        block = ht.merge_result()  # both inserts ran before either mask could be reused
        assert pred_ref.result_dict(block.columns[2:], block.columns[:2]) == pred_ref.group_reference(mask, [ikey], [v])
        assert sum(kernel_counts().values()) - sum(before.values()) == 2
        assert mask[:half].any() and mask[half:].any()
    finally:
        ht.close()


def test_growth_and_rehash_over_three_batches():
    """More groups than the initial table holds: the overflow retry and the rehash read each batch's
    predicate — and so its mask — again, after later batches were added."""
    rng = np.random.default_rng(51)
    n = 150_000
    keys = [Column.from_numbers(col.Int64, rng.integers(0, 40_000, n) * 7919 - 12345)]
    words = [b"a google b", b"nothing", b"goo gle", b"xgooglex"]
    s = Column.from_strings([words[i] for i in rng.integers(0, len(words), n)])
    v = Column.from_numbers(col.Int64, rng.integers(-100, 100, n))
    pred = like(0, b"%google%")
    mask = like_ref.evaluate(pred, [s], n) == TRUE
    exp = pred_ref.group_reference(mask, keys, [v])
    assert len(exp) > 32768 / 1.5
    for on_device in (True, False):
        gk, ga = gpu_aggregate(keys, [("count", None), ("sum", v)], filt=(pred, [s]), on_device=on_device, batches=3)
        assert pred_ref.result_dict(gk, ga) == exp, on_device


def test_host_staging_flushes_when_the_pattern_differs_in_one_byte():
    rng = np.random.default_rng(52)
    blk = 65_536
    words = [b"see google.com", b"see goegle.com", b"plain", b""]
    mk = lambda n: (Column.from_numbers(col.Int32, rng.integers(0, 300, n).astype(np.int32)),
                    Column.from_strings([words[i] for i in rng.integers(0, len(words), n)]),
                    Column.from_numbers(col.Int64, rng.integers(-50, 50, n)))
    blocks = [mk(blk), mk(blk), mk(5000)]
    pats = [b"%google%", b"%google%", b"%goegle%"]
    fns = [FN.get("count", [], []), FN.get("sum", [], [col.Int64])]
    ht = AggregateHashTable(AggregatorParams([col.Int32], fns), HashTableConfig(True, 0))
    try:
        ht.set_host_staging(1 << 20)
        for (k, s, v), pat in zip(blocks, pats):
            ht.add_groups([k], [None, v], filter_program=FilterProgram(like(0, pat), [s]), on_device=False)
        assert sum(ht.insert_paths().values()) == 1  # the first two blocks, flushed by the third's different program
        block = ht.merge_result()
        assert sum(ht.insert_paths().values()) == 2
        got = pred_ref.result_dict(block.columns[2:], block.columns[:2])
    finally:
        ht.close()
    cat = lambda cs: Column.from_numbers(cs[0].dtype, np.concatenate([np.asarray(c.data) for c in cs]))
    mask = np.concatenate([like_ref.evaluate(like(0, pat), [s], len(s)) == TRUE for (_, s, _), pat in zip(blocks, pats)])
    exp = pred_ref.group_reference(mask, [cat([b[0] for b in blocks])], [cat([b[2] for b in blocks])])
    assert got == exp
    assert mask[2 * blk:].any() and mask[:blk].any()


# ---- f. refusals ---------------------------------------------------------------------------------------------
def test_refusals_run_no_kernel(urls):
    url, ikey, v = urls["url"], urls["ikey"], urls["v"]
    d_url, d_ikey, d_v = DevCol(url), DevCol(ikey), DevCol(v)
    sel = __import__("torch").empty(N, dtype=__import__("torch").int32, device="cuda")

    def programs():
        wrong_col = FilterProgram(like(0, "%google%"), [d_url, d_ikey])
        wrong_col.nodes[0].col = 1  # an Int64 column (FilterProgram itself refuses to build this)
        null_str = FilterProgram(like(0, "%google%"), [d_url])
        null_str.nodes[0].str = None
        out_of_range = FilterProgram(like(0, "%google%"), [d_url])
        out_of_range.nodes[0].col = 1
        return [("non-String column", wrong_col, abi.DBG_ERR_INVALID, "String"),
                ("null pattern with a length", null_str, abi.DBG_ERR_INVALID, "null"),
                ("column out of range", out_of_range, abi.DBG_ERR_INVALID, "out of range"),
                ("pattern over the cap", FilterProgram(like(0, b"%" + b"a" * abi.LIKE_MAX_PATTERN), [d_url]), abi.DBG_ERR_UNSUPPORTED,
                 str(abi.LIKE_MAX_PATTERN)),
                ("segments over the cap", FilterProgram(like(0, b"%".join([b"s"] * (abi.LIKE_MAX_SEGMENTS + 1))), [d_url]),
                 abi.DBG_ERR_UNSUPPORTED, str(abi.LIKE_MAX_SEGMENTS))]

    fns = [FN.get("count", [], []), FN.get("sum", [], [v.dtype])]
    ht = AggregateHashTable(AggregatorParams([ikey.dtype], fns), HashTableConfig(True, 0))
    try:
        before = kernel_counts()
        for name, prog, code, word in programs():
            n_sel = C.c_uint64()
            assert lib().dbg_filter_select(prog.ptr(), N, sel.data_ptr(), C.byref(n_sel), None) == code, name
            assert word in lib().dbg_last_error().decode(), (name, lib().dbg_last_error())
            with pytest.raises(Unsupported if code == abi.DBG_ERR_UNSUPPORTED else DbgError) as e:
                ht.add_groups([d_ikey], [None, d_v], rows=N, filter_program=prog, on_device=True)
            assert e.value.code == code, name
        assert kernel_counts() == before and sum(ht.insert_paths().values()) == 0
        with pytest.raises(DbgError) as e:
            FilterProgram(like(1, "%google%"), [d_url, d_ikey])
        assert e.value.code == abi.DBG_ERR_INVALID
        # the handle still works
        ht.reset()
        ht.add_groups([d_ikey], [None, d_v], rows=N, filter_program=FilterProgram(like(0, "%google%"), [d_url]), on_device=True)
        block = ht.merge_result()
        mask = like_ref.evaluate(like(0, "%google%"), [url], N) == TRUE
        assert pred_ref.result_dict(block.columns[2:], block.columns[:2]) == pred_ref.group_reference(mask, [ikey], [v])
    finally:
        ht.close()
