"""The Parquet page case table (tests/pq_pages.py) on the CPU: every stream's expected bytes are
what libsnappy and liblz4 (pyarrow's codecs) and the oracle's decoders give, every chunk decodes
through oracle.parquet_oracle.decode_chunk to the expected rows, the walkers find every feature
a case claims, every feature the table must contain is claimed by some case, the window sweeps
cover the range that brackets the first restage boundary, and every malformed page is refused by
libsnappy / liblz4 or, for the hybrid and page-level ones, by the walker assertion the table names.
The lane arithmetic of the device is tests/test_gpu_pq_pages.py."""
import pytest

pa = pytest.importorskip("pyarrow")

from oracle import parquet_oracle as pq  # noqa: E402
from tests import pq_pages as pp  # noqa: E402

NAMES = [c.name for c in pp.cases()]
LIB = {pp.SNAPPY: "snappy", pp.LZ4_RAW: "lz4_raw"}


def oracle_rows(chunk, c):
    rows = pq.decode_chunk(chunk, c.ptype, c.codec, c.max_def, c.tlen)
    if c.ptype == pp.FLBA:
        rows = [None if v is None else pq.be_decimal(v) for v in rows]
    return rows


def test_enums_match_the_oracle():
    assert (pp.BOOLEAN, pp.INT32, pp.INT64, pp.BYTE_ARRAY, pp.FLBA) == (pq.BOOLEAN, pq.INT32, pq.INT64, pq.BYTE_ARRAY, pq.FIXED_LEN_BYTE_ARRAY)
    assert (pp.UNCOMPRESSED, pp.SNAPPY, pp.ZSTD, pp.LZ4_RAW) == (pq.UNCOMPRESSED, pq.SNAPPY, pq.ZSTD, pq.LZ4_RAW)
    assert (pp.PLAIN, pp.RLE, pp.RLE_DICTIONARY) == (pq.PLAIN, pq.RLE, pq.RLE_DICTIONARY)
    assert (pp.DATA_PAGE, pp.DICTIONARY_PAGE, pp.DATA_PAGE_V2) == (pq.DATA_PAGE, pq.DICTIONARY_PAGE, pq.DATA_PAGE_V2)


@pytest.mark.parametrize("name", NAMES)
def test_case(name):
    c = pp.case(name)
    for stream, exp in c.streams:
        if c.lib:
            assert pa.decompress(stream, decompressed_size=len(exp), codec=LIB[c.codec], asbytes=True) == exp, name
        assert pq.decompress(c.codec, stream, len(exp)) == exp, name
    assert oracle_rows(b"".join(c.pages), c) == c.expected, name
    feats = pp.features(c)
    missing = sorted(k for k in c.claims if not feats[k])
    assert not missing, (name, "claimed features not produced", missing, dict(feats))


def test_liblz4_refuses_only_the_case_marked():
    """lz_last_nolits ends with a match and a lone zero token: liblz4 wants the last five bytes
    of a block to be literals, the oracle and the kernel take the block as the format describes it."""
    marked = [c.name for c in pp.cases() if c.streams and not c.lib]
    assert marked == ["lz_last_nolits"]
    (stream, exp), = pp.case("lz_last_nolits").streams
    with pytest.raises(Exception):
        pa.decompress(stream, decompressed_size=len(exp), codec="lz4_raw", asbytes=True)


def test_table_covers_every_path():
    """Every feature the table must contain is claimed by at least one case."""
    claimed = set().union(*(c.claims for c in pp.cases()))
    back = {"off_%d" % o for o in pp.EDGE_OFFS} | {"off_1", "off_lt64_npot", "off_eq_w", "off_half_ring", "off_ge_ring", "overlap",
                                                   "ring_multiseg", "ring_multiseg_half", "ring_seg_plus1", "ring_multiseg_x3"}
    want = {"sn_" + k for k in back | {"lit_short", "lit_1b", "lit_2b", "lit_3b", "lit_4b", "lit_4b_small", "lit_gt_iwin", "copy_k1", "copy_k2",
                                       "copy_k3", "copy_k3_gt_65535", "off_gt_65535", "ring_seg_1byte_x64", "end_after_tag"}}
    want |= {"lz_" + k for k in back | {"far_overlap", "off_1_long", "off_lt64_npot_long", "lit0", "lit_gt_iwin", "last_lits", "last_nolits"}}
    want |= {"lz_%s_%s" % (w, k) for w in ("lit", "ml") for k in ("nochain", "chain_0", "chain_1", "chain_2", "chain_ge40")}
    want |= {"idx_bw_%d" % b for b in range(33)} | {"idx_topbit_bw%d" % b for b in range(1, 21)} | {"idx_bw_0_explicit", "page_all_null_no_index"}
    want |= {"idx_rle_vb%d" % v for v in (1, 2, 3, 4)} | {"def_bw_1"}
    want |= {"%s_runs_%d" % (s, n) for s in ("def", "idx") for n in pp.EDGE_RUNS}
    want |= {"%s_%s" % (s, k) for s in ("def", "idx") for k in ("alternating", "runs_gt_rmax", "runs_gt_2rmax", "rle_overshoot", "bp_overshoot",
                                                                "padded_varint", "pad_bits_set")}
    want |= {"idx_bp_truncated", "page_zero_values_between", "bool_rle", "bool_bp", "page_v1_rle", "page_v2_rle",
             "page_v2_compressed", "page_v2_dict_flag_uncompressed"}
    want |= {"mixed_order_%s_%s" % (k, t) for k in ("none", "snappy", "lz4", "zstd") for t in ("int64", "byte_array")}
    want |= {"flba_%d_%s" % (t, k) for t in range(1, 17) for k in ("required", "nullable")}
    want |= {"flba_" + k for k in ("min", "max", "minus1", "zero", "0080", "ff7f")}
    assert not want - claimed, sorted(want - claimed)
    # the patterns of every FIXED_LEN_BYTE_ARRAY length, not of some
    for c in pp.cases():
        if c.ptype == pp.FLBA:
            assert {"flba_min", "flba_max", "flba_minus1", "flba_zero"} <= c.claims and (c.tlen == 1 or {"flba_0080", "flba_ff7f"} <= c.claims)


@pytest.mark.parametrize("name", [c.name for c in pp.cases() if c.sweep])
def test_sweep_brackets_the_window_boundary(name):
    """The swept element's first byte stands at every stream offset of a contiguous range that
    contains [8161 - E, 8176]: the first restage boundary (8176 - sa, sa in [0, 15]) falls before
    every byte of the element, and after its last, in some page, whatever sa is."""
    c = pp.case(name)
    at, elen = pp.sweep_positions(c)
    assert at == list(range(at[0], at[0] + len(at))), "not contiguous"
    assert at[0] <= pp.IWIN - 15 - elen and at[-1] >= pp.IWIN, (at[0], at[-1], elen)
    assert len(c.pages) == len(at) and max(len(p) for p in c.pages) < 12_000


def test_pages_are_small():
    for c in pp.cases():
        limit = (5 << 20) if c.name == "hy_index_widths" else (4 << 20) if c.sweep else 200 * 1024
        assert sum(len(p) for p in c.pages) <= limit, c.name
        for _, exp in c.streams:
            assert len(exp) <= 200 * 1024, c.name


def test_walkers_reject_what_they_check():
    with pytest.raises(AssertionError):
        pp.walk_snappy(pp.snappy([pp.lit(b"abc"), pp.copy(2, 4, 5)], check=False)[0])
    with pytest.raises(AssertionError):
        pp.walk_snappy(pp.snappy([pp.lit(b"abc")], preamble=4)[0])
    with pytest.raises(AssertionError):
        pp.walk_lz4(pp.lz4([(b"abc", 4, 5), (b"", 0, 0)], check=False)[0], 8)
    with pytest.raises(AssertionError):
        pp.walk_lz4(pp.lz4([(b"abc", 3, 5), (b"x", 0, 0)])[0], 10)
    with pytest.raises(AssertionError):
        pp.walk_hybrid(pp.hybrid([pp.rle(3, 1)], 1), 1, 4)


@pytest.mark.parametrize("name", [m.name for m in pp.malformed()])
def test_malformed_rejected(name):
    m = next(x for x in pp.malformed() if x.name == name)
    if m.lib:
        try:
            refused = len(pa.decompress(m.stream, decompressed_size=m.size, codec=LIB[m.codec], asbytes=True)) != m.size
        except Exception:
            refused = True
        assert refused, (name, m.reason)
        with pytest.raises(AssertionError):
            pp.walk_snappy(m.stream) if m.codec == pp.SNAPPY else pp.walk_lz4(m.stream, m.size)
    elif m.stream is not None:
        with pytest.raises(AssertionError, match=m.reason):
            pp.walk_lz4(m.stream, m.size)
    else:
        c = pp.Case(m.name, m.codec, m.ptype, m.max_def, 0, m.target, (m.chunk,), None, frozenset(), (), False, None)
        with pytest.raises(AssertionError, match=m.reason):
            pp.walk_chunk(c)


def test_malformed_are_one_step_from_good():
    """The good neighbours decode: a malformed page is refused for the one thing changed."""
    chunk, rows = pp.malformed_good()
    assert pq.decode_chunk(chunk, pp.INT64, pp.UNCOMPRESSED, 1) == rows
    c = pp.Case("good", pp.UNCOMPRESSED, pp.INT64, 1, 0, "i64", (chunk,), rows, frozenset(), (), False, None)
    assert pp.walk_chunk(c)["idx_bw_3"] == 1
    for name, (chunk, rows) in pp.wide_good().items():
        assert pq.decode_chunk(chunk, pp.INT64, pp.UNCOMPRESSED, 1) == rows, name
        bad = next(m for m in pp.malformed() if m.name == "hy_" + name.replace("_low", "_high"))
        diff = [i for i, (a, b) in enumerate(zip(chunk, bad.chunk)) if a != b]
        assert len(chunk) == len(bad.chunk) and len(diff) == 1 and bad.chunk[diff[0]] == chunk[diff[0]] | 0x80 >> (-int(name.split("_")[1]) % 8), name
    (s, e), = pp.case("sn_end_on_copy_k2").streams  # the Snappy ones' neighbour: 40 literals and a 24-byte copy
    assert len(e) == 64 and pa.decompress(s, decompressed_size=64, codec="snappy", asbytes=True) == e
    s, e = pp.lz4([(bytes(range(40)), 17, 19), (b"12345", 0, 0)])
    assert len(e) == 64 and pa.decompress(s, decompressed_size=64, codec="lz4_raw", asbytes=True) == e


def test_headers_read_back():
    """The three page headers as the oracle parses them."""
    chunk = pp.page_dict(b"x" * 16, 2) + pp.page_v1(b"v" * 9, 70_000, pp.RLE_DICTIONARY, defs=b"dd") + \
        pp.page_v2(b"w" * 300, 5, 3, pp.PLAIN, defs=b"ddd", is_compressed=False) + pp.page_v2(b"w", 1 << 20, 0, pp.RLE, defs=b"")
    d, p1, p2, p3 = pq.parse_pages(chunk)
    assert (d.ptype, d.uncompressed, d.compressed, d.num_values, d.encoding) == (pq.DICTIONARY_PAGE, 16, 16, 2, pq.PLAIN)
    assert (p1.ptype, p1.uncompressed, p1.compressed, p1.num_values, p1.encoding) == (pq.DATA_PAGE, 15, 15, 70_000, pq.RLE_DICTIONARY)
    assert chunk[p1.data_off:p1.data_off + 15] == b"\x02\x00\x00\x00dd" + b"v" * 9
    assert (p2.ptype, p2.uncompressed, p2.compressed, p2.num_values, p2.encoding, p2.def_len, p2.rep_len, p2.v2_compressed) == \
        (pq.DATA_PAGE_V2, 303, 303, 5, pq.PLAIN, 3, 0, False)
    assert (p3.num_values, p3.encoding, p3.def_len, p3.v2_compressed) == (1 << 20, pq.RLE, 0, True)
