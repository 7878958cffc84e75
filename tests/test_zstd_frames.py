"""The zstd case table (tests/zstd_frames.py) on the CPU: for every case libzstd (pyarrow's codec)
gives the expected bytes, the frame walker passes its own consistency assertions and reports every
feature the case claims, and the host build of the device decoder (zstd_dev.hpp under ZS_HOST)
returns the same bytes; every malformed frame is rejected by the host build; and the page wrapper
the GPU tests use reads back through the Parquet oracle.  The lane arithmetic of the device build
is tests/test_gpu_zstd_frames.py; the same frames under the sanitizers are tests/test_zstd_host.py."""
import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")

from oracle import parquet_oracle as pq  # noqa: E402
from tests import zstd_frames as zf  # noqa: E402
from tests.test_zstd_host import _build, _decode  # noqa: E402

NAMES = [c.name for c in zf.cases()]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("zsf")), asan=False)


@pytest.mark.parametrize("name", NAMES)
def test_case(host, name):
    c = zf.case(name)
    if c.libzstd:
        assert pa.decompress(c.frame, decompressed_size=len(c.expected), codec="zstd", asbytes=True) == c.expected
    feats, maxima, n = zf.inspect(c.frame)
    assert n == len(c.expected)
    missing = sorted(k for k in c.claims if not feats[k])
    assert not missing, (name, "claimed features not produced (another libzstd?)", missing, dict(feats), maxima)
    rc, got = _decode(host, c.frame, n)
    assert rc == 0, (name, maxima)
    assert got == c.expected, (name, next(i for i, (a, b) in enumerate(zip(got, c.expected)) if a != b), maxima)


def test_checksum_twin():
    """The frame with the checksum flag differs from its twin by the flag and four trailing bytes
    only, and libzstd, which verifies them, refuses it."""
    on, off = zf.case("checksum_on"), zf.case("checksum_off")
    assert on.expected == off.expected and len(on.frame) == len(off.frame) + 4
    assert on.frame[:4] == off.frame[:4] and on.frame[4] == off.frame[4] | 4 and on.frame[5:-4] == off.frame[5:]
    with pytest.raises(Exception):
        pa.decompress(on.frame, decompressed_size=len(on.expected), codec="zstd", asbytes=True)


def test_table_covers_every_path():
    """Every path of zs_decode that the walker can name is claimed by at least one case."""
    claimed = set().union(*(c.claims for c in zf.cases()))
    want = {"block_raw", "block_rle", "lit_raw", "lit_rle", "lit_treeless", "huf_1stream", "huf_4stream", "huf_direct", "huf_fse",
            "nseq0", "nseq_1byte", "nseq_2byte", "nseq_3byte", "multi_batch", "tail_literals",
            "ring", "ring_multiseg", "ring_overlap", "ring_seg_minus1", "ring_seg_exact", "ring_seg_plus1",
            "ring_off_lt64", "ring_off_eq64", "ring_off_gt64", "far", "far_gt_ring", "far_gt_block", "far_overlap",
            "rep1", "rep2", "rep3", "rep2_ll0", "rep3_ll0", "rep4_ll0", "skippable", "checksum", "empty_frame"}
    want |= {"%s_%s" % (t, m) for t in ("ll", "of", "ml") for m in ("predef", "rle", "fse", "repeat")}
    want |= {"off_%d" % o for o in zf.EDGE_OFFS} | {"ll_%d" % v for v in zf.EDGE_LLS} | {"nseq_%d" % v for v in zf.EDGE_NSEQ}
    assert not want - claimed, sorted(want - claimed)


def test_walker_rejects_what_it_checks():
    """The walker's own assertions fire: a stream one byte too long, literals past the section, an
    offset past the output, a wrong declared size."""
    bad = {m.name: m for m in zf.malformed()}
    for name in ("bitstream_extra_byte", "literals_past_section", "offset_past_output", "repeat_table_first_block",
                 "treeless_first_block", "modes_reserved_bits", "block_past_frame", "frame_reserved_bit"):
        with pytest.raises(AssertionError):
            zf.inspect(bad[name].frame)
    good = zf.case("checksum_off").frame
    with pytest.raises(AssertionError):
        zf.inspect(good[:5] + (len(zf.case("checksum_off").expected) + 1).to_bytes(4, "little") + good[9:])


@pytest.mark.parametrize("name", [m.name for m in zf.malformed()])
def test_malformed_rejected(host, name):
    m = next(x for x in zf.malformed() if x.name == name)
    rc, _ = _decode(host, m.frame, m.size)
    assert rc != 0


def test_malformed_are_one_step_from_good(host):
    """The malformed frames' good neighbours decode: each is rejected for the one thing changed."""
    rng = np.random.default_rng(3)
    lits = rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
    hist = zf.history(rng, 96)
    for seq, size in (((16, 688, zf.new(50)), 800), ((16, 688, zf.new(112)), 800)):  # 112: every byte produced so far
        fr = zf.frame([hist, zf.compressed_block(lits, [seq])])
        exp = pa.decompress(fr, decompressed_size=size, codec="zstd", asbytes=True)
        rc, got = _decode(host, fr, size)
        assert rc == 0 and got == exp


def test_page_wrapper_reads_back():
    """page(): the header fields as the Parquet oracle parses them, and the values it decodes."""
    c = zf.case("litrun_raw")
    fr, exp = zf.pad8(c)
    assert len(exp) % 8 == 0 and len(exp) - len(c.expected) == -len(c.expected) % 8 != 0
    chunk = zf.page(fr, len(exp)) + zf.case_page(zf.case("batch_256"))[0]
    p0, p1 = pq.parse_pages(chunk)
    assert (p0.ptype, p0.uncompressed, p0.compressed, p0.num_values, p0.encoding) == (pq.DATA_PAGE, len(exp), len(fr), len(exp) // 8, pq.PLAIN)
    assert chunk[p0.data_off:p0.data_off + p0.compressed] == fr
    assert p1.num_values == len(zf.case("batch_256").expected) // 8
    vals = pq.decode_chunk(chunk, pq.INT64, pq.ZSTD, 0)
    assert vals == np.frombuffer(exp + zf.case("batch_256").expected, "<i8").tolist()
    # sizes that take one, two and three varint bytes
    for n in (8, 64, 8192, 1 << 20):
        pg, = pq.parse_pages(zf.page(b"x" * 5, n))
        assert (pg.uncompressed, pg.compressed, pg.num_values) == (n, 5, n // 8)
