"""The device page decode (scan.hip: pq_inflate_kernel, one wave per page; hybrid_expand and put_value
in pq_decode_kernel, one workgroup per page) on the case table of tests/pq_pages.py, through
ParquetChunkDecoder: values and validity exactly as the table expects them.  Only this build has
64 lanes and LDS: the 64-wide copies with j % off, the 32 KiB ring and its segments, the ring /
output split, the 8176-byte input window restaged between a tag and its extra bytes, the run
table refilled after 512 runs run nowhere else.  tests/test_pq_pages.py pins the same table on the
CPU (libsnappy, liblz4, the oracle, the walkers) and says which case reaches which path; a
mismatch here names the case, the first differing byte or row and the walker's features of the case,
which name the path that was live."""
import numpy as np
import pytest

pytest.importorskip("pyarrow")

from databend_amd import column as col  # noqa: E402
from databend_amd.ffi import DbgError  # noqa: E402
from databend_amd.scan import ColumnChunk, ParquetChunkDecoder  # noqa: E402
from tests import pq_pages as pp  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in pp.cases()]
TARGET = {"i64": col.Int64, "i32": col.Int32, "str": col.String, "bool": col.Boolean, "dec": col.Decimal128(38, 0)}


@pytest.fixture(scope="module")
def dec():
    d = ParquetChunkDecoder()
    yield d
    d.close()


def decode(dec, chunk, codec, ptype=pp.INT64, max_def=0, tlen=0, target="i64"):
    t = TARGET[target]
    return dec.decode(ColumnChunk(chunk, ptype, max_def, tlen, codec), t.wrap_nullable() if max_def else t).to_host()


def check_streams(dec, cs):
    """Stream cases as the pages of one required INT64 chunk, byte for byte."""
    codec = cs[0].codec
    assert all(c.codec == codec and c.streams for c in cs)
    got = np.asarray(decode(dec, b"".join(p for c in cs for p in c.pages), codec).data).tobytes()
    want = b"".join(e for c in cs for _, e in c.streams)
    assert len(got) == len(want)
    if got != want:
        at = int(np.nonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))[0][0])
        start = 0
        for c in cs:
            for k, (_, e) in enumerate(c.streams):  # the page that holds the first differing byte
                if at < start + len(e):
                    pytest.fail("case %s page %d: first differing byte at %d of %d (chunk byte %d); walker maxima %r, features %r"
                                % (c.name, k, at - start, len(e), at, pp.maxima(c), dict(pp.features(c))))
                start += len(e)


def check_chunk(dec, c):
    got = decode(dec, b"".join(c.pages), c.codec, c.ptype, c.max_def, c.tlen, c.target).values()
    assert len(got) == len(c.expected), (c.name, len(got), len(c.expected))
    if got != c.expected:
        at = next(i for i, (a, b) in enumerate(zip(got, c.expected)) if a != b)
        pytest.fail("case %s: first differing row %d of %d: got %r, expected %r; features %r"
                    % (c.name, at, len(got), got[at], c.expected[at], dict(pp.features(c))))


def run_case(dec, name):
    c = pp.case(name)
    if c.streams:
        check_streams(dec, [c])
    else:
        check_chunk(dec, c)


@pytest.mark.parametrize("name", NAMES)
def test_case(dec, name):
    """One case, one chunk; a window sweep is one chunk of all its pages (one launch)."""
    run_case(dec, name)


@pytest.mark.parametrize("order", ["table", "reversed"])
@pytest.mark.parametrize("codec", [pp.SNAPPY, pp.LZ4_RAW], ids=["snappy", "lz4"])
def test_stream_cases_one_launch(dec, codec, order):
    """Every stream case of a codec as a page of one chunk: one launch, one wave per page, long and
    short pages as neighbours."""
    cs = pp.stream_cases(codec)
    assert len(cs) >= 9
    check_streams(dec, cs if order == "table" else cs[::-1])


def test_nothing_survives_between_calls(dec):
    """A chunk with 1025-run pages, the 2^20-entry dictionary, a short chunk and the first again on one
    decoder: the run table, the index scratch and the page buffer of a call are not what the next reads."""
    for name in ("hy_runs_1025", "hy_index_widths", "hy_truncated_tail", "lz_ring_segments", "sn_off_eq_w_small", "hy_runs_1025"):
        run_case(dec, name)


@pytest.mark.parametrize("name", [m.name for m in pp.malformed()])
def test_malformed_is_an_error(dec, name):
    """Each malformed page is a decode error, and the decoder decodes a good chunk afterwards."""
    m = next(x for x in pp.malformed() if x.name == name)
    with pytest.raises(DbgError):
        decode(dec, m.chunk, m.codec, m.ptype, m.max_def, 0, m.target)
    chunk, rows = pp.malformed_good()
    assert decode(dec, chunk, pp.UNCOMPRESSED, pp.INT64, 1).values() == rows
    if m.stream is not None:
        check_streams(dec, [pp.case("sn_end_on_copy_k2" if m.codec == pp.SNAPPY else "lz_off_eq_w")])


@pytest.mark.parametrize("name", sorted(pp.wide_good()))
def test_wide_index_good_twin(dec, name):
    """Widths 21..32 with small indices decode: their twins with the top bit set are refused for that bit."""
    chunk, rows = pp.wide_good()[name]
    assert decode(dec, chunk, pp.UNCOMPRESSED, pp.INT64, 1).values() == rows


@pytest.mark.parametrize("codec,good,bad", [(pp.SNAPPY, "sn_offsets_lanes", "sn_copy_off_w_plus_1"), (pp.LZ4_RAW, "lz_lit0", "lz_offset_past_output")],
                         ids=["snappy", "lz4"])
def test_malformed_page_between_good_ones(dec, codec, good, bad):
    """A malformed page between two good ones fails the chunk; the good ones alone decode afterwards."""
    g = pp.case(good)
    m = next(x for x in pp.malformed() if x.name == bad)
    with pytest.raises(DbgError):
        decode(dec, g.pages[0] + m.chunk + g.pages[0], codec)
    check_streams(dec, [g, g])


def testmalformed_hybrid_page_between_good_ones(dec):
    """The same for the hybrid: the pages of a chunk share one dictionary page."""
    good = pp.malformed_hybrid(None)[0]
    bad = pp.malformed_hybrid("rle_run_0")[0]
    rows = pp.malformed_good()[1]
    with pytest.raises(DbgError):
        decode(dec, good[0] + good[1] + bad[1] + good[1], pp.UNCOMPRESSED, pp.INT64, 1)
    assert decode(dec, good[0] + good[1] + good[1], pp.UNCOMPRESSED, pp.INT64, 1).values() == rows + rows
