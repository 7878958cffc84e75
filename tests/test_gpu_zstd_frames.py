"""The device build of the Zstandard decoder (zstd_dev.hpp, pq_zstd_kernel: one wave per page) on
the case table of tests/zstd_frames.py: every case as a required INT64 ZSTD page, byte for byte
against libzstd's output.  Only this build has 64 lanes: the lane walk of a match (r = lane % off,
step = 64 % off), the 64-wide copies, the LDS ring and its segments, the ring / output split at
8192, the syncs between them and the four Huffman streams on lanes 0-3 run nowhere else.
tests/test_zstd_frames.py pins the same table on the CPU (libzstd, the frame walker, the host
build) and says which case reaches which path; a mismatch here reports the walker's maxima of the
case, which name the path that was live."""
import numpy as np
import pytest

from databend_amd import abi
from databend_amd import column as col
from databend_amd.ffi import DbgError
from databend_amd.scan import ColumnChunk, ParquetChunkDecoder
from tests import zstd_frames as zf

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in zf.cases()]


@pytest.fixture(scope="module")
def dec():
    d = ParquetChunkDecoder()
    yield d
    d.close()


def decode(dec, pages: bytes) -> bytes:
    c = dec.decode(ColumnChunk(pages, abi.PQ_INT64, 0, 0, abi.PQ_ZSTD), col.Int64).to_host()
    return np.asarray(c.data).tobytes()


def check(dec, names):
    pages, exp = zip(*(zf.case_page(zf.case(n)) for n in names))
    got, want = decode(dec, b"".join(pages)), b"".join(exp)
    assert len(got) == len(want)
    if got != want:
        at = int(np.nonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))[0][0])
        start = 0
        for n, e in zip(names, exp):  # the page that holds the first differing byte
            if at < start + len(e):
                pytest.fail("case %s: first differing byte at %d of %d (page byte %d); walker maxima %r, features %r"
                            % (n, at - start, len(e), at, zf.inspect(zf.case(n).frame)[1], dict(zf.inspect(zf.case(n).frame)[0])))
            start += len(e)


@pytest.mark.parametrize("name", NAMES)
def test_case(dec, name):
    check(dec, [name])


@pytest.mark.parametrize("order", ["table", "reversed"])
def test_all_cases_one_launch(dec, order):
    """Every case as a page of one chunk: one launch, one wave and one literal scratch slice per
    page, literal modes and block counts mixed across neighbouring waves."""
    check(dec, NAMES if order == "table" else NAMES[::-1])


def test_nothing_survives_between_calls(dec):
    """Huffman literals, raw literals, Huffman again on one decoder: the literal scratch and the
    tables of the first call are not what the third call reads."""
    for name in ("text_l3", "litrun_raw", "few_l1", "nseq0_rle_70000", "text_l3"):
        check(dec, [name])


def test_malformed_pages_are_errors(dec):
    """Frames the host build rejects cleanly under the sanitizers (tests/test_zstd_host.py), as
    pages: a decode error each, and the decoder still decodes a good page afterwards."""
    for m in zf.malformed():
        assert m.size % 8 == 0
        with pytest.raises(DbgError):
            decode(dec, zf.page(m.frame, m.size))
    check(dec, ["repeat_offsets"])
    # a malformed page among good ones fails the chunk
    good = zf.case_page(zf.case("batch_257"))[0]
    bad = next(m for m in zf.malformed() if m.name == "offset_past_output")
    with pytest.raises(DbgError):
        decode(dec, good + zf.page(bad.frame, bad.size) + good)
    check(dec, ["batch_257", "lanes_61_67"])
