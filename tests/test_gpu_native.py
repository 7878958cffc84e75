"""GPU parity of the native (strawboat) page decode (dbg_native_decode, scan.hip) against the
restated reader (oracle/native_oracle.py; tests/test_native_oracle.py).  Every codec the device
takes x every integer width, signed and unsigned, Date / Timestamp, String; nullable and not;
Dict with each nested index codec; ragged and 131072-row pages; codecs mixed across the pages of a
column; errors (truncated, corrupt, out-of-range, Freq, float targets) that must come back as
errors, never faults; and native pages -> HBM -> GROUP BY against the aggregation oracle.
Parity is exact: values at every row (NULL rows included — the decoded array holds what the codec
reproduces there) and the validity bitmap.  No reference fixture holds native bytes, so the
restatement is the only anchor ("parity unpinned")."""
import numpy as np
import pytest

from databend_amd import abi
from databend_amd import column as col
from databend_amd.ffi import DbgError, Unsupported
from databend_amd.scan import NativeColumnChunk, ParquetChunkDecoder, deserialize_native_chunks
from oracle import native_oracle as nat

pytestmark = pytest.mark.gpu

INT_TYPES = [  # (target, width, signed)
    (abi.INT8, 1, True), (abi.UINT8, 1, False), (abi.INT16, 2, True), (abi.UINT16, 2, False),
    (abi.INT32, 4, True), (abi.UINT32, 4, False), (abi.DATE, 4, True),
    (abi.INT64, 8, True), (abi.UINT64, 8, False), (abi.TIMESTAMP, 8, True),
]
INT_CODECS = [nat.NONE, nat.LZ4, nat.ZSTD, nat.SNAPPY, nat.RLE, nat.DICT, nat.ONE_VALUE]


@pytest.fixture(scope="module")
def dec():
    d = ParquetChunkDecoder()
    yield d
    d.close()


def _vals(rng, n, width, signed, kind):
    dt = nat._dtype(width, signed)
    lo, hi = (-(1 << (8 * width - 1)), (1 << (8 * width - 1)) - 1) if signed else (0, (1 << (8 * width)) - 1)
    if kind == "runs":
        v = np.repeat(rng.integers(max(lo, -1000), min(hi, 1000), n // 7 + 1), 7)[:n]
    elif kind == "few":
        v = rng.integers(max(lo, -5), min(hi, 5) + 1, n)
    elif kind == "const":
        v = np.full(n, min(hi, 42))
    else:
        v = rng.integers(lo, hi, n, dtype=np.int64 if signed or width < 8 else np.uint64, endpoint=True)
    return np.asarray(v).astype(dt)


def decode_int(dec, buf, lens, rows, ttype, nullable_col, nullable_target=True):
    ch = NativeColumnChunk(buf, lens, rows, nullable_col)
    c = dec.decode_native(ch, col.DataType(ttype, nullable=nullable_target)).to_host()
    valid = c.validity if c.validity is not None else np.ones(len(c.data), bool)
    return np.asarray(c.data), valid


def check_int(dec, v, width, signed, ttype, valid=None, nullable=False, **kw):
    buf, lens, rows = nat.write_column(v, "int", width, valid, nullable, **kw)
    ev, evalid = nat.read_column(buf, lens, rows, "int", width, signed, nullable)
    got, gvalid = decode_int(dec, buf, lens, rows, ttype, nullable)
    assert len(got) == len(ev)
    bad = np.nonzero(got.view(ev.dtype) != ev)[0] if len(ev) else []
    assert len(bad) == 0, (ttype, kw, bad[:5], got[bad[:5]], ev[bad[:5]])
    assert (gvalid == evalid).all()
    return got


@pytest.mark.parametrize("codec", INT_CODECS)
def test_int_codecs(dec, codec):
    for ttype, width, signed in INT_TYPES:
        for nullable in (False, True):
            rng = np.random.default_rng(ttype * 31 + codec * 3 + nullable)
            n = 1000
            kind = "const" if codec == nat.ONE_VALUE else ("few" if codec == nat.DICT else
                                                            ("runs" if codec == nat.RLE else "uniform"))
            v = _vals(rng, n, width, signed, kind)
            valid = rng.random(n) > 0.2 if nullable else None
            check_int(dec, v, width, signed, ttype, valid, nullable, page_rows=384, codecs=[codec])


@pytest.mark.parametrize("codec", [nat.BITPACK, nat.DELTA_BITPACK])
@pytest.mark.parametrize("ttype", [abi.UINT32, abi.INT32, abi.DATE])
def test_bitpacking(dec, codec, ttype):
    """every num_bits 0..32 (one block each), ragged last blocks, nullable."""
    rng = np.random.default_rng(codec + ttype)
    blocks = []
    for b in range(33):
        hi = (1 << b) - 1
        blocks.append(rng.integers(0, hi, 128, endpoint=True, dtype=np.uint64) if b else np.zeros(128, np.uint64))
    v = np.concatenate(blocks).astype(np.uint32)
    if codec == nat.DELTA_BITPACK:  # lossless for sorted values (delta_bp.rs); bits from the values
        v = np.sort(v)
    signed = ttype != abi.UINT32
    for n, page in [(len(v), 1024), (len(v) - 37, 1000), (300, 300)]:
        got = check_int(dec, v[:n], 4, signed, ttype, page_rows=page, codecs=[codec])
        assert (got.view(np.uint32) == v[:n]).all()
    valid = rng.random(len(v)) > 0.1
    check_int(dec, v, 4, signed, ttype, valid, True, page_rows=640, codecs=[codec])


@pytest.mark.parametrize("nested", [nat.NONE, nat.LZ4, nat.ZSTD, nat.SNAPPY, nat.RLE, nat.ONE_VALUE, nat.BITPACK,
                                    nat.DELTA_BITPACK])
def test_dict_nested_index_codecs(dec, nested):
    rng = np.random.default_rng(nested)
    for ttype, width, signed in [(abi.INT64, 8, True), (abi.UINT16, 2, False), (abi.INT32, 4, True)]:
        n = 2048
        if nested == nat.ONE_VALUE:
            v = np.full(n, 7, nat._dtype(width, signed))
        elif nested == nat.DELTA_BITPACK:  # sorted indices: first-seen order of a sorted column
            v = np.sort(_vals(rng, n, width, signed, "few"))
        else:
            v = _vals(rng, n, width, signed, "few")
        valid = rng.random(n) > 0.3
        valid[0] = valid[1024] = True  # a leading NULL would put 0 first in the dictionary (unsorted indices)
        for nullable in (False, True):
            check_int(dec, v, width, signed, ttype, valid if nullable else None, nullable, page_rows=1024, codecs=[nat.DICT],
                      nested=nested)


def test_mixed_codecs_across_pages(dec):
    rng = np.random.default_rng(11)
    n = 12 * 500 + 77
    v = _vals(rng, n, 4, True, "runs")
    codecs = [nat.NONE, nat.RLE, nat.DICT, nat.LZ4, nat.ONE_VALUE, nat.ZSTD, nat.BITPACK, nat.SNAPPY, nat.DELTA_BITPACK]
    w = v.copy()
    for k, c in enumerate(codecs * 2):  # per-page shapes each codec needs
        s = slice(500 * k, 500 * (k + 1))
        if c == nat.ONE_VALUE:
            w[s] = 9
        if c in (nat.BITPACK, nat.DELTA_BITPACK):
            w[s] = np.sort(np.abs(w[s]))
    valid = rng.random(n) > 0.25
    valid[::500] = True
    for nullable in (False, True):
        check_int(dec, w, 4, True, abi.INT32, valid if nullable else None, nullable, page_rows=500, codecs=codecs)


def test_writer_choice_pages(dec):
    """the restated writer's own codec choice (choose_compressor) on typical column shapes."""
    rng = np.random.default_rng(3)
    n = 2 * 8192 + 300  # the rule on 8192-row pages (the pure-Python writer is slow at 131072)
    cols = {
        "const": np.full(n, 5, np.int64),
        "low_card": rng.integers(0, 20, n).astype(np.int16),
        "runs": np.repeat(rng.integers(0, 1 << 20, n // 64 + 1), 64)[:n].astype(np.int32),
        "sorted_u32": np.sort(rng.integers(0, 1 << 30, n)).astype(np.uint32),
        "small_u32": rng.integers(0, 1000, n).astype(np.uint32),
    }
    tt = {np.dtype(np.int64): (abi.INT64, 8, True), np.dtype(np.int16): (abi.INT16, 2, True),
          np.dtype(np.int32): (abi.INT32, 4, True), np.dtype(np.uint32): (abi.UINT32, 4, False)}
    for name, v in cols.items():
        ttype, width, signed = tt[v.dtype]
        got = check_int(dec, v, width, signed, ttype, page_rows=8192)
        assert (got == v).all(), name


def test_full_size_pages_round_trip(dec):
    """131072-row pages at 2M rows (the oracle's reader is too slow here): the decode equals the
    values written — lossless codecs — and a second column shape, nullable, equals them on the
    valid rows."""
    rng = np.random.default_rng(21)
    n = 2_000_000
    v = rng.integers(-(1 << 40), 1 << 40, n)
    buf, lens, rows = nat.write_column(v, "int", 8, codecs=[nat.LZ4, nat.NONE, nat.ZSTD, nat.SNAPPY])
    got, gvalid = decode_int(dec, buf, lens, rows, abi.INT64, False)
    assert (got == v).all() and gvalid.all()
    d = np.sort(rng.integers(0, 1 << 31, n)).astype(np.uint32)
    valid = rng.random(n) > 0.01
    buf, lens, rows = nat.write_column(d, "int", 4, valid, True, codecs=[nat.NONE, nat.LZ4, nat.BITPACK])
    got, gvalid = decode_int(dec, buf, lens, rows, abi.UINT32, True)
    assert (gvalid == valid).all()
    assert (got[valid] == d[valid]).all()


def _strs(rng, n, kind):
    if kind == "few":
        pool = [b"", b"a", b"hello", b"x" * 40, bytes(range(200))]
        return [pool[i] for i in rng.integers(0, len(pool), n)]
    if kind == "const":
        return [b"databend"] * n
    return [bytes(rng.integers(0, 256, int(rng.integers(0, 60)), dtype=np.uint8)) for _ in range(n)]


def check_str(dec, v, valid=None, nullable=False, **kw):
    buf, lens, rows = nat.write_column(v, "str", 0, valid, nullable, **kw)
    ev, evalid = nat.read_column(buf, lens, rows, "str", 0, True, nullable)
    c = dec.decode_native(NativeColumnChunk(buf, lens, rows, nullable), col.DataType(abi.STRING, nullable=True)).to_host()
    offs = c.offsets
    got = [bytes(c.data[int(offs[i]):int(offs[i + 1])]) for i in range(len(ev))]
    assert len(offs) == len(ev) + 1
    assert got == ev
    gvalid = c.validity if c.validity is not None else np.ones(len(ev), bool)
    assert (gvalid == evalid).all()


@pytest.mark.parametrize("codec", [nat.NONE, nat.LZ4, nat.ZSTD, nat.SNAPPY, nat.ONE_VALUE, nat.DICT])
def test_string_codecs(dec, codec):
    rng = np.random.default_rng(40 + codec)
    n = 1500
    kind = "const" if codec == nat.ONE_VALUE else ("few" if codec == nat.DICT else "random")
    v = _strs(rng, n, kind)
    for nullable in (False, True):
        valid = rng.random(n) > 0.2 if nullable else None
        check_str(dec, v, valid, nullable, page_rows=512, codecs=[codec])


@pytest.mark.parametrize("nested", [nat.RLE, nat.BITPACK, nat.LZ4])
def test_string_dict_nested(dec, nested):
    rng = np.random.default_rng(nested)
    v = _strs(rng, 4096, "few")
    check_str(dec, v, page_rows=2048, codecs=[nat.DICT], nested=nested)


@pytest.mark.parametrize("codec", [nat.LZ4, nat.SNAPPY, nat.ZSTD])
def test_long_back_references(dec, codec):
    """a 40000-byte value repeated: the compressors emit one match of ~120 KB at offset 40000 —
    longer than the offset, which is more than the inflate's 32 KiB history ring (LZ4 / Snappy) and
    more than the Zstd ring: both read it from the output."""
    rng = np.random.default_rng(8)
    x = bytes(rng.integers(0, 256, 40000, dtype=np.uint8))
    check_str(dec, [x, x, x, x, b"tail"], codecs=[codec])


def test_zstd_ring_segments_and_far_overlap(dec):
    """The native launch site of the Zstd kernel on both match paths: a String payload of zero
    bytes and a period of 3 (ring matches of several 16 KiB segments) and a 10 000-byte value six
    times (one overlapping match read from the output), as the frame walker classifies what the
    writer's libzstd emits for it."""
    import struct
    from collections import Counter

    from tests import zstd_frames as zf
    x = bytes(np.random.default_rng(9).integers(0, 256, 10_000, dtype=np.uint8))
    v = [bytes(100_000), b"abc" * 30_000, x * 6, b"tail"]
    buf, _, _ = nat.write_column(v, "str", 0, None, False, codecs=[nat.ZSTD])
    feats, at = Counter(), buf.find(b"\x28\xb5\x2f\xfd")
    while at >= 0:
        codec, ln, _ = struct.unpack_from("<BII", buf, at - 9)
        assert codec == nat.ZSTD
        feats.update(zf.inspect(buf[at:at + ln])[0])
        at = buf.find(b"\x28\xb5\x2f\xfd", at + ln)
    assert feats["ring_multiseg"] and feats["far_overlap"] and feats["off_1"] and feats["off_3"], feats
    check_str(dec, v, codecs=[nat.ZSTD])


def test_string_dict_expands_payload(dec):
    """a dictionary whose rows reference a long entry many times: the payload is far larger
    than the page bytes, so the first call reports the size and the wrapper repeats it."""
    v = [b"y" * 3000 if i % 2 else b"" for i in range(4000)]
    check_str(dec, v, page_rows=4000, codecs=[nat.DICT])


def test_empty_and_tiny(dec):
    for n in (0, 1, 127, 128, 129):
        v = np.arange(n, dtype=np.int32)
        if n:
            check_int(dec, v, 4, True, abi.INT32, codecs=[nat.NONE])
            check_int(dec, v, 4, True, abi.INT32, codecs=[nat.BITPACK])
            check_str(dec, [b"k%d" % i for i in range(n)], codecs=[nat.LZ4])
    c = dec.decode_native(NativeColumnChunk(b"", [], [], False), col.Int64)
    assert c.length == 0


def test_pipeline_native_to_group_by(dec):
    """native pages of a C2-shaped table -> HBM columns -> GPU GROUP BY == oracle."""
    from databend_amd.aggregates import AggregateFunctionFactory
    from databend_amd.aggregator import AggregateHashTable, AggregatorParams, HashTableConfig
    from databend_amd.filter import FilterProgram, cmp
    from oracle import oracle
    from tests.parity import assert_results_equal
    rng = np.random.default_rng(5)
    n = 1_000_000
    adv = np.where(rng.random(n) < 0.99, 0, rng.integers(1, 33, n)).astype(np.int16)
    uid = rng.integers(0, 1000, n)
    a = nat.write_column(adv, "int", 2, codecs=[nat.RLE, nat.DICT, nat.LZ4])
    u = nat.write_column(uid, "int", 8, codecs=[nat.DICT, nat.ZSTD])
    chunks = {0: NativeColumnChunk(*a), 1: NativeColumnChunk(*u)}
    cols = deserialize_native_chunks(n, {0: col.Int16, 1: col.Int64}, chunks, dec)
    F = AggregateFunctionFactory.instance()
    fns = [F.get("count"), F.get("sum", [], [col.Int64])]
    ht = AggregateHashTable(AggregatorParams([col.Int16], fns), HashTableConfig(True))
    dadv, duid = cols[0], cols[1]
    ht.add_groups([dadv], [None, duid], rows=n, filter_program=FilterProgram(cmp(0, "<>", 0), [dadv.to_abi()]), on_device=True)
    block = ht.merge_result()
    ht.close()
    hadv, huid = col.Column.from_numbers(col.Int16, adv), col.Column.from_numbers(col.Int64, uid)
    specs = [(f.to_abi(), c) for f, c in zip(fns, [None, huid])]
    ok, oa = oracle.aggregate([hadv], specs, filter_program=FilterProgram(cmp(0, "<>", 0), [hadv.to_abi()]), threads=4)
    assert_results_equal(block.columns[2:], block.columns[:2], ok, oa)


def test_errors_not_faults(dec):
    rng = np.random.default_rng(9)
    v = _vals(rng, 2000, 4, True, "runs")
    good = nat.write_column(v, "int", 4, codecs=[nat.LZ4], page_rows=1000)
    T = col.Int32
    # truncated column: a page runs past the bytes
    with pytest.raises(DbgError):
        dec.decode_native(NativeColumnChunk(good[0][:-10], good[1], good[2]), T)
    # corrupt LZ4 payload (headers intact)
    bad = bytearray(good[0])
    for j in range(12, 60):
        bad[j] = 0xFF
    with pytest.raises(DbgError):
        dec.decode_native(NativeColumnChunk(bytes(bad), good[1], good[2]), T)
    # Rle runs covering fewer rows than the page
    r = nat.write_column(v, "int", 4, codecs=[nat.RLE], page_rows=2000)
    rb = bytearray(r[0])
    rb[9:13] = (1).to_bytes(4, "little")  # first run: count 1
    with pytest.raises(DbgError):
        dec.decode_native(NativeColumnChunk(bytes(rb), r[1], r[2]), T)
    # dictionary index out of range: shrink the entry count
    d = nat.write_column(_vals(rng, 1000, 4, True, "few"), "int", 4, codecs=[nat.DICT], page_rows=1000)
    db = bytearray(d[0])
    inner_comp = int.from_bytes(db[10:14], "little")
    cnt_at = 9 + 9 + inner_comp
    db[cnt_at:cnt_at + 4] = (1).to_bytes(4, "little")
    with pytest.raises(DbgError):
        dec.decode_native(NativeColumnChunk(bytes(db), d[1], d[2]), T)
    # Freq pages and float targets stay on the CPU reader
    fb = bytearray(good[0])
    fb[0] = nat.FREQ
    with pytest.raises(Unsupported):
        dec.decode_native(NativeColumnChunk(bytes(fb), good[1], good[2]), T)
    with pytest.raises(Unsupported):
        dec.decode_native(NativeColumnChunk(*good), col.DataType(abi.DATE + 100))
    # Bitpacking is not a Float codec
    bp = nat.write_column(np.arange(256, dtype=np.int32), "int", 4, codecs=[nat.BITPACK])
    with pytest.raises(DbgError):
        dec.decode_native(NativeColumnChunk(*bp), col.DataType(abi.FLOAT32))
    # a NULL in a non-nullable target
    valid = np.ones(2000, bool)
    valid[1234] = False
    nb = nat.write_column(v, "int", 4, valid, True, codecs=[nat.NONE], page_rows=1000)
    with pytest.raises(DbgError):
        dec.decode_native(NativeColumnChunk(*nb, nullable=True), T)
    got, gvalid = decode_int(dec, *nb, abi.INT32, True)
    assert (gvalid == valid).all()
    # the context still decodes after every error
    check_int(dec, v, 4, True, abi.INT32, codecs=[nat.LZ4], page_rows=1000)


@pytest.mark.parametrize("codec", [nat.NONE, nat.LZ4, nat.ZSTD, nat.SNAPPY, nat.RLE, nat.DICT, nat.ONE_VALUE])
def test_float_columns(dec, codec):
    """Float32 / Float64 pages: their bits in the integer layouts (compression/double/mod.rs)."""
    rng = np.random.default_rng(60 + codec)
    for ttype, width, fdt, idt in [(abi.FLOAT64, 8, np.float64, np.int64), (abi.FLOAT32, 4, np.float32, np.int32)]:
        n = 1500
        base = rng.standard_normal(n).astype(fdt)
        base[::97] = np.nan
        if codec in (nat.RLE, nat.DICT):
            base = np.repeat(base[:40], n // 40 + 1)[:n]
        if codec == nat.ONE_VALUE:
            base = np.full(n, -0.0, fdt)
        for nullable in (False, True):
            valid = rng.random(n) > 0.2 if nullable else None
            if valid is not None:
                valid[0] = True
            buf, lens, rows = nat.write_column(base.view(idt), "int", width, valid, nullable, page_rows=512, codecs=[codec])
            ev, evalid = nat.read_column(buf, lens, rows, "int", width, True, nullable)
            c = dec.decode_native(NativeColumnChunk(buf, lens, rows, nullable), col.DataType(ttype, nullable=True)).to_host()
            got = np.asarray(c.data).view(idt)
            assert (got == ev).all(), (ttype, codec, nullable)
            gvalid = c.validity if c.validity is not None else np.ones(n, bool)
            assert (gvalid == evalid).all()


@pytest.mark.parametrize("codec", [nat.NONE, nat.LZ4, nat.ZSTD, nat.SNAPPY, nat.RLE, nat.ONE_VALUE])
def test_bool_columns(dec, codec):
    """Boolean pages (compression/boolean/mod.rs): the bitmap under the basic codecs, Rle of
    [u32 count][u8 value], OneValue; ragged pages so page bitmaps start mid-byte in the output."""
    rng = np.random.default_rng(70 + codec)
    n = 3001
    v = np.repeat(rng.random(n // 11 + 1) < 0.5, 11)[:n] if codec == nat.RLE else (
        np.zeros(n, bool) if codec == nat.ONE_VALUE else rng.random(n) < 0.4)
    for nullable in (False, True):
        valid = rng.random(n) > 0.25 if nullable else None
        if valid is not None:
            valid[0] = True
        buf, lens, rows = nat.write_column(v, "bool", 0, valid, nullable, page_rows=1000, codecs=[codec])
        ev, evalid = nat.read_column(buf, lens, rows, "bool", 0, True, nullable)
        c = dec.decode_native(NativeColumnChunk(buf, lens, rows, nullable), col.DataType(abi.BOOLEAN, nullable=True)).to_host()
        got = np.asarray(c.data).astype(bool)
        assert (got == ev).all(), (codec, nullable, np.nonzero(got != ev)[0][:5])
        gvalid = c.validity if c.validity is not None else np.ones(n, bool)
        assert (gvalid == evalid).all()


@pytest.mark.parametrize("codec", [nat.NONE, nat.LZ4, nat.ZSTD, nat.SNAPPY, nat.RLE, nat.DICT, nat.ONE_VALUE])
def test_decimal128_columns(dec, codec):
    """Decimal128 pages: i128 values through the integer codecs (write/primitive.rs:67-70), decoded
    as two 8-byte halves at a 16-byte stride; Dict with Rle / Bitpacking nested indices too."""
    rng = np.random.default_rng(80 + codec)
    n = 2500
    lo = rng.integers(-(1 << 62), 1 << 62, n, dtype=np.int64)
    vals = np.zeros(n, nat._I128)
    vals["lo"] = lo.view(np.uint64)
    vals["hi"] = np.where(lo < 0, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0))
    if codec in (nat.RLE, nat.DICT):
        vals = np.repeat(vals[:60], n // 60 + 1)[:n]
    if codec == nat.ONE_VALUE:
        vals = np.repeat(vals[:1], n)
    for nullable in (False, True):
        for nested in ((nat.NONE, nat.RLE, nat.BITPACK) if codec == nat.DICT else (nat.NONE,)):
            valid = rng.random(n) > 0.2 if nullable else None
            if valid is not None:
                valid[0] = True
            buf, lens, rows = nat.write_column(vals, "int", 16, valid, nullable, page_rows=1000, codecs=[codec], nested=nested)
            ev, evalid = nat.read_column(buf, lens, rows, "int", 16, True, nullable)
            c = dec.decode_native(NativeColumnChunk(buf, lens, rows, nullable),
                                  col.DataType(abi.DECIMAL128, 38, 4, nullable=True)).to_host()
            got = np.frombuffer(np.asarray(c.data).tobytes()[:16 * n], nat._I128)
            assert (got == ev).all(), (codec, nested, nullable)
            gvalid = c.validity if c.validity is not None else np.ones(n, bool)
            assert (gvalid == evalid).all()
