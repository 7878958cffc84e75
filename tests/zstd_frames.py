"""Zstandard frames built to reach every path of the device decoder (databend_amd/csrc/zstd_dev.hpp,
zs_decode), shared by the CPU tests (tests/test_zstd_frames.py) and the GPU tests
(tests/test_gpu_zstd_frames.py).  Three parts:

  * inspect(frame): a frame walker restated from RFC 8878 (its own bit readers, FSE table reader and
    builder, Python integers) that decodes every sequence and classifies it the way zs_decode
    executes it: a match whose offset is <= 8192 reads the 16 KiB LDS ring (in more than one
    segment when longer than 16384 - off), a farther one reads the output.  It does not decode
    Huffman literals.
  * a frame assembler: raw / RLE blocks and compressed blocks with raw or RLE literals whose three
    sequence tables are all in RLE mode, so that every code and every extra bit is chosen exactly.
  * cases(): name, frame, expected bytes and the features the case claims; malformed(): frames
    aimed at one check of zs_decode each; page() / case_page(): a frame as a required INT64 data
    page.

The case table is the coverage contract of zs_decode: a case that stops producing a
feature it claims fails tests/test_zstd_frames.py."""
import functools
import struct
from collections import Counter, namedtuple

import numpy as np

RING = 16384        # ZS_RING: bytes of output history in LDS
SPLIT = RING // 2   # offsets up to this read the ring, longer ones the output
LANES = 64
BATCH = 256         # ZS_SEQ: sequences decoded per batch
MAX_BLOCK = 128 * 1024
MAGIC = 0xFD2FB528
SKIP_MAGIC = 0x184D2A50

# ---- RFC 8878 section 3.1.1.3.2.1.1: codes -> (baseline, extra bits), generated from the rule ----


def _codes(direct, first, bits):
    base, nb = [first + c for c in range(direct)], [0] * direct
    v = first + direct
    for b in bits:
        base.append(v)
        nb.append(b)
        v += 1 << b
    return base, nb


LL_BASE, LL_BITS = _codes(16, 0, [1, 1, 1, 1, 2, 2, 3, 3, 4, 6] + list(range(7, 17)))
ML_BASE, ML_BITS = _codes(32, 3, [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5] + list(range(7, 17)))
assert len(LL_BASE) == 36 and LL_BASE[-1] == 65536 and len(ML_BASE) == 53 and ML_BASE[-1] == 65539

# section 3.1.1.3.2.2: the predefined distributions
LL_DEFAULT = [4, 3] + [2] * 11 + [1, 1, 1] + [2] * 9 + [3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
ML_DEFAULT = [1, 4, 3] + [2] * 6 + [1] * 37 + [-1] * 7
OF_DEFAULT = [1] * 6 + [2, 2, 2] + [1] * 15 + [-1] * 5
assert (len(LL_DEFAULT), sum(map(abs, LL_DEFAULT))) == (36, 64)
assert (len(ML_DEFAULT), sum(map(abs, ML_DEFAULT))) == (53, 64)
assert (len(OF_DEFAULT), sum(map(abs, OF_DEFAULT))) == (29, 32)

# offsets, literal lengths and sequence counts that get a feature of their own
EDGE_OFFS = {1, 2, 3, 7, 31, 32, 33, 61, 62, 63, 64, 65, 66, 67, 8191, 8192, 8193, 16383, 16384, 16385}
EDGE_LLS = {63, 64, 65, 127}
EDGE_NSEQ = {127, 128, 255, 256, 257, 512, 513}


# ---- the walker ------------------------------------------------------------------------------------
class _Forward:
    """Little-endian bit reader from the first byte on (FSE table descriptions)."""

    def __init__(self, data):
        self.v = int.from_bytes(data, "little")
        self.n = 8 * len(data)
        self.pos = 0

    def read(self, k):
        r = (self.v >> self.pos) & ((1 << k) - 1)
        self.pos += k
        return r


class _Backward:
    """RFC 8878 section 4.1: read from the last byte down; the highest set bit of the last byte is the
    end marker.  Bits asked for below the first byte read as zeros (pos goes negative)."""

    def __init__(self, data):
        assert len(data) and data[-1], "bitstream: empty or no end marker"
        self.d = bytes(data)
        self.pos = 8 * (len(data) - 1) + data[-1].bit_length() - 1

    def read(self, k):
        if not k:
            return 0
        self.pos -= k
        p = self.pos
        if p >= 0:
            return (int.from_bytes(self.d[p >> 3:(p + k + 7) >> 3], "little") >> (p & 7)) & ((1 << k) - 1)
        have = p + k
        if have <= 0:
            return 0
        return (int.from_bytes(self.d[:(have + 7) >> 3], "little") & ((1 << have) - 1)) << -p


def _read_fse_description(data, max_symbols, max_log):
    """Section 4.1.1: the probabilities, the accuracy log and the bytes used."""
    r = _Forward(data)
    al = r.read(4) + 5
    assert al <= max_log, "fse: accuracy log"
    left = 1 << al
    probs = []
    while left > 0 and len(probs) < max_symbols:
        bits = (left + 1).bit_length()
        v = r.read(bits)
        low_mask = (1 << (bits - 1)) - 1
        small = (1 << bits) - 1 - (left + 1)
        if (v & low_mask) < small:
            r.pos -= 1
            v &= low_mask
        elif v > low_mask:
            v -= small
        p = v - 1
        left -= abs(p)
        probs.append(p)
        if p == 0:
            while True:
                rep = r.read(2)
                probs += [0] * rep
                if rep != 3:
                    break
    assert left == 0 and len(probs) <= max_symbols and r.pos <= r.n, "fse: description"
    return probs, al, (r.pos + 7) >> 3


def _build_fse(probs, al):
    """Section 4.1.1: states -> (symbol, bits to read, baseline)."""
    size = 1 << al
    sym_of = [None] * size
    high = size
    for s, p in enumerate(probs):
        if p == -1:
            high -= 1
            sym_of[high] = s
    pos = 0
    for s, p in enumerate(probs):
        for _ in range(max(p, 0)):
            sym_of[pos] = s
            pos = (pos + (size >> 1) + (size >> 3) + 3) % size
            while pos >= high:
                pos = (pos + (size >> 1) + (size >> 3) + 3) % size
    assert pos == 0 and None not in sym_of, "fse: spread"
    seen = [abs(p) for p in probs]
    table = []
    for s in sym_of:
        x = seen[s]
        seen[s] += 1
        nb = al - (x.bit_length() - 1)
        table.append((s, nb, (x << nb) - size))
    return table


_TABLES = (("ll", 6, 35, 9, LL_DEFAULT, 6), ("of", 4, 31, 8, OF_DEFAULT, 5), ("ml", 2, 52, 9, ML_DEFAULT, 6))


def _classify(f, mx, ll, ml, off):
    mx["ll"], mx["ml"], mx["off"] = max(mx["ll"], ll), max(mx["ml"], ml), max(mx["off"], off)
    if ll in EDGE_LLS:
        f["ll_%d" % ll] += 1
    if off in EDGE_OFFS:
        f["off_%d" % off] += 1
    if off <= SPLIT:
        f["ring"] += 1
        room = RING - off
        mx["segments"] = max(mx["segments"], -(-ml // room))
        if ml > room:
            f["ring_multiseg"] += 1
        if ml in (room - 1, room, room + 1):
            f["ring_seg_" + {room - 1: "minus1", room: "exact", room + 1: "plus1"}[ml]] += 1
        if ml > off:
            f["ring_overlap"] += 1
        f["ring_off_lt64" if off < LANES else ("ring_off_eq64" if off == LANES else "ring_off_gt64")] += 1
    else:
        f["far"] += 1
        if off > RING:
            f["far_gt_ring"] += 1
        if off > MAX_BLOCK:
            f["far_gt_block"] += 1
        if ml > off:
            f["far_overlap"] += 1


def _walk_compressed(b, f, mx, st):
    """One compressed block's content; returns the bytes it regenerates."""
    lt, sf = b[0] & 3, (b[0] >> 2) & 3
    if lt < 2:
        hl = (1, 2, 1, 3)[sf]
        h = int.from_bytes(b[:hl], "little")
        regen = h >> (3 if hl == 1 else 4)
        q = hl + (regen if lt == 0 else 1)
        f["lit_raw" if lt == 0 else "lit_rle"] += 1
    else:
        hl, fb = ((3, 10), (3, 10), (4, 14), (5, 18))[sf]
        h = int.from_bytes(b[:hl], "little")
        regen, csize = (h >> 4) & ((1 << fb) - 1), (h >> (4 + fb)) & ((1 << fb) - 1)
        f["huf_1stream" if sf == 0 else "huf_4stream"] += 1
        if lt == 2:
            f["lit_huf"] += 1
            f["huf_direct" if b[hl] >= 128 else "huf_fse"] += 1
            st["huf"] = True
        else:
            assert st.get("huf"), "treeless literals without a previous tree"
            f["lit_treeless"] += 1
        q = hl + csize
    assert q <= len(b) and regen <= MAX_BLOCK, "literals section"
    mx["regen"] = max(mx["regen"], regen)
    c0 = b[q]
    if c0 < 128:
        nseq, q, form = c0, q + 1, 1
    elif c0 < 255:
        nseq, q, form = ((c0 - 128) << 8) + b[q + 1], q + 2, 2
    else:
        nseq, q, form = b[q + 1] + (b[q + 2] << 8) + 0x7F00, q + 3, 3
    mx["nseq"] = max(mx["nseq"], nseq)
    if nseq == 0:
        assert q == len(b), "bytes after an empty sequences section"
        f["nseq0"] += 1
        if regen:
            f["tail_literals"] += 1
        return regen
    f["nseq_%dbyte" % form] += 1
    if nseq in EDGE_NSEQ:
        f["nseq_%d" % nseq] += 1
    if nseq > BATCH:
        f["multi_batch"] += 1
    modes = b[q]
    q += 1
    assert modes & 3 == 0, "sequence modes: reserved bits"
    tabs = {}
    for name, shift, max_sym, max_log, default, default_log in _TABLES:
        m = (modes >> shift) & 3
        if m == 0:
            t = _build_fse(default, default_log)
        elif m == 1:
            assert b[q] <= max_sym
            t = [(b[q], 0, 0)]
            q += 1
        elif m == 2:
            probs, al, used = _read_fse_description(b[q:q + 512], max_sym + 1, max_log)
            q += used
            t = _build_fse(probs, al)
        else:
            assert name in st, "repeat mode without a previous table"
            t = st[name]
        f["%s_%s" % (name, ("predef", "rle", "fse", "repeat")[m])] += 1
        st[name] = tabs[name] = t
    bs = _Backward(b[q:])
    tl, to, tm = tabs["ll"], tabs["of"], tabs["ml"]
    sl = bs.read(len(tl).bit_length() - 1)
    so = bs.read(len(to).bit_length() - 1)
    sm = bs.read(len(tm).bit_length() - 1)
    rep = st["rep"]
    used = out = 0
    for i in range(nseq):
        llc, ofc, mlc = tl[sl][0], to[so][0], tm[sm][0]
        ofv = (1 << ofc) + bs.read(ofc)
        ml = ML_BASE[mlc] + bs.read(ML_BITS[mlc])
        ll = LL_BASE[llc] + bs.read(LL_BITS[llc])
        if ofv > 3:
            off = ofv - 3
            rep[:] = [off, rep[0], rep[1]]
        else:
            idx = ofv + (ll == 0)
            f["rep%d%s" % (idx, "_ll0" if ll == 0 else "")] += 1
            if idx == 1:
                off = rep[0]
            elif idx == 2:
                off = rep[1]
                rep[:] = [off, rep[0], rep[2]]
            elif idx == 3:
                off = rep[2]
                rep[:] = [off, rep[0], rep[1]]
            else:
                off = rep[0] - 1
                assert off > 0, "repeat offset 1 minus one"
                rep[:] = [off, rep[0], rep[1]]
        if i + 1 < nseq:
            sl = tl[sl][2] + bs.read(tl[sl][1])
            sm = tm[sm][2] + bs.read(tm[sm][1])
            so = to[so][2] + bs.read(to[so][1])
        used += ll
        out += ll
        assert used <= regen, "literals consumed past the literals section"
        assert 0 < off <= st["out"] + out, "offset past the start of the frame"
        _classify(f, mx, ll, ml, off)
        out += ml
    assert bs.pos == 0, "sequence bitstream not consumed exactly (bit %d)" % bs.pos
    if regen > used:
        f["tail_literals"] += 1
    return out + regen - used


def inspect(frame):
    """(features, maxima, output length) of a sequence of zstd frames."""
    frame = bytes(frame)
    f = Counter()
    mx = dict(off=0, ml=0, ll=0, nseq=0, regen=0, segments=0, blocks=0, frames=0)
    p = total = 0
    while p < len(frame):
        magic, = struct.unpack_from("<I", frame, p)
        if magic & 0xFFFFFFF0 == SKIP_MAGIC:
            size, = struct.unpack_from("<I", frame, p + 4)
            p += 8 + size
            assert p <= len(frame)
            f["skippable"] += 1
            continue
        assert magic == MAGIC, "magic"
        fhd = frame[p + 4]
        p += 5
        assert not fhd & 8, "frame header: reserved bit"
        single = (fhd >> 5) & 1
        p += (0 if single else 1) + (0, 1, 2, 4)[fhd & 3]
        flen = ((1 if single else 0), 2, 4, 8)[fhd >> 6]
        declared = int.from_bytes(frame[p:p + flen], "little") + (256 if flen == 2 else 0) if flen else None
        p += flen
        st = {"rep": [1, 4, 8], "out": 0}
        nblocks = 0
        while True:
            bh = int.from_bytes(frame[p:p + 3], "little")
            p += 3
            btype, bsize = (bh >> 1) & 3, bh >> 3
            nblocks += 1
            if btype == 0:
                f["block_raw"] += 1
                p += bsize
                st["out"] += bsize
            elif btype == 1:
                f["block_rle"] += 1
                p += 1
                st["out"] += bsize
            else:
                assert btype == 2 and bsize <= MAX_BLOCK, "block type / size"
                f["block_compressed"] += 1
                st["out"] += _walk_compressed(frame[p:p + bsize], f, mx, st)
                p += bsize
            assert p <= len(frame), "block past the frame"
            if bh & 1:
                break
        if fhd & 4:
            p += 4
            assert p <= len(frame)
            f["checksum"] += 1
        assert declared is None or declared == st["out"], "output length %d, declared %d" % (st["out"], declared)
        if st["out"] == 0:
            f["empty_frame"] += 1
        f["frame"] += 1
        mx["blocks"] = max(mx["blocks"], nblocks)
        total += st["out"]
    mx["frames"] = f["frame"]
    return f, mx, total


# ---- the assembler ---------------------------------------------------------------------------------
Block = namedtuple("Block", "btype size payload out")  # size: the header's Block_Size; out: bytes produced


def frame_header(size, checksum=False, fhd_or=0):
    """Single segment, 4-byte content size."""
    return struct.pack("<IBI", MAGIC, 0xA0 | (4 if checksum else 0) | fhd_or, size)


def skippable(payload, nibble=0):
    return struct.pack("<II", SKIP_MAGIC | nibble, len(payload)) + payload


def raw_block(data):
    return Block(0, len(data), bytes(data), len(data))


def rle_block(byte, n):
    return Block(1, n, bytes([byte]), n)


def literals_header(kind, regen):
    """kind 0 raw, 1 RLE; the shortest size format that holds regen."""
    if regen < 32:
        return bytes([regen << 3 | kind])
    if regen < 4096:
        return struct.pack("<H", regen << 4 | 1 << 2 | kind)
    return (regen << 4 | 3 << 2 | kind).to_bytes(3, "little")


def nseq_header(n):
    if n < 128:
        return bytes([n])
    if n < 0x7F00:
        return bytes([(n >> 8) + 128, n & 255])
    return b"\xff" + struct.pack("<H", n - 0x7F00)


def _code_of(v, base):
    c = max(k for k, b0 in enumerate(base) if b0 <= v)
    return c, v - base[c]


def new(off):
    """The offset value of a new offset (values 1-3 are the repeat codes)."""
    return off + 3


def sequence_section(seqs):
    """seqs: (ll, ml, offset value) that share one code each; all three tables in RLE mode (modes
    0x54): states take no bits, the stream is each sequence's extra bits — offset, match length,
    literal length — the first sequence highest, under a 1-bit end marker."""
    acc, total, codes = 0, 0, None
    for ll, ml, ofv in seqs:
        llc, lx = _code_of(ll, LL_BASE)
        mlc, mx_ = _code_of(ml, ML_BASE)
        ofc = ofv.bit_length() - 1
        assert codes in (None, (llc, ofc, mlc)), "one block, one code per table: %r then %r" % (codes, (llc, ofc, mlc))
        codes = (llc, ofc, mlc)
        for v, nb in ((ofv - (1 << ofc), ofc), (mx_, ML_BITS[mlc]), (lx, LL_BITS[llc])):
            assert 0 <= v < 1 << nb or (nb == 0 and v == 0)
            acc = acc << nb | v
            total += nb
    acc |= 1 << total
    return nseq_header(len(seqs)) + bytes([0x54, *codes]) + acc.to_bytes(total // 8 + 1, "little")


def compressed_block(lits, seqs):
    """lits: bytes (raw literals) or (byte, count) (RLE literals)."""
    if isinstance(lits, tuple):
        regen, body = lits[1], literals_header(1, lits[1]) + bytes([lits[0]])
    else:
        regen, body = len(lits), literals_header(0, len(lits)) + bytes(lits)
    assert sum(s[0] for s in seqs) <= regen
    body += sequence_section(seqs) if seqs else b"\x00"
    assert len(body) <= MAX_BLOCK
    return Block(2, len(body), body, regen + sum(s[1] for s in seqs))


def frame(blocks, checksum=None, size=None, fhd_or=0):
    out = [frame_header(sum(b.out for b in blocks) if size is None else size, checksum is not None, fhd_or)]
    for k, b in enumerate(blocks):
        out.append((b.size << 3 | b.btype << 1 | (k == len(blocks) - 1)).to_bytes(3, "little") + b.payload)
    return b"".join(out) + (checksum or b"")


def seq_blocks(rng, groups, rle=None):
    """One compressed block per group of sequences, with exactly the literals they take (random
    bytes, or `rle` repeated)."""
    blocks = []
    for g in groups:
        n = sum(s[0] for s in g)
        blocks.append(compressed_block((rle, n) if rle is not None else rng.integers(0, 256, n, dtype=np.uint8).tobytes(), g))
    return blocks


def history(rng, n):
    return raw_block(rng.integers(0, 256, n, dtype=np.uint8).tobytes())


# ---- the case table --------------------------------------------------------------------------------
Case = namedtuple("Case", "name frame expected claims libzstd")  # libzstd: pa.decompress takes it


def _libzstd(fr, n):
    import pyarrow as pa
    return pa.decompress(fr, decompressed_size=n, codec="zstd", asbytes=True)


def _compressed_cases():
    import pyarrow as pa
    rng = np.random.default_rng(1)
    rb = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    words = [b"alpha", b"beta", b"gamma", b"delta", b"epsilon", b"zeta"]
    text = b" ".join(words[i] for i in rng.integers(0, 6, 100_000))
    few = rng.integers(0, 4, 300_000, dtype=np.uint8).tobytes()
    zipf = (rng.zipf(1.3, 75_000) % 1000).astype(np.int32).tobytes()
    arange = np.arange(37_500, dtype=np.int64).tobytes()
    short = b" ".join(words[i] for i in np.random.default_rng(5).integers(0, 6, 45))[:236]
    r10, r40, r150, r100, rep10 = rb(10_000), rb(40_000), rb(150_000), rb(100), rb(10_000)
    mixed = rb(3000) + bytes(20_000) + rep10 * 3 + rb(500) + b"xyz" * 4000 + rep10 + bytes(9000) + rb(64)
    table = [
        ("far_10000x6", r10 * 6, 3, {"far", "far_overlap"}),
        ("far_40000x3", r40 * 3, 3, {"far", "far_gt_ring", "far_overlap"}),
        ("far_past_block", r150 + rb(1000) + r150[:50_000], 3, {"block_raw", "far_gt_block"}),
        ("zeros_300k", bytes(300_000), 3, {"block_rle", "ring_multiseg", "ring_off_lt64", "off_1"}),
        ("period_3", b"abc" * 30_000, 3, {"ring_multiseg", "off_3"}),
        ("period_100", r100 * 900, 3, {"ring_multiseg", "ring_off_gt64"}),
        ("text_l1", text, 1, {"huf_1stream", "lit_treeless"}),
        ("text_l3", text, 3, {"huf_4stream", "huf_fse", "ll_fse", "of_fse", "ml_fse"}),
        ("text_l9", text, 9, {"ml_repeat"}),
        ("text_l19", text, 19, {"ll_rle", "rep3_ll0"}),
        ("few_l1", few, 1, {"huf_direct", "lit_treeless"}),
        ("few_l19", few, 19, {"huf_direct", "lit_treeless", "ll_repeat", "of_repeat", "ml_repeat"}),
        ("zipf_l9", zipf, 9, {"lit_treeless", "ml_repeat", "far_gt_block"}),
        ("zipf_l19", zipf, 19, {"rep2", "rep3", "rep3_ll0"}),
        ("arange_l1", arange, 1, {"of_rle", "multi_batch"}),
        ("arange_l9", arange, 9, {"of_rle", "ll_repeat", "ml_repeat", "multi_batch"}),
        ("arange_l19", arange, 19, {"ll_rle", "ml_rle", "multi_batch"}),
        ("short_l3", short, 3, {"ll_predef", "of_predef", "ml_predef"}),
        ("short_l9", short, 9, {"ll_fse", "of_fse"}),
        ("short_l19", short, 19, {"ll_fse", "huf_1stream"}),
        ("random_5000", rb(5000), 3, {"block_raw"}),
        ("mixed", mixed, 3, {"ring", "far"}),
    ]
    return [Case(name, pa.Codec("zstd", compression_level=lvl).compress(d, asbytes=True), d, frozenset(cl), True)
            for name, d, lvl, cl in table]


def _assembled_frames():
    """(name, frame, claims): every frame here decodes with libzstd, which gives the expected bytes."""
    out = []
    rng = np.random.default_rng(2)

    def add(name, blocks, claims, **kw):
        out.append((name, frame(blocks, **kw) if isinstance(blocks, list) else blocks, set(claims)))

    # offsets at the ring / output split; match lengths around one ring segment (16384 - off)
    for off in (8191, 8192, 8193):
        room = RING - off
        groups = [[(5, 40, new(off))],
                  [(24, room - 1, new(off)), (25, room, new(off)), (26, room + 1, new(off))],  # code 48: 4099..8194
                  [(4, 16386, new(off))]]                                                    # code 49
        claims = {"off_%d" % off}
        claims |= {"ring", "ring_seg_minus1", "ring_seg_exact", "ring_seg_plus1", "ring_multiseg", "ring_overlap"} if off <= SPLIT \
            else {"far", "far_overlap"}
        add("split_%d" % off, [history(rng, 9000)] + seq_blocks(rng, groups), claims)
    # offsets at the ring's size, matches shorter and longer than the offset
    for off in (16383, 16384, 16385):
        groups = [[(7, 100, new(off))], [(3, 20_000, new(off))]]
        add("ring_edge_%d" % off, [history(rng, 17_000)] + seq_blocks(rng, groups),
            {"off_%d" % off, "far", "far_overlap"} | ({"far_gt_ring"} if off > RING else set()))
    # offsets around the lane count: 64 + ll fresh random literals before every match, so no match
    # reads a stretch that an earlier one made periodic
    for name, offs in (("lanes_61_67", range(61, 68)), ("lanes_small", (1, 2, 3, 7, 31, 32, 33))):
        groups = []
        for off in offs:
            for k, ml in enumerate((3, 63, 64, 65, 200, RING - off + 1, RING + 70)):
                groups.append([(70 + k + off % 5, ml, new(off))])
        claims = {"off_%d" % o for o in offs} | {"ring_multiseg", "ring_overlap", "ring_seg_plus1"}
        claims |= {"ring_off_lt64", "ring_off_eq64", "ring_off_gt64"} if 64 in offs else {"ring_off_lt64"}
        add(name, [history(rng, 300)] + seq_blocks(rng, groups), claims)
    # literal runs around the lane count, raw and RLE literals
    for name, rle in (("litrun_raw", None), ("litrun_rle", 0xC3)):
        groups = [[(63, 5, new(37))], [(64, 6, new(200)), (65, 6, new(130)), (127, 6, new(250))]]
        add(name, [history(rng, 500)] + seq_blocks(rng, groups, rle),
            {"ll_63", "ll_64", "ll_65", "ll_127", "lit_rle" if rle else "lit_raw"})
    # sequence counts at the batch edge; every sequence its own offset and literal
    for n in sorted(EDGE_NSEQ):
        g = [(1, 4, new(61 + (i * 7) % 64)) for i in range(n)]
        add("batch_%d" % n, [history(rng, 200)] + seq_blocks(rng, [g]),
            {"nseq_%d" % n, "nseq_1byte" if n < 128 else "nseq_2byte"} | ({"multi_batch"} if n > BATCH else set()))
    g = [(0, 3, new(1 + (i * i + i // 3) % 4)) for i in range(33_000)]
    add("batch_33000", [history(rng, 64)] + seq_blocks(rng, [g]), {"nseq_3byte", "multi_batch", "off_1", "off_2", "off_3"})
    # repeat offsets: every index, with and without ll == 0, between new offsets so the history
    # rotates (no index 4 while the first repeat offset is 1: libzstd calls that corrupt)
    groups = [[(64, 51, new(70)), (65, 52, new(90)), (66, 53, new(110))],
              [(64, 54, 1), (70, 55, 1)],           # index 1
              [(66, 56, 2), (67, 57, 3)],           # indices 2 and 3
              [(0, 51, 2), (0, 52, 3)],             # ll == 0: indices 3 and 4
              [(0, 53, 1)],                         # ll == 0: index 2
              [(64, 54, new(300)), (65, 55, new(400))],
              [(68, 56, 3), (69, 57, 2)],
              [(0, 51, 3), (0, 52, 2), (0, 53, 3)],
              [(71, 58, 1)]]
    add("repeat_offsets", [history(rng, 600)] + seq_blocks(rng, groups),
        {"rep1", "rep2", "rep3", "rep2_ll0", "rep3_ll0", "rep4_ll0"})
    # blocks without sequences
    add("nseq0_raw", [history(rng, 100), compressed_block(rng.integers(0, 256, 777, dtype=np.uint8).tobytes(), []),
                      compressed_block(b"", [])], {"nseq0", "lit_raw", "tail_literals"})
    add("nseq0_rle_70000", [history(rng, 100), compressed_block((0x5A, 70_000), []), history(rng, 60)], {"nseq0", "lit_rle"})
    # raw and RLE blocks between compressed ones
    add("raw_rle_blocks", [history(rng, 1000), rle_block(0x11, 20_000), compressed_block(b"q" * 9, [(9, 9000, new(19_000))]),
                           rle_block(0xEE, 3), history(rng, 5)], {"block_raw", "block_rle", "far", "far_gt_ring"})
    # framing
    small = lambda: frame([history(rng, 300)] + seq_blocks(rng, [[(3, 30, new(100))]]))  # noqa: E731
    empty = frame([raw_block(b"")])
    add("frames_two", small() + small(), {"frame"})
    add("frames_skippable", skippable(b"") + small() + skippable(b"between", 7) + small() + skippable(bytes(300), 15), {"skippable"})
    add("frames_empty", empty + small() + empty, {"empty_frame"})
    blocks = [history(rng, 300)] + seq_blocks(rng, [[(3, 30, new(100))]])
    add("checksum_off", blocks, {"frame"})
    add("checksum_on", blocks, {"checksum"}, checksum=b"\xde\xad\xbe\xef")
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = _compressed_cases()
    twin = None
    for name, fr, claims in _assembled_frames():
        if name == "checksum_on":  # libzstd would verify the four bytes; the device skips them
            out.append(Case(name, fr, twin, frozenset(claims), False))
            continue
        _, _, n = inspect(fr)
        exp = _libzstd(fr, n)
        if name == "checksum_off":
            twin = exp
        out.append(Case(name, fr, exp, frozenset(claims), True))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


# ---- malformed frames: each aimed at one check of zs_decode ----------------------------------------
Malformed = namedtuple("Malformed", "name frame size")  # size: the output size the decoder is given


def _tamper_block(fr, at, f):
    """Rewrite the content of the block whose header is at byte `at` with f(content)."""
    bh = int.from_bytes(fr[at:at + 3], "little")
    size = bh >> 3
    body = f(fr[at + 3:at + 3 + size])
    return fr[:at] + ((len(body) << 3) | (bh & 7)).to_bytes(3, "little") + body + fr[at + 3 + size:]


@functools.lru_cache(maxsize=None)
def malformed():
    rng = np.random.default_rng(3)
    lits = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    hist = history(rng, 96)
    hdr = 9  # frame header bytes
    out = []

    def add(name, fr, size):
        out.append(Malformed(name, bytes(fr), size))

    # 96 bytes of history and 8 literals are produced when the match starts: op == 104
    add("offset_past_output", frame([hist, compressed_block(lits(8), [(8, 696, new(105))])]), 800)
    # the match runs one byte past the output size
    add("match_past_size", frame([hist, compressed_block(lits(8), [(8, 697, new(50))])]), 800)
    # the literal length is one more than the literals section holds
    good = frame([hist, compressed_block(lits(16), [(16, 688, new(50))])])
    one = compressed_block(lits(17), [(17, 687, new(50))]).payload
    add("literals_past_section", frame([hist, Block(2, len(one) - 1, literals_header(0, 16) + one[1:17] + one[18:], 800 - 96)]), 800)
    # the literals section's size is one more than the bytes left in the block
    add("regen_past_block", frame([hist, Block(2, 1 + 19, literals_header(0, 20) + lits(19), 704)], size=800), 800)
    first = hdr + 3 + 96  # the second block's header
    add("repeat_table_first_block", _tamper_block(good, first, lambda b: b[:18] + b"\xfc" + b[22:]), 800)
    # treeless literals (type 3, one stream, regen 16, 4 compressed bytes) in a frame's first block
    tl = (3 | 0 << 2 | 16 << 4 | 4 << 14).to_bytes(3, "little") + b"\x01\x02\x03\x81" + b"\x00"
    add("treeless_first_block", frame([Block(2, len(tl), tl, 16)]), 16)
    add("modes_reserved_bits", _tamper_block(good, first, lambda b: b[:18] + b"\x55" + b[19:]), 800)
    add("nseq_truncated", _tamper_block(good, first, lambda b: b[:17] + b"\x80"), 800)
    add("nseq_truncated_3byte", _tamper_block(good, first, lambda b: b[:17] + b"\xff\x01"), 800)
    # one byte too many under the sequence bits: the stream does not end at bit 0
    add("bitstream_extra_byte", _tamper_block(good, first, lambda b: b[:22] + b"\x00" + b[22:]), 800)
    add("bitstream_zero_last_byte", _tamper_block(good, first, lambda b: b + b"\x00"), 800)
    add("block_past_frame", good[:first] + ((int.from_bytes(good[first:first + 3], "little") + 8).to_bytes(3, "little")) + good[first + 3:], 800)
    add("frame_reserved_bit", frame([hist, compressed_block(lits(16), [(16, 688, new(50))])], fhd_or=8), 800)
    # the decoder is told a size one more / one less than the frame produces
    add("size_one_more", frame([hist, compressed_block(lits(16), [(16, 687, new(50))])]), 800)
    add("size_one_less", frame([compressed_block(lits(16), [(16, 688, new(9))]), hist, raw_block(b"!")]), 800)
    return tuple(out)


# ---- a frame as a required INT64 Parquet data page -------------------------------------------------
def _zigzag_varint(v):
    v = (v << 1) ^ (v >> 63)
    out = bytearray()
    while v >= 0x80:
        out.append(v & 0x7F | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def page(fr, uncompressed):
    """Thrift compact PageHeader of a v1 data page — type DATA_PAGE, the two sizes, then
    DataPageHeader {num_values, PLAIN, RLE, RLE} — and the frame as its payload: `uncompressed`
    bytes of PLAIN INT64 values of a required column (no levels)."""
    assert uncompressed % 8 == 0
    i32 = lambda delta, v: bytes([delta << 4 | 5]) + _zigzag_varint(v)  # noqa: E731
    dph = i32(1, uncompressed // 8) + i32(1, 0) + i32(1, 3) + i32(1, 3) + b"\x00"
    return i32(1, 0) + i32(1, uncompressed) + i32(1, len(fr)) + bytes([2 << 4 | 12]) + dph + b"\x00" + fr


def pad8(c):
    """The case as a whole number of INT64 values: (frames, expected), a raw-block frame of zero
    bytes appended where the case's output is no multiple of 8."""
    k = -len(c.expected) % 8
    if not k:
        return c.frame, c.expected
    return c.frame + frame([raw_block(bytes(k))]), c.expected + bytes(k)


def case_page(c):
    """(page bytes, the bytes its values hold) of one case."""
    fr, exp = pad8(c)
    return page(fr, len(exp)), exp
