"""Parquet pages built by hand to reach every path of the device page decode
(databend_amd/csrc/scan.hip): pq_inflate_kernel (Snappy and LZ4 block decode, one wave per page) and
hybrid_expand (the RLE / bit-packed hybrid of definition levels, dictionary indices and RLE
booleans), plus put_value's FIXED_LEN_BYTE_ARRAY arm.  Shared by the CPU tests
(tests/test_pq_pages.py) and the GPU tests (tests/test_gpu_pq_pages.py); plain Python and numpy, no
Parquet writer.  Four parts:

  * a Thrift compact writer for the DATA_PAGE, DATA_PAGE_V2 and DICTIONARY_PAGE headers and page
    builders over it;
  * assemblers: snappy(elements), lz4(sequences) and hybrid(runs, bit width).  Each emits exactly
    the elements it is given (length forms, tag kinds, 255-chains, padded varints) and computes the
    expected output by executing them;
  * walkers: walk_snappy, walk_lz4, walk_hybrid and walk_chunk read the *bytes* back (their own tag,
    varint and Thrift readers; nothing of oracle/ is imported) and classify every element the way
    the kernel executes it: tag kind, length form and chain length, the offset's class against the
    lane count (64), the output produced so far (w) and the 32 KiB LDS ring, overlap (len > off),
    a ring copy in more than one segment (len > RING - off), a literal longer than the LDS input
    window; for the hybrid the runs per stream against the run table's 512, run kinds, bit width,
    RLE value bytes, overshoot of the value count, a truncated tail and padded headers;
  * cases(): name, pages, expected values and the features the case claims; malformed(): pages
    aimed at one check each, every one a single edit away from a page that decodes.

The window sweep.  pq_inflate_kernel parses the compressed stream from an LDS window of IWIN = 8176
bytes that starts at a 16-byte aligned address: with sa = (payload address) mod 16, the first
window holds stream offsets [-sa, 8176 - sa), so the first restage boundary B lies in [8161, 8176]
(sa in [0, 15]; it depends on where the page lies in the chunk, and the pages of one chunk differ
in it).  A sweep case puts one element of E bytes at stream offset e0 in one page per e0 of a
contiguous range that contains [8161 - E, 8176]: for every sa and every byte b of the element
(and the byte after it) some page has e0 + b == B, so the boundary falls before each byte of the
element — between a tag and its extra bytes, inside a literal, inside a length chain, between
a chain and the offset.  When the kernel restages is not restated here; the range is the
guarantee, and walk_snappy / walk_lz4 report the stream offset of every element so the test can
check the range really was produced (Case.sweep, sweep_positions).

The case table is the coverage contract of pq_inflate_kernel and hybrid_expand: a case
that stops producing a feature it claims, or a feature of tests/test_pq_pages.py's list that no
case claims, fails the CPU tests."""
import functools
import struct
from collections import Counter, namedtuple

import numpy as np

RING = 32768            # bytes of output history in LDS (scan.hip RING)
IWIN = 8192 - 16        # the compressed stream's LDS window (scan.hip IWIN)
RMAX = 512              # run headers parsed per pass of hybrid_expand
LANES = 64

# parquet.thrift enums (restated: this module imports nothing of the oracle)
BOOLEAN, INT32, INT64, BYTE_ARRAY, FLBA = 0, 1, 2, 6, 7
UNCOMPRESSED, SNAPPY, ZSTD, LZ4_RAW = 0, 1, 6, 7
PLAIN, RLE, RLE_DICTIONARY = 0, 3, 8
DATA_PAGE, DICTIONARY_PAGE, DATA_PAGE_V2 = 0, 2, 3
CODEC_NAME = {UNCOMPRESSED: "none", SNAPPY: "snappy", LZ4_RAW: "lz4", ZSTD: "zstd"}

# offsets that get a feature of their own: the lane count, half the ring, RING - 64 (a 64-byte
# Snappy copy farther back than that is cut in ring segments), the ring's size
EDGE_OFFS = frozenset([1, 2, 3, 7, *range(61, 68), 16383, 16384, 16385, 32703, 32704, 32705, 32767, 32768, 32769])
EDGE_RUNS = (511, 512, 513, 1025)


# ---- Thrift compact page headers -------------------------------------------------------------------
def uvarint(v, pad=0):
    """LEB128; `pad` extra bytes make it non-minimal (continuation bits, then zeros)."""
    out = bytearray()
    while v >= 0x80:
        out.append(v & 0x7F | 0x80)
        v >>= 7
    out.append(v)
    for _ in range(pad):
        out[-1] |= 0x80
        out.append(0)
    return bytes(out)


def _i32(delta, v):
    return bytes([delta << 4 | 5]) + uvarint((v << 1) ^ (v >> 63))


def _bool(delta, v):
    return bytes([delta << 4 | (1 if v else 2)])


def _struct(delta, body):
    return bytes([delta << 4 | 12]) + body + b"\x00"


def _page_header(ptype, uncomp, comp, delta, body):
    return _i32(1, ptype) + _i32(1, uncomp) + _i32(1, comp) + _struct(delta, body) + b"\x00"


def header_v1(n, uncomp, comp, enc):
    """PageHeader {type, sizes, 5: DataPageHeader {num_values, encoding, RLE, RLE}}."""
    return _page_header(DATA_PAGE, uncomp, comp, 2, _i32(1, n) + _i32(1, enc) + _i32(1, RLE) + _i32(1, RLE))


def header_dict(n, uncomp, comp):
    """PageHeader {.., 7: DictionaryPageHeader {num_values, PLAIN}}."""
    return _page_header(DICTIONARY_PAGE, uncomp, comp, 4, _i32(1, n) + _i32(1, PLAIN))


def header_v2(n, nulls, uncomp, comp, enc, def_len, is_compressed):
    """PageHeader {.., 8: DataPageHeaderV2 {num_values, num_nulls, num_rows, encoding,
    definition_levels_byte_length, repetition_levels_byte_length, is_compressed}}."""
    body = _i32(1, n) + _i32(1, nulls) + _i32(1, n) + _i32(1, enc) + _i32(1, def_len) + _i32(1, 0) + _bool(1, is_compressed)
    return _page_header(DATA_PAGE_V2, uncomp, comp, 5, body)


# ---- Snappy ----------------------------------------------------------------------------------------
Lit = namedtuple("Lit", "data form")
Copy = namedtuple("Copy", "kind off len")


def lit(data, form="short"):
    """A literal; form "short" (length in the tag, up to 60 bytes) or 1-4 length bytes."""
    return Lit(bytes(data), form)


def copy(kind, off, ln):
    return Copy(kind, off, ln)


def _back(out, off, ln, check=True):
    """Append ln bytes that repeat the last off bytes of out."""
    if not 0 < off <= len(out):
        assert not check, "offset %d at output %d" % (off, len(out))
        out += bytes(ln)
        return
    pat = bytes(out[len(out) - off:])
    out += pat[:ln] if ln <= off else (pat * (ln // off + 1))[:ln]


def snappy(elements, preamble=None, check=True):
    """(stream, expected output): the preamble varint and the elements as given."""
    s, out = bytearray(), bytearray()
    for e in elements:
        if isinstance(e, Lit):
            n = len(e.data)
            assert n >= 1
            if e.form == "short":
                assert n <= 60
                s.append((n - 1) << 2)
            else:
                assert e.form in (1, 2, 3, 4) and n - 1 < 1 << (8 * e.form)
                s.append((59 + e.form) << 2)
                s += (n - 1).to_bytes(e.form, "little")
            s += e.data
            out += e.data
        else:
            if e.kind == 1:
                assert 4 <= e.len <= 11 and e.off < 2048
                s += bytes([1 | (e.len - 4) << 2 | (e.off >> 8) << 5, e.off & 255])
            else:
                assert e.kind in (2, 3) and 1 <= e.len <= 64 and e.off < 1 << (16 if e.kind == 2 else 32)
                s.append(e.kind | (e.len - 1) << 2)
                s += e.off.to_bytes(2 if e.kind == 2 else 4, "little")
            _back(out, e.off, e.len, check)
    return uvarint(len(out) if preamble is None else preamble) + bytes(s), bytes(out)


def _classify(f, mx, off, ln, w):
    """One back-reference of ln bytes at distance off with w bytes of output produced."""
    mx["off"], mx["len"] = max(mx["off"], off), max(mx["len"], ln)
    if off in EDGE_OFFS:
        f["off_%d" % off] += 1
    npot = off & (off - 1) != 0
    if off == w:
        f["off_eq_w"] += 1
    if off == 1:
        f["off_1"] += 1
    elif off < LANES and npot:
        f["off_lt64_npot"] += 1
    if off < LANES and ln > LANES:
        f["off_1_long" if off == 1 else ("off_lt64_npot_long" if npot else "off_lt64_pot_long")] += 1
    if RING // 2 <= off < RING:
        f["off_half_ring"] += 1
    if off >= RING:
        f["off_ge_ring"] += 1
    if off > 65535:
        f["off_gt_65535"] += 1
    if ln > off:
        f["overlap"] += 1
        if off >= RING:
            f["far_overlap"] += 1
    if off < RING and ln > RING - off:
        room = RING - off
        segs = -(-ln // room)
        mx["segments"] = max(mx["segments"], segs)
        f["ring_multiseg"] += 1
        if off >= RING // 2:
            f["ring_multiseg_half"] += 1
            if ln == room + 1:
                f["ring_seg_plus1"] += 1
            if segs >= 3:
                f["ring_multiseg_x3"] += 1
        if room == 1 and ln == LANES:
            f["ring_seg_1byte_x64"] += 1


def _maxima():
    return dict(off=0, len=0, lit=0, segments=0, elements=0)


def walk_snappy(stream):
    """(features, maxima, output length, [(stream offset, element bytes, tag)]) of a Snappy block."""
    b = bytes(stream)
    f, mx, pos = Counter(), _maxima(), []
    n = sh = p = 0
    while True:
        assert p < len(b) and sh <= 28, "preamble"
        c = b[p]
        p += 1
        n |= (c & 0x7F) << sh
        sh += 7
        if not c & 0x80:
            break
    w = 0
    last = None
    while p < len(b):
        t0, tag = p, b[p]
        kind = tag & 3
        if kind == 0:
            ln, extra = tag >> 2, 0
            if ln >= 60:
                extra = ln - 59
                assert p + 1 + extra <= len(b), "literal tag cut off"
                ln = int.from_bytes(b[p + 1:p + 1 + extra], "little")
            ln += 1
            p += 1 + extra
            assert p + ln <= len(b), "literal past the stream"
            f["lit_short" if not extra else "lit_%db" % extra] += 1
            if extra == 4 and ln <= 60:
                f["lit_4b_small"] += 1
            if ln > IWIN:
                f["lit_gt_iwin"] += 1
            mx["lit"] = max(mx["lit"], ln)
            p += ln
            w += ln
            pos.append((t0, 1 + extra, "lit_%d" % extra))
            last = "lit"
        else:
            size = (0, 2, 3, 5)[kind]
            assert p + size <= len(b), "copy tag cut off"
            if kind == 1:
                ln, off = ((tag >> 2) & 7) + 4, (tag >> 5) << 8 | b[p + 1]
            else:
                ln, off = (tag >> 2) + 1, int.from_bytes(b[p + 1:p + size], "little")
            p += size
            assert 0 < off <= w, "copy offset %d at output %d" % (off, w)
            f["copy_k%d" % kind] += 1
            if kind == 3 and off > 65535:
                f["copy_k3_gt_65535"] += 1
            _classify(f, mx, off, ln, w)
            w += ln
            pos.append((t0, size, "copy_%d" % kind))
            last = "copy"
        mx["elements"] += 1
    assert w == n, "output %d, preamble %d" % (w, n)
    if last == "copy":
        f["end_after_tag"] += 1
    return f, mx, w, pos


# ---- LZ4 block -------------------------------------------------------------------------------------
def _chain(v):
    """The nibble and the explicit 255-chain of a length."""
    if v < 15:
        return v, b""
    v -= 15
    return 15, b"\xff" * (v // 255) + bytes([v % 255])


def lz4_sequence(lits, off=0, ml=0, last=False):
    ln, lc = _chain(len(lits))
    if last:
        assert off == 0 and ml == 0
        return bytes([ln << 4]) + lc + bytes(lits)
    assert ml >= 4 and 0 <= off < 65536
    mn, mc = _chain(ml - 4)
    return bytes([ln << 4 | mn]) + lc + bytes(lits) + off.to_bytes(2, "little") + mc


def lz4(seqs, check=True):
    """(block, expected output) of sequences (literals, offset, match length); the final one is
    (literals, 0, 0): literals only (an empty `literals` there is a lone zero token)."""
    s, out = bytearray(), bytearray()
    for i, (lits, off, ml) in enumerate(seqs):
        last = i == len(seqs) - 1
        s += lz4_sequence(lits, off, ml, last)
        out += lits
        if not last:
            _back(out, off, ml, check)
    return bytes(s), bytes(out)


def _chain_feature(f, what, nibble, n255):
    if nibble < 15:
        f[what + "_nochain"] += 1
    else:
        f["%s_chain_%s" % (what, n255 if n255 <= 2 else ("ge40" if n255 >= 40 else "mid"))] += 1


def walk_lz4(block, n):
    """(features, maxima, output length, [(stream offset, bytes, part)]) of an LZ4 block that
    decodes to n bytes."""
    b = bytes(block)
    f, mx, pos = Counter(), _maxima(), []
    p = w = 0

    def chain(p, v):
        k = 0
        if v == 15:
            while True:
                assert p < len(b), "length chain past the block"
                c = b[p]
                p += 1
                v += c
                if c != 255:
                    break
                k += 1
        return p, v, k

    while p < len(b):
        t0, tok = p, b[p]
        p, ll, k = chain(p + 1, tok >> 4)
        pos.append((t0, p - t0, "token_lit"))
        assert p + ll <= len(b), "literals past the block"
        if ll > IWIN:
            f["lit_gt_iwin"] += 1
        mx["lit"] = max(mx["lit"], ll)
        mx["elements"] += 1
        p += ll
        w += ll
        if p == len(b):  # the last sequence: literals only
            _chain_feature(f, "lit", tok >> 4, k)
            assert tok & 15 == 0, "match length in the last token"
            f["last_lits" if ll else "last_nolits"] += 1
            break
        _chain_feature(f, "lit", tok >> 4, k)
        if ll == 0:
            f["lit0"] += 1
        assert p + 2 <= len(b), "offset past the block"
        o0 = p
        off = b[p] | b[p + 1] << 8
        p, ml, k = chain(p + 2, tok & 15)
        pos.append((o0, p - o0, "off_ml"))
        _chain_feature(f, "ml", tok & 15, k)
        ml += 4
        assert 0 < off <= w, "match offset %d at output %d" % (off, w)
        _classify(f, mx, off, ml, w)
        w += ml
    else:
        f["end_after_match"] += 1
    assert w == n, "output %d, expected %d" % (w, n)
    return f, mx, w, pos


# ---- the RLE / bit-packed hybrid -------------------------------------------------------------------
RleRun = namedtuple("RleRun", "count value pad")
BpRun = namedtuple("BpRun", "values truncate_tail pad groups")


def rle(count, value, pad=0):
    return RleRun(count, value, pad)


def bp(values, truncate_tail=False, pad=0, groups=None):
    """A bit-packed run of len(values) values in ceil(len / 8) groups (or `groups`, for a header that
    lies); truncate_tail: only ceil(len * bw / 8) bytes are written."""
    return BpRun(tuple(values), truncate_tail, pad, groups)


def hybrid(runs, bw):
    out = bytearray()
    vb = (bw + 7) // 8
    for r in runs:
        if isinstance(r, RleRun):
            out += uvarint(r.count << 1, r.pad) + r.value.to_bytes(vb, "little")
        else:
            g = -(-len(r.values) // 8)
            bits = 0
            for i, v in enumerate(r.values):
                assert 0 <= v < 1 << bw or (bw == 0 and v == 0)
                bits |= v << (i * bw)
            nbytes = -(-len(r.values) * bw // 8) if r.truncate_tail else g * bw
            out += uvarint((g if r.groups is None else r.groups) << 1 | 1, r.pad) + bits.to_bytes(nbytes, "little")
    return bytes(out)


def expand(runs, n):
    """The first n values the runs hold."""
    out = []
    for r in runs:
        out += [r.value] * r.count if isinstance(r, RleRun) else list(r.values) + [0] * (-len(r.values) % 8)
    assert len(out) >= n
    return out[:n]


def walk_hybrid(sec, bw, n, f=None, pre=""):
    """The n values of a hybrid stream that fills `sec`, and its features (names prefixed `pre`)."""
    sec = bytes(sec)
    f = Counter() if f is None else f
    vb = (bw + 7) // 8
    assert bw <= 32, "bit width"
    p = k = runs = 0
    kinds, vals = [], []
    while k < n:
        assert p < len(sec), "run header past the section"
        h = sh = nb = 0
        while True:
            assert p < len(sec) and nb < 5, "run header varint"
            c = sec[p]
            p += 1
            nb += 1
            h |= (c & 0x7F) << sh
            sh += 7
            if not c & 0x80:
                break
        assert h < 1 << 32, "run header past 32 bits"
        if nb > len(uvarint(h)):
            f[pre + "padded_varint"] += 1
        if h & 1:
            groups = h >> 1
            assert groups * 8 < 1 << 32, "bit-packed count past 32 bits"
            nbytes, avail = groups * bw, len(sec) - p
            if nbytes > avail:
                assert -(-(n - k) * bw // 8) <= avail, "bit-packed run past the section"
                f[pre + "bp_truncated"] += 1
                nbytes = avail
            bits = int.from_bytes(sec[p:p + nbytes], "little")
            p += nbytes
            take = min(groups * 8, n - k)
            vals += [(bits >> (i * bw)) & ((1 << bw) - 1) for i in range(take)]
            if groups * 8 > n - k:
                f[pre + "bp_overshoot"] += 1
                if bits >> (take * bw):
                    f[pre + "pad_bits_set"] += 1
            k += groups * 8
            f[pre + "bp"] += 1
            kinds.append(1)
        else:
            cnt = h >> 1
            assert cnt > 0, "RLE run of length 0"
            assert p + vb <= len(sec), "RLE value past the section"
            v = int.from_bytes(sec[p:p + vb], "little")
            p += vb
            vals += [v] * min(cnt, n - k)
            if cnt > n - k:
                f[pre + "rle_overshoot"] += 1
            k += cnt
            f[pre + "rle"] += 1
            f[pre + "rle_vb%d" % vb] += 1
            kinds.append(0)
        runs += 1
    f[pre + "bw_%d" % bw] += 1
    if runs in EDGE_RUNS:
        f[pre + "runs_%d" % runs] += 1
    if runs > RMAX:
        f[pre + "runs_gt_rmax"] += 1
    if runs > 2 * RMAX:
        f[pre + "runs_gt_2rmax"] += 1
    if runs >= 3 and all(a != b for a, b in zip(kinds, kinds[1:])):
        f[pre + "alternating"] += 1
    if bw and any(v >> (bw - 1) for v in vals):
        f[pre + "topbit_bw%d" % bw] += 1
    return vals, f


# ---- pages -----------------------------------------------------------------------------------------
def compress(codec, data):
    """A page payload under the chunk's codec: one literal (Snappy, LZ4: the assemblers above), or
    libzstd's frame."""
    if codec == UNCOMPRESSED:
        return bytes(data)
    if codec == SNAPPY:
        return snappy([lit(data, 1 if len(data) <= 256 else 2 if len(data) <= 65536 else 3)])[0]
    if codec == LZ4_RAW:
        return lz4([(data, 0, 0)])[0]
    import pyarrow as pa
    return pa.compress(bytes(data), codec="zstd", asbytes=True)


def page_v1(values, n, enc, codec=UNCOMPRESSED, defs=None, level_len=None):
    """A v1 data page: [u32 length + definition levels, nullable columns only][values]."""
    raw = b"" if defs is None else struct.pack("<I", len(defs) if level_len is None else level_len) + defs
    raw += values
    c = compress(codec, raw)
    return header_v1(n, len(raw), len(c), enc) + c


def page_v2(values, n, nulls, enc, codec=UNCOMPRESSED, defs=b"", is_compressed=True):
    """A v2 data page: the levels in front, never compressed; the values under the codec unless
    is_compressed is false."""
    c = compress(codec, values) if is_compressed else bytes(values)
    return header_v2(n, nulls, len(defs) + len(values), len(defs) + len(c), enc, len(defs), is_compressed) + defs + c


def page_dict(values, n, codec=UNCOMPRESSED):
    c = compress(codec, values)
    return header_dict(n, len(values), len(c)) + c


def stream_page(stream, uncompressed):
    """A compressed stream as the payload of a required INT64 PLAIN v1 page."""
    assert uncompressed % 8 == 0
    return header_v1(uncompressed // 8, uncompressed, len(stream), PLAIN) + stream


def plain(ptype, vals):
    if ptype == BYTE_ARRAY:
        return b"".join(struct.pack("<I", len(v)) + v for v in vals)
    if ptype == FLBA:
        return b"".join(vals)
    if ptype == BOOLEAN:
        return int("".join("1" if v else "0" for v in reversed(vals)) or "0", 2).to_bytes(-(-len(vals) // 8), "little")
    return np.asarray(vals, {INT32: "<i4", INT64: "<i8"}[ptype]).tobytes()


# ---- the chunk walker ------------------------------------------------------------------------------
def _read_struct(b, p):
    """A Thrift compact struct of i32 / bool / struct fields: ({field id: value}, end)."""
    out, last = {}, 0
    while True:
        h = b[p]
        p += 1
        if h == 0:
            return out, p
        assert h >> 4, "long-form field id"
        last += h >> 4
        t = h & 15
        if t in (1, 2):
            out[last] = t == 1
        elif t == 5:
            v = sh = 0
            while True:
                c = b[p]
                p += 1
                v |= (c & 0x7F) << sh
                sh += 7
                if not c & 0x80:
                    break
            out[last] = (v >> 1) ^ -(v & 1)
        else:
            assert t == 12, "field type %d" % t
            out[last], p = _read_struct(b, p)


def walk_chunk(c):
    """Features of a case's chunk from its bytes: page kinds and their order, and, where the bytes
    of a page lie uncompressed in the chunk, its hybrid streams (def_, idx_, bool_ features), its
    dictionary indices against the dictionary's size and its FIXED_LEN_BYTE_ARRAY values."""
    b = b"".join(c.pages)
    f = Counter()
    p, order, dict_n, npages = 0, [], None, 0
    while p < len(b):
        h, p = _read_struct(b, p)
        ptype, uncomp, comp = h[1], h[2], h[3]
        body = b[p:p + comp]
        assert len(body) == comp, "page past the chunk"
        p += comp
        npages += 1
        if ptype == DICTIONARY_PAGE:
            dict_n = h[7][1]
            order.append("dict")
            f["page_dict"] += 1
            continue
        d = h[5] if ptype == DATA_PAGE else h[8]
        n = d[1]
        enc = d[2] if ptype == DATA_PAGE else d[4]
        flag = ptype == DATA_PAGE_V2 and not d[7]
        kind = ("v1" if ptype == DATA_PAGE else "v2") + ("_dict" if enc == RLE_DICTIONARY else "_plain" if enc == PLAIN else "_rle") + \
            ("_flag_uncompressed" if flag else "")
        order.append(kind)
        f["page_" + kind] += 1
        if n == 0:
            f["page_zero_values"] += 1
            if any(k != "dict" for k in order[:-1]) and p < len(b):
                f["page_zero_values_between"] += 1
        stored = c.codec == UNCOMPRESSED or flag
        if ptype == DATA_PAGE_V2 and c.codec != UNCOMPRESSED and not flag:
            f["page_v2_compressed"] += 1
        if not stored:
            continue
        assert comp == uncomp, "stored page sizes differ"
        if ptype == DATA_PAGE_V2:
            d0, d1 = 0, d[5]
            assert d1 <= len(body), "v2 level length past the page"
        elif c.max_def:
            assert len(body) >= 4, "no level length"
            ln, = struct.unpack_from("<I", body)
            assert ln <= len(body) - 4, "v1 level length past the page"
            d0, d1 = 4, 4 + ln
        else:
            d0 = d1 = 0
        if c.max_def:
            defs, _ = walk_hybrid(body[d0:d1], 1, n, f, "def_")
        else:
            defs = [1] * n
        nn = sum(defs)
        if c.max_def and n and nn == 0:
            f["page_all_null"] += 1
        vp = d1
        if enc == RLE_DICTIONARY:
            if vp == len(body):
                assert nn == 0, "no index bytes"
                f["page_all_null_no_index"] += 1
                continue
            bw = body[vp]
            if bw == 0:
                f["idx_bw_0_explicit"] += 1
            idx, _ = walk_hybrid(body[vp + 1:], bw, nn, f, "idx_")
            assert dict_n is not None and all(i < dict_n for i in idx), "dictionary index past the dictionary"
        elif enc == RLE:
            assert c.ptype == BOOLEAN
            ln, = struct.unpack_from("<I", body, vp)
            assert vp + 4 + ln <= len(body), "RLE boolean length past the page"
            walk_hybrid(body[vp + 4:vp + 4 + ln], 1, nn, f, "bool_")
        elif c.ptype == FLBA:
            t = c.tlen
            assert vp + nn * t <= len(body), "values past the page"
            f["flba_%d_%s" % (t, "nullable" if c.max_def else "required")] += 1
            pats = {b"\x80" + bytes(t - 1): "min", b"\x7f" + b"\xff" * (t - 1): "max", b"\xff" * t: "minus1", bytes(t): "zero"}
            if t > 1:
                pats.update({b"\x00\x80" + bytes(t - 2): "0080", b"\xff\x7f" + b"\xff" * (t - 2): "ff7f"})
            for k in range(nn):
                name = pats.get(body[vp + k * t:vp + (k + 1) * t])
                if name:
                    f["flba_%s" % name] += 1
    if order == ["dict", "v1_dict", "v2_dict_flag_uncompressed", "v2_dict", "v1_plain"]:
        f["mixed_order_%s_%s" % (CODEC_NAME[c.codec], {INT64: "int64", BYTE_ARRAY: "byte_array"}.get(c.ptype, "other"))] += 1
    return f


def features(c):
    """Every feature the walkers find in a case: its streams (prefixed sn_ / lz_) and its chunk."""
    f = Counter()
    for stream, exp in c.streams:
        if c.codec == SNAPPY:
            g, _, n, _ = walk_snappy(stream)
            pre = "sn_"
        else:
            g, _, n, _ = walk_lz4(stream, len(exp))
            pre = "lz_"
        assert n == len(exp)
        for k, v in g.items():
            f[pre + k] += v
    if not c.streams:
        f.update(walk_chunk(c))
    return f


def maxima(c):
    """The walkers' maxima over a stream case's streams (the path that was live, for a report)."""
    out = _maxima()
    for stream, exp in c.streams:
        mx = walk_snappy(stream)[1] if c.codec == SNAPPY else walk_lz4(stream, len(exp))[1]
        out = {k: max(out[k], mx[k]) for k in out}
    return out


def sweep_positions(c):
    """The stream offsets at which a sweep case's pages put the swept element's first byte, and
    the element's length in bytes."""
    tag, at, elen = c.sweep
    out = []
    for stream, exp in c.streams:
        pos = walk_snappy(stream)[3] if c.codec == SNAPPY else walk_lz4(stream, len(exp))[3]
        hits = [p for p in pos if p[2] == tag]
        out.append(hits[at][0])
    return out, elen


# ---- the case table --------------------------------------------------------------------------------
# target: the Databend type the chunk is decoded to ("i64", "i32", "str", "bool", "dec"), nullable
# when max_def; expected: one Python value per row, None for NULL; streams: (compressed stream,
# bytes it decodes to) of each page of a stream case, where `expected` is those bytes as INT64;
# lib: libsnappy / liblz4 decode the streams; sweep: (walker part, index, element bytes) or None
Case = namedtuple("Case", "name codec ptype max_def tlen target pages expected claims streams lib sweep")


def _stream_case(name, codec, streams, claims, lib=True, sweep=None):
    for s, e in streams:
        assert len(e) % 8 == 0, (name, len(e))
    exp = np.frombuffer(b"".join(e for _, e in streams), "<i8").tolist()
    return Case(name, codec, INT64, 0, 0, "i64", tuple(stream_page(s, len(e)) for s, e in streams), exp,
                frozenset(("sn_" if codec == SNAPPY else "lz_") + x for x in claims), tuple(streams), lib, sweep)


def _sn(name, elements, claims, rng, pad=True):
    """A Snappy case; the output is brought to whole INT64 values by a trailing literal."""
    if pad:
        _, out = snappy(elements)
        elements = list(elements) + [lit(rng.integers(0, 256, 8 + -len(out) % 8, dtype=np.uint8).tobytes())]
    return _stream_case(name, SNAPPY, [snappy(elements)], claims)


def _lz(name, seqs, claims, rng, tail=5, lib=True):
    """An LZ4 case; the final literal-only sequence brings the output to whole INT64 values."""
    _, out = lz4(list(seqs) + [(b"", 0, 0)])
    k = tail + -(len(out) + tail) % 8
    return _stream_case(name, LZ4_RAW, [lz4(list(seqs) + [(rng.integers(0, 256, k, dtype=np.uint8).tobytes(), 0, 0)])], claims, lib)


def _snappy_cases():
    rng = np.random.default_rng(21)
    rb = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    out = []
    # every literal length form; a 4-byte form that carries a small length; one longer than the window
    out.append(_sn("sn_literal_forms", [lit(rb(1)), lit(rb(60)), lit(rb(61), 1), lit(rb(256), 1), lit(rb(3), 1), lit(rb(300), 2),
                                        lit(rb(65536), 2), lit(rb(7), 3), lit(rb(70_000), 3), lit(rb(5), 4), lit(rb(60), 4),
                                        lit(rb(9000), 4), lit(rb(1), 2)],
                   {"lit_short", "lit_1b", "lit_2b", "lit_3b", "lit_4b", "lit_4b_small", "lit_gt_iwin"}, rng))
    # the three copy kinds; kind 3 with an offset past 16 bits (70 000 bytes of history) and with a small one
    el = [lit(rb(70_000), 3)]
    for e in (copy(1, 5, 11), copy(1, 2047, 4), copy(1, 256, 7), copy(2, 2048, 64), copy(2, 65535, 1), copy(2, 9, 33), copy(3, 65536, 64),
              copy(3, 69_000, 33), copy(3, 70_001, 64), copy(3, 100, 10), copy(3, 40_000, 17)):
        el += [e, lit(rb(3))]
    out.append(_sn("sn_copy_kinds", el, {"copy_k1", "copy_k2", "copy_k3", "copy_k3_gt_65535", "off_gt_65535", "off_ge_ring"}, rng))
    # offsets around the lane count, shorter and longer than the offset
    el = [lit(rb(300), 2)]
    for off in (1, 2, 3, 7, *range(61, 68)):
        for ln in (1, 4, 11, 63, 64):
            el += [copy(2, off, ln), lit(rb(5))]
    out.append(_sn("sn_offsets_lanes", el, {"off_%d" % o for o in (1, 2, 3, 7, *range(61, 68))} | {"off_1", "off_lt64_npot", "overlap"}, rng))
    # offsets at half the ring, at RING - 64 and at the ring's size; every offset from RING - 66 to
    # RING + 1 with a 64-byte copy: the segmented ring loop from 62 bytes per segment down to 1
    el = [lit(rb(40_000), 2)]
    for off in (16383, 16384, 16385, 32703, 32704, 32705, 32767, 32768, 32769):
        for kind, ln in ((2, 1), (2, 64), (3, 37)):
            el += [copy(kind, off, ln), lit(rb(3))]
    for off in range(RING - 66, RING + 2):
        el += [copy(2, off, 64), lit(rb(1))]
    out.append(_sn("sn_offsets_ring", el, {"off_%d" % o for o in EDGE_OFFS if o > 100} |
                   {"off_half_ring", "off_ge_ring", "ring_multiseg", "ring_multiseg_half", "ring_seg_plus1", "ring_multiseg_x3",
                    "ring_seg_1byte_x64"}, rng))
    # a copy whose offset is everything produced so far: it starts at output byte 0
    out.append(_sn("sn_off_eq_w_small", [lit(rb(37)), copy(2, 37, 64), lit(rb(2))], {"off_eq_w", "overlap"}, rng))
    out.append(_sn("sn_off_eq_w_first_byte", [lit(rb(1)), copy(1, 1, 11)], {"off_eq_w", "off_1"}, rng))
    out.append(_sn("sn_off_eq_w_far", [lit(rb(40_000), 2), copy(3, 40_000, 64)], {"off_eq_w", "off_ge_ring"}, rng))
    # the stream ends with a copy tag's last byte (outputs of 48, 64 and 56 bytes: no padding literal)
    out.append(_sn("sn_end_on_copy_k1", [lit(rb(37)), copy(1, 5, 11)], {"end_after_tag", "copy_k1"}, rng, pad=False))
    out.append(_sn("sn_end_on_copy_k2", [lit(rb(40)), copy(2, 40, 24)], {"end_after_tag", "copy_k2"}, rng, pad=False))
    out.append(_sn("sn_end_on_copy_k3", [lit(rb(40)), copy(3, 7, 16)], {"end_after_tag", "copy_k3"}, rng, pad=False))
    return out


def _lz4_cases():
    rng = np.random.default_rng(22)
    rb = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    out = []
    long_chain = 15 + 40 * 255 + 7
    # literal and match length chains of no, 0, 1, 2 and 40 / 41 bytes of 255; a literal past the window
    seqs = [(rb(3), 2, 7), (rb(15), 9, 4 + 15), (rb(15 + 254), 100, 4 + 15 + 254), (rb(270), 33, 4 + 270), (rb(525), 300, 4 + 525),
            (rb(long_chain), 5000, 4 + 15 + 41 * 255 + 2), (rb(14), 20_000, 4 + 14)]
    out.append(_lz("lz_chains", seqs, {"lit_nochain", "lit_chain_0", "lit_chain_1", "lit_chain_2", "lit_chain_ge40", "ml_nochain",
                                       "ml_chain_0", "ml_chain_1", "ml_chain_2", "ml_chain_ge40", "lit_gt_iwin", "last_lits"}, rng))
    # sequences without literals: the offset is taken from the bytes peeked with the token
    seqs = [(rb(100), 50, 20), (b"", 7, 4), (b"", 100, 18), (b"", 1, 19), (b"", 120, 300), (b"", 3, 4 + 15 + 255), (rb(1), 64, 9), (b"", 160, 5)]
    out.append(_lz("lz_lit0", seqs, {"lit0", "ml_chain_0", "ml_chain_1"}, rng))
    # ring offsets from RING / 2 up with matches one byte and several times longer than RING - off
    seqs = [(rb(33_000), 100, 4)]
    for off, over in ((16384, 2), (20_000, 3), (32_000, 5), (32_767, 5000), (32_767, 20), (32_704, 3)):
        room = RING - off
        seqs += [(rb(5), off, max(room + 1, 4)), (rb(3), off, over if over > 100 else over * room + 17), (b"", off, max(room, 4)), (rb(2), off, max(room - 1, 4))]
    out.append(_lz("lz_ring_segments", seqs, {"ring_multiseg", "ring_multiseg_half", "ring_seg_plus1", "ring_multiseg_x3", "overlap",
                                              "off_half_ring", "off_16384", "off_32767", "off_32704"}, rng))
    # offsets of the ring's size and more, matches longer than the offset (read back from the output)
    seqs = [(rb(40_000), 39_000, 50), (rb(5), 33_000, 34_000), (rb(3), 32_768, 33_000), (b"", 65_535, 66_000), (rb(1), 32_769, 10)]
    out.append(_lz("lz_far_overlap", seqs, {"off_ge_ring", "far_overlap", "off_32768", "off_32769"}, rng))
    # offset 1 and the offsets around the lane count with matches longer than 64 bytes
    seqs = [(rb(300), 100, 4)]
    for off in (1, 2, 3, 5, 6, 7, 33, *range(61, 68)):
        for ml in (4, 63, 64, 65, 200, 1000):
            seqs.append((rb(70 + off % 5), off, ml))
    out.append(_lz("lz_offsets_lanes", seqs, {"off_%d" % o for o in (1, 2, 3, 7, *range(61, 68))} | {"off_1", "off_lt64_npot", "off_1_long", "off_lt64_npot_long", "overlap"},
                   rng))
    seqs = [(rb(33_000), 100, 4)]
    for off in sorted(o for o in EDGE_OFFS if o > 100):
        seqs += [(rb(4), off, 4), (rb(3), off, 100), (b"", off, 64)]
    out.append(_lz("lz_offsets_ring", seqs, {"off_%d" % o for o in EDGE_OFFS if o > 100} | {"off_half_ring", "off_ge_ring", "ring_multiseg"}, rng))
    out.append(_lz("lz_off_eq_w", [(rb(50), 50, 300), (rb(9), 359, 20)], {"off_eq_w", "overlap"}, rng))
    out.append(_lz("lz_off_eq_w_far", [(rb(33_000), 33_000, 70)], {"off_eq_w", "off_ge_ring"}, rng))
    # the last sequence without literals: a lone zero token after the final match.  liblz4 refuses
    # a match that ends in the block's last 5 bytes (its encoder never writes one); the format
    # description allows the decoder to take it, and the kernel and the oracle do
    s = lz4([(rb(40), 17, 24), (b"", 0, 0)])
    out.append(_stream_case("lz_last_nolits", LZ4_RAW, [s], {"last_nolits"}, lib=False))
    return out


def _sweep_range(elen, margin=3):
    return range(IWIN - 15 - elen - margin, IWIN + margin + 1)


def _sweep_cases():
    rng = np.random.default_rng(23)
    rb = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    out = []
    # Snappy: a lead literal (3-byte tag) after the 2-byte preamble puts the element at e0 = 5 + L
    for name, elem, tail, tag in (("sweep_sn_copy3", copy(3, 4097, 61), [lit(rb(11))], "copy_3"),
                                  ("sweep_sn_lit4", lit(rb(23), 4), [copy(2, 100, 9), lit(rb(4))], "lit_4")):
        streams = []
        for e0 in range(8110, 8210):
            L = e0 - 5
            el = [lit(rb(L), 2), elem] + tail
            _, o = snappy(el)
            el.append(lit(rb(8 + -len(o) % 8)))
            s = snappy(el)
            assert len(s[1]) < 16384  # the preamble is two bytes
            streams.append(s)
        out.append(_stream_case(name, SNAPPY, streams, {"copy_k3"} if tag == "copy_3" else {"lit_4b", "lit_4b_small"},
                                sweep=(tag, 0, 5)))
    # LZ4: [token + literal chain][270 literals][offset][match chain of 3 x 255 + 1 byte]: 283 bytes.  The
    # lead is a sequence of its own (L literals and a short match); where L's chain grows by a
    # byte the match takes a one-byte chain instead, so every e0 is produced
    lits, ml = 270, 4 + 15 + 3 * 255 + 5
    elen = len(lz4_sequence(bytes(lits), 1, ml))
    streams = []
    for e0 in _sweep_range(elen):
        lead = None
        for L in range(e0 - 3 - (e0 // 255 + 2), e0):
            for m in (4, 19):
                if L > 0 and len(lz4_sequence(bytes(L), 1, m)) == e0:
                    lead = (rb(L), 77, m)
        assert lead, e0
        seqs = [lead, (rb(lits), 4099, ml)]
        _, o = lz4(seqs + [(b"", 0, 0)])
        streams.append(lz4(seqs + [(rb(5 + -(len(o) + 5) % 8), 0, 0)]))
    out.append(_stream_case("sweep_lz_chains", LZ4_RAW, streams, {"lit_chain_1", "ml_chain_mid"}, sweep=("token_lit", 1, elen)))
    return out


def _chunk_case(name, ptype, max_def, pages, expected, claims, codec=UNCOMPRESSED, tlen=0):
    target = {INT32: "i32", INT64: "i64", BYTE_ARRAY: "str", BOOLEAN: "bool", FLBA: "dec"}[ptype]
    return Case(name, codec, ptype, max_def, tlen, target, tuple(pages), list(expected), frozenset(claims), (), False, None)


def _rows(defs, vals):
    it = iter(vals)
    out = [next(it) if d else None for d in defs]
    assert next(it, None) is None
    return out


def _dict_page_pair(dic, n, def_runs, idx_runs, bw, v2=False, **kw):
    """(page, rows) of a nullable dictionary-encoded page from its runs."""
    defs = expand(def_runs, n)
    idx = expand(idx_runs, sum(defs))
    values = bytes([bw]) + hybrid(idx_runs, bw)
    if v2:
        pg = page_v2(values, n, n - sum(defs), RLE_DICTIONARY, defs=hybrid(def_runs, 1), **kw)
    else:
        pg = page_v1(values, n, RLE_DICTIONARY, defs=hybrid(def_runs, 1), **kw)
    return pg, _rows(defs, [dic[i] for i in idx])


def _alternating(rng, nruns, bw, top, total=None):
    """nruns runs of alternating kinds that end with an RLE run; with `total`, the values sum to it
    (width 1) by the last run's count."""
    runs, ones = [], 0
    for i in range(nruns):
        if (nruns - 1 - i) % 2 == 0:
            v = int(rng.integers(0, top))
            cnt = int(rng.integers(1, 5))
            if total is not None and i == nruns - 1:
                v, cnt = 1, total - ones
                assert cnt > 0
            runs.append(rle(cnt, v))
            ones += cnt * v
        else:
            vals = [int(x) for x in rng.integers(0, top, 8)]
            runs.append(bp(vals))
            ones += sum(vals)
    return runs


def _count(runs):
    return sum(r.count if isinstance(r, RleRun) else 8 * -(-len(r.values) // 8) for r in runs)


def _hybrid_cases():
    rng = np.random.default_rng(24)
    out = []
    # every index width 0..32 as pages of one required INT32 chunk over a 2^20-entry dictionary: RLE
    # runs (value bytes 0..4) and bit-packed runs in every page; up to width 20 the largest index
    # of the width is used, wider pages hold indices below 2^20
    dn = 1 << 20
    dic = (np.arange(dn, dtype=np.int64) * 2654435761 % (1 << 32) - (1 << 31)).astype("<i4")
    pages, rows, claims = [page_dict(dic.tobytes(), dn)], [], {"page_dict", "idx_bw_0_explicit"}
    for bw in range(33):
        hi = min(1 << bw, dn)
        top = hi - 1
        r = lambda k: [int(x) for x in rng.integers(0, hi, k)]  # noqa: E731
        runs = [rle(5, top), bp(r(15) + [top]), rle(3, r(1)[0]), rle(70, top // 2 + 1 if bw else 0), bp(r(24)), bp([top] + r(6))]
        n = 5 + 16 + 3 + 70 + 24 + 7
        pages.append(page_v1(bytes([bw]) + hybrid(runs, bw), n, RLE_DICTIONARY))
        rows += [int(dic[i]) for i in expand(runs, n)]
        claims |= {"idx_bw_%d" % bw, "idx_rle", "idx_bp", "idx_bp_overshoot"}
        if 1 <= bw <= 20:
            claims.add("idx_topbit_bw%d" % bw)
        if bw:
            claims.add("idx_rle_vb%d" % ((bw + 7) // 8))
    out.append(_chunk_case("hy_index_widths", INT32, 0, pages, rows, claims))
    # a small INT64 dictionary for the rest
    dic = [int(x) for x in rng.integers(-2**62, 2**62, 8)]
    dpage = page_dict(plain(INT64, dic), 8)
    # 511, 512, 513 and 1025 runs of alternating kinds, in the definition levels and in the indices
    for nruns in EDGE_RUNS:
        idx_runs = _alternating(rng, nruns, 3, 8)
        nn = _count(idx_runs)
        def_runs = _alternating(rng, nruns, 1, 2, total=nn)
        n = _count(def_runs)
        pg, r = _dict_page_pair(dic, n, def_runs, idx_runs, 3)
        claims = {"def_runs_%d" % nruns, "idx_runs_%d" % nruns, "def_alternating", "idx_alternating", "idx_bw_3", "def_bw_1"}
        if nruns > RMAX:
            claims |= {"def_runs_gt_rmax", "idx_runs_gt_rmax"}
        if nruns > 2 * RMAX:
            claims |= {"def_runs_gt_2rmax", "idx_runs_gt_2rmax"}
        out.append(_chunk_case("hy_runs_%d" % nruns, INT64, 1, [dpage, pg], r, claims))
    # the last run holds more values than the page: an RLE count and a bit-packed group past n, the
    # group's padding bits set (levels: padding 1s are not values; indices: padding 7s are not read)
    p1, r1 = _dict_page_pair(dic, 20, [bp([1, 0, 1, 1, 0, 1, 1, 1]), rle(100, 1)], [rle(3, 5), bp([1, 2, 3, 4, 5, 6, 7, 0] * 2 + [7] * 8)], 3)
    p2, r2 = _dict_page_pair(dic, 13, [rle(6, 1), bp([0, 1, 1, 0, 1, 0, 1, 1])], [bp([7, 6, 5, 4, 3, 2, 1, 0]), rle(1000, 6)], 3, v2=True)
    out.append(_chunk_case("hy_overshoot", INT64, 1, [dpage, p1, p2], r1 + r2,
                           {"def_rle_overshoot", "def_bp_overshoot", "def_pad_bits_set", "idx_rle_overshoot", "idx_bp_overshoot",
                            "idx_pad_bits_set", "page_v1_dict", "page_v2_dict"}))
    # a bit-packed tail cut to ceil(remaining * bw / 8) bytes (11 values of width 5 in 7 bytes, not 10)
    tail = [int(x) for x in rng.integers(0, 8, 11)]
    p1, r1 = _dict_page_pair(dic, 30, [rle(30, 1)], [rle(19, 2), bp(tail, truncate_tail=True)], 5)
    p2, r2 = _dict_page_pair(dic, 11, [rle(11, 1)], [bp(tail, truncate_tail=True)], 5, v2=True)
    p3, r3 = _dict_page_pair(dic, 11, [rle(11, 1)], [bp(tail)], 5)
    out.append(_chunk_case("hy_truncated_tail", INT64, 1, [dpage, p1, p2, p3], r1 + r2 + r3, {"idx_bp_truncated", "idx_bw_5"}))
    # run headers as padded varints (2 to 5 bytes for a one-byte value)
    p1, r1 = _dict_page_pair(dic, 40, [rle(9, 1, pad=1), bp([1, 0] * 4, pad=2), rle(23, 1, pad=4)],
                             [rle(4, 7, pad=3), bp(range(8), pad=1), bp(range(8), pad=4), rle(16, 1, pad=2)], 3)
    out.append(_chunk_case("hy_padded_varint", INT64, 1, [dpage, p1], r1, {"def_padded_varint", "idx_padded_varint"}))
    # a page without values between two others; a page of NULLs that carries no index bytes at all
    pa_, ra = _dict_page_pair(dic, 10, [bp([1, 0, 1, 1, 0, 1, 1, 1]), rle(2, 1)], [rle(2, 3), bp([1, 2, 3, 4, 5, 6])], 3)
    pz = page_v1(bytes([3]), 0, RLE_DICTIONARY, defs=b"")
    pb, rb_ = _dict_page_pair(dic, 9, [rle(9, 1)], [bp([7, 0, 7, 0, 1, 2, 3, 4]), rle(1, 5)], 3)
    out.append(_chunk_case("hy_zero_values_page", INT64, 1, [dpage, pa_, pz, pb], ra + rb_, {"page_zero_values_between"}))
    pn = page_v1(b"", 300, RLE_DICTIONARY, defs=hybrid([rle(300, 0)], 1))
    pn2 = page_v2(b"", 17, 17, RLE_DICTIONARY, defs=hybrid([bp([0] * 17)], 1))
    out.append(_chunk_case("hy_all_null_no_index", INT64, 1, [dpage, pa_, pn, pb, pn2], ra + [None] * 300 + rb_ + [None] * 17,
                           {"page_all_null_no_index", "page_all_null"}))
    # RLE-encoded BOOLEAN values (u32 length, then the hybrid at width 1), mixed runs, v1 and v2
    pages, rows = [], []
    for v2 in (False, True):
        def_runs = [rle(7, 1), bp([1, 0, 0, 1, 1, 1, 0, 1] * 3), rle(5, 0), rle(90, 1), bp([1, 1, 0, 1])]
        n = 7 + 24 + 5 + 90 + 4
        defs = expand(def_runs, n)
        nn = sum(defs)
        val_runs = [rle(3, 1), bp([0, 1, 1, 0, 1, 0, 0, 1] * 2), rle(60, 0), bp([1] * 8), rle(1, 1), bp([0, 0, 1, 1, 1, 0, 1, 0] * 4)]
        vals = expand(val_runs, nn)
        body = hybrid(val_runs, 1)
        body = struct.pack("<I", len(body)) + body
        pages.append(page_v2(body, n, n - nn, RLE, defs=hybrid(def_runs, 1)) if v2 else page_v1(body, n, RLE, defs=hybrid(def_runs, 1)))
        rows += _rows(defs, [bool(v) for v in vals])
    out.append(_chunk_case("hy_bool_rle", BOOLEAN, 1, pages, rows, {"bool_rle", "bool_bp", "bool_bp_overshoot", "page_v1_rle", "page_v2_rle"}))
    return out


def _mixed_cases():
    """dictionary page, v1 dictionary-encoded, v2 dictionary-encoded stored (is_compressed = false), v2
    compressed, v1 PLAIN fallback: one chunk under every codec, nullable INT64 and BYTE_ARRAY."""
    out = []
    for ptype in (INT64, BYTE_ARRAY):
        for codec in (UNCOMPRESSED, SNAPPY, LZ4_RAW, ZSTD):
            rng = np.random.default_rng(25)
            if ptype == INT64:
                dic = [int(x) for x in rng.integers(-2**63, 2**63 - 1, 50)]
                fresh = lambda k: [int(x) for x in rng.integers(-2**63, 2**63 - 1, k)]  # noqa: E731
            else:
                dic = [rng.integers(97, 123, int(ln), dtype=np.uint8).tobytes() for ln in rng.integers(0, 40, 50)]
                fresh = lambda k: [rng.integers(65, 91, int(ln), dtype=np.uint8).tobytes() for ln in rng.integers(0, 300, k)]  # noqa: E731
            pages, rows = [page_dict(plain(ptype, dic), 50, codec)], []
            for v2, kw in ((False, {}), (True, {"is_compressed": False}), (True, {})):
                def_runs = [rle(40, 1), bp([int(x) for x in rng.integers(0, 2, 400)]), rle(33, 0), rle(300, 1)]
                n = 773
                nn = sum(expand(def_runs, n))
                a = nn // 3
                idx_runs = [bp([int(x) for x in rng.integers(0, 50, a)]), rle(a, 49), bp([int(x) for x in rng.integers(0, 50, nn - 2 * a)])]
                pg, r = _dict_page_pair(dic, n, def_runs, idx_runs, 6, v2=v2, codec=codec, **kw)
                pages.append(pg)
                rows += r
            defs = [int(x) for x in rng.integers(0, 4, 500) > 0]
            vals = fresh(sum(defs))
            pages.append(page_v1(plain(ptype, vals), 500, PLAIN, codec, defs=hybrid([bp(defs)], 1)))
            rows += _rows(defs, vals)
            claims = {"mixed_order_%s_%s" % (CODEC_NAME[codec], "int64" if ptype == INT64 else "byte_array")}
            if codec != UNCOMPRESSED:
                claims |= {"page_v2_compressed", "page_v2_dict_flag_uncompressed"}
            out.append(_chunk_case("mixed_%s_%s" % ("int64" if ptype == INT64 else "byte_array", CODEC_NAME[codec]), ptype, 1, pages, rows,
                                   claims, codec))
    return out


def _flba_cases():
    """PLAIN FIXED_LEN_BYTE_ARRAY decimals of every length 1..16, required (two pages, the second
    one value long) and nullable (v1 and v2): the extremes of the length, minus one, zero, and the
    two patterns whose second byte carries the sign of a value one byte shorter."""
    rng = np.random.default_rng(26)
    out = []
    for t in range(1, 17):
        pats = [b"\x80" + bytes(t - 1), b"\x7f" + b"\xff" * (t - 1), b"\xff" * t, bytes(t)]
        names = {"flba_min", "flba_max", "flba_minus1", "flba_zero"}
        if t > 1:
            pats += [b"\x00\x80" + bytes(t - 2), b"\xff\x7f" + b"\xff" * (t - 2)]
            names |= {"flba_0080", "flba_ff7f"}
        vals = pats + [rng.integers(0, 256, t, dtype=np.uint8).tobytes() for _ in range(300)] + pats[::-1]
        ints = [int.from_bytes(v, "big", signed=True) for v in vals]
        pages = [page_v1(plain(FLBA, vals), len(vals), PLAIN), page_v1(pats[0], 1, PLAIN)]
        out.append(_chunk_case("flba_%d_required" % t, FLBA, 0, pages, ints + [ints[0]], names | {"flba_%d_required" % t}, tlen=t))
        defs = [1] * len(pats) + [int(x) for x in rng.integers(0, 3, 300) > 0] + [1] * len(pats)
        nv = [v for v, d in zip(vals, defs) if d]
        rows = _rows(defs, [int.from_bytes(v, "big", signed=True) for v in nv])
        d = hybrid([bp(defs)], 1)
        pages = [page_v1(plain(FLBA, nv), len(defs), PLAIN, defs=d), page_v2(plain(FLBA, nv), len(defs), len(defs) - len(nv), PLAIN, defs=d)]
        out.append(_chunk_case("flba_%d_nullable" % t, FLBA, 1, pages, rows + rows, names | {"flba_%d_nullable" % t}, tlen=t))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = _snappy_cases() + _lz4_cases() + _sweep_cases() + _hybrid_cases() + _mixed_cases() + _flba_cases()
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


def stream_cases(codec):
    """The single-page stream cases of a codec, in table order."""
    return [c for c in cases() if c.codec == codec and len(c.streams) == 1]


# ---- malformed pages: each aimed at one check --------------------------------------------------------
# stream, size: a stream case's compressed bytes and the output size its page header declares; lib:
# libsnappy / liblz4 refuse the stream (liblz4 as pyarrow calls it reports neither a short output
# nor an offset of 0); reason: what is wrong, and where lib is false the walker assertion (a
# substring of its message) that refuses the stream or the chunk
Malformed = namedtuple("Malformed", "name codec ptype max_def chunk target reason stream size lib")


@functools.lru_cache(maxsize=None)
def malformed_good():
    """The chunk the hybrid and page-level malformed cases are one edit away from: (chunk, rows)."""
    pages, rows = malformed_hybrid(None)
    return b"".join(pages), rows


def malformed_hybrid(edit):
    """A nullable INT64 dictionary chunk of one v1 page; `edit` names the one thing wrong with it."""
    dic = [11, -22, 33, -44, 55, -66, 77, -88]
    def_runs = [rle(12, 1), bp([1, 0, 1, 1, 0, 1, 1, 1]), rle(20, 1)]
    n = 40
    nn = sum(expand(def_runs, n))  # 38
    idx_runs = [rle(6, 7), bp([0, 1, 2, 3, 4, 5, 6, 7] * 2), rle(16, 2)]
    bw = 3
    defs, idx = hybrid(def_runs, 1), hybrid(idx_runs, bw)
    level_len = None
    if edit == "header_varint_6":
        idx = uvarint(6 << 1, pad=5) + idx[1:]
    elif edit == "rle_run_0":
        idx = hybrid([rle(6, 7), rle(0, 1)] + idx_runs[1:], bw)
    elif edit == "bp_groups_2p29":  # a header of 2^32 values over the bytes of every value that remains
        idx = hybrid([rle(6, 7), bp([0, 1, 2, 3, 4, 5, 6, 7] * 4, groups=1 << 29)], bw)
    elif edit == "def_bp_groups_2p29":
        defs = hybrid([rle(12, 1), bp([1, 0, 1, 1, 0, 1, 1, 1] + [1] * 20, groups=1 << 29)], 1)
    elif edit == "run_past_section":  # the last run's value byte is gone
        idx = idx[:-1]
    elif edit == "bp_past_section":  # 16 of the 32 values that remain, in a run that claims 4 groups
        idx = hybrid([rle(6, 7), bp([0, 1, 2, 3, 4, 5, 6, 7] * 2, groups=4)], bw)
    elif edit == "level_len_past_page":
        level_len = len(defs) + 1 + len(idx) + 1
    elif edit == "index_eq_dict_size":
        dic = dic[:7]
    elif edit == "bit_width_33":
        bw = 33
    if edit is not None and edit.startswith("wide_"):  # width 21..32: the good index, and its twin with the top bit
        bw = int(edit.split("_")[1])
        idx_runs = [rle(6, 7), bp([0, 1, 2, 3, 4, 5, 6, 7] * 2), rle(16, 2 | (1 << (bw - 1) if edit.endswith("_high") else 0))]
        idx = hybrid(idx_runs, bw)
    pages = [page_dict(plain(INT64, dic), len(dic)), page_v1(bytes([bw]) + idx, n, RLE_DICTIONARY, defs=defs, level_len=level_len)]
    rows = _rows(expand(def_runs, n), [dic[i & 7] for i in expand(idx_runs, nn)]) if edit is None or edit.endswith("_low") else None
    return pages, rows


WIDE = tuple(range(21, 33))


@functools.lru_cache(maxsize=None)
def wide_good():
    """name -> (chunk, rows): the malformed width twins' good halves (small indices at widths 21..32)."""
    out = {}
    for bw in WIDE:
        pages, rows = malformed_hybrid("wide_%d_low" % bw)
        out["wide_%d_low" % bw] = (b"".join(pages), rows)
    return out


@functools.lru_cache(maxsize=None)
def malformed():
    rng = np.random.default_rng(27)
    rb = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    out = []

    def stream(name, codec, s, size, reason, lib=True):
        pg = header_v1(size // 8, size, len(s), PLAIN) + s
        out.append(Malformed(name, codec, INT64, 0, pg, "i64", reason, s, size, lib))

    # Snappy: the good page is [40 literals][copy 2, off 40, 24 bytes] -> 64 bytes
    l40 = rb(40)
    good = [lit(l40), copy(2, 40, 24)]
    stream("sn_preamble_ne_page", SNAPPY, snappy(good, preamble=72)[0], 64, "the preamble says 72 bytes, the page header 64")
    stream("sn_copy_off_0", SNAPPY, snappy([lit(l40), copy(2, 0, 24)], check=False)[0], 64, "copy offset 0")
    stream("sn_copy_off_w_plus_1", SNAPPY, snappy([lit(l40), copy(2, 41, 24)], check=False)[0], 64, "copy offset one past the output's start")
    stream("sn_output_short", SNAPPY, snappy([lit(l40), copy(2, 40, 23)], preamble=64)[0], 64, "63 bytes of output for 64")
    stream("sn_output_long", SNAPPY, snappy([lit(l40), copy(2, 40, 25)], preamble=64)[0], 64, "65 bytes of output for 64")
    stream("sn_output_long_literal", SNAPPY, snappy([lit(l40), copy(2, 40, 23), lit(b"ab")], preamble=64)[0], 64, "a literal past the output")
    stream("sn_tag_cut_copy", SNAPPY, snappy(good)[0][:-1], 64, "the stream ends inside a copy tag")
    stream("sn_tag_cut_literal", SNAPPY, snappy([lit(l40), copy(2, 40, 23)], preamble=64)[0] + bytes([62 << 2, 0]), 64,
           "the stream ends inside a literal's length bytes")
    # LZ4: the good page is [40 literals][off 17, 19 bytes][5 literals] -> 64 bytes
    t5 = rb(5)
    stream("lz_chain_off_end", LZ4_RAW, lz4([(l40, 17, 19), (b"", 0, 0)])[0][:-1] + b"\xf0\xff\xff", 64, "a length chain runs off the block")
    stream("lz_ml_chain_off_end", LZ4_RAW, lz4_sequence(l40, 17, 19)[:-1] + b"\xff", 64,
           "a match length chain runs off the block")
    stream("lz_offset_past_output", LZ4_RAW, lz4([(l40, 41, 19), (t5, 0, 0)], check=False)[0], 64, "match offset one past the output's start")
    stream("lz_offset_0", LZ4_RAW, lz4([(l40, 0, 19), (t5, 0, 0)], check=False)[0], 64, "match offset 0 at output 40", lib=False)
    stream("lz_output_short", LZ4_RAW, lz4([(l40, 17, 18), (t5, 0, 0)])[0], 64, "output 63, expected 64", lib=False)
    stream("lz_output_long", LZ4_RAW, lz4([(l40, 17, 20), (t5, 0, 0)])[0], 64, "65 bytes of output for 64")
    stream("lz_offset_cut", LZ4_RAW, lz4_sequence(l40, 17, 10)[:-1], 64, "the block ends inside an offset")
    # the hybrid and the page: the walker's assertion that names the fault
    for edit, reason in (("header_varint_6", "run header varint"), ("rle_run_0", "RLE run of length 0"),
                         ("bp_groups_2p29", "bit-packed count past 32 bits"), ("def_bp_groups_2p29", "bit-packed count past 32 bits"),
                         ("run_past_section", "RLE value past the section"), ("bp_past_section", "bit-packed run past the section"),
                         ("level_len_past_page", "v1 level length past the page"),
                         ("index_eq_dict_size", "dictionary index past the dictionary"), ("bit_width_33", "bit width")):
        out.append(Malformed("hy_" + edit, UNCOMPRESSED, INT64, 1, b"".join(malformed_hybrid(edit)[0]), "i64", reason, None, 0, False))
    for bw in WIDE:
        out.append(Malformed("hy_wide_%d_high" % bw, UNCOMPRESSED, INT64, 1, b"".join(malformed_hybrid("wide_%d_high" % bw)[0]), "i64",
                             "dictionary index past the dictionary", None, 0, False))
    names = [m.name for m in out]
    assert len(set(names)) == len(names)
    return tuple(out)
