"""Columns built by hand to reach every path of the device ORDER BY ... LIMIT (csrc/sort.hip), and a
CPU replay of its two host loops that says which path a case reaches.

A case is (name, columns, asc, nulls_first, limit, claims) plus how it is run: `entry` "single"
(dbg_sort_limit_indices; its numeric cases also go through dbg_sort_limit_multi with one column) or
"multi" (dbg_sort_limit_multi), `raises` (the entry point answers Unsupported: min(limit, rows) is
above SORT_CAP — the 2049-row column asked for all its rows, and the NULL-boundary limits that
fall beyond 2048 of the 3000 rows), `expected` (a closed form where the comparator reference would
be too slow), and `voff` / `doff` (validity and Boolean value bitmaps passed at a bit offset).

`claims` names the path the case is built for; predict() replays sort_limit_run /
sort_multi_limit_run from a model of the composite key and check_claims() compares.  The model
key is the kernel's trick (sign flips, byte groups); the expected row order never comes from it
but from tests/sort_ref.py, and tests/test_sort_cases.py checks the two against each other.

The single-column levels: 0 = null rank, 1..8 = order-key bytes (most significant first), 9..12 =
row-index bytes.  The multi steps: (word, byte), word W = the row index.  Per step the replay
records ("skipped" | "hist" | "stop", chosen digit, non-empty buckets).
"""
import functools
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from databend_amd import abi
from databend_amd import column as col
from databend_amd.column import Column

SORT_CAP = 2048  # csrc/sort.hpp
SORT_MAX_COLS = 8
KEY_LEVELS = list(range(1, 9))  # the single-column levels that hold the order-key bytes


@dataclass
class Case:
    name: str
    columns: list
    asc: tuple
    nulls_first: tuple
    limit: Optional[int]
    claims: dict
    entry: str = "single"
    raises: bool = False
    expected: Optional[list] = None
    voff: int = 0
    doff: int = 0
    _order: dict = field(default_factory=dict, repr=False)  # shared by the cases of one family


# ------------------------------------------------------------------------------------------
# the key model and the replay of the two host loops
# ------------------------------------------------------------------------------------------
def valid_mask(c: Column) -> np.ndarray:
    if c.validity is None or not c.dtype.nullable:
        return np.ones(len(c), bool)
    return np.asarray(c.validity, bool)


def order_key(c: Column) -> np.ndarray:
    """sort_key() for ASC: a u64 whose unsigned order is the value order."""
    t = c.dtype.type_id
    v = np.asarray(c.data)
    top = np.uint64(1 << 63)
    if t == abi.FLOAT64:
        b = v.view(np.uint64)
        return np.where(b >> np.uint64(63) != 0, ~b, b | top)
    if t == abi.FLOAT32:
        b = v.view(np.uint32)
        return np.where(b >> np.uint32(31) != 0, ~b, b | np.uint32(1 << 31)).astype(np.uint64)
    if t in (abi.UINT8, abi.UINT16, abi.UINT32, abi.UINT64, abi.BOOLEAN):
        return v.astype(np.uint64)
    return v.astype(np.int64).view(np.uint64) ^ top


def _pick(h, need):
    cum = 0
    for d in range(256):
        if cum + int(h[d]) >= need:
            return d, cum
        cum += int(h[d])
    raise AssertionError("fewer rows in play than needed")


def predict_single(c: Column, asc: bool, nulls_first: bool, limit) -> dict:
    """sort_limit_run's host loop."""
    n = len(c)
    need = n if limit is None else min(int(limit), n)
    if need == 0:
        return {"path": "empty"}
    if need > SORT_CAP:
        return {"path": "unsupported"}
    if n <= SORT_CAP:
        return {"path": "direct"}
    valid = valid_mask(c)
    has_nulls = c.dtype.nullable and c.validity is not None
    ok = order_key(c)
    if not asc:
        ok = ~ok
    ok = np.where(valid, ok, np.uint64(0))
    nr = (valid == bool(nulls_first)).astype(np.uint32)
    ix = np.arange(n, dtype=np.uint32)
    play = np.ones(n, bool)
    steps, stop, common, common_val = {}, None, None, 0
    level = 0 if has_nulls else 1
    while level <= 12:
        if 1 <= level <= 8:
            sh = 8 * (8 - level)
            if common is None:
                a, o = int(np.bitwise_and.reduce(ok[play])), int(np.bitwise_or.reduce(ok[play]))
                common, common_val = ~(a ^ o) & (2**64 - 1), a
            if (common >> sh) & 255 == 255:
                steps[level] = ("skipped", (common_val >> sh) & 255, 1)
                level += 1
                continue
            digit = ((ok >> np.uint64(sh)) & np.uint64(255)).astype(np.int64)
        elif level == 0:
            digit = nr.astype(np.int64)
        else:
            digit = ((ix >> np.uint32(8 * (12 - level))) & np.uint32(255)).astype(np.int64)
        h = np.bincount(digit[play], minlength=256)
        d, cum = _pick(h, need)
        play &= digit == d
        need -= cum
        if int(h[d]) == need:
            steps[level] = ("stop", d, int(np.count_nonzero(h)))
            stop = level
            break
        steps[level] = ("hist", d, int(np.count_nonzero(h)))
        level += 1
    return {"path": "select", "steps": steps, "stop": stop}


def _string_groups(s: bytes, inv: int) -> bytes:
    groups = max(1, (len(s) + 7) // 8)
    out = bytearray()
    for g in range(groups):
        part = s[8 * g:8 * g + 8]
        out += part + bytes(8 - len(part))
        out.append(9 if g + 1 < groups else len(part))
    return bytes(x ^ inv for x in out)


def multi_keys(columns, asc, nulls_first, null_string_by_length=False):
    """Per row the composite key's bytes under the rule "a NULL String is one zero group", and
    whether some fixed-width value starts off a word boundary.  null_string_by_length: the
    encoding this rule replaced, as many zero groups as the bytes under the NULL would fill."""
    n = len(columns[0])
    parts, fixed = [], []
    for c, a, nf in zip(columns, asc, nulls_first):
        t = c.dtype.type_id
        valid = valid_mask(c)
        inv = 0 if a else 0xFF
        if t == abi.STRING:
            o = [int(x) for x in c.offsets]
            raw = np.ascontiguousarray(c.data).tobytes()
            enc = [_string_groups(raw[o[i]:o[i + 1]], inv) if valid[i]
                   else bytes(9 * max(1, (o[i + 1] - o[i] + 7) // 8) if null_string_by_length else 9) for i in range(n)]
        elif t == abi.DECIMAL128:
            raw = np.ascontiguousarray(c.data).tobytes()
            enc = []
            for i in range(n):
                v = int.from_bytes(raw[16 * i:16 * i + 16], "little", signed=True) + (1 << 127)
                enc.append(bytes(x ^ inv for x in v.to_bytes(16, "big")) if valid[i] else bytes(16))
        else:
            k = order_key(c)
            raw = (k if a else ~k).astype(">u8").tobytes()
            enc = [raw[8 * i:8 * i + 8] if valid[i] else bytes(8) for i in range(n)]
        if c.dtype.nullable:
            enc = [bytes([1 if bool(valid[i]) == bool(nf) else 0]) + e for i, e in enumerate(enc)]
        parts.append(enc)
        fixed.append(t != abi.STRING)
    keys, straddle = [], False
    for i in range(n):
        pos = 0
        for enc, fx, c in zip(parts, fixed, columns):
            if fx and (pos + (1 if c.dtype.nullable else 0)) % 8:
                straddle = True
            pos += len(enc[i])
        keys.append(b"".join(enc[i] for enc in parts))
    return keys, straddle


def predict_multi(columns, asc, nulls_first, limit) -> dict:
    """sort_multi_limit_run's host loop."""
    n = len(columns[0])
    need = n if limit is None else min(int(limit), n)
    if need == 0:
        return {"path": "empty"}
    if need > SORT_CAP:
        return {"path": "unsupported"}
    keys, straddle = multi_keys(columns, asc, nulls_first)
    W = (max(len(k) for k in keys) + 7) // 8
    out = {"W": W, "straddle": straddle}
    if n <= SORT_CAP:
        return dict(out, path="direct")
    words = np.frombuffer(b"".join(k + bytes(8 * W - len(k)) for k in keys), ">u8").reshape(n, W).astype(np.uint64)
    ix = np.arange(n, dtype=np.uint32)
    play = np.ones(n, bool)
    steps, stop = {}, None
    for w in range(W + 1):
        if w < W:
            a, o = int(np.bitwise_and.reduce(words[play, w])), int(np.bitwise_or.reduce(words[play, w]))
            common = ~(a ^ o) & (2**64 - 1)
        for b in range(8 if w < W else 4):
            if w < W:
                sh = 8 * (7 - b)
                if (common >> sh) & 255 == 255:
                    steps[(w, b)] = ("skipped", (a >> sh) & 255, 1)
                    continue
                digit = ((words[:, w] >> np.uint64(sh)) & np.uint64(255)).astype(np.int64)
            else:
                digit = ((ix >> np.uint32(8 * (3 - b))) & np.uint32(255)).astype(np.int64)
            h = np.bincount(digit[play], minlength=256)
            d, cum = _pick(h, need)
            play &= digit == d
            need -= cum
            if int(h[d]) == need:
                steps[(w, b)] = ("stop", d, int(np.count_nonzero(h)))
                stop = (w, b)
                break
            steps[(w, b)] = ("hist", d, int(np.count_nonzero(h)))
        if stop is not None:
            break
    assert stop is not None, "the selection did not converge"
    return dict(out, path="select", steps=steps, stop=stop)


def predict(case: Case) -> dict:
    if case.entry == "single":
        return predict_single(case.columns[0], case.asc[0], case.nulls_first[0], case.limit)
    return predict_multi(case.columns, case.asc, case.nulls_first, case.limit)


def check_claims(pred: dict, claims: dict) -> list:
    """The claims the prediction does not bear out (empty: all hold)."""
    bad = []
    steps = pred.get("steps", {})
    kinds = {k: {s for s, v in steps.items() if v[0] == k} for k in ("skipped", "hist", "stop")}
    for key, want in claims.items():
        if key in ("path", "stop", "straddle"):
            ok = pred.get(key) == want
        elif key == "deeper_than":  # the loop went past this step
            ok = pred.get("stop") is not None and pred["stop"] > want
        elif key in ("skipped", "hist"):
            ok = set(want) <= kinds[key]
        elif key == "digit":
            ok = all(s in steps and steps[s][1] == d for s, d in want.items())
        elif key == "many":  # steps whose histogram has more than one non-empty bucket
            ok = all(s in steps and steps[s][2] > 1 for s in want)
        elif key == "none_skipped":
            ok = pred.get("path") == "select" and not kinds["skipped"]
        elif key == "W_min":
            ok = pred.get("W", 0) >= want
        elif key == "stop_word":  # multi: the word of the stop; "row" = the row index
            ok = pred.get("stop") is not None and pred["stop"][0] == (pred["W"] if want == "row" else want)
        else:
            ok = False
        if not ok:
            bad.append((key, want))
    return bad


# ------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------
def _family(out, name, columns, asc, nulls_first, limits, entry="single", **kw):
    """One case per (limit, claims[, raises]) over the same columns; they share one reference order."""
    shared = {}
    if not isinstance(asc, tuple):
        asc, nulls_first = (asc,), (nulls_first,)
    for item in limits:
        limit, claims = item[0], item[1]
        raises = len(item) > 2 and item[2]
        out.append(Case("%s-limit%s" % (name, "all" if limit is None else limit), columns, asc, nulls_first, limit,
                        claims, entry=entry, raises=raises, _order=shared, **kw))


def level_column(dt, L, n, k, rng):
    """Order-key bytes above L equal in every row, byte L 0x10 in k rows and 0x20 in the rest,
    the bytes below random (L = 1: the most significant byte)."""
    v = np.zeros(n, np.uint64)
    for byte in range(1, 9):
        sh = np.uint64(8 * (8 - byte))
        if byte < L:
            b = np.full(n, 0x11, np.uint64)
        elif byte == L:
            b = np.full(n, 0x20, np.uint64)
            b[rng.permutation(n)[:k]] = 0x10
        else:
            b = rng.integers(0, 256, n).astype(np.uint64)
        v |= b << sh
    return Column.from_numbers(dt, v.view(np.int64) if dt.type_id == abi.INT64 else v)


F32 = dict(zero=0, inf=0x7F800000, big=0x7F7FFFFF, den_min=1, den_max=0x007FFFFF, nan_1=0x7F800001,
           nan_quiet=0x7FC00000, nan_ones=0x7FFFFFFF)
F64 = dict(zero=0, inf=0x7FF0 << 48, big=(0x7FF0 << 48) - 1, den_min=1, den_max=(1 << 52) - 1, nan_1=(0x7FF0 << 48) + 1,
           nan_quiet=0x7FF8 << 48, nan_ones=(1 << 63) - 1)

NUMBER_TYPES = [("i8", col.Int8), ("i16", col.Int16), ("i32", col.Int32), ("i64", col.Int64), ("u8", col.UInt8),
                ("u16", col.UInt16), ("u32", col.UInt32), ("u64", col.UInt64), ("date", col.Date), ("ts", col.Timestamp)]


def _extremes(kind, dt, n, rng):
    """Each extreme value three times, shuffled, padded with mid values to n rows."""
    if kind == "bool":
        vals = np.array([False, True] * 3)
        pad = rng.random(max(0, n - len(vals))) < 0.5
    elif kind in ("f32", "f64"):
        table, ut, ft, sign = (F32, np.uint32, np.float32, 1 << 31) if kind == "f32" else (F64, np.uint64, np.float64, 1 << 63)
        vals = np.array([b | s for b in table.values() for s in (0, sign)] * 3, ut)
        pad = rng.normal(size=max(0, n - len(vals))).astype(ft).view(ut)
    else:
        info = np.iinfo(dt.np_dtype)
        ext = [info.min, info.max, 0, 1] + ([-1] if info.min < 0 else [])
        vals = np.array(ext * 3, dt.np_dtype)
        pad = rng.integers(2, 100, max(0, n - len(vals))).astype(dt.np_dtype)
    v = np.concatenate([vals, pad])[:max(n, len(vals))]
    v = v[rng.permutation(len(v))]
    if kind == "bool":
        return Column.from_bools(v)
    if kind in ("f32", "f64"):
        return Column(dt, v.view(ft))  # from bit patterns: numpy never sees the NaNs as numbers
    return Column.from_numbers(dt, v)


def _single_cases(out):
    rng = np.random.default_rng(2048)
    # cap boundary: <= SORT_CAP rows go straight to the bitonic sort
    for n in (1, 2, 2047, 2048):
        c = Column.from_numbers(col.Int64, rng.integers(-50, 50, n))
        limits = sorted({1, n - 1, n, n + 5}) + [None]
        _family(out, "cap-n%d" % n, [c], True, False, [(k, {"path": "empty" if k == 0 else "direct"}) for k in limits])
    c = Column.from_numbers(col.Int64, rng.integers(-50, 50, 2049))
    _family(out, "cap-n2049", [c], True, False,
            [(1, {"path": "select"}), (2048, {"path": "select"}), (2049, {"path": "unsupported"}, True),
             (None, {"path": "unsupported"}, True)])
    # break at level L
    k = 1000
    for tag, dt in (("i64", col.Int64), ("u64", col.UInt64)):
        for L in range(1, 9):
            c = level_column(dt, L, 4096, k, rng)
            skipped = list(range(1, L))
            _family(out, "level%d-%s" % (L, tag), [c], True, False,
                    [(k - 1, {"deeper_than": L, "skipped": skipped, "hist": [L]}),
                     (k, {"stop": L, "skipped": skipped}),
                     (k + 1, {"deeper_than": L, "skipped": skipped, "hist": [L]})])
    # nothing common
    c = Column.from_numbers(col.UInt64, rng.integers(0, 2**64 - 1, 4096, dtype=np.uint64, endpoint=True))
    _family(out, "nothing-common", [c], True, False, [(1, {"hist": [1], "none_skipped": True}), (2048, {"hist": [1], "none_skipped": True})])
    # all equal: every key byte common, the row-index levels decide
    c = Column.from_numbers(col.UInt64, np.full(70_000, 7, np.uint64))
    _family(out, "all-equal", [c], True, False,
            [(1, {"skipped": KEY_LEVELS, "stop": 12, "many": [10, 11, 12]}), (255, {"skipped": KEY_LEVELS, "stop": 12}),
             (256, {"skipped": KEY_LEVELS, "stop": 11}), (257, {"skipped": KEY_LEVELS, "stop": 12, "digit": {11: 1}}),
             (2048, {"skipped": KEY_LEVELS, "stop": 11, "digit": {11: 7}})])
    # two values with heavy ties: the limit cuts inside a tie group
    v = np.full(5000, 9, np.int32)
    v[rng.permutation(5000)[:1000]] = 3
    c = Column.from_numbers(col.Int32, v)
    _family(out, "ties-asc", [c], True, False, [(700, {"deeper_than": 8}), (1500, {"deeper_than": 8})])
    _family(out, "ties-desc", [c], False, False, [(700, {"deeper_than": 8}), (1500, {"deeper_than": 8})])
    # index byte 3: the threshold row is at or above 2^24
    v = np.ones(2**24 + 300, np.uint8)
    v[2**24:] = 0
    out.append(Case("index-byte3", [Column.from_numbers(col.UInt8, v)], (True,), (False,), 100,
                    {"stop": 12, "digit": {9: 1}, "skipped": list(range(1, 8)), "hist": [8]},
                    expected=list(range(2**24, 2**24 + 100))))
    # NULL boundary: the data is distinct and descending, also under the NULLs.  The boundary lies
    # at nv rows with NULLs last and at n - nv with NULLs first, and a select serves at most
    # SORT_CAP = 2048 of the 3000 rows: nv = 100 reaches it with NULLs last (limits 99..101) and
    # nv = 2900 with NULLs first (again 99..101).  The other two pairings put all three limits
    # (2899..2901) above SORT_CAP, so those six cases can only be asked to raise Unsupported.
    n = 3000
    for nv in (100, 2900):
        valid = np.zeros(n, bool)
        valid[rng.permutation(n)[:nv]] = True
        c = Column.from_numbers(col.Int64, 10_000 - np.arange(n), valid)
        for nf, edge in ((False, nv), (True, n - nv)):
            fam = []
            for k in (edge - 1, edge, edge + 1):
                if k > SORT_CAP:
                    fam.append((k, {"path": "unsupported"}, True))
                elif k == edge:
                    fam.append((k, {"stop": 0}))
                elif k < edge:
                    fam.append((k, {"deeper_than": 0, "digit": {0: 0}}))
                else:  # the first row of rank 1: NULLs last -> the first NULL, by row index alone
                    fam.append((k, {"digit": {0: 1}, "skipped": KEY_LEVELS if not nf else []}))
            _family(out, "nulledge-nv%d-%s" % (nv, "first" if nf else "last"), [c], True, nf, fam)
    data = 10_000 - np.arange(n)
    c = Column.from_numbers(col.Int64, data, np.zeros(n, bool))
    _family(out, "all-null-last", [c], True, False, [(10, {"digit": {0: 1}, "skipped": KEY_LEVELS, "deeper_than": 8})])
    _family(out, "all-null-first", [c], False, True, [(10, {"digit": {0: 0}, "skipped": KEY_LEVELS, "deeper_than": 8})])
    c = Column.from_numbers(col.Int64, data, np.ones(n, bool))
    _family(out, "validity-all-ones", [c], True, False, [(50, {"digit": {0: 0}, "hist": [0]})])
    c = Column(col.Int64.wrap_nullable(), np.ascontiguousarray(data, np.int64), None, None)
    _family(out, "validity-none", [c], True, True, [(50, {"path": "select"})])
    # bitmaps at a bit offset
    for n, limit in ((300, None), (3000, 200)):
        path = {"path": "direct" if n <= SORT_CAP else "select"}
        valid = rng.random(n) < 0.7
        c = Column.from_numbers(col.Int32, rng.integers(-1000, 1000, n), valid)
        _family(out, "bitoffset-i32-n%d" % n, [c], True, False, [(limit, path)], voff=3)
        _family(out, "bitoffset-i32-desc-n%d" % n, [c], False, True, [(limit, path)], voff=3)
        c = Column.from_bools(rng.random(n) < 0.5, rng.random(n) < 0.7)
        _family(out, "bitoffset-bool-n%d" % n, [c], True, False, [(limit, path)], voff=3, doff=5)
        _family(out, "bitoffset-bool-desc-n%d" % n, [c], False, True, [(limit, path)], voff=3, doff=5)
    # types and extremes
    kinds = NUMBER_TYPES + [("bool", col.Boolean), ("f32", col.Float32), ("f64", col.Float64)]
    for kind, dt in kinds:
        small, padded = _extremes(kind, dt, 0, rng), _extremes(kind, dt, 2049, rng)
        for asc in (True, False):
            d = "asc" if asc else "desc"
            _family(out, "extremes-%s-%s-direct" % (kind, d), [small], asc, False, [(None, {"path": "direct"})])
            _family(out, "extremes-%s-%s-select" % (kind, d), [padded], asc, False, [(2048, {"path": "select"})])


def _tile(values, times, rng):
    v = list(values) * times
    return [v[i] for i in rng.permutation(len(v))]


def _multi_cases(out):
    rng = np.random.default_rng(9)
    sel, direct = {"path": "select"}, {"path": "direct"}
    # a NULL String before another column: the bytes under the NULLs are 0..40 long, and the Int64
    # grows with that length, so ordering by the garbage length (longer keys hold more zeros and
    # sort first) is the reverse of ordering by the Int64.  Few rows of the larger block are valid,
    # so that its limit reaches into the NULLs also where they come last.
    for n, limit in ((300, None), (3000, 500)):
        valid = rng.random(n) < (0.5 if n == 300 else 0.1)
        glen = rng.integers(0, 41, n)
        few = [b"", b"a", b"ab", b"abcdefgh", b"abcdefghi"]
        strs = [few[rng.integers(0, 5)] if valid[i] else bytes(rng.integers(1, 256, glen[i]).astype(np.uint8)) for i in range(n)]
        s = Column.from_strings(strs, validity=valid)
        i64 = Column.from_numbers(col.Int64, glen.astype(np.int64) * 100_000 + rng.permutation(n))
        i32 = Column.from_numbers(col.Int32, rng.integers(0, 3, n))
        claim = direct if n <= SORT_CAP else sel
        for asc in (True, False):
            for nf in (False, True):
                _family(out, "nullstr-%s-%s-n%d" % ("asc" if asc else "desc", "first" if nf else "last", n), [s, i64],
                        (asc, True), (nf, False), [(limit, claim)], entry="multi")
        _family(out, "nullstr-middle-n%d" % n, [i32, s, i64], (False, True, True), (False, False, False), [(limit, claim)],
                entry="multi")
    # String group edges
    base = bytes(range(0x41, 0x41 + 24))
    strs = []
    for L in (0, 1, 7, 8, 9, 15, 16, 17, 24):
        strs.append(base[:L])
        if L:
            strs += [base[:L - 1] + bytes([last]) for last in (0x00, 0x09, 0xFF, base[L - 1] + 1)]
    strs += [bytes([b]) * L for b in (0x00, 0x09, 0xFF) for L in (7, 8, 9, 16)]
    for tag, times, limit in (("small", 2, None), ("large", 48, 300)):
        v = _tile(strs, times, rng)
        s = Column.from_strings(v)
        i32 = Column.from_numbers(col.Int32, rng.integers(-3, 3, len(v)))
        claim = direct if len(v) <= SORT_CAP else sel
        for asc in (True, False):
            d = "asc" if asc else "desc"
            _family(out, "stredges-%s-%s" % (tag, d), [s], (asc,), (False,), [(limit, claim)], entry="multi")
            _family(out, "stredges-%s-%s-then-i32" % (tag, d), [s, i32], (asc, False), (False, False), [(limit, claim)], entry="multi")
    # a long common prefix: 28 whole words shared, the tail decides
    prefix = bytes(rng.integers(1, 256, 200).astype(np.uint8))
    s = Column.from_strings([prefix + b"%d" % x for x in rng.integers(0, 3000, 3000)])
    shared = [(w, b) for w in range(28) for b in range(8)]
    _family(out, "long-prefix", [s], (True,), (False,),
            [(1, {"W_min": 26, "skipped": shared, "deeper_than": (27, 7)}),
             (100, {"W_min": 26, "skipped": shared, "deeper_than": (27, 7)})], entry="multi")
    # Decimal128: differ in the high word only, in the low word only, the extremes; non-zero under NULLs
    vals = [k << 64 for k in (-3, -2, -1, 1, 2, 3)] + [0, 1, 2, 3, 2**64 - 1, 2**63] + [-2**127, 2**127 - 1, -1, 0]
    for tag, times, limit in (("small", 4, None), ("large", 160, 300)):
        v = _tile(vals, times, rng)
        valid = rng.random(len(v)) < 0.75
        d128 = Column.from_decimals(38, 0, v, validity=valid)
        claim = direct if len(v) <= SORT_CAP else sel
        for asc, nf in ((True, False), (False, True), (False, False)):
            _family(out, "decimal-%s-%s-%s" % (tag, "asc" if asc else "desc", "first" if nf else "last"), [d128], (asc,), (nf,),
                    [(limit, claim)], entry="multi")
    # eight nullable columns: every marker byte shifts the next value off the word boundary
    for n, limit in ((300, None), (3000, 500)):
        def two(dt, a, b):
            return Column.from_numbers(dt, np.where(rng.random(n) < 0.5, a, b).astype(dt.np_dtype), rng.random(n) < 0.9)
        cols = [two(col.Int8, -1, 1), two(col.UInt16, 0, 65535), two(col.Int32, -2**31, 7), two(col.Int64, -5, 2**40),
                two(col.Float32, -0.0, 0.0), two(col.Float64, -1.5, np.inf), two(col.Date, -1, 19000),
                Column.from_bools(rng.random(n) < 0.5, rng.random(n) < 0.9)]
        asc = (True, False, True, False, True, False, True, False)
        nf = (False, False, True, True, False, True, False, True)
        claim = dict(direct if n <= SORT_CAP else sel, straddle=True, W_min=9)
        _family(out, "eight-columns-n%d" % n, cols, asc, nf, [(limit, claim)], entry="multi")
    # every row equal on every column: the row index decides
    cols = [Column.from_numbers(col.Int32, np.full(70_000, 5, np.int32)), Column.from_strings([b"abc"] * 70_000)]
    _family(out, "all-rows-equal", cols, (True, False), (False, False),
            [(300, {"stop_word": "row"}), (2048, {"stop_word": "row"})], entry="multi")
    # the whole bucket taken in word 0, and in word 1 behind a constant column
    lev = level_column(col.UInt64, 3, 4096, 1000, rng)
    const = Column.from_numbers(col.Int64, np.full(4096, -3, np.int64))
    _family(out, "bucket-word0", [lev], (True,), (False,), [(1000, {"stop": (0, 2)}), (999, {"deeper_than": (0, 2)})], entry="multi")
    _family(out, "bucket-word1", [const, lev], (True, True), (False, False),
            [(1000, {"stop": (1, 2), "skipped": [(0, b) for b in range(8)]}), (1001, {"deeper_than": (1, 2)})], entry="multi")
    # mixed NULL placement
    for n, limit in ((500, None), (3000, 400)):
        a = Column.from_numbers(col.Int32, rng.integers(0, 3, n), rng.random(n) < 0.8)
        b = Column.from_strings([[b"x", b"xy", b"", b"xy\x00"][j] for j in rng.integers(0, 4, n)], validity=rng.random(n) < 0.8)
        c = Column.from_numbers(col.Float64, rng.integers(-2, 2, n).astype(np.float64), rng.random(n) < 0.8)
        _family(out, "mixed-nulls-n%d" % n, [a, b, c], (True, False, False), (False, True, False),
                [(limit, direct if n <= SORT_CAP else sel)], entry="multi")


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    out = []
    _single_cases(out)
    _multi_cases(out)
    names = [c.name for c in out]
    assert len(set(names)) == len(names), "duplicate case names"
    return tuple(out)


def case(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


def reference(c: Case) -> list:
    """The expected row indices: the closed form, or tests/sort_ref.py (one full order per family)."""
    from tests import sort_ref
    if c.expected is not None:
        return c.expected
    if "order" not in c._order:
        c._order["order"] = sort_ref.full_order(c.columns, c.asc, c.nulls_first)
    order = c._order["order"]
    return order if c.limit is None else order[:c.limit]


def runs_multi_too(c: Case) -> bool:
    """Single-column cases also go through dbg_sort_limit_multi with one column."""
    return c.entry == "single"


# ------------------------------------------------------------------------------------------
# block level: databend_amd.sort.sort over a block with payload columns
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def block():
    """(columns, {name: descriptions as (offset, asc, nulls_first)})."""
    rng = np.random.default_rng(500)
    n = 500
    words = [b"", b"k", b"key", b"key\x00", b"keys", b"longer than eight", b"longer than eight bytes"]
    cols = [
        Column.from_numbers(col.Int32, rng.integers(-20, 20, n)),
        Column.from_strings([words[j] for j in rng.integers(0, len(words), n)]),
        Column.from_strings([b"p%d" % x for x in rng.integers(0, 50, n)], validity=rng.random(n) < 0.8),
        Column.from_bools(rng.random(n) < 0.5),
        Column.from_decimals(38, 2, [int(x) * 10**20 for x in rng.integers(-9, 9, n)], validity=rng.random(n) < 0.8),
        Column.from_numbers(col.Float64, rng.normal(size=n)),
    ]
    sorts = {"by-number": [(0, False, False)], "by-string-int": [(1, True, False), (0, False, False)]}
    return cols, sorts


BLOCK_LIMITS = (0, 1, 37, None)
