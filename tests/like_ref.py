"""An independent reference for SQL LIKE as Databend's select path evaluates it, in plain Python
`bytes`.  Written from the rules of EXP/filter/like.rs (generate_like_pattern and the matcher of each
LikePattern class), not from databend_amd/csrc/like.hpp: slices, `bytes.find`, `startswith` /
`endswith` instead of index loops.

The reference's behaviour is the contract, quirks included:
  * any `_`, or `\\` followed by `%`, `_` or `\\`, makes a pattern Complex; a `\\` elsewhere only
    clears "simple" — so with no `%`, one leading or trailing `%`, or one of each, such a pattern is
    compared raw, the backslash a byte like any other
  * `%%` matches everything, the empty string too; a SimplePattern (`%%%`, `a%b`, ...) never matches ''
  * in a Complex pattern `_` is one BYTE, `\\` escapes the next pattern byte if there is one, and a
    mismatch goes back to the last `%`
  * a NULL cell is selected by neither LIKE nor NOT LIKE: the node's value is NULL there
"""
import numpy as np

from databend_amd.filter import _Like
from tests import pred_ref

ORDINAL, START_OF_PERCENT, END_OF_PERCENT, SURROUND_BY_PERCENT, SIMPLE, COMPLEX = range(6)
KIND_NAMES = ("OrdinalStr", "StartOfPercent", "EndOfPercent", "SurroundByPercent", "SimplePattern", "ComplexPattern")


def classify(pat: bytes):
    """-> (kind, has_start_percent, has_end_percent, segments); the last three only for SIMPLE."""
    pat = bytes(pat)
    if not pat:
        return ORDINAL, False, False, []
    has_start = pat[:1] == b"%"
    has_end = False
    simple = True
    percents = 1 if has_start else 0
    seg_from = 1 if has_start else 0
    segments = []
    i = seg_from
    while i < len(pat):
        c = pat[i:i + 1]
        if c == b"_":
            return COMPLEX, False, False, []
        if c == b"%":
            percents += 1
            if i > seg_from:
                segments.append(pat[seg_from:i])
            seg_from = i + 1
            has_end = has_end or i == len(pat) - 1
        elif c == b"\\":
            simple = False
            if i + 1 < len(pat):
                i += 1
                if pat[i:i + 1] in (b"%", b"_", b"\\"):
                    return COMPLEX, False, False, []
        i += 1
    if percents == 0:
        return ORDINAL, False, False, []
    if percents == 1 and has_start:
        return START_OF_PERCENT, False, False, []
    if percents == 1 and has_end:
        return END_OF_PERCENT, False, False, []
    if percents == 2 and has_start and has_end:
        return SURROUND_BY_PERCENT, False, False, []
    if not simple:
        return COMPLEX, False, False, []
    if seg_from < len(pat):
        segments.append(pat[seg_from:])
    return SIMPLE, has_start, has_end, segments


def kind(pat: bytes) -> int:
    return classify(pat)[0]


def _simple(s: bytes, has_start: bool, has_end: bool, segments) -> bool:
    if not s:
        return False
    segs = list(segments)
    pos = 0
    if not has_start:
        if not s.startswith(segs[0]):
            return False
        pos = len(segs[0])
        segs = segs[1:]
    for j, seg in enumerate(segs):
        if pos >= len(s):
            return False
        if j == len(segs) - 1 and not has_end:
            if len(s) - pos < len(seg) or not s.endswith(seg):
                return False
        else:
            at = s.find(seg, pos)
            if at < 0:
                return False
            pos = at + len(seg)
    return True


def _complex(s: bytes, pat: bytes) -> bool:
    px = tx = 0
    back_px = back_tx = 0  # where to resume after a mismatch: the last % and one byte further in s
    while px < len(pat) or tx < len(s):
        if px < len(pat):
            c = pat[px:px + 1]
            if c == b"_":
                if tx < len(s):
                    px, tx = px + 1, tx + 1
                    continue
            elif c == b"%":
                back_px, back_tx = px, tx + 1
                px += 1
                continue
            else:
                if c == b"\\" and px + 1 < len(pat):
                    px += 1
                if s[tx:tx + 1] == pat[px:px + 1] and tx < len(s):
                    px, tx = px + 1, tx + 1
                    continue
        if 0 < back_tx <= len(s):
            px, tx = back_px, back_tx
            continue
        return False
    return True


def matcher(pat: bytes):
    """The pattern classified once: a function bytes -> bool."""
    pat = bytes(pat)
    k, has_start, has_end, segments = classify(pat)
    if k == ORDINAL:
        return lambda s: s == pat
    if k == END_OF_PERCENT:
        return lambda s: s.startswith(pat[:-1])
    if k == START_OF_PERCENT:
        return lambda s: s.endswith(pat[1:])
    if k == SURROUND_BY_PERCENT:
        return lambda s: len(pat) <= 2 or pat[1:-1] in s
    if k == SIMPLE:
        return lambda s: _simple(s, has_start, has_end, segments)
    return lambda s: _complex(s, pat)


def match(s: bytes, pat: bytes) -> bool:
    return bool(matcher(pat)(bytes(s)))


def column_values(col) -> list:
    """The cells of a String column as bytes (a NULL row's bytes as stored)."""
    raw = bytes(np.asarray(col.data, np.uint8))
    o = [int(x) for x in col.offsets]
    return [raw[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def like_column(col, pat: bytes, n: int) -> np.ndarray:
    """The node's value per row in pred_ref's {FALSE, TRUE, NULL}."""
    vals = column_values(col)
    m = matcher(pat)
    truth = np.fromiter((m(vals[i]) for i in range(n)), dtype=bool, count=n)
    return pred_ref._tri(truth, pred_ref.validity(col, n))


def evaluate(pred, cols, n: int) -> np.ndarray:
    """pred_ref.evaluate for trees that may hold LIKE nodes (AND / OR / NOT compose as there)."""
    if isinstance(pred, _Like):
        return like_column(cols[pred.col], pred.pattern, n)
    if isinstance(pred, pred_ref._Bin):
        a, b = evaluate(pred.a, cols, n), evaluate(pred.b, cols, n)
        F, T, N = pred_ref.FALSE, pred_ref.TRUE, pred_ref.NULL
        if pred.op == pred_ref.abi.PRED_AND:
            return np.where((a == F) | (b == F), F, np.where((a == N) | (b == N), N, T)).astype(np.uint8)
        return np.where((a == T) | (b == T), T, np.where((a == N) | (b == N), N, F)).astype(np.uint8)
    if isinstance(pred, pred_ref._Un) and pred.op == pred_ref.abi.PRED_NOT:
        a = evaluate(pred.a, cols, n)
        return np.where(a == pred_ref.NULL, pred_ref.NULL, np.where(a == pred_ref.TRUE, pred_ref.FALSE, pred_ref.TRUE)).astype(np.uint8)
    return pred_ref.evaluate(pred, cols, n)


def select(pred, cols, n: int) -> np.ndarray:
    return np.flatnonzero(evaluate(pred, cols, n) == pred_ref.TRUE).astype(np.uint32)
