"""LIKE on the CPU: the Python reference (tests/like_ref.py) against a regex translation, the
reference implementation's own recorded results and its named quirks; then the library's host entry
points (dbg_like_pattern_kind, dbg_like_match_host: the host build of the source the kernels
compile, databend_amd/csrc/like.hpp) against the Python reference, exhaustively on short inputs and
on random inputs at the caps; and the same matcher as a stand-alone program under
-fsanitize=address,undefined.  All comparisons are exact.  The device side: tests/test_gpu_like.py."""
import ctypes as C
import functools
import itertools
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from databend_amd import abi
from databend_amd import column as col
from databend_amd.column import Column
from databend_amd.ffi import DbgError, lib
from databend_amd.filter import FilterProgram, and_, cmp, like, not_like
from tests import like_ref

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "databend_amd", "csrc")
GOLD = json.load(open(os.path.join(HERE, "golden", "like", "reference_like_results.json"), encoding="utf-8"))
SMALL = b"ab%_\\"


# ---- the Python reference itself ----------------------------------------------------------------
def regex_of(pat: bytes):
    parts = [b".*" if c == 0x25 else b"." if c == 0x5F else re.escape(bytes([c])) for c in pat]
    return re.compile(b"".join(parts), re.DOTALL)


def test_reference_equals_regex_without_backslash():
    """Random patterns over {a, b, c, %, _} and haystacks over {a, b, c, newline}: LIKE is the anchored
    regex with % -> .* and _ -> . (DOTALL, bytes), except that a SimplePattern never matches the empty
    haystack.  Those cases are left out: 60,000 draws with haystack lengths 0..9 leave out the
    SimplePattern patterns among the ~10 % empty haystacks, 1.8 % of the draws here (1,097 of 60,000; asserted < 5 %)."""
    rng = np.random.default_rng(21)
    pa, ha = b"abc%%_", b"abc\n"
    skipped = total = 0
    for _ in range(60_000):
        pat = bytes(pa[i] for i in rng.integers(0, len(pa), int(rng.integers(0, 8))))
        s = bytes(ha[i] for i in rng.integers(0, len(ha), int(rng.integers(0, 10))))
        total += 1
        if not s and like_ref.kind(pat) == like_ref.SIMPLE:
            skipped += 1
            continue
        assert like_ref.match(s, pat) == (regex_of(pat).fullmatch(s) is not None), (s, pat)
    assert 0 < skipped < 0.05 * total, (skipped, total)


QUIRKS = [
    ("empty_like_three_percents_is_false", b"", b"%%%", False),
    ("empty_like_two_percents_is_true", b"", b"%%", True),
    ("empty_like_one_percent_is_true", b"", b"%", True),
    ("raw_backslash_compare_ordinal", b"a\\b", b"a\\b", True),
    ("raw_backslash_compare_is_not_an_escape", b"ab", b"a\\b", False),
    ("raw_backslash_in_surround", b"xa\\by", b"%a\\b%", True),
    ("raw_backslash_prefix_and_suffix", b"a\\bz", b"a\\b%", True),
    ("underscore_is_one_byte_of_utf8", "é".encode(), b"_", False),
    ("two_underscores_for_two_byte_utf8", "é".encode(), b"__", True),
    ("escaped_percent", b"%", b"\\%", True),
    ("escaped_percent_is_not_a_wildcard", b"a", b"\\%", False),
    ("underscore_escaped_percent_percent", b"v%xx", b"_\\%%", True),
    ("trailing_backslash_is_itself", b"a\\", b"_\\", True),
    ("simple_pattern_nonempty", b"a", b"%%%", True),
]


@pytest.mark.parametrize("name,s,pat,exp", QUIRKS, ids=[q[0] for q in QUIRKS])
def test_quirks(name, s, pat, exp):
    assert like_ref.match(s, pat) is exp


SEGS = [b"databend", b"cloud", b"data", b"warehouse"]
CLASSIFY = [  # the eleven cases of the reference's test_generate_like_pattern
    (b"databend", like_ref.ORDINAL, None),
    (b"%databend", like_ref.START_OF_PERCENT, None),
    (b"databend%", like_ref.END_OF_PERCENT, None),
    (b"%databend%", like_ref.SURROUND_BY_PERCENT, None),
    (b"databend%cloud%data%warehouse", like_ref.SIMPLE, (False, False, SEGS)),
    (b"%databend%cloud%data%warehouse", like_ref.SIMPLE, (True, False, SEGS)),
    (b"databend%cloud%data%warehouse%", like_ref.SIMPLE, (False, True, SEGS)),
    (b"%databend%cloud%data%warehouse%", like_ref.SIMPLE, (True, True, SEGS)),
    (b"databend_cloud%data%warehouse", like_ref.COMPLEX, None),
    (b"databend\\%cloud%data%warehouse", like_ref.COMPLEX, None),
    (b"databend%cloud_data%warehouse", like_ref.COMPLEX, None),
]


@pytest.mark.parametrize("pat,kind,simple", CLASSIFY, ids=[c[0].decode() for c in CLASSIFY])
def test_classification_cases_of_the_reference(pat, kind, simple):
    got = like_ref.classify(pat)
    assert got[0] == kind
    if simple is not None:
        assert (got[1], got[2], got[3]) == simple
    assert lib_kind(pat) == kind


def test_recorded_results_of_the_reference():
    for s, pat, exp in GOLD["scalars"] + GOLD["rows"]:
        assert like_ref.match(s.encode(), pat.encode()) is exp, (s, pat)
        assert lib_match(s.encode(), pat.encode()) is exp, (s, pat)
    for case in GOLD["columns"]:
        pats = case.get("patterns") or [case["pattern"]] * len(case["lhs"])
        assert [like_ref.match(s.encode(), p.encode()) for s, p in zip(case["lhs"], pats)] == case["output"], case
        assert [lib_match(s.encode(), p.encode()) for s, p in zip(case["lhs"], pats)] == case["output"], case
    for pat, count in GOLD["counts"]:
        assert sum(like_ref.match(s.encode(), pat.encode()) for s in GOLD["table"]) == count, pat
        assert sum(lib_match(s.encode(), pat.encode()) for s in GOLD["table"]) == count, pat


# ---- the library's host entry points --------------------------------------------------------------
def lib_kind(pat: bytes) -> int:
    k = C.c_int32(-1)
    assert lib().dbg_like_pattern_kind(pat, len(pat), C.byref(k)) == abi.DBG_OK
    return k.value


def lib_match(s: bytes, pat: bytes) -> bool:
    out = C.c_int32(-1)
    assert lib().dbg_like_match_host(s, len(s), pat, len(pat), C.byref(out)) == abi.DBG_OK
    assert out.value in (0, 1)
    return out.value == 1


@functools.lru_cache(maxsize=None)
def short_strings():
    return [bytes(t) for n in range(5) for t in itertools.product(SMALL, repeat=n)]


@functools.lru_cache(maxsize=None)
def exhaustive_expected():
    """(kind, match) of every pattern x haystack of length <= 4 over {a, b, %, _, \\}: 781 x 781 cases,
    patterns outermost — computed once for the host entry points and the sanitizer program."""
    strs = short_strings()
    out = []
    for pat in strs:
        k, m = like_ref.kind(pat), like_ref.matcher(pat)
        out.append((k, [bool(m(s)) for s in strs]))
    return out


def test_host_entry_points_exhaustive_short_inputs():
    strs = short_strings()
    L = lib()
    out = C.c_int32()
    for pat, (k, exp) in zip(strs, exhaustive_expected()):
        assert lib_kind(pat) == k, pat
        got = []
        for s in strs:
            assert L.dbg_like_match_host(s, len(s), pat, len(pat), C.byref(out)) == abi.DBG_OK
            got.append(out.value == 1)
        assert got == exp, (pat, [s for s, g, e in zip(strs, got, exp) if g != e][:3])


def random_cases_at_the_caps(seed: int, n: int):
    """(haystack, pattern) pairs: patterns of up to the pattern cap and the segment cap, built from
    short segments joined by % (and sometimes _ or a backslash), haystacks built to match often."""
    rng = np.random.default_rng(seed)
    words = [b"a", b"ab", b"ba", b"abc", b"x", b"/", b"go", b"google", b"\\", b"\xff\x00", b".com"]
    cases = []
    for t in range(n):
        n_seg = int(rng.choice([1, 2, 3, abi.LIKE_MAX_SEGMENTS - 1, abi.LIKE_MAX_SEGMENTS]))
        segs = [b"".join(words[i] for i in rng.integers(0, len(words), int(rng.integers(1, 4)))) for _ in range(n_seg)]
        pat = (b"%" if rng.random() < 0.5 else b"") + b"%".join(segs) + (b"%" if rng.random() < 0.5 else b"")
        if rng.random() < 0.3:
            j = int(rng.integers(0, len(pat) + 1))
            pat = pat[:j] + (b"_" if rng.random() < 0.6 else b"\\%") + pat[j:]
        at_cap = t % 9 == 0 and n_seg <= 3  # exactly at the pattern cap (and within the segment cap)
        if at_cap:
            pat = (pat + b"a" * abi.LIKE_MAX_PATTERN)[:abi.LIKE_MAX_PATTERN - 1] + (b"%" if t % 2 else b"b")
        pat = pat[:abi.LIKE_MAX_PATTERN]
        glue = [words[i] * int(rng.integers(0, 3)) for i in rng.integers(0, len(words), n_seg + 1)]
        hay = b"".join(g + s for g, s in zip(glue, segs)) + glue[-1]
        if rng.random() < 0.3:
            hay = hay[int(rng.integers(0, 3)):len(hay) - int(rng.integers(0, 3))]
        if at_cap and rng.random() < 0.5:
            hay = pat.replace(b"%", b"zz").replace(b"_", b"q").replace(b"\\", b"")
        cases.append((hay, pat))
    return cases


def test_host_entry_points_random_inputs_at_the_caps():
    cases = random_cases_at_the_caps(5, 3000)
    assert any(len(p) == abi.LIKE_MAX_PATTERN for _, p in cases)
    assert any(like_ref.kind(p) == like_ref.SIMPLE and len(like_ref.classify(p)[3]) == abi.LIKE_MAX_SEGMENTS for _, p in cases)
    hits = 0
    for s, pat in cases:
        exp = like_ref.match(s, pat)
        hits += exp
        assert lib_kind(pat) == like_ref.kind(pat), pat
        assert lib_match(s, pat) is exp, (s, pat)
    assert 0.1 * len(cases) < hits < 0.9 * len(cases), hits  # both outcomes are exercised


def test_caps_and_refusals():
    L = lib()
    k, out = C.c_int32(), C.c_int32()
    at_cap = b"a" * abi.LIKE_MAX_PATTERN
    assert L.dbg_like_pattern_kind(at_cap, len(at_cap), C.byref(k)) == abi.DBG_OK and k.value == like_ref.ORDINAL
    over = at_cap + b"a"
    assert L.dbg_like_pattern_kind(over, len(over), C.byref(k)) == abi.DBG_ERR_UNSUPPORTED
    assert str(abi.LIKE_MAX_PATTERN) in L.dbg_last_error().decode()
    assert L.dbg_like_match_host(b"a", 1, over, len(over), C.byref(out)) == abi.DBG_ERR_UNSUPPORTED
    segs_at_cap = b"%".join([b"s"] * abi.LIKE_MAX_SEGMENTS)
    assert L.dbg_like_pattern_kind(segs_at_cap, len(segs_at_cap), C.byref(k)) == abi.DBG_OK and k.value == like_ref.SIMPLE
    segs_over = segs_at_cap + b"%s"
    assert L.dbg_like_pattern_kind(segs_over, len(segs_over), C.byref(k)) == abi.DBG_ERR_UNSUPPORTED
    assert str(abi.LIKE_MAX_SEGMENTS) in L.dbg_last_error().decode()
    # more segments than the cap in a pattern that is not a SimplePattern are no refusal
    cx = segs_over + b"_"
    assert L.dbg_like_pattern_kind(cx, len(cx), C.byref(k)) == abi.DBG_OK and k.value == like_ref.COMPLEX
    assert L.dbg_like_pattern_kind(None, 3, C.byref(k)) == abi.DBG_ERR_INVALID


def test_program_marshals_like_nodes():
    s = Column.from_strings([b"a", b"b"])
    i = Column.from_numbers(col.Int32, np.array([1, 2], np.int32))
    prog = FilterProgram(and_(like(0, "%goo\\gle%"), not_like(0, b"\xff_")), [s.to_abi()])
    ops = [n.op for n in prog.nodes]
    assert ops == [abi.PRED_LIKE, abi.PRED_LIKE, abi.PRED_NOT, abi.PRED_AND] and abi.PRED_LIKE == 16
    assert C.string_at(prog.nodes[0].str, prog.nodes[0].str_len) == b"%goo\\gle%"
    assert C.string_at(prog.nodes[1].str, prog.nodes[1].str_len) == b"\xff_"
    with pytest.raises(DbgError) as e:
        FilterProgram(and_(cmp(0, "=", 1), like(0, "%a%")), [i.to_abi()])
    assert e.value.code == abi.DBG_ERR_INVALID


# ---- the host build under AddressSanitizer + UBSan, as a program of its own ------------------------
def _pack(cases) -> bytes:
    parts = [struct.pack("<I", len(cases))]
    for s, p in cases:
        parts += [struct.pack("<HH", len(s), len(p)), s, p]
    return b"".join(parts)


def test_matcher_under_sanitizers_standalone(tmp_path):
    """tests/csrc/like_host_main.cpp (its own main; nothing sanitised is loaded into this process):
    the exhaustive short set, the random set at the caps and random bytes, every haystack and
    pattern in a heap block of exactly its length.  Its answers equal the Python reference's."""
    exe = str(tmp_path / "like_host_main")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(HERE, "csrc", "like_host_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    if build.returncode != 0 and "cannot find" in build.stderr and ("asan" in build.stderr or "ubsan" in build.stderr):
        pytest.skip("no host AddressSanitizer / UBSan runtime to link against")
    assert build.returncode == 0, build.stderr[-3000:]
    strs = short_strings()
    rng = np.random.default_rng(77)
    noise = [(rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8).tobytes(),
              bytes(rng.choice(np.frombuffer(b"%_\\ab\x00\xff", np.uint8), int(rng.integers(0, 12))))) for _ in range(20_000)]
    cases = [(s, pat) for pat in strs for s in strs] + random_cases_at_the_caps(6, 3000) + noise
    (tmp_path / "cases.bin").write_bytes(_pack(cases))
    run = subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "out.txt")], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stderr[-3000:]
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    got = (tmp_path / "out.txt").read_text()
    assert len(got) == 2 * len(cases)
    exp = []
    for k, row in exhaustive_expected():
        exp += [f"{k}{int(m)}" for m in row]
    memo = {}
    for s, pat in cases[len(strs) ** 2:]:
        if pat not in memo:
            memo[pat] = (like_ref.kind(pat), like_ref.matcher(pat))
        k, m = memo[pat]
        exp.append(f"{k}{int(bool(m(s)))}")
    bad = [(cases[i], got[2 * i:2 * i + 2], e) for i, e in enumerate(exp) if got[2 * i:2 * i + 2] != e]
    assert not bad, bad[:5]
