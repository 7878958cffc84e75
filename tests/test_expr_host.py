"""The host build of the projection's evaluator (databend_amd/csrc/expr.hpp: expr_compile and the
per-row operators the kernel compiles) as a stand-alone program under -fsanitize=address,undefined,
over case files that tests/expr_ref.py writes.  Types, values and error flags are compared exactly.
Nothing sanitised is loaded into this process."""
import os
import subprocess

import pytest

from tests import expr_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "databend_amd", "csrc")


def build_program(tmp_path):
    exe = str(tmp_path / "expr_host_main")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(HERE, "csrc", "expr_host_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    if build.returncode != 0 and "cannot find" in build.stderr and ("asan" in build.stderr or "ubsan" in build.stderr):
        pytest.skip("no host AddressSanitizer / UBSan runtime to link against")
    assert build.returncode == 0, build.stderr[-3000:]
    return exe


def run_program(args, tmp_path):
    run = subprocess.run(args, capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stderr[-3000:]
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    return (tmp_path / "out.txt").read_text().splitlines()


def test_whole_programs_under_sanitizers_standalone(tmp_path):
    """Multi-node programs whose integer intermediates (negative, wrapped, unsigned with the top bit
    set) feed decimal operators, NULLs included: the value a number operator leaves must be extended
    to 128 bits by its result type before a decimal operator reads it."""
    exe = build_program(tmp_path)
    progs = R.mixed_programs(rows=131)
    (tmp_path / "programs.bin").write_bytes(R.pack_programs(progs))
    lines = run_program([exe, "--programs", str(tmp_path / "programs.bin"), str(tmp_path / "out.txt")], tmp_path)
    at = 0
    for e, types, values in progs:
        t, want, err = R.evaluate(e, types, values)
        assert err is None
        assert any(w is not None and w < 0 for w in want) and len(want) == 131
        for i, w in enumerate(want):
            f = lines[at + i].split()
            assert int(f[0]) == 0 and (int(f[1]), int(f[2]), int(f[3])) == (t.type_id, t.precision, t.scale), (e, f)
            assert int(f[7]) == 0 and (int(f[6]) == 1) == (w is not None), (e, i, f, w)
            if w is not None:
                assert R.uncanon(int(f[4], 16), int(f[5], 16), t) == w, (e, i, f, w)
        at += len(want)
    assert at == len(lines)


def test_evaluator_under_sanitizers_standalone(tmp_path):
    exe = build_program(tmp_path)
    cases = R.number_cases() + R.decimal_cases()
    (tmp_path / "cases.bin").write_bytes(R.pack_cases(cases))
    lines = run_program([exe, str(tmp_path / "cases.bin"), str(tmp_path / "out.txt")], tmp_path)
    assert len(lines) == len(cases)
    bad = []
    errors = 0
    for case, line in zip(cases, lines):
        f = line.split()
        t, want, err = R.expected(case)
        errors += err
        ok = int(f[0]) == 0 and (int(f[1]), int(f[2]), int(f[3])) == (t.type_id, t.precision, t.scale) and int(f[6]) == err
        if ok and not err:
            ok = R.same_value(t, R.uncanon(int(f[4], 16), int(f[5], 16), t), want)
        if not ok:
            bad.append((case, line, want, err))
    assert not bad, bad[:5]
    assert 500 < errors < len(cases) // 2  # both outcomes are exercised
