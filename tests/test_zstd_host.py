"""The device Zstandard decoder (databend_amd/csrc/zstd_dev.hpp) built for the host (ZS_HOST) and
checked against libzstd-made frames (pyarrow's zstd codec: levels 1-19 and negative, raw / RLE /
compressed blocks, Huffman 1- and 4-stream literals, predefined / RLE / FSE / repeat sequence
tables), plus corrupted frames under AddressSanitizer: every malformed input is rejected without
an out-of-bounds access.  The case table of tests/zstd_frames.py (frames built to reach every
decoder path, and malformed ones) runs through a stand-alone AddressSanitizer + UBSan program,
tests/csrc/zstd_host_main.cpp.  The GPU parity of the same decoder on Parquet pages is
tests/test_gpu_parquet.py and tests/test_gpu_zstd_frames.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "databend_amd", "csrc")


def _build(tmp, asan):
    out = os.path.join(tmp, "zstd_host_asan.so" if asan else "zstd_host.so")
    cmd = ["g++", "-O1" if asan else "-O2", "-std=c++17", "-shared", "-fPIC", "-I", CSRC,
           os.path.join(HERE, "csrc", "zstd_host.cpp"), "-o", out]
    if asan:
        cmd[1:1] = ["-fsanitize=address", "-fno-omit-frame-pointer"]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(out)
    lib.zs_host_decode.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64]
    return lib


@pytest.fixture(scope="module")
def zlib_(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("zs")), asan=False)


def _cases():
    rng = np.random.default_rng(1)
    words = [b"alpha", b"beta", b"gamma", b"delta", b"epsilon", b"zeta"]
    return [
        b"", b"a" * 1000, rng.integers(0, 256, 5000, dtype=np.uint8).tobytes(),
        rng.integers(0, 4, 300_000, dtype=np.uint8).tobytes(),
        b" ".join(words[i] for i in rng.integers(0, 6, 100_000)),
        np.arange(200_000, dtype=np.int64).tobytes(),
        (rng.zipf(1.3, 300_000) % 1000).astype(np.int32).tobytes(),
    ]


def _decode(lib, c, n):
    out = C.create_string_buffer(n + 1)
    rc = lib.zs_host_decode(c, len(c), out, n)
    return rc, out.raw[:n]


@pytest.mark.parametrize("level", [-5, 1, 3, 9, 19])
def test_frames_roundtrip(zlib_, level):
    codec = pa.Codec("zstd", compression_level=level)
    for d in _cases():
        rc, got = _decode(zlib_, codec.compress(d, asbytes=True), len(d))
        assert rc == 0 and got == d


def test_corrupted_frames_rejected_in_bounds(tmp_path):
    """Byte flips, truncations and wrong sizes under AddressSanitizer: no invalid access.  (A flip
    inside a raw literal run decodes "successfully" to different bytes — zstd frames without a
    content checksum cannot detect it; Parquet's page CRC is that check — so only memory safety
    is asserted here.)"""
    env_ok = subprocess.run(["g++", "-fsanitize=address", "-x", "c++", "-", "-o", os.path.join(str(tmp_path), "t")],
                            input=b"int main(){return 0;}", capture_output=True).returncode == 0
    if not env_ok:
        pytest.skip("no host AddressSanitizer runtime")
    # the ASan runtime must be the first library: run the fuzz loop in a child interpreter
    script = f"""
import ctypes as C, numpy as np, pyarrow as pa, sys
sys.path.insert(0, {HERE!r})
from test_zstd_host import _build, _cases, _decode
lib = _build({str(tmp_path)!r}, asan=True)
rng = np.random.default_rng(7)
bad_ok = 0
for level in (1, 19):
    codec = pa.Codec("zstd", compression_level=level)
    for d in _cases()[1:]:
        c = bytearray(codec.compress(d, asbytes=True))
        for t in range(40):
            x = bytearray(c)
            for _ in range(int(rng.integers(1, 4))):
                j = int(rng.integers(0, len(x)))
                x[j] ^= int(rng.integers(1, 256))
            if t % 5 == 0:
                x = x[:int(rng.integers(1, len(x)))]
            n = len(d) if t % 7 else len(d) // 2 + 1
            rc, got = _decode(lib, bytes(x), n)
            if rc == 0 and got != d[:n]:
                bad_ok += 1
print("silent", bad_ok)
"""
    asan = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    pre = os.environ.get("LD_PRELOAD", "")
    env = dict(os.environ, LD_PRELOAD=asan + (":" + pre if pre else ""), ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0")
    r = subprocess.run(["python", "-c", script], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr


# ---- the host build under AddressSanitizer + UBSan, as a program of its own ------------------------
def _fnv1a64(b: bytes) -> int:
    h = 0xcbf29ce484222325
    for x in np.frombuffer(b, np.uint8).tolist():
        h = ((h ^ x) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_case_table_under_sanitizers_standalone(tmp_path):
    """tests/csrc/zstd_host_main.cpp (its own main; nothing sanitised is loaded into this process):
    every frame of the case table (tests/zstd_frames.py) and every malformed frame, each in a heap
    block of exactly its length and decoded into one of exactly the output size, in one run.  The
    good frames decode to the expected bytes (by hash), the malformed ones are rejected, and
    neither sanitizer reports anything."""
    import struct

    from tests import zstd_frames as zf
    exe = str(tmp_path / "zstd_host_main")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(HERE, "csrc", "zstd_host_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    if build.returncode != 0 and "cannot find" in build.stderr and ("asan" in build.stderr or "ubsan" in build.stderr):
        pytest.skip("no host AddressSanitizer / UBSan runtime to link against")
    assert build.returncode == 0, build.stderr[-3000:]
    good, bad = zf.cases(), zf.malformed()
    recs = [(c.frame, len(c.expected)) for c in good] + [(m.frame, m.size) for m in bad]
    (tmp_path / "records.bin").write_bytes(struct.pack("<I", len(recs)) +
                                           b"".join(struct.pack("<IQ", len(f), n) + f for f, n in recs))
    run = subprocess.run([exe, str(tmp_path / "records.bin"), str(tmp_path / "out.txt")], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stderr[-3000:]
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    got = (tmp_path / "out.txt").read_text().split("\n")[:-1]
    assert len(got) == len(recs)
    exp = ["0 %016x" % _fnv1a64(c.expected) for c in good] + ["1"] * len(bad)
    wrong = [(n, g, e) for n, g, e in zip([c.name for c in good] + [m.name for m in bad], got, exp) if g != e]
    assert not wrong, wrong[:5]
