"""Buf<T, Mem> (databend_amd/csrc/dev_buf.hpp), the owner of every grow-only device / pinned
buffer, checked on the CPU: tests/dev_buf_check.cpp instantiates it over a malloc-backed policy that
counts live allocations and can fail on request, is built with AddressSanitizer and UBSan, and runs
as a plain program (no device, nothing loaded into Python).  It shows that ensure allocates only
above the capacity and at the requested size, that a failed ensure leaves {nullptr, 0} and a failed
grow_keep leaves the buffer untouched, that grow_keep carries the used elements over, that a move
empties its source, that a reallocating std::vector of buffers frees every block exactly once, and
that nothing is live at exit."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "databend_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_dev_buf_under_sanitizers(tmp_path):
    exe = os.path.join(str(tmp_path), "dev_buf_check")
    # host only: the HIP headers give the types the header names, no HIP call is instantiated
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "dev_buf_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("dev_buf ok:") and r.stdout.rstrip().endswith("0 live"), r.stdout
