"""The engine's activation pool and its owning handle (genpercept_amd/csrc/pool.h), checked on the host: no GPU needed.

pool.h includes no HIP header and takes its device allocator as two function pointers, so tests/pool_check.cpp (a stand-alone program) runs
the very code the engine uses over malloc / free.  It is built with the ROCm clang++ under AddressSanitizer and UBSan and run once: the
program checks the reuse policy, the handle's move / reset semantics, the outstanding count, unwinding, persistent buffers and the
`h = f(h)` ordering rule; the sanitizers report a double free, a use after free or a leak in the handle itself.
"""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from post_support import clangxx as _clangxx  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "pool_check.cpp")


def test_pool_and_handle_under_sanitizers(tmp_path):
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("the ROCm clang++ is not on this machine: pool_check.cpp cannot be built")
    exe = tmp_path / "pool_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                        SRC, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "ok", r.stdout + r.stderr
