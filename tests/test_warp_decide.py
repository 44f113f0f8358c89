"""The two host decisions of the warped integrate (dynamicfusion_amd/csrc/dfusion_warp_decide.h) on the host: tests/cxx/warp_decide_test.cpp pins
the kernel variant with its launch shape and the verdict pass's look-ahead policy against written-out tables, over every combination of
the inputs' edge values.  Plain C++ with the compiler's address and undefined-behaviour checks -- no GPU."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_warp_decide_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler")
    exe = str(tmp_path / "warp_decide_test")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(REPO, "dynamicfusion_amd", "csrc"), "-I", os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cxx", "warp_decide_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "warp decide ok" in out.stdout
