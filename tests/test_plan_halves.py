"""The half-layer bits of the warped sweep's launch plan (dynamicfusion_amd/csrc/dfusion_plan_halves.h) on the host: tests/cxx/plan_halves_test.cpp
packs random verdicts as the plan kernel does and walks them as the sweep does; every plane must be swept exactly once where the plan says
so.  Plain C++ with the compiler's address and undefined-behaviour checks -- no GPU."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_halves_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler")
    exe = str(tmp_path / "plan_halves_test")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(REPO, "dynamicfusion_amd", "csrc"), os.path.join(REPO, "tests", "cxx", "plan_halves_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "plan halves ok" in out.stdout
