"""The host part of the mesh kit (dynamicfusion_amd/csrc/dfusion_mesh_kit.h) on the host: tests/cxx/mesh_kit_test.cpp checks the capped
grid at both caps (0 items give 0 workgroups, as the three functions it replaces gave), the rounding to 16, the overlap test of the
argument checks and the workspace carve.  Plain C++ with the compiler's address and undefined-behaviour checks -- no GPU, no HIP."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mesh_kit_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler")
    exe = str(tmp_path / "mesh_kit_test")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(REPO, "dynamicfusion_amd", "csrc"), os.path.join(REPO, "tests", "cxx", "mesh_kit_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "mesh kit ok" in out.stdout
