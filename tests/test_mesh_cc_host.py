"""The find / union step of dfusion_mesh_components (dynamicfusion_amd/csrc/dfusion_mesh_cc.h) on the host: tests/cxx/mesh_cc_test.cpp runs
the text the kernels run over a descending chain, stars and random soups, single-threaded over a plain array and with 8 threads over
std::atomic, and compares the labels with a sequential union-find.  Plain C++ with the compiler's address and undefined-behaviour
checks -- no GPU."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mesh_cc_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler")
    exe = str(tmp_path / "mesh_cc_test")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(REPO, "dynamicfusion_amd", "csrc"), os.path.join(REPO, "tests", "cxx", "mesh_cc_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "mesh cc ok" in out.stdout
