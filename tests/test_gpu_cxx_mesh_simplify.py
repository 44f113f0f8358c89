"""The C++ mirror of the mesh simplification: the `simplify_mesh` app (kfusion::cuda::simplifyMesh over dfusion_mesh_simplify) writes,
byte for byte, what the Python mirror mesh_ops.simplify_mesh returns on the same input -- which tests/test_gpu_mesh_simplify.py pins to
the numpy restatement."""
import subprocess

import numpy as np
import pytest
import torch

import mesh_simplify_ref as S
from dynamicfusion_amd import build, simplify_mesh

pytestmark = pytest.mark.gpu
F32 = np.float32


def run_app(tmp_path, v, t, cell, flags):
    build.build_host()
    fin, fout = str(tmp_path / "simplify_in.bin"), str(tmp_path / "simplify_out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([len(v), len(t), flags], np.uint32).tobytes())
        f.write(np.array([cell], F32).tobytes())
        f.write(np.ascontiguousarray(v, F32).tobytes())
        f.write(np.ascontiguousarray(t, np.uint32).tobytes())
    r = subprocess.run([build.HOST_SIMPLIFY_MESH, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return open(fout, "rb").read()


def python_mirror(v, t, cell, flags):
    vd = torch.from_numpy(np.ascontiguousarray(v, F32)).cuda()
    td = torch.from_numpy(np.ascontiguousarray(t, np.uint32).view(np.int32)).cuda()
    gv, gt, gs, _, gn = simplify_mesh(vd, td, cell, keep_first=bool(flags & S.KEEP_FIRST), keep_duplicates=bool(flags & S.KEEP_DUPLICATES),
                                      return_counts=True)
    return b"".join(a.cpu().numpy().tobytes() for a in (gn, gv, gt, gs)), gn.tolist()


@pytest.mark.parametrize("flags", [0, S.KEEP_FIRST | S.KEEP_DUPLICATES])
@pytest.mark.parametrize("mesh", ["sphere", "soup"])
def test_cxx_simplify_mesh_app_equals_the_python_mirror(tmp_path, mesh, flags):
    if mesh == "sphere":
        m = S.mesh_named("sphere")
        v, t, cell = m.vertices, m.triangles, float(F32(2 * S.median_edge("sphere")))
    else:
        v, t = S.soup(20000, 9000, 31, p_bad=0.01)
        v[::501, 1] = np.nan
        cell = 0.125
    want, counts = python_mirror(v, t, cell, flags)
    assert counts[0] > 500 and counts[1] > 500 and (mesh == "sphere" or counts[2] > 100)
    assert run_app(tmp_path, v, t, cell, flags) == want


def test_cxx_simplify_mesh_app_on_an_empty_mesh(tmp_path):
    got = run_app(tmp_path, np.zeros((0, 4), F32), np.zeros((0, 3), np.uint32), 1.0, 0)
    assert got == np.zeros(8, np.uint64).tobytes()
