"""The C++ mirror of the mesh adjacency and smoothing: the `smooth_mesh` app (kfusion::cuda::meshAdjacency and smoothMesh over
dfusion_mesh_adjacency / dfusion_mesh_smooth) writes, byte for byte, what the Python mirrors mesh_ops.mesh_adjacency and smooth_mesh return
on the same input -- which tests/test_gpu_mesh_smooth.py pins to the numpy restatement."""
import subprocess

import numpy as np
import pytest
import torch

import mesh_ref as R
import mesh_smooth_ref as S
from dynamicfusion_amd import build, mesh_adjacency, smooth_mesh

pytestmark = pytest.mark.gpu
F32 = np.float32


def run_app(tmp_path, v, t, flags, iterations, lam, mu):
    build.build_host()
    fin, fout = str(tmp_path / "smooth_in.bin"), str(tmp_path / "smooth_out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([len(v), len(t), flags, iterations], np.uint32).tobytes())
        f.write(np.array([lam, mu], F32).tobytes())
        f.write(np.ascontiguousarray(v, F32).tobytes())
        f.write(np.ascontiguousarray(t, np.uint32).tobytes())
    r = subprocess.run([build.HOST_SMOOTH_MESH, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return open(fout, "rb").read()


def python_mirror(v, t, flags, iterations, lam, mu):
    vd = torch.from_numpy(np.ascontiguousarray(v, F32)).cuda()
    td = torch.from_numpy(np.ascontiguousarray(t, np.uint32).view(np.int32)).cuda()
    rows, nbr, cls, counts = mesh_adjacency(td, len(v), return_counts=True)
    out = smooth_mesh(vd, td, iterations, float(F32(lam)), float(F32(mu)), fix_boundary=bool(flags & S.FIX_BOUNDARY), adjacency=(rows, nbr, cls))
    return b"".join(a.cpu().numpy().tobytes() for a in (counts, rows, nbr, cls, out)), counts.tolist()


@pytest.mark.parametrize("flags,iterations,mu", [(S.FIX_BOUNDARY, 3, -0.53), (0, 2, 0.0)])
@pytest.mark.parametrize("mesh", ["cut", "soup"])
def test_cxx_smooth_mesh_app_equals_the_python_mirror(tmp_path, mesh, flags, iterations, mu):
    if mesh == "cut":
        m = R.mesh_of("cut")
        v, t = m.vertices, m.triangles
    else:
        v, t = S.soup(20000, 9000, 31, p_bad=0.01, p_degenerate=0.02, p_reverse=0.2)
    want, counts = python_mirror(v, t, flags, iterations, 0.5, mu)
    assert counts[1] > 5000 and counts[2] > 100 and (mesh == "cut" or (counts[3] > 100 and counts[5] > 100 and counts[6] > 100))
    assert run_app(tmp_path, v, t, flags, iterations, 0.5, mu) == want


def test_cxx_smooth_mesh_app_on_an_empty_mesh(tmp_path):
    got = run_app(tmp_path, np.zeros((0, 4), F32), np.zeros((0, 3), np.uint32), 1, 2, 0.5, -0.53)
    assert got == np.zeros(8, np.uint64).tobytes() + np.zeros(1, np.uint32).tobytes()
