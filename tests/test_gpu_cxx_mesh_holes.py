"""The C++ mirror of the boundary loops and the hole filling: the `fill_holes` app (kfusion::cuda::boundaryLoops and fillHoles over
dfusion_mesh_boundary_loops / dfusion_mesh_fill_holes) writes, byte for byte, what the Python mirrors mesh_ops.boundary_loops and
fill_holes return on the same input -- which tests/test_gpu_mesh_holes.py pins to the numpy restatement."""
import subprocess

import numpy as np
import pytest
import torch

import mesh_ref as R
import mesh_smooth_ref as S
from dynamicfusion_amd import boundary_loops, build, fill_holes

pytestmark = pytest.mark.gpu
F32 = np.float32


def run_app(tmp_path, v, t, max_edges):
    build.build_host()
    fin, fout = str(tmp_path / "holes_in.bin"), str(tmp_path / "holes_out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([len(v), len(t)], np.uint32).tobytes())
        f.write(np.ascontiguousarray(v, F32).tobytes())
        f.write(np.ascontiguousarray(t, np.uint32).tobytes())
    r = subprocess.run([build.HOST_FILL_HOLES, fin, fout, str(max_edges)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return open(fout, "rb").read()


def python_mirror(v, t, max_edges):
    vd = torch.from_numpy(np.ascontiguousarray(v, F32)).cuda()
    td = torch.from_numpy(np.ascontiguousarray(t, np.uint32).view(np.int32)).cuda()
    nxt, loop, rank, start, members, lc = boundary_loops(td, len(v), return_counts=True)
    fv, ft, src, fc = fill_holes(vd, td, max_edges, return_counts=True)
    return b"".join(a.cpu().numpy().tobytes() for a in (lc, nxt, loop, rank, start, members, fc, fv, ft, src)), lc.tolist(), fc.tolist()


@pytest.mark.parametrize("mesh,max_edges", [("hand", 32), ("hand", 0xffffffff), ("soup", 3), ("soup", 0)])
def test_cxx_fill_holes_app_equals_the_python_mirror(tmp_path, mesh, max_edges):
    if mesh == "hand":
        m = R.mesh_of("hand")
        v, t = m.vertices, m.triangles
    else:
        v, t = S.soup(60000, 50000, 3, p_bad=0.02, p_degenerate=0.05, p_reverse=0.3)
    want, lc, fc = python_mirror(v, t, max_edges)
    assert lc[0] >= 3 and (mesh == "hand" or (lc[3] > 100 and lc[4] > 100 and lc[6] > 100 and lc[7] > 100))
    assert fc[2] == (0 if max_edges == 0 else 2 if max_edges == 32 else lc[0])
    assert run_app(tmp_path, v, t, max_edges) == want


def test_cxx_fill_holes_app_on_an_empty_mesh(tmp_path):
    got = run_app(tmp_path, np.zeros((0, 4), F32), np.zeros((0, 3), np.uint32), 9)
    assert got == np.zeros(8, np.uint64).tobytes() + np.zeros(1, np.uint32).tobytes() + np.zeros(8, np.uint64).tobytes()
