"""The C++ mirror of the ray query: the `mesh_rays` app (kfusion::cuda::rayHits and visiblePoints over dfusion_mesh_ray_hits) writes,
byte for byte, what the Python mirrors mesh_ops.ray_hits and visible_points return on the same input -- which
tests/test_gpu_mesh_rays.py pins to the numpy restatement, as this test does once more for the triangles and the mask."""
import re
import subprocess

import numpy as np
import pytest
import torch

import mesh_closest_ref as M
import mesh_rays_ref as Y
from dynamicfusion_amd import build, ray_hits, visible_points

pytestmark = pytest.mark.gpu
F32 = np.float32


def run_app(tmp_path, v, t, o, d, t_min, t_max, eye, margin):
    build.build_host()
    fm, fr, fout = (str(tmp_path / n) for n in ("mesh.bin", "rays.bin", "rays_out.bin"))
    with open(fm, "wb") as f:
        f.write(np.array([len(v), len(t)], np.uint32).tobytes())
        f.write(np.ascontiguousarray(v, F32).tobytes())
        f.write(np.ascontiguousarray(t, np.uint32).tobytes())
    with open(fr, "wb") as f:
        f.write(np.array([len(o)], np.uint32).tobytes())
        f.write(np.array([t_min, t_max] + list(eye) + [margin], F32).tobytes())
        f.write(np.ascontiguousarray(o, F32).tobytes())
        f.write(np.ascontiguousarray(d, F32).tobytes())
    r = subprocess.run([build.HOST_MESH_RAYS, fm, fr, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return open(fout, "rb").read(), r.stdout


def python_mirror(v, t, o, d, t_min, t_max, eye, margin):
    vd = torch.from_numpy(np.ascontiguousarray(v, F32).reshape(-1, 4)).cuda()
    td = torch.from_numpy(np.ascontiguousarray(t, np.uint32).reshape(-1, 3).view(np.int32)).cuda()
    od, dd = torch.from_numpy(np.ascontiguousarray(o, F32)).cuda(), torch.from_numpy(np.ascontiguousarray(d, F32)).cuda()
    tri, hit, bary, counts = ray_hits(vd, td, od, dd, t_min, t_max, return_barycentric=True, return_counts=True)
    tri_any, counts_any = ray_hits(vd, td, od, dd, t_min, t_max, any_hit=True, return_counts=True)
    vis = visible_points(vd, td, vd, eye, margin)
    return b"".join(x.cpu().numpy().tobytes() for x in (counts, tri, hit, bary, counts_any, tri_any, vis.to(torch.uint8)))


@pytest.mark.parametrize("case", ["soup", "hostile"])
def test_cxx_mesh_rays_app_equals_the_python_mirror(tmp_path, case):
    v, t = M.soup(600, 1, size=0.12)
    o, d = Y.aimed_rays(v, t, 900, 2)
    limits, eye, margin = (0.0, float("inf")), [0.5, 0.4, -2.0], 2.0 ** -10
    if case == "hostile":
        t[::9, 1] = t[::9, 0]                                            # skipped triangles
        v[::50, 2] = np.nan                                              # non-finite vertices: skipped triangles, and points that are not visible
        o[::13, 0], d[5::13, :3] = np.inf, 0.0                           # invalid rays
        limits, margin = (0.25, 1.5), 0.125
    want = python_mirror(v, t, o, d, *limits, eye, margin)
    got, stdout = run_app(tmp_path, v, t, o, d, *limits, eye, margin)
    assert got == want
    ref = Y.ray_hits(v, t, o, d, *limits)
    R, V = len(o), len(v)
    assert np.array_equal(np.frombuffer(got, np.uint32, R, 64), ref.triangle) and ref.counts[0] > 300
    assert np.array_equal(np.frombuffer(got, np.uint8, V, len(got) - V).astype(bool), Y.visible_points(v, t, v, eye, margin))
    m = re.search(r"rays (\d+) hits (\d+) misses (\d+) invalid (\d+) tests \d+ nodes \d+; any-hit hits (\d+) tests \d+; visible (\d+) of (\d+)", stdout)
    assert m, stdout
    assert [int(x) for x in m.groups()[:5]] == [R] + [int(ref.counts[k]) for k in (0, 1, 4, 0)] and int(m.group(7)) == V
    if case == "hostile":
        assert ref.counts[4] == len(o[::13]) + len(o[5::13]) and ref.counts[3] > 60


def test_cxx_mesh_rays_app_on_an_empty_mesh_and_no_rays(tmp_path):
    none = np.zeros((0, 4), F32)
    got, stdout = run_app(tmp_path, none, np.zeros((0, 3), np.uint32), none, none, 0.0, 1.0, [0, 0, 0], 0.0)
    assert got == np.zeros(16, np.uint64).tobytes() and "rays 0 hits 0" in stdout
