"""The C++ mirror of the closest-point query: the `mesh_distance` app (kfusion::cuda::closestPoints and meshDistance over
dfusion_mesh_closest_points) writes, byte for byte, what the Python mirror mesh_ops.closest_points returns on the same input -- which
tests/test_gpu_mesh_closest.py pins to the numpy restatement -- and prints the figures of mesh_ops.mesh_distance."""
import re
import subprocess

import numpy as np
import pytest
import torch

import mesh_closest_ref as M
import mesh_ref as R
from dynamicfusion_amd import build, closest_points, mesh_distance, simplify_mesh

pytestmark = pytest.mark.gpu
F32 = np.float32


def write_mesh(path, v, t):
    with open(path, "wb") as f:
        f.write(np.array([len(v), len(t)], np.uint32).tobytes())
        f.write(np.ascontiguousarray(v, F32).tobytes())
        f.write(np.ascontiguousarray(t, np.uint32).tobytes())


def run_app(tmp_path, a, b):
    build.build_host()
    fa, fb, fout = (str(tmp_path / n) for n in ("a.bin", "b.bin", "distance_out.bin"))
    write_mesh(fa, *a)
    write_mesh(fb, *b)
    r = subprocess.run([build.HOST_MESH_DISTANCE, fa, fb, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return open(fout, "rb").read(), r.stdout


def device(v, t):
    return (torch.from_numpy(np.ascontiguousarray(v, F32).reshape(-1, 4)).cuda(),
            torch.from_numpy(np.ascontiguousarray(t, np.uint32).reshape(-1, 3).view(np.int32)).cuda())


def python_mirror(a, b):
    (va, ta), (vb, tb) = device(*a), device(*b)
    out = []
    for samples, v, t in ((va, vb, tb), (vb, va, ta)):
        tri, point, bary, counts = closest_points(v, t, samples, return_barycentric=True, return_counts=True)
        out += [counts, tri, point, bary]
    return b"".join(x.cpu().numpy().tobytes() for x in out), mesh_distance(va, ta, vb, tb)


def printed(stdout):
    """The app's summary -> {side: {name: number}}, hausdorff."""
    num = r"([-+.\dinfae]+)"
    side = "answered %s unanswered %s max %s at %s mean %s rms %s" % ((num,) * 6)
    m = re.search("a_to_b " + side + "; b_to_a " + side + "; hausdorff " + num, stdout)
    assert m, stdout
    g = [float(x) for x in m.groups()]
    names = ("answered", "unanswered", "max", "max_vertex", "mean", "rms")
    return dict(zip(names, g[:6])), dict(zip(names, g[6:12])), g[12]


def sphere_and_simplified():
    m = R.mesh_of("sphere")
    vd, td = device(m.vertices, m.triangles)
    sv, st, src, vmap = simplify_mesh(vd, td, 2 * float(R.VS[0]))
    return (m.vertices, m.triangles), (sv.cpu().numpy(), st.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("case", ["sphere", "soups"])
def test_cxx_mesh_distance_app_equals_the_python_mirror(tmp_path, case):
    if case == "sphere":
        a, b = sphere_and_simplified()
    else:
        a, b = M.soup(700, 1), M.soup(300, 2, offset=0.25)
        a[1][::9, 1] = a[1][::9, 0]                                      # skipped triangles on one side
        b[0][::50, 2] = np.nan                                           # non-finite samples and triangles on the other
    want, md = python_mirror(a, b)
    got, stdout = run_app(tmp_path, a, b)
    assert got == want
    ab, ba, hausdorff = printed(stdout)
    for got_side, want_side in ((ab, md["a_to_b"]), (ba, md["b_to_a"])):
        assert got_side["answered"] == want_side["answered"] > 0 and got_side["unanswered"] == want_side["unanswered"]
        assert got_side["max"] == want_side["max"] and got_side["max_vertex"] == want_side["max_vertex"]
        rel = (2 * want_side["answered"] + 4) * 2.0 ** -53               # two sums of n terms in different orders, a division and a root
        assert abs(got_side["mean"] - want_side["mean"]) <= rel * want_side["mean"] and abs(got_side["rms"] - want_side["rms"]) <= rel * want_side["rms"]
    assert hausdorff == md["hausdorff"] > 0
    if case == "soups":
        assert md["b_to_a"]["unanswered"] == 18 and md["a_to_b"]["unanswered"] == 0


def test_cxx_mesh_distance_app_on_empty_meshes(tmp_path):
    empty = (np.zeros((0, 4), F32), np.zeros((0, 3), np.uint32))
    got, stdout = run_app(tmp_path, empty, empty)
    none = np.array([0, 0, 0, 0, 0, 0xffffffff, 0, 0], np.uint64).tobytes()
    assert got == none + none and "hausdorff 0" in stdout
