"""The C++ mirror of the mesh filter: `headless_frame mesh OUT.ply 25` (TsdfVolume::fetchMesh's overload over
kfusion::cuda::removeSmallComponents) writes, byte for byte, the file write_ply makes of the Python mirror's filtered mesh."""
import subprocess

import numpy as np
import pytest

from dynamicfusion_amd import TsdfVolume, build, mesh_io, synth

pytestmark = pytest.mark.gpu
F32 = np.float32


def test_headless_frame_mesh_with_a_threshold_writes_the_python_mirrors_ply(tmp_path):
    from scene import Scene
    cfg = synth.Config(32, 1.0, cols=80, rows=60, nodes=0, k=4)
    frames = 2
    sc = Scene(cfg, n_frames=frames, with_nodes=False)
    _, app = build.build_host()
    fin, fout, ply = str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(tmp_path / "cxx.ply")
    with open(fin, "wb") as f:
        f.write(synth.aff12(sc.pose).tobytes())
        f.write(np.asarray(cfg.intr, F32).tobytes())
        for i in range(frames):
            f.write(sc.depths[i].tobytes())
            f.write(synth.aff12(sc.cam_poses[i]).tobytes())
    r = subprocess.run([app, "mesh", ply, "25", str(cfg.dims[0]), str(cfg.size), str(cfg.cols), str(cfg.rows), str(frames), "0", str(cfg.k), fin, fout],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    nv = int(np.prod(cfg.dims))
    vol = np.fromfile(fout, np.uint32, count=nv).reshape(cfg.dims[2], cfg.dims[1], cfg.dims[0])     # the volume the harness fused from those frames
    v = TsdfVolume(cfg.dims)
    v.setSize([cfg.size] * 3)
    v.setPose(sc.pose)
    v.upload(vol)
    vertices, triangles = v.fetchMesh(min_component_triangles=25)
    all_vertices, all_triangles = v.fetchMesh()
    assert 1000 < triangles.shape[0] < all_triangles.shape[0] and vertices.shape[0] < all_vertices.shape[0]     # the threshold dropped something
    mine = str(tmp_path / "py.ply")
    mesh_io.write_ply(mine, vertices, triangles)
    assert open(ply, "rb").read() == open(mine, "rb").read()
