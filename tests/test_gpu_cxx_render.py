"""The mesh rasteriser through the C++ mirror: the `render_mesh` app (kfusion::cuda::renderMesh) reproduces the bytes of the Python
mirror's frontend.renderMesh -- which tests/test_gpu_render_mesh.py pins to the numpy restatement -- on the same inputs."""
import subprocess

import numpy as np
import pytest
import torch

from dynamicfusion_amd import Intr, build, frontend, synth
from test_gpu_render_mesh import dressed, random_triangles

pytestmark = pytest.mark.gpu
F32 = np.float32


def run_app(tmp_path, v, t, cols, rows, intr, ext, w2c=None, nrm=None, att=None, col=None):
    build.build_host()
    fin, fout = str(tmp_path / "render_in.bin"), str(tmp_path / "render_out.bin")
    flags = (1 if w2c is not None else 0) | (2 if nrm is not None else 0) | (4 if att is not None else 0) | (8 if col is not None else 0)
    with open(fin, "wb") as f:
        f.write(np.array([len(v), len(t), cols, rows, ext, flags], np.int32).tobytes())
        f.write(np.array(intr, F32).tobytes())
        for a, dt in ((w2c, F32), (v, F32), (np.asarray(t, np.uint32), np.uint32), (nrm, F32), (att, F32), (col, np.uint8)):
            if a is not None:
                f.write(np.ascontiguousarray(a, dt).tobytes())
    r = subprocess.run([build.HOST_RENDER_MESH, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(fout, np.uint8)
    px, out, o = rows * cols, {}, 0
    for k, present, bpp in (("points", True, 16), ("normals", nrm is not None, 16), ("attr", att is not None, 16), ("colors", col is not None, 4),
                            ("tri", True, 4)):
        if present:
            out[k] = raw[o:o + px * bpp]
            o += px * bpp
    out["counts"] = raw[o:].view(np.uint64)
    assert raw.size == o + 48
    return out


def python_mirror(v, t, cols, rows, intr, ext, w2c=None, nrm=None, att=None, col=None):
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    got = frontend.renderMesh(Intr(*intr), dev(v), dev(np.asarray(t, np.uint32).view(np.int32)), cols, rows, world2cam=w2c, normals=dev(nrm), attr=dev(att),
                              colors=dev(col), max_extent=ext, return_tri=True, return_counts=True)
    out = {k: g.cpu().numpy().reshape(-1).view(np.uint8) for k, g in zip(("points", "normals", "attr", "colors", "tri"), got[:5]) if g is not None}
    out["counts"] = got[5].cpu().numpy().astype(np.uint64)
    return out


@pytest.mark.parametrize("dressing", ["all", "none", "normals-and-colours"])
def test_cxx_render_mesh_app_equals_the_python_mirror(tmp_path, dressing):
    v, t, intr = random_triangles(5000, 64, 48, seed=41, size=2.0)
    n, a, c = dressed(v)
    pose = synth.rot_y_about(np.deg2rad(3.0), (0.0, 0.0, 1.0))
    w2c = synth.aff12(np.linalg.inv(pose.astype(np.float64)).astype(F32)) if dressing != "none" else None
    kw = {"all": dict(nrm=n, att=a, col=c), "none": {}, "normals-and-colours": dict(nrm=n, col=c)}[dressing]
    for ext in (4, 16):
        want = python_mirror(v, t, 64, 48, intr, ext, w2c=w2c, **kw)
        got = run_app(tmp_path, v, t, 64, 48, intr, ext, w2c=w2c, **kw)
        assert sorted(got) == sorted(want)
        for k in want:
            assert np.array_equal(got[k], want[k]), (k, ext)
        assert want["counts"][0] > 500 and want["counts"][5] > 500


def test_cxx_render_mesh_app_on_an_empty_mesh(tmp_path):
    got = run_app(tmp_path, np.zeros((0, 4), F32), np.zeros((0, 3), np.uint32), 16, 12, (20.0, 20.0, 8.0, 6.0), 16)
    assert (got["points"].view(np.uint32) == 0x7fffffff).all() and (got["tri"].view(np.int32) == -1).all() and got["counts"].tolist() == [0] * 6


def test_cxx_kinfu_render_live_equals_the_python_mirror(tmp_path):
    """KinFu::renderLive after 4 warped frames at 64^3 / 160 x 120 (kinfu_headless mode word `renderlive`): the live model's point, normal
    and canonical-point images and the shaded view are the bytes the Python mirror makes of the volume, the nodes and the inverted pose
    that the app wrote beside them (fetchMesh with normals, warp, renderMesh, renderImage)."""
    from dynamicfusion_amd import TsdfVolume, WarpField
    cfg = synth.Config(64, 1.0, cols=160, rows=120, nodes=0, k=8)
    frames, px, nvox = 4, 160 * 120, 64 ** 3
    build.build_host()
    fin, fout = str(tmp_path / "kin.bin"), str(tmp_path / "kout.bin")
    with open(fin, "wb") as f:
        f.write(np.asarray(cfg.intr, F32).tobytes())
        for i in range(frames):
            f.write(synth.depth_frame(cfg, 2 * i).tobytes())
    r = subprocess.run([build.HOST_KINFU_APP, str(cfg.cols), str(cfg.rows), str(frames), str(cfg.dims[0]), str(cfg.size), fin, fout, "warped-renderlive"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(fout, np.uint8)
    o = frames * 52 + 8
    volume = raw[o:o + 4 * nvox].view(np.uint32).reshape(64, 64, 64); o += 4 * nvox
    M, k = (int(x) for x in raw[o:o + 8].view(np.int32)); o += 8
    nodes = raw[o:o + 48 * M].view(F32).reshape(M, 12); o += 48 * M
    w2c = raw[o:o + 48].view(F32).copy(); o += 48
    to_live = raw[o:o + 48].view(F32).copy(); o += 48
    light = raw[o:o + 12].view(F32).copy(); o += 12
    images = [raw[o + i * px * 16:o + (i + 1) * px * 16].view(np.uint32).reshape(120, 160, 4) for i in range(3)]; o += 3 * px * 16
    shaded = raw[o:o + px * 4].reshape(120, 160, 4); o += px * 4
    assert o == raw.size and M > 20 and k == 8

    vol = TsdfVolume(cfg.dims)
    vol.setSize([cfg.size] * 3); vol.setTruncDist(cfg.trunc_dist); vol.setMaxWeight(cfg.max_weight); vol.setPose(cfg.volume_pose)
    vol.setRaycastStepFactor(cfg.raycast_step_factor); vol.setGradientDeltaFactor(cfg.gradient_delta_factor)
    vol.upload(volume)
    wf = WarpField(k=k)
    wf.init(np.ascontiguousarray(nodes[:, :3]), sigma=np.ascontiguousarray(nodes[:, 11]), transforms=np.ascontiguousarray(nodes[:, 3:11]))
    pose = np.eye(4, dtype=F32); pose[:3, :3] = to_live[:9].reshape(3, 3); pose[:3, 3] = to_live[9:]
    wf.setWarpToLive(pose)
    intr = Intr(*cfg.intr)
    v, t, n = vol.fetchMesh(with_normals=True)
    p3, n3 = v[:, :3].contiguous(), n[:, :3].contiguous()
    wf.warp(p3, n3)
    warped, wn = torch.zeros_like(v), torch.zeros_like(n)
    warped[:, :3] = p3; wn[:, :3] = n3
    points, normals, attr, _ = frontend.renderMesh(intr, warped, t, cfg.cols, cfg.rows, world2cam=w2c, normals=wn, attr=v)
    want_shaded = frontend.renderImage(points, normals, intr, light).cpu().numpy()
    for name, got, want in zip(("points", "normals", "canonical"), images, (points, normals, attr)):
        assert np.array_equal(got, want.cpu().numpy().view(np.uint32)), name
    assert np.array_equal(shaded, want_shaded)
    hit = images[0][..., 2] != 0x7fffffff
    assert len(t) > 10000 and hit.sum() > 8000 and len(np.unique(shaded[hit][:, :3], axis=0)) > 20
