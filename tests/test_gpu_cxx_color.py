"""kfusion::KinFu with KinFuParams::integrate_color, through host/apps/color_frame: 4 RGB-D frames at 64^3 / 160 x 120.  The colour volume
and the vertex colours it leaves are those of the Python mirror (ColorVolume) fed the same frames -- the frame's image, the dists of the
depth image KinFu fuses, the pose, the TSDF volume and the warp nodes the app recorded; with the flag off the frame's outputs are the
ones without an image."""
import subprocess

import numpy as np
import pytest
import torch

import color_ref as CR
from dynamicfusion_amd import ColorVolume, Intr, TsdfVolume, WarpField, build, compute_dists, frontend, synth, upload_u16

pytestmark = pytest.mark.gpu
F32 = np.float32
FRAMES = 4


def scene():
    cfg = synth.Config(64, 1.0, cols=160, rows=120, nodes=0, k=8)
    depths = [synth.depth_frame(cfg, 2 * i) for i in range(FRAMES)]
    images = [CR.paint_checker(d, synth.camera_pose(cfg, 2 * i), cfg.intr) for i, d in enumerate(depths)]
    return cfg, depths, images


def run_app(tmp_path, cfg, depths, images, mode):
    build.build_host()
    fin, fout = str(tmp_path / "cin.bin"), str(tmp_path / ("cout_%s.bin" % (mode or "plain")))
    with open(fin, "wb") as f:
        f.write(np.asarray(cfg.intr, F32).tobytes())
        for d, im in zip(depths, images):
            f.write(d.tobytes())
            f.write(im.tobytes())
    r = subprocess.run([build.HOST_COLOR_FRAME, str(cfg.cols), str(cfg.rows), str(FRAMES), str(cfg.dims[0]), str(cfg.size), fin, fout] + ([mode] if mode else []),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return parse(np.fromfile(fout, np.uint8), cfg)


def parse(raw, cfg):
    nvox = int(np.prod(cfg.dims))
    o = [0]

    def take(dtype, n):
        a = raw[o[0]:o[0] + n * np.dtype(dtype).itemsize].view(dtype)
        o[0] += a.nbytes
        return a
    out = {"ksz": int(take(np.int32, 1)[0]), "k": int(take(np.int32, 1)[0])}
    out["sigma_spatial"], out["sigma_depth"], out["truncate"], out["trunc_dist"] = (float(x) for x in take(F32, 4))
    out["frames"] = []
    for _ in range(FRAMES):
        fr = {"tracked": int(take(np.int32, 1)[0]), "pose": take(F32, 12).copy(), "w2l": take(F32, 12).copy()}
        M = int(take(np.int32, 1)[0])
        fr["pos"], fr["dq"], fr["sigma"] = take(F32, 3 * M).reshape(M, 3).copy(), take(F32, 8 * M).reshape(M, 8).copy(), take(F32, M).copy()
        fr["counts"] = [int(c) for c in take(np.uint64, 2)]
        fr["vol"] = take(np.uint32, nvox).reshape(cfg.dims[2], cfg.dims[1], cfg.dims[0])
        out["frames"].append(fr)
    out["has_color"] = int(take(np.int32, 1)[0])
    if out["has_color"]:
        out["color"] = take(np.uint8, 4 * nvox).reshape(cfg.dims[2], cfg.dims[1], cfg.dims[0], 4)
        nv = int(take(np.uint64, 1)[0])
        out["vertices"], out["vertex_colors"] = take(F32, 4 * nv).reshape(nv, 4), take(np.uint8, 4 * nv).reshape(nv, 4)
    assert o[0] == raw.size
    return out


def pose44(a):
    T = np.eye(4, dtype=F32)
    T[:3, :3] = a[:9].reshape(3, 3)
    T[:3, 3] = a[9:]
    return T


@pytest.mark.parametrize("mode", ["color", "color-warped"])
def test_kinfu_leaves_the_python_mirrors_colours(tmp_path, mode):
    cfg, depths, images = scene()
    got = run_app(tmp_path, cfg, depths, images, mode)
    plain = run_app(tmp_path, cfg, depths, images, mode.replace("color", "").strip("-"))
    assert [f["tracked"] for f in got["frames"]] == [0] + [1] * (FRAMES - 1) and got["has_color"] == 1 and plain["has_color"] == 0
    # with the flag off: the same poses, nodes and volumes, frame by frame (the colour reads the geometry and adds nothing to it)
    for a, b in zip(got["frames"], plain["frames"]):
        assert a["tracked"] == b["tracked"] and np.array_equal(a["pose"].view(np.uint32), b["pose"].view(np.uint32))
        assert np.array_equal(a["dq"].view(np.uint32), b["dq"].view(np.uint32)) and np.array_equal(a["vol"], b["vol"]) and b["counts"] == [0, 0]
    # the Python mirror on the same frames
    intr = Intr(*cfg.intr)
    vol = TsdfVolume(cfg.dims)
    vol.setSize([cfg.size] * 3); vol.setTruncDist(got["trunc_dist"]); vol.setPose(cfg.volume_pose)
    assert np.float32(vol.getTruncDist()) == np.float32(got["trunc_dist"])
    cv = ColorVolume(vol)
    warped_frames = 0
    for f, fr in enumerate(got["frames"]):
        depth = upload_u16(depths[f])
        if f > 0:                                                       # KinFu fuses the bilateral-filtered depth from the second frame on
            depth = frontend.depthBilateralFilter(depth, got["ksz"], got["sigma_spatial"], got["sigma_depth"])
            assert got["truncate"] == 0.0
        dists = compute_dists(depth, intr)
        vol.upload(fr["vol"])
        wf = None
        if "warped" in mode and f > 0 and len(fr["pos"]) >= got["k"]:
            wf = WarpField(k=got["k"], voxel_table=False, weight_table=False)
            wf.init(fr["pos"], sigma=fr["sigma"], transforms=fr["dq"])
            wf.setWarpToLive(pose44(fr["w2l"]))
            warped_frames += 1
        counts = cv.integrate(torch.from_numpy(images[f]).cuda(), dists, pose44(fr["pose"]), intr, warp_field=wf, return_counts=True)
        assert counts.tolist() == fr["counts"] and fr["counts"][1] > 1000, (f, counts.tolist(), fr["counts"])
    assert warped_frames == (FRAMES - 1 if "warped" in mode else 0)
    mine = cv.download()
    assert np.array_equal(mine, got["color"]), int((mine != got["color"]).any(-1).sum())
    assert mine[..., 3].max() == FRAMES and len(np.unique(mine[mine[..., 3] > 0][:, :3], axis=0)) > 2
    vertices, _ = vol.fetchMesh()
    assert np.array_equal(vertices.cpu().numpy().view(np.uint32), got["vertices"].view(np.uint32)) and len(got["vertices"]) > 10000
    colors = cv.fetchColors(vertices).cpu().numpy()
    assert np.array_equal(colors, got["vertex_colors"]) and (colors[:, 3] == 255).mean() > 0.9
