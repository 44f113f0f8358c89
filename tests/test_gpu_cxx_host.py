"""The C++ drop-in boundary (dynamicfusion_amd/host: kfusion::cuda::TsdfVolume, DeviceArray2D, WarpField, computeDists)
driven through the headless harness, which makes the hot-path calls of KinFu::operator() / dynamicfusion
(kinfu.cpp:226,248,297,351,391) -- diffed against the oracle on the same inputs."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from dynamicfusion_amd import build, synth
from scene import Scene, compare_volumes

pytestmark = pytest.mark.gpu
F32 = np.float32


# ---- the harness derives vol2cam / cam2vol / Rinv with the arithmetic of host/include/kfusion/types.hpp
def cxx_inv(m):
    R = m[:3, :3].astype(np.float64)
    d = np.array([R[1, 1] * R[2, 2] - R[1, 2] * R[2, 1], R[0, 2] * R[2, 1] - R[0, 1] * R[2, 2], R[0, 1] * R[1, 2] - R[0, 2] * R[1, 1],
                  R[1, 2] * R[2, 0] - R[1, 0] * R[2, 2], R[0, 0] * R[2, 2] - R[0, 2] * R[2, 0], R[0, 2] * R[1, 0] - R[0, 0] * R[1, 2],
                  R[1, 0] * R[2, 1] - R[1, 1] * R[2, 0], R[0, 1] * R[2, 0] - R[0, 0] * R[2, 1], R[0, 0] * R[1, 1] - R[0, 1] * R[1, 0]])
    det = R[0, 0] * d[0] + R[0, 1] * d[3] + R[0, 2] * d[6]
    Ri = (d / det).astype(F32).reshape(3, 3)
    out = np.eye(4, dtype=F32)
    out[:3, :3] = Ri
    t = m[:3, 3].astype(np.float64)
    out[:3, 3] = np.array([-(float(Ri[i, 0]) * t[0] + float(Ri[i, 1]) * t[1] + float(Ri[i, 2]) * t[2]) for i in range(3)], F32)
    return out


def cxx_mul(a, b):
    out = np.eye(4, dtype=F32)
    A, B = a.astype(np.float64), b.astype(np.float64)
    for i in range(3):
        for j in range(3):
            out[i, j] = F32(A[i, 0] * B[0, j] + A[i, 1] * B[1, j] + A[i, 2] * B[2, j])
        out[i, 3] = F32(A[i, 0] * B[0, 3] + A[i, 1] * B[1, 3] + A[i, 2] * B[2, 3] + A[i, 3])
    return out


def run_harness(tmp_path, cfg, sc, frames, with_nodes, surface_fusion=False):
    _, app = build.build_host()
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    M = cfg.nodes if with_nodes else 0
    with open(fin, "wb") as f:
        f.write(synth.aff12(sc.pose).tobytes())
        f.write(np.asarray(cfg.intr, F32).tobytes())
        for i in range(frames):
            f.write(sc.depths[i].tobytes())
            f.write(synth.aff12(sc.cam_poses[i]).tobytes())
        if M:
            f.write(sc.pos.astype(F32).tobytes())
            for i in range(frames):
                f.write(sc.dqs[i].astype(F32).tobytes())
            f.write(sc.sigma.astype(F32).tobytes())
    r = subprocess.run([app, str(cfg.dims[0]), str(cfg.size), str(cfg.cols), str(cfg.rows), str(frames), str(M), str(cfg.k), fin, fout] + (["surface_fusion"] if surface_fusion else []),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(fout, np.uint8)
    nv = int(np.prod(cfg.dims))
    vol = raw[:4 * nv].view(np.uint32).reshape(cfg.dims[2], cfg.dims[1], cfg.dims[0])
    n_img = 2 * cfg.rows * cfg.cols * 16
    img = raw[4 * nv:4 * nv + n_img].view(np.float32).reshape(2, cfg.rows, cfg.cols, 4)
    tail = raw[4 * nv + n_img:]
    cnt = int(tail[:8].view(np.uint64)[0])
    cloud = tail[8:8 + 16 * cnt].view(np.float32).reshape(cnt, 4)
    cnormals = tail[8 + 16 * cnt:8 + 32 * cnt].view(np.float32).reshape(cnt, 4)
    if surface_fusion:
        rest = tail[8 + 32 * cnt:]
        npx = cfg.rows * cfg.cols
        warped = rest[:12 * npx].view(np.float32).reshape(npx, 3)
        depth_after = rest[12 * npx:14 * npx].view(np.uint16).reshape(cfg.rows, cfg.cols)
        vol_after = rest[14 * npx:14 * npx + 4 * nv].view(np.uint32).reshape(cfg.dims[2], cfg.dims[1], cfg.dims[0])
        return vol, img[0], img[1], cloud, cnormals, warped, depth_after, vol_after
    return vol, img[0], img[1], cloud, cnormals


@pytest.mark.parametrize("with_nodes", [False, True], ids=["rigid", "warped"])
def test_cxx_api_matches_oracle(tmp_path, with_nodes):
    cfg = synth.Config(64, 1.0, cols=160, rows=120, nodes=100, k=8)
    frames = 2
    sc = Scene(cfg, n_frames=frames)
    vol, pts, nrm, cloud, cnormals = run_harness(tmp_path, cfg, sc, frames, with_nodes)
    ref = sc.new_volume()
    for f in range(frames):
        cam_inv = cxx_inv(sc.cam_poses[f])
        if with_nodes:
            O.integrate_warped(sc.dists[f], ref, sc.ovol(ref), synth.aff12(sc.pose), synth.aff12(cam_inv), sc.intr, sc.pos,
                               sc.dqs[f], sc.sigma, cfg.k)
        else:
            O.integrate(sc.dists[f], ref, sc.ovol(ref), synth.aff12(cxx_mul(cam_inv, sc.pose)), sc.intr)
    s = compare_volumes(vol, ref)
    print(s)
    assert s["bits_mismatch"] == 0, s
    cam2vol = cxx_mul(cxx_inv(sc.pose), sc.cam_poses[frames - 1])
    rinv = cxx_inv(cam2vol)[:3, :3]
    rp, rn, _, stats = O.raycast_points(sc.ovol(ref), synth.aff12(cam2vol), rinv, sc.reproj, cfg.cols, cfg.rows,
                                        cfg.raycast_step_factor, cfg.gradient_delta_factor)
    assert stats[1] > 1000
    assert np.array_equal(pts.view(np.uint32), rp.view(np.uint32)) and np.array_equal(nrm.view(np.uint32), rn.view(np.uint32))
    # compute_points / compute_normals (kinfu.cpp:398-399) through the C++ class: same SET of points as the oracle
    rc, n = O.extract_cloud(sc.ovol(ref), synth.aff12(sc.pose), 1 << 22)
    assert n == cloud.shape[0] > 1000
    order = lambda a: a[np.lexsort(np.ascontiguousarray(a).view(np.uint32).T[::-1])]
    assert np.array_equal(order(cloud).view(np.uint32), order(rc).view(np.uint32))
    pinv = cxx_inv(sc.pose)[:3, :3]
    rnrm = O.extract_normals(sc.ovol(ref), synth.aff12(sc.pose), pinv, cloud, cfg.gradient_delta_factor)
    assert np.array_equal(cnormals.view(np.uint32), rnrm.view(np.uint32))


def test_cxx_surface_fusion_matches_oracle(tmp_path):
    """KinFu::dynamicfusion's tail (kinfu.cpp:344-393): canonical points -> WarpField::warp -> TsdfVolume::surface_fusion
    (psdf on the GPU, explained depth pixels removed, leftover depth fused rigidly)."""
    cfg = synth.Config(64, 1.0, cols=160, rows=120, nodes=100, k=8)
    frames = 2
    sc = Scene(cfg, n_frames=frames)
    vol, pts, nrm, _, _, warped, depth_after, vol_after = run_harness(tmp_path, cfg, sc, frames, True, surface_fusion=True)
    f = frames - 1
    # the warp the harness applied == the oracle's warp of the same canonical points (kinfu.cpp:357-387)
    inv = cxx_inv(sc.cam_poses[f])
    P = pts.reshape(-1, 4)[:, :3]
    canonical = np.empty_like(P)
    for i in range(3):
        canonical[:, i] = ((inv[i, 0] * P[:, 0] + inv[i, 1] * P[:, 1]) + inv[i, 2] * P[:, 2]) + inv[i, 3]
    wp, _ = O.warp_points(sc.pos, sc.dqs[f], sc.sigma, canonical, nrm.reshape(-1, 4)[:, :3], cfg.k)
    nan_a, nan_b = np.isnan(wp), np.isnan(warped)
    assert np.array_equal(nan_a, nan_b) and 1000 < (~nan_a[:, 0]).sum() < wp.shape[0]
    assert np.array_equal(wp.view(np.uint32)[~nan_a], warped.view(np.uint32)[~nan_a])
    # psdf + removal + rigid integrate of the leftover depth
    dists0 = O.compute_dists(sc.depths[f], sc.intr)
    w4 = np.zeros((warped.shape[0], 4), F32); w4[:, :3] = warped
    _, removed_mask_img, ro, n_in = O.project_and_remove(dists0, w4, sc.intr)
    assert n_in > 1000
    expect_depth = sc.depths[f].copy()
    expect_depth[(removed_mask_img == 0) & (dists0 != 0)] = 0
    assert np.array_equal(depth_after, expect_depth)
    assert (depth_after == 0).sum() > (sc.depths[f] == 0).sum()
    ref = vol.copy()
    cam_inv = cxx_inv(sc.cam_poses[f])
    O.integrate(O.compute_dists(expect_depth, sc.intr), ref, sc.ovol(ref), synth.aff12(cxx_mul(cam_inv, sc.pose)), sc.intr)
    s = compare_volumes(vol_after, ref)
    assert s["bits_mismatch"] == 0, s
    assert not np.array_equal(vol_after, vol)


def test_cxx_kinfu_tracks_the_camera(tmp_path):
    """kfusion::KinFu::operator() end to end through the C++ mirror (apps/demo.cpp loop without capture / viz): bilateral ->
    pyramid -> point normals -> ProjectiveICP -> dynamicfusion (GPU warp + psdf + fusion) -> raycast -> resize.  Frame 0's
    volume equals the oracle's rigid integrate bit for bit; the frame-1 pose equals the Python ProjectiveICP mirror's (same
    GPU sums, different 6x6 solver) to 1e-5; the camera trajectory follows the ground truth."""
    from dynamicfusion_amd import Intr, frontend, upload_u16
    from frontend_ref import BILATERAL
    cfg = synth.Config(64, 1.0, cols=320, rows=240, nodes=0, k=8)
    frames = 6
    depths = [synth.depth_frame(cfg, 2 * f) for f in range(frames)]
    build.build_host()
    fin, fout = str(tmp_path / "kin.bin"), str(tmp_path / "kout.bin")
    with open(fin, "wb") as f:
        f.write(np.asarray(cfg.intr, F32).tobytes())
        for d in depths:
            f.write(d.tobytes())
    outputs = {}
    for mode in ("nosolver", "", "host", "warped", "warped-host", "nosolver-depth"):
        r = subprocess.run([build.HOST_KINFU_APP, str(cfg.cols), str(cfg.rows), str(frames), str(cfg.dims[0]), str(cfg.size), fin, fout] +
                           ([mode] if mode else []), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = np.fromfile(fout, np.uint8)
        outputs[mode] = raw
        rec = raw[:frames * 52].reshape(frames, 52)
        tracked = rec[:, :4].copy().view(np.int32).ravel()
        poses = rec[:, 4:].copy().view(np.float32).reshape(frames, 12)
        cnt = int(raw[frames * 52:frames * 52 + 8].view(np.uint64)[0])
        assert list(tracked) == [0] + [1] * (frames - 1), r.stdout
        assert cnt > 1000
        if "depth" in mode:                                                 # USE_DEPTH build: only the trajectory / tracking checks below
            for f in range(1, frames):
                true = synth.affine_mul(synth.affine_inv(synth.camera_pose(cfg, 0)), synth.camera_pose(cfg, 2 * f))
                assert np.abs(poses[f][9:12] - true[:3, 3]).max() < 1e-2 and np.abs(poses[f][[2, 5, 8]] - true[:3, 2]).max() < 1e-2
            continue
        # frame 1 ICP: prev pyramids are frame 0's own point normals (kinfu.cpp:257-262)
        intr = Intr(*cfg.intr)
        pyr = []
        for d in depths[:2]:
            lv = [frontend.depthBilateralFilter(upload_u16(d), BILATERAL["ksz"], BILATERAL["sigma_spatial"], BILATERAL["sigma_depth"])]
            for i in range(1, 3):
                lv.append(frontend.depthBuildPyramid(lv[-1], BILATERAL["sigma_depth"]))
            pn = [frontend.computePointNormals(frontend.intr_level(intr, i), lv[i]) for i in range(3)]
            pyr.append(([a for a, _ in pn], [b for _, b in pn]))
        icp = frontend.ProjectiveICP()
        icp.setAngleThreshold(float(F32(30.0) * F32(0.017453293)))          # KinFuParams icp_angle_thres, kinfu.cpp:35
        ok, aff = icp.estimateTransform(intr, pyr[1][0], pyr[1][1], pyr[0][0], pyr[0][1])
        assert ok
        assert np.abs(synth.aff12(aff) - poses[1]).max() < 1e-5
        # trajectory vs ground truth (global frame = first camera frame); roll about the scene's symmetry axis is unobservable
        for f in range(1, frames):
            true = synth.affine_mul(synth.affine_inv(synth.camera_pose(cfg, 0)), synth.camera_pose(cfg, 2 * f))
            got = poses[f]
            # with the warp solver on, the (unregularised, as in the reference) deformation absorbs part of the camera motion
            tol = 1e-2 if mode.startswith("nosolver") else 5e-2
            assert np.abs(got[9:12] - true[:3, 3]).max() < tol, (mode, f, got[9:12], true[:3, 3])
            assert np.abs(got[[2, 5, 8]] - true[:3, 2]).max() < tol
    # the device-resident data flow of dynamicfusion() (default) and the reference's host-staged one give the same bytes:
    # poses, surface count and the whole volume
    for dev, host in (("", "host"), ("warped", "warped-host")):
        d = np.nonzero(outputs[dev] != outputs[host])[0]
        assert d.size == 0, "modes %r / %r: %d bytes differ, first at %s (poses end at byte %d)" % (dev, host, d.size, d[:4], frames * 52)
    assert not np.array_equal(outputs[""], outputs["warped"]) and not np.array_equal(outputs[""], outputs["nosolver"])
    # frame 0 only: the volume is the oracle's rigid integrate of frame 0 at the identity pose, bit for bit
    r = subprocess.run([build.HOST_KINFU_APP, str(cfg.cols), str(cfg.rows), "1", str(cfg.dims[0]), str(cfg.size), fin, fout],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(fout, np.uint8)
    vol = raw[52 + 8:].view(np.uint32).reshape(cfg.dims[2], cfg.dims[1], cfg.dims[0])
    sc = Scene(cfg, n_frames=1, with_nodes=False)
    # KinFu::KinFu sets the truncation distance BEFORE the size (kinfu.cpp:102-104): the clamp of tsdf_volume.cpp:68-73 is taken
    # against the constructor's 3 m default and sticks (quirk kept by the mirror, pinned in test_host_logic.py)
    sc.trunc = float(max(F32(0.04), F32(2.1) * (F32(3.0) / F32(cfg.dims[0]))))
    ref = sc.new_volume()
    pose = np.eye(4, dtype=F32); pose[:3, 3] = [-cfg.size / 2, -cfg.size / 2, 0.5]
    O.integrate(O.compute_dists(depths[0], sc.intr), ref, sc.ovol(ref), synth.aff12(cxx_mul(cxx_inv(np.eye(4, dtype=F32)), pose)), sc.intr)
    s = compare_volumes(vol, ref)
    assert s["bits_mismatch"] == 0, s


def test_cxx_demo_calls_render_and_warp_cloud(tmp_path):
    """host/apps/demo_calls.cpp makes the kfusion calls of the reference's apps/demo.cpp (construction, operator(), getCameraPose,
    both renderImage overloads + download, getNodesAsMat) against the mirror headers.  The views it saves are checked against the
    oracle's restatement of render_image_kernel / tangent_colors_kernel (imgproc.cu:420-583, pinned to the reference's own kernels in
    tests/test_oracle_refcu.py) on what the same pipeline produces through the Python mirror."""
    from dynamicfusion_amd import Intr, frontend, upload_u16
    cfg = synth.Config(64, 1.0, cols=320, rows=240, nodes=0, k=8)
    frames = 4
    depths = [synth.depth_frame(cfg, 2 * f) for f in range(frames)]
    build.build_host()
    fin, prefix = str(tmp_path / "demo_in.bin"), str(tmp_path / "demo")
    with open(fin, "wb") as f:
        f.write(np.asarray(cfg.intr, F32).tobytes())
        for d in depths:
            f.write(d.tobytes())
    r = subprocess.run([build.HOST_DEMO_CALLS, str(cfg.cols), str(cfg.rows), str(frames), str(cfg.dims[0]), str(cfg.size), fin, prefix],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "demo_calls ok" in r.stdout, r.stdout + r.stderr
    shown = frames - 1                                                   # operator() returns false on frame 0 (kinfu.cpp:250)
    views = np.fromfile(prefix + ".views.bin", np.uint8).reshape(shown, 2, cfg.rows, 2 * cfg.cols, 4)
    phong, tangent = views[..., :cfg.cols, :], views[..., cfg.cols:, :]
    # the shaded half shows a surface (many grey levels) over the blue-ish background gradient; alpha byte is 0
    for v in (phong[-1, 0], phong[-1, 1]):
        assert (v[..., 3] == 0).all() and len(np.unique(v[..., 0])) > 30
        grey = (v[..., 0] == v[..., 1]) & (v[..., 1] == v[..., 2])
        assert 0.2 < grey.mean() < 0.95
    # renderImage(image, pose, 3) of the last frame == oracle shading of the oracle... of a ray-cast from the same pose: the second view
    # of frame i is a fresh ray-cast from getCameraPose(); its tangent half and Phong half come from the same points / normals, so the
    # oracle's render of normals recovered from the tangent colours cannot be had -- instead re-render through the Python mirror
    nodes = np.fromfile(prefix + ".nodes.bin", F32).reshape(-1, 3)
    assert len(nodes) > 50 and np.isfinite(nodes).all()
    assert np.abs(nodes[:, :2]).max() < cfg.size and 0.4 < nodes[:, 2].min() and nodes[:, 2].max() < 0.6 + cfg.size
    assert os.path.getsize(prefix + ".ppm") > cfg.rows * 2 * cfg.cols * 3


@pytest.mark.parametrize("with_nodes", [False, True], ids=["rigid", "warped"])
def test_cxx_zslab_rccl_path(tmp_path, with_nodes):
    """kfusion::cuda::ZSlabComm + TsdfVolume::setSlab (host/src/zslab_rccl.cpp, host/apps/zslab_frame.cpp): the C++ side of the Z-slab
    sharding.  One GPU here, so (i) the whole frame with a real RCCL communicator of ONE rank (broadcast, the two-stage ray-cast's
    all-reduces and reduce with nranks = 1) must give the unsharded harness's bytes, and (ii) every shard of a 4-way partition,
    integrated alone through the C++ slab path, must give its planes of the unsharded volume.  (N > 1 needs N GPUs: RCCL refuses two
    ranks on one device; the collective sequence is the one of dynamicfusion_amd/sharded.py, which the gloo tests run at N = 2, 3.)"""
    cfg = synth.Config(64, 1.0, cols=160, rows=120, nodes=100, k=8)
    frames = 2
    sc = Scene(cfg, n_frames=frames)
    vol, pts, nrm, _, _ = run_harness(tmp_path, cfg, sc, frames, with_nodes)
    build.build_host()
    fin = str(tmp_path / "in.bin")                                         # written by run_harness
    M = cfg.nodes if with_nodes else 0
    base = [build.HOST_ZSLAB_APP, str(cfg.dims[0]), str(cfg.size), str(cfg.cols), str(cfg.rows), str(frames), str(M), str(cfg.k), fin]
    nv, npx = int(np.prod(cfg.dims)), cfg.rows * cfg.cols
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    for mode in ("exchange", "recompute"):
        fout, idf = str(tmp_path / ("z_%s.bin" % mode)), str(tmp_path / ("id_%s" % mode))
        r = subprocess.run(base + [fout, idf, mode], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and "zslab_frame ok" in r.stdout, r.stdout + r.stderr
        raw = np.fromfile(fout, np.uint8)
        img = raw[:2 * npx * 16].view(np.float32).reshape(2, cfg.rows, cfg.cols, 4)
        zvol = raw[2 * npx * 16:].view(np.uint32).reshape(cfg.dims[2], cfg.dims[1], cfg.dims[0])
        assert np.array_equal(zvol, vol)
        assert np.array_equal(img[0].view(np.uint32), pts.view(np.uint32)) and np.array_equal(img[1].view(np.uint32), nrm.view(np.uint32))
    for r_ in range(4):
        fout = str(tmp_path / ("slab%d.bin" % r_))
        r = subprocess.run(base + [fout, str(tmp_path / "unused_id"), "exchange", "slab=%d/4" % r_], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        planes = np.fromfile(fout, np.uint8)[2 * npx * 16:].view(np.uint32).reshape(-1, cfg.dims[1], cfg.dims[0])
        z0 = r_ * cfg.dims[2] // 4
        assert planes.shape[0] == cfg.dims[2] // 4 and np.array_equal(planes, vol[z0:z0 + cfg.dims[2] // 4])
    # halo-recompute shards: setSlab(z0, n, halo, integrate_halo = true) integrates the halo planes too -- every STORED
    # plane equals the unsharded volume -- while the own range the ray-cast partitions rays by stays [z0, z0 + n)
    from dynamicfusion_amd import sharded
    halo = sharded.halo_planes(sc.trunc, cfg.raycast_step_factor, cfg.gradient_delta_factor, float(sc.vs[2]))
    for r_ in range(4):
        fout = str(tmp_path / ("slabr%d.bin" % r_))
        r = subprocess.run(base + [fout, str(tmp_path / "unused_id"), "recompute", "slab=%d/4" % r_], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "planes [%d, %d)" % (r_ * cfg.dims[2] // 4, (r_ + 1) * cfg.dims[2] // 4) in r.stdout, r.stdout + r.stderr
        planes = np.fromfile(fout, np.uint8)[2 * npx * 16:].view(np.uint32).reshape(-1, cfg.dims[1], cfg.dims[0])
        z0 = r_ * cfg.dims[2] // 4
        lo, hi = max(0, z0 - halo), min(cfg.dims[2], z0 + cfg.dims[2] // 4 + halo)
        assert planes.shape[0] == hi - lo and np.array_equal(planes, vol[lo:hi])
    # work-balanced (unequal) slabs: ZSlabComm::slabBounds gives the boundaries sharded.slab_bounds gives, and shards cut there
    # still equal the unsharded volume
    w = sharded.frustum_plane_weights(cfg.dims, cfg.size, sc.pose, sc.cam_poses[0], cfg.intr, cfg.cols, cfg.rows, depth_mm=sc.depths[0],
                                      trunc=sc.trunc, margin=0.1, samples=16) * np.linspace(0.05, 1.0, cfg.dims[2]) ** 3
    wf_ = str(tmp_path / "weights.f64")
    w.astype(np.float64).tofile(wf_)
    for world in (2, 4):
        want = sharded.slab_bounds(cfg.dims[2], world, halo, w)
        r = subprocess.run([build.HOST_ZSLAB_APP, "bounds", str(world), str(halo), wf_], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and [int(x) for x in r.stdout.strip().split(",")] == want, (r.stdout, want)
    # ... and the min-max boundaries of round 6 (halo planes counted), on this profile and on random ones
    rng_b = np.random.RandomState(17)
    for world, prof in [(2, w), (4, w), (3, rng_b.rand(cfg.dims[2]) ** 3 + 0.02), (4, np.concatenate([np.full(24, 0.02), np.linspace(0.05, 1.0, cfg.dims[2] - 24)]))]:
        wf2 = str(tmp_path / "weights_mm.f64")
        np.asarray(prof, np.float64).tofile(wf2)
        want = sharded.slab_bounds_minmax(cfg.dims[2], world, halo, prof)
        r = subprocess.run([build.HOST_ZSLAB_APP, "bounds-minmax", str(world), str(halo), wf2], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and [int(x) for x in r.stdout.strip().split(",")] == want, (r.stdout, want)
    bounds = sharded.slab_bounds(cfg.dims[2], 4, halo, w)
    assert bounds != sharded.slab_bounds(cfg.dims[2], 4)
    for r_ in range(4):
        fout = str(tmp_path / ("slabb%d.bin" % r_))
        r = subprocess.run(base + [fout, str(tmp_path / "unused_id"), "recompute", "slab=%d/4" % r_, "bounds=" + ",".join(str(b) for b in bounds)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        planes = np.fromfile(fout, np.uint8)[2 * npx * 16:].view(np.uint32).reshape(-1, cfg.dims[1], cfg.dims[0])
        lo, hi = max(0, bounds[r_] - halo), min(cfg.dims[2], bounds[r_ + 1] + halo)
        assert planes.shape[0] == hi - lo and np.array_equal(planes, vol[lo:hi])


@pytest.mark.parametrize("key_merge", ["direct", "ring"])
@pytest.mark.parametrize("rows", [False, "rs", "a2a"], ids=["root", "rows-rs", "rows-a2a"])
def test_cxx_zslab_rccl_calls_issued_with_one_rank(tmp_path, rows, key_merge):
    """Round 6: every RCCL call of ZSlabComm's casts REALLY issued on this one-GPU box (DFUSION_ZSLAB_FORCE_COLLECTIVES=1: with one rank each
    is the identity -- ncclAllReduce / ncclReduce / ncclReduceScatter over one rank, ncclSend / ncclRecv to oneself in a group,
    ncclAllGather of one piece): the ring key merge and the direct one (send / recv group -> dfusion_raycast_min_pieces -> ncclAllGather),
    the normals to the root, reduce-scattered by rows, and as the direct all-to-all -- types, counts, grouping and buffer sizes of the
    calls N > 1 ranks make, and the unsharded harness's bytes at the end."""
    cfg = synth.Config(64, 1.0, cols=160, rows=120, nodes=100, k=8)
    frames = 2
    sc = Scene(cfg, n_frames=frames)
    vol, pts, nrm, _, _ = run_harness(tmp_path, cfg, sc, frames, True)
    build.build_host()
    fin, fout, idf = str(tmp_path / "in.bin"), str(tmp_path / "zf.bin"), str(tmp_path / "idf")
    cmd = [build.HOST_ZSLAB_APP, str(cfg.dims[0]), str(cfg.size), str(cfg.cols), str(cfg.rows), str(frames), str(cfg.nodes), str(cfg.k), fin, fout, idf, "recompute"]
    if rows: cmd.append("rows")
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", DFUSION_ZSLAB_FORCE_COLLECTIVES="1", DFUSION_ZSLAB_KEY_MERGE=key_merge,
               DFUSION_ZSLAB_MERGE="a2a" if rows == "a2a" else "rs", DFUSION_ZSLAB_BCAST="ring" if key_merge == "ring" else "direct")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "zslab_frame ok: rank 0 of 1" in r.stdout, r.stdout + r.stderr
    npx = cfg.rows * cfg.cols
    raw = np.fromfile(fout, np.uint8)
    if rows:
        b = np.fromfile(fout + ".band0", np.uint8)
        r0, nr = [int(v) for v in b[:8].view(np.int32)]
        assert (r0, nr) == (0, cfg.rows)
        img = b[8:].view(np.float32).reshape(2, nr, cfg.cols, 4)
    else:
        img = raw[:2 * npx * 16].view(np.float32).reshape(2, cfg.rows, cfg.cols, 4)
    assert np.array_equal(img[0].view(np.uint32), pts.view(np.uint32)) and np.array_equal(img[1].view(np.uint32), nrm.view(np.uint32))
    assert np.array_equal(raw[2 * npx * 16:].view(np.uint32).reshape(cfg.dims[2], cfg.dims[1], cfg.dims[0]), vol)


@pytest.mark.parametrize("world,mode,rows", [(2, "exchange", False), (2, "recompute", False), (3, "recompute", False), (2, "recompute", True), (4, "recompute", True),
                                             (3, "recompute", "a2a"), (4, "recompute", "a2a")])
def test_cxx_zslab_collectives_with_more_than_one_rank(tmp_path, world, mode, rows):
    """VERDICT r3 #6 iii: the C++ collective SEQUENCE (ZSlabComm: frame-input broadcasts, halo exchange or recompute, march ->
    all-reduce(MIN) of the keys -> shade -> reduce(SUM) of the normals -> points of the keys) with MORE THAN ONE rank.  RCCL refuses two
    ranks on one device, so the ranks -- real processes, each with its own slab, all on cuda:0 -- use ZSlabComm's HOST_STAGED backend
    (DFUSION_ZSLAB_BACKEND=host: every collective staged through a shared-memory segment).  Rank 0's image and every rank's own
    planes must be the unsharded harness's bytes.  At most four ranks: with the test process itself that keeps the processes holding
    the GPU at five; at four ranks the image has 122 rows, so that the row bands do not divide it."""
    cfg = synth.Config(64, 1.0, cols=160, rows=122 if world == 4 else 120, nodes=100, k=8)
    frames = 2
    sc = Scene(cfg, n_frames=frames)
    vol, pts, nrm, _, _ = run_harness(tmp_path, cfg, sc, frames, True)
    build.build_host()
    fin, fout, idf = str(tmp_path / "in.bin"), str(tmp_path / "zn.bin"), str(tmp_path / "idn")
    cmd = [build.HOST_ZSLAB_APP, str(cfg.dims[0]), str(cfg.size), str(cfg.cols), str(cfg.rows), str(frames), str(cfg.nodes), str(cfg.k), fin, fout, idf, mode]
    if rows:                                                 # ZSlabComm::raycastRowBands: the normals reduce-scattered by pixel rows (122 rows over 4 ranks: padded)
        cmd.append("rows")
        if world == 4: cmd.append("bounds=0,16,24,32,64")                  # (64 planes, halo 8: two of the four slabs exactly 8 planes)
    procs = [subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                              env=dict(os.environ, WORLD_SIZE=str(world), RANK=str(r), LOCAL_RANK="0", DFUSION_ZSLAB_BACKEND="host",
                                       DFUSION_ZSLAB_MERGE="a2a" if rows == "a2a" else "rs",       # (round 5: the direct row-band merge -- pieces + dfusion_raycast_sum_pieces)
                                       DFUSION_ZSLAB_NONCE=str(os.getpid()), DFUSION_ZSLAB_HOST_SLOT_MB="16")) for r in range(world)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    import re
    alive = []
    for r, p in enumerate(procs):
        assert p.returncode == 0 and "zslab_frame ok: rank %d of %d" % (r, world) in outs[r], outs[r]
        alive.append(int(re.search(r"(\d+) alive blocks", outs[r]).group(1)))
    assert sum(alive) > 0                                    # WarpField::aliveBlocksPerLayer: the measured work profile of the re-balance
    npx = cfg.rows * cfg.cols
    raw = np.fromfile(fout, np.uint8)
    if rows:
        got_p, got_n, next_row = np.empty_like(pts), np.empty_like(nrm), 0
        for r in range(world):
            b = np.fromfile(fout + ".band%d" % r, np.uint8)
            r0, nr = [int(v) for v in b[:8].view(np.int32)]
            assert r0 == next_row
            body = b[8:].view(np.float32).reshape(2, nr, cfg.cols, 4)
            got_p[r0:r0 + nr], got_n[r0:r0 + nr] = body[0], body[1]
            next_row = r0 + nr
        assert next_row == cfg.rows
        assert np.array_equal(got_p.view(np.uint32), pts.view(np.uint32)) and np.array_equal(got_n.view(np.uint32), nrm.view(np.uint32))
    else:
        img = raw[:2 * npx * 16].view(np.float32).reshape(2, cfg.rows, cfg.cols, 4)
        assert np.array_equal(img[0].view(np.uint32), pts.view(np.uint32)) and np.array_equal(img[1].view(np.uint32), nrm.view(np.uint32))
    assert (~np.isnan(pts)).mean() > 0.2
    from dynamicfusion_amd import sharded
    bounds4 = [0, 16, 24, 32, 64]
    for r in range(world):
        z0, zn = (bounds4[r], bounds4[r + 1] - bounds4[r]) if (rows and world == 4) else sharded.slab_range(cfg.dims[2], r, world)
        planes = (raw[2 * npx * 16:] if r == 0 else np.fromfile(fout + ".r%d" % r, np.uint8)).view(np.uint32).reshape(-1, cfg.dims[1], cfg.dims[0])
        assert planes.shape[0] == zn and np.array_equal(planes, vol[z0:z0 + zn])


def test_cxx_headline_sequence_equals_the_python_mirror(tmp_path):
    """`headless_frame bench` (round 6: what bench.py reports as cxx_host) is the headline frame through the C++ mirror with nothing waiting
    for anything: WarpField::setTransformsDevice (node transforms already on the device) + computeDists + TsdfVolume::integrateAsync(...,
    warp) + raycast, `prime` frames, clear, the rest.  Its final volume and last ray-cast must be the Python mirror's over the same
    sequence, bit for bit -- the timing it prints is then a timing of the same work."""
    import torch
    from dynamicfusion_amd import Intr, TsdfVolume, WarpField, compute_dists, upload_u16
    build.build_host()
    cfg = synth.Config(64, 1.0, cols=160, rows=120, nodes=100, k=8)
    frames, prime, warmup = 6, 2, 1
    pos, sigma = synth.make_nodes(cfg)
    fin, fout = str(tmp_path / "hb_in.bin"), str(tmp_path / "hb_out.bin")
    with open(fin, "wb") as f:
        f.write(synth.aff12(cfg.volume_pose).tobytes()); f.write(np.asarray(cfg.intr, F32).tobytes())
        for i in range(frames):
            f.write(np.ascontiguousarray(synth.depth_frame(cfg, i), np.uint16).tobytes()); f.write(synth.aff12(synth.camera_pose(cfg, i)).tobytes())
        f.write(np.ascontiguousarray(pos, F32).tobytes())
        for i in range(frames):
            f.write(np.ascontiguousarray(synth.node_transforms(cfg, i), F32).tobytes())
        f.write(np.ascontiguousarray(sigma, F32).tobytes())
    r = subprocess.run([build.HOST_APP, "bench", str(cfg.dims[0]), str(cfg.size), str(cfg.cols), str(cfg.rows), str(frames), str(cfg.nodes), str(cfg.k),
                        str(prime), str(warmup), fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "cxx_host_ms_per_frame" in r.stdout, r.stdout + r.stderr
    # the same sequence through the Python mirror
    assert (cfg.trunc_dist, cfg.max_weight, cfg.raycast_step_factor, cfg.gradient_delta_factor) == (0.04, 64, 0.75, 0.5)     # (what the app sets)
    intr = Intr(*cfg.intr)
    vol = TsdfVolume(cfg.dims); vol.setSize([cfg.size] * 3); vol.setTruncDist(cfg.trunc_dist); vol.setMaxWeight(cfg.max_weight); vol.setPose(cfg.volume_pose)
    vol.setRaycastStepFactor(cfg.raycast_step_factor); vol.setGradientDeltaFactor(cfg.gradient_delta_factor)
    wf = WarpField(k=cfg.k); wf.init(pos, sigma=sigma, transforms=synth.node_transforms(cfg, 0))
    pts = torch.empty((cfg.rows, cfg.cols, 4), dtype=torch.float32, device="cuda"); nrm = torch.empty_like(pts)
    for i in range(frames):
        if i == prime: vol.clear()
        wf.set_transforms(torch.from_numpy(synth.node_transforms(cfg, i)).cuda())
        vol.integrate_warped(compute_dists(upload_u16(synth.depth_frame(cfg, i)), intr), synth.camera_pose(cfg, i), intr, wf)
        vol.raycast(synth.camera_pose(cfg, i), intr, pts, nrm)
    torch.cuda.synchronize()
    raw = np.fromfile(fout, np.uint8)
    nv, npx = int(np.prod(cfg.dims)), cfg.rows * cfg.cols
    assert raw.size == nv * 4 + 2 * npx * 16
    got_vol = raw[:nv * 4].view(np.uint32).reshape(cfg.dims[2], cfg.dims[1], cfg.dims[0])
    got = raw[nv * 4:].view(np.uint32).reshape(2, cfg.rows, cfg.cols, 4)
    want_vol = vol.download()
    assert (want_vol >> 16).any() and np.array_equal(got_vol, want_vol)
    assert np.array_equal(got[0], pts.cpu().numpy().view(np.uint32)) and np.array_equal(got[1], nrm.cpu().numpy().view(np.uint32))
    assert np.isfinite(pts.cpu().numpy()[..., 0]).mean() > 0.2


def test_cxx_warp_field_dqb_equals_reference_classes(tmp_path):
    """WarpField::DQB / getWeightsAndUpdateKNN / weighting of the C++ mirror (round 6; warp_field.hpp:66-72): the k-NN comes from the GPU
    (dfusion_knn), the weights and the blend are the reference's expressions on the host.  1000 points around 300 nodes with
    non-trivial transforms and per-node dg_w: every blend equals WarpField::DQB of the REFERENCE's classes (nanoflann + warp_field.cpp
    :203-241 through oracle/_ref) bit for bit; so do the weights and the neighbour lists against the oracle's k-NN."""
    build.build_host()
    cfg = synth.Config(64, 1.0, cols=160, rows=120, nodes=300, k=8)
    sc = Scene(cfg, n_frames=2)
    rng = np.random.RandomState(5)
    pts = (sc.pos[rng.randint(0, cfg.nodes, 1000)] + rng.normal(0, 0.05, (1000, 3))).astype(F32)
    fin, fout = str(tmp_path / "dqb_in.bin"), str(tmp_path / "dqb_out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([cfg.nodes, pts.shape[0], cfg.k], np.uint32).tobytes())
        f.write(sc.pos.astype(F32).tobytes()); f.write(sc.dqs[1].astype(F32).tobytes()); f.write(sc.sigma.astype(F32).tobytes()); f.write(pts.tobytes())
    r = subprocess.run([build.HOST_WARP_TESTS, "dqb", fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "warp_tests dqb ok" in r.stdout, r.stdout + r.stderr
    raw = np.fromfile(fout, np.uint8)
    n, k = pts.shape[0], cfg.k
    got = raw[:32 * n].view(F32).reshape(n, 8)
    w = raw[32 * n:32 * n + 4 * n * k].view(F32).reshape(n, k)
    ids = raw[32 * n + 4 * n * k:].view(np.uint32).reshape(n, k)
    have_ref = O.have_ref()
    want = O.dqb(sc.pos, sc.dqs[1], sc.sigma, pts, k, use_ref=have_ref)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%d of %d blends differ" % (int((got.view(np.uint32) != want.view(np.uint32)).any(1).sum()), n)
    idx, d2 = O.knn(sc.pos, pts, k, use_ref=have_ref)
    assert np.array_equal(ids.astype(np.int64), idx.astype(np.int64))
    sg = sc.sigma[idx].astype(F32)
    ww = np.exp((-d2.astype(F32) / (F32(2) * sg * sg)).astype(np.float64)).astype(F32)     # the argument in float, the exponential in double (warp_field.cpp:240)
    assert np.array_equal(w.view(np.uint32), ww.view(np.uint32))
    assert len(np.unique(got[:, 0])) > 100                                  # (not all the identity)


def test_cxx_reference_warp_test_suites():
    """The reference's own solver tests (tests/ceres_warp_test.cpp, tests/warp_test.cpp) compiled against the C++ mirror: same
    WarpField calls and inputs, same 1e-3 bound (WarpAndReverseTest: the data term's least-squares optimum, see the source)."""
    build.build_host()
    r = subprocess.run([build.HOST_WARP_TESTS], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.count("OK") == 5, r.stdout + r.stderr
