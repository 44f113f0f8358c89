"""dfusion_color_* / ColorVolume (dynamicfusion_amd/csrc/dfusion_color.hip) against the numpy restatement of the rule, tests/color_ref.py:
the colour volume's bytes after every frame, the counters and the fetched colours, bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import color_ref as CR
from dynamicfusion_amd import ColorVolume, Intr, TsdfVolume, WarpField, capi, synth, upload_u16

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID = 100001
MAXW = 2                                      # so that the cap engages within the three frames


def gpu_volume(S, f, slab=None):
    """A TsdfVolume of the scene's geometry holding the oracle's TSDF after frame f (its stored planes)."""
    cfg, sc = S.cfg, S.sc
    v = TsdfVolume(cfg.dims, slab=slab)
    v.setSize([cfg.size] * 3); v.setTruncDist(cfg.trunc_dist); v.setMaxWeight(cfg.max_weight); v.setPose(sc.pose)
    assert np.array_equal(v.getVoxelSize().view(np.uint32), sc.vs.view(np.uint32)) and v.getTruncDist() == sc.trunc
    v.upload(S.vols[f][v.z_store0:v.z_store0 + v.z_store_n])
    return v


def slab4(v):
    return (v.z_store0, v.z_store_n, v.z_own0, v.z_own_n)


def pitched(arr, pad, x0):
    """numpy [rows, cols(, 4)] -> a view at pixel column x0 of a wider sentinel-filled device buffer (rows `pad` pixels longer)."""
    a = np.ascontiguousarray(arr)
    t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)
    shape = (a.shape[0], x0 + a.shape[1] + pad) + a.shape[2:]
    buf = torch.full(shape, 0x55, dtype=t.dtype, device="cuda")
    buf[:, x0:x0 + a.shape[1]].copy_(t.cuda())
    return buf[:, x0:x0 + a.shape[1]]


def dense(arr):
    a = np.ascontiguousarray(arr)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def far_nodes(S):
    """Nodes on the x < -0.25 end of the scene only, with a dg_w of 1 cm: the blend weights of voxels tens of centimetres away underflow to
    0, the blended rotation cannot be normalised and the warp is NaN -- those voxels are skipped."""
    cfg = synth.Config(S.cfg.dims, S.cfg.size, cols=S.cfg.cols, rows=S.cfg.rows, nodes=60, k=4)
    pos, _ = synth.make_nodes(cfg)
    pos = pos[pos[:, 0] < -0.25][:12]
    assert len(pos) >= 8
    return pos, synth.node_transforms(synth.Config(S.cfg.dims, S.cfg.size, nodes=len(pos)), 3), np.full(len(pos), 0.01, F32)


@functools.lru_cache(None)
def reference(dims, cols, rows, nodes, k):
    """The restatement's colour volume after each of the three frames (+ counts); nodes: 0 = rigid, -1 = the far nodes.  Shared, read-only."""
    S = CR.scene(dims, cols, rows, nodes=max(nodes, 0), k=k or 4)
    sc = S.sc
    color = np.zeros(S.vols[0].shape + (4,), np.uint8)
    out = []
    for f in range(3):
        nd = None if nodes == 0 else far_nodes(S) if nodes < 0 else (sc.pos, sc.dqs[f], sc.sigma)
        n_sel, n_fused, _, obs = CR.integrate(color, S.vols[f], S.cfg.dims, sc.vs, sc.trunc, S.images[f], sc.dists[f], S.vol2world, S.world2cam(f),
                                              sc.intr, nodes=nd, k=k, max_weight=MAXW)
        out.append((color.copy(), n_sel, n_fused))
    return S, out


def make_field(S, nodes, k, f, index, volume):
    sc = S.sc
    pos, dq, sigma = far_nodes(S) if nodes < 0 else (sc.pos, sc.dqs[f], sc.sigma)
    wf = WarpField(k=k, voxel_table=False, weight_table=False)
    wf.init(pos, sigma=sigma, transforms=dq)
    if index:
        wf.ensure_index(volume, k)                                       # brick lists only
        info = (C.c_ulonglong(), C.c_uint(), C.c_int())
        capi.check(capi.lib().dfusion_warp_index_info(wf.handle, *(C.byref(i) for i in info)))
        assert info[2].value >= k and info[0].value > 0
    return wf


def run_frames(dims, cols, rows, nodes, k, index=False, pad=None):
    S, ref = reference(dims, cols, rows, nodes, k)
    sc, intr = S.sc, Intr(*S.cfg.intr)
    vol = gpu_volume(S, 0)
    cv = ColorVolume(vol)
    for f in range(3):
        vol.upload(S.vols[f])
        wf = make_field(S, nodes, k, f, index, vol) if nodes else None
        image = pitched(S.images[f], *pad) if pad else dense(S.images[f])
        dists = pitched(sc.dists[f], pad[0] + 3, pad[1] + 1) if pad else upload_u16(sc.dists[f])
        counts = cv.integrate(image, dists, sc.cam_poses[f], intr, warp_field=wf, k=k if nodes else None, max_weight=MAXW, return_counts=True)
        want, n_sel, n_fused = ref[f]
        got = cv.download()
        assert counts.tolist() == [n_sel, n_fused], (f, counts.tolist(), n_sel, n_fused)
        assert np.array_equal(got, want), (f, int((got != want).any(-1).sum()))
    final = ref[2][0]
    assert (final[..., 3] == MAXW).sum() > 100 and final[..., 3].max() == MAXW                 # the cap engaged
    assert len(np.unique(final[final[..., 3] > 0][:, :3], axis=0)) > 2                         # and averages of the two paints exist
    return S, ref


@pytest.mark.parametrize("dims,cols,rows,pad", [(32, 80, 60, None), (64, 160, 120, None), ((40, 24, 16), 80, 60, (5, 3)), (32, 160, 120, (1, 0))],
                         ids=["32-80x60", "64-160x120", "40x24x16-80x60-pitched", "32-160x120-pitched"])
def test_rigid_frames_equal_the_restatement(dims, cols, rows, pad):
    S, ref = run_frames(dims, cols, rows, 0, 0, pad=pad)
    assert ref[0][2] > 300


@pytest.mark.parametrize("index", [False, True], ids=["scan", "bricks"])
@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("nodes", [20, 64, 300])
def test_warped_frames_equal_the_restatement(nodes, k, index):
    S, ref = run_frames(32, 80, 60, nodes, k, index=index)
    rigid = reference(32, 80, 60, 0, 0)[1]
    assert ref[0][2] > 300 and not np.array_equal(ref[2][0], rigid[2][0])                     # the warp moved some look-ups


@pytest.mark.parametrize("index", [False, True], ids=["scan", "bricks"])
def test_nan_warps_are_skipped(index):
    S, ref = run_frames(32, 80, 60, -1, 4, index=index)
    rigid = reference(32, 80, 60, 0, 0)[1]
    assert 100 < ref[0][2] < rigid[0][2] - 100 and ref[0][1] == rigid[0][1]                   # as many selected, far fewer fused


@pytest.mark.parametrize("nodes", [0, 20], ids=["rigid", "warped"])
def test_capacity_exact_short_and_too_large(nodes):
    k = 4 if nodes else 0
    S, ref = reference(32, 80, 60, nodes, k)
    sc, intr = S.sc, Intr(*S.cfg.intr)
    vol = gpu_volume(S, 0)
    wf = make_field(S, nodes, k, 0, True, vol) if nodes else None
    n_sel = ref[0][1]
    nd = (sc.pos, sc.dqs[0], sc.sigma) if nodes else None
    for cap in (n_sel, n_sel - 1, 10 * n_sel, 7):
        want = np.zeros(S.vols[0].shape + (4,), np.uint8)
        r_sel, r_fused, idx, obs = CR.integrate(want, S.vols[0], S.cfg.dims, sc.vs, sc.trunc, S.images[0], sc.dists[0], S.vol2world, S.world2cam(0),
                                                sc.intr, nodes=nd, k=k, max_weight=MAXW, capacity=cap)
        cv = ColorVolume(vol)
        counts = cv.integrate(dense(S.images[0]), upload_u16(sc.dists[0]), sc.cam_poses[0], intr, warp_field=wf, k=k or None, max_weight=MAXW,
                              capacity=cap, return_counts=True)
        assert counts.tolist() == [n_sel, r_fused] and r_sel == n_sel and len(idx) == min(cap, n_sel)
        assert np.array_equal(cv.download(), want), cap
    # without the counters (both NULL) the bytes are the same
    cv = ColorVolume(vol)
    assert cv.integrate(dense(S.images[0]), upload_u16(sc.dists[0]), sc.cam_poses[0], intr, warp_field=wf, k=k or None, max_weight=MAXW) is None
    assert np.array_equal(cv.download(), ref[0][0])


@pytest.mark.parametrize("nodes", [0, 64], ids=["rigid", "warped"])
def test_two_z_slabs_equal_the_unsharded_volume_on_their_own_planes(nodes):
    k = 8 if nodes else 0
    S, ref = reference(32, 80, 60, nodes, k)
    sc, intr = S.sc, Intr(*S.cfg.intr)
    for z0, zn in ((0, 13), (13, 19)):
        vol = gpu_volume(S, 0, slab=(z0, zn, 2))
        cv = ColorVolume(vol)
        assert cv.data().shape[0] == vol.z_store_n
        for f in range(3):
            vol.upload(S.vols[f][vol.z_store0:vol.z_store0 + vol.z_store_n])
            wf = make_field(S, nodes, k, f, True, vol) if nodes else None
            cv.integrate(dense(S.images[f]), upload_u16(sc.dists[f]), sc.cam_poses[f], intr, warp_field=wf, k=k or None, max_weight=MAXW)
            got = cv.download()
            own = slice(z0 - vol.z_store0, z0 - vol.z_store0 + zn)
            assert np.array_equal(got[own], ref[f][0][z0:z0 + zn]), (z0, f)
            halo = np.ones(vol.z_store_n, bool); halo[own] = False
            assert not got[halo].any()                                                        # only the own planes are written
            want = np.zeros((vol.z_store_n,) + got.shape[1:], np.uint8) if f == 0 else want
            CR.integrate(want, S.vols[f][vol.z_store0:vol.z_store0 + vol.z_store_n], S.cfg.dims, sc.vs, sc.trunc, S.images[f], sc.dists[f], S.vol2world,
                         S.world2cam(f), sc.intr, nodes=(sc.pos, sc.dqs[f], sc.sigma) if nodes else None, k=k, max_weight=MAXW, slab=slab4(vol))
            assert np.array_equal(got, want)


def test_fetch_equals_the_restatement():
    S, ref = reference(32, 80, 60, 0, 0)
    sc, cfg = S.sc, S.cfg
    vol = gpu_volume(S, 2)
    cv = ColorVolume(vol)
    cv.upload(ref[2][0])
    vertices, _ = vol.fetchMesh()
    cloud = vol.fetchCloud()
    vs = sc.vs.astype(np.float64)
    lo = sc.pose[:3, 3].astype(np.float64)
    rng = np.random.default_rng(3)
    extra = np.zeros((4096 + 12, 4), F32)
    extra[:2048, :3] = lo + rng.uniform(-3, 35, (2048, 3)) * vs                               # in and around the volume
    edge = np.stack([rng.uniform(0, 32, 2048), rng.uniform(0, 32, 2048), rng.uniform(24, 29, 2048)], 1)      # around the back plane ...
    edge[:1024, 0] = 30.0 + rng.uniform(0, 2.5, 1024)                                          # ... on the last cell in x and just past it
    edge[1024:, 1] = 30.0 + rng.uniform(0, 2.5, 1024)                                          # ... and in y
    extra[2048:4096, :3] = lo + edge * vs
    extra[4096:, :3] = lo + 16 * vs
    extra[4096, 0] = np.nan; extra[4097, 1] = np.nan; extra[4098, 2] = np.nan; extra[4099, 0] = np.inf; extra[4100, 2] = -np.inf
    extra[4101, :3] = 1e30; extra[4102, :3] = -1e30; extra[4103, :3] = 3e38; extra[4104, :3] = lo - 1e-7
    pts = torch.cat([vertices, cloud, torch.from_numpy(extra).cuda()]).contiguous()
    got = cv.fetchColors(pts).cpu().numpy()
    want = CR.fetch(ref[2][0], cfg.dims, sc.vs, S.world2vol, pts.cpu().numpy())
    nv, nc = len(vertices), len(cloud)
    assert nv > 3000 and nc > 1000 and (want[:nv, 3] == 255).mean() > 0.9 and (want[nv:nv + nc, 3] == 255).mean() > 0.9
    tail = want[nv + nc:]
    assert 0 < (tail[:2048, 3] == 255).sum() < 2048 and 0 < (tail[2048:4096, 3] == 255).sum() < 2048 and not tail[4096:4104].any()
    assert np.array_equal(got, want), int((got != want).any(1).sum())
    assert cv.fetchColors(pts[:0]).shape == (0, 4)
    # a slab's colour volume answers with its stored planes only
    sv = gpu_volume(S, 2, slab=(10, 9, 1))
    scv = ColorVolume(sv)
    scv.upload(ref[2][0][sv.z_store0:sv.z_store0 + sv.z_store_n])
    got = scv.fetchColors(pts).cpu().numpy()
    want_s = CR.fetch(ref[2][0][sv.z_store0:sv.z_store0 + sv.z_store_n], cfg.dims, sc.vs, S.world2vol, pts.cpu().numpy(), slab=slab4(sv))
    assert np.array_equal(got, want_s) and 0 < (want_s[:, 3] == 255).sum() < (want[:, 3] == 255).sum()


def test_geometry_is_read_and_never_written():
    S, _ = reference(32, 80, 60, 20, 4)
    sc, intr = S.sc, Intr(*S.cfg.intr)
    vol = gpu_volume(S, 2)
    before = vol.download().copy()
    v0, t0 = (x.clone() for x in vol.fetchMesh())
    cv = ColorVolume(vol)
    for wf in (None, make_field(S, 20, 4, 2, True, vol)):
        cv.integrate(dense(S.images[2]), upload_u16(sc.dists[2]), sc.cam_poses[2], intr, warp_field=wf)
    cv.fetchColors(v0)
    torch.cuda.synchronize()
    v1, t1 = vol.fetchMesh()
    assert np.array_equal(vol.download(), before) and cv.download()[..., 3].max() == 2
    assert torch.equal(v0.view(torch.int32), v1.view(torch.int32)) and torch.equal(t0, t1) and len(t0) > 1000


def test_invalid_arguments_are_rejected():
    S, _ = reference(32, 80, 60, 20, 4)
    sc, cfg = S.sc, S.cfg
    vol = gpu_volume(S, 0)
    cv = ColorVolume(vol)
    wf = make_field(S, 20, 4, 0, False, vol)
    L = capi.lib()
    img, dists = dense(S.images[0]), upload_u16(sc.dists[0])
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    aff = capi.floats(S.vol2world)
    w2c = capi.floats(S.world2cam(0))
    proj = capi.floats(cfg.intr)

    def call(rgb=p(img), rgb_pitch=cfg.cols * 4, d=p(dists), d_pitch=cfg.cols * 2, cols=cfg.cols, rows=cfg.rows, v=None, color=p(cv.data()), a=aff, w=w2c,
             pr=proj, field=wf.handle, k=4, band=1.0, max_weight=64, capacity=1000):
        return L.dfusion_color_integrate(rgb, rgb_pitch, d, d_pitch, cols, rows, vol.c_volume() if v is None else v, None, color, a, w, pr, field, k,
                                         band, max_weight, capacity, p(cnt), C.c_void_p(cnt.data_ptr() + 8), None)
    assert call() == 0
    assert call(field=None, k=0) == 0 and call(field=None, k=99) == 0                          # k is not looked at without a warp field
    for bad in (dict(rgb=None), dict(d=None), dict(color=None), dict(a=None), dict(w=None), dict(pr=None), dict(v=capi.DfVolume()),
                dict(band=0.0), dict(band=-0.5), dict(band=1.0001), dict(band=float("nan")), dict(max_weight=0), dict(max_weight=256),
                dict(max_weight=-3), dict(capacity=0), dict(capacity=-5), dict(k=0), dict(k=9), dict(k=-1), dict(rgb_pitch=cfg.cols * 4 - 4),
                dict(d_pitch=cfg.cols * 2 - 2), dict(cols=0), dict(rows=0)):
        assert call(**bad) == INVALID, bad
    few = WarpField(k=4, voxel_table=False, weight_table=False)
    few.init(sc.pos[:3], sigma=0.1)
    assert call(field=few.handle, k=4) == INVALID and call(field=few.handle, k=3) == 0         # fewer nodes than k
    g = vol.c_volume()
    out = torch.zeros((4, 4), dtype=torch.uint8, device="cuda")
    pts = torch.zeros((4, 4), dtype=torch.float32, device="cuda")
    w2v = capi.floats(S.world2vol)
    assert L.dfusion_color_clear(None, g, None, None) == INVALID and L.dfusion_color_clear(p(cv.data()), capi.DfVolume(), None, None) == INVALID
    assert L.dfusion_color_fetch(None, g, None, w2v, p(pts), 4, p(out), None) == INVALID
    assert L.dfusion_color_fetch(p(cv.data()), g, None, None, p(pts), 4, p(out), None) == INVALID
    assert L.dfusion_color_fetch(p(cv.data()), g, None, w2v, None, 4, p(out), None) == INVALID
    assert L.dfusion_color_fetch(p(cv.data()), g, None, w2v, p(pts), 4, None, None) == INVALID
    assert L.dfusion_color_fetch(p(cv.data()), capi.DfVolume(), None, w2v, p(pts), 4, p(out), None) == INVALID
    assert L.dfusion_color_fetch(p(cv.data()), g, None, w2v, p(pts), 4, p(out), None) == 0
    bad_slab = capi.DfSlab(0, 40, 0, 40)
    assert L.dfusion_color_clear(p(cv.data()), g, C.byref(bad_slab), None) == INVALID
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        cv.integrate(img[:, :, :3], dists, sc.cam_poses[0], Intr(*cfg.intr))
    with pytest.raises(ValueError):
        cv.integrate(img, dists[:-1], sc.cam_poses[0], Intr(*cfg.intr))


def test_clear_zeroes_the_stored_planes():
    S, ref = reference(32, 80, 60, 0, 0)
    vol = gpu_volume(S, 0)
    cv = ColorVolume(vol)
    cv.upload(ref[2][0])
    assert cv.download().any()
    cv.clear()
    assert not cv.download().any()
