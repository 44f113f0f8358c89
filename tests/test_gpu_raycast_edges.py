"""The ray-cast (unsharded, depth variant, and the march / min-merge / shade / points-of-keys slab form) on volumes where the march's
window logic has work to do: noise puts first events of both kinds on each of the four window slots and most of them into the first
window, the back wall puts them behind dozens of skipped free-space steps and lets other rays leave without one, checkerboards and
z-parity planes flip the sign at every sample (tests/volume_cases.py; tests/test_volume_readers_rule.py shows the coverage without the
kernel).  Against O.raycast_points / O.raycast_depth: keys exactly, points and normals bit for bit where the oracle is not NaN and NaN
where it is."""
import numpy as np
import pytest
import torch

import mesh_ref as R
import oracle_lib as O
import volume_cases as VC
from dynamicfusion_amd import Intr, capi, download_u16, sharded, synth
from test_gpu_parity import make_gpu_volume

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL = -7.0


# ------------------------------------------------------------------------------------------------ scaffolding
def gpu_vol(sc, vol, vs=None, slab=None):
    """The scene's TsdfVolume holding `vol` (its stored planes, for a slab); vs: three voxel sizes in place of the scene's."""
    v = make_gpu_volume(sc, slab=slab)
    if vs is not None:
        v.setSize([float(F32(d) * vs[i]) for i, d in enumerate(sc.cfg.dims)])
        assert np.array_equal(v.getVoxelSize().view(np.uint32), np.array(vs, F32).view(np.uint32))
    v.upload(vol[v.z_store0:v.z_store0 + v.z_store_n])
    return v


def cast_args(v, cam):
    cam2vol = synth.affine_mul(synth.affine_inv(v.getPose()), np.asarray(cam, F32))
    rinv = np.linalg.inv(cam2vol[:3, :3].astype(np.float64)).astype(F32)
    return synth.aff12(cam2vol), rinv


def reproj_of(intr):
    return np.array([F32(1) / F32(intr.fx), F32(1) / F32(intr.fy), intr.cx, intr.cy], F32)


def oracle_volume(v, vol):
    return O.make_volume(vol, v.getDims(), v.getVoxelSize(), v.getTruncDist(), v.getMaxWeight())


def oracle_points(v, vol, cam, intr, cols, rows):
    aff, rinv = cast_args(v, cam)
    p, n, k, _ = O.raycast_points(oracle_volume(v, vol), aff, rinv, reproj_of(intr), cols, rows, v.getRaycastStepFactor(),
                                  v.getGradientDeltaFactor(), want_keys=True)
    return p, n, k


def gpu_points(v, cam, intr, cols, rows, out=None):
    """out: a list that receives the (sentinel-filled) output tensors before the call, for the caller that expects a refusal."""
    pts = torch.full((rows, cols, 4), SENTINEL, dtype=torch.float32, device="cuda")
    nrm = torch.full_like(pts, SENTINEL)
    keys = torch.full((rows, cols), 12345, dtype=torch.int32, device="cuda")
    if out is not None:
        out.extend([pts, nrm, keys])
    v.raycast(cam, intr, pts, nrm, keys=keys)
    torch.cuda.synchronize()
    return pts, nrm, keys


def assert_same_off_nan(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what + ": NaN masks differ at %d values" % int((np.isnan(got) != nan).sum())
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), what + ": bits differ"


def assert_cast_equals_oracle(v, vol, cam, intr, cols, rows, what):
    """-> (oracle points, oracle keys) after comparing the unsharded points cast with them."""
    pts, nrm, keys = gpu_points(v, cam, intr, cols, rows)
    wp, wn, wk = oracle_points(v, vol, cam, intr, cols, rows)
    assert np.array_equal(keys.cpu().numpy().view(np.uint32), wk), what + ": first events differ"
    assert_same_off_nan(pts.cpu().numpy(), wp, what + " points")
    assert_same_off_nan(nrm.cpu().numpy(), wn, what + " normals")
    return wp, wk


def cameras(sc):
    """name -> (4x4 camera pose, Intr); the image is cfg.cols x cfg.rows."""
    cfg = sc.cfg
    intr = Intr(*cfg.intr)
    centre = np.array([0.0, 0.0, 0.5 + cfg.size / 2])
    inside = R.rotated_pose().copy()
    inside[:3, 3] = centre                                               # in the middle of the volume, rolled and looking askew
    away = np.eye(4, dtype=F32)
    away[0, 0] = away[2, 2] = -1                                         # half a turn about y at the origin: the volume is behind
    # on the volume's axis, closer than pose 0, with no rotation; the principal point on a whole pixel, whose ray is (0, 0, 1) exactly
    on_axis = Intr(cfg.intr[0], cfg.intr[1], float(cfg.cols // 2), float(cfg.rows // 2))
    return {"pose0": (sc.cam_poses[0], intr), "pose1": (sc.cam_poses[1], intr), "inside": (inside, intr),
            "on_axis": (synth.translation(0.0, 0.0, 0.3), on_axis), "away": (away, intr)}


VOLUMES = {            # name: (dims, volume, voxel sizes or None for the scene's)
    "noise_0.0": (VC.NOISE_DIMS, lambda: VC.case("noise_0.0"), None),
    "noise_0.1": (VC.NOISE_DIMS, lambda: VC.case("noise_0.1"), None),
    "noise_0.6": (VC.NOISE_DIMS, lambda: VC.case("noise_0.6"), None),
    "back_wall": (VC.NOISE_DIMS, lambda: VC.case("back_wall"), None),
    "checker": (VC.NOISE_DIMS, lambda: VC.case("checker", VC.NOISE_DIMS), None),
    "z_parity": (VC.NOISE_DIMS, lambda: VC.case("z_parity", VC.NOISE_DIMS), None),
    "noise_36x20x44": ((36, 20, 44), lambda: VC.case("noise_0.1", (36, 20, 44)), None),
    "noise_24x11x13": ((24, 11, 13), lambda: VC.case("noise_0.1", (24, 11, 13)), None),
    "noise_aniso": (VC.NOISE_DIMS, lambda: VC.case("noise_0.1"), R.ANISO_VS),
}


# ---- 1. every volume from every camera
@pytest.mark.parametrize("name", list(VOLUMES))
def test_points_cast_equals_oracle(name):
    dims, make, vs = VOLUMES[name]
    vol = make()
    sc = VC.ray_scene(dims)
    v = gpu_vol(sc, vol, vs)
    cfg = sc.cfg
    seen = 0
    for cam_name, (cam, intr) in cameras(sc).items():
        wp, wk = assert_cast_equals_oracle(v, vol, cam, intr, cfg.cols, cfg.rows, "%s from %s" % (name, cam_name))
        if cam_name == "away":                                           # every pixel a miss, with the documented fill
            pts, nrm, keys = gpu_points(v, cam, intr, cfg.cols, cfg.rows)
            assert bool(torch.isnan(pts).all()) and bool(torch.isnan(nrm).all()) and bool((keys == -1).all())
            assert (wk == VC.NO_EVENT).all()
        elif cam_name == "on_axis":
            aff, _ = cast_args(v, cam)
            assert intr.cx == cfg.cols // 2 and np.array_equal(aff[:9].reshape(3, 3), np.eye(3, dtype=F32))
        seen += int(np.isfinite(wp[..., 0]).sum())
    small = synth.Config(dims, 1.0, cols=67, rows=45, nodes=0, k=4)      # a ragged image: the last tiles hang over both edges
    wp, _ = assert_cast_equals_oracle(v, vol, sc.cam_poses[1], Intr(*small.intr), 67, 45, name + " at 67x45")
    assert seen > 1000 and np.isfinite(wp[..., 0]).sum() > 100


# ---- 2. the depth variant
@pytest.mark.parametrize("name", ["noise_0.0", "noise_0.1", "noise_0.6"])
def test_depth_cast_equals_oracle(name):
    dims, make, vs = VOLUMES[name]
    vol = make()
    sc = VC.ray_scene(dims)
    v = gpu_vol(sc, vol, vs)
    cfg = sc.cfg
    for cam_name, (cam, intr) in cameras(sc).items():
        dep = torch.full((cfg.rows, cfg.cols), 777, dtype=torch.int16, device="cuda")
        nrm = torch.full((cfg.rows, cfg.cols, 4), SENTINEL, dtype=torch.float32, device="cuda")
        v.raycast(cam, intr, dep, nrm)
        torch.cuda.synchronize()
        aff, rinv = cast_args(v, cam)
        wd, wn = O.raycast_depth(oracle_volume(v, vol), aff, rinv, reproj_of(intr), cfg.cols, cfg.rows, v.getRaycastStepFactor(),
                                 v.getGradientDeltaFactor())
        assert np.array_equal(download_u16(dep), wd), "%s from %s: depth differs" % (name, cam_name)
        assert_same_off_nan(nrm.cpu().numpy(), wn, "%s from %s normals" % (name, cam_name))
        assert not cam_name.startswith("pose") or (wd > 0).sum() > 1000
        assert cam_name != "away" or not wd.any()


# ---- 3. the slab form: march per slab, min-merge, shade per slab summed as integers, points of the keys
SLABS = [(0, 9), (9, 22), (31, 13)]


@pytest.mark.parametrize("name", ["noise_0.1", "back_wall"])
def test_slab_form_equals_oracle_and_the_unsharded_cast(name):
    dims, make, _ = VOLUMES[name]
    vol = make()
    sc = VC.ray_scene(dims)
    cfg = sc.cfg
    rows, cols = cfg.rows, cfg.cols
    full = gpu_vol(sc, vol)
    halo = sharded.halo_planes(sc.trunc, cfg.raycast_step_factor, cfg.gradient_delta_factor, float(sc.vs[2]))
    assert sum(n for _, n in SLABS) == dims[2] and halo > 0
    slabs = [gpu_vol(sc, vol, slab=(z0, zn, halo)) for z0, zn in SLABS]
    world = len(slabs)
    cams = cameras(sc)
    seen = 0
    for cam_name in ("pose1", "inside", "pose0"):
        cam, intr = cams[cam_name]
        what = "%s from %s" % (name, cam_name)
        wp, wn, wk = oracle_points(full, vol, cam, intr, cols, rows)
        p0, n0, k0 = gpu_points(full, cam, intr, cols, rows)
        pieces = torch.empty((world, rows, cols), dtype=torch.int64, device="cuda")
        for r, s in enumerate(slabs):
            s.raycast_march(cam, intr, pieces[r], rank=r)
        merged = torch.empty((rows, cols), dtype=torch.int64, device="cuda")
        capi.check(capi.lib().dfusion_raycast_min_pieces(pieces.data_ptr(), world, rows * cols, merged.data_ptr(), None), "dfusion_raycast_min_pieces")
        assert torch.equal(merged, pieces.min(0).values)
        event = torch.where(merged == sharded.KEY_NONE, torch.full_like(merged, 0xFFFFFFFF), (merged >> 39) & 0xFFFFFF)
        assert np.array_equal(event.cpu().numpy().astype(np.uint32), wk), what + ": merged event index / kind differ from the oracle"
        assert torch.equal(event, k0.to(torch.int64) & 0xFFFFFFFF), what
        acc = torch.zeros((2, rows, cols, 4), dtype=torch.int32, device="cuda")
        for s in slabs:
            p = torch.empty((rows, cols, 4), dtype=torch.float32, device="cuda")
            n = torch.empty_like(p)
            s.raycast_shade(cam, intr, merged, p, n)
            acc[0] += p.view(torch.int32)
            acc[1] += n.view(torch.int32)
        p3 = torch.full((rows, cols, 4), SENTINEL, dtype=torch.float32, device="cuda")
        slabs[1].raycast_points_of_keys(cam, intr, merged, acc[1].view(torch.float32), p3)
        torch.cuda.synchronize()
        for got, label in ((acc[0].view(torch.float32), "summed points"), (p3, "points of keys")):
            assert_same_off_nan(got.cpu().numpy(), wp, what + " " + label)
            assert torch.equal(got.view(torch.int32), p0.view(torch.int32)), what + " " + label + " differ from the unsharded cast"
        assert_same_off_nan(acc[1].view(torch.float32).cpu().numpy(), wn, what + " summed normals")
        assert torch.equal(acc[1], n0.view(torch.int32)), what + ": summed normals differ from the unsharded cast"
        seen += int(np.isfinite(wp[..., 0]).sum())
    assert seen > 5000


# ---- 4. volumes of a few voxels
@pytest.mark.parametrize("dims", [(4, 2, 2), (4, 7, 3), (8, 1, 5)], ids=["4x2x2", "4x7x3", "8x1x5"])
def test_tiny_volumes(dims):
    vol = R.noise_volume(dims, 3, 0.0)
    sc = VC.ray_scene(dims)
    cfg = sc.cfg
    v = gpu_vol(sc, vol)
    for cam_name, (cam, intr) in cameras(sc).items():
        out = []
        try:
            pts, nrm, keys = gpu_points(v, cam, intr, cfg.cols, cfg.rows, out)
        except capi.DfusionError as e:                                   # a refused shape: said so, and nothing written
            torch.cuda.synchronize()
            assert "code 100001" in str(e)
            assert bool((out[0] == SENTINEL).all()) and bool((out[1] == SENTINEL).all()) and bool((out[2] == 12345).all())
            continue
        wp, wn, wk = oracle_points(v, vol, cam, intr, cfg.cols, cfg.rows)
        what = "%dx%dx%d from %s" % (dims + (cam_name,))
        assert np.array_equal(keys.cpu().numpy().view(np.uint32), wk), what + ": first events differ"
        assert_same_off_nan(pts.cpu().numpy(), wp, what + " points")
        assert_same_off_nan(nrm.cpu().numpy(), wn, what + " normals")
