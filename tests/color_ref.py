"""numpy restatement of the colour volume's rule (include/dfusion.h dfusion_color_*): select, warp and project, fuse, fetch.
f32 arithmetic in the stated order (mesh_ref.fma32 / aff_mul restate the fused forms exactly), integers for the running average; the
warp is the oracle's (oracle_lib.warp_points: nanoflann's tie order, DQB).  Nothing is taken from the HIP source.  Also the test paint:
images synthesised from a depth frame and a pose by colouring every pixel by the world position it sees."""
import functools

import numpy as np

import oracle_lib as O
from mesh_ref import aff_mul, fma32

F32 = np.float32
IDENT12 = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F32)


def h2f(u16):
    return np.ascontiguousarray(u16, np.uint16).view(np.float16).astype(F32)


# ------------------------------------------------------------------------------------------------ select
def select(vol_u32, dims, slab, band):
    """vol_u32 [z_store_n, Y, X]; slab = (z_store0, z_store_n, z_own0, z_own_n) or None -> the STORED linear indices (ascending) of
    the voxels of the own planes with weight > 0 and |tsdf| < band."""
    X, Y, Z = dims
    z_store0, z_store_n, z_own0, z_own_n = slab if slab is not None else (0, Z, 0, Z)
    v = vol_u32.reshape(-1, Y, X)
    tsdf = h2f((v & 0xffff).astype(np.uint16))
    with np.errstate(invalid="ignore"):
        sel = ((v >> 16) != 0) & (np.abs(tsdf) < F32(band))
    own = np.zeros(v.shape[0], bool)
    own[z_own0 - z_store0:z_own0 - z_store0 + z_own_n] = True
    sel &= own[:, None, None]
    return np.flatnonzero(sel.reshape(-1))


def voxel_positions(idx, dims, vs, vol2world, slab):
    """x_c = vol2world * (x vsx, y vsy, z vsz) of stored linear indices (z is the GLOBAL plane)."""
    X, Y, Z = dims
    z_store0 = slab[0] if slab is not None else 0
    x = idx % X
    y = (idx // X) % Y
    z = idx // (X * Y) + z_store0
    V = np.stack([x.astype(F32) * F32(vs[0]), y.astype(F32) * F32(vs[1]), z.astype(F32) * F32(vs[2])], 1)
    return aff_mul(vol2world, V)


# ------------------------------------------------------------------------------------------------ warp and project
def warp(xc, nodes, k):
    """nodes = (pos [M,3], dq [M,8], sigma [M]) or None -> x_w (NaN rows where the blend has no finite result)."""
    if nodes is None:
        return xc
    pos, dq, sigma = nodes
    out, _ = O.warp_points(pos, dq, sigma, xc, None, k, IDENT12)
    return out


def project(xw, world2cam, proj, dists, band, trunc):
    """-> (observed bool [n], row int [n], col int [n]): the projector and gates of tsdf_update and the occlusion test."""
    rows, cols = dists.shape
    vc = aff_mul(world2cam, np.ascontiguousarray(xw, F32))
    fx, fy, cx, cy = (np.full(len(vc), F32(p), F32) for p in proj)
    with np.errstate(all="ignore"):
        u = fma32(fx, vc[:, 0] / vc[:, 2], cx)
        v = fma32(fy, vc[:, 1] / vc[:, 2], cy)
        ok = (u >= 0) & (v >= 0) & (u < F32(cols)) & (v < F32(rows))
        ui = np.where(ok, u, 0).astype(np.int64)
        vi = np.where(ok, v, 0).astype(np.int64)
        Dp = h2f(dists)[vi, ui]
        ok &= ~((Dp == 0) | (vc[:, 2] <= 0))
        dot = fma32(vc[:, 0], vc[:, 0], fma32(vc[:, 1], vc[:, 1], vc[:, 2] * vc[:, 2]))
        sdf = Dp - np.sqrt(dot)
        ok &= np.abs(sdf) < F32(band) * F32(trunc)
    return ok, vi, ui


# ------------------------------------------------------------------------------------------------ fuse
def fuse(color_u8, idx, pixels, max_weight):
    """color_u8 [..., 4] (modified in place at the stored linear indices idx, each at most once); pixels [n, >= 3] uint8."""
    flat = color_u8.reshape(-1, 4)
    old = flat[idx].astype(np.int64)
    w = old[:, 3]
    c = pixels[:, :3].astype(np.int64)
    new = (old[:, :3] * w[:, None] + c + ((w[:, None] + 1) >> 1)) // (w[:, None] + 1)
    wn = np.minimum(w + 1, int(max_weight))
    flat[idx] = np.concatenate([new, wn[:, None]], 1).astype(np.uint8)


def integrate(color_u8, vol_u32, dims, vs, trunc, image, dists, vol2world, world2cam, proj, nodes=None, k=0, band=1.0, max_weight=64,
              capacity=None, slab=None):
    """One frame into color_u8 [z_store_n, Y, X, 4], in place.  -> (n_selected, n_fused, idx processed, observed among them)."""
    idx_all = select(vol_u32, dims, slab, band)
    idx = idx_all if capacity is None else idx_all[:int(capacity)]
    xw = warp(voxel_positions(idx, dims, vs, vol2world, slab), nodes, k)
    obs, vi, ui = project(xw, world2cam, proj, dists, band, trunc)
    fuse(color_u8, idx[obs], image[vi[obs], ui[obs]], max_weight)
    return len(idx_all), int(obs.sum()), idx, obs


# ------------------------------------------------------------------------------------------------ fetch
def fetch(color_u8, dims, vs, world2vol, points, slab=None):
    """points [n, 4] float32 (world) -> uint8 [n, 4]."""
    X, Y, Z = dims
    z_store0, z_store_n = (slab[0], slab[1]) if slab is not None else (0, Z)
    col = color_u8.reshape(z_store_n, Y, X, 4)
    pts = np.ascontiguousarray(points, F32)[:, :3]
    n = len(pts)
    out = np.zeros((n, 4), np.uint8)
    finite = np.isfinite(pts).all(1)
    with np.errstate(all="ignore"):
        p = aff_mul(world2vol, np.where(finite[:, None], pts, F32(0)))
        cf = np.stack([p[:, i] / F32(vs[i]) for i in range(3)], 1)
        g = np.floor(cf)
        fr = cf - g
        one = F32(1)
        sw = np.zeros(n, F32)
        sc = np.zeros((n, 3), F32)
        for dx in (0, 1):
            for dy in (0, 1):
                for dz in (0, 1):                                        # the oracle's interpolate order: z fastest, then y, then x
                    tx, ty, tz = g[:, 0] + F32(dx), g[:, 1] + F32(dy), g[:, 2] + F32(dz)
                    inside = (tx >= 0) & (tx < F32(X)) & (ty >= 0) & (ty < F32(Y)) & (tz >= F32(z_store0)) & (tz < F32(z_store0 + z_store_n))
                    ix = np.where(inside, tx, 0).astype(np.int64)
                    iy = np.where(inside, ty, 0).astype(np.int64)
                    iz = np.where(inside, tz, z_store0).astype(np.int64) - z_store0
                    c = col[iz, iy, ix]
                    use = inside & (c[:, 3] != 0)
                    wt = ((fr[:, 0] if dx else one - fr[:, 0]) * (fr[:, 1] if dy else one - fr[:, 1])) * (fr[:, 2] if dz else one - fr[:, 2])
                    wt = np.where(use, wt, F32(0)).astype(F32)           # (adding +0 changes no bit of a sum that starts at +0)
                    sw = sw + wt
                    for ch in range(3):
                        sc[:, ch] = sc[:, ch] + np.where(use, c[:, ch].astype(F32) * wt, F32(0)).astype(F32)
        have = finite & (sw > 0)
        q = np.floor(sc / np.where(have, sw, one)[:, None] + F32(0.5))
    out[have, :3] = np.minimum(255, q[have].astype(np.int64)).astype(np.uint8)
    out[have, 3] = 255
    return out


# ------------------------------------------------------------------------------------------------ the test paint
BACKGROUND = (9, 9, 9)
HALF_A, HALF_B = (200, 40, 90), (30, 170, 250)
CHECK_A, CHECK_B = (240, 230, 20), (15, 60, 130)


def backproject(depth_u16, cam_pose, intr):
    """World position seen by every pixel (f64) and whether the pixel has a depth."""
    rows, cols = depth_u16.shape
    fx, fy, cx, cy = (float(v) for v in intr)
    xs, ys = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    z = depth_u16.astype(np.float64) * 0.001
    pc = np.stack([(xs - cx) / fx * z, (ys - cy) / fy * z, z], -1)
    pose = np.asarray(cam_pose, np.float64)
    return pc @ pose[:3, :3].T + pose[:3, 3], depth_u16 != 0


def paint_half_space(depth_u16, cam_pose, intr, x0):
    """uint8 [rows, cols, 4]: HALF_A where the pixel sees a world point with x < x0, else HALF_B; BACKGROUND without a depth; 4th byte 77."""
    pw, have = backproject(depth_u16, cam_pose, intr)
    img = np.empty(depth_u16.shape + (4,), np.uint8)
    img[..., :3] = np.where((pw[..., 0] < x0)[..., None], np.array(HALF_A, np.uint8), np.array(HALF_B, np.uint8))
    img[~have, :3] = BACKGROUND
    img[..., 3] = 77
    return img


def paint_checker(depth_u16, cam_pose, intr, cell=0.05):
    """uint8 [rows, cols, 4]: a 3-D checker of `cell` metres in world space."""
    pw, have = backproject(depth_u16, cam_pose, intr)
    odd = (np.floor(pw / cell).astype(np.int64).sum(-1) & 1).astype(bool)
    img = np.empty(depth_u16.shape + (4,), np.uint8)
    img[..., :3] = np.where(odd[..., None], np.array(CHECK_A, np.uint8), np.array(CHECK_B, np.uint8))
    img[~have, :3] = BACKGROUND
    img[..., 3] = 201
    return img


# ------------------------------------------------------------------------------------------------ shared scenes (read-only)
class ColorScene:
    """A small sphere-over-plane scene: `frames` depth frames from `frames` poses, the oracle's TSDF after each (rigid integrate), the
    checker paint of each frame."""

    def __init__(self, dims, cols, rows, frames=3, size=1.0, nodes=0, k=4):
        from dynamicfusion_amd import synth
        from scene import Scene
        self.cfg = synth.Config(dims, size, cols=cols, rows=rows, nodes=nodes, k=k)
        self.sc = sc = Scene(self.cfg, n_frames=frames, with_nodes=nodes > 0)
        # poses a few degrees apart (the synthetic camera turns 0.25 degrees a frame: the three frames would see the same voxels)
        centre = (0.0, 0.0, 0.5 + self.cfg.size / 2)
        sc.cam_poses = [synth.rot_y_about(np.deg2rad(4.0 * f), centre) for f in range(frames)]
        sc.depths = [depth_from_pose(self.cfg, p, f) for f, p in enumerate(sc.cam_poses)]
        sc.dists = [O.compute_dists(d, sc.intr) for d in sc.depths]
        self.vols = []
        vol = sc.new_volume()
        for f in range(frames):
            O.integrate(sc.dists[f], vol, sc.ovol(vol), synth.aff12(sc.vol2cam(f)), sc.intr)
            self.vols.append(vol.copy())
        self.images = [paint_checker(sc.depths[f], sc.cam_poses[f], self.cfg.intr) for f in range(frames)]
        self.vol2world = synth.aff12(sc.pose)
        self.world2vol = synth.aff12(np.linalg.inv(sc.pose.astype(np.float64)).astype(F32))

    def world2cam(self, f):
        from dynamicfusion_amd import synth
        return synth.aff12(self.sc.world2cam(f))


def depth_from_pose(cfg, pose, frame):
    """synth.depth_frame for an arbitrary camera pose (same scene, same 2 % holes)."""
    from dynamicfusion_amd import synth
    t, _ = synth._hit_points(cfg, pose)
    valid = np.isfinite(t) & (t >= 0.4) & (t <= 0.5 + cfg.size)
    mm = np.clip(np.where(valid, np.rint(np.where(valid, t, 0.0) * 1000.0), 0.0), 0, 65535).astype(np.uint16)
    rng = np.random.RandomState(1 + 7919 * frame)
    mm[rng.random_sample(mm.shape) < 0.02] = 0
    return mm


@functools.lru_cache(None)
def scene(dims, cols, rows, nodes=0, k=4):
    return ColorScene(dims, cols, rows, nodes=nodes, k=k)
