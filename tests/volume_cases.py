"""Volumes that the three per-frame readers of the fused volume -- dfusion_extract_cloud, dfusion_extract_normals and the ray-cast --
never get from `integrate` over a smooth scene, and a numpy restatement of how many crossings each wave-item of the extractor's scan
holds.  The generators are tests/mesh_ref.py's (noise_volume, checker_volume) plus five crafted ones; tests/test_volume_readers_rule.py
shows, with the oracle alone, which branch of the kernels each of them reaches.  All volumes are uint32
[Z, Y, X]: lo16 = half tsdf bits, hi16 = weight."""
import functools

import numpy as np

import mesh_ref as R
import oracle_lib as O
from dynamicfusion_amd import synth
from scene import Scene

F32 = np.float32
P = np.uint32((1 << 16) | 0x3800)          # weight 1, tsdf +0.5
N = np.uint32((1 << 16) | 0xb800)          # weight 1, tsdf -0.5
CLEARED = np.uint32(0x3c00)                # weight 0, tsdf +1.0: free space no frame has touched

# ---- the extractor's constants, named after dynamicfusion_amd/csrc/dfusion_raycast.hip
ITEM_VOXELS = 256           # a wave-item: 64 lanes x 4 x-adjacent voxels, consecutive in address order
ITEMS_PER_WORKGROUP = 16    # phase 1: 4 waves x U = 4 items per trip (one trip at these sizes: the grid has a workgroup per 1024 voxels)
ITEMS_PER_ROUND = 4         # phase 2: one listed item per wave and round
DF_EX_CAP = 1024            # points a workgroup buffers in LDS; a round with more goes straight to global memory (`direct`)

CRAFTED_DIMS = (256, 8, 9)  # a row is one wave-item; planes [0, 8) are scanned: 64 items, 4 workgroups, four rounds each
NOISE_DIMS, BIG_DIMS = (64, 48, 44), (128, 96, 86)


# ------------------------------------------------------------------------------------------------ crafted volumes
def z_parity(dims):
    """N on odd z, P on even z: every scanned voxel has exactly one crossing (its +z edge)."""
    X, Y, Z = dims
    vol = np.empty((Z, Y, X), np.uint32)
    vol[0::2], vol[1::2] = P, N
    return vol


def z_parity_split(dims):
    """z_parity with the sign flipped where (x >> 7) & 1: one more crossing per row, on the x edge 127|128."""
    vol = z_parity(dims)
    flip = ((np.arange(dims[0]) >> 7) & 1).astype(bool)
    vol[:, :, flip] ^= np.uint32(0x8000)
    return vol


def z_parity_even_x(dims):
    """z_parity with weight 0 on odd x: half the crossings, none along x."""
    vol = z_parity(dims)
    vol[:, :, 1::2] &= np.uint32(0xffff)
    return vol


ONE_PAST_ROWS, ONE_PAST_VOXELS = 5, 206


def one_past(dims):
    """P on even x, N on odd x, in the first ONE_PAST_VOXELS voxels of rows y < ONE_PAST_ROWS of the even planes; weight 0 elsewhere.  A
    listed row holds its 205 x crossings and nothing else (rows beside and planes above it are equal or invalid).  At CRAFTED_DIMS a
    workgroup (two planes) lists five such rows: a round of four buffers 820 points, the fifth item makes it 1025 -- one past the buffer."""
    X, Y, Z = dims
    vol = np.zeros((Z, Y, X), np.uint32)
    vol[0:Z - 1:2, :ONE_PAST_ROWS, 0:ONE_PAST_VOXELS:2] = P
    vol[0:Z - 1:2, :ONE_PAST_ROWS, 1:ONE_PAST_VOXELS:2] = N
    return vol


def back_wall(dims, seed, planes=6, p_invalid=0.1):
    """A cleared volume (tsdf +1.0, weight 0) whose last `planes` z-planes hold noise_volume values: rays march dozens of windows of
    free space, then meet events at every window slot, or leave without one."""
    X, Y, Z = dims
    vol = np.full((Z, Y, X), CLEARED, np.uint32)
    vol[Z - planes:] = R.noise_volume((X, Y, planes), seed, p_invalid)
    return vol


BACK_WALL_SEED = 41


@functools.lru_cache(None)
def case(name, dims=None):
    """A named volume, built once per process and shared (do not modify).  'noise_<p>': noise_volume at p_invalid = p, seed 7; the
    crafted ones default to CRAFTED_DIMS, noise and the back wall to NOISE_DIMS."""
    if name.startswith("noise_"):
        vol = R.noise_volume(dims or NOISE_DIMS, 7, float(name[6:]))
    elif name == "back_wall":
        vol = back_wall(dims or NOISE_DIMS, BACK_WALL_SEED)
    else:
        vol = {"z_parity": z_parity, "z_parity_split": z_parity_split, "z_parity_even_x": z_parity_even_x, "one_past": one_past,
               "checker": R.checker_volume}[name](dims or CRAFTED_DIMS)
    return np.ascontiguousarray(vol, np.uint32)


# ------------------------------------------------------------------------------------------------ the crossing count, restated
def crossings_per_voxel(vol):
    """-> int64 [Z - 1, Y, X]: how many of a scanned voxel's +x, +y, +z edges carry a crossing.  A voxel counts when its weight is not
    0 and its tsdf is not 1.0; an edge carries a crossing when both ends count and one tsdf is > 0, the other < 0 (+0 and -0 are neither)."""
    half = (vol & 0xffff).astype(np.uint16)
    f = half.view(np.float16).astype(F32)
    valid = ((vol >> 16) != 0) & (half != 0x3c00)
    pos, neg = valid & (f > 0), valid & (f < 0)
    Z = vol.shape[0]
    n = np.zeros((Z - 1,) + vol.shape[1:], np.int64)
    n += (pos[:-1] & neg[1:]) | (neg[:-1] & pos[1:])
    n[:, :-1] += (pos[:-1, :-1] & neg[:-1, 1:]) | (neg[:-1, :-1] & pos[:-1, 1:])
    n[:, :, :-1] += (pos[:-1, :, :-1] & neg[:-1, :, 1:]) | (neg[:-1, :, :-1] & pos[:-1, :, 1:])
    return n, valid[:-1]


def item_counts(vol):
    """-> (crossings of every wave-item int64 [n_items], listed bool [n_items]): a wave-item is ITEM_VOXELS consecutive voxels of the
    planes [0, Z - 1) in address order (the last one may be short); it is listed when any of its voxels counts."""
    n, valid = crossings_per_voxel(vol)
    pad = -n.size % ITEM_VOXELS
    per = np.concatenate([n.reshape(-1), np.zeros(pad, np.int64)]).reshape(-1, ITEM_VOXELS).sum(1)
    listed = np.concatenate([valid.reshape(-1), np.zeros(pad, bool)]).reshape(-1, ITEM_VOXELS).any(1)
    return per, listed


def round_sum_bounds(vol):
    """Per workgroup (ITEMS_PER_WORKGROUP consecutive items) with at least ITEMS_PER_ROUND listed items: (smallest, largest) sum that
    ITEMS_PER_ROUND of its listed items can have -- the workgroup's list is in scheduling order, so a round may hold any four of them.
    -> int64 [n_workgroups, 3]: listed items, smallest, largest."""
    per, listed = item_counts(vol)
    out = []
    for g in range(0, len(per), ITEMS_PER_WORKGROUP):
        c = np.sort(per[g:g + ITEMS_PER_WORKGROUP][listed[g:g + ITEMS_PER_WORKGROUP]])
        if len(c) >= ITEMS_PER_ROUND:
            out.append((len(c), c[:ITEMS_PER_ROUND].sum(), c[-ITEMS_PER_ROUND:].sum()))
    return np.array(out, np.int64).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------ the oracle's answers
def ovolume(vol, dims, vs=R.VS, trunc=0.03, max_weight=128):
    return O.make_volume(vol, dims, np.array(vs, F32), trunc, max_weight)


def sort_rows(a):
    """Rows of a [n, 4] array in the lexicographic order of their uint32 bits."""
    a = np.ascontiguousarray(a).view(np.uint32).reshape(-1, 4)
    return a[np.lexsort(a.T[::-1])]


def oracle_cloud(vol, dims, aff12=R.POSE, vs=R.VS, slab=None):
    """-> (sorted rows uint32 [n, 4], n) of O.extract_cloud; `vol` holds the stored planes of `slab` = (z_store0, z_store_n, z_own0, z_own_n)."""
    cap = 3 * int(np.prod(vol.shape)) + 1
    pts, n = O.extract_cloud(ovolume(vol, dims, vs), aff12, cap, slab=O.make_slab(*slab) if slab else None)
    assert n == len(pts)
    return sort_rows(pts), n


@functools.lru_cache(None)
def named_cloud(name, dims=None):
    """oracle_cloud of case(name, dims) at mesh_ref.POSE and VS; shared (do not modify)."""
    return oracle_cloud(case(name, dims), dims or (NOISE_DIMS if name.startswith("noise_") or name == "back_wall" else CRAFTED_DIMS))


# ------------------------------------------------------------------------------------------------ the ray-cast's scene
@functools.lru_cache(None)
def ray_scene(dims=NOISE_DIMS, cols=160, rows=120):
    """The camera and volume geometry of the ray-cast cases: a 1 m volume of `dims` voxels in front of synth's camera."""
    return Scene(synth.Config(dims, 1.0, cols=cols, rows=rows, nodes=0, k=4), n_frames=2, with_nodes=False)


def oracle_cast(sc, vol, cam_pose, cols=None, rows=None, reproj=None, vs=None):
    """O.raycast_points with keys from the 4x4 camera pose -> (points, normals, keys)."""
    cfg = sc.cfg
    cam2vol = synth.affine_mul(synth.affine_inv(sc.pose), np.asarray(cam_pose, F32))
    rinv = np.linalg.inv(cam2vol[:3, :3].astype(np.float64)).astype(F32)
    ov = sc.ovol(vol) if vs is None else O.make_volume(vol, cfg.dims, np.array(vs, F32), sc.trunc, cfg.max_weight)
    p, n, k, _ = O.raycast_points(ov, synth.aff12(cam2vol), rinv, sc.reproj if reproj is None else reproj, cols or cfg.cols,
                                  rows or cfg.rows, cfg.raycast_step_factor, cfg.gradient_delta_factor, want_keys=True)
    return p, n, k


NO_EVENT = np.uint32(0xffffffff)
DF_RC_WINDOW = 4            # speculative samples per trip of the march


def event_classes(keys):
    """keys uint32 [rows, cols] -> int64 [DF_RC_WINDOW, 2]: pixels whose first event falls on window slot (step mod 4), by kind
    (0 = back-face break, 1 = hit)."""
    k = keys[keys != NO_EVENT].astype(np.int64)
    out = np.zeros((DF_RC_WINDOW, 2), np.int64)
    np.add.at(out, ((k >> 1) % DF_RC_WINDOW, k & 1), 1)
    return out
