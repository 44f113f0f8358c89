"""numpy restatement of dfusion_associate_projective (include/dfusion.h): the ONLY expected value of the association
tests.  f32 throughout, the fused multiply-adds exact through mesh_ref.fma32, dot3 in its fused order
fmaf(a.x, b.x, fmaf(a.y, b.y, a.z * b.z)).  Also the planted sphere scene the rule and the GPU tests share.
"""
import numpy as np

from mesh_ref import fma32

F32 = np.float32
QNAN_BITS = np.uint32(0x7FFFFFFF)
STATUS = ("paired", "invalid", "behind", "outside", "occluded", "hole", "far", "normal")


def dot3(a, b):
    """dfusion_device.h dot3 on [n, 3] f32 arrays."""
    with np.errstate(all="ignore"):
        return fma32(a[:, 0], b[:, 0], fma32(a[:, 1], b[:, 1], a[:, 2] * b[:, 2]))


def project(points, cols, rows, intr):
    """Tests 1 (points only) to 3.  Returns (status [N] with 0 = on a pixel, ui, vi); ui, vi are 0 where status != 0."""
    p = np.ascontiguousarray(points, F32).reshape(-1, 3)
    fx, fy, cx, cy = (F32(v) for v in intr)
    n = len(p)
    st = np.zeros(n, np.uint8)
    st[~np.isfinite(p).all(1)] = 1
    with np.errstate(all="ignore"):
        st[(st == 0) & ~(p[:, 2] > 0)] = 2
        ok = st == 0
        z = np.where(ok, p[:, 2], F32(1))
        x, y = np.where(ok, p[:, 0], F32(0)), np.where(ok, p[:, 1], F32(0))
        u = fma32(np.full(n, fx, F32), (x / z).astype(F32), np.full(n, cx, F32))
        v = fma32(np.full(n, fy, F32), (y / z).astype(F32), np.full(n, cy, F32))
        inside = (u >= 0) & (v >= 0) & (u < F32(cols)) & (v < F32(rows))
    st[ok & ~inside] = 3
    on = st == 0
    ui = np.where(on, u, 0).astype(np.int32)
    vi = np.where(on, v, 0).astype(np.int32)
    return st, ui, vi


def associate(points, normals, live_points, live_normals, intr, dist_thres, min_cosine, occlusion_margin=-1.0):
    """points / normals [N, 3] (normals None together with live_normals), live_points / live_normals [rows, cols, >= 3] f32.
    Returns (live [N, 3] f32 -- rejected rows are 0x7fffffff words --, status uint8 [N], counts uint64 [8])."""
    if (normals is None) != (live_normals is None):
        raise ValueError("normals and live_normals go together")
    p = np.ascontiguousarray(points, F32).reshape(-1, 3)
    rows, cols = live_points.shape[:2]
    st, ui, vi = project(p, cols, rows, intr)
    if normals is not None:
        nr = np.ascontiguousarray(normals, F32).reshape(-1, 3)
        bad = ~np.isfinite(nr).all(1)
        st[bad] = 1                                      # test 1 comes first, whatever tests 2 and 3 said
        ui[bad] = 0; vi[bad] = 0
    margin = F32(occlusion_margin)
    with np.errstate(all="ignore"):
        if margin >= 0:
            on = st == 0
            zmin = np.full(rows * cols, np.inf, F32)
            pix = vi.astype(np.int64) * cols + ui
            np.minimum.at(zmin, pix[on], p[on, 2])
            occ = on & ((p[:, 2] - zmin[pix]).astype(F32) > margin)
            st[occ] = 4
        q = np.ascontiguousarray(live_points[vi, ui, :3], F32)
        on = st == 0
        st[on & np.isnan(q[:, 0])] = 5
        on = st == 0
        d = (p - q).astype(F32)
        d[~on] = 0
        thr2 = F32(dist_thres) * F32(dist_thres)
        st[on & (dot3(d, d) > thr2)] = 6
        if normals is not None:
            on = st == 0
            nl = np.ascontiguousarray(live_normals[vi, ui, :3], F32)
            a = np.where(on[:, None], nr, F32(0))
            c = np.abs(dot3(a, nl))
            st[on & ~(c >= F32(min_cosine))] = 7
    live = np.empty((len(p), 3), np.uint32)
    live[:] = QNAN_BITS
    on = st == 0
    live[on] = q[on].view(np.uint32)
    counts = np.bincount(st, minlength=8).astype(np.uint64)
    return live.view(F32), st, counts


def index_pairs(points, live_points):
    """The pairing the loop uses without association: point i with live pixel i (row-major)."""
    return np.ascontiguousarray(live_points[..., :3], F32).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------ the planted sphere
COLS, ROWS = 160, 120
INTR = tuple(F32(v * 0.25) for v in (570.342, 570.342, 320.0, 240.0))      # synth.Config at 160 x 120
CENTRE, RADIUS = np.array([0.0, 0.0, 1.0]), 0.2
DT = np.array([0.004, 0.002, -0.003])
DIST_THRES, MIN_COSINE = 0.05, float(F32(np.cos(np.deg2rad(30.0))))


def _cast_sphere(centre):
    """Ray-cast a sphere through every pixel centre (f64): (points [rows, cols, 3], normals), NaN where the ray misses."""
    fx, fy, cx, cy = (float(v) for v in INTR)
    u, v = np.meshgrid(np.arange(COLS, dtype=np.float64), np.arange(ROWS, dtype=np.float64))
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    a = (d * d).sum(-1)
    b = (d * centre).sum(-1)
    disc = b * b - a * ((centre * centre).sum() - RADIUS * RADIUS)
    with np.errstate(invalid="ignore"):
        t = (b - np.sqrt(disc)) / a
    pts = d * t[..., None]
    pts[~(disc > 0)] = np.nan
    return pts, (pts - centre) / RADIUS


def planted(t0):
    """The planted scene: model points canonical + t0 (numpy, not through warp) with the canonical sphere's normals, and the live maps of
    the sphere moved by t0 + DT, its depth rounded to millimetres and re-projected.  Returns a dict: points, normals [N, 3] f32 (N =
    19 200, NaN rows where the canonical ray misses), live_points, live_normals [rows, cols, 4] f32, truth [N, 3] = points + DT."""
    t0 = np.asarray(t0, np.float64)
    canon, cn = _cast_sphere(CENTRE)
    model = canon + t0
    lp, ln = _cast_sphere(CENTRE + t0 + DT)
    fx, fy, cx, cy = (float(v) for v in INTR)
    u, v = np.meshgrid(np.arange(COLS, dtype=np.float64), np.arange(ROWS, dtype=np.float64))
    z = np.rint(lp[..., 2] * 1000.0) / 1000.0
    lp = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], -1)
    live_points = np.zeros((ROWS, COLS, 4), F32); live_normals = np.zeros((ROWS, COLS, 4), F32)
    live_points[..., :3] = lp; live_normals[..., :3] = ln
    hole = np.isnan(live_points[..., 0])
    live_points[hole] = np.nan; live_normals[hole] = np.nan
    pts = model.reshape(-1, 3).astype(F32)
    return dict(points=pts, normals=cn.reshape(-1, 3).astype(F32), live_points=live_points, live_normals=live_normals,
                truth=(model + DT).reshape(-1, 3))


def pair_error_mm(live, truth):
    """|paired live - truth| in millimetres over the rows where both are finite."""
    ok = np.isfinite(live).all(1) & np.isfinite(truth).all(1)
    return np.linalg.norm(live[ok].astype(np.float64) - truth[ok], axis=1) * 1000.0
