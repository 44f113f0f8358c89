"""numpy restatement of the rule of dfusion_mesh_ray_hits (include/dfusion.h): which triangles are eligible and which rays valid,
Moeller-Trumbore with every f32 operation in the stated order, the slab test of the triangle's own grown vertex box with its explicit
parallel-axis case, the clamp of t into that box, and the winner by brute force over ALL eligible triangles -- no tree, no pruning.
Nothing taken from the HIP source.  Beside it the inputs that the rule test and the GPU tests share."""
import functools

import numpy as np

import mesh_closest_ref as M

F32 = np.float32
NONE = M.NONE
NAN_BITS = M.NAN_BITS
INF = F32(np.inf)
ONE, ZERO = F32(1), F32(0)
positions, soup, eligible = M.positions, M.soup, M.eligible


def fmax(a, b):
    """The rule's max: a NaN operand is dropped; of two equal operands (zeros of either sign included) the second is returned."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(b) | (a > b), a, b)


def fmin(a, b):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(b) | (a < b), a, b)


def dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def valid_rays(origins, directions):
    """bool [R]: six finite numbers and a direction that is not (+-0, +-0, +-0)."""
    o, d = M._v4(origins)[:, :3], M._v4(directions)[:, :3]
    return np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1)


def slab(lo, hi, o, d, slack, t_min, t_max):
    """The slab test of boxes [lo, hi] ([..., 3]) grown by slack ([...]) against rays o, d ([..., 3]) and [t_min, t_max]
    -> (passes bool [...], tn, tf f32 [...]).  An axis whose 1 / d_k is infinite is parallel: an interval test, no constraint on t."""
    t_min, t_max = F32(t_min), F32(t_max)
    with np.errstate(all="ignore"):
        inv = ONE / d
        par = np.isinf(inv)
        glo, ghi = lo - slack[..., None], hi + slack[..., None]
        a, b = (glo - o) * inv, (ghi - o) * inv
        near, far = fmin(a, b), fmax(a, b)
        ok = (~par | ((glo <= o) & (o <= ghi))).all(-1)
        tn = np.full(ok.shape, -INF, F32)
        tf = np.full(ok.shape, INF, F32)
        for k in range(3):
            tn = np.where(par[..., k], tn, fmax(tn, near[..., k]))
            tf = np.where(par[..., k], tf, fmin(tf, far[..., k]))
        tn = fmax(tn, t_min)
        tf = fmin(tf, t_max)
        ok = ok & (tn <= tf)
    assert tn.dtype == F32 and tf.dtype == F32
    return ok, tn, tf


def moller_trumbore(o, d, a, b, c):
    """o, d, a, b, c: f32 [..., 3] that broadcast -> (det, u, v, t), every operation one f32 operation."""
    with np.errstate(all="ignore"):
        e1x, e1y, e1z = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1], b[..., 2] - a[..., 2]
        e2x, e2y, e2z = c[..., 0] - a[..., 0], c[..., 1] - a[..., 1], c[..., 2] - a[..., 2]
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        px, py, pz = dy * e2z - dz * e2y, dz * e2x - dx * e2z, dx * e2y - dy * e2x
        det = dot(e1x, e1y, e1z, px, py, pz)
        inv = ONE / det
        sx, sy, sz = o[..., 0] - a[..., 0], o[..., 1] - a[..., 1], o[..., 2] - a[..., 2]
        u = dot(sx, sy, sz, px, py, pz) * inv
        qx, qy, qz = sy * e1z - sz * e1y, sz * e1x - sx * e1z, sx * e1y - sy * e1x
        v = dot(dx, dy, dz, qx, qy, qz) * inv
        t = dot(e2x, e2y, e2z, qx, qy, qz) * inv
    assert t.dtype == F32 and u.dtype == F32 and det.dtype == F32
    return det, u, v, t


def candidates(det, u, v, t, t_min, t_max):
    with np.errstate(invalid="ignore"):
        return (det != 0) & (u >= 0) & (v >= 0) & (u + v <= ONE) & (t >= F32(t_min)) & (t <= F32(t_max))


def ray_slack(root_m, o):
    """slack = m 2^-18 + 2^-126, m the largest |coordinate| of the eligible triangles (root_m) and of o [..., 3]."""
    m = np.maximum(F32(root_m), np.abs(o).max(-1))
    return m * F32(2.0 ** -18) + F32(2.0 ** -126)


class Hits:
    pass


def ray_hits(vertices, triangles, origins, directions, t_min=0.0, t_max=np.inf, chunk=1 << 20, grow=True, clamp=True):
    """-> Hits: triangle uint32 [R], hit f32 [R, 4] (x, y, z, t_hit), bary f32 [R, 4] (1 - u - v, u, v, side), any bool [R] (some
    candidate is accepted), counts uint64 [6] (the first six of the call's eight), bound int (accepted candidates whose t the clamp
    changed), lost int (candidates whose own box fails).  grow=False, clamp=False: the rule without its slack / its clamp, for the tests
    that show what each is for."""
    v, tr, o4, d4 = M._v4(vertices), M._tri(triangles), M._v4(origins), M._v4(directions)
    t_min, t_max = F32(t_min), F32(t_max)
    ids = np.where(eligible(v, tr))[0]
    E, R = len(ids), len(o4)
    ok_ray = valid_rays(o4, d4)
    out = Hits()
    out.triangle = np.full(R, NONE, np.uint32)
    out.hit = np.empty((R, 4), F32)
    out.hit.view(np.uint32)[:, :3] = NAN_BITS
    out.hit[:, 3] = INF
    out.bary = np.zeros((R, 4), F32)
    out.any = np.zeros(R, bool)
    out.bound = out.lost = 0
    rays = np.where(ok_ray)[0]
    if E and len(rays):
        a, b, c = (v[tr[ids, k]][None, :, :3] for k in range(3))
        lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
        root_m = max(np.abs(lo).max(), np.abs(hi).max())
        step = max(1, chunk // E)
        for r0 in range(0, len(rays), step):
            ri = rays[r0:r0 + step]
            o, d = o4[ri, None, :3], d4[ri, None, :3]
            det, u, vv, t = moller_trumbore(o, d, a, b, c)               # [r, E]
            cand = candidates(det, u, vv, t, t_min, t_max)
            slack = ray_slack(root_m, o) if grow else np.zeros((len(ri), 1), F32)
            passes, tn, tf = slab(lo, hi, o, d, np.broadcast_to(slack, (len(ri), E)), t_min, t_max)
            acc = cand & passes
            t_hit = fmin(fmax(t, tn), tf) if clamp else t
            out.lost += int((cand & ~passes).sum())
            out.bound += int((acc & (t_hit != t)).sum())
            with np.errstate(invalid="ignore"):
                best = np.where(acc, t_hit, INF).min(1)
                first = (acc & (t_hit == best[:, None])).argmax(1)       # ties: the smaller index (ids ascend)
            won = acc.any(1)
            rows = np.arange(len(won))[won]
            k = first[won]
            qi = ri[won]
            th = t_hit[rows, k]
            out.any[qi] = True
            out.triangle[qi] = ids[k]
            with np.errstate(all="ignore"):
                out.hit[qi, :3] = o4[qi, :3] + d4[qi, :3] * th[:, None]
            out.hit[qi, 3] = th
            uu, v2 = u[rows, k], vv[rows, k]
            out.bary[qi, 0] = (ONE - uu) - v2
            out.bary[qi, 1] = uu
            out.bary[qi, 2] = v2
            out.bary[qi, 3] = np.where(det[rows, k] > 0, ONE, -ONE)
    n = int(out.any.sum())
    out.counts = np.array([n, R - n, E, len(tr) - E, R - len(rays), 0], np.uint64)
    return out


def visible_points(vertices, triangles, points, eye, margin=2.0 ** -10):
    """bool [N]: the segment eye -> p, on [0, 1 - margin] of d = p - eye, meets no accepted candidate, and p is finite."""
    p = M._v4(points)
    o = np.zeros_like(p)
    o[:, :3] = np.asarray(eye, F32)
    with np.errstate(invalid="ignore"):
        d = p - o
    res = ray_hits(vertices, triangles, o, d, 0.0, ONE - F32(margin))
    return ~res.any & np.isfinite(p[:, :3]).all(1)


# ------------------------------------------------------------------------------------------------ shared inputs
def cube_rays(n, seed, offset=0.0, scale=1.0):
    """Origins in the unit cube, directions uniform in [-0.5, 0.5]^3 (never normalised); both translated / scaled with the mesh."""
    rng = np.random.default_rng(seed)
    o = (rng.random((n, 3)).astype(F32) + F32(offset)) * F32(scale)
    d = (rng.random((n, 3)) - 0.5).astype(F32) * F32(scale)
    return positions(o), positions(d)


def aimed_rays(vertices, triangles, n, seed):
    """n rays: the even ones from origins in the unit cube towards a point inside one of the given (eligible) triangles, d = (target - o)
    times 0.5 .. 2 (so that t is 0.5 .. 2 there); the odd ones cube_rays'.  -> origins, directions."""
    v, t = M._v4(vertices), M._tri(triangles)
    o, d = cube_rays(n, seed)
    if len(t):
        rng = np.random.default_rng(seed + 1000)
        m = len(o[::2])
        k = rng.integers(0, len(t), m)
        u = rng.random((m, 1)) * 0.8 + 0.1
        w = rng.random((m, 1)) * (0.9 - u)
        a, b, c = (v[t[k, i]][:, :3].astype(np.float64) for i in range(3))
        target = a + (b - a) * u + (c - a) * w
        d[::2, :3] = ((target - o[::2, :3]) * rng.uniform(0.5, 2, (m, 1))).astype(F32)
    return o, d


@functools.lru_cache(maxsize=None)
def slivers(n_tri, rays_per, seed):
    """n_tri long slivers -- A in [0, 4]^3, B within 0.02 of A, C about 1000 away -- and rays_per rays for each, aimed at a point
    of its face from 1 .. 40 units away at 1 .. 5 degrees off its plane, along the long edge.  -> vertices, triangles, origins,
    directions."""
    rng = np.random.default_rng(seed)
    a = rng.random((n_tri, 3)) * 4
    b = a + (rng.random((n_tri, 3)) - 0.5) * 0.04
    long_dir = rng.normal(size=(n_tri, 3))
    long_dir /= np.linalg.norm(long_dir, axis=1, keepdims=True)
    c = a + long_dir * (1000 + rng.random((n_tri, 1)) * 50)
    tri = np.stack([a, b, c], 1)
    roll = rng.integers(0, 3, n_tri)                                     # which corner is the rule's A: with the far one s = o - A is long
    tri = np.stack([np.roll(tri[i], roll[i], 0) for i in range(n_tri)])
    v = positions(tri.reshape(-1, 3).astype(F32))
    t = np.arange(3 * n_tri, dtype=np.uint32).reshape(-1, 3)
    normal = np.cross(b - a, c - a)
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    k = np.repeat(np.arange(n_tri), rays_per)
    uu = rng.random(len(k)) * 0.9
    vv = rng.random(len(k)) * (0.9 - uu) * 0.05                          # near the short end, where the sliver is wide enough to be hit
    target = a[k] + (b - a)[k] * uu[:, None] + (c - a)[k] * vv[:, None]
    theta = np.radians(rng.uniform(1, 5, len(k))) * rng.choice([-1, 1], len(k))
    d = long_dir[k] * np.cos(theta)[:, None] + normal[k] * np.sin(theta)[:, None]
    o = target - d * rng.uniform(1, 40, (len(k), 1))
    return v, t, positions(o.astype(F32)), positions(d.astype(F32))


@functools.lru_cache(maxsize=None)
def grid_plane(n=9):
    """The n x n vertex grid plane z = 0 over [0, n - 1]^2 (2 (n - 1)^2 triangles) -> vertices, triangles."""
    g = np.arange(n, dtype=F32)
    x, y = np.meshgrid(g, g, indexing="xy")
    v = positions(np.stack([x.ravel(), y.ravel(), np.zeros(n * n, F32)], 1))
    i = (np.arange(n - 1)[:, None] * n + np.arange(n - 1)[None, :]).ravel().astype(np.uint32)
    return v, np.concatenate([np.stack([i, i + 1, i + n], 1), np.stack([i + 1, i + n + 1, i + n], 1)])


@functools.lru_cache(maxsize=None)
def grid_rays(n=9):
    """Against grid_plane: the n^2 rays (x, y, 3) -> -z through its vertices, the same from below, rays IN the plane z = 0 along +x,
    -y and a diagonal (every box of the plane is flat in z and contains o.z: the parallel case), and rays from three eyes above the
    plane towards every vertex (d = vertex - eye, so the hit lies on the faces of up to six boxes, as exactly as f32 lets it).
    -> origins, directions, the number of axis-parallel rays through vertices (the first ones)."""
    g = np.arange(n, dtype=F32)
    x, y = (c.ravel() for c in np.meshgrid(g, g, indexing="xy"))
    z = np.zeros_like(x)
    o = [np.stack([x, y, z + 3], 1), np.stack([x, y, z - 2], 1), np.stack([z - 1, y + 0.5, z], 1), np.stack([x + 0.25, z + n, z], 1),
         np.stack([x - 3, y - 3, z], 1)]
    d = [np.stack([z, z, z - 1], 1), np.stack([z, -z, z + 2], 1), np.stack([z + 1, z, z], 1), np.stack([z, z - 1, -z], 1),
         np.stack([z + 1, z + 1, z], 1)]
    for eye in ([3.3, 4.1, 7.7], [-2.6, 9.3, 1.9], [11.2, 0.7, 0.3]):
        e = np.broadcast_to(F32(eye), (n * n, 3))
        o.append(e)
        d.append(np.stack([x, y, z], 1) - e)
    return positions(np.concatenate(o)), positions(np.concatenate(d)), 2 * n * n


@functools.lru_cache(maxsize=None)
def wall_and_far():
    """One large wall in the plane x = 0.5 (centroid inside [0, 1]^3) in front of the 64 far triangles of mesh_closest_ref.two_clusters
    (inside [7, 8] x [0, 1]^2), and 200 rays from x = -1 towards points of the far triangles' box: every one goes through the wall first.
    -> vertices, triangles (0: the wall), origins, directions."""
    cv, ct, _ = M.two_clusters()
    far = cv[ct[64:]][:, :, :3].reshape(-1, 3)
    wall = np.array([[0.5, -40, -40], [0.5, 41.5, -40], [0.5, 0, 81.5]], F32)
    v = positions(np.concatenate([wall, far]))
    t = np.arange(len(v), dtype=np.uint32).reshape(-1, 3)
    rng = np.random.default_rng(23)
    o = np.concatenate([np.full((200, 1), -1.0), rng.random((200, 2))], 1).astype(F32)
    target = (far.min(0) + rng.random((200, 3)) * (far.max(0) - far.min(0))).astype(F32)      # inside the far triangles' own box
    return v, t, positions(o), positions(target - o)


@functools.lru_cache(maxsize=None)
def two_clusters_rays():
    """mesh_closest_ref.two_clusters (64 triangles in [0, 1]^3, 64 in [7, 8] x [0, 1]^2) and 300 rays from x = -1 along +x that hit a
    triangle of the near cluster (chosen by this restatement among 4000 drawn).  -> vertices, triangles, origins, directions."""
    v, t, _ = M.two_clusters()
    rng = np.random.default_rng(24)
    o = np.concatenate([np.full((4000, 1), -1.0), 0.1 + 0.8 * rng.random((4000, 2))], 1).astype(F32)
    d = np.concatenate([np.ones((4000, 1)), (rng.random((4000, 2)) - 0.5) * 0.05], 1).astype(F32)
    res = ray_hits(v, t, positions(o), positions(d))
    keep = np.where(res.any & (res.triangle < 64))[0][:300]
    assert len(keep) == 300
    return v, t, positions(o[keep]), positions(d[keep])


@functools.lru_cache(maxsize=None)
def grown_face_rays():
    """The triangle (0, 0, 0), (1, 0, 0), (0, 1, 0) and 64 rays along -z whose o.x lies EXACTLY on a face of its grown box: m = 1 gives
    slack = 2^-18, so the faces are x = -2^-18 (even rays) and x = 1 + 2^-18 (odd rays; there m = 1 + 2^-18, slack = 2^-18 + 2^-36 and
    1 + slack rounds to 1 + 2^-18 again).  x is a parallel axis for them; the rule passes the box, and no ray meets the triangle.
    -> vertices, triangles, origins, directions."""
    v = positions([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    y = np.linspace(0.0, 0.9, 64)
    x = np.where(np.arange(64) % 2 == 0, -2.0 ** -18, 1 + 2.0 ** -18)
    o = positions(np.stack([x, y, np.ones(64)], 1))
    return v, np.array([[0, 1, 2]], np.uint32), o, positions(np.tile([0.0, -0.0, -1.0], (64, 1)))
