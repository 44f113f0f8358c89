"""numpy restatement of the rule of dfusion_mesh_closest_points (include/dfusion.h): which triangles are eligible, Ericson's
Voronoi-region routine with every f32 operation in the stated order, and the winner by brute force over ALL eligible triangles -- no
tree, no pruning.  Nothing taken from the HIP source.  Beside it the 62-bit sort keys (Morton code << 32 | index) with the depth of the
radix tree over them, and the inputs that the rule test and the GPU test share."""
import functools

import numpy as np

F32 = np.float32
NONE = 0xffffffff
NAN_BITS = 0x7fc00000
INF = F32(np.inf)
REGIONS = ("vertex A", "vertex B", "edge AB", "vertex C", "edge AC", "edge BC", "face")
ONE, ZERO = F32(1), F32(0)


def _v4(v):
    return np.ascontiguousarray(v, F32).reshape(-1, 4)


def _tri(t):
    return np.ascontiguousarray(t, np.uint32).reshape(-1, 3)


def eligible(vertices, triangles):
    """bool [T]: three indices < V (tested before anything is indexed), pairwise different, nine finite coordinates."""
    v, t = _v4(vertices), _tri(triangles)
    ok = (t < len(v)).all(1)
    ok &= (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    idx = np.where(ok)[0]
    ok[idx] = np.isfinite(v[t[idx]][:, :, :3]).all((1, 2))
    return ok


def dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def routine(p, a, b, c):
    """p, a, b, c: f32 arrays [..., 3] that broadcast -> (region 0 .. 6, v, w, point [..., 3], d2), every operation one f32 operation."""
    with np.errstate(all="ignore"):
        px, py, pz = p[..., 0], p[..., 1], p[..., 2]
        abx, aby, abz = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1], b[..., 2] - a[..., 2]
        acx, acy, acz = c[..., 0] - a[..., 0], c[..., 1] - a[..., 1], c[..., 2] - a[..., 2]
        apx, apy, apz = px - a[..., 0], py - a[..., 1], pz - a[..., 2]
        d1, d2 = dot(abx, aby, abz, apx, apy, apz), dot(acx, acy, acz, apx, apy, apz)
        bpx, bpy, bpz = px - b[..., 0], py - b[..., 1], pz - b[..., 2]
        d3, d4 = dot(abx, aby, abz, bpx, bpy, bpz), dot(acx, acy, acz, bpx, bpy, bpz)
        cpx, cpy, cpz = px - c[..., 0], py - c[..., 1], pz - c[..., 2]
        d5, d6 = dot(abx, aby, abz, cpx, cpy, cpz), dot(acx, acy, acz, cpx, cpy, cpz)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        denom = ONE / ((va + vb) + vc)
        w_bc = e43 / (e43 + e56)
        tests = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e43 >= 0) & (e56 >= 0)]
        zero, one = np.zeros_like(d1), np.ones_like(d1)
        vs = [zero, one, d1 / (d1 - d3), zero, zero, ONE - w_bc, vb * denom]
        ws = [zero, zero, zero, one, d2 / (d2 - d6), w_bc, vc * denom]
        region = np.full(d1.shape, 6, np.int8)
        v, w = vs[6], ws[6]
        for r in range(5, -1, -1):                                       # the first test that holds decides
            region = np.where(tests[r], np.int8(r), region)
            v = np.where(tests[r], vs[r], v)
            w = np.where(tests[r], ws[r], w)
        x = (a[..., 0] + abx * v) + acx * w
        y = (a[..., 1] + aby * v) + acy * w
        z = (a[..., 2] + abz * v) + acz * w
        ex, ey, ez = px - x, py - y, pz - z
        dd = dot(ex, ey, ez, ex, ey, ez)
    assert dd.dtype == F32 and v.dtype == F32 and x.dtype == F32
    return region, v, w, np.stack([x, y, z], -1), dd


class Closest:
    pass


def closest_points(vertices, triangles, queries, max_dist2=np.inf, chunk=1 << 20):
    """-> Closest: triangle uint32 [Q], point f32 [Q, 4] (x, y, z, d2), bary f32 [Q, 4] (u, v, w, 0), region int8 [Q] (-1 without a
    winner), counts uint64 [6] (the first six of the call's eight)."""
    v, t, q = _v4(vertices), _tri(triangles), _v4(queries)
    max_dist2 = F32(max_dist2)
    el = eligible(v, t)
    ids = np.where(el)[0]
    E, Q = len(ids), len(q)
    out = Closest()
    out.triangle = np.full(Q, NONE, np.uint32)
    out.point = np.empty((Q, 4), F32)
    out.point.view(np.uint32)[:, :3] = NAN_BITS
    out.point[:, 3] = INF
    out.bary = np.zeros((Q, 4), F32)
    out.region = np.full(Q, -1, np.int8)
    if E and Q:
        a, b, c = (v[t[ids, k]][None, :, :3] for k in range(3))
        step = max(1, chunk // E)
        for q0 in range(0, Q, step):
            p = q[q0:q0 + step, None, :3]
            region, bv, bw, point, d2 = routine(p, a, b, c)              # [q, E]
            with np.errstate(invalid="ignore"):
                adm = (d2 <= max_dist2) & np.isfinite(p).all(-1)         # a NaN is never admissible; a non-finite query has no winner
            best = np.where(adm, d2, INF).min(1)
            first = (adm & (d2 == best[:, None])).argmax(1)              # ties: the smaller index (ids ascend)
            won = adm.any(1)
            rows = np.arange(len(won))[won]
            k = first[won]
            qi = q0 + rows
            out.triangle[qi] = ids[k]
            out.point[qi, :3] = point[rows, k]
            out.point[qi, 3] = d2[rows, k]
            vv, ww = bv[rows, k], bw[rows, k]
            out.bary[qi, 0] = (ONE - vv) - ww
            out.bary[qi, 1] = vv
            out.bary[qi, 2] = ww
            out.region[qi] = region[rows, k]
    won = out.triangle != NONE
    n = int(won.sum())
    top_bits, top_q = 0, NONE
    if n:
        bits = out.point[:, 3].view(np.uint32).astype(np.uint64)
        packed = np.where(won, bits << np.uint64(32) | (np.uint64(NONE) - np.arange(Q, dtype=np.uint64)), np.uint64(0)).max()
        top_bits, top_q = int(packed) >> 32, NONE - (int(packed) & NONE)
    out.counts = np.array([n, Q - n, E, len(t) - E, top_bits, top_q], np.uint64)
    return out


# ------------------------------------------------------------------------------------------------ the sort keys and their tree
def _spread(x):
    x = x.astype(np.uint64)
    out = np.zeros_like(x)
    for bit in range(10):
        out |= ((x >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit)
    return out


def sort_keys(vertices, triangles):
    """The sorted 62-bit keys of the eligible triangles: the 30-bit Morton code of the centroid ((a + b) + c) / 3 in the box of the
    eligible centroids (cell = clamp(((c - lo) / (hi - lo)) * 1024, 0, 1023), a NaN gives 0) << 32 | the triangle's index."""
    v, t = _v4(vertices), _tri(triangles)
    ids = np.where(eligible(v, t))[0]
    if not len(ids):
        return np.zeros(0, np.uint64)
    a, b, c = (v[t[ids, k]][:, :3] for k in range(3))
    with np.errstate(all="ignore"):
        cen = ((a + b) + c) / F32(3)
        lo, hi = cen.min(0), cen.max(0)
        s = ((cen - lo) / (hi - lo)) * F32(1024)
        cell = np.where(np.isnan(s), F32(0), np.minimum(np.maximum(s, F32(0)), F32(1023))).astype(np.uint32)
    code = _spread(cell[:, 0]) << np.uint64(2) | _spread(cell[:, 1]) << np.uint64(1) | _spread(cell[:, 2])
    return np.sort(code << np.uint64(32) | ids.astype(np.uint64))


def tree_depth(keys):
    """The largest number of internal nodes on a root-to-leaf path of the binary radix tree over sorted unique keys (0 for E <= 1)."""
    keys = [int(k) for k in keys]
    deepest, todo = 0, [(0, len(keys), 1)]
    while todo:
        lo, hi, depth = todo.pop()
        if hi - lo < 2:
            continue
        deepest = max(deepest, depth)
        top = (keys[lo] ^ keys[hi - 1]).bit_length() - 1                # the highest bit in which the range's ends differ
        mid = next(i for i in range(lo + 1, hi) if (keys[i] >> top) & 1)
        todo += [(lo, mid, depth + 1), (mid, hi, depth + 1)]
    return deepest


def lower_bound(lo, hi, p, m):
    """The traversal's bound for a box [lo, hi] ([..., 3] each) and queries p, as DESIGN section 28 derives it, f32 operation by
    operation: the squared distance to the box grown by slack = m 2^-18 + 2^-126 (m: the largest |coordinate| of mesh and query), less
    2^-19 of itself and 2^-120.  -> (bound, slack)."""
    with np.errstate(all="ignore"):
        slack = (m * F32(2.0 ** -18) + F32(2.0 ** -126))[..., None]
        e = np.maximum(np.maximum(lo - p, p - hi) - slack, ZERO)
        bound = np.maximum(dot(e[..., 0], e[..., 1], e[..., 2], e[..., 0], e[..., 1], e[..., 2]) * F32(1 - 2.0 ** -19) - F32(2.0 ** -120), ZERO)
    assert bound.dtype == F32
    return bound, slack


# ------------------------------------------------------------------------------------------------ shared inputs
def positions(xyz):
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    return np.concatenate([xyz, np.zeros((len(xyz), 1), F32)], 1)


def soup(n_tri, seed, size=0.08, offset=0.0):
    """n_tri separate triangles with corners within `size` of a centre in the unit cube, translated by `offset` on every axis."""
    rng = np.random.default_rng(seed)
    centre = rng.random((n_tri, 1, 3))
    corners = (centre + (rng.random((n_tri, 3, 3)) - 0.5) * 2 * size).astype(F32) + F32(offset)
    return positions(corners.reshape(-1, 3)), np.arange(3 * n_tri, dtype=np.uint32).reshape(-1, 3)


def cube_queries(n, seed, offset=0.0):
    return positions(np.random.default_rng(seed).random((n, 3)).astype(F32) + F32(offset))


REGION_TRIANGLE = positions([[0, 0, 0], [4, 0, 0], [0, 3, 0]])


@functools.lru_cache(maxsize=None)
def region_queries():
    """Queries around REGION_TRIANGLE planted in each of the seven regions, at z = 0.75 and z = -0.75, then a grid around it."""
    planted = {"vertex A": (-1, -1), "vertex B": (6, -0.5), "edge AB": (2, -1), "vertex C": (-0.5, 5), "edge AC": (-1, 1.5), "edge BC": (3, 3),
               "face": (1, 1)}
    pts = [(x, y, z) for name in REGIONS for (x, y) in [planted[name]] for z in (0.75, -0.75)]
    g = np.linspace(-2, 6, 17)
    pts += [(x, y, z) for x in g for y in g for z in (-0.5, 0.0, 0.5)]
    return positions(pts)


@functools.lru_cache(maxsize=None)
def deep_chain():
    """Centroids at exactly x = 2^-k, k = 0 .. 29 (triangles of 2^-8 of x around them), the last one 33 times over: 62 triangles."""
    xs = [2.0 ** -k for k in range(30)] + [2.0 ** -29] * 32
    s = 2.0 ** -8
    tri = np.array([[[x * (1 - s), -x * s, 0], [x * (1 + s), -x * s, 0], [x, 2 * x * s, 0]] for x in xs], F32)
    v = positions(tri.reshape(-1, 3))
    t = np.arange(3 * len(xs), dtype=np.uint32).reshape(-1, 3)
    rng = np.random.default_rng(5)
    q = positions(np.concatenate([np.stack([np.array(xs[:30], F32), np.zeros(30, F32), np.full(30, 2.0 ** -30, F32)], 1),
                                  (rng.random((200, 3)) * [1.2, 0.02, 0.02] - [0.1, 0.01, 0.01]).astype(F32)]))
    return v, t, q


@functools.lru_cache(maxsize=None)
def translated_soup():
    """500 triangles x 2000 queries translated by +1024 on every axis; the first 600 queries sit within 64 ulp (of 1024) of a face of
    some triangle's box: on it, and 1 .. 64 ulp outside it, beside a point of the triangle's own face."""
    v, t = soup(500, 11, offset=1024.0)
    q = cube_queries(2000, 12, offset=1024.0)
    ulp = np.spacing(F32(1024))
    tri = v[t][:, :, :3]
    hi = tri.max(1)
    mid = ((tri[:, 0] + tri[:, 1]) / 2 + tri[:, 2]) / 2
    rng = np.random.default_rng(13)
    for i in range(600):
        k, axis = i % 500, i % 3
        p = mid[k].copy()
        p[axis] = hi[k, axis] + ulp * F32(rng.integers(0, 65))
        q[i, :3] = p
    return v, t, q


@functools.lru_cache(maxsize=None)
def two_clusters():
    """64 triangles inside [0, 1]^3, 64 inside [7, 8] x [0, 1]^2, 300 queries inside [0, 1]^3."""
    rng = np.random.default_rng(21)

    def cluster(x0):
        centre = 0.1 + 0.8 * rng.random((64, 1, 3))
        return (centre + (rng.random((64, 3, 3)) - 0.5) * 0.2 + [x0, 0, 0]).astype(F32)
    tri = np.concatenate([cluster(0.0), cluster(7.0)])
    return positions(tri.reshape(-1, 3)), np.arange(3 * 128, dtype=np.uint32).reshape(-1, 3), cube_queries(300, 22)


@functools.lru_cache(maxsize=None)
def straying_pairs():
    """Where the routine's point leaves the triangle's box, so that the plain box distance is no lower bound.  40 pairs of long triangles
    (A, B, C) and (A, B, C2) with A about 1000 from B: at vertex B the point is a + (b - a) . 1, which misses b by the rounding of
    b - a -- some ulp of 1000, far more than an ulp of b.  Every query lies in the vertex-B region of both, (g, -s) from B with g << s,
    outside the first triangle's box by (g, s) and beside the second's by s alone; both give the same point and the same d2, the tie
    belongs to the first (smaller index), and its box's plain distance exceeds that d2 wherever the point strays towards the query.
    -> vertices, triangles (pair i = triangles 2 i and 2 i + 1), queries (50 per pair)."""
    rng = np.random.default_rng(77)
    tri, q = [], []
    for i in range(40):
        b = np.array([0.0, 10.0 * i, 0.0]) + rng.random(3) * 0.01
        a = b + [-1000.3 - rng.random(), 0.7, 0.0]
        tri += [[a, b, b + [-0.5, 0.5, 0.0]], [a, b, b + [0.5, 0.5, 0.0]]]
        for _ in range(50):
            q.append(b + [rng.uniform(0.0005, 0.002), -rng.uniform(0.005, 0.02), rng.uniform(-1e-4, 1e-4)])
    v = positions(np.array(tri, np.float64).reshape(-1, 3))
    return v, np.arange(len(v), dtype=np.uint32).reshape(-1, 3), positions(q)


@functools.lru_cache(maxsize=None)
def one_near_many_far():
    """One triangle inside [0, 1]^3, 64 inside [7, 8] x [0, 1]^2, 200 queries inside [0, 1]^3: the root splits the one leaf from the rest."""
    v, t, q = two_clusters()
    keep = np.concatenate([[5], np.arange(64, 128)])
    return v, t[keep], q[:200]
