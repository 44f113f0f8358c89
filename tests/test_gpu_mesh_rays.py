"""dfusion_mesh_ray_hits and its Python mirrors against the brute-force numpy restatement tests/mesh_rays_ref.py: triangle, hit, bary
and counts [0] - [5], bit for bit, through the C-ABI into guarded buffers -- nearest hit and any-hit on every case.  The winner does
not depend on the tree, so any over-eager pruning shows up as an inequality."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mesh_closest_ref as M
import mesh_rays_ref as Y
import mesh_ref as R
from dynamicfusion_amd import capi, mesh_ops, ray_hits, visible_points
from mesh_gpu import ptr, stream, u32

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID = 100001
GUARD = 4                                            # guard rows behind every output
G32 = -7                                             # what they hold
NONE = Y.NONE
ANY = 1                                              # DF_RAYS_ANY_HIT
GRID_CAP = 2048 * 256                                # DF_MESH_MAX_BLOCKS workgroups of 256 lanes: past it a lane takes a second element
INF = float("inf")


def raw(v, t, o, d, t_min=0.0, t_max=INF, flags=0, with_bary=True):
    """One dfusion_mesh_ray_hits call into guarded buffers -> (triangle uint32 [R], hit as uint32 [R, 4], bary as uint32 [R, 4] -- None
    each where not asked for --, counts uint64 [8])."""
    v, t, o, d = M._v4(v), M._tri(t), M._v4(o), M._v4(d)
    V, T, n = len(v), len(t), len(o)
    vd = torch.from_numpy(v).cuda()
    td = torch.from_numpy(t.view(np.int32)).cuda()
    od, dd = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    tri = torch.full((n + GUARD,), G32, dtype=torch.int32, device="cuda")
    hit = torch.full((n + GUARD, 4), G32, dtype=torch.int32, device="cuda")
    bary = torch.full((n + GUARD, 4), G32, dtype=torch.int32, device="cuda")
    counts = torch.full((8 + GUARD,), 123, dtype=torch.int64, device="cuda")
    any_hit = bool(flags & ANY)
    with_bary = with_bary and not any_hit
    capi.check(capi.lib().dfusion_mesh_ray_hits(ptr(vd) if V else None, V, ptr(td) if T else None, T, ptr(od) if n else None, ptr(dd) if n else None, n,
                                                t_min, t_max, flags, ptr(tri) if n else None, ptr(hit) if n and not any_hit else None,
                                                ptr(bary) if with_bary and n else None, ptr(counts), stream()), "dfusion_mesh_ray_hits")
    torch.cuda.synchronize()
    assert (tri[n:] == G32).all() and (hit[n:] == G32).all() and (bary[n:] == G32).all() and (counts[8:] == 123).all()
    assert with_bary or (bary == G32).all()
    assert not any_hit or (hit == G32).all()
    return u32(tri[:n]), None if any_hit else u32(hit[:n]), u32(bary[:n]) if with_bary else None, counts[:8].cpu().numpy().astype(np.uint64)


def check(v, t, o, d, t_min=0.0, t_max=INF, with_bary=True, want=None):
    """The call equals the restatement, in both modes; -> (the restatement's result, the nearest-hit call's counts, the any-hit call's)."""
    want = Y.ray_hits(v, t, o, d, t_min, t_max) if want is None else want
    tri, hit, bary, n = raw(v, t, o, d, t_min, t_max, 0, with_bary)
    bad = np.where(tri != want.triangle)[0]
    assert not len(bad), (len(bad), bad[:5], tri[bad[:5]], want.triangle[bad[:5]], hit[bad[:5], 3].view(F32), want.hit[bad[:5], 3])
    assert np.array_equal(hit, want.hit.view(np.uint32)), int((hit != want.hit.view(np.uint32)).any(1).sum())
    assert not with_bary or np.array_equal(bary, want.bary.view(np.uint32)), int((bary != want.bary.view(np.uint32)).any(1).sum())
    assert np.array_equal(n[:6], want.counts), (n, want.counts)
    tri_any, _, _, n_any = raw(v, t, o, d, t_min, t_max, ANY)
    assert np.array_equal(tri_any, np.where(want.any, 0, NONE).astype(np.uint32)), int((tri_any != np.where(want.any, 0, NONE)).sum())
    assert np.array_equal(n_any[:6], want.counts) and n_any[6] <= n[6] and n_any[7] <= n[7], (n_any, n)
    return want, n, n_any


# ------------------------------------------------------------------------------------------------ tiny trees
@pytest.mark.parametrize("T", [0, 1, 2, 3, 5])
def test_tiny_trees(T):
    v, t = M.soup(5, 3, size=0.3)
    o, d = Y.aimed_rays(v, t[:T], 600, 4)
    want, n, n_any = check(v, t[:T], o, d)
    assert want.counts[2] == T and (want.counts[0] >= 290) == (T > 0)   # of the 300 aimed ones a few graze an edge
    assert (n[7] > 0) == (T >= 2)                                        # one leaf: no internal node


def test_no_eligible_triangle_no_ray_no_vertex():
    v, t = M.soup(4, 3)
    o, d = Y.cube_rays(70, 4)
    d[::10, :3] = 0
    want, n, _ = check(v, [[0, 1, 1], [0, 1, 99], [5, 5, 5]], o, d)     # E == 0 with T > 0: invalid rays are still counted
    assert want.counts.tolist() == [0, 70, 0, 3, 7, 0] and n[6] == 0 and n[7] == 0
    want, n, _ = check(v, t, o[:0], d[:0])                              # R == 0: the triangles are still counted
    assert n.tolist() == [0, 0, 4, 0, 0, 0, 0, 0]
    want, n, _ = check(v[:0], t, o, d)                                  # V == 0: every triangle is skipped
    assert n.tolist() == [0, 70, 0, 4, 7, 0, 0, 0]
    want, n, _ = check(v[:0], t[:0], o, d)                              # T == 0
    assert n.tolist() == [0, 70, 0, 0, 7, 0, 0, 0]
    want, n, _ = check(v[:0], t[:0], o[:0], d[:0])
    assert n.tolist() == [0] * 8


def test_the_same_triangle_named_three_ways_and_coincident_triangles():
    v = M.positions([[0.3, -0.2, 0.7], [4.3, -0.2, 0.7], [0.3, 2.8, 2.2]])
    o, d = Y.cube_rays(400, 8)
    o[:, :3] = o[:, :3] * F32(3) + F32([0, 0, 3])
    d[:, 2] = -np.abs(d[:, 2]) - F32(0.2)
    want, n, _ = check(v, [[0, 1, 2], [2, 1, 0], [1, 2, 0]], o, d)
    assert want.counts[0] > 40 and len(set(want.triangle[want.any].tolist())) > 1       # each naming has bits of its own: no tie is promised
    v = M.positions([[0, 0, 0], [3, 0, 0], [0, 3, 0]])
    o[:, 2] = 1
    want, n, _ = check(v, [[0, 1, 2]] * 70, o, d)                       # equal codes: the index bits alone split the 70 keys
    assert (want.triangle[want.any] == 0).all() and want.counts[0] > 100 and n[7] > 0
    want, n, _ = check(np.tile(v, (70, 1)), np.arange(210).reshape(70, 3), o, d)
    assert (want.triangle[want.any] == 0).all()


def test_the_deep_chain():
    v, t, q = M.deep_chain()
    o = q.copy()
    o[:, 2] = 1
    d = M.positions(np.tile([0, 0, -1], (len(q), 1)))
    d[30:, :2] = (np.random.default_rng(6).random((len(q) - 30, 2)) - 0.5) * 0.01
    want, n, _ = check(v, t, o, d)
    assert want.counts[0] >= 30 and M.tree_depth(M.sort_keys(v, t)) == 15
    check(v, t, o, d, t_min=1.0, t_max=1.0)


# ------------------------------------------------------------------------------------------------ hostile inputs
def test_skipped_triangles_mixed_in():
    v, t = M.soup(400, 31)
    rng = np.random.default_rng(32)
    t = t.copy()
    v = v.copy()
    kinds = rng.integers(0, 12, len(t))
    t[kinds == 0, 1] = len(v) + 7                                        # index >= V
    t[kinds == 1, 2] = 0xffffffff
    t[kinds == 2, 2] = t[kinds == 2, 0]                                  # repeated index
    v[t[kinds == 3, 0], 1] = np.nan
    v[t[kinds == 4, 2], 0] = np.inf
    v[t[kinds == 5, 1], 2] = -np.inf
    v[:, 3] = np.where(rng.random(len(v)) < 0.1, np.nan, v[:, 3])        # w takes no part
    want, n, _ = check(v, t, *Y.cube_rays(1000, 33))
    assert want.counts[3] == (kinds < 6).sum() > 100 and want.counts[2] == (kinds >= 6).sum() and want.counts[0] > 100


def test_invalid_rays_and_signed_zero_and_denormal_components():
    v, t = M.soup(300, 41, size=0.15)
    o, d = Y.cube_rays(1100, 42)
    o[::11, 0], o[1::11, 1], o[2::11, 2] = np.nan, np.inf, -np.inf
    d[3::11, 0], d[4::11, 1], d[5::11, 2] = np.nan, np.inf, -np.inf
    d[6::11, :3] = [0.0, -0.0, 0.0]                                      # no direction
    d[7::11, 0] = -0.0                                                   # valid: one parallel axis
    d[8::11, 1], d[8::11, 2] = 2.0 ** -140, -0.0                         # valid: a denormal component's reciprocal overflows -- two parallel axes
    d[9::11, :3] = [2.0 ** -140, -2.0 ** -149, 2.0 ** -127]              # valid, and parallel on every axis
    o[10::11, 3] = d[10::11, 3] = np.nan                                 # w ignored
    want, n, _ = check(v, t, o, d)
    assert want.counts[4] == 700 and want.counts[0] > 50
    assert want.any[7::11].sum() > 10 and want.any[10::11].sum() > 10 and not want.any[9::11].any()


def test_t_min_and_t_max():
    v, t = M.soup(300, 51, size=0.15)
    o, d = Y.cube_rays(800, 52)
    free = Y.ray_hits(v, t, o, d)
    ts = np.sort(free.hit[free.any, 3])
    assert ts[0] > 0 and len(ts) > 200
    exact = float(ts[100])
    below, above = float(np.nextafter(ts[100], F32(0))), float(np.nextafter(ts[100], F32(9)))
    hits = {}
    for name, limits in {"to exact": (0.0, exact), "to below": (0.0, below), "from exact": (exact, INF), "from above": (above, INF),
                         "only exact": (exact, exact), "behind": (-5.0, INF), "behind only": (-5.0, 0.0), "nan min": (float("nan"), INF),
                         "nan max": (0.0, float("nan")), "empty": (1.0, 0.5), "free": (0.0, INF)}.items():
        want, n, _ = check(v, t, o, d, *limits)
        hits[name] = int(want.counts[0])
    assert hits["to exact"] >= hits["to below"] + 1 and hits["only exact"] >= 1 and hits["from exact"] >= hits["from above"]
    assert hits["nan min"] == hits["nan max"] == hits["empty"] == 0 and hits["behind"] > hits["free"] and hits["behind only"] > 50


# ------------------------------------------------------------------------------------------------ the rule's own inputs
@pytest.mark.parametrize("offset,scale", [(0.0, 1.0), (1024.0, 1.0), (0.0, 1e18), (0.0, 1e-18)])
def test_random_soup(offset, scale):
    v, t = M.soup(2000, 61, offset=offset)
    o, d = Y.cube_rays(1024, 62, offset=offset, scale=scale)
    v = v * F32(scale)
    want, n, _ = check(v, t, o, d)
    if scale == 1.0:
        assert 0.5 < want.counts[0] / 1024 < 0.9 and n[6] < 2000 * 1024 // 10       # the tree prunes at all


def test_slivers_where_the_clamp_binds():
    v, t, o, d = Y.slivers(300, 20, 9)
    want, n, _ = check(v, t, o, d)
    assert want.bound > 50 and want.counts[0] > 5000


def test_grid_plane_with_axis_parallel_in_plane_and_oblique_rays():
    v, t = Y.grid_plane()
    o, d, n_axis = Y.grid_rays()
    want, n, _ = check(v, t, o, d)
    assert want.any[:n_axis].all() and not want.any[n_axis:n_axis + 243].any() and want.any[n_axis + 243:].sum() > 200
    check(v + F32([100, -50, 25, 0]), t, o + F32([100, -50, 25, 0]), d)


# ------------------------------------------------------------------------------------------------ grid caps, nullable bary
def test_more_rays_than_the_grid_cap():
    v, t = M.soup(8, 81, size=0.3)
    want, n, _ = check(v, t, *Y.aimed_rays(v, t, GRID_CAP + 3, 82))
    assert want.counts[0] + want.counts[1] == GRID_CAP + 3 and want.counts[0] > GRID_CAP // 2 and want.any[-3:].any()


def test_more_triangles_than_the_grid_cap():
    g = np.arange(513, dtype=F32) / F32(512)
    x, y = np.meshgrid(g, g, indexing="xy")
    v = M.positions(np.stack([x.ravel(), y.ravel(), np.zeros(513 * 513, F32)], 1))
    i = (np.arange(512)[:, None] * 513 + np.arange(512)[None, :]).ravel().astype(np.uint32)
    t = np.concatenate([np.stack([i, i + 1, i + 513], 1), np.stack([i + 1, i + 514, i + 513], 1),
                        np.array([[0, 512, 513 * 512], [513 * 513 - 1, 513 * 512, 512]], np.uint32)])      # plus two, over the whole plane
    assert len(t) == GRID_CAP + 2
    o, d = Y.cube_rays(16, 83)
    o[:, 2] = 1
    d[:, :3] = d[:, :3] * F32(0.2) - F32([0, 0, 1])
    o[:4, :2] = np.round(o[:4, :2] * 512) / 512                          # above grid vertices: seven-fold ties
    d[:4, :2] = 0
    want, n, _ = check(v, t, o, d)
    assert want.counts[0] >= 12 and want.counts[2] == GRID_CAP + 2


def test_nullable_bary():
    v, t = M.soup(50, 91, size=0.2)
    check(v, t, *Y.cube_rays(100, 92), with_bary=False)                 # (raw asserts that nothing was written)


# ------------------------------------------------------------------------------------------------ pruning, derived
def test_a_near_wall_is_tested_alone():
    """The root has the wall as a leaf and the 64 far triangles as a subtree; every ray meets the wall at t < 0.2 and would enter the far
    box at tn > 0.8.  Nearer child first: the wall is tested, best < 0.2, the subtree is pruned -- exactly one test and one node per ray.
    The farther child first would walk into the subtree with best = t_max."""
    v, t, o, d = Y.wall_and_far()
    want, n, n_any = check(v, t, o, d)
    assert (want.triangle == 0).all()
    assert n[6] == len(o) and n[7] == len(o), (n, len(o))
    assert n_any[6] == len(o) and n_any[7] == len(o)


def test_rays_on_a_grown_face_of_a_parallel_axis_still_reach_the_triangle():
    """o.x lies exactly on a face of the triangle's grown box and d.x = 0: by the rule's explicit parallel case the box passes, so the walk
    tests the triangle (and finds no candidate) -- one test per ray and leaf.  Computing the slab products there gives 0 * inf."""
    v, t, o, d = Y.grown_face_rays()
    want, n, _ = check(v, t, o, d)
    assert want.counts[1] == 64 and n[6] == 64 and n[7] == 0
    want, n, _ = check(v, [[0, 1, 2]] * 3, o, d)                        # three leaves with that box under two internal nodes
    assert n[6] == 3 * 64 and n[7] == 2 * 64


def test_the_far_cluster_is_pruned():
    """The root splits the two clusters (top x bit).  Every ray hits the near cluster at t <= 2; the far box begins at tn >= 7.9: at most
    the near cluster's 64 tests per ray."""
    v, t, o, d = Y.two_clusters_rays()
    want, n, _ = check(v, t, o, d)
    assert n[6] <= 64 * len(o), (n[6], 64 * len(o))


# ------------------------------------------------------------------------------------------------ repeats, the Python mirrors
def test_repeats_streams_and_released_scratch():
    small, big = (M.soup(40, 101, size=0.2), Y.cube_rays(90, 102)), (M.soup(3000, 103), Y.cube_rays(500, 104))
    wants = [Y.ray_hits(*m[0], *m[1]) for m in (small, big)]
    tests = []
    for k in (0, 0, 1, 0):                                               # the same call twice; a large one, then a small one in the same scratch
        tests.append(check(*(small, big)[k][0], *(small, big)[k][1], want=wants[k])[1][6:].tolist())
    assert tests[0] == tests[1] == tests[3]                              # [6] and [7] are reproducible for one input
    with torch.cuda.stream(torch.cuda.Stream()):
        check(*big[0], *big[1], want=wants[1])
        check(*small[0], *small[1], want=wants[0])
    assert capi.lib().dfusion_release_scratch() == 0
    check(*big[0], *big[1], want=wants[1])


@functools.lru_cache(None)
def sphere():
    m = R.mesh_of("sphere")
    v = np.ascontiguousarray(m.vertices, F32)
    t = np.ascontiguousarray(m.triangles, np.uint32)
    return v, t, torch.from_numpy(v).cuda(), torch.from_numpy(t.view(np.int32)).cuda()


def test_python_mirrors_equal_the_raw_call():
    v, t = M.soup(500, 121)
    o, d = Y.cube_rays(700, 122)
    vd, td, od, dd = torch.from_numpy(v).cuda(), torch.from_numpy(t.view(np.int32)).cuda(), torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    tri, hit, bary, n = raw(v, t, o, d)
    g = ray_hits(vd, td, od, dd, return_barycentric=True, return_counts=True)
    assert [x.dtype for x in g] == [torch.int32, torch.float32, torch.float32, torch.int64] and len(ray_hits(vd, td, od, dd)) == 2
    assert np.array_equal(u32(g[0]), tri) and np.array_equal(u32(g[1]), hit) and np.array_equal(u32(g[2]), bary) and g[3].tolist() == n.tolist()
    assert mesh_ops.ray_hits is ray_hits and len(mesh_ops.RAY_COUNT_NAMES) == 8
    tri2, hit2, _, n2 = raw(v, t, o, d, 0.25, 0.75)
    g = ray_hits(vd, td, od, dd, t_min=0.25, t_max=0.75, return_counts=True)
    assert np.array_equal(u32(g[0]), tri2) and np.array_equal(u32(g[1]), hit2) and g[2].tolist() == n2.tolist() and 0 < n2[0] < n[0]
    tri3, _, _, n3 = raw(v, t, o, d, flags=ANY)
    g = ray_hits(vd, td, od, dd, any_hit=True, return_counts=True)
    assert len(g) == 2 and np.array_equal(u32(g[0]), tri3) and g[1].tolist() == n3.tolist()
    e = ray_hits(vd, td[:0], od[:3], dd[:3], return_counts=True)
    assert u32(e[0]).tolist() == [NONE] * 3 and e[2].tolist() == [0, 3, 0, 0, 0, 0, 0, 0]
    assert ray_hits(vd, td, od[:0], dd[:0])[1].shape == (0, 4)
    for bad in (lambda: ray_hits(vd[:, :3], td, od, dd), lambda: ray_hits(vd, td, od.double(), dd), lambda: ray_hits(vd, td, od, dd[:5]),
                lambda: ray_hits(vd, td, od, dd, any_hit=True, return_barycentric=True)):
        with pytest.raises(ValueError):
            bad()


def test_visible_points_of_a_fetch_mesh_sphere_seen_from_outside():
    """Every vertex of the extracted sphere from an eye outside it: the restatement's mask, in which the hemisphere that faces the eye is
    seen and the one behind hidden."""
    v, t, vd, td = sphere()
    pd = vd[::4].contiguous()                                            # a quarter of the vertices: the restatement is a brute force
    p = v[::4]
    centre = v[:, :3].mean(0)
    radius = float(np.linalg.norm(v[:, :3] - centre, axis=1).mean())
    eye = (centre + F32([0.3, -0.2, -3.0]) * F32(radius)).astype(F32)
    want = Y.visible_points(v, t, p, eye)
    got = visible_points(vd, td, pd, [float(x) for x in eye])
    assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(visible_points(vd, td, pd, torch.from_numpy(eye)).cpu().numpy(), want)
    towards = ((p[:, :3] - centre) @ (eye - centre)) / (radius * np.linalg.norm(eye - centre))       # the cosine at the centre
    # the eye, at distance D = |(0.3, -0.2, -3)| r = 3.02 r, sees the cap cosine > r / D = 0.331; a voxel of slack on either side
    assert want[towards > 0.45].all() and not want[towards < 0.2].any()
    assert want.sum() == (towards > 0.45).sum() + want[(towards <= 0.45) & (towards >= 0.2)].sum() and 0.25 < want.mean() < 0.45
    pts = vd[:5].clone()
    pts[1, 0], pts[3, 2] = float("nan"), float("inf")
    want5 = Y.visible_points(v, t, pts.cpu().numpy(), eye)
    assert visible_points(vd, td, pts, eye.tolist()).cpu().numpy().tolist() == want5.tolist() and not want5[1] and not want5[3]
    assert visible_points(vd, td, vd[:0], eye.tolist()).shape == (0,)
    assert visible_points(vd, td, pd, eye.tolist(), margin=1.0).all()   # nothing of the segment is looked at


# ------------------------------------------------------------------------------------------------ argument checks
def test_every_argument_check():
    L = capi.lib()
    v, t = M.soup(5, 111, size=0.3)
    o, d = Y.cube_rays(6, 112)
    vd, td, od, dd = torch.from_numpy(v).cuda(), torch.from_numpy(t.view(np.int32)).cuda(), torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    tri = torch.zeros(16, dtype=torch.int32, device="cuda")
    hit = torch.zeros((16, 4), dtype=torch.float32, device="cuda")
    bary = torch.zeros((16, 4), dtype=torch.float32, device="cuda")
    n = torch.zeros(8, dtype=torch.int64, device="cuda")
    big = 1 << 32
    good = lambda **kw: [kw.get("vtx", ptr(vd)), kw.get("V", 15), kw.get("tris", ptr(td)), kw.get("T", 5), kw.get("o", ptr(od)), kw.get("d", ptr(dd)),
                         kw.get("R", 6), kw.get("t_min", 0.0), kw.get("t_max", INF), kw.get("flags", 0), kw.get("tri", ptr(tri)), kw.get("hit", ptr(hit)),
                         kw.get("bary", ptr(bary)), kw.get("counts", ptr(n)), None]
    assert L.dfusion_mesh_ray_hits(*good()) == 0
    torch.cuda.synchronize()
    want = Y.ray_hits(v, t, o, d)
    assert n.tolist()[:6] == want.counts.tolist() and np.array_equal(u32(tri[:6]), want.triangle) and np.array_equal(u32(hit[:6]), want.hit.view(np.uint32))
    inputs = (vd, td, od, dd)
    bad_calls = [dict(vtx=None), dict(tris=None), dict(o=None), dict(d=None), dict(tri=None), dict(hit=None), dict(counts=None), dict(V=big), dict(T=big),
                 dict(R=big), dict(flags=2), dict(flags=3), dict(flags=1 << 31), dict(flags=ANY), dict(flags=ANY, bary=None), dict(flags=ANY, hit=None)]
    bad_calls += [{out: ptr(x)} for out in ("tri", "hit", "bary", "counts") for x in inputs]
    bad_calls += [dict(hit=C.c_void_p(od.data_ptr() + 80)), dict(tri=C.c_void_p(td.data_ptr() + 56)), dict(bary=C.c_void_p(vd.data_ptr() + 224)),
                  dict(tri=C.c_void_p(dd.data_ptr() + 92)), dict(flags=ANY, hit=None, bary=None, tri=ptr(dd))]
    for bad in bad_calls:
        assert L.dfusion_mesh_ray_hits(*good(**bad)) == INVALID, bad
    assert L.dfusion_mesh_ray_hits(*good(bary=None)) == 0                                               # nullable
    assert L.dfusion_mesh_ray_hits(*good(flags=ANY, hit=None, bary=None)) == 0
    assert L.dfusion_mesh_ray_hits(*good(o=None, d=None, R=0, tri=None, hit=None, bary=None)) == 0    # arrays of length 0 may be NULL
    torch.cuda.synchronize()
    assert n.tolist() == [0, 0, 5, 0, 0, 0, 0, 0]
    assert L.dfusion_mesh_ray_hits(*good(tris=None, T=0)) == 0
    assert L.dfusion_mesh_ray_hits(*good(vtx=None, V=0)) == 0
    torch.cuda.synchronize()
    assert n.tolist() == [0, 6, 0, 5, 0, 0, 0, 0] and u32(tri[:6]).tolist() == [NONE] * 6
