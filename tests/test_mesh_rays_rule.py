"""The rule of dfusion_mesh_ray_hits as tests/mesh_rays_ref.py restates it, checked on the CPU: that the slab test is monotone in the
box -- the one property the tree's exactness rests on --, that the guard (box and clamp) bites on long slivers and nowhere else among
the shared inputs, the winners against an f64 Moeller-Trumbore, exact hits and ties on a grid plane -- and that the inputs of
tests/test_gpu_mesh_rays.py contain what they claim."""
import ctypes as C
import os

import numpy as np
import pytest

import mesh_closest_ref as M
import mesh_rays_ref as Y

F32 = np.float32
INF = np.inf
DENORMAL = F32(2.0 ** -140)
TINY = F32(2.0 ** -127)                               # a normal-looking step below the smallest normal: 1 / TINY overflows too


def assert_monotone(lo, hi, LO, HI, o, d, slack, t_min=0.0, t_max=INF):
    """Whenever the small box [lo, hi] passes, the large one [LO, HI] passes with TN <= tn and TF >= tf.  -> how many small ones pass."""
    assert (LO <= lo).all() and (HI >= hi).all() and (lo <= hi).all()
    ok, tn, tf = Y.slab(lo, hi, o, d, slack, t_min, t_max)
    OK, TN, TF = Y.slab(LO, HI, o, d, slack, t_min, t_max)
    bad = ok & ~(OK & (TN <= tn) & (TF >= tf))
    assert not bad.any(), (int(bad.sum()), lo[bad][:2], hi[bad][:2], LO[bad][:2], HI[bad][:2], o[bad][:2], d[bad][:2], tn[bad][:2], TN[bad][:2])
    return int(ok.sum())


def nested(rng, n, draw):
    """n nested box pairs from four sorted draws per axis."""
    c = np.sort(draw((n, 3, 4)), axis=2)
    return c[:, :, 1].copy(), c[:, :, 2].copy(), c[:, :, 0].copy(), c[:, :, 3].copy()


def slack_of(lo, hi, LO, HI, o):
    return Y.ray_slack(max(np.abs(LO).max(), np.abs(HI).max()), o) * np.ones(len(o), F32)


@pytest.mark.parametrize("t_range", [(0.0, INF), (-INF, INF), (0.25, 3.0)])
def test_slab_is_monotone_on_quarter_integers_with_special_direction_components(t_range):
    rng = np.random.default_rng(1)
    n = 200000
    quarter = lambda shape: (rng.integers(-16, 17, shape) / 4).astype(F32)
    lo, hi, LO, HI = nested(rng, n, quarter)                            # flat boxes (lo == hi) and shared faces come often
    o = quarter((n, 3))                                                  # origins on faces and inside flat boxes
    special = np.array([0.0, -0.0, DENORMAL, -DENORMAL, TINY, -TINY, 1.0, -1.0, 0.375, -2.5, 3e38, -1e-30], F32)
    d = special[rng.integers(0, len(special), (n, 3))]
    keep = (d != 0).any(1)
    passed = assert_monotone(lo[keep], hi[keep], LO[keep], HI[keep], o[keep], d[keep], slack_of(lo, hi, LO, HI, o)[keep], *t_range)
    assert passed > n // 100, passed                                     # the sample of passing small boxes is not a handful
    flat = (lo == hi).any(1) & keep
    on_face = ((o == lo) | (o == hi)).any(1) & keep
    assert flat.sum() > n // 10 and on_face.sum() > n // 10


def test_slab_is_monotone_on_random_floats():
    rng = np.random.default_rng(2)
    n = 200000
    for scale, offset in [(1.0, 0.0), (1.0, 1024.0), (1e18, 0.0), (1e-18, 0.0), (3e38, 0.0)]:
        uniform = lambda shape: ((rng.random(shape) * 2 - 1 + offset) * scale).astype(F32)
        lo, hi, LO, HI = nested(rng, n, uniform)
        o = uniform((n, 3))
        d = ((rng.random((n, 3)) - 0.5) * scale).astype(F32)
        d[rng.random((n, 3)) < 0.1] = 0
        keep = (d != 0).any(1) & np.isfinite(o).all(1)
        passed = assert_monotone(lo[keep], hi[keep], LO[keep], HI[keep], o[keep], d[keep], slack_of(lo, hi, LO, HI, o)[keep], -INF, INF)
        assert passed > n // 100, (scale, offset, passed)


def test_the_nan_dropping_parallel_case_would_not_be_monotone():
    """What the rule avoids: with (lo - o) * inv computed for a parallel axis too and the 0 * inf NaNs dropped by fminf / fmaxf, a flat box
    through o passes while a larger box with only hi == o computes near = far = -inf on that axis and fails."""
    o, d = F32([[1, 0, 0]]), F32([[0, 0, 1]])
    lo, hi, LO = F32([[1, -1, 2]]), F32([[1, 1, 3]]), F32([[0, -1, 2]])

    def dropping(lo, hi):
        with np.errstate(all="ignore"):
            inv = F32(1) / d
            a, b = (lo - o) * inv, (hi - o) * inv
            near, far = np.fmin(a, b), np.fmax(a, b)
            tn = np.fmax(np.fmax(np.fmax(near[:, 0], near[:, 1]), near[:, 2]), F32(0))
            tf = np.fmin(np.fmin(far[:, 0], far[:, 1]), far[:, 2])
        return bool((tn <= tf)[0])
    assert dropping(lo, hi) and not dropping(LO, hi)
    zero = np.zeros(1, F32)
    assert Y.slab(lo, hi, o, d, zero, 0, INF)[0][0] and Y.slab(LO, hi, o, d, zero, 0, INF)[0][0]      # the rule's explicit case passes both


def pairwise(v, t, o, d, per):
    """Every ray against the sliver it was aimed at -> (candidate, box passes, t, tn, tf)."""
    k = np.repeat(np.arange(len(t)), per)
    a, b, c = (v[t[k, i]][:, :3] for i in range(3))
    det, u, vv, tt = Y.moller_trumbore(o[:, :3], d[:, :3], a, b, c)
    cand = Y.candidates(det, u, vv, tt, 0.0, INF)
    lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
    ok, tn, tf = Y.slab(lo, hi, o[:, :3], d[:, :3], Y.ray_slack(np.abs(v[:, :3]).max(), o[:, :3]), 0.0, INF)
    return cand, ok, tt, tn, tf


SLIVERS_BELOW_ENTRY = 2199                            # of 372 665 candidates among 400 000 pairs; 44 more lie beyond the exit


def test_the_guard_bites_on_long_slivers():
    """Moeller-Trumbore's t of a long sliver hit at a grazing angle falls BELOW the entry parameter of the triangle's own grown vertex
    box: a tree that prunes on tn > best would lose such a winner, whatever slack it adds.  The count is recorded, not a tolerance."""
    v, t, o, d = Y.slivers(400000, 1, 7)
    cand, ok, tt, tn, tf = pairwise(v, t, o, d, 1)
    below = int((cand & ok & (tt < tn)).sum())
    print("slivers: %d candidates, %d with t < tn of their own box, %d with t > tf, %d whose box fails" %
          (cand.sum(), below, (cand & ok & (tt > tf)).sum(), (cand & ~ok).sum()))
    assert below > 0
    assert below == SLIVERS_BELOW_ENTRY and cand.sum() == 372665


def test_the_gpu_sliver_set_makes_the_clamp_bind_and_change_winners():
    v, t, o, d = Y.slivers(300, 20, 9)
    res = Y.ray_hits(v, t, o, d)
    plain = Y.ray_hits(v, t, o, d, clamp=False)
    assert res.bound > 50 and res.counts[0] > 5000
    assert (plain.triangle != res.triangle).sum() >= 5 and (plain.hit.view(np.uint32) != res.hit.view(np.uint32)).any(1).sum() > 50


def f64_winners(v, t, o, d):
    """Plain two-sided Moeller-Trumbore in f64 over all triangles, no box: the nearest t >= 0 -> triangle [R] (NONE without)."""
    a, b, c = (v[t[:, k]][None, :, :3].astype(np.float64) for k in range(3))
    o, d = o[:, None, :3].astype(np.float64), d[:, None, :3].astype(np.float64)
    e1, e2 = b - a, c - a
    p = np.cross(d, e2)
    det = (e1 * p).sum(-1)
    s = o - a
    u = (s * p).sum(-1) / det
    q = np.cross(s, e1)
    vv = (d * q).sum(-1) / det
    tt = (e2 * q).sum(-1) / det
    hit = (det != 0) & (u >= 0) & (vv >= 0) & (u + vv <= 1) & (tt >= 0)
    tt = np.where(hit, tt, np.inf)
    return np.where(hit.any(1), tt.argmin(1), Y.NONE).astype(np.uint32)


@pytest.mark.parametrize("offset", [0.0, 1024.0])
def test_soup_winners_equal_an_f64_moller_trumbore(offset):
    v, t = M.soup(2000, 61, offset=offset)
    o, d = Y.cube_rays(1024, 62, offset=offset)
    res = Y.ray_hits(v, t, o, d)
    share = res.counts[0] / 1024
    assert 0.5 < share < 0.9, share
    assert res.bound == 0 and res.lost == 0                              # the box rejects nothing and the clamp never binds
    if offset == 0.0:                                                    # translated, f32 has 2^-14 left of the soup's 0.08: f64 sees other edges
        assert np.array_equal(res.triangle, f64_winners(v, t, o, d))
    plain = Y.ray_hits(v, t, o, d, grow=False, clamp=False)
    assert np.array_equal(plain.triangle, res.triangle) and np.array_equal(plain.hit.view(np.uint32), res.hit.view(np.uint32))


def test_axis_parallel_rays_through_grid_vertices_hit_exactly_with_ties_to_the_smaller_index():
    v, t = Y.grid_plane()
    o, d, n_axis = Y.grid_rays()
    res = Y.ray_hits(v, t, o, d)
    assert n_axis == 162 and res.any[:n_axis].all()
    assert res.hit[:81, 3].tolist() == [3.0] * 81 and res.hit[81:162, 3].tolist() == [1.0] * 81
    assert np.array_equal(res.hit[:162, :3], np.tile(v[:, :3], (2, 1)))  # the vertices themselves
    lowest = np.array([min(np.where((t == i).any(1))[0]) for i in range(81)], np.uint32)
    assert np.array_equal(res.triangle[:162], np.tile(lowest, 2))
    assert (res.bary[:81, 3] == 1).all() and (res.bary[81:162, 3] == -1).all()      # the normal is +z: from above det > 0
    in_plane = slice(162, 162 + 3 * 81)
    assert not res.any[in_plane].any()                                   # det == 0: a ray in the plane hits nothing
    a, b, c = (v[t[:, k]][:, :3] for k in range(3))
    lo, hi = np.minimum(np.minimum(a, b), c)[None], np.maximum(np.maximum(a, b), c)[None]
    oo, dd = o[in_plane, None, :3], d[in_plane, None, :3]
    ok, tn, tf = Y.slab(lo, hi, oo, dd, np.broadcast_to(Y.ray_slack(8.0, oo), (243, len(t))), 0.0, INF)
    assert ok.any(1).sum() > 200 and (dd == 0).any(-1).all()      # yet their flat boxes pass, through the parallel case
    oblique = slice(162 + 3 * 81, None)
    assert res.any[oblique].sum() > 200
    ungrown = Y.ray_hits(v, t, o, d, grow=False)
    assert ungrown.lost > 20 and (ungrown.triangle != res.triangle).sum() > 5   # why the box is grown


def test_invalid_rays_limits_and_skipped_triangles():
    v = M.positions([[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 2], [4, 0, 2], [0, 4, 2], [np.nan, 0, 1]])
    t = [[0, 1, 2], [3, 4, 5], [0, 1, 6], [0, 0, 1], [0, 1, 9]]
    o = M.positions([[1, 1, 5], [1, 1, 5], [1, 1, 5], [np.nan, 1, 5], [1, 1, 5], [1, 1, 1], [1, 1, 5]])
    d = M.positions([[0, 0, -1], [0, 0, -2], [0, 0, 0], [0, 0, -1], [0, np.inf, -1], [0, -0.0, DENORMAL], [-0.0, 0, -1]])
    o[0, 3] = d[1, 3] = np.nan                                           # w ignored
    res = Y.ray_hits(v, t, o, d)
    assert res.triangle.tolist() == [1, 1, Y.NONE, Y.NONE, Y.NONE, Y.NONE, 1]
    assert res.hit[[0, 1, 6], 3].tolist() == [3.0, 1.5, 3.0] and res.counts.tolist() == [3, 4, 2, 3, 3, 0]
    assert res.bary[0].tolist() == [0.5, 0.25, 0.25, 1.0]
    with np.errstate(over="ignore"):
        assert np.isinf(F32(1) / DENORMAL)                               # ray 5 is parallel on every axis and hits nothing
    for limits, want in [((0, 3), [1, 1]), ((0, np.nextafter(F32(3), F32(0))), [Y.NONE, 1]), ((3, 5), [1, Y.NONE]), ((np.nextafter(F32(3), F32(4)), 5), [0, Y.NONE]), ((2.5, 5), [1, 0]),
                         ((-1, 1), [Y.NONE, Y.NONE]), ((np.nan, 5), [Y.NONE, Y.NONE]), ((0, np.nan), [Y.NONE, Y.NONE]), ((4, 3), [Y.NONE, Y.NONE]),
                         ((-10, INF), [1, 1])]:
        r = Y.ray_hits(v, t, o[:2], d[:2], *limits)
        assert r.triangle.tolist() == want, (limits, r.triangle)
    back = Y.ray_hits(v, t, M.positions([[1, 1, 1]]), M.positions([[0, 0, 1]]), -10, INF)
    assert back.triangle.tolist() == [0] and back.hit[0].tolist() == [1, 1, 0, -1]      # a negative t_min looks behind the origin


def test_visible_points_of_two_parallel_triangles():
    v = M.positions([[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 2], [4, 0, 2], [0, 4, 2], [np.inf, 1, 1]])
    t = [[0, 1, 2], [3, 4, 5]]
    vis = Y.visible_points(v, t, v, [1, 1, 5])
    assert vis.tolist() == [False, False, False, True, True, True, False]
    assert Y.visible_points(v, t, v, [1, 1, 5], margin=0.5).tolist() == [True] * 6 + [False]


# ------------------------------------------------------------------------------------------------ what the GPU cases claim
def test_the_wall_is_a_leaf_of_the_root_and_every_ray_meets_it_first():
    v, t, o, d = Y.wall_and_far()
    keys = M.sort_keys(v, t)
    assert len(keys) == 65 and ((keys >> np.uint64(32 + 29)) & np.uint64(1)).tolist() == [0] + [1] * 64 and int(keys[0]) & 0xffffffff == 0
    res = Y.ray_hits(v, t, o, d)
    assert (res.triangle == 0).all() and res.hit[:, 3].max() < 0.2
    far = v[t[1:]][:, :, :3].reshape(-1, 3)
    ok, tn, tf = Y.slab(far.min(0)[None], far.max(0)[None], o[:, :3], d[:, :3], Y.ray_slack(100.0, o[:, :3]), 0.0, INF)
    assert ok.all() and tn.min() > 0.8                                   # every ray would enter the far box, far behind the wall's t


def test_the_grown_face_rays_lie_exactly_on_the_grown_faces():
    v, t, o, d = Y.grown_face_rays()
    slack = Y.ray_slack(1.0, o[:, :3])
    assert np.array_equal(np.where(np.arange(64) % 2 == 0, F32(0) - slack, F32(1) + slack), o[:, 0])
    ok, tn, tf = Y.slab(F32([[0, 0, 0]]), F32([[1, 1, 0]]), o[:, :3], d[:, :3], slack, 0.0, INF)
    assert ok.all() and (d[:, :2] == 0).all()                            # the rule's parallel case passes the box ...
    with np.errstate(all="ignore"):
        inv = F32(1) / d[:, 0]
        a, b = ((F32(0) - slack) - o[:, 0]) * inv, ((F32(1) + slack) - o[:, 0]) * inv
    assert np.isnan(a[::2]).all() and np.isnan(b[1::2]).all()            # ... where the products would be 0 * inf
    res = Y.ray_hits(v, t, o, d)
    assert not res.any.any() and res.lost == 0


def test_the_ray_clusters_are_separated_by_the_top_x_bit():
    v, t, o, d = Y.two_clusters_rays()
    res = Y.ray_hits(v, t, o, d)
    assert (res.triangle < 64).all() and res.hit[:, 3].max() <= 2.0      # the far box begins at x = 7: tn >= 8 - slack


def test_the_deep_chain_rays_hit():
    v, t, q = M.deep_chain()
    o = q.copy()
    o[:, 2] = 1
    d = M.positions(np.tile([0, 0, -1], (len(q), 1)))
    assert Y.ray_hits(v, t, o, d).counts[0] >= 30


# ------------------------------------------------------------------------------------------------ the layers above the kernel
def test_library_binding_and_mirrors_declare_the_ray_query():
    import inspect
    from dynamicfusion_amd import build, capi, mesh_ops, ray_hits, visible_points
    assert "dfusion_mesh_ray_hits" in capi.SYMBOLS and "dfusion_mesh_rays.hip" in build.SOURCES
    L = C.CDLL(build.build_library())
    assert hasattr(L, "dfusion_mesh_ray_hits") and hasattr(L, "dfusion_mesh_closest_points")
    assert len(capi.load(build.build_library()).dfusion_mesh_ray_hits.argtypes) == 15
    assert build.kernel_source_sha("df_mry_walk_kernel(DfMryArgs)") != build.kernel_source_sha("df_mbv_query_kernel(DfMbvArgs)")
    assert "dfusion_mesh_bvh.h" in build._csrc_includes("dfusion_mesh_rays.hip", []) and "dfusion_mesh_bvh.h" in build._csrc_includes("dfusion_mesh_bvh.hip", [])
    assert mesh_ops.ray_hits is ray_hits and mesh_ops.visible_points is visible_points and len(mesh_ops.RAY_COUNT_NAMES) == 8
    assert list(inspect.signature(ray_hits).parameters)[4:] == ["t_min", "t_max", "any_hit", "return_barycentric", "return_counts"]
    assert inspect.signature(visible_points).parameters["margin"].default == 2.0 ** -10
    hdr = open(os.path.join(build.REPO_DIR, "include", "dfusion.h")).read()
    assert "#define DFUSION_ABI_VERSION 7" in hdr or "ABI 7" in hdr
    cxx = open(os.path.join(build.HOST_DIR, "include", "kfusion", "cuda", "mesh_ops.hpp")).read()
    assert "void rayHits(" in cxx and "void visiblePoints(" in cxx and build.HOST_MESH_RAYS in build.HOST_APPS
