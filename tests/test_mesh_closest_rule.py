"""The rule of dfusion_mesh_closest_points as tests/mesh_closest_ref.py restates it, checked on the CPU: against an independent f64
evaluation (projection onto the plane, the three edges with their ends, then the minimum), exact zeros, the tie rule, skipped
triangles, non-finite queries and max_dist2 -- and that the inputs of tests/test_gpu_mesh_closest.py contain what they claim."""
import numpy as np
import pytest

import mesh_closest_ref as M

F32 = np.float32
EPS = 2.0 ** -24                                     # the unit roundoff of f32


def exact_d2(p, a, b, c):
    """f64: the squared distance of p to the triangle, not by Voronoi regions: the foot on the plane if it lies inside, else the nearest
    of the three segments."""
    p, a, b, c = (np.asarray(x, np.float64)[:3] for x in (p, a, b, c))
    best = np.inf
    for s, e in ((a, b), (b, c), (c, a)):
        d = e - s
        t = np.clip(np.dot(p - s, d) / np.dot(d, d), 0.0, 1.0)
        best = min(best, float(np.sum((p - (s + t * d)) ** 2)))
    n = np.cross(b - a, c - a)
    nn = np.dot(n, n)
    if nn > 0:
        foot = p - n * (np.dot(p - a, n) / nn)
        g = np.array([[np.dot(b - a, b - a), np.dot(b - a, c - a)], [np.dot(b - a, c - a), np.dot(c - a, c - a)]])
        v, w = np.linalg.solve(g, [np.dot(foot - a, b - a), np.dot(foot - a, c - a)])
        if v >= 0 and w >= 0 and v + w <= 1:
            best = min(best, float(np.sum((p - foot) ** 2)))
    return best


def tolerance(p, a, b, c, d2):
    """What |d2_f32 - d2| may be, from the routine's operations.  S = the longest of ab, ac, ap, bp, cp, M = the largest |coordinate|,
    A = the area, kappa = S^2 / (2 A) >= 1.
      each d_i  a dot of two differences: 2 roundings in the inputs, 3 products, 2 adds -> |error| <= 6 eps S^2
      va, vb, vc  two products of d's and one subtraction -> <= 2 (2 . 6 eps S^4) + 2 eps S^4 = 26 eps S^4
      v, w      a quotient over va + vb + vc = 4 A^2 (3 more such errors below the line) -> <= 104 eps S^4 / (4 A^2) = 104 eps kappa^2;
                the edge cases divide one d by a difference of two and are better conditioned than that
      point     ab v + ac w moves by <= 208 eps kappa^2 S, and its own five roundings per axis by <= 16 eps M
      region    where rounding picks a neighbouring region the two regions' points differ by as much again: a factor of 2
    So the point is within D = eps (512 kappa^2 S + 32 M) of the true closest point, the distance within D of the true one, and the final
    dot adds 5 roundings: |d2_f32 - d2| <= 2 sqrt(d2) D + D^2 + 8 eps d2.  Returns (that, kappa)."""
    p, a, b, c = (np.asarray(x, np.float64)[:3] for x in (p, a, b, c))
    S = max(np.linalg.norm(x) for x in (b - a, c - a, p - a, p - b, p - c))
    Mx = max(np.abs(x).max() for x in (p, a, b, c))
    area2 = np.linalg.norm(np.cross(b - a, c - a))
    kappa = S * S / area2 if area2 > 0 else np.inf
    D = EPS * (512 * kappa * kappa * S + 32 * Mx)
    return 2 * np.sqrt(d2) * D + D * D + 8 * EPS * d2, kappa


def one(p, tri):
    """The routine on one query and one triangle -> (region, v, w, point, d2)."""
    r, v, w, pt, d2 = M.routine(np.asarray(p, F32)[None, :3], *(np.asarray(x, F32)[None, :3] for x in tri))
    return int(r[0]), v[0], w[0], pt[0], d2[0]


def test_random_triangles_against_the_f64_evaluation():
    rng = np.random.default_rng(1)
    kept, seen = 0, set()
    for _ in range(3000):
        tri = rng.random((3, 3)).astype(F32) * F32(rng.choice([1.0, 16.0]))
        p = (tri.mean(0) + (rng.random(3) - 0.5) * 2 * rng.choice([0.05, 0.5, 1.5]) * np.abs(tri).max()).astype(F32)
        want = exact_d2(p, *tri)
        tol, kappa = tolerance(p, *tri, want)
        if kappa > 8:                                                    # slivers: the bound is kappa^2 and says nothing there
            continue
        kept += 1
        r, v, w, pt, d2 = one(p, tri)
        seen.add(r)
        assert abs(float(d2) - want) <= tol, (tri, p, float(d2), want, tol, kappa, M.REGIONS[r])
    assert kept > 1500 and seen == set(range(7)), (kept, seen)


def test_the_seven_regions_on_both_sides_of_the_plane():
    tri = M.REGION_TRIANGLE[:, :3]
    q = M.region_queries()
    for i, name in enumerate(M.REGIONS):
        for side in (0, 1):
            p = q[2 * i + side, :3]
            r, v, w, pt, d2 = one(p, tri)
            assert M.REGIONS[r] == name, (name, p, M.REGIONS[r])
            want = exact_d2(p, *tri)
            assert abs(float(d2) - want) <= tolerance(p, *tri, want)[0]
    res = M.closest_points(M.REGION_TRIANGLE, [[0, 1, 2]], q)            # what the GPU case claims: its winners cover all seven
    assert set(res.region.tolist()) == set(range(7)) and min(np.bincount(res.region)) >= 2


@pytest.mark.parametrize("z", [0.0, 5.0])
def test_exact_zeros_on_vertices_edges_and_face(z):
    tri = np.array([[0, 0, z], [4, 0, z], [0, 4, z]], F32)              # every operation of the routine is exact on these
    for p, region in [((0, 0, z), "vertex A"), ((4, 0, z), "vertex B"), ((0, 4, z), "vertex C"), ((2, 0, z), "edge AB"), ((0, 1, z), "edge AC"),
                      ((2, 2, z), "edge BC"), ((3, 1, z), "edge BC"), ((1, 1, z), "face"), ((0.5, 2, z), "face")]:
        r, v, w, pt, d2 = one(p, tri)
        assert M.REGIONS[r] == region and d2 == 0 and np.array_equal(pt, np.asarray(p, F32)), (p, M.REGIONS[r], pt, d2)
    res = M.closest_points(M.positions(tri), [[0, 1, 2]], M.positions([[1, 1, z], [1, 1, z + 2]]))
    assert res.point[:, 3].tolist() == [0.0, 4.0] and res.bary.tolist() == [[0.5, 0.25, 0.25, 0], [0.5, 0.25, 0.25, 0]]
    assert res.counts.tolist() == [2, 0, 1, 0, int(F32(4).view(np.uint32)), 1]


def test_ties_go_to_the_smaller_index():
    v = M.positions([[0, 0, 0], [4, 0, 0], [0, 4, 0], [4, 4, 0]])
    q = M.positions([[2, 2, 3], [2, 2, 0], [3, 1, -1]])                 # above, on and below the shared edge
    for t in ([[0, 1, 2], [1, 3, 2]], [[1, 3, 2], [0, 1, 2]]):
        alone = [M.closest_points(v, [tri], q) for tri in t]
        assert np.array_equal(alone[0].point, alone[1].point)            # an exact tie, as the arithmetic gives it
        res = M.closest_points(v, t, q)
        assert res.triangle.tolist() == [0, 0, 0] and res.point[:, 3].tolist() == [9.0, 0.0, 1.0]
    res = M.closest_points(v, [[1, 3, 2]] * 3 + [[0, 1, 2]] * 4, M.positions([[3, 3, 1], [1, 1, 1], [2, 2, 1]]))
    assert res.triangle.tolist() == [0, 3, 0]                            # duplicates: the first copy; the shared edge: index 0


def test_skipped_triangles_are_counted_and_never_win():
    v = M.positions([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 5], [0, 0, 5], [1, 0, 5], [0, 1, 5], [np.inf, 1, 5]])
    t = [[3, 4, 5], [4, 5, 8], [4, 4, 5], [0, 1, 2], [4, 5, 7], [4, 5, 6]]      # NaN, index >= V, repeated index, fine, inf, fine
    assert M.eligible(v, t).tolist() == [False, False, False, True, False, True]
    res = M.closest_points(v, t, M.positions([[0.2, 0.2, 4], [0.2, 0.2, 1]]))
    assert res.triangle.tolist() == [5, 3] and res.counts[:4].tolist() == [2, 0, 2, 4]
    v[3, 3] = np.nan                                                      # w takes no part
    assert M.eligible(v, t).tolist() == [False, False, False, True, False, True]


def test_non_finite_queries_and_no_eligible_triangle_have_no_winner():
    v = M.positions([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    q = M.positions([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0.2, 0.2, 1]])
    q[3, 3] = np.nan                                                      # w ignored
    res = M.closest_points(v, [[0, 1, 2]], q)
    assert res.triangle.tolist() == [M.NONE] * 3 + [0] and res.counts.tolist() == [1, 3, 1, 0, int(F32(1).view(np.uint32)), 3]
    assert (res.point.view(np.uint32)[:3, :3] == M.NAN_BITS).all() and np.isposinf(res.point[:3, 3]).all() and not res.bary[:3].any()
    for t in ([], [[0, 1, 1]], [[0, 1, 3]]):
        res = M.closest_points(v, np.array(t, np.uint32).reshape(-1, 3), q)
        assert res.counts.tolist() == [0, 4, 0, len(t), 0, M.NONE] and (res.triangle == M.NONE).all()


def test_max_dist2_admits_a_candidate_at_exactly_the_limit():
    v = M.positions([[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 1], [4, 0, 1], [0, 4, 1]])
    t = [[0, 1, 2], [3, 4, 5]]
    q = M.positions([[1, 1, 3], [1, 1, 0.25], [1, 1, 0.5]])              # d2 to the nearer: 4, 0.0625, 0.25 (triangle 1, 0, then a tie -> 0)
    for limit, want in [(np.inf, [1, 0, 0]), (4.0, [1, 0, 0]), (np.nextafter(F32(4), F32(0)), [M.NONE, 0, 0]), (0.0625, [M.NONE, 0, M.NONE]),
                        (0.0, [M.NONE] * 3), (-1.0, [M.NONE] * 3), (np.nan, [M.NONE] * 3)]:
        assert M.closest_points(v, t, q, limit).triangle.tolist() == want, limit


@pytest.mark.parametrize("offset", [0.0, 1024.0])
@pytest.mark.parametrize("sliver", [1.0, 1e-2, 1e-4, 1e-6, 0.0])
def test_the_pruning_bound_never_exceeds_the_routines_d2(offset, sliver):
    """The one requirement on the traversal, on the CPU: for triangles down to exactly collinear ones (sliver = 0), near and far queries,
    at the origin and translated by 1024, the routine's point stays within the slack of the triangle's own box and the bound of that box,
    as computed in f32, is <= the d2 the routine computes.  (A union of boxes only lowers the bound.)"""
    rng = np.random.default_rng(int(offset) + int(sliver * 1e6))
    n = 30000
    for spread in (0.05, 1.0, 20.0):
        a = (rng.random((n, 3)) + offset).astype(F32)
        ab = (rng.random((n, 3)) - 0.5) * 0.2
        ac = ab * rng.random((n, 1)) * 2 + (rng.random((n, 3)) - 0.5) * 0.2 * sliver
        b, c = (a + ab).astype(F32), (a + ac).astype(F32)
        p = (a + (rng.random((n, 3)) - 0.5) * spread).astype(F32)
        region, v, w, point, d2 = M.routine(p, a, b, c)
        lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
        m = np.abs(np.stack([a, b, c, p])).max((0, 2))
        bound, slack = M.lower_bound(lo, hi, p, m)
        ok = np.isfinite(d2)                                             # a NaN d2 is never a candidate
        assert ok.sum() > n // 2
        assert (np.maximum(np.maximum(lo - point, point - hi), 0)[ok] <= slack[ok]).all()
        assert (bound[ok] <= d2[ok]).all()
        assert sliver == 0 or (bound > 0).sum() > n // 10                # and it is not trivially 0


# ------------------------------------------------------------------------------------------------ what the GPU cases claim
DEEP_CHAIN_DEPTH = 15                                # 9 levels of code bits (x cells 1023, 511, .., 1, 0), then 6 of index bits


def test_the_deep_chain_has_the_stated_depth():
    v, t, q = M.deep_chain()
    keys = M.sort_keys(v, t)
    assert len(keys) == 62 and len(set(keys.tolist())) == 62
    codes = keys >> np.uint64(32)
    assert (np.bincount(np.unique(codes, return_inverse=True)[1].reshape(-1)).max()) >= 33          # 33 equal codes: index bits alone split them
    assert M.tree_depth(keys) == DEEP_CHAIN_DEPTH
    assert M.tree_depth(np.arange(70, dtype=np.uint64)) == 7             # 70 coincident triangles: 7 index bits


def test_the_translated_soup_has_queries_within_64_ulp_of_a_box_face():
    v, t, q = M.translated_soup()
    ulp = np.spacing(F32(1024))
    tri = v[t][:, :, :3]
    lo, hi = tri.min(1), tri.max(1)
    near = 0
    for p in q[:600, :3]:
        gap = p[None] - hi                                               # [T, 3], >= 0 outside the face
        inside_others = ((p[None] >= lo) & (p[None] <= hi))
        for axis in range(3):
            others = [k for k in range(3) if k != axis]
            if ((gap[:, axis] >= 0) & (gap[:, axis] <= 64 * ulp) & inside_others[:, others].all(1)).any():
                near += 1
                break
    assert near == 600 and v[:, :3].min() > 1023.5


def test_the_two_clusters_are_separated_by_the_top_x_bit():
    v, t, q = M.two_clusters()
    codes = (M.sort_keys(v, t) >> np.uint64(32)).astype(np.int64)
    ids = (M.sort_keys(v, t) & np.uint64(0xffffffff)).astype(np.int64)
    top_x = (codes >> 29) & 1
    assert np.array_equal(top_x == 1, ids >= 64) and top_x[:64].sum() == 0 and top_x[64:].sum() == 64
    res = M.closest_points(v, t, q)
    assert (res.triangle < 64).all() and res.point[:, 3].max() <= 3.0
    far_lo = v[t[64:]][:, :, 0].min()
    assert far_lo >= 7.0 and q[:, 0].max() <= 1.0                        # the far box is >= 6 away: 36 - slack > 3


def test_the_straying_pairs_stray():
    v, t, q = M.straying_pairs()
    res = M.closest_points(v, t, q)
    assert (res.region == 1).all() and (res.triangle % 2 == 0).all() and (res.triangle // 2 == np.arange(len(q)) // 50).all()
    first, second = v[t[res.triangle]][:, :, :3], v[t[res.triangle + 1]][:, :, :3]
    _, _, _, _, d2_second = M.routine(q[:, :3], second[:, 0], second[:, 1], second[:, 2])
    assert np.array_equal(d2_second, res.point[:, 3])                    # the pair ties exactly
    lo, hi = first.min(1), first.max(1)
    e = np.maximum(np.maximum(lo - q[:, :3], q[:, :3] - hi), 0)
    plain = M.dot(e[:, 0], e[:, 1], e[:, 2], e[:, 0], e[:, 1], e[:, 2])  # the box distance with no slack, in f32
    assert (plain > res.point[:, 3]).sum() > 400                         # no lower bound for hundreds of the 2000 queries
    bound, slack = M.lower_bound(lo, hi, q[:, :3], np.abs(v[:, :3]).max() * np.ones(len(q), F32))
    assert (bound <= res.point[:, 3]).all()


def test_one_near_many_far_is_split_at_the_root():
    v, t, q = M.one_near_many_far()
    keys = M.sort_keys(v, t)
    assert len(keys) == 65 and ((keys >> np.uint64(32 + 29)) & np.uint64(1)).tolist() == [0] + [1] * 64 and int(keys[0]) & 0xffffffff == 0
    res = M.closest_points(v, t, q)
    assert (res.triangle == 0).all() and res.point[:, 3].max() <= 3.0
