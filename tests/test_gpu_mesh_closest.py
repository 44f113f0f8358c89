"""dfusion_mesh_closest_points and its Python mirrors against the brute-force numpy restatement tests/mesh_closest_ref.py: triangle,
point, bary and counts [0] - [5], bit for bit, through the C-ABI into guarded buffers.  The winner does not depend on the tree, so any
over-eager pruning shows up as an inequality."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mesh_closest_ref as M
import mesh_ref as R
from dynamicfusion_amd import capi, closest_points, mesh_distance, mesh_ops, simplify_mesh
from mesh_gpu import ptr, stream, u32

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID = 100001
GUARD = 4                                            # guard rows behind every output
G32 = -7                                             # what they hold
NONE = M.NONE
GRID_CAP = 2048 * 256                                # DF_MESH_MAX_BLOCKS workgroups of 256 lanes: past it a lane takes a second element
INF = float("inf")


def raw(v, t, q, max_d2=INF, with_bary=True):
    """One dfusion_mesh_closest_points call into guarded buffers -> (triangle uint32 [Q], point as uint32 [Q, 4], bary as uint32 [Q, 4] or
    None, counts uint64 [8])."""
    v, t, q = M._v4(v), M._tri(t), M._v4(q)
    V, T, Q = len(v), len(t), len(q)
    vd = torch.from_numpy(v).cuda()
    td = torch.from_numpy(t.view(np.int32)).cuda()
    qd = torch.from_numpy(q).cuda()
    tri = torch.full((Q + GUARD,), G32, dtype=torch.int32, device="cuda")
    point = torch.full((Q + GUARD, 4), G32, dtype=torch.int32, device="cuda")
    bary = torch.full((Q + GUARD, 4), G32, dtype=torch.int32, device="cuda")
    counts = torch.full((8 + GUARD,), 123, dtype=torch.int64, device="cuda")
    capi.check(capi.lib().dfusion_mesh_closest_points(ptr(vd) if V else None, V, ptr(td) if T else None, T, ptr(qd) if Q else None, Q, max_d2,
                                                      ptr(tri) if Q else None, ptr(point) if Q else None, ptr(bary) if with_bary and Q else None,
                                                      ptr(counts), stream()), "dfusion_mesh_closest_points")
    torch.cuda.synchronize()
    assert (tri[Q:] == G32).all() and (point[Q:] == G32).all() and (bary[Q:] == G32).all() and (counts[8:] == 123).all()
    assert with_bary or (bary == G32).all()
    return u32(tri[:Q]), u32(point[:Q]), u32(bary[:Q]) if with_bary else None, counts[:8].cpu().numpy().astype(np.uint64)


def check(v, t, q, max_d2=INF, with_bary=True, want=None):
    """The call equals the restatement; -> (the restatement's result, the call's counts)."""
    want = M.closest_points(v, t, q, max_d2) if want is None else want
    tri, point, bary, n = raw(v, t, q, max_d2, with_bary)
    bad = np.where(tri != want.triangle)[0]
    assert not len(bad), (len(bad), bad[:5], tri[bad[:5]], want.triangle[bad[:5]], point[bad[:5], 3].view(F32), want.point[bad[:5], 3])
    assert np.array_equal(point, want.point.view(np.uint32)), int((point != want.point.view(np.uint32)).any(1).sum())
    assert not with_bary or np.array_equal(bary, want.bary.view(np.uint32)), int((bary != want.bary.view(np.uint32)).any(1).sum())
    assert np.array_equal(n[:6], want.counts), (n, want.counts)
    return want, n


# ------------------------------------------------------------------------------------------------ tiny trees
@pytest.mark.parametrize("T", [0, 1, 2, 3, 5])
def test_tiny_trees(T):
    v, t = M.soup(5, 3, size=0.3)
    q = M.cube_queries(300, 4)
    want, n = check(v, t[:T], q)
    assert want.counts[0] == (300 if T else 0) and want.counts[2] == T
    assert n[6] >= (300 if T else 0) and (n[7] > 0) == (T >= 2)         # one leaf: no internal node


def test_no_eligible_triangle_no_query_no_vertex():
    v, t = M.soup(4, 3)
    q = M.cube_queries(70, 4)
    want, n = check(v, [[0, 1, 1], [0, 1, 99], [5, 5, 5]], q)            # E == 0 with T > 0
    assert want.counts.tolist() == [0, 70, 0, 3, 0, NONE] and n[6] == 0 and n[7] == 0
    want, n = check(v, t, q[:0])                                         # Q == 0: the triangles are still counted
    assert want.counts.tolist() == [0, 0, 4, 0, 0, NONE]
    want, n = check(v[:0], t, q)                                         # V == 0: every triangle is skipped
    assert want.counts.tolist() == [0, 70, 0, 4, 0, NONE]
    want, n = check(v[:0], t[:0], q[:0])
    assert n.tolist() == [0, 0, 0, 0, 0, NONE, 0, 0]


# ------------------------------------------------------------------------------------------------ the routine
def test_the_seven_region_triangle():
    q = M.region_queries()
    want, n = check(M.REGION_TRIANGLE, [[0, 1, 2]], q)
    assert set(want.region.tolist()) == set(range(7))
    sheared = M.REGION_TRIANGLE + F32([0.3, -0.2, 0.7, 0])
    sheared[2, 2] += 1.5
    check(sheared, [[0, 1, 2], [2, 1, 0], [1, 2, 0]], q)                # the same triangle named three ways: every tie to index 0


def test_coincident_triangles_tie_to_index_0():
    v = M.positions([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    q = M.cube_queries(200, 8)
    want, n = check(v, [[0, 1, 2]] * 70, q)                             # equal codes: the index bits alone split the 70 keys
    assert (want.triangle == 0).all() and n[7] > 0
    want, n = check(np.tile(v, (70, 1)), np.arange(210).reshape(70, 3), q)
    assert (want.triangle == 0).all()


def test_the_deep_chain():
    v, t, q = M.deep_chain()
    want, n = check(v, t, q)
    assert want.counts[0] == len(q) and M.tree_depth(M.sort_keys(v, t)) == 15
    check(v, t, q, max_d2=float(F32(2.0 ** -40)))


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
    want, n = check(v, t, M.cube_queries(1000, 33))
    assert want.counts[3] == (kinds < 6).sum() > 100 and want.counts[2] == (kinds >= 6).sum() and want.counts[0] == 1000


def test_non_finite_queries():
    v, t = M.soup(100, 41)
    q = M.cube_queries(400, 42)
    q[::7, 0], q[1::7, 1], q[2::7, 2] = np.nan, np.inf, -np.inf
    q[3::7, 3] = np.nan                                                  # w ignored
    want, n = check(v, t, q)
    assert want.counts[1] == len(q[::7]) + len(q[1::7]) + len(q[2::7])


def test_max_dist2():
    v, t = M.soup(300, 51)
    q = M.cube_queries(800, 52)
    free = M.closest_points(v, t, q)
    d2 = np.sort(free.point[:, 3])
    assert d2[0] > 0
    exact = float(d2[400])                                               # exactly at a candidate: admitted
    below = float(np.nextafter(d2[400], F32(0)))
    got = {}
    for limit in (0.0, float(d2[5]), exact, below, INF, -1.0, float("nan")):
        want, n = check(v, t, q, max_d2=limit)
        got[repr(limit)] = int(want.counts[0])
    assert got[repr(exact)] == got[repr(below)] + 1 == 401 and got[repr(0.0)] == 0 and got[repr(INF)] == 800 and got[repr(float(d2[5]))] == 6
    on = M.positions(v[t[:50, 0], :3])                                   # queries on vertices: d2 == 0 is within max_dist2 == 0
    want, n = check(v, t, on, max_d2=0.0)
    assert want.counts[0] == 50 and want.counts[4] == 0 and want.counts[5] == 0


# ------------------------------------------------------------------------------------------------ soups and a real mesh
def test_random_soup():
    v, t = M.soup(2000, 61)
    want, n = check(v, t, M.cube_queries(4096, 62))
    assert n[6] < 2000 * 4096 // 10                                      # the tree prunes at all


def test_translated_soup():
    v, t, q = M.translated_soup()
    want, n = check(v, t, q)
    assert want.counts[0] == 2000


def test_large_coordinates_and_a_wide_range():
    rng = np.random.default_rng(71)
    v, t = M.soup(300, 72)
    q = M.cube_queries(500, 73)
    check(v * F32(1e18), t, q * F32(1e18))                               # squares near the top of the f32 range
    check(v * F32(1e-18), t, q * F32(1e-18))                             # and in the denormals
    v[:, :3] *= (10.0 ** rng.uniform(-3, 3, (300, 1, 1)) * np.ones((1, 3, 1))).reshape(900, 1).astype(F32)
    check(v, t, q)


@functools.lru_cache(None)
def sphere():
    m = R.mesh_of("sphere")
    vd = torch.from_numpy(np.ascontiguousarray(m.vertices, F32)).cuda()
    td = torch.from_numpy(np.ascontiguousarray(m.triangles, np.uint32).view(np.int32)).cuda()
    sv, st, src, vmap = simplify_mesh(vd, td, 2 * float(R.VS[0]))
    return m.vertices, m.triangles, vd, td, sv, st


def test_a_fetch_mesh_sphere_queried_by_its_simplified_vertices():
    v, t, vd, td, sv, st = sphere()
    q = sv.cpu().numpy()
    want, n = check(v, t, q)
    assert len(q) > 100 and want.counts[0] == len(q) and want.point[:, 3].max() < (2 * float(R.VS[0])) ** 2 * 3


# ------------------------------------------------------------------------------------------------ grid caps
def test_more_queries_than_the_grid_cap():
    v, t = M.soup(8, 81, size=0.3)
    want, n = check(v, t, M.cube_queries(GRID_CAP + 3, 82))
    assert want.counts[0] == GRID_CAP + 3


def test_more_triangles_than_the_grid_cap():
    g = np.arange(513, dtype=F32) / F32(512)
    x, y = np.meshgrid(g, g, indexing="xy")
    v = M.positions(np.stack([x.ravel(), y.ravel(), np.zeros(513 * 513, F32)], 1))
    i = (np.arange(512)[:, None] * 513 + np.arange(512)[None, :]).ravel().astype(np.uint32)
    t = np.concatenate([np.stack([i, i + 1, i + 513], 1), np.stack([i + 1, i + 514, i + 513], 1),
                        np.array([[0, 512, 513 * 512], [513 * 513 - 1, 513 * 512, 512]], np.uint32)])      # plus two, over the whole plane
    assert len(t) == GRID_CAP + 2
    q = M.cube_queries(16, 83)
    q[:, 2] *= F32(0.01)
    q[:4, :2] = np.round(q[:4, :2] * 512) / 512                          # above grid vertices: six-fold ties
    want, n = check(v, t, q)
    assert want.counts[0] == 16 and want.counts[2] == GRID_CAP + 2


def test_nullable_bary():
    v, t = M.soup(50, 91)
    check(v, t, M.cube_queries(100, 92), with_bary=False)               # (raw asserts that nothing was written)


# ------------------------------------------------------------------------------------------------ pruning, derived
def test_the_far_cluster_is_pruned():
    """The root splits the two clusters (top x bit).  After the near cluster best <= 3 (both in the unit cube); the far box is >= 6 away,
    36 less the slack: so the nearer child first and the far subtree pruned mean at most the near cluster's 64 tests per query."""
    v, t, q = M.two_clusters()
    want, n = check(v, t, q)
    assert n[6] <= 64 * len(q), (n[6], 64 * len(q))


def test_one_near_triangle_is_tested_alone():
    """The root has the one near triangle as a leaf and the 64 far ones as a subtree, >= 6 away.  Nearer child first: the leaf is tested,
    best <= 3, the subtree's bound is >= 36 less the slack and it is pruned -- exactly one test and one node per query.  The farther
    child first would walk into the subtree with best = +inf."""
    v, t, q = M.one_near_many_far()
    want, n = check(v, t, q)
    assert n[6] == len(q) and n[7] == len(q), (n, len(q))


def test_points_that_stray_out_of_their_triangles_box():
    """The bound must carry its slack: without it the first triangle of a pair is pruned behind the second's equal d2."""
    v, t, q = M.straying_pairs()
    want, n = check(v, t, q)
    assert (want.triangle % 2 == 0).all()


# ------------------------------------------------------------------------------------------------ repeats, the Python mirrors
def test_repeats_streams_and_released_scratch():
    small, big = (M.soup(40, 101), M.cube_queries(90, 102)), (M.soup(3000, 103), M.cube_queries(500, 104))
    wants = [M.closest_points(*m[0], m[1]) for m in (small, big)]
    tests = []
    for k in (0, 0, 1, 0):                                               # the same call twice; a large one, then a small one in the same scratch
        tests.append(check(*(small, big)[k][0], (small, big)[k][1], want=wants[k])[1][6:].tolist())
    assert tests[0] == tests[1] == tests[3]                              # [6] and [7] are reproducible for one input
    with torch.cuda.stream(torch.cuda.Stream()):
        check(*big[0], big[1], want=wants[1])
        check(*small[0], small[1], want=wants[0])
    assert capi.lib().dfusion_release_scratch() == 0
    check(*big[0], big[1], want=wants[1])


def test_python_mirrors_equal_the_raw_call():
    v, t, vd, td, sv, st = sphere()
    q = sv.cpu().numpy()
    tri, point, bary, n = raw(v, t, q)
    g = closest_points(vd, td, sv, return_barycentric=True, return_counts=True)
    assert [x.dtype for x in g] == [torch.int32, torch.float32, torch.float32, torch.int64] and len(closest_points(vd, td, sv)) == 2
    assert np.array_equal(u32(g[0]), tri) and np.array_equal(u32(g[1]), point) and np.array_equal(u32(g[2]), bary) and g[3].tolist() == n.tolist()
    assert mesh_ops.closest_points is closest_points and len(mesh_ops.CLOSEST_COUNT_NAMES) == 8
    d = float(np.sqrt(np.sort(point[:, 3].view(F32))[len(q) // 2]))      # a limit that about half the queries meet
    lim = F32(d) * F32(d)
    tri2, point2, bary2, n2 = raw(v, t, q, float(lim))
    g = closest_points(vd, td, sv, max_distance=d, return_counts=True)
    assert np.array_equal(u32(g[0]), tri2) and g[2].tolist() == n2.tolist() and 0 < n2[0] < len(q)
    e = closest_points(vd, td[:0], sv[:3], return_counts=True)
    assert u32(e[0]).tolist() == [NONE] * 3 and e[2].tolist()[:6] == [0, 3, 0, 0, 0, NONE]
    assert closest_points(vd, td, sv[:0])[1].shape == (0, 4)
    with pytest.raises(ValueError):
        closest_points(vd[:, :3], td, sv)
    with pytest.raises(ValueError):
        closest_points(vd, td, sv.double())

    md = mesh_distance(vd, td, sv, st)
    sides = {"a_to_b": (np.ascontiguousarray(v, F32), sv.cpu().numpy(), st.cpu().numpy()), "b_to_a": (q, v, t)}
    for name, (samples, mv, mt) in sides.items():
        tri, point, bary, n = raw(mv, mt, samples)
        got, won = md[name], tri != NONE
        d2 = point[:, 3].view(F32)[won].astype(np.float64)
        assert got["answered"] == n[0] == won.sum() and got["unanswered"] == n[1] and got["max_vertex"] == n[5]
        assert got["max"] == float(np.sqrt(np.float64(np.uint32(n[4]).view(F32)))) == float(np.sqrt(d2.max()))
        rel = len(d2) * 2.0 ** -53                                       # the summation order alone differs
        assert abs(got["mean"] - np.sqrt(d2).sum() / len(d2)) <= rel * got["mean"]
        assert abs(got["rms"] - np.sqrt(d2.sum() / len(d2))) <= rel * got["rms"]
    assert md["hausdorff"] == max(md["a_to_b"]["max"], md["b_to_a"]["max"]) > 0
    same = mesh_distance(vd, td, vd, td)
    assert same["hausdorff"] == 0 and same["a_to_b"]["rms"] == 0 and same["a_to_b"]["answered"] == len(v)


# ------------------------------------------------------------------------------------------------ argument checks
def test_every_argument_check():
    L = capi.lib()
    v, t = M.soup(5, 111)
    q = M.cube_queries(6, 112)
    vd, td, qd = torch.from_numpy(v).cuda(), torch.from_numpy(t.view(np.int32)).cuda(), torch.from_numpy(q).cuda()
    tri = torch.zeros(16, dtype=torch.int32, device="cuda")
    point = torch.zeros((16, 4), dtype=torch.float32, device="cuda")
    bary = torch.zeros((16, 4), dtype=torch.float32, device="cuda")
    n = torch.zeros(8, dtype=torch.int64, device="cuda")
    big = 1 << 32
    good = lambda **kw: [kw.get("vtx", ptr(vd)), kw.get("V", 15), kw.get("tris", ptr(td)), kw.get("T", 5), kw.get("q", ptr(qd)), kw.get("Q", 6),
                         kw.get("max_d2", INF), kw.get("tri", ptr(tri)), kw.get("point", ptr(point)), kw.get("bary", ptr(bary)), kw.get("counts", ptr(n)), None]
    assert L.dfusion_mesh_closest_points(*good()) == 0
    torch.cuda.synchronize()
    want = M.closest_points(v, t, q)
    assert n.tolist()[:6] == want.counts.tolist() and np.array_equal(u32(tri[:6]), want.triangle) and np.array_equal(u32(point[:6]), want.point.view(np.uint32))
    bad_calls = [dict(vtx=None), dict(tris=None), dict(q=None), dict(tri=None), dict(point=None), dict(counts=None), dict(V=big), dict(T=big), dict(Q=big),
                 dict(tri=ptr(vd)), dict(tri=ptr(td)), dict(tri=ptr(qd)), dict(point=ptr(vd)), dict(point=ptr(td)), dict(point=ptr(qd)),
                 dict(bary=ptr(vd)), dict(bary=ptr(td)), dict(bary=ptr(qd)), dict(counts=ptr(vd)), dict(counts=ptr(td)), dict(counts=ptr(qd)),
                 dict(point=C.c_void_p(qd.data_ptr() + 80)), dict(tri=C.c_void_p(td.data_ptr() + 56)), dict(bary=C.c_void_p(vd.data_ptr() + 224))]
    for bad in bad_calls:
        assert L.dfusion_mesh_closest_points(*good(**bad)) == INVALID, bad
    assert L.dfusion_mesh_closest_points(*good(bary=None)) == 0                                           # nullable
    assert L.dfusion_mesh_closest_points(*good(q=None, Q=0, tri=None, point=None, bary=None)) == 0      # arrays of length 0 may be NULL
    torch.cuda.synchronize()
    assert n.tolist() == [0, 0, 5, 0, 0, NONE, 0, 0]
    assert L.dfusion_mesh_closest_points(*good(tris=None, T=0)) == 0
    assert L.dfusion_mesh_closest_points(*good(vtx=None, V=0)) == 0
    torch.cuda.synchronize()
    assert n.tolist() == [0, 6, 0, 5, 0, NONE, 0, 0] and u32(tri[:6]).tolist() == [NONE] * 6
