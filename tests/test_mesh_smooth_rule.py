"""The numpy restatement tests/mesh_smooth_ref.py (the rules of dfusion_mesh_adjacency and dfusion_mesh_smooth) against a dict-and-loop
implementation written here, its topology counts against mesh_ref.edge_use, and what the smoothing does to the shared meshes.  No GPU."""
import numpy as np
import pytest

import mesh_ref as R
import mesh_smooth_ref as S

F32 = np.float32


# ------------------------------------------------------------------------------------------------ the rules once more, in loops
def loop_adjacency(triangles, V):
    half = {}                                                            # (a, b) -> the number of half-edges a -> b
    invalid = degenerate = 0
    for tri in np.asarray(triangles).reshape(-1, 3).tolist():
        tri = [int(i) & 0xffffffff for i in tri]
        if not all(i < V for i in tri):
            invalid += 1
            continue
        if len(set(tri)) < 3:
            degenerate += 1
        for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
            if a != b:
                half[(a, b)] = half.get((a, b), 0) + 1
    rows = [set() for _ in range(V)]
    for a, b in half:
        rows[a].add(b)
        rows[b].add(a)
    cls = [1 if r else 0 for r in rows]
    n_edges = n_boundary = n_irregular = 0
    for lo, hi in {(min(a, b), max(a, b)) for a, b in half}:
        f, b = half.get((lo, hi), 0), half.get((hi, lo), 0)
        n_edges += 1
        if f == 1 and b == 1:
            c = 1
        elif f + b == 1:
            c, n_boundary = 2, n_boundary + 1
        else:
            c, n_irregular = 3, n_irregular + 1
        cls[lo], cls[hi] = max(cls[lo], c), max(cls[hi], c)
    row_start, neighbours = [0], []
    for r in rows:
        neighbours += sorted(r)
        row_start.append(len(neighbours))
    counts = [len(neighbours), n_edges, n_boundary, n_irregular, sum(1 for r in rows if r), invalid, degenerate, sum(1 for c in cls if c >= 2)]
    return row_start, neighbours, cls, counts


def loop_step(P, row_start, neighbours, cls, s, fix):
    Q = P.copy()
    with np.errstate(all="ignore"):
        for v in range(len(P)):
            row = neighbours[row_start[v]:row_start[v + 1]]
            if not len(row) or (fix and cls[v] != 1):
                continue
            for a in range(3):
                acc = F32(0)
                for u in row:
                    acc = F32(acc + P[u, a])
                mean = F32(acc / F32(len(row)))
                delta = F32(mean - P[v, a])
                Q[v, a] = F32(P[v, a] + F32(F32(s) * delta))
    return Q


def same_as_loops(t, V):
    a = S.adjacency(t, V)
    rs, nb, cls, counts = loop_adjacency(t, V)
    assert a.row_start.tolist() == rs and a.neighbours.tolist() == nb and a.vertex_class.tolist() == cls
    assert [int(c) for c in a.counts] == counts
    assert a.row_start.dtype == np.uint32 and a.neighbours.dtype == np.uint32 and a.vertex_class.dtype == np.uint8 and a.counts.dtype == np.uint64
    return a


CASES = S.small_cases()


@pytest.mark.parametrize("name,V,t", CASES, ids=[c[0] for c in CASES])
def test_adjacency_of_the_small_cases_equals_the_loops(name, V, t):
    a = same_as_loops(t, V)
    c = [int(x) for x in a.counts]
    if name == "one triangle":
        assert c == [6, 3, 3, 0, 3, 0, 0, 3] and a.vertex_class.tolist() == [2, 2, 2]
    if name == "two triangles on an edge":
        assert c[:4] == [10, 5, 4, 0] and a.vertex_class.tolist() == [2, 2, 2, 2] and a.neighbours.tolist() == [1, 2, 3, 0, 2, 3, 0, 1, 0, 1]
    if name == "two triangles on an edge, same direction":
        assert c[:4] == [10, 5, 4, 1] and a.vertex_class.tolist() == [3, 3, 2, 2]      # used twice in the same direction: irregular
    if name in ("the same triangle twice", "a rotation is the same triangle"):
        assert c[:4] == [6, 3, 0, 3]
    if name == "a triangle and its reverse":
        assert c[:4] == [6, 3, 0, 0] and a.vertex_class.tolist() == [1, 1, 1]
    if name == "tetrahedron":
        assert c == [12, 6, 0, 0, 4, 0, 0, 0] and S.euler(a, 4) == 2
    if name == "tetrahedron with one face flipped":
        assert c[:4] == [12, 6, 0, 3] and sorted(a.edges[a.edge_class == 3].tolist()) == [[1, 2], [1, 3], [2, 3]]
    if name == "fan of three on one edge":
        assert c[:4] == [14, 7, 6, 1] and a.edges[a.edge_class == 3].tolist() == [[0, 1]] and a.vertex_class.tolist() == [3, 3, 2, 2, 2]
    if name == "(a, a, b)":
        assert c == [4, 2, 0, 0, 3, 0, 2, 0]                                           # a -> b and b -> a: an interior edge
    if name == "(a, a, a)":
        assert c == [0, 0, 0, 0, 0, 0, 1, 0]
    if name == "no vertex":
        assert c == [0, 0, 0, 0, 0, 2, 0, 0] and a.row_start.tolist() == [0]
    if name.startswith("index"):
        assert c[5] == 1 and c[1] == 6 and c[2] == 3


@pytest.mark.parametrize("seed", range(4))
def test_adjacency_of_soups_with_bad_and_degenerate_triangles_equals_the_loops(seed):
    _, t = S.soup(900, 60, seed, p_bad=0.03, p_degenerate=0.1, p_reverse=0.3)
    a = same_as_loops(t, 60)
    assert a.counts[5] > 20 and a.counts[6] > 30 and a.counts[3] > 100 and (a.f + a.b >= 3).any() and ((a.f == 2) & (a.b == 0)).any()


@pytest.mark.parametrize("fix", [0, 1])
def test_steps_equal_the_loops(fix):
    v, t = S.soup(700, 90, 5, p_bad=0.02, p_degenerate=0.05, p_reverse=0.2, lo=-3.0, hi=3.0)
    t = np.concatenate([t, 90 + S.strip(40)[1], 132 + S.double_hub(12)])             # a strip (class 2) and a closed surface (class 1) beside it
    v = np.concatenate([v, S.strip(40)[0], S.positions(14)])
    a = S.adjacency(t, len(v))
    rs, nb, cls, _ = loop_adjacency(t, len(v))
    assert (a.vertex_class == 1).sum() > 10 and (a.vertex_class == 2).sum() > 10 and (a.vertex_class == 3).sum() > 10
    want = loop_step(loop_step(v, rs, nb, cls, 0.5, fix), rs, nb, cls, -0.53, fix)
    got = S.smooth(v, a, 1, 0.5, -0.53, flags=fix)
    assert got.tobytes() == want.tobytes()
    assert S.smooth(v, a, 1, 0.5, 0.0, flags=fix).tobytes() == loop_step(v, rs, nb, cls, 0.5, fix).tobytes()
    assert np.array_equal(got[:, 3], v[:, 3])                                          # w is copied
    if fix:
        still = a.vertex_class != 1
        assert got[still].tobytes() == v[still].tobytes() and (got[~still, :3] != v[~still, :3]).any(1).all()
        every = S.smooth(v, a, 1, 0.5, -0.53, flags=fix, use_class=False)             # no classes: every vertex with a neighbour is class 1
        assert every.tobytes() == S.smooth(v, a, 1, 0.5, -0.53, flags=0).tobytes()


def test_nan_and_inf_propagate_to_the_neighbours_only():
    m = R.mesh_of("sphere")
    a = S.adjacency_of("sphere")
    v = m.vertices.copy()
    v[100, 1], v[2000, 0] = np.nan, np.inf
    out = S.smooth(v, a, 1, 0.5, 0.0)
    bad = ~np.isfinite(out[:, :3]).all(1)
    ring = set(a.neighbours[a.row_start[100]:a.row_start[101]].tolist()) | set(a.neighbours[a.row_start[2000]:a.row_start[2001]].tolist()) | {100, 2000}
    assert set(np.nonzero(bad)[0].tolist()) == ring


# ------------------------------------------------------------------------------------------------ topology of the shared meshes
@pytest.mark.parametrize("name,E,boundary,irregular,chi,classes", [
    ("sphere", 14934, 0, 0, 2, [0, 4980, 0, 0]),
    ("torus", 28236, 0, 0, 0, [0, 9412, 0, 0]),
    ("cut", 9787, 182, 0, 1, [0, 3142, 182, 0]),
    ("hand", 2408, 184, 0, -1, [4, 679, 184, 0]),
])
def test_topology_counts_of_the_extracted_meshes(name, E, boundary, irregular, chi, classes):
    m = R.mesh_of(name)
    a = S.adjacency_of(name)
    und, use, fwd = R.edge_use(m.triangles)                              # the helper the mesh tests have used so far
    assert len(und) == E and int((use == 1).sum()) == boundary and int(((use != 1) & ~((use == 2) & (fwd == 1))).sum()) == irregular
    assert [int(c) for c in a.counts[:4]] == [2 * E, E, boundary, irregular] and a.counts[5] == 0 and a.counts[6] == 0
    assert np.array_equal(a.edges, und) and np.array_equal(a.f, fwd) and np.array_equal(a.b, use - fwd)
    assert S.euler(a, len(m.triangles)) == chi
    assert np.bincount(a.vertex_class, minlength=4).tolist() == classes and a.counts[7] == classes[2] + classes[3] and a.counts[4] == sum(classes[1:])
    on_boundary = np.zeros(len(m.vertices), bool)
    on_boundary[und[use == 1].reshape(-1)] = True
    assert np.array_equal(a.vertex_class == 2, on_boundary)
    d = np.diff(a.row_start.astype(np.int64))
    assert d.sum() == len(a.neighbours) and all((np.diff(a.neighbours[a.row_start[v]:a.row_start[v + 1]].astype(np.int64)) > 0).all()
                                                for v in range(0, len(d), 37))


def test_one_flipped_triangle_in_a_closed_mesh_makes_its_three_edges_irregular():
    t = R.mesh_of("sphere").triangles.copy()
    t[1234] = t[1234][[0, 2, 1]]
    a = S.adjacency(t, len(R.mesh_of("sphere").vertices))
    assert [int(c) for c in a.counts[:4]] == [29868, 14934, 0, 3] and a.counts[7] == 3
    assert set(a.edges[a.edge_class == 3].reshape(-1).tolist()) == set(t[1234].tolist()) and ((a.f + a.b)[a.edge_class == 3] == 2).all()
    assert (a.vertex_class[t[1234].astype(np.int64)] == 3).all()


def test_the_adjacency_does_not_depend_on_the_order_of_the_triangles():
    m = R.mesh_of("cut")
    a = S.adjacency_of("cut")
    b = S.adjacency(m.triangles[np.random.default_rng(1).permutation(len(m.triangles))], len(m.vertices))
    for k in ("row_start", "neighbours", "vertex_class", "counts"):
        assert np.array_equal(getattr(a, k), getattr(b, k))


# ------------------------------------------------------------------------------------------------ what the smoothing does
def test_taubin_removes_noise_without_shrinking_and_laplace_shrinks():
    a = S.adjacency_of("sphere")
    v = S.noisy_sphere()
    mean0, rms0 = S.radial(v, S.SPHERE_CENTRE)
    mean1, rms1 = S.radial(S.smooth(v, a, 10), S.SPHERE_CENTRE)
    mean2, _ = S.radial(S.smooth(v, a, 10, mu=0.0), S.SPHERE_CENTRE)
    assert 0.0029 < rms0 < 0.0030                                        # 2.95 mm on a radius of 110.07 mm
    assert rms1 < 0.5 * rms0                                             # this draw: 0.382 x (1.13 mm)
    assert abs(mean1 / mean0 - 1) < 1e-3                                 # this draw: -0.028 %
    assert mean2 / mean0 - 1 < -5e-3                                     # this draw: -0.996 % (plain Laplacian, 10 steps)


def test_taubin_removes_the_slivers_of_marching_tetrahedra():
    m = R.mesh_of("sphere")
    a = S.adjacency_of("sphere")
    before = S.smallest_angles(m.vertices, m.triangles)
    after = S.smallest_angles(S.smooth(m.vertices, a, 10), m.triangles)
    assert (before < 10).mean() > 0.10                                   # 13.36 %, the median smallest angle 30.8 degrees
    assert (after < 10).mean() < 0.005                                   # 0.0 %, the median 42.4 degrees
    assert np.median(after) > np.median(before) + 10


def test_fixed_boundary_zero_iterations_and_unchanged_topology():
    m = R.mesh_of("cut")
    a = S.adjacency_of("cut")
    out = S.smooth(m.vertices, a, 10)
    still = a.vertex_class != 1
    assert still.sum() == 182 and out[still].tobytes() == m.vertices[still].tobytes()
    assert (out[~still, :3] != m.vertices[~still, :3]).any(1).sum() == 3142                 # all the others move
    assert S.smooth(m.vertices, a, 0).tobytes() == m.vertices.tobytes()
    moved = S.smooth(m.vertices, a, 10, flags=0)
    assert (moved[still, :3] != m.vertices[still, :3]).any(1).all()
    b = S.adjacency(m.triangles, len(out))                               # smoothing moves vertices, nothing else
    assert np.array_equal(a.row_start, b.row_start) and np.array_equal(a.neighbours, b.neighbours) and np.array_equal(a.vertex_class, b.vertex_class)


def test_the_order_of_the_sum_matters_on_the_wide_range_soup():
    v, t = S.soup(4000, 300, 13, lo=-3.0, hi=3.0)
    a = S.adjacency(t, 300)
    assert np.diff(a.row_start.astype(np.int64)).min() >= 8
    up = S.step(v, a.row_start, a.neighbours, None, 0.5, 0)
    down = S.step(v, a.row_start, a.neighbours, None, 0.5, 0, descending=True)
    assert (up.view(np.uint32) != down.view(np.uint32)).any(1).sum() > 100
