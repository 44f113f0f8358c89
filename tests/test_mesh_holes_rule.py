"""The rule of dfusion_mesh_boundary_loops and dfusion_mesh_fill_holes on the CPU: the numpy restatement tests/mesh_holes_ref.py against
an independent dict-and-loop implementation written here, the four properties the rule gives, and the figures of the meshes the GPU
suite runs on -- which show that its cases reach every branch."""
import collections

import numpy as np
import pytest

import mesh_holes_ref as H
import mesh_ref as R
import mesh_smooth_ref as S

F32 = np.float32
NONE = H.NONE


def plain_loops(triangles, V):
    """The rule with dicts and loops, one half-edge at a time -> (next, label, rank as dicts over the vertices that have one, loops as
    lists from the label vertex, counts)."""
    use = collections.Counter()                                                          # (a, b) -> half-edges a -> b
    invalid = degenerate = 0
    for tri in np.asarray(triangles).reshape(-1, 3).tolist():
        a, b, c = (int(x) & 0xffffffff for x in tri)
        if not (a < V and b < V and c < V):
            invalid += 1
            continue
        if a == b or b == c or a == c:
            degenerate += 1
        for s, d in ((a, b), (b, c), (c, a)):
            if s != d:
                use[(s, d)] += 1
    out, inn, irregular = collections.Counter(), collections.Counter(), set()
    heads = {}
    n_boundary = 0
    for (s, d), f in use.items():
        b = use.get((d, s), 0)
        if f + b == 1:                                                                   # f == 1: the edge's one use is s -> d
            out[s] += 1
            inn[d] += 1
            heads.setdefault(s, []).append(d)
            n_boundary += 1
        elif not (f == 1 and b == 1):
            irregular |= {s, d}
    simple = {v for v in out if out[v] == 1 and inn[v] == 1 and v not in irregular}
    nxt = {v: heads[v][0] for v in simple}
    label, rank, loops, chain = {}, {}, [], set()
    for v in sorted(simple):
        if v in label or v in chain:
            continue
        walk, u = [v], nxt[v]
        while u != v and u in simple and len(walk) <= V:
            walk.append(u)
            u = nxt[u]
        if u == v:
            lo = min(walk)
            assert lo == v                                                               # ascending order: the first vertex met is the smallest
            for j, w in enumerate(walk):
                label[w], rank[w] = v, j
            loops.append(walk)
        else:
            chain.add(v)                                                                 # only v: the others of the walk are judged on their own walk
    touched = set(out) | set(inn)
    counts = [len(loops), len(label), n_boundary, len(touched - simple), len(chain), max((len(w) for w in loops), default=0), invalid, degenerate]
    return nxt, label, rank, loops, counts


def assert_same(triangles, V):
    got = H.boundary_loops(triangles, V)
    nxt, label, rank, loops, counts = plain_loops(triangles, V)
    assert [int(c) for c in got.counts] == counts
    for name, arr, d in (("next", got.vertex_next, nxt), ("loop", got.vertex_loop, label), ("rank", got.vertex_rank, rank)):
        want = np.full(V, NONE, np.uint32)
        if d:
            want[list(d)] = list(d.values())
        assert np.array_equal(arr, want), name
    assert got.loop_start.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in loops])]).astype(np.int64).tolist()
    assert got.loop_vertices.tolist() == [u for w in loops for u in w]
    assert (got.lengths >= 3).all()
    adj = S.adjacency(triangles, V)
    assert got.counts[2] == adj.counts[2] and got.counts[6] == adj.counts[5] and got.counts[7] == adj.counts[6]
    assert (adj.vertex_class[got.simple] == 2).all()                                     # every simple vertex has class 2; not the reverse
    return got


CASES = H.small_cases()


@pytest.mark.parametrize("name,V,t", CASES, ids=[c[0] for c in CASES])
def test_restatement_equals_the_plain_implementation_on_the_hand_made_cases(name, V, t):
    got = assert_same(t, V)
    expect = {"one triangle": [1, 3, 3, 0, 0, 3, 0, 0], "quad": [1, 4, 4, 0, 0, 4, 0, 0], "pinch": [0, 0, 6, 1, 4, 0, 0, 0],
              "annulus of 6": [2, 12, 12, 0, 0, 6, 0, 0], "tetrahedron": [0] * 8, "sphere hub pair": [0] * 8, "flipped fan": [0, 0, 8, 2, 6, 0, 0, 0],
              "grid of 5 disjoint triangles": [5, 15, 15, 0, 0, 3, 0, 0], "fan of 5": [1, 5, 5, 0, 0, 5, 0, 0]}
    if name in expect:
        assert got.counts.tolist() == expect[name]


@pytest.mark.parametrize("seed,n,V", [(1, 3000, 40), (2, 20000, 700), (3, 60000, 50000), (4, 2000, 1500)])
def test_restatement_equals_the_plain_implementation_on_soups(seed, n, V):
    v, t = S.soup(n, V, seed, p_bad=0.02, p_degenerate=0.05, p_reverse=0.3)
    got = assert_same(t, V)
    assert got.counts[6] > 0 and got.counts[7] > 0
    if V == 50000:
        assert got.counts[0] > 10 and got.counts[3] > 1000 and got.counts[4] > 1000       # loops, vertices that are not simple, open chains


@pytest.mark.parametrize("n", [3, 4, 5, 63, 64, 65, 257, 1024])
def test_renumberings_move_the_label_vertex_round_the_loop(n):
    V, base = H.polygon_fan(n)
    for where in ("first", "last", "mid"):
        V, t = H.fan_with_label_at(n, where)
        got = assert_same(t, V)
        assert got.lengths.tolist() == [n] and got.loop_vertices[0] == 0 and got.vertex_loop[n] == NONE        # the hub is on no loop
    for seed in range(3):
        perm = np.random.default_rng(100 * n + seed).permutation(V)
        got = assert_same(H.renumbered(V, base, perm)[1], V)
        rim = perm[1:]                                                                   # the fan's own walk 1, 2, .. n under the new names
        at = int(np.argmin(rim))
        assert got.loop_vertices.tolist() == np.roll(rim, -at).tolist()                  # the same cycle, started at its smallest index


def check_properties(vertices, triangles, max_edges):
    """Boundary edges fall by the sum of the filled L, irregular edges are unchanged, the Euler characteristic rises by one per filled
    loop, and filling the result again adds nothing -- for a mesh none of whose invalid triangles names an index in V .. V + F - 1, which
    the F new vertices would make valid (the input triangles go across as they are; test_an_invalid_triangle_that_names_a_new_vertex)."""
    V, T = len(vertices), len(triangles)
    lp = H.boundary_loops(triangles, V)
    f = H.fill_holes(vertices, triangles, max_edges, lp)
    filled = lp.lengths[lp.lengths <= max_edges]
    assert f.counts.tolist() == [V + len(filled), T + filled.sum(), len(filled), len(lp.lengths) - len(filled), filled.sum(), filled.max() if len(filled) else 0,
                                 lp.lengths[lp.lengths > max_edges].max() if len(filled) < len(lp.lengths) else 0, lp.counts[4]]
    assert np.array_equal(f.vertices[:V].view(np.uint32), np.asarray(vertices, F32).view(np.uint32)) and np.array_equal(f.triangles[:T], triangles)
    assert (f.vertex_src[:V] == np.arange(V)).all() and (f.vertex_src[V:] == NONE).all() and (f.vertices[V:, 3] == 0).all()
    before, after = S.adjacency(triangles, V), S.adjacency(f.triangles, len(f.vertices))
    tt = S._tri(triangles)
    if ((tt >= V) & (tt < len(f.vertices))).any():
        return lp, f, after
    assert after.counts[2] == before.counts[2] - filled.sum()
    assert after.counts[3] == before.counts[3]
    assert after.counts[5] == before.counts[5] and after.counts[6] == before.counts[6]
    if before.counts[6] == 0:
        assert S.euler(after, len(f.triangles)) == S.euler(before, T) + len(filled)
    und0, use0, fwd0 = R.edge_use(triangles[(S._tri(triangles) < V).all(1)])
    und1, use1, fwd1 = R.edge_use(f.triangles[(S._tri(f.triangles) < len(f.vertices)).all(1)])
    spokes = und1[und1[:, 1] >= V]
    assert len(spokes) == filled.sum() and (use1[und1[:, 1] >= V] == 2).all() and (fwd1[und1[:, 1] >= V] == 1).all()      # each spoke once each way
    again = H.fill_holes(f.vertices, f.triangles, max_edges)
    assert again.counts.tolist()[:5] == [len(f.vertices), len(f.triangles), 0, f.counts[3], 0]
    assert np.array_equal(again.triangles, f.triangles)
    return lp, f, after


def test_the_four_properties_on_hand_made_meshes_and_soups():
    for name, V, t in CASES:
        for max_edges in (0, 2, 3, 4, 6, 0xffffffff):
            check_properties(S.positions(V), t, max_edges)
    for seed, n, V in [(2, 20000, 700), (3, 60000, 50000)]:
        v, t = S.soup(n, V, seed, p_bad=0.02, p_degenerate=0.05, p_reverse=0.3)
        check_properties(v, t, 3)
        check_properties(v, t, 0xffffffff)


def test_an_invalid_triangle_that_names_a_new_vertex():
    """The input triangles go across as they are, so one that was invalid because it names V is a valid triangle on new vertex V after a
    fill.  The rule says so; the four properties are stated without such triangles."""
    t = S.tetrahedron()
    t[1, 0] = 4                                                                          # (4, 1, 3) over 4 vertices: invalid, a loop of 3 is left
    f = H.fill_holes(S.positions(4), t, 3)
    assert f.counts.tolist() == [5, 7, 1, 0, 3, 3, 0, 0] and np.array_equal(f.triangles[:4], t)
    assert S.adjacency(t, 4).counts[5] == 1 and S.adjacency(f.triangles, 5).counts[5] == 0 and S.adjacency(f.triangles, 5).counts[3] > 0
    t[1, 0] = 5                                                                          # names V + F: stays invalid, and the properties hold
    lp, f, after = check_properties(S.positions(4), t, 3)
    assert after.counts[5] == 1 and after.counts[2] == 0 and after.counts[3] == 0


def test_the_centroid_is_summed_in_rank_order():
    n = 200
    V, t = H.fan_with_label_at(n, "mid")
    rng = np.random.default_rng(17)
    v = np.zeros((V, 4), F32)
    v[:, :3] = (10.0 ** rng.uniform(-3.0, 3.0, (V, 3)) * rng.choice([-1.0, 1.0], (V, 3))).astype(F32)
    lp = H.boundary_loops(t, V)
    want = H.fill_holes(v, t, n, lp).vertices[V]
    acc = np.zeros(3, F32)
    u = 0
    for _ in range(n):                                                                   # from the label vertex along next
        acc = acc + v[u, :3]
        u = int(lp.vertex_next[u])
    assert u == 0 and np.array_equal((acc / F32(n)).view(np.uint32), want[:3].view(np.uint32)) and want[3] == 0
    for r in (1, n // 2, n - 1):
        assert (H.fill_holes(v, t, n, lp, start_rank=r).vertices[V].view(np.uint32) != want.view(np.uint32)).any()
    assert abs(float(want[0]) - v[lp.loop_vertices.astype(np.int64), 0].astype(np.float64).mean()) < 1e-3 * np.abs(v[:, 0]).max()


# ------------------------------------------------------------------------------------------------ the pinned figures
def figures(m):
    lp = assert_same(m.triangles, len(m.vertices))
    touched = int(((lp.out_deg + lp.in_deg) > 0).sum())
    return lp, [len(m.vertices), len(m.triangles), int(lp.counts[2]), touched, int(lp.counts[3]), int(lp.counts[0])]


def test_figures_of_the_extracted_meshes():
    cut = R.mesh_of("cut")
    lp, f, after = check_properties(cut.vertices, cut.triangles, 182)
    assert lp.lengths.tolist() == [182] and f.counts[2] == 1 and S.euler(after, len(f.triangles)) == 2 and after.counts[2] == 0
    assert H.fill_holes(cut.vertices, cut.triangles, 181, lp).counts[2] == 0
    hand = R.mesh_of("hand")
    assert sorted(H.loops_of("hand").lengths.tolist()) == [32, 32, 120]
    check_properties(hand.vertices, hand.triangles, 32)
    check_properties(hand.vertices, hand.triangles, 120)
    for name in ("sphere", "torus"):
        assert H.loops_of(name).counts.tolist() == [0] * 8
        m = R.mesh_of(name)
        assert np.array_equal(H.fill_holes(m.vertices, m.triangles, 0xffffffff, H.loops_of(name)).triangles, m.triangles)


def test_figures_of_the_scene_mesh():
    m = H.scene_mesh()
    lp, fig = figures(m)
    assert fig == [14575, 26932, 1402, 1384, 18, 44]
    assert sorted(lp.lengths.tolist())[-2:] == [296, 516] and ((lp.lengths >= 4) & (lp.lengths <= 20)).sum() == 42
    assert lp.counts[4] > 0                                                              # open chains
    lp, f, after = check_properties(m.vertices, m.triangles, 32)
    assert f.counts[2] == 42 and f.counts[3] == 2


def test_figures_of_the_noise_meshes():
    lp, fig = figures(H.noise_mesh(0.1))
    assert fig == [9676, 7884, 4456, 4386, 70, 133] and lp.counts[4] > 0                 # so the open-chain branch is reached
    m = H.noise_mesh(0.1)
    check_properties(m.vertices, m.triangles, 8)
    lp, fig = figures(H.noise_mesh(0.0))
    assert fig[2] == 2018 and fig[4] == 0 and fig[5] == 41
