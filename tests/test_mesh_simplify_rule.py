"""The rule of dfusion_mesh_simplify (include/dfusion.h), checked on its numpy restatement tests/mesh_simplify_ref.py: against an
independent dict-and-loop implementation written here, and by the properties the rule is what it is for -- a closed oriented surface
stays closed and keeps its Euler characteristic.  No GPU: tests/test_gpu_mesh_simplify.py then pins the HIP kernels to the restatement
bit for bit."""
import math

import numpy as np
import pytest

import mesh_ref as R
import mesh_simplify_ref as S

F32 = np.float32
KF, KD = S.KEEP_FIRST, S.KEEP_DUPLICATES


# ------------------------------------------------------------------------------------------------ the rule once more, with dicts and loops
def loops(vertices, triangles, cell, flags=0):
    vertices = np.asarray(vertices, F32).reshape(-1, 4)
    tris = [[int(i) & 0xffffffff for i in row] for row in np.asarray(triangles).reshape(-1, 3).tolist()]
    V, cellf = len(vertices), F32(cell)
    place = {}

    def where(v):
        if v not in place:
            cs, qs = [], []
            for a in range(3):
                with np.errstate(all="ignore"):
                    t = F32(vertices[v, a]) / cellf
                if not abs(t) < F32(2.0 ** 30):
                    cs = None
                    break
                fl = F32(math.floor(t))
                cs.append(int(fl))
                qs.append(int(F32(F32(t - fl) * F32(16777216.0))))
            place[v] = (tuple(cs), qs) if cs is not None else None
        return place[v]

    counts = dict.fromkeys(S.COUNT_NAMES, 0)
    valid, bad_vertices = [], set()
    for i, row in enumerate(tris):
        if max(row) >= V:
            counts["invalid"] += 1
            continue
        bad = [v for v in row if where(v) is None]
        bad_vertices.update(bad)
        if bad:
            counts["invalid"] += 1
        else:
            valid.append(i)
    counts["unclusterable"] = len(bad_vertices)
    clusters = {}                                                                        # cell -> [src, n, [Sx, Sy, Sz]]
    for v in sorted({v for i in valid for v in tris[i]}):
        c, q = where(v)
        k = clusters.setdefault(c, [v, 0, [0, 0, 0]])
        k[1] += 1
        for a in range(3):
            k[2][a] += q[a]
    counts["clusters"] = len(clusters)
    name = lambda v: clusters[where(v)[0]][0]                                            # a cluster is named by its src
    groups, kept = {}, []
    for i in valid:
        a, b, c = (name(v) for v in tris[i])
        if a == b or b == c or a == c:
            counts["collapsed"] += 1
        elif flags & KD:
            kept.append(i)
        else:
            even = (a, b, c) in (tuple(sorted((a, b, c))[r:] + sorted((a, b, c))[:r]) for r in range(3))
            groups.setdefault(tuple(sorted((a, b, c))), ([], []))[0 if even else 1].append(i)
    for P, N in groups.values():
        if len(P) == len(N):
            counts["fin"] += len(P) + len(N)
        else:
            kept.append(min(P if len(P) > len(N) else N))
            counts["duplicate"] += len(P) + len(N) - 1
    kept.sort()
    used = sorted({name(v) for i in kept for v in tris[i]})
    new = {s: j for j, s in enumerate(used)}
    out_v = np.zeros((len(used), 4), F32)
    for j, s in enumerate(used):
        c, (_, n, sums) = where(s)[0], clusters[where(s)[0]]
        if flags & KF:
            out_v[j] = vertices[s]
        else:
            with np.errstate(over="ignore"):
                out_v[j, :3] = [F32((float(c[a]) + (float(sums[a]) / float(n)) * 2.0 ** -24) * float(cellf)) for a in range(3)]
    out_t = np.array([[new[name(v)] for v in tris[i]] for i in kept], np.uint32).reshape(-1, 3)
    vmap = np.full(V, S.NONE, np.uint32)
    for v in {v for i in valid for v in tris[i]}:
        vmap[v] = new.get(name(v), 0xffffffff)
    counts["vertices"], counts["triangles"] = len(used), len(kept)
    return out_v, out_t, np.array(used, np.uint32), vmap, np.array([counts[k] for k in S.COUNT_NAMES], np.uint64)


def same(got, want):
    v, t, src, vmap, counts = want
    assert np.array_equal(got.counts, counts), (got.counts, counts)
    assert got.vertices.tobytes() == v.tobytes() and np.array_equal(got.triangles, t)
    assert np.array_equal(got.vertex_src, src) and np.array_equal(got.vertex_map, vmap)
    assert got.vertices.dtype == F32 and got.triangles.dtype == np.uint32 and got.vertex_src.dtype == np.uint32


@pytest.mark.parametrize("flags", [0, KF, KD, KF | KD])
@pytest.mark.parametrize("name,factor", [("sphere", 1.0), ("sphere", 4.0), ("torus", 2.0), ("noise", 0.5), ("noise", 2.0)])
def test_restatement_equals_the_loops_on_extracted_meshes(name, factor, flags):
    m = S.mesh_named(name)
    cell = factor * S.median_edge(name)
    same(S.simplify(m.vertices, m.triangles, cell, flags), loops(m.vertices, m.triangles, cell, flags))


@pytest.mark.parametrize("flags", [0, KF, KD, KF | KD])
def test_restatement_equals_the_loops_on_hand_made_cases_and_soups(flags):
    for name, v, t, cell in S.small_cases():
        same(S.simplify(v, t, cell, flags), loops(v, t, cell, flags))
    for seed, (n, V, cell) in enumerate([(3000, 400, 0.3), (3000, 2000, 0.11), (500, 3000, 0.05)]):
        v, t = S.soup(n, V, seed, p_bad=0.02)
        v[::97, 1] = np.nan
        v[5::131, 2] = -np.inf
        got = S.simplify(v, t, cell, flags)
        same(got, loops(v, t, cell, flags))
        assert got.counts[2] and got.counts[7] and (flags & KD or got.counts[5] or V > 400)


# ------------------------------------------------------------------------------------------------ closed surfaces stay closed
def topology(triangles, n_vertices):
    """-> (every directed edge a -> b is matched by exactly one b -> a, every undirected edge is used twice, Euler characteristic)."""
    und, use, fwd = R.edge_use(triangles)
    return bool((2 * fwd == use).all()), bool((use == 2).all()), n_vertices - len(und) + len(triangles)


# what the restatement gives at 1, 2 and 4 median edge lengths (6.65 mm on the sphere, 6.64 mm on the torus)
PINNED = {("sphere", 1): (2695, 5386), ("sphere", 2): (1018, 2032), ("sphere", 4): (296, 588),
          ("torus", 1): (5139, 10280), ("torus", 2): (1931, 3862), ("torus", 4): (542, 1084)}


@pytest.mark.parametrize("name,factor", sorted(PINNED))
def test_sphere_and_torus_stay_closed_oriented_surfaces(name, factor):
    m = R.mesh_of(name)
    assert topology(m.triangles[(m.triangles[:, [0, 1, 2]] != m.triangles[:, [1, 2, 0]]).all(1)], len(m.vertices))[0]      # the input is balanced
    got = S.simplified(name, factor * S.median_edge(name))
    balanced, all_twice, euler = topology(got.triangles, len(got.vertices))
    assert balanced
    assert all_twice or name == "torus"
    assert euler == {"sphere": 2, "torus": 0}[name]
    assert (len(got.vertices), len(got.triangles)) == PINNED[name, factor]
    assert got.counts[2] == 0 and got.counts[7] == 0 and got.counts[1:6].sum() == len(m.triangles)     # every triangle is accounted for once
    # the representative lies in its cluster's cell (or on its upper faces, by the last rounding)
    cell = F32(factor * S.median_edge(name))
    _, c, _ = S.cells(m.vertices[got.vertex_src], cell)
    lo = c * np.float64(cell)
    assert ((got.vertices[:, :3] >= lo.astype(F32)) & (got.vertices[:, :3] <= (lo + np.float64(cell)).astype(F32))).all() and (got.vertices[:, 3] == 0).all()


@pytest.mark.parametrize("name,factor", sorted(PINNED))
def test_collapsing_alone_keeps_the_surface_balanced(name, factor):
    got = S.simplified(name, factor * S.median_edge(name), KD)
    ruled = S.simplified(name, factor * S.median_edge(name))
    assert topology(got.triangles, len(got.vertices))[0]
    assert got.counts[4] == 0 and got.counts[5] == 0 and got.counts[3] == ruled.counts[3] and got.counts[6] == ruled.counts[6]
    assert len(got.triangles) == len(ruled.triangles) + ruled.counts[4] + ruled.counts[5] and len(got.vertices) >= len(ruled.vertices)


def test_plain_duplicate_removal_would_not_do():
    """Why fins cancel: keeping one triangle of every group, whatever its orientations, leaves the sphere unbalanced."""
    name, factor = "sphere", 2
    got = S.simplified(name, factor * S.median_edge(name), KD)
    first = np.unique(np.sort(got.triangles, 1), axis=0, return_index=True)[1]
    assert not topology(got.triangles[np.sort(first)], len(got.vertices))[0]
    assert S.simplified(name, factor * S.median_edge(name)).counts[4] > 0


# ------------------------------------------------------------------------------------------------ keep_first
TINY = 1e-6                                                              # far below the smallest vertex spacing of either mesh


def test_keep_first_at_a_tiny_cell_returns_the_sphere_unchanged():
    m = R.mesh_of("sphere")
    got = S.simplified("sphere", TINY, KF)
    used = np.unique(m.triangles)
    assert np.array_equal(got.vertex_src, used) and got.vertices.tobytes() == m.vertices[used].tobytes()
    assert np.array_equal(got.vertex_src[got.triangles], m.triangles)
    assert got.counts.tolist() == [len(used), len(m.triangles), 0, 0, 0, 0, len(used), 0]


def coincident(m):
    p, t = m.vertices[:, :3], m.triangles.astype(np.int64)
    return (p[t[:, 0]] == p[t[:, 1]]).all(1) | (p[t[:, 1]] == p[t[:, 2]]).all(1) | (p[t[:, 0]] == p[t[:, 2]]).all(1)


def test_keep_first_at_a_tiny_cell_on_the_torus_and_the_noise_mesh():
    """The torus, like the sphere, has no two vertices at one position (its shortest edge is 3.4e-6): nothing collapses, nothing
    changes.  The noise mesh has: 545 of its triangles have two corners at one position and 31 more two corners within the cell;
    those 576 collapse, and the corners are welded."""
    m = R.mesh_of("torus")
    got = S.simplified("torus", TINY, KF)
    assert coincident(m).sum() == 0 and got.counts.tolist() == [9412, 18824, 0, 0, 0, 0, 9412, 0]
    assert got.vertices.tobytes() == m.vertices.tobytes() and np.array_equal(got.triangles, m.triangles)
    m = S.noise_mesh()
    got = S.simplified("noise", TINY, KF)
    assert coincident(m).sum() == 545 and got.counts.tolist() == [4377, 5404, 0, 576, 0, 0, 4379, 0] and len(m.triangles) == 5980
    p = got.vertices[:, :3]
    assert len(np.unique(p, axis=0)) == len(p) and not coincident(got).any()             # welded: one vertex a position
    assert got.vertices.tobytes() == m.vertices[got.vertex_src].tobytes()


@pytest.mark.parametrize("flags", [KF, KF | KD])
@pytest.mark.parametrize("name,factor", [("sphere", 2), ("torus", 1), ("noise", 1)])
def test_keep_first_is_idempotent(name, factor, flags):
    cell = factor * S.median_edge(name)
    once = S.simplified(name, cell, flags)
    twice = S.simplify(once.vertices, once.triangles, cell, flags)
    assert twice.vertices.tobytes() == once.vertices.tobytes() and np.array_equal(twice.triangles, once.triangles)
    assert np.array_equal(twice.vertex_src, np.arange(len(once.vertices))) and twice.counts[2:6].sum() == 0


# ------------------------------------------------------------------------------------------------ hand-made cases, by what they are for
CASES = {c[0]: c[1:] for c in S.small_cases()}


def run(name, flags=0):
    v, t, cell = CASES[name]
    return S.simplify(v, t, cell, flags)


def test_fins_cancel_and_the_larger_side_keeps_its_lowest_triangle():
    got = run("fin pair")
    assert got.counts.tolist() == [0, 0, 0, 0, 2, 0, 3, 0] and (got.vertex_map == S.NONE).all()
    assert run("fin pair", KD).counts.tolist() == [3, 2, 0, 0, 0, 0, 3, 0]
    got = run("fin pair beside a triangle")
    assert got.kept.tolist() == [2] and got.vertex_src.tolist() == [0, 1, 6] and got.vertex_map.tolist() == [0, 1, 0xffffffff, 0, 1, 0xffffffff, 2]
    got = run("three against one")
    assert got.kept.tolist() == [1] and got.counts.tolist() == [3, 1, 0, 0, 0, 3, 3, 0] and got.triangles.tolist() == [[0, 1, 2]]
    got = run("one against three")
    assert got.kept.tolist() == [1] and got.triangles.tolist() == [[2, 1, 0]]
    assert run("two against two").counts.tolist() == [0, 0, 0, 0, 4, 0, 3, 0]
    got = run("rotations are duplicates")
    assert got.kept.tolist() == [0] and got.triangles.tolist() == [[1, 2, 0]] and got.counts[5] == 3        # in its original rotation
    got = run("two in one cell")
    assert got.counts.tolist() == [3, 1, 0, 1, 0, 0, 3, 0] and got.kept.tolist() == [1]
    assert run("all in one cell").counts.tolist() == [0, 0, 0, 2, 0, 0, 1, 0]


def test_cells_floor_and_zero_signs():
    v, t, cell = CASES["on the cell faces"]
    ok, c, q = S.cells(v, cell)
    assert ok.all() and c.tolist() == [[0, 2, 4], [-2, -4, 6], [1, 0, -2], [0, 2, 5], [0, 0, 0], [0, 0, 0], [6, 0, 0]]      # k * cell opens cell k
    assert (q[[0, 1, 4, 5, 6]] == 0).all() and q[2].tolist() == [0, 1 << 23, 1 << 23]
    got = run("on the cell faces")
    assert got.counts.tolist() == [4, 2, 0, 0, 2, 0, 6, 0]                               # +0 and -0 share a cell: (4, 1, 6) and (5, 6, 1) are a fin
    dup = run("on the cell faces", KD)
    assert dup.vertex_map[4] == dup.vertex_map[5] == 4 and dup.vertex_src.tolist() == [0, 1, 2, 3, 4, 6]
    assert got.vertices[:, :3].tolist()[:2] == [[0.0, 1.0, 2.0], [-1.0, -2.0, 3.0]]
    v, t, cell = CASES["negative coordinates"]
    ok, c, q = S.cells(v, cell)
    assert c.tolist() == [[-1, -1, -1], [-2, -1, -1], [-1, -2, -1], [0, 0, 0], [-1, -1, -1], [-1, -1, -1]]                   # floor, not truncation
    assert q[0].tolist() == [3 << 22] * 3 and q[5].tolist() == [1 << 24, 1 << 24, 1]     # a fraction that rounds to 1 stays in its cell
    got = run("negative coordinates")
    assert got.counts[6] == 4 and got.vertex_map[0] == got.vertex_map[4] == got.vertex_map[5]


def test_the_limit_of_2_to_the_30_cells():
    got = run("just below 2^30")
    assert got.counts.tolist() == [4, 2, 0, 0, 0, 0, 4, 0]
    assert got.vertices[0, :2].tolist() == [float(2 ** 30 - 64), -float(2 ** 30 - 64)]
    for name in CASES:
        if name.startswith("at 2^30"):
            got = run(name)
            assert got.counts.tolist() == [6, 2, 2, 0, 0, 0, 6, 1] and got.vertex_map[6] == S.NONE, name
    assert run("cell scales 2^30").counts.tolist() == [0, 0, 2, 0, 0, 0, 0, 3]


def test_nan_and_inf_vertices_and_indices_past_the_end():
    for bad in ("nan", "inf", "-inf"):
        got = run("vertex %s" % bad)
        assert got.counts.tolist() == [4, 2, 2, 0, 2, 0, 6, 2] and got.kept.tolist() == [0, 5] and got.vertex_src.tolist() == [0, 1, 2, 4]
        assert np.isfinite(got.vertices).all()
    for name in CASES:
        if name.startswith("index"):
            got = run(name)
            assert got.counts.tolist() == [6, 2, 1, 0, 0, 1, 6, 0] and got.kept.tolist() == [0, 2], name           # (4, 5, 3) is (3, 4, 5) rotated
    assert run("no vertex").counts.tolist() == [0, 0, 2, 0, 0, 0, 0, 0]
    assert run("no triangle").counts.tolist() == [0] * 8 and (run("no triangle").vertex_map == S.NONE).all()


def test_sums_are_64_bit():
    v = np.zeros((70000, 4), F32)
    v[:, :3] = F32(1.0) - F32(2.0 ** -24)                                                # q = 2^24 - 1 on every axis
    t = np.stack([np.arange(70000), np.roll(np.arange(70000), 1), np.roll(np.arange(70000), 2)], 1).astype(np.uint32)
    got = S.simplify(v, t, 1.0)
    assert got.counts.tolist() == [0, 0, 0, 70000, 0, 0, 1, 0] and 70000 * ((1 << 24) - 1) > 1 << 32
    v2 = np.concatenate([v, S.v4([[1.5, 0.5, 0.5], [0.5, 1.5, 0.5]])])
    got = S.simplify(v2, np.concatenate([t, S.u3([[69999, 70000, 70001]])]), 1.0)
    assert got.counts.tolist() == [3, 1, 0, 70000, 0, 0, 3, 0] and got.vertices[0, :3].tolist() == [float(F32(1.0) - F32(2.0 ** -24))] * 3
