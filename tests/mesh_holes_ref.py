"""numpy restatement of the rules of dfusion_mesh_boundary_loops and dfusion_mesh_fill_holes (include/dfusion.h): the boundary
half-edges, which vertices are simple, the walk along next as plain Python, labels, ranks, the CSR of the loops and the eight counts;
the fan triangles and the centroid with its f32 operations in the stated order.  Nothing taken from the HIP source.  Also the meshes
the hole tests share."""
import functools

import numpy as np

import mesh_ref as R
import mesh_smooth_ref as S

F32 = np.float32
NONE = 0xffffffff
LOOP_COUNT_NAMES = ("loops", "loop_vertices", "boundary_half_edges", "other_boundary_vertices", "chain_vertices", "longest_loop",
                    "invalid_triangles", "degenerate_triangles")
FILL_COUNT_NAMES = ("vertices", "triangles", "loops_filled", "loops_open", "triangles_added", "longest_filled", "longest_open", "chain_vertices")


class Loops:
    pass


def boundary_loops(triangles, V):
    """-> Loops: vertex_next, vertex_loop, vertex_rank uint32 [V], loop_start uint32 [loops + 1], loop_vertices uint32, counts uint64 [8];
    beside them simple bool [V], out_deg and in_deg int64 [V] and lengths int64 [loops]."""
    t = S._tri(triangles)
    V = int(V)
    valid = (t < V).all(1)                                                              # tested before anything is indexed
    tv = t[valid]
    degenerate = (tv[:, 0] == tv[:, 1]) | (tv[:, 1] == tv[:, 2]) | (tv[:, 0] == tv[:, 2])
    he = np.concatenate([tv[:, [0, 1]], tv[:, [1, 2]], tv[:, [2, 0]]])                  # half-edges a -> b, b -> c, c -> a
    he = he[he[:, 0] != he[:, 1]]                                                       # leaving out those with equal ends
    lo, hi = he.min(1), he.max(1)
    ekey, inv, uses = np.unique(lo.astype(np.uint64) << np.uint64(32) | hi.astype(np.uint64), return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    fwd = he[:, 0] < he[:, 1]
    f = np.bincount(inv[fwd], minlength=len(ekey))
    b = np.bincount(inv[~fwd], minlength=len(ekey))
    boundary = f + b == 1
    irregular = ~boundary & ~((f == 1) & (b == 1))
    bh = he[boundary[inv]]                                                              # the boundary half-edges
    out_deg = np.bincount(bh[:, 0], minlength=V).astype(np.int64)
    in_deg = np.bincount(bh[:, 1], minlength=V).astype(np.int64)
    on_irregular = np.zeros(V, bool)
    on_irregular[(ekey[irregular] >> np.uint64(32)).astype(np.int64)] = True
    on_irregular[(ekey[irregular] & np.uint64(0xffffffff)).astype(np.int64)] = True
    simple = (out_deg == 1) & (in_deg == 1) & ~on_irregular
    nxt = np.full(V, NONE, np.int64)
    leaving_simple = simple[bh[:, 0]]
    nxt[bh[leaving_simple, 0]] = bh[leaving_simple, 1]

    label = np.full(V, NONE, np.int64)
    rank = np.full(V, NONE, np.int64)
    state = np.zeros(V, np.int8)                                                        # 0 not walked, 1 on a loop, 2 on an open chain
    loops = []
    for v in np.nonzero(simple)[0].tolist():                                            # ascending: the first vertex met of a loop is its label
        if state[v]:
            continue
        walk, u = [v], int(nxt[v])
        while simple[u] and u != v and not state[u]:
            walk.append(u)
            u = int(nxt[u])
        if u == v:                                                                      # back at v having met only simple vertices
            assert len(walk) >= 3, "a loop of %d vertices" % len(walk)                  # 2 would make the edge interior
            state[walk] = 1
            label[walk] = v
            rank[walk] = np.arange(len(walk))
            loops.append(walk)
        else:                                                                           # ended at a vertex that is not simple, or ran into a chain
            assert not simple[u] or state[u] == 2                                       # (next is injective: a walk cannot run into a loop)
            state[walk] = 2
    assert (state[simple] != 0).all()

    out = Loops()
    out.vertex_next = nxt.astype(np.uint32)
    out.vertex_loop = label.astype(np.uint32)
    out.vertex_rank = rank.astype(np.uint32)
    out.lengths = np.array([len(w) for w in loops], np.int64)
    out.loop_start = np.concatenate([[0], np.cumsum(out.lengths)]).astype(np.uint32)
    out.loop_vertices = np.array([u for w in loops for u in w], np.uint32)
    out.simple, out.out_deg, out.in_deg = simple, out_deg, in_deg
    out.counts = np.array([len(loops), (state == 1).sum(), len(bh), (~simple & (out_deg + in_deg > 0)).sum(), (state == 2).sum(),
                           out.lengths.max() if len(loops) else 0, (~valid).sum(), degenerate.sum()], np.uint64)
    return out


class Filled:
    pass


def fill_holes(vertices, triangles, max_edges, loops=None, start_rank=0):
    """-> Filled: vertices f32 [V + F, 4], triangles uint32 [T + A, 3], vertex_src uint32 [V + F], counts uint64 [8].  start_rank: the
    centroid summed from the vertex of that rank on (NOT the rule; for the test that shows the order matters)."""
    P = np.ascontiguousarray(vertices, F32).reshape(-1, 4)
    t = np.asarray(triangles).reshape(-1, 3).astype(np.uint32)
    V, T = len(P), len(t)
    lp = boundary_loops(t, V) if loops is None else loops
    new_v, new_t, filled, left = [], [], [], []
    for i, L in enumerate(lp.lengths.tolist()):
        if L > int(max_edges):
            left.append(L)
            continue
        w = lp.loop_vertices[lp.loop_start[i]:lp.loop_start[i + 1]].astype(np.int64)
        m = V + len(filled)
        filled.append(L)
        acc = np.zeros(3, F32)
        with np.errstate(all="ignore"):
            for j in range(L):
                acc = acc + P[w[(j + start_rank) % L], :3]                              # f32 adds, one after the other, in rank order
            centre = acc / F32(L)                                                       # IEEE f32 division
        new_v.append([centre[0], centre[1], centre[2], F32(0)])
        new_t.append(np.stack([np.roll(w, -1), w, np.full(L, m)], 1))                   # triangle j = (v_(j+1) mod L, v_j, m)
    out = Filled()
    out.vertices = np.concatenate([P, np.array(new_v, F32).reshape(-1, 4)])
    out.triangles = np.concatenate([t] + [x.astype(np.uint32) for x in new_t]).reshape(-1, 3)
    out.vertex_src = np.concatenate([np.arange(V), np.full(len(filled), NONE)]).astype(np.uint32)
    added = int(sum(filled))
    out.counts = np.array([V + len(filled), T + added, len(filled), len(left), added, max(filled, default=0), max(left, default=0),
                           lp.counts[4]], np.uint64)
    return out


# ------------------------------------------------------------------------------------------------ hand-made meshes
def polygon_fan(n):
    """n triangles (hub, 1 + i, 1 + (i + 1) % n) around vertex 0: one loop of the n rim vertices."""
    return n + 1, S.hub(n)


def annulus(n):
    """A ring of 2 n triangles between an inner and an outer polygon of n vertices each: two loops of n."""
    i = np.arange(n)
    j = (i + 1) % n
    return 2 * n, np.concatenate([np.stack([i, j, n + i], 1), np.stack([j, n + j, n + i], 1)]).astype(np.uint32)


def pinch():
    """Two triangles meeting in vertex 0 only: out(0) == in(0) == 2, so no loop and two open chains of two simple vertices."""
    return 5, S.u3([[0, 1, 2], [0, 3, 4]])


def flipped_fan(n):
    """polygon_fan(n) with triangle 1 reversed: its two spokes are used twice in one direction (irregular)."""
    V, t = polygon_fan(n)
    t = t.copy()
    t[1] = t[1][[0, 2, 1]]
    return V, t


def disjoint_triangles(n):
    """n triangles over 3 n vertices, no two sharing one: n loops of 3."""
    return 3 * n, np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def renumbered(V, triangles, perm):
    """The same mesh with vertex v called perm[v]."""
    return V, np.asarray(perm)[S._tri(triangles)].astype(np.uint32)


def fan_with_label_at(n, where):
    """polygon_fan(n) renumbered: the hub becomes vertex n, and the rim, along the walk from the label vertex 0, is numbered
    "first" 0, 1, 2, .. n - 1 (the smallest index of a window that does not wrap is its first vertex), "last" 0, n - 1, n - 2, .. 1 (it
    is its last vertex: every doubling round merges), "mid" at random, with vertex 0 half way round the fan's own numbering."""
    V, t = polygon_fan(n)
    if where == "first":
        rim = np.arange(n)
    elif where == "last":
        rim = (n - np.arange(n)) % n
    else:
        rim = np.empty(n, np.int64)
        rim[n // 2] = 0
        rim[np.arange(n) != n // 2] = 1 + np.random.default_rng(n).permutation(n - 1)
    return renumbered(V, t, np.concatenate([[n], rim]))


def positions(V, seed=3):
    return S.positions(V, seed)


def small_cases():
    """[(name, V, triangles uint32 [T, 3])]: the hand-made cases every layer is checked on."""
    cases = [(name, V, t) for name, V, t in S.small_cases()]
    cases += [("fan of %d" % n,) + polygon_fan(n) for n in (3, 4, 5, 7)]
    cases += [("annulus of 6",) + annulus(6), ("pinch",) + pinch(), ("flipped fan",) + flipped_fan(8), ("quad", 4, S.u3([[0, 1, 2], [0, 2, 3]])),
              ("grid of 5 disjoint triangles",) + disjoint_triangles(5), ("sphere hub pair", 12, S.double_hub(10))]
    for where in ("first", "last", "mid"):
        cases.append(("fan of 9, label %s" % where,) + fan_with_label_at(9, where))
    return cases


# ------------------------------------------------------------------------------------------------ shared extracted meshes
@functools.lru_cache(None)
def scene_mesh():
    """The mesh of mesh_ref.scene_small() (64^3, two fused frames); shared, read-only."""
    from dynamicfusion_amd import synth
    sc, ref = R.scene_small()
    return R.extract_mesh(ref, sc.cfg.dims, sc.vs, synth.aff12(R.rotated_pose()))


@functools.lru_cache(None)
def noise_mesh(p_invalid):
    """The mesh of noise_volume((16, 16, 16), 5, p_invalid) under ANISO_VS; shared, read-only."""
    dims = (16, 16, 16)
    return R.extract_mesh(R.noise_volume(dims, 5, p_invalid), dims, R.ANISO_VS, R.POSE)


@functools.lru_cache(None)
def loops_of(name):
    m = R.mesh_of(name)
    return boundary_loops(m.triangles, len(m.vertices))
