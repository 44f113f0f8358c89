"""numpy restatement of the rules of dfusion_mesh_adjacency and dfusion_mesh_smooth (include/dfusion.h): which vertices are neighbours,
the CSR they come in, the classes of edges and vertices and the eight counts; the lambda | mu step with its f32 operations in the stated
order.  Nothing taken from the HIP source.  Also the meshes and helpers the smoothing tests share."""
import functools

import numpy as np

import mesh_ref as R

F32 = np.float32
FIX_BOUNDARY = 1                                                                         # DF_SMOOTH_FIX_BOUNDARY
COUNT_NAMES = ("csr_entries", "edges", "boundary_edges", "irregular_edges", "used_vertices", "invalid_triangles", "degenerate_triangles",
               "open_vertices")


def _tri(triangles):
    return np.asarray(triangles).reshape(-1, 3).astype(np.int64) & 0xffffffff           # uint32 bits, whatever the dtype


class Adjacency:
    pass


def adjacency(triangles, V):
    """-> Adjacency: row_start uint32 [V + 1], neighbours uint32 [2 E], vertex_class uint8 [V], counts uint64 [8]; beside them edges
    int64 [E, 2] (lo < hi, ascending), f and b int64 [E], edge_class uint8 [E] (1 interior, 2 boundary, 3 irregular)."""
    t = _tri(triangles)
    V = int(V)
    valid = (t < V).all(1)                                                              # tested before anything is indexed
    tv = t[valid]
    degenerate = (tv[:, 0] == tv[:, 1]) | (tv[:, 1] == tv[:, 2]) | (tv[:, 0] == tv[:, 2])
    he = np.concatenate([tv[:, [0, 1]], tv[:, [1, 2]], tv[:, [2, 0]]])                  # half-edges a -> b, b -> c, c -> a
    he = he[he[:, 0] != he[:, 1]]                                                       # leaving out those with equal ends
    lo, hi = he.min(1), he.max(1)
    ekey, inv = np.unique(lo.astype(np.uint64) << np.uint64(32) | hi.astype(np.uint64), return_inverse=True)
    inv = inv.reshape(-1)
    E = len(ekey)
    fwd = he[:, 0] < he[:, 1]
    f = np.bincount(inv[fwd], minlength=E).astype(np.int64)                             # lo -> hi
    b = np.bincount(inv[~fwd], minlength=E).astype(np.int64)                            # hi -> lo
    edges = np.stack([(ekey >> np.uint64(32)).astype(np.int64), (ekey & np.uint64(0xffffffff)).astype(np.int64)], 1).reshape(-1, 2)
    edge_class = np.full(E, 3, np.uint8)
    edge_class[(f == 1) & (b == 1)] = 1
    edge_class[f + b == 1] = 2
    both = np.concatenate([edges, edges[:, ::-1]])                                      # u is a neighbour of v and v of u
    both = both[np.lexsort((both[:, 1], both[:, 0]))]                                   # by vertex, ascending neighbour; each once
    degree = np.bincount(both[:, 0], minlength=V).astype(np.int64)
    vertex_class = (degree > 0).astype(np.uint8)
    vertex_class[edges[edge_class == 2].reshape(-1)] = 2
    vertex_class[edges[edge_class == 3].reshape(-1)] = 3
    out = Adjacency()
    out.row_start = np.concatenate([[0], np.cumsum(degree)]).astype(np.uint32)
    out.neighbours = both[:, 1].astype(np.uint32)
    out.vertex_class = vertex_class
    out.edges, out.f, out.b, out.edge_class = edges, f, b, edge_class
    out.counts = np.array([2 * E, E, (edge_class == 2).sum(), (edge_class == 3).sum(), (degree > 0).sum(), (~valid).sum(), degenerate.sum(),
                           (vertex_class >= 2).sum()], np.uint64)
    return out


def euler(adj, n_triangles):
    """The Euler characteristic of a mesh without degenerate triangles from its counts."""
    c = [int(x) for x in adj.counts]
    return c[4] - c[1] + (int(n_triangles) - c[5])


def step(P, row_start, neighbours, vertex_class, s, flags=FIX_BOUNDARY, descending=False):
    """One step with factor s: P f32 [V, 4] -> Q.  Vectorised by neighbour rank: for j = 0 .. max degree - 1 the j-th neighbour of every
    row that has one is added -- per vertex exactly the sequential f32 order of the rule.  descending: the rows summed from their last
    entry to their first (NOT the rule; for the test that shows the order matters)."""
    P = np.ascontiguousarray(P, F32).reshape(-1, 4)
    rs = np.asarray(row_start).astype(np.int64)
    nb = np.asarray(neighbours).astype(np.int64)
    V = len(P)
    d = rs[1:] - rs[:-1]
    cls = np.where(d > 0, 1, 0) if vertex_class is None else np.asarray(vertex_class)
    movable = (d > 0) & ((cls == 1) | (not (flags & FIX_BOUNDARY)))
    acc = np.zeros((V, 3), F32)
    with np.errstate(all="ignore"):
        for j in range(int(d.max()) if V else 0):
            rows = np.nonzero(d > j)[0]
            u = nb[rs[rows] + (d[rows] - 1 - j if descending else j)]
            acc[rows] = acc[rows] + P[u, :3]                                            # f32 adds, one after the other
        Q = P.copy()                                                                    # not movable: all 16 bytes; w as it is
        m = np.nonzero(movable)[0]
        mean = acc[m] / d[m].astype(F32)[:, None]                                       # IEEE f32 division
        delta = mean - P[m, :3]
        Q[m, :3] = P[m, :3] + F32(s) * delta                                            # a multiply, then an add
    return Q


def smooth(vertices, adj, iterations=10, lam=0.5, mu=-0.53, flags=FIX_BOUNDARY, use_class=True):
    """iterations of (a step with lam, then unless mu == 0 a step with mu) -> f32 [V, 4]."""
    P = np.ascontiguousarray(vertices, F32).reshape(-1, 4).copy()
    cls = adj.vertex_class if use_class else None
    for _ in range(int(iterations)):
        P = step(P, adj.row_start, adj.neighbours, cls, lam, flags)
        if mu != 0:
            P = step(P, adj.row_start, adj.neighbours, cls, mu, flags)
    return P


# ------------------------------------------------------------------------------------------------ quality measures (f64; not part of the rule)
def smallest_angles(vertices, triangles):
    """The smallest angle of every triangle, in degrees."""
    p = np.asarray(vertices)[:, :3].astype(np.float64)
    t = _tri(triangles)
    a, b, c = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]

    def angle(o, x, y):
        u, w = x - o, y - o
        cos = (u * w).sum(1) / np.maximum(np.linalg.norm(u, axis=1) * np.linalg.norm(w, axis=1), 1e-300)
        return np.degrees(np.arccos(np.clip(cos, -1, 1)))
    return np.minimum(np.minimum(angle(a, b, c), angle(b, c, a)), angle(c, a, b))


def radial(vertices, centre):
    """(mean radius, rms deviation of the radius about its mean) of the vertices about a centre."""
    r = np.linalg.norm(np.asarray(vertices)[:, :3].astype(np.float64) - np.asarray(centre, np.float64), axis=1)
    return float(r.mean()), float(np.sqrt(((r - r.mean()) ** 2).mean()))


# ------------------------------------------------------------------------------------------------ shared meshes
SPHERE_CENTRE = tuple(float(c) * float(R.VS[0]) for c in R.SPHERE_C)                    # mesh_ref's sphere, volume units


@functools.lru_cache(None)
def adjacency_of(name):
    """adjacency() of a mesh_ref mesh, once per process; shared, read-only."""
    m = R.mesh_of(name)
    return adjacency(m.triangles, len(m.vertices))


@functools.lru_cache(None)
def noisy_sphere():
    """The sphere's vertices with Gaussian noise of a quarter voxel planted on them; shared, read-only."""
    v = R.mesh_of("sphere").vertices.copy()
    v[:, :3] += (np.random.default_rng(7).standard_normal((len(v), 3)) * 0.25 * float(R.VS[0])).astype(F32)
    return v


def u3(rows):
    return np.array(rows, np.uint32).reshape(-1, 3)


def soup(n, V, seed, p_bad=0.0, p_degenerate=0.0, p_reverse=0.0, lo=-1.0, hi=1.0):
    """n random triangles over V random vertices: p_bad of the indices replaced by V, V + 7 or 0xffffffff, p_degenerate of the triangles
    given two equal corners (a tenth of those three), p_reverse of them a reversed or rotated copy of the triangle before.  Coordinates
    are +-10^uniform(lo, hi), w a normal draw."""
    rng = np.random.default_rng(seed)
    v = np.zeros((V, 4), F32)
    v[:, :3] = (10.0 ** rng.uniform(lo, hi, (V, 3)) * rng.choice([-1.0, 1.0], (V, 3))).astype(F32)
    v[:, 3] = rng.standard_normal(V)
    t = rng.integers(0, max(V, 1), (n, 3)).astype(np.uint32)
    if n > 1:
        rev = np.nonzero(rng.random(n) < p_reverse)[0]
        rev = rev[rev > 0]
        for i in rev:
            t[i] = t[i - 1][[[0, 2, 1], [1, 2, 0], [0, 1, 2]][int(rng.integers(0, 3))]]
    deg = rng.random(n) < p_degenerate
    t[deg, 1] = t[deg, 0]
    tri = deg & (rng.random(n) < 0.1)
    t[tri, 2] = t[tri, 0]
    bad = rng.random((n, 3)) < p_bad
    t[bad] = rng.choice(np.array([V, V + 7, 0xffffffff], np.uint32), int(bad.sum()))
    return v, t


def strip(n, seed=None):
    """A strip of n triangles over n + 2 vertices, one orientation along it; seed: the vertices renumbered by a random permutation."""
    V = n + 2
    perm = np.arange(V) if seed is None else np.random.default_rng(seed).permutation(V)
    i = np.arange(n)
    tri = np.stack([i, i + 1, i + 2], 1)
    tri[1::2] = tri[1::2][:, [1, 0, 2]]
    pos = np.zeros((V, 4), F32)
    j = np.arange(V)
    pos[perm, 0] = (j // 2) * 0.5 + 0.125 * (j % 3)
    pos[perm, 1] = (j % 2) * 1.0 + 0.25
    pos[perm, 2] = np.sin(j * 0.37)
    pos[:, 3] = 1.0
    return pos, perm[tri].astype(np.uint32)


def tetrahedron():
    return u3([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])


def positions(V, seed=3):
    v = np.zeros((V, 4), F32)
    rng = np.random.default_rng(seed)
    v[:, :3] = rng.uniform(-1, 1, (V, 3))
    v[:, 3] = rng.standard_normal(V)
    return v


def fan_on_one_edge(n):
    """n triangles (0, 1, 2 + i) on the edge {0, 1}, all in the same direction."""
    return np.stack([np.zeros(n, np.int64), np.ones(n, np.int64), 2 + np.arange(n)], 1).astype(np.uint32)


def hub(n):
    """A closed fan of n triangles around vertex 0: the hub has degree n, the rim vertices 3."""
    i = np.arange(n)
    return np.stack([np.zeros(n, np.int64), 1 + i, 1 + (i + 1) % n], 1).astype(np.uint32)


def double_hub(n):
    """Two hubs (vertices 0 and n + 1) on either side of one rim of n vertices: a closed surface of 2 n triangles over n + 2 vertices."""
    below = hub(n)[:, [0, 2, 1]].astype(np.int64)
    below[:, 0] = n + 1
    return np.concatenate([hub(n), below.astype(np.uint32)])


def small_cases():
    """[(name, V, triangles uint32 [T, 3])]: the hand-made cases every layer is checked on."""
    F = 0xffffffff
    flipped = tetrahedron()
    flipped[2] = flipped[2][[0, 2, 1]]
    cases = [
        ("no triangle", 6, u3([])),
        ("no vertex", 0, u3([[0, 1, 2], [3, 3, 3]])),
        ("one triangle", 3, u3([[0, 1, 2]])),
        ("one triangle and unused vertices", 9, u3([[7, 2, 4]])),
        ("two triangles on an edge", 4, u3([[0, 1, 2], [1, 0, 3]])),
        ("two triangles on an edge, same direction", 4, u3([[0, 1, 2], [0, 1, 3]])),
        ("the same triangle twice", 3, u3([[0, 1, 2], [0, 1, 2]])),
        ("a triangle and its reverse", 3, u3([[0, 1, 2], [2, 1, 0]])),
        ("a rotation is the same triangle", 3, u3([[0, 1, 2], [1, 2, 0]])),
        ("tetrahedron", 4, tetrahedron()),
        ("tetrahedron with one face flipped", 4, flipped),
        ("fan of three on one edge", 5, fan_on_one_edge(3)),
        ("(a, a, b)", 3, u3([[0, 0, 1], [1, 2, 2]])),
        ("(a, b, a)", 3, u3([[0, 1, 0]])),
        ("(a, a, a)", 3, u3([[1, 1, 1]])),
        ("(a, a, b) beside its edge's triangle", 3, u3([[0, 1, 2], [1, 1, 0]])),
        ("highest vertex only", 5, u3([[4, 4, 3]])),
    ]
    for slot in range(3):
        for bad in (4, F):                                                              # V itself and 0xffffffff, in each slot
            rows = tetrahedron().tolist()
            rows[1][slot] = bad
            cases.append(("index %#x in slot %d" % (bad, slot), 4, u3(rows)))
    for n in (1, 63, 64, 65, 255, 256, 257):
        cases.append(("soup of %d" % n, n, soup(n, n, 200 + n, p_bad=0.05, p_degenerate=0.1, p_reverse=0.2)[1]))
    return cases
