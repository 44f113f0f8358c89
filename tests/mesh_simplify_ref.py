"""numpy restatement of the rule of dfusion_mesh_simplify (include/dfusion.h): which vertices cluster, what a cluster's representative
is, which triangles are kept, collapsed, cancelled as fins or dropped as duplicates, and in which order everything comes out.  f32
division and subtraction as numpy does them (IEEE), integer sums, f64 positions; nothing taken from the HIP source.  Also the meshes the
simplification tests share."""
import functools

import numpy as np

import mesh_ref as R

F32 = np.float32
NONE = np.uint32(0xffffffff)
KEEP_FIRST, KEEP_DUPLICATES = 1, 2                                                       # DF_SIMPLIFY_*
COUNT_NAMES = ("vertices", "triangles", "invalid", "collapsed", "fin", "duplicate", "clusters", "unclusterable")


def _tri(triangles):
    return np.asarray(triangles).reshape(-1, 3).astype(np.int64) & 0xffffffff           # uint32 bits, whatever the dtype


def cells(vertices, cell):
    """-> (clusterable bool [V], cell int64 [V, 3], q uint64 [V, 3]: the 24-bit fraction inside the cell); 0 where not clusterable."""
    p = np.asarray(vertices, F32).reshape(-1, 4)[:, :3]
    with np.errstate(all="ignore"):
        t = p / F32(cell)                                                               # IEEE f32 division
        ok = (np.abs(t) < F32(2.0 ** 30)).all(1)                                        # NaN and inf fail
        t = np.where(ok[:, None], t, F32(0))
        fl = np.floor(t)
        f = (t - fl).astype(F32)                                                        # IEEE f32 subtraction, in [0, 1]
        q = (f * F32(16777216.0)).astype(np.uint64)                                     # exact scaling, truncated
    return ok, fl.astype(np.int64), q


def _group_rows(rows):
    """rows int64 [n, 3] -> (group number of every row, number of groups); equal rows share a number."""
    n = len(rows)
    if not n:
        return np.zeros(0, np.int64), 0
    order = np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))
    s = rows[order]
    first = np.ones(n, bool)
    first[1:] = (s[1:] != s[:-1]).any(1)
    g = np.cumsum(first) - 1
    inv = np.empty(n, np.int64)
    inv[order] = g
    return inv, int(g[-1]) + 1


class Simplified:
    pass


def simplify(vertices, triangles, cell, flags=0):
    """-> Simplified: vertices f32 [n, 4], triangles uint32 [m, 3], vertex_src uint32 [n], vertex_map uint32 [V], counts uint64 [8];
    kept (the input indices of the kept triangles) beside them."""
    vertices = np.ascontiguousarray(vertices, F32).reshape(-1, 4)
    t = _tri(triangles)
    V = len(vertices)
    inb = (t < V).all(1)                                                                # tested before anything is indexed
    ok, c, q = cells(vertices, cell)
    valid = inb.copy()
    valid[inb] = ok[t[inb]].all(1)
    tv = t[valid]
    member = np.zeros(V, bool)
    member[tv.reshape(-1)] = True
    touched = np.zeros(V, bool)
    touched[t[inb].reshape(-1)] = True
    mi = np.nonzero(member)[0]
    inv, K = _group_rows(c[mi])                                                         # clusters: the members of one cell
    src = np.full(K, V, np.int64)
    np.minimum.at(src, inv, mi)
    n = np.bincount(inv, minlength=K).astype(np.int64)
    S = np.zeros((K, 3), np.uint64)
    np.add.at(S, inv, q[mi])                                                            # unsigned 64-bit sums
    cell_of = np.zeros((K, 3), np.int64)
    cell_of[inv] = c[mi]
    cl = np.full(V, -1, np.int64)                                                       # a cluster is named by its src
    cl[mi] = src[inv]
    # triangles
    tc = cl[tv].reshape(-1, 3)
    distinct = (tc[:, 0] != tc[:, 1]) & (tc[:, 1] != tc[:, 2]) & (tc[:, 0] != tc[:, 2])
    ti = np.nonzero(valid)[0][distinct]
    tcd = tc[distinct]
    n_fin = n_dup = 0
    if flags & KEEP_DUPLICATES:
        kept = ti
    else:
        ginv, G = _group_rows(np.sort(tcd, 1))                                          # groups: the unordered cluster triple
        even = ((tcd[:, 0] > tcd[:, 1]).astype(int) + (tcd[:, 1] > tcd[:, 2]) + (tcd[:, 0] > tcd[:, 2])) % 2 == 0
        P, N = np.bincount(ginv[even], minlength=G), np.bincount(ginv[~even], minlength=G)
        big = np.int64(1) << 40
        min_p, min_n = np.full(G, big), np.full(G, big)
        np.minimum.at(min_p, ginv[even], ti[even])
        np.minimum.at(min_n, ginv[~even], ti[~even])
        fin = P == N
        n_fin = int((P + N)[fin].sum())
        kept = np.sort(np.where(P > N, min_p, min_n)[~fin])                             # original order
        n_dup = int((P + N)[~fin].sum()) - len(kept)
    ck = cl[t[kept]].reshape(-1, 3)
    vertex_src = np.unique(ck)                                                          # ascending src
    new = np.full(V, NONE, np.uint32)
    new[vertex_src] = np.arange(len(vertex_src), dtype=np.uint32)
    out = Simplified()
    out.kept = kept
    out.triangles = new[ck].astype(np.uint32).reshape(-1, 3)
    out.vertex_src = vertex_src.astype(np.uint32)
    out.vertex_map = np.full(V, NONE, np.uint32)
    out.vertex_map[mi] = new[cl[mi]]
    if flags & KEEP_FIRST:
        out.vertices = vertices[vertex_src].copy()
    else:
        k_of = np.full(V, -1, np.int64)
        k_of[src] = np.arange(K)
        k = k_of[vertex_src]
        m = S[k].astype(np.float64) / n[k].astype(np.float64)[:, None]
        with np.errstate(over="ignore"):
            pos = ((cell_of[k].astype(np.float64) + m * 2.0 ** -24) * np.float64(F32(cell))).astype(F32)
        out.vertices = np.zeros((len(k), 4), F32)
        out.vertices[:, :3] = pos
    out.counts = np.array([len(vertex_src), len(kept), (~valid).sum(), (~distinct).sum(), n_fin, n_dup, K, (touched & ~ok).sum()], np.uint64)
    return out


# ------------------------------------------------------------------------------------------------ shared meshes
@functools.lru_cache(None)
def noise_mesh():
    """The mesh of the 24 x 11 x 13 noise volume (mesh_ref.FUZZ_DIMS[9], a tenth of it invalid); shared, read-only."""
    return R.fuzz_case(9, 0.1)[1]


def mesh_named(name):
    return noise_mesh() if name == "noise" else R.mesh_of(name)


@functools.lru_cache(None)
def median_edge(name):
    """The median edge length of a mesh_ref mesh over its non-degenerate edges, in f64."""
    m = mesh_named(name)
    p = m.vertices[:, :3].astype(np.float64)
    t = m.triangles.astype(np.int64)
    e = np.concatenate([p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 1]], p[t[:, 0]] - p[t[:, 2]]])
    length = np.sqrt((e * e).sum(1))
    return float(np.median(length[length > 0]))


@functools.lru_cache(None)
def simplified(name, cell, flags=0):
    """simplify() of a named mesh, once per process; shared, read-only."""
    m = mesh_named(name)
    return simplify(m.vertices, m.triangles, cell, flags)


def v4(rows):
    a = np.zeros((len(rows), 4), F32)
    if len(rows):
        a[:, :3] = np.array(rows, F32).reshape(-1, 3)
    return a


def u3(rows):
    return np.array(rows, np.uint32).reshape(-1, 3)


def soup(n, V, seed, extent=1.0, p_bad=0.0):
    """n random triangles over V random vertices in [-extent, extent]^3; p_bad of the indices replaced by V, V + 7 or 0xffffffff."""
    rng = np.random.default_rng(seed)
    v = np.zeros((V, 4), F32)
    v[:, :3] = rng.uniform(-extent, extent, (V, 3))
    v[:, 3] = rng.standard_normal(V)                                                    # w is carried by KEEP_FIRST only
    t = rng.integers(0, max(V, 1), (n, 3)).astype(np.uint32)
    bad = rng.random((n, 3)) < p_bad
    t[bad] = rng.choice(np.array([V, V + 7, 0xffffffff], np.uint32), int(bad.sum()))
    return v, t


def strip(n, order="ascending", seed=0):
    """A strip of n triangles, two vertices a unit step, numbered along it; `order` renumbers the vertices."""
    V = n + 2
    perm = {"ascending": np.arange(V), "descending": np.arange(V)[::-1], "shuffled": np.random.default_rng(seed).permutation(V)}[order]
    i = np.arange(n)
    tri = np.stack([i, i + 1, i + 2], 1)
    tri[1::2] = tri[1::2][:, [1, 0, 2]]                                                 # one orientation along the strip
    pos = np.zeros((V, 4), F32)
    j = np.arange(V)
    pos[perm, 0] = (j // 2) * 0.5 + 0.125
    pos[perm, 1] = (j % 2) * 1.0 + 0.25
    return pos, perm[tri].astype(np.uint32)


def small_cases():
    """[(name, vertices f32 [V, 4], triangles uint32 [T, 3], cell)]: the hand-made cases every layer is checked on."""
    F = 0xffffffff
    # six vertices in six cells of size 1 -- a, b, c and d, e, f; triangles over them
    six = v4([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.5, 0.5, 1.5], [1.5, 1.5, 0.5], [1.5, 0.5, 1.5]])
    # the same three cells twice: vertices 0-2 and 3-5 pairwise share a cell
    twin = v4([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.25, 0.75, 0.5], [1.75, 0.25, 0.25], [0.125, 1.5, 0.875]])
    cases = [
        ("no triangle", six, u3([]), 1.0),
        ("no vertex", v4([]), u3([[0, 1, 2], [3, 3, 3]]), 1.0),
        ("one triangle", six, u3([[0, 1, 2]]), 1.0),
        ("all in one cell", six, u3([[0, 1, 2], [3, 4, 5]]), 8.0),
        ("two in one cell", twin, u3([[0, 3, 1], [0, 1, 2]]), 1.0),
        ("fin pair", twin, u3([[0, 1, 2], [3, 5, 4]]), 1.0),
        ("fin pair beside a triangle", np.concatenate([twin, v4([[2.5, 2.5, 2.5]])]), u3([[0, 1, 2], [5, 4, 3], [0, 1, 6]]), 1.0),
        ("three against one", twin, u3([[2, 1, 0], [0, 1, 2], [4, 5, 3], [3, 4, 5]]), 1.0),
        ("one against three", twin, u3([[0, 1, 2], [2, 1, 0], [5, 4, 3], [1, 0, 5]]), 1.0),
        ("two against two", twin, u3([[0, 1, 2], [2, 1, 0], [4, 5, 3], [3, 5, 4]]), 1.0),
        ("rotations are duplicates", twin, u3([[1, 2, 0], [2, 0, 1], [0, 1, 2], [5, 3, 4]]), 1.0),
        ("on the cell faces", v4([[0.0, 1.0, 2.0], [-1.0, -2.0, 3.0], [0.5, 0.25, -0.75], [-0.0, 1.0, 2.5], [0.0, -0.0, 0.0], [-0.0, 0.0, -0.0],
                                  [3.0, 0.0, 0.0]]),
         u3([[0, 1, 2], [3, 1, 2], [4, 1, 6], [5, 6, 1]]), 0.5),
        ("negative coordinates", v4([[-0.25, -0.25, -0.25], [-1.25, -0.5, -0.75], [-0.5, -1.5, -0.25], [0.25, 0.25, 0.25], [-0.75, -0.75, -0.5],
                                     [-1e-30, -3e-9, -0.99999994]]),
         u3([[0, 1, 2], [3, 1, 2], [4, 2, 1], [5, 3, 1]]), 1.0),
    ]
    lim = float(2 ** 30)
    below = float(np.nextafter(F32(lim), F32(0)))
    cases.append(("just below 2^30", v4([[below, -below, 0.5], [below - 128, 0.5, -below], [0.5, below, below - 64], [0.5, 0.5, 0.5]]),
                  u3([[0, 1, 2], [0, 2, 3]]), 1.0))
    for axis in range(3):
        for sign in (1.0, -1.0):
            p = [0.5, 0.5, 0.5]
            p[axis] = sign * lim
            cases.append(("at 2^30 on axis %d sign %+d" % (axis, sign), np.concatenate([six, v4([p])]), u3([[0, 1, 2], [3, 6, 4], [6, 6, 6], [3, 4, 5]]), 1.0))
    cases.append(("cell scales 2^30", v4([[0.5, 0.25, 0.125], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]) * F32(2.0 ** 20),
                  u3([[0, 1, 2], [1, 2, 3]]), float(2.0 ** -10)))
    for bad in (np.nan, np.inf, -np.inf):
        w = np.concatenate([six, v4([[0.5, bad, 0.5], [bad, bad, bad]])])
        cases.append(("vertex %r" % bad, w, u3([[0, 1, 2], [6, 3, 4], [3, 4, 7], [3, 4, 5], [5, 4, 3], [1, 2, 4]]), 1.0))
    for slot in range(3):
        for bad in (6, F):                                                              # V itself and 0xffffffff, in each slot
            rows = [[0, 1, 2], [2, 3, 4], [3, 4, 5], [4, 5, 3]]
            rows[1][slot] = bad
            cases.append(("index %#x in slot %d" % (bad, slot), six, u3(rows), 1.0))
    for n in (1, 63, 64, 65, 255, 256, 257):
        v, t = soup(n, n, 100 + n, p_bad=0.05)
        cases.append(("soup of %d" % n, v, t, 0.25))
    return cases
