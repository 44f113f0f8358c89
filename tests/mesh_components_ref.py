"""numpy restatement of the rule of dfusion_mesh_components / dfusion_mesh_filter (include/dfusion.h): which triangles are valid, what
connects, what a label is, what is kept and in which order.  Integers only; iterated minimum propagation with pointer jumping, nothing
taken from the HIP source and no scipy.  Also the meshes the component tests share."""
import functools

import numpy as np

import mesh_ref as R

NONE = np.uint32(0xffffffff)


def _tri(triangles):
    return np.asarray(triangles).reshape(-1, 3).astype(np.int64) & 0xffffffff           # uint32 bits, whatever the dtype


def valid_triangles(triangles, V):
    """bool per triangle: all three indices are < V."""
    return (_tri(triangles) < V).all(1)


def components(triangles, V):
    """-> (vertex_label uint32 [V], triangle_count uint32 [V], counts uint64 [4]) by the rule."""
    t = _tri(triangles)
    ok = (t < V).all(1)
    tv = t[ok]
    label = np.arange(V, dtype=np.int64)
    while True:
        before = label.copy()
        if len(tv):
            seen = label[tv]
            m = seen.min(1)                                                             # the smallest label a triangle sees ...
            for c in range(3):
                np.minimum.at(label, seen[:, c], m)                                     # ... goes to the labels of its three vertices
                np.minimum.at(label, tv[:, c], m)                                       # (members of the same component) and to them
        while True:                                                                     # pointer jumping: label[v] <= v always
            nxt = label[label]
            if (nxt == label).all():
                break
            label = nxt
        if (label == before).all():
            break
    count = np.bincount(label[tv[:, 0]], minlength=V).astype(np.int64) if V else np.zeros(0, np.int64)
    used = np.zeros(V, bool)
    used[tv.reshape(-1)] = True
    counts = np.array([(count > 0).sum(), (~used).sum(), (~ok).sum(), count.max() if V else 0], np.uint64)
    return label.astype(np.uint32), count.astype(np.uint32), counts


def largest_label(triangle_count):
    """The label of the component with the most triangles; an exact tie goes to the smaller label."""
    return int(np.argmax(triangle_count)) if len(triangle_count) else 0                 # (argmax returns the FIRST maximum)


def kept_triangles(triangles, V, label, triangle_count, min_triangles=0, keep_largest=False):
    t = _tri(triangles)
    keep = (t < V).all(1)
    lab = np.zeros(len(t), np.int64)
    lab[keep] = label[t[keep, 0]]
    if V:
        keep &= triangle_count.astype(np.int64)[lab] >= int(min_triangles)
    if keep_largest:
        keep &= lab == largest_label(triangle_count)
    return keep


def mesh_filter(triangles, V, label, triangle_count, min_triangles=0, keep_largest=False):
    """-> (triangles_out uint32 [m, 3] with the new indices, vertex_src uint32 [n], vertex_map uint32 [V], counts uint64 [2])."""
    t = _tri(triangles)
    keep = kept_triangles(t, V, label, triangle_count, min_triangles, keep_largest)
    tk = t[keep]
    vkeep = np.zeros(V, bool)
    vkeep[tk.reshape(-1)] = True
    vertex_src = np.nonzero(vkeep)[0].astype(np.uint32)                                 # ascending: the kept vertices keep their order
    vertex_map = np.full(V, NONE, np.uint32)
    vertex_map[vertex_src] = np.arange(len(vertex_src), dtype=np.uint32)
    out = vertex_map[tk].astype(np.uint32).reshape(-1, 3)
    return out, vertex_src, vertex_map, np.array([len(vertex_src), len(out)], np.uint64)


def remove_small(vertices, triangles, min_triangles=0, keep_largest=False):
    """-> (vertices[vertex_src], triangles_out, vertex_src): the filtered mesh of a (vertices, triangles) pair."""
    V = len(vertices)
    label, count, _ = components(triangles, V)
    out, src, _, _ = mesh_filter(triangles, V, label, count, min_triangles, keep_largest)
    return vertices[src], out, src


def bfs_labels(triangles, V):
    """The labels by a plain breadth-first search over adjacency lists (the check of `components` on small cases)."""
    t = _tri(triangles)
    adj = [[] for _ in range(V)]
    for a, b, c in t[(t < V).all(1)].tolist():
        adj[a] += [b, c]; adj[b] += [a, c]; adj[c] += [a, b]
    label = [-1] * V
    for s in range(V):                                                                  # ascending: s is the smallest of what it reaches
        if label[s] >= 0:
            continue
        label[s] = s
        queue = [s]
        while queue:
            nxt = []
            for u in queue:
                for w in adj[u]:
                    if label[w] < 0:
                        label[w] = s
                        nxt.append(w)
            queue = nxt
    return np.array(label, np.int64).astype(np.uint32)


# ------------------------------------------------------------------------------------------------ shared meshes
PLANTED_BALLS = (((5.0, 5.0, 5.0), 1.3), ((27.0, 26.0, 6.0), 2.2), ((4.5, 27.5, 27.5), 0.9))      # centre, radius in voxel units
PLANTED_THRESHOLDS = (24, 25, 144, 145, 9957)
PLANTED_SIZES = (24, 144, 600, 9956)


@functools.lru_cache(None)
def planted_volume():
    """The sphere volume of mesh_ref with three balls planted away from it."""
    d = R.sphere_dist(R.SPHERE_DIMS, R.SPHERE_C, R.SPHERE_R)
    for c, r in PLANTED_BALLS:
        d = np.minimum(d, R.sphere_dist(R.SPHERE_DIMS, c, r))
    return R.pack(d)


@functools.lru_cache(None)
def planted_mesh():
    """The restatement's mesh of planted_volume(); shared, read-only."""
    return R.extract_mesh(planted_volume(), R.SPHERE_DIMS, R.VS, R.IDENT)


@functools.lru_cache(None)
def components_of(name):
    """(mesh, label, count, counts) of "planted", a mesh_ref.mesh_of name, or ("fuzz", index, p_invalid); shared, read-only."""
    m = planted_mesh() if name == "planted" else R.fuzz_case(name[1], name[2])[1] if isinstance(name, tuple) else R.mesh_of(name)
    return (m,) + components(m.triangles, len(m.vertices))


def soup(n, V, seed, p_bad=0.0):
    """n random triangles over V vertices; p_bad of the indices replaced by V, V + 7 or 0xffffffff."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, V, (n, 3)).astype(np.uint32)
    bad = rng.random((n, 3)) < p_bad
    t[bad] = rng.choice(np.array([V, V + 7, 0xffffffff], np.uint32), int(bad.sum()))
    return t


def small_cases():
    """[(name, triangles uint32 [T, 3], V)]: the hand-made cases every layer is checked on."""
    u = lambda rows: np.array(rows, np.uint32).reshape(-1, 3)
    F = 0xffffffff
    cases = [("no triangle", u([]), 5), ("no vertex", u([[0, 1, 2], [3, 3, 3]]), 0), ("one triangle", u([[4, 2, 6]]), 9),
             ("aab", u([[5, 5, 2], [7, 8, 8], [1, 3, 1]]), 10), ("aaa", u([[4, 4, 4], [4, 6, 7], [2, 2, 2]]), 8),
             ("two equal", u([[5, 6, 7], [6, 7, 8], [0, 1, 2], [1, 2, 3], [9, 9, 9]]), 11),
             ("two equal, larger label first", u([[0, 1, 2], [5, 6, 7], [6, 7, 8], [1, 2, 3]]), 9)]
    for slot in range(3):
        for bad in (6, F):                                                              # V itself and 0xffffffff, in each slot
            rows = [[0, 1, 2], [2, 3, 4], [3, 4, 5], [4, 5, 3]]
            rows[1][slot] = bad                                                         # cuts 0-1-2 from 3-4-5
            cases.append(("index %#x in slot %d" % (bad, slot), u(rows), 6))
    for n in (63, 64, 65, 255, 256, 257):
        cases.append(("soup of %d" % n, soup(n, 2 * n, 100 + n, p_bad=0.05), 2 * n))
    t, V = islands(7, 3)
    cases.append(("islands", t, V))
    return cases


def strip(n, order="ascending", seed=0):
    """A strip of n triangles over n + 2 vertices, (i, i + 1, i + 2) in the strip's own numbering; `order` renumbers the vertices."""
    V = n + 2
    perm = {"ascending": np.arange(V), "descending": np.arange(V)[::-1], "shuffled": np.random.default_rng(seed).permutation(V)}[order]
    i = np.arange(n)
    return perm[np.stack([i, i + 1, i + 2], 1)].astype(np.uint32), V


def islands(n_components, n_triangles):
    """n_components separate fans of exactly n_triangles triangles each (n_triangles + 2 vertices a piece), interleaved in the
    triangle list so that no wave holds one component only."""
    per = n_triangles + 2
    base = (np.arange(n_components) * per)[None, :, None]                                # [1, C, 1]
    k = np.arange(n_triangles)[:, None, None]                                            # [n, 1, 1]
    fan = np.concatenate([np.zeros_like(k), k + 1, k + 2], 2)                            # (0, k + 1, k + 2)
    return (fan + base).reshape(-1, 3).astype(np.uint32), n_components * per
