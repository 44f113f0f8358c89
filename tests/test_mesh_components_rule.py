"""The rule of dfusion_mesh_components / dfusion_mesh_filter (include/dfusion.h), checked on its numpy restatement
tests/mesh_components_ref.py: against a plain breadth-first search, against scipy's connected components, and on the numbers of the
shared meshes.  No GPU: tests/test_gpu_mesh_components.py then pins the HIP kernels to the restatement."""
import numpy as np
import pytest

import mesh_components_ref as M
import mesh_ref as R


def check_against_bfs(tri, V):
    label, count, counts = M.components(tri, V)
    want = M.bfs_labels(tri, V)
    assert label.dtype == np.uint32 and (label == want).all()
    ok = M.valid_triangles(tri, V)
    t = tri.reshape(-1, 3)[ok].astype(np.int64)
    assert (count == np.bincount(want[t[:, 0]], minlength=V)).all()
    used = np.zeros(V, bool)
    used[t.reshape(-1)] = True
    assert [int(c) for c in counts] == [int((count > 0).sum()), int((~used).sum()), int((~ok).sum()), int(count.max()) if V else 0]
    assert (count[label != np.arange(V)] == 0).all()                 # only labels have triangles
    return label, count, counts


@pytest.mark.parametrize("name,tri,V", M.small_cases(), ids=[c[0] for c in M.small_cases()])
def test_restatement_equals_breadth_first_search(name, tri, V):
    check_against_bfs(tri, V)


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_strips_are_one_component(order):
    tri, V = M.strip(500, order)
    label, count, counts = check_against_bfs(tri, V)
    assert (label == 0).all() and [int(c) for c in counts] == [1, 0, 0, 500]


def test_hand_made_cases_say_what_the_rule_says():
    cases = {c[0]: c[1:] for c in M.small_cases()}
    label, count, counts = M.components(*cases["aab"])
    assert list(label) == [0, 1, 2, 1, 4, 2, 6, 7, 7, 9] and count[2] == 1 and count[7] == 1 and count[1] == 1
    label, count, counts = M.components(*cases["aaa"])
    assert list(label) == [0, 1, 2, 3, 4, 5, 4, 4] and count[4] == 2 and count[2] == 1       # (a, a, a) connects nothing, counts for a
    assert [int(c) for c in counts] == [2, 4, 0, 2]
    assert [int(c) for c in M.components(*cases["no triangle"])[2]] == [0, 5, 0, 0]
    assert [int(c) for c in M.components(*cases["no vertex"])[2]] == [0, 0, 2, 0]
    label, count, counts = M.components(*cases["index 0x6 in slot 1"])
    assert list(label) == [0, 0, 0, 3, 3, 3] and [int(c) for c in counts] == [2, 0, 1, 2]
    for name in ("two equal", "two equal, larger label first"):                              # the tie goes to the smaller label
        tri, V = cases[name]
        label, count, _ = M.components(tri, V)
        assert count[0] == count[5] == 2 and M.largest_label(count) == 0
        out, src, vmap, n = M.mesh_filter(tri, V, label, count, keep_largest=True)
        assert list(src) == [0, 1, 2, 3] and out.tolist() == [[0, 1, 2], [1, 2, 3]] and [int(c) for c in n] == [4, 2]
        assert list(vmap[:4]) == [0, 1, 2, 3] and (vmap[4:] == M.NONE).all()


def scipy_labels(tri, V):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    t = tri.reshape(-1, 3)[M.valid_triangles(tri, V)].astype(np.int64)
    i = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    j = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    n, comp = connected_components(sp.coo_matrix((np.ones(len(i)), (i, j)), shape=(V, V)), directed=False)
    smallest = np.full(n, V, np.int64)
    np.minimum.at(smallest, comp, np.arange(V))
    return smallest[comp].astype(np.uint32)


COMMITTED = ["sphere", "torus", "planted", ("fuzz", 9, 0.1), ("fuzz", 8, 0.1), ("fuzz", 0, 0.1)]


@pytest.mark.parametrize("name", COMMITTED, ids=str)
def test_restatement_equals_scipy_on_the_committed_meshes(name):
    pytest.importorskip("scipy")
    m, label, _, _ = M.components_of(name)
    assert (label == scipy_labels(m.triangles, len(m.vertices))).all()


def summary(name):
    m, label, count, counts = M.components_of(name)
    return len(m.vertices), len(m.triangles), [int(c) for c in counts], sorted(int(c) for c in count[count > 0])


def test_numbers_of_the_committed_meshes():
    assert summary("sphere") == (4980, 9956, [1, 0, 0, 9956], [9956])
    assert summary("torus") == (9412, 18824, [1, 0, 0, 18824], [18824])
    assert summary("planted") == (5370, 10724, [4, 0, 0, 9956], [24, 144, 600, 9956])
    V, T, counts, _ = summary(("fuzz", 9, 0.1))
    assert (V, T, counts) == (7825, 5980, [87, 3004, 0, 3742])
    V, T, counts, _ = summary(("fuzz", 8, 0.1))
    assert counts == [87, 3611, 0, 4976]
    assert summary(("fuzz", 0, 0.1)) == (3, 0, [0, 3, 0, 0], [])


def assert_closed_oriented(vertices, triangles, euler):
    """tests/test_mesh_rule.py's check: every edge in exactly two triangles, once in each direction; the Euler characteristic; no
    vertex unreferenced, no index out of range."""
    und, use, fwd = R.edge_use(triangles)
    assert (use == 2).all() and (fwd == 1).all()
    V, E, F = len(vertices), len(und), len(triangles)
    assert V - E + F == euler, (V, E, F)
    assert len(np.unique(triangles)) == V
    assert triangles.max() < V


@pytest.mark.parametrize("min_triangles,pieces", list(zip(M.PLANTED_THRESHOLDS, (4, 3, 3, 2, 0))))
def test_planted_sphere_thresholds(min_triangles, pieces):
    m, label, count, _ = M.components_of("planted")
    V = len(m.vertices)
    out, src, vmap, n = M.mesh_filter(m.triangles, V, label, count, min_triangles)
    sizes = M.PLANTED_SIZES[4 - pieces:]
    assert len(out) == sum(sizes) == int(n[1]) and len(src) == int(n[0])
    if not pieces:
        assert len(src) == 0 and (vmap == M.NONE).all()
        return
    assert sorted(int(c) for c in M.components(out, len(src))[1] if c) == list(sizes)
    assert_closed_oriented(m.vertices[src], out, 2 * pieces)                            # closed spheres, each of Euler characteristic 2
    assert (np.diff(src.astype(np.int64)) > 0).all() and (vmap[src] == np.arange(len(src))).all()
    kept = M.kept_triangles(m.triangles, V, label, count, min_triangles)
    assert (src[out] == m.triangles[kept]).all()                                        # the same triangles, in the same order


def test_planted_sphere_keep_largest_is_the_sphere():
    m, label, count, _ = M.components_of("planted")
    verts, out, src = M.remove_small(m.vertices, m.triangles, keep_largest=True)
    sphere = R.mesh_of("sphere")
    assert len(src) == 4980 and (out == sphere.triangles).all()
    assert verts.tobytes() == sphere.vertices.tobytes()
    assert_closed_oriented(verts, out, 2)
    # keep_largest and a threshold hold together
    assert len(M.mesh_filter(m.triangles, len(m.vertices), label, count, 9957, keep_largest=True)[0]) == 0
