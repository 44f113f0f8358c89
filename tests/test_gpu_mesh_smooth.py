"""dfusion_mesh_adjacency, dfusion_mesh_smooth and their Python mirrors against the numpy restatement tests/mesh_smooth_ref.py: every
output array and all eight counts, bit for bit, through the C-ABI into guarded buffers."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mesh_ref as R
import mesh_smooth_ref as S
from dynamicfusion_amd import capi, mesh_adjacency, mesh_ops, mesh_topology, smooth_mesh
from mesh_gpu import ptr, same_bits, same_or_both_nan, stream, u32

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID = 100001
GUARD = 4                                            # guard rows behind every output
G32, G8 = -7, 0xa5                                   # what they hold
FIX = S.FIX_BOUNDARY
GRID_CAP = 2048 * 256                                # DF_MESH_MAX_BLOCKS workgroups of 256 lanes: past it a lane takes a second element
ITERATIONS = (0, 1, 2, 5)


class Mesh:
    """A mesh on the device, uploaded once for all the calls made on it, with the restatement's adjacency."""

    def __init__(self, v, t, V=None):
        self.t = np.ascontiguousarray(t, np.uint32).reshape(-1, 3)
        self.V = len(v) if V is None else V
        self.v = S.positions(self.V) if v is None else np.ascontiguousarray(v, F32).reshape(-1, 4)
        self.T = len(self.t)
        self.td = torch.from_numpy(self.t.view(np.int32)).cuda()
        self.vd = torch.from_numpy(self.v).cuda()
        self.adj = S.adjacency(self.t, self.V)
        self.rows_d = torch.from_numpy(self.adj.row_start.view(np.int32)).cuda()
        self.nbr_d = torch.from_numpy(self.adj.neighbours.view(np.int32)).cuda()
        self.cls_d = torch.from_numpy(self.adj.vertex_class).cuda()


def raw_adjacency(m, cap, with_rows=True, with_class=True):
    """One dfusion_mesh_adjacency call into guarded buffers -> (row_start, neighbours, vertex_class) device tensors, guards included, and
    the counts."""
    rows = torch.full((m.V + 1 + GUARD,), G32, dtype=torch.int32, device="cuda")
    nbr = torch.full((cap + GUARD,), G32, dtype=torch.int32, device="cuda")
    cls = torch.full((m.V + GUARD,), G8, dtype=torch.uint8, device="cuda")
    counts = torch.full((8 + GUARD,), 123, dtype=torch.int64, device="cuda")
    capi.check(capi.lib().dfusion_mesh_adjacency(ptr(m.td) if m.T else None, m.T, m.V, ptr(rows) if with_rows else None, ptr(nbr) if cap else None, cap,
                                                 ptr(cls) if with_class and m.V else None, ptr(counts), stream()), "dfusion_mesh_adjacency")
    torch.cuda.synchronize()
    assert (rows[m.V + 1:] == G32).all() and (nbr[cap:] == G32).all() and (cls[m.V:] == G8).all() and (counts[8:] == 123).all()
    assert with_rows or (rows == G32).all()
    assert with_class or (cls == G8).all()
    return rows, nbr, cls, counts[:8].cpu().numpy().astype(np.uint64)


def check_adjacency(m):
    """Capacity 0, then the exact capacity: everything equals the restatement."""
    want = m.adj
    rows, nbr, cls, n = raw_adjacency(m, 0)
    assert np.array_equal(n, want.counts), (n, want.counts)
    assert np.array_equal(u32(rows[:m.V + 1]), want.row_start) and np.array_equal(cls[:m.V].cpu().numpy(), want.vertex_class)
    cap = int(n[0])
    rows, nbr, cls, n = raw_adjacency(m, cap)
    assert np.array_equal(n, want.counts), (n, want.counts)
    assert np.array_equal(u32(rows[:m.V + 1]), want.row_start)
    assert np.array_equal(u32(nbr[:cap]), want.neighbours), int((u32(nbr[:cap]) != want.neighbours).sum())
    assert np.array_equal(cls[:m.V].cpu().numpy(), want.vertex_class)
    return want


def raw_smooth(m, iterations, lam=0.5, mu=-0.53, flags=FIX, with_class=True, in_place=False):
    """One dfusion_mesh_smooth call over the restatement's adjacency into a guarded buffer -> the smoothed vertices as uint32 [V, 4]."""
    out = torch.full((m.V + GUARD, 4), G32, dtype=torch.int32, device="cuda")
    if in_place:
        out[:m.V] = m.vd.view(torch.int32)
    nn = int(m.nbr_d.shape[0])
    capi.check(capi.lib().dfusion_mesh_smooth((ptr(out) if in_place else ptr(m.vd)) if m.V else None, m.V, ptr(m.rows_d), ptr(m.nbr_d) if nn else None, nn,
                                              ptr(m.cls_d) if with_class and m.V else None, iterations, lam, mu, flags, ptr(out) if m.V else None,
                                              stream()), "dfusion_mesh_smooth")
    torch.cuda.synchronize()
    assert (out[m.V:] == G32).all()
    return u32(out[:m.V])


def check_smooth(m, iterations=ITERATIONS, lam=0.5, mu=-0.53, flags=FIX, with_class=True, in_place=False):
    """The restatement after each of the iteration counts (ascending), computed incrementally, against one call each."""
    P, done, last = m.v.copy(), 0, None
    for it in iterations:
        P = S.smooth(P, m.adj, it - done, lam, mu, flags, use_class=with_class)
        done = it
        got = raw_smooth(m, it, lam, mu, flags, with_class, in_place)
        assert np.array_equal(got, P.view(np.uint32)), (it, int((got != P.view(np.uint32)).any(1).sum()))
        last = P
    return last


# ------------------------------------------------------------------------------------------------ hand-made cases and wave boundaries
CASES = S.small_cases()


@pytest.mark.parametrize("name,V,t", CASES, ids=[c[0] for c in CASES])
def test_small_cases(name, V, t):
    m = Mesh(None, t, V)
    want = check_adjacency(m)
    if name == "fan of three on one edge":
        assert want.counts[3] == 1 and want.vertex_class.tolist() == [3, 3, 2, 2, 2]
    if name == "tetrahedron with one face flipped":
        assert want.counts[3] == 3
    for flags in (0, FIX):
        check_smooth(m, flags=flags)
    check_smooth(m, mu=0.0, flags=0)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_strips_of_t_triangles_and_fans_over_v_vertices(n):
    m = Mesh(*S.strip(n, seed=n))                                        # T = n
    check_adjacency(m)
    check_smooth(m, flags=0)
    if n >= 4:
        m = Mesh(None, S.hub(n - 1), n)                                  # V = n
        check_adjacency(m)
        check_smooth(m)


@pytest.mark.parametrize("seed,n,V", [(1, 3000, 40), (2, 20000, 700), (3, 60000, 50000)])
def test_soups_with_duplicate_reversed_invalid_and_degenerate_triangles(seed, n, V):
    v, t = S.soup(n, V, seed, p_bad=0.02, p_degenerate=0.05, p_reverse=0.3)
    m = Mesh(v, t)
    want = check_adjacency(m)
    assert want.counts[5] > n // 40 and want.counts[6] > n // 40 and want.counts[3] > n // 20 and (V == 40 or want.counts[2] > 0)
    assert V != 40 or want.counts[1] == 40 * 39 // 2                    # few vertices: every pair is an edge, used many times
    check_smooth(m, flags=0)
    check_smooth(m, iterations=(2,))


def test_an_edge_shared_by_3000_triangles():
    m = Mesh(None, S.fan_on_one_edge(3000), 3002)
    want = check_adjacency(m)
    assert want.counts.tolist() == [2 * 6001, 6001, 6000, 1, 3002, 0, 0, 3002] and want.f[0] == 3000 and want.b[0] == 0
    both = Mesh(None, np.concatenate([S.fan_on_one_edge(1500), S.fan_on_one_edge(1500)[:, [1, 0, 2]]]), 1502)
    want = check_adjacency(both)
    assert want.f[0] == 1500 and want.b[0] == 1500 and want.counts[3] == 1
    check_smooth(m, flags=0)


def test_a_hub_vertex_of_degree_5000():
    m = Mesh(None, S.hub(5000), 5001)
    want = check_adjacency(m)
    assert want.row_start[1] == 5000 and want.counts.tolist() == [20000, 10000, 5000, 0, 5001, 0, 0, 5000]
    check_smooth(m, flags=0)                                             # the hub sums 5000 neighbours in their order
    closed = Mesh(None, S.double_hub(5000), 5002)
    want = check_adjacency(closed)                                       # a second hub below the same rim: closed, every vertex moves
    assert want.counts[2] == 0 and want.counts[3] == 0 and S.euler(want, 10000) == 2
    check_smooth(closed)


@functools.lru_cache(None)
def extracted(name):
    m = R.mesh_of(name)
    return Mesh(m.vertices, m.triangles)


@pytest.mark.parametrize("name", ["sphere", "torus", "cut", "hand"])
def test_extracted_meshes(name):
    m = extracted(name)
    want = check_adjacency(m)
    assert np.array_equal(want.counts, S.adjacency_of(name).counts)
    for flags in (0, FIX):
        check_smooth(m, flags=flags)
    check_smooth(m, mu=0.0)
    check_smooth(m, with_class=False)
    check_smooth(m, in_place=True)
    check_smooth(m, iterations=(1, 3), mu=0.0, in_place=True)


def test_ten_iterations_on_the_noisy_sphere_do_what_the_rule_test_says():
    m = Mesh(S.noisy_sphere(), R.mesh_of("sphere").triangles)
    out = check_smooth(m, iterations=(10,))
    mean0, rms0 = S.radial(m.v, S.SPHERE_CENTRE)
    mean1, rms1 = S.radial(out, S.SPHERE_CENTRE)
    assert rms1 < 0.5 * rms0 and abs(mean1 / mean0 - 1) < 1e-3


def test_one_strip_past_the_grid_cap():
    m = Mesh(*S.strip(GRID_CAP + 5003, seed=5))
    want = check_adjacency(m)
    assert want.counts.tolist() == [4 * m.T + 2, 2 * m.T + 1, m.T + 2, 0, m.V, 0, 0, m.V]
    check_smooth(m, iterations=(1, 2), flags=0)
    assert (m.adj.vertex_class == 2).all()
    assert np.array_equal(raw_smooth(m, 2), m.v.view(np.uint32))         # every vertex is on the boundary: fixed, nothing moves


def test_triangles_renumbered_by_a_random_permutation():
    base = R.mesh_of("torus")
    perm = np.random.default_rng(3).permutation(len(base.vertices))
    v = np.empty_like(base.vertices)
    v[perm] = base.vertices
    t = perm[base.triangles.astype(np.int64)].astype(np.uint32)[np.random.default_rng(4).permutation(len(base.triangles))]
    m = Mesh(v, t)
    want = check_adjacency(m)
    assert np.array_equal(want.counts, S.adjacency_of("torus").counts)
    out = check_smooth(m, iterations=(2,))
    ref = S.smooth(base.vertices, S.adjacency_of("torus"), 2)
    assert np.abs(out[perm] - ref).max() < 1e-5 and (out[perm] != ref).any()     # the same surface; the sums run in another order


# ------------------------------------------------------------------------------------------------ capacities, nullable outputs
def test_capacity_one_short_and_half():
    m = extracted("cut")
    want = m.adj
    full = int(want.counts[0])
    for cap in (full - 1, full // 2):
        rows, nbr, cls, n = raw_adjacency(m, cap)                        # (asserts the guard rows: nothing past the capacity)
        assert np.array_equal(n, want.counts) and np.array_equal(u32(rows[:m.V + 1]), want.row_start)
        assert np.array_equal(cls[:m.V].cpu().numpy(), want.vertex_class)


def test_nullable_outputs():
    m = Mesh(*S.soup(5000, 3000, 9, p_bad=0.02, p_degenerate=0.03, p_reverse=0.2))
    want = m.adj
    cap = int(want.counts[0])
    for with_rows, with_class in ((False, True), (True, False), (False, False)):
        rows, nbr, cls, n = raw_adjacency(m, cap, with_rows=with_rows, with_class=with_class)
        assert np.array_equal(n, want.counts) and np.array_equal(u32(nbr[:cap]), want.neighbours)
        assert not with_rows or np.array_equal(u32(rows[:m.V + 1]), want.row_start)
        assert not with_class or np.array_equal(cls[:m.V].cpu().numpy(), want.vertex_class)
    rows, nbr, cls, n = raw_adjacency(m, 0, with_rows=False, with_class=False)      # counts only
    assert np.array_equal(n, want.counts)


# ------------------------------------------------------------------------------------------------ smoothing: order, non-finite, scratch
def test_the_sum_runs_in_the_rows_order_on_a_wide_range_soup():
    v, t = S.soup(4000, 300, 13, lo=-3.0, hi=3.0)
    m = Mesh(v, t)
    a = m.adj
    assert np.diff(a.row_start.astype(np.int64)).min() >= 8
    up = S.step(v, a.row_start, a.neighbours, None, 0.5, 0)
    down = S.step(v, a.row_start, a.neighbours, None, 0.5, 0, descending=True)
    assert (up.view(np.uint32) != down.view(np.uint32)).any(1).sum() > 100          # otherwise the case proves nothing
    assert np.array_equal(raw_smooth(m, 1, 0.5, 0.0, 0), up.view(np.uint32))
    check_smooth(m, flags=0)
    check_smooth(m, flags=0, lam=0.33, mu=-0.34)


def test_nan_and_inf_propagate():
    base = extracted("sphere")
    v = base.v.copy()
    v[100, 1], v[2000, 0], v[3000, 2], v[77, 3] = np.nan, np.inf, -np.inf, np.nan
    m = Mesh(v, base.t)
    for it in (1, 2):
        want = S.smooth(v, m.adj, it)
        got = raw_smooth(m, it)
        assert np.isnan(want).any(1).sum() > 10 and same_or_both_nan(got, want)
    assert np.array_equal(raw_smooth(m, 0), v.view(np.uint32))           # a copy moves bits, NaN payloads included


def test_repeats_sizes_streams_and_released_scratch():
    small, big = Mesh(*S.soup(300, 200, 21, p_bad=0.03, p_reverse=0.2)), extracted("torus")
    for m in (small, small, big, small):                                 # the same call twice; a large call, then a small one in the same scratch
        check_adjacency(m)
        check_smooth(m, iterations=(1, 2))
    with torch.cuda.stream(torch.cuda.Stream()):
        check_adjacency(small)
        check_smooth(big, iterations=(2,), in_place=True)
        check_adjacency(big)
    assert capi.lib().dfusion_release_scratch() == 0
    check_adjacency(small)
    check_smooth(small, iterations=(3,))


# ------------------------------------------------------------------------------------------------ argument checks
def test_every_argument_check_of_the_adjacency():
    L = capi.lib()
    t = torch.from_numpy(S.tetrahedron().view(np.int32)).cuda()
    rows = torch.zeros(8, dtype=torch.int32, device="cuda")
    nbr = torch.zeros(32, dtype=torch.int32, device="cuda")
    cls = torch.zeros(8, dtype=torch.uint8, device="cuda")
    n = torch.zeros(8, dtype=torch.int64, device="cuda")
    big = 1 << 32
    good = lambda **kw: [kw.get("tri", ptr(t)), kw.get("T", 4), kw.get("V", 4), kw.get("rows", ptr(rows)), kw.get("nbr", ptr(nbr)), kw.get("cap", 24),
                         kw.get("cls", ptr(cls)), kw.get("counts", ptr(n)), None]
    assert L.dfusion_mesh_adjacency(*good()) == 0
    torch.cuda.synchronize()
    assert n.tolist() == [12, 6, 0, 0, 4, 0, 0, 0] and u32(rows[:5]).tolist() == [0, 3, 6, 9, 12] and u32(nbr[:3]).tolist() == [1, 2, 3]
    bad_calls = [dict(tri=None), dict(nbr=None), dict(counts=None), dict(V=big), dict(T=(big - 1) // 6 + 1), dict(T=big),
                 dict(rows=ptr(t)), dict(nbr=ptr(t)), dict(cls=ptr(t)), dict(counts=ptr(t)), dict(nbr=C.c_void_p(t.data_ptr() + 44)),
                 dict(rows=C.c_void_p(t.data_ptr() + 40))]
    for bad in bad_calls:
        assert L.dfusion_mesh_adjacency(*good(**bad)) == INVALID, bad
    assert L.dfusion_mesh_adjacency(*good(rows=None, cls=None, nbr=None, cap=0)) == 0                     # counts only
    assert L.dfusion_mesh_adjacency(*good(tri=None, T=0)) == 0                                           # arrays of length 0 may be NULL
    torch.cuda.synchronize()
    assert n.tolist() == [0] * 8 and u32(rows[:5]).tolist() == [0] * 5
    assert L.dfusion_mesh_adjacency(*good(V=0, cls=None)) == 0
    torch.cuda.synchronize()
    assert n.tolist() == [0, 0, 0, 0, 0, 4, 0, 0]
    with pytest.raises(ValueError):
        mesh_adjacency(torch.zeros((2, 3), dtype=torch.int64, device="cuda"), 4)


def test_every_argument_check_of_the_smoothing():
    L = capi.lib()
    m = Mesh(None, S.tetrahedron(), 4)
    out = torch.zeros((8, 4), dtype=torch.float32, device="cuda")
    big = 1 << 32
    good = lambda **kw: [kw.get("vtx", ptr(m.vd)), kw.get("V", 4), kw.get("rows", ptr(m.rows_d)), kw.get("nbr", ptr(m.nbr_d)), kw.get("nn", 12),
                         kw.get("cls", ptr(m.cls_d)), kw.get("it", 2), kw.get("lam", 0.5), kw.get("mu", -0.53), kw.get("flags", FIX), kw.get("out", ptr(out)), None]
    assert L.dfusion_mesh_smooth(*good()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(u32(out[:4]), S.smooth(m.v, m.adj, 2).view(np.uint32))
    bad_calls = [dict(vtx=None), dict(rows=None), dict(nbr=None), dict(out=None), dict(it=-1), dict(lam=float("nan")), dict(lam=float("inf")),
                 dict(mu=float("nan")), dict(mu=float("-inf")), dict(flags=2), dict(flags=0x80000001), dict(V=big), dict(nn=big),
                 dict(out=ptr(m.rows_d)), dict(out=ptr(m.nbr_d)), dict(out=ptr(m.cls_d)), dict(out=C.c_void_p(m.vd.data_ptr() + 16)),
                 dict(vtx=C.c_void_p(out.data_ptr() + 32))]
    for bad in bad_calls:
        assert L.dfusion_mesh_smooth(*good(**bad)) == INVALID, bad
    assert L.dfusion_mesh_smooth(*good(cls=None)) == 0                                                   # nullable
    assert L.dfusion_mesh_smooth(*good(vtx=None, V=0, out=None, nbr=None, nn=0)) == 0                    # arrays of length 0 may be NULL
    assert L.dfusion_mesh_smooth(*good(it=0, flags=0)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(u32(out[:4]), m.v.view(np.uint32))
    with pytest.raises(ValueError):
        smooth_mesh(m.vd[:, :3], m.td)
    with pytest.raises(ValueError):
        smooth_mesh(m.vd, m.td, adjacency=(m.rows_d[:3], m.nbr_d, m.cls_d))
    with pytest.raises(capi.DfusionError):
        smooth_mesh(m.vd, m.td, iterations=-1)


# ------------------------------------------------------------------------------------------------ the Python mirrors
def test_mirror_functions_equal_the_restatement():
    m = extracted("hand")
    want = m.adj
    rows, nbr, cls, n = mesh_adjacency(m.td, m.V, return_counts=True)
    assert rows.dtype == torch.int32 and nbr.dtype == torch.int32 and cls.dtype == torch.uint8 and nbr.shape == (int(want.counts[0]),)
    assert np.array_equal(u32(rows), want.row_start) and np.array_equal(u32(nbr), want.neighbours) and np.array_equal(cls.cpu().numpy(), want.vertex_class)
    assert n.tolist() == [int(c) for c in want.counts]
    assert len(mesh_adjacency(m.td, m.V)) == 3 and mesh_ops.mesh_adjacency is mesh_adjacency and mesh_ops.smooth_mesh is smooth_mesh
    topo = mesh_topology(m.td, m.V)
    assert topo == dict(zip(S.COUNT_NAMES, (int(c) for c in want.counts)), euler=-1)
    assert mesh_topology(extracted("sphere").td, extracted("sphere").V)["euler"] == 2 and mesh_topology(extracted("torus").td, extracted("torus").V)["euler"] == 0
    assert np.array_equal(u32(smooth_mesh(m.vd, m.td)), S.smooth(m.v, want, 10).view(np.uint32))                     # the defaults
    assert np.array_equal(u32(smooth_mesh(m.vd, m.td, 3, 0.4, 0.0, fix_boundary=False, adjacency=(rows, nbr, cls))),
                          S.smooth(m.v, want, 3, 0.4, 0.0, flags=0).view(np.uint32))
    assert np.array_equal(u32(smooth_mesh(m.vd, m.td, 2, adjacency=(rows, nbr, None))), S.smooth(m.v, want, 2, use_class=False).view(np.uint32))
    e = mesh_adjacency(m.td[:0], 5, return_counts=True)
    assert u32(e[0]).tolist() == [0] * 6 and e[1].shape == (0,) and e[2].tolist() == [0] * 5 and e[3].tolist() == [0] * 8
    assert smooth_mesh(m.vd[:0], m.td[:0]).shape == (0, 4)
    assert np.array_equal(u32(smooth_mesh(m.vd, m.td[:0])), m.v.view(np.uint32))                                     # no triangle: nothing moves


def test_fetch_mesh_with_smooth_iterations_on_a_fused_scene():
    from test_gpu_mesh_components import fused_scene
    import mesh_simplify_ref as MS
    S_, vol, cv, wf, intr, ref = fused_scene()
    voxel = float(S_.sc.vs[0])
    v0, t0 = vol.fetchMesh()
    assert np.array_equal(u32(v0), ref.vertices.view(np.uint32)) and np.array_equal(u32(t0), ref.triangles)
    v1, t1, n1 = vol.fetchMesh(with_normals=True, smooth_iterations=0)   # 0: today's bytes
    assert same_bits(v0, v1) and same_bits(t0, t1) and same_bits(n1, vol.fetchNormals(v0))
    adj = S.adjacency(ref.triangles, len(ref.vertices))
    want = S.smooth(ref.vertices, adj, 3)
    assert (want[:, :3] != ref.vertices[:, :3]).any(1).sum() > len(want) // 4
    gv, gt = vol.fetchMesh(smooth_iterations=3)
    assert np.array_equal(u32(gv), want.view(np.uint32)) and same_bits(gt, t0)
    gv, gt, gn = vol.fetchMesh(with_normals=True, smooth_iterations=3)
    assert np.array_equal(u32(gv), want.view(np.uint32)) and same_bits(gn, vol.fetchNormals(gv))
    want = S.smooth(ref.vertices, adj, 2, 0.3, 0.0)
    assert np.array_equal(u32(vol.fetchMesh(smooth_iterations=2, smooth_lambda=0.3, smooth_mu=0.0)[0]), want.view(np.uint32))
    cell = 2 * voxel                                                     # after the simplification
    simple = MS.simplify(ref.vertices, ref.triangles, cell)
    want = S.smooth(simple.vertices, S.adjacency(simple.triangles, len(simple.vertices)), 3)
    gv, gt = vol.fetchMesh(simplify_cell=cell, smooth_iterations=3)
    assert np.array_equal(u32(gv), want.view(np.uint32)) and np.array_equal(u32(gt), simple.triangles)
