"""dfusion_mesh_boundary_loops, dfusion_mesh_fill_holes and their Python mirrors against the numpy restatement tests/mesh_holes_ref.py:
every output array and all eight counts, bit for bit, through the C-ABI into guarded buffers."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mesh_holes_ref as H
import mesh_ref as R
import mesh_smooth_ref as S
from dynamicfusion_amd import boundary_loops, capi, fill_holes, mesh_ops
from mesh_gpu import ptr, same_bits, same_or_both_nan, stream, u32

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID = 100001
GUARD = 4                                            # guard rows behind every output
G32 = -7                                             # what they hold
NONE = H.NONE
GRID_CAP = 2048 * 256                                # DF_MESH_MAX_BLOCKS workgroups of 256 lanes: past it a lane takes a second element
ALL = 0xffffffff


class Mesh:
    """A mesh on the device, uploaded once for all the calls made on it, with the restatement's loops."""

    def __init__(self, v, t, V=None):
        self.t = np.ascontiguousarray(t, np.uint32).reshape(-1, 3)
        self.V = len(v) if V is None else V
        self.v = S.positions(self.V) if v is None else np.ascontiguousarray(v, F32).reshape(-1, 4)
        self.T = len(self.t)
        self.td = torch.from_numpy(self.t.view(np.int32)).cuda()
        self.vd = torch.from_numpy(self.v).cuda()
        self.loops = H.boundary_loops(self.t, self.V)


def raw_loops(m, loop_cap, vertex_cap, with_next=True, with_rank=True):
    """One dfusion_mesh_boundary_loops call into guarded buffers -> (next, loop, rank, loop_start, loop_vertices) device tensors, guards
    included, and the counts."""
    nxt = torch.full((m.V + GUARD,), G32, dtype=torch.int32, device="cuda")
    loop = torch.full((m.V + GUARD,), G32, dtype=torch.int32, device="cuda")
    rank = torch.full((m.V + GUARD,), G32, dtype=torch.int32, device="cuda")
    start = torch.full((loop_cap + 1 + GUARD,), G32, dtype=torch.int32, device="cuda")
    members = torch.full((vertex_cap + GUARD,), G32, dtype=torch.int32, device="cuda")
    counts = torch.full((8 + GUARD,), 123, dtype=torch.int64, device="cuda")
    capi.check(capi.lib().dfusion_mesh_boundary_loops(ptr(m.td) if m.T else None, m.T, m.V, ptr(nxt) if with_next and m.V else None, ptr(loop) if m.V else None,
                                                      ptr(rank) if with_rank and m.V else None, ptr(start), loop_cap, ptr(members) if vertex_cap else None,
                                                      vertex_cap, ptr(counts), stream()), "dfusion_mesh_boundary_loops")
    torch.cuda.synchronize()
    assert (nxt[m.V:] == G32).all() and (loop[m.V:] == G32).all() and (rank[m.V:] == G32).all() and (counts[8:] == 123).all()
    assert (start[loop_cap + 1:] == G32).all() and (members[vertex_cap:] == G32).all()
    assert with_next or (nxt == G32).all()
    assert with_rank or (rank == G32).all()
    assert loop_cap or vertex_cap or ((start == G32).all() and (members == G32).all())           # both 0: neither CSR array is touched
    return nxt, loop, rank, start, members, counts[:8].cpu().numpy().astype(np.uint64)


def assert_per_vertex(m, nxt, loop, rank, n, with_next=True, with_rank=True):
    want = m.loops
    assert np.array_equal(n, want.counts), (n, want.counts)
    assert np.array_equal(u32(loop[:m.V]), want.vertex_loop), int((u32(loop[:m.V]) != want.vertex_loop).sum())
    assert not with_next or np.array_equal(u32(nxt[:m.V]), want.vertex_next)
    assert not with_rank or np.array_equal(u32(rank[:m.V]), want.vertex_rank), int((u32(rank[:m.V]) != want.vertex_rank).sum())


def check_loops(m):
    """Capacities 0, then the exact capacities (no loop: room for one, since both 0 leaves the CSR alone): everything equals the
    restatement."""
    want = m.loops
    nxt, loop, rank, start, members, n = raw_loops(m, 0, 0)
    assert_per_vertex(m, nxt, loop, rank, n)
    nl, nm = int(n[0]), int(n[1])
    nxt, loop, rank, start, members, n = raw_loops(m, nl if nl else 1, nm)
    assert_per_vertex(m, nxt, loop, rank, n)
    assert np.array_equal(u32(start[:nl + 1]), want.loop_start), (u32(start[:nl + 1])[:8], want.loop_start[:8])
    assert np.array_equal(u32(members[:nm]), want.loop_vertices), int((u32(members[:nm]) != want.loop_vertices).sum())
    return want


def raw_fill(m, max_edges, vcap, tcap, with_src=True, flags=0):
    """One dfusion_mesh_fill_holes call into guarded buffers -> (vertices as uint32 [vcap, 4], triangles, vertex_src, counts)."""
    out_v = torch.full((vcap + GUARD, 4), G32, dtype=torch.int32, device="cuda")
    out_t = torch.full((tcap + GUARD, 3), G32, dtype=torch.int32, device="cuda")
    src = torch.full((vcap + GUARD,), G32, dtype=torch.int32, device="cuda")
    counts = torch.full((8 + GUARD,), 123, dtype=torch.int64, device="cuda")
    capi.check(capi.lib().dfusion_mesh_fill_holes(ptr(m.vd) if m.V else None, m.V, ptr(m.td) if m.T else None, m.T, max_edges, flags,
                                                  ptr(out_v) if vcap else None, vcap, ptr(out_t) if tcap else None, tcap,
                                                  ptr(src) if with_src and vcap else None, ptr(counts), stream()), "dfusion_mesh_fill_holes")
    torch.cuda.synchronize()
    assert (out_v[vcap:] == G32).all() and (out_t[tcap:] == G32).all() and (src[vcap:] == G32).all() and (counts[8:] == 123).all()
    assert with_src or (src == G32).all()
    return u32(out_v[:vcap]), u32(out_t[:tcap]), u32(src[:vcap]), counts[:8].cpu().numpy().astype(np.uint64)


def check_fill(m, max_edges, nan_ok=False):
    """A count-only call, then one of exactly that size: everything equals the restatement."""
    want = H.fill_holes(m.v, m.t, max_edges, m.loops)
    _, _, _, n = raw_fill(m, max_edges, 0, 0)
    assert np.array_equal(n, want.counts), (max_edges, n, want.counts)
    gv, gt, gs, n = raw_fill(m, max_edges, int(n[0]), int(n[1]))
    assert np.array_equal(n, want.counts)
    assert np.array_equal(gt, want.triangles), int((gt != want.triangles).any(1).sum())
    assert np.array_equal(gs, want.vertex_src)
    if nan_ok:
        assert np.array_equal(gv[:m.V], m.v.view(np.uint32)) and same_or_both_nan(gv[m.V:], want.vertices[m.V:])
    else:
        assert np.array_equal(gv, want.vertices.view(np.uint32)), int((gv != want.vertices.view(np.uint32)).any(1).sum())
    return want


def fill_settings(m):
    """max_edges 0, 2, 3, 0xffffffff, and L - 1, L, L + 1 around the shortest and the longest loop."""
    out = {0, 2, 3, ALL}
    if len(m.loops.lengths):
        for L in (int(m.loops.lengths.min()), int(m.loops.lengths.max())):
            out |= {L - 1, L, L + 1}
    return sorted(out)


def check_all(m, nan_ok=False):
    check_loops(m)
    for max_edges in fill_settings(m):
        check_fill(m, max_edges, nan_ok)


# ------------------------------------------------------------------------------------------------ hand-made cases
CASES = H.small_cases()


@pytest.mark.parametrize("name,V,t", CASES, ids=[c[0] for c in CASES])
def test_small_cases(name, V, t):
    m = Mesh(None, t, V)
    check_all(m)
    if name == "pinch":
        assert m.loops.counts.tolist() == [0, 0, 6, 1, 4, 0, 0, 0]
    if name == "flipped fan":
        assert m.loops.counts[0] == 0 and m.loops.counts[4] == 6
    if name == "annulus of 6":
        assert m.loops.lengths.tolist() == [6, 6]


@pytest.mark.parametrize("T,V", [(0, 0), (0, 1), (1, 0), (1, 1), (1, 3), (0, 7)])
def test_t_or_v_of_0_and_1(T, V):
    m = Mesh(None, S.u3([[0, 1, 2]] * T), V)
    check_all(m)
    assert m.loops.counts[0] == (1 if (T, V) == (1, 3) else 0) and m.loops.counts[6] == (T if V < 3 else 0)


# the doubling windows at 2^r and 2^r +- 1, and one long loop; each with the label vertex first, last and mid-loop
LENGTHS = [3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 5000]


@pytest.mark.parametrize("n", LENGTHS)
def test_one_loop_of_n_under_three_renumberings(n):
    for where in ("first", "last", "mid"):
        V, t = H.fan_with_label_at(n, where)
        m = Mesh(None, t, V)
        want = check_loops(m)
        assert want.lengths.tolist() == [n] and want.vertex_loop[0] == 0 and want.vertex_rank[0] == 0
        walk = want.loop_vertices.astype(np.int64).tolist()
        assert where != "first" or walk == list(range(n))
        assert where != "last" or walk == [0] + list(range(n - 1, 0, -1))
        for max_edges in (n - 1, n, ALL):
            check_fill(m, max_edges)
    V, t = H.polygon_fan(n)                                                               # not renumbered: the hub is vertex 0, the label 1
    check_all(Mesh(None, t, V))


def test_70000_disjoint_triangles():
    V, t = H.disjoint_triangles(70000)
    perm = np.random.default_rng(5).permutation(V)
    m = Mesh(None, perm[t.astype(np.int64)], V)
    want = check_loops(m)
    assert want.counts.tolist() == [70000, 210000, 210000, 0, 0, 3, 0, 0]
    check_fill(m, 2)
    check_fill(m, 3)


def test_a_polygon_fan_past_the_grid_cap():
    n = GRID_CAP + 5003
    V, t = H.polygon_fan(n)
    perm = np.concatenate([[n], np.roll(np.arange(n), 77777)])                           # the hub last; the label 77777 steps into the rim
    m = Mesh(None, perm[t.astype(np.int64)], V)
    want = check_loops(m)
    assert want.counts.tolist() == [1, n, n, 0, 0, n, 0, 0]
    check_fill(m, n - 1)
    check_fill(m, n)


@pytest.mark.parametrize("seed,n,V", [(1, 3000, 40), (2, 20000, 700), (3, 60000, 50000)])
def test_soups_with_duplicate_reversed_invalid_and_degenerate_triangles(seed, n, V):
    v, t = S.soup(n, V, seed, p_bad=0.02, p_degenerate=0.05, p_reverse=0.3)
    m = Mesh(v, t)
    check_all(m)
    assert m.loops.counts[6] > n // 40 and m.loops.counts[7] > n // 40
    if V == 50000:
        assert m.loops.counts[0] > 10 and m.loops.counts[3] > 1000 and m.loops.counts[4] > 1000


@functools.lru_cache(None)
def extracted(name):
    m = {"scene": H.scene_mesh, "noise 0.1": lambda: H.noise_mesh(0.1), "noise 0.0": lambda: H.noise_mesh(0.0)}.get(name, lambda: R.mesh_of(name))()
    return Mesh(m.vertices, m.triangles)


@pytest.mark.parametrize("name", ["sphere", "torus", "cut", "hand", "scene", "noise 0.1", "noise 0.0"])
def test_extracted_meshes(name):
    m = extracted(name)
    check_all(m)
    if name == "scene":
        assert m.loops.counts.tolist() == [44, 1062, 1402, 18, 304, 516, 0, 0]
        assert check_fill(m, 32).counts.tolist() == [m.V + 42, m.T + 250, 42, 2, 250, 20, 516, 304]
    if name == "noise 0.1":
        assert m.loops.counts[0] == 133 and m.loops.counts[4] > 0                        # the open-chain branch


# ------------------------------------------------------------------------------------------------ capacities, nullable outputs
def test_capacities_one_short_and_half():
    m = extracted("scene")
    nl, nm = int(m.loops.counts[0]), int(m.loops.counts[1])
    for lcap, vcap in ((nl - 1, nm), (nl, nm - 1), (nl // 2, nm // 2), (nl, 0), (0, nm)):
        nxt, loop, rank, start, members, n = raw_loops(m, lcap, vcap)                    # (asserts the guards: nothing past a capacity)
        assert_per_vertex(m, nxt, loop, rank, n)
        if lcap == nl:
            assert np.array_equal(u32(start[:nl + 1]), m.loops.loop_start)
    want = H.fill_holes(m.v, m.t, 32, m.loops)
    kv, kt = int(want.counts[0]), int(want.counts[1])
    for vcap, tcap in ((kv - 1, kt), (kv, kt - 1), (kv // 2, kt // 2), (kv, 0), (0, kt), (m.V - 5, m.T - 5)):
        gv, gt, gs, n = raw_fill(m, 32, vcap, tcap)
        assert np.array_equal(n, want.counts)
        if tcap == kt:
            assert np.array_equal(gt, want.triangles)
        if vcap == kv:
            assert np.array_equal(gv, want.vertices.view(np.uint32)) and np.array_equal(gs, want.vertex_src)


def test_nullable_outputs():
    m = extracted("noise 0.1")
    nl, nm = int(m.loops.counts[0]), int(m.loops.counts[1])
    for with_next, with_rank in ((False, True), (True, False), (False, False)):
        nxt, loop, rank, start, members, n = raw_loops(m, nl, nm, with_next, with_rank)
        assert_per_vertex(m, nxt, loop, rank, n, with_next, with_rank)
        assert np.array_equal(u32(start[:nl + 1]), m.loops.loop_start) and np.array_equal(u32(members[:nm]), m.loops.loop_vertices)
    want = H.fill_holes(m.v, m.t, 16, m.loops)
    gv, gt, gs, n = raw_fill(m, 16, int(want.counts[0]), int(want.counts[1]), with_src=False)
    assert np.array_equal(n, want.counts) and np.array_equal(gt, want.triangles) and np.array_equal(gv, want.vertices.view(np.uint32))


def test_repeats_sizes_streams_and_released_scratch():
    small, big = Mesh(*S.soup(300, 200, 21, p_bad=0.03, p_reverse=0.2)), extracted("hand")
    for m in (small, small, big, small):                                 # the same call twice; a large call, then a small one in the same scratch
        check_loops(m)
        check_fill(m, 32)
    with torch.cuda.stream(torch.cuda.Stream()):
        check_loops(small)
        check_fill(big, 120)
        check_loops(big)
    assert capi.lib().dfusion_release_scratch() == 0
    check_loops(small)
    check_fill(big, 32)


# ------------------------------------------------------------------------------------------------ the centroid's arithmetic
def test_the_centroid_is_summed_from_the_label_vertex_on_a_wide_range_loop():
    n = 200
    V, t = H.fan_with_label_at(n, "mid")
    rng = np.random.default_rng(17)
    v = np.zeros((V, 4), F32)
    v[:, :3] = (10.0 ** rng.uniform(-3.0, 3.0, (V, 3)) * rng.choice([-1.0, 1.0], (V, 3))).astype(F32)
    v[:, 3] = rng.standard_normal(V)
    m = Mesh(v, t)
    want = check_fill(m, n)
    others = [H.fill_holes(v, t, n, m.loops, start_rank=r).vertices[V] for r in (1, n // 2, n - 1)]
    assert all((o.view(np.uint32) != want.vertices[V].view(np.uint32)).any() for o in others)    # otherwise the case proves nothing
    assert want.vertices[V, 3] == 0 and want.vertex_src[V] == NONE


def test_nan_and_inf_propagate():
    base = extracted("hand")
    v = base.v.copy()
    lp = base.loops
    first = lp.loop_vertices[lp.loop_start[:-1].astype(np.int64)]                         # one vertex of each of the three loops
    v[first[0], 1], v[first[1], 0], v[first[2], 2] = np.nan, np.inf, -np.inf
    v[lp.loop_vertices[lp.loop_start[2] + 5], 2] = np.inf                                 # inf - inf on the third loop
    m = Mesh(v, base.t)
    want = check_fill(m, ALL, nan_ok=True)
    new = want.vertices[m.V:]
    assert np.isnan(new).any(1).sum() == 2 and np.isinf(new).any(1).sum() == 1


def test_the_second_fill_adds_nothing_and_the_adjacency_of_the_result():
    for name, max_edges in (("scene", 32), ("hand", 32), ("hand", ALL), ("noise 0.1", 8), ("cut", 182)):
        m = extracted(name)
        want = H.fill_holes(m.v, m.t, max_edges, m.loops)
        gv, gt, src, n = fill_holes(m.vd, m.td, max_edges, return_counts=True)
        assert np.array_equal(u32(gt), want.triangles) and np.array_equal(u32(gv), want.vertices.view(np.uint32))
        v2, t2, src2, n2 = fill_holes(gv, gt, max_edges, return_counts=True)
        assert n2.tolist()[:5] == [len(want.vertices), len(want.triangles), 0, int(want.counts[3]), 0]
        assert np.array_equal(u32(t2), want.triangles) and np.array_equal(u32(v2), u32(gv))
        before, after = S.adjacency(m.t, m.V), S.adjacency(want.triangles, len(want.vertices))
        rows, nbr, cls, counts = mesh_ops.mesh_adjacency(gt, len(want.vertices), return_counts=True)
        assert np.array_equal(u32(rows), after.row_start) and np.array_equal(u32(nbr), after.neighbours)
        assert np.array_equal(cls.cpu().numpy(), after.vertex_class) and counts.tolist() == [int(c) for c in after.counts]
        assert after.counts[2] == before.counts[2] - want.counts[4] and after.counts[3] == before.counts[3]
        assert S.euler(after, len(want.triangles)) == S.euler(before, m.T) + int(want.counts[2])
        if name == "cut":
            assert S.euler(after, len(want.triangles)) == 2 and after.counts[2] == 0


# ------------------------------------------------------------------------------------------------ argument checks
def test_every_argument_check_of_the_loops():
    L = capi.lib()
    t = torch.from_numpy(H.polygon_fan(5)[1].view(np.int32)).cuda()                       # 5 triangles over 6 vertices
    a = [torch.zeros(16, dtype=torch.int32, device="cuda") for _ in range(5)]
    n = torch.zeros(8, dtype=torch.int64, device="cuda")
    big = 1 << 32
    good = lambda **kw: [kw.get("tri", ptr(t)), kw.get("T", 5), kw.get("V", 6), kw.get("nxt", ptr(a[0])), kw.get("loop", ptr(a[1])), kw.get("rank", ptr(a[2])),
                         kw.get("start", ptr(a[3])), kw.get("lcap", 4), kw.get("members", ptr(a[4])), kw.get("vcap", 8), kw.get("counts", ptr(n)), None]
    assert L.dfusion_mesh_boundary_loops(*good()) == 0
    torch.cuda.synchronize()
    assert n.tolist() == [1, 5, 5, 0, 0, 5, 0, 0] and u32(a[3][:2]).tolist() == [0, 5] and u32(a[4][:5]).tolist() == [1, 2, 3, 4, 5]
    assert u32(a[0][:6]).tolist() == [NONE, 2, 3, 4, 5, 1] and u32(a[1][:6]).tolist() == [NONE, 1, 1, 1, 1, 1] and u32(a[2][:6]).tolist() == [NONE, 0, 1, 2, 3, 4]
    bad_calls = [dict(tri=None), dict(loop=None), dict(start=None), dict(members=None), dict(counts=None), dict(V=big), dict(T=(big - 1) // 6 + 1),
                 dict(T=big), dict(lcap=big), dict(vcap=big), dict(start=None, vcap=0), dict(start=None, lcap=0),
                 dict(nxt=ptr(t)), dict(loop=ptr(t)), dict(rank=ptr(t)), dict(start=ptr(t)), dict(members=ptr(t)), dict(counts=ptr(t)),
                 dict(members=C.c_void_p(t.data_ptr() + 56)), dict(loop=C.c_void_p(t.data_ptr() + 40))]
    for bad in bad_calls:
        assert L.dfusion_mesh_boundary_loops(*good(**bad)) == INVALID, bad
    assert L.dfusion_mesh_boundary_loops(*good(nxt=None, rank=None, start=None, lcap=0, members=None, vcap=0)) == 0       # per-vertex and counts only
    assert L.dfusion_mesh_boundary_loops(*good(members=None, vcap=0)) == 0
    assert L.dfusion_mesh_boundary_loops(*good(tri=None, T=0)) == 0                                                     # arrays of length 0 may be NULL
    torch.cuda.synchronize()
    assert n.tolist() == [0] * 8 and u32(a[1][:6]).tolist() == [NONE] * 6 and u32(a[3][:1]).tolist() == [0]
    assert L.dfusion_mesh_boundary_loops(*good(V=0, nxt=None, loop=None, rank=None)) == 0
    torch.cuda.synchronize()
    assert n.tolist() == [0, 0, 0, 0, 0, 0, 5, 0]
    with pytest.raises(ValueError):
        boundary_loops(torch.zeros((2, 3), dtype=torch.int64, device="cuda"), 4)


def test_every_argument_check_of_the_fill():
    L = capi.lib()
    m = Mesh(None, H.polygon_fan(5)[1], 6)
    out_v = torch.zeros((16, 4), dtype=torch.float32, device="cuda")
    out_t = torch.zeros((16, 3), dtype=torch.int32, device="cuda")
    src = torch.zeros(16, dtype=torch.int32, device="cuda")
    n = torch.zeros(8, dtype=torch.int64, device="cuda")
    big = 1 << 32
    good = lambda **kw: [kw.get("vtx", ptr(m.vd)), kw.get("V", 6), kw.get("tri", ptr(m.td)), kw.get("T", 5), kw.get("max_edges", 5), kw.get("flags", 0),
                         kw.get("out_v", ptr(out_v)), kw.get("vcap", 7), kw.get("out_t", ptr(out_t)), kw.get("tcap", 10), kw.get("src", ptr(src)),
                         kw.get("counts", ptr(n)), None]
    assert L.dfusion_mesh_fill_holes(*good()) == 0
    torch.cuda.synchronize()
    want = H.fill_holes(m.v, m.t, 5)
    assert n.tolist() == [7, 10, 1, 0, 5, 5, 0, 0] and np.array_equal(u32(out_t[:10]), want.triangles) and np.array_equal(u32(out_v[:7]), want.vertices.view(np.uint32))
    assert u32(out_t[5]).tolist() == [2, 1, 6] and u32(src[:7]).tolist() == [0, 1, 2, 3, 4, 5, NONE]
    bad_calls = [dict(vtx=None), dict(tri=None), dict(out_v=None), dict(out_t=None), dict(counts=None), dict(flags=1), dict(flags=0x80000000), dict(V=big),
                 dict(T=(big - 1) // 6 + 1), dict(vcap=big), dict(tcap=big),
                 dict(out_v=ptr(m.vd)), dict(out_v=ptr(m.td)), dict(out_t=ptr(m.td)), dict(out_t=ptr(m.vd)), dict(src=ptr(m.td)), dict(src=ptr(m.vd)),
                 dict(counts=ptr(m.td)), dict(counts=ptr(m.vd)), dict(out_t=C.c_void_p(m.td.data_ptr() + 48)), dict(out_v=C.c_void_p(m.vd.data_ptr() + 80))]
    for bad in bad_calls:
        assert L.dfusion_mesh_fill_holes(*good(**bad)) == INVALID, bad
    assert L.dfusion_mesh_fill_holes(*good(src=None)) == 0                                                              # nullable
    assert L.dfusion_mesh_fill_holes(*good(out_v=None, vcap=0, out_t=None, tcap=0, src=None)) == 0                      # counts only
    assert L.dfusion_mesh_fill_holes(*good(max_edges=4)) == 0
    torch.cuda.synchronize()
    assert n.tolist() == [6, 5, 0, 1, 0, 0, 5, 0]
    assert L.dfusion_mesh_fill_holes(*good(tri=None, T=0)) == 0                                                         # arrays of length 0 may be NULL
    torch.cuda.synchronize()
    assert n.tolist() == [6, 0, 0, 0, 0, 0, 0, 0] and np.array_equal(u32(out_v[:6]), m.v.view(np.uint32)) and u32(src[:6]).tolist() == list(range(6))
    assert L.dfusion_mesh_fill_holes(*good(vtx=None, V=0)) == 0
    torch.cuda.synchronize()
    assert n.tolist() == [0, 5, 0, 0, 0, 0, 0, 0] and np.array_equal(u32(out_t[:5]), m.t)
    with pytest.raises(ValueError):
        fill_holes(m.vd[:, :3], m.td, 5)
    with pytest.raises(ValueError):
        fill_holes(m.vd, m.td, -1)


# ------------------------------------------------------------------------------------------------ the Python mirrors
def test_mirror_functions_equal_the_restatement():
    m = extracted("hand")
    want = m.loops
    nxt, loop, rank, start, members, n = boundary_loops(m.td, m.V, return_counts=True)
    assert all(x.dtype == torch.int32 for x in (nxt, loop, rank, start, members)) and start.shape == (4,) and members.shape == (184,)
    assert np.array_equal(u32(nxt), want.vertex_next) and np.array_equal(u32(loop), want.vertex_loop) and np.array_equal(u32(rank), want.vertex_rank)
    assert np.array_equal(u32(start), want.loop_start) and np.array_equal(u32(members), want.loop_vertices)
    assert n.tolist() == [int(c) for c in want.counts] and len(boundary_loops(m.td, m.V)) == 5
    assert mesh_ops.boundary_loops is boundary_loops and mesh_ops.fill_holes is fill_holes
    assert len(mesh_ops.LOOP_COUNT_NAMES) == 8 and mesh_ops.LOOP_COUNT_NAMES == H.LOOP_COUNT_NAMES and mesh_ops.FILL_COUNT_NAMES == H.FILL_COUNT_NAMES
    wf = H.fill_holes(m.v, m.t, 32, want)
    gv, gt, src, n = fill_holes(m.vd, m.td, 32, return_counts=True)
    assert gv.dtype == torch.float32 and gv.shape == (m.V + 2, 4) and gt.shape == (m.T + 64, 3) and len(fill_holes(m.vd, m.td, 32)) == 3
    assert np.array_equal(u32(gv), wf.vertices.view(np.uint32)) and np.array_equal(u32(gt), wf.triangles) and np.array_equal(u32(src), wf.vertex_src)
    assert n.tolist() == [int(c) for c in wf.counts]
    e = boundary_loops(m.td[:0], 5, return_counts=True)
    assert u32(e[1]).tolist() == [NONE] * 5 and u32(e[3]).tolist() == [0] and e[4].shape == (0,) and e[5].tolist() == [0] * 8
    e = boundary_loops(m.td[:0], 0)
    assert e[0].shape == (0,) and u32(e[3]).tolist() == [0]
    assert fill_holes(m.vd[:0], m.td[:0], 9)[0].shape == (0, 4)
    gv, gt, src = fill_holes(m.vd, m.td[:0], 9)                                           # no triangle: the vertices are copied
    assert np.array_equal(u32(gv), m.v.view(np.uint32)) and gt.shape == (0, 3) and u32(src).tolist() == list(range(m.V))


def test_fetch_mesh_with_fill_holes_max_edges_on_a_fused_scene():
    from test_gpu_mesh_components import fused_scene
    import mesh_simplify_ref as MS
    S_, vol, cv, wf, intr, ref = fused_scene()
    voxel = float(S_.sc.vs[0])
    v0, t0 = vol.fetchMesh()
    assert np.array_equal(u32(v0), ref.vertices.view(np.uint32)) and np.array_equal(u32(t0), ref.triangles)
    v1, t1, n1 = vol.fetchMesh(with_normals=True, fill_holes_max_edges=0)                 # 0: today's bytes
    assert same_bits(v0, v1) and same_bits(t0, t1) and same_bits(n1, vol.fetchNormals(v0))
    want = H.fill_holes(ref.vertices, ref.triangles, 32)
    assert want.counts[2] > 0 and want.counts[3] > 0                                      # some loops are filled, the rim is not
    gv, gt = vol.fetchMesh(fill_holes_max_edges=32)
    assert np.array_equal(u32(gv), want.vertices.view(np.uint32)) and np.array_equal(u32(gt), want.triangles)
    gv, gt, gn = vol.fetchMesh(with_normals=True, fill_holes_max_edges=32)
    assert np.array_equal(u32(gv), want.vertices.view(np.uint32)) and same_bits(gn, vol.fetchNormals(gv))
    smooth = S.smooth(want.vertices, S.adjacency(want.triangles, len(want.vertices)), 3)  # the fill comes before the smoothing
    gv, gt = vol.fetchMesh(fill_holes_max_edges=32, smooth_iterations=3)
    assert np.array_equal(u32(gv), smooth.view(np.uint32)) and np.array_equal(u32(gt), want.triangles)
    unfilled = S.smooth(ref.vertices, S.adjacency(ref.triangles, len(ref.vertices)), 3)
    assert (smooth[:len(unfilled)] != unfilled).any()                                     # a closed-up rim is not frozen any more
    cell = 2 * voxel                                                                      # after the simplification
    simple = MS.simplify(ref.vertices, ref.triangles, cell)
    want = H.fill_holes(simple.vertices, simple.triangles, 32)
    gv, gt = vol.fetchMesh(simplify_cell=cell, fill_holes_max_edges=32)
    assert np.array_equal(u32(gv), want.vertices.view(np.uint32)) and np.array_equal(u32(gt), want.triangles)
    smooth = S.smooth(want.vertices, S.adjacency(want.triangles, len(want.vertices)), 3)
    gv, gt = vol.fetchMesh(simplify_cell=cell, fill_holes_max_edges=32, smooth_iterations=3)
    assert np.array_equal(u32(gv), smooth.view(np.uint32)) and np.array_equal(u32(gt), want.triangles)
