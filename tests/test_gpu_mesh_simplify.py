"""dfusion_mesh_simplify and its Python mirror against the numpy restatement tests/mesh_simplify_ref.py: every output array and all eight
counts, bit for bit, through the C-ABI into guarded buffers."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_simplify_ref as S
from dynamicfusion_amd import capi, mesh_ops, simplify_mesh
from mesh_gpu import dev_tri, dev_vtx, ptr, same_bits, stream, u32

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID = 100001
GUARD = 4                                            # guard rows behind every output
G32 = -7                                             # what they hold (0xfffffff9)
KF, KD = S.KEEP_FIRST, S.KEEP_DUPLICATES
ALL_FLAGS = (0, KF, KD, KF | KD)
GRID_CAP = 2048 * 256                                # DF_MESH_MAX_BLOCKS workgroups of 256 lanes: past it a lane takes a second element


class Mesh:
    """A mesh on the device, uploaded once for all the calls made on it."""

    def __init__(self, v, t):
        self.v, self.t = np.ascontiguousarray(v, F32).reshape(-1, 4), np.ascontiguousarray(t, np.uint32).reshape(-1, 3)
        self.vd, self.td = dev_vtx(self.v), dev_tri(self.t)
        self.V, self.T = len(self.v), len(self.t)


def raw(m, cell, flags, vcap, tcap, with_src=True, with_map=True):
    """One dfusion_mesh_simplify call into guarded buffers of the given capacities -> (vertices, triangles, vertex_src, vertex_map) device
    tensors, guards included, and the counts."""
    out_v = torch.full((vcap + GUARD, 4), G32, dtype=torch.int32, device="cuda")
    out_t = torch.full((tcap + GUARD, 3), G32, dtype=torch.int32, device="cuda")
    src = torch.full((vcap + GUARD,), G32, dtype=torch.int32, device="cuda")
    vmap = torch.full((m.V + GUARD,), G32, dtype=torch.int32, device="cuda")
    counts = torch.full((8 + GUARD,), 123, dtype=torch.int64, device="cuda")
    capi.check(capi.lib().dfusion_mesh_simplify(ptr(m.vd) if m.V else None, m.V, ptr(m.td) if m.T else None, m.T, cell, flags,
                                                ptr(out_v) if vcap else None, vcap, ptr(out_t) if tcap else None, tcap,
                                                ptr(src) if with_src and vcap else None, ptr(vmap) if with_map else None, ptr(counts), stream()),
               "dfusion_mesh_simplify")
    torch.cuda.synchronize()
    assert (out_v[vcap:] == G32).all() and (out_t[tcap:] == G32).all() and (src[vcap:] == G32).all() and (vmap[m.V:] == G32).all()
    assert (counts[8:] == 123).all()
    assert with_src or (src == G32).all()
    assert with_map or (vmap == G32).all()
    return out_v, out_t, src, vmap, counts[:8].cpu().numpy().astype(np.uint64)


def check(m, cell, flags=0, want=None):
    """Count-only, then exact capacities: everything equals the restatement."""
    want = S.simplify(m.v, m.t, cell, flags) if want is None else want
    out_v, out_t, src, vmap, n = raw(m, cell, flags, 0, 0)
    assert np.array_equal(n, want.counts), (n, want.counts)
    assert (vmap == G32).all()                                          # counts only: nothing else is written
    kv, kt = int(n[0]), int(n[1])
    out_v, out_t, src, vmap, n = raw(m, cell, flags, kv, kt)
    assert np.array_equal(n, want.counts), (n, want.counts)
    assert np.array_equal(u32(out_t[:kt]), want.triangles), int((u32(out_t[:kt]) != want.triangles).any(1).sum())
    assert np.array_equal(u32(src[:kv]), want.vertex_src)
    assert np.array_equal(u32(out_v[:kv]), want.vertices.view(np.uint32)), int((u32(out_v[:kv]) != want.vertices.view(np.uint32)).any(1).sum())
    if kt or kv:
        assert np.array_equal(u32(vmap[:m.V]), want.vertex_map)
    else:
        assert (want.vertex_map == S.NONE).all() and (vmap == G32).all()   # nothing kept: exact capacities are 0 and 0, counts only again
    return want


def check_flags(m, cell, flags=ALL_FLAGS):
    return [check(m, cell, f) for f in flags]


# ------------------------------------------------------------------------------------------------ hand-made cases and wave boundaries
@pytest.mark.parametrize("name,v,t,cell", S.small_cases(), ids=[c[0] for c in S.small_cases()])
def test_small_cases(name, v, t, cell):
    plain, first, dups, both = check_flags(Mesh(v, t), cell)
    if name == "fin pair":
        assert plain.counts.tolist() == [0, 0, 0, 0, 2, 0, 3, 0] and dups.counts.tolist() == [3, 2, 0, 0, 0, 0, 3, 0]
    if name == "three against one":
        assert plain.kept.tolist() == [1] and plain.counts[5] == 3
    if name == "two against two":
        assert plain.counts[4] == 4 and plain.counts[1] == 0
    if name.startswith("at 2^30"):
        assert plain.counts[7] == 1 and plain.counts[2] == 2
    if name == "just below 2^30":
        assert plain.counts[7] == 0 and plain.counts[1] == 2


def test_5000_vertices_each_in_a_cell_of_its_own():
    rng = np.random.default_rng(11)
    cellsxyz = rng.permutation(40 ** 3)[:5000]
    v = np.zeros((5000, 4), F32)
    v[:, 0], v[:, 1], v[:, 2] = cellsxyz % 40 - 20 + 0.5, cellsxyz // 40 % 40 - 20 + 0.25, cellsxyz // 1600 - 20 + 0.75
    t = rng.integers(0, 5000, (12000, 3)).astype(np.uint32)
    t[::6] = t[1::6][:, [1, 2, 0]]                                       # a rotation of every sixth, and
    t[2::6] = t[3::6][:, [0, 2, 1]]                                      # the other orientation of another
    every = t[5::6].reshape(-1)
    every[:5000] = rng.permutation(5000)                                 # every vertex is a member
    t[5::6] = every.reshape(-1, 3)
    plain = check_flags(Mesh(v, t), 1.0)[0]
    assert plain.counts[6] == 5000 and plain.counts[5] > 1900 and plain.counts[4] > 3800     # 10 001 slots: the claims probe past collisions


def test_70000_vertices_in_one_cell_with_sums_past_32_bits():
    v = np.zeros((70002, 4), F32)
    v[:, :3] = np.nextafter(F32(1), F32(0))                              # q = 2^24 - 1 on every axis: S = 70 000 (2^24 - 1) > 2^40
    v[70000, :3], v[70001, :3] = (1.5, 0.5, 0.5), (0.5, 1.5, 0.5)
    i = np.arange(70000)
    t = np.stack([i, np.roll(i, 1), np.roll(i, 2)], 1).astype(np.uint32)
    alone = check(Mesh(v[:70000], t), 1.0)
    assert alone.counts.tolist() == [0, 0, 0, 70000, 0, 0, 1, 0]         # one cluster; no triangle is left to use it
    used = check(Mesh(v, np.concatenate([t, S.u3([[69999, 70000, 70001]])])), 1.0)   # one triangle that does: the mean comes out
    assert used.counts.tolist() == [3, 1, 0, 70000, 0, 0, 3, 0] and used.vertices[0, :3].tolist() == [float(np.nextafter(F32(1), F32(0)))] * 3
    rng = np.random.default_rng(4)
    v[:70000, :3] = rng.uniform(0.9, 1.0, (70000, 3)).astype(F32) - F32(2.0 ** -24)
    check(Mesh(v, np.concatenate([t, S.u3([[3, 70000, 70001]])])), 1.0)


@pytest.mark.parametrize("cell", [0.5, 0.12, 0.05])
def test_soup_of_100000_triangles_over_70000_vertices(cell):
    v, t = S.soup(100000, 70000, 5, p_bad=0.01)
    v[::997, 0] = np.nan
    v[3::1009, 2] = np.inf
    v[7::1013, 1] = -3e9
    m = Mesh(v, t)
    plain = check(m, cell)
    assert plain.counts[2] > 2000 and plain.counts[7] > 100 and plain.counts[6] < 69000
    assert cell != 0.5 or (plain.counts[5] > 20000 and plain.counts[4] > 100 and plain.counts[3] > 1000)
    check(m, cell, KF | KD)


@pytest.mark.parametrize("name", ["sphere", "torus", "noise"])
def test_extracted_meshes_with_both_flags_in_all_combinations(name):
    mesh = S.mesh_named(name)
    m = Mesh(mesh.vertices, mesh.triangles)
    for factor in (1, 2):
        cell = factor * S.median_edge(name)
        for flags in ALL_FLAGS:
            check(m, cell, flags, want=S.simplified(name, cell, flags))
    check(m, 4 * S.median_edge(name), 0, want=S.simplified(name, 4 * S.median_edge(name)))
    check(m, 1e-6, KF, want=S.simplified(name, 1e-6, KF))


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_strips_of_20000_triangles_come_out_in_src_order(order):
    v, t = S.strip(20000, order)
    m = Mesh(v, t)
    for cell in (1.0, 0.75):
        for want in check_flags(m, cell, (0, KF)):
            assert (np.diff(want.vertex_src.astype(np.int64)) > 0).all() and len(want.vertex_src) > 3000 and len(want.triangles) > 3000


def test_one_case_past_the_grid_cap():
    V, T = GRID_CAP + 5003, GRID_CAP + 70001
    rng = np.random.default_rng(17)
    v = np.zeros((V, 4), F32)
    base = rng.uniform(-4.0, 4.0, (V // 4 + 1, 3))                       # four vertices in a row lie within 0.12 of each other
    v[:, :3] = base[np.arange(V) // 4] + rng.uniform(-0.06, 0.06, (V, 3))
    t = rng.integers(0, V, (T, 3)).astype(np.uint32)
    i = rng.integers(0, V - 2, len(t[2::9]))
    t[2::9] = np.stack([i, i + 1, i + 2], 1)                             # triangles of neighbours: many collapse
    t[1::9] = t[::9][:len(t[1::9]), [1, 2, 0]]                           # rotations: duplicates
    t[4::9] = t[3::9][:len(t[4::9]), [0, 2, 1]]                          # the other orientation: fins
    m = Mesh(v, t)
    want = check(m, 0.1)
    assert want.counts[6] > 100000 and min(want.counts[1:2].tolist() + want.counts[3:6].tolist()) > 10000
    assert want.kept[-1] >= GRID_CAP and want.vertex_src[-1] >= GRID_CAP  # the second trip of the grid-stride loops left its mark


# ------------------------------------------------------------------------------------------------ scratch, capacities, nullable outputs
def test_repeats_sizes_streams_and_released_scratch():
    small, big = Mesh(*S.soup(300, 200, 21, p_bad=0.03)), Mesh(*S.soup(60000, 50000, 22, p_bad=0.01))
    ws, wb = S.simplify(small.v, small.t, 0.3), S.simplify(big.v, big.t, 0.05)
    check(small, 0.3, want=ws)
    check(small, 0.3, want=ws)                                           # the same call twice
    check(big, 0.05, want=wb)                                            # a large call, then a small one in the same scratch
    check(small, 0.3, want=ws)
    check(small, 0.3, KD)                                                # no group table after one with it
    with torch.cuda.stream(torch.cuda.Stream()):
        check(small, 0.3, want=ws)
        check(big, 0.05, want=wb)
    assert capi.lib().dfusion_release_scratch() == 0
    check(small, 0.3, want=ws)


@pytest.mark.parametrize("caps", ["zero", "exact", "no vertices, half the triangles", "half the vertices, no triangles", "one short"])
def test_capacities_keep_their_guards(caps):
    name, cell = "sphere", 2 * S.median_edge("sphere")
    mesh, want = S.mesh_named(name), S.simplified(name, cell)
    m = Mesh(mesh.vertices, mesh.triangles)
    kv, kt = len(want.vertices), len(want.triangles)
    vcap, tcap = {"zero": (0, 0), "exact": (kv, kt), "no vertices, half the triangles": (0, kt // 2), "half the vertices, no triangles": (kv // 2, 0),
                  "one short": (kv - 1, kt - 1)}[caps]
    out_v, out_t, src, vmap, n = raw(m, cell, 0, vcap, tcap)             # (asserts the guard rows)
    assert np.array_equal(n, want.counts)                                # always the full numbers
    if tcap == kt:
        assert np.array_equal(u32(out_t[:kt]), want.triangles)
    if vcap == kv:
        assert np.array_equal(u32(src[:kv]), want.vertex_src) and np.array_equal(u32(out_v[:kv]), want.vertices.view(np.uint32))
    if caps != "zero":
        assert np.array_equal(u32(vmap[:m.V]), want.vertex_map)          # V entries whatever the capacities


def test_nullable_outputs():
    m = Mesh(*S.soup(5000, 3000, 9, p_bad=0.02))
    want = S.simplify(m.v, m.t, 0.2)
    kv, kt = len(want.vertices), len(want.triangles)
    for with_src, with_map in ((False, True), (True, False), (False, False)):
        out_v, out_t, src, vmap, n = raw(m, 0.2, 0, kv, kt, with_src=with_src, with_map=with_map)
        assert np.array_equal(n, want.counts) and np.array_equal(u32(out_t[:kt]), want.triangles)
        assert np.array_equal(u32(out_v[:kv]), want.vertices.view(np.uint32))
        assert not with_src or np.array_equal(u32(src[:kv]), want.vertex_src)
        assert not with_map or np.array_equal(u32(vmap[:m.V]), want.vertex_map)


# ------------------------------------------------------------------------------------------------ argument checks
def test_every_argument_check():
    L = capi.lib()
    t = dev_tri(np.array([[0, 1, 2]], np.uint32))
    v = dev_vtx(S.v4([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5]]))
    ov = torch.zeros((4, 4), dtype=torch.float32, device="cuda")
    ot = torch.zeros((4, 3), dtype=torch.int32, device="cuda")
    a = torch.zeros(8, dtype=torch.int32, device="cuda")
    b = torch.zeros(8, dtype=torch.int32, device="cuda")
    n = torch.zeros(8, dtype=torch.int64, device="cuda")
    big = 1 << 32
    good = lambda **kw: [kw.get("vtx", ptr(v)), kw.get("V", 3), kw.get("tri", ptr(t)), kw.get("T", 1), kw.get("cell", 1.0), kw.get("flags", 0),
                         kw.get("ov", ptr(ov)), kw.get("vcap", 3), kw.get("ot", ptr(ot)), kw.get("tcap", 1), kw.get("src", ptr(a)), kw.get("vmap", ptr(b)),
                         kw.get("counts", ptr(n)), None]
    assert L.dfusion_mesh_simplify(*good()) == 0
    torch.cuda.synchronize()
    assert n.tolist() == [3, 1, 0, 0, 0, 0, 3, 0] and u32(ot[:1]).tolist() == [[0, 1, 2]] and u32(a[:3]).tolist() == [0, 1, 2]
    bad_calls = [dict(vtx=None), dict(tri=None), dict(counts=None), dict(ov=None), dict(ot=None), dict(V=big), dict(T=big),
                 dict(cell=0.0), dict(cell=-1.0), dict(cell=float("nan")), dict(cell=float("inf")), dict(cell=-0.0), dict(flags=4), dict(flags=0x80000001),
                 dict(ov=ptr(v)), dict(ot=ptr(t)), dict(src=ptr(v)), dict(vmap=ptr(v)), dict(counts=ptr(v)), dict(vmap=ptr(t), V=1),
                 dict(ov=C.c_void_p(v.data_ptr() + 32)), dict(ot=C.c_void_p(t.data_ptr() + 8))]
    for bad in bad_calls:
        assert L.dfusion_mesh_simplify(*good(**bad)) == INVALID, bad
    assert L.dfusion_mesh_simplify(*good(ov=None, vcap=0, ot=None, tcap=0, src=None, vmap=None)) == 0      # counts only
    assert L.dfusion_mesh_simplify(*good(src=None, vmap=None)) == 0                                       # both nullable
    assert L.dfusion_mesh_simplify(*good(vtx=None, V=0, vmap=None)) == 0                                  # arrays of length 0 may be NULL
    torch.cuda.synchronize()
    assert n.tolist() == [0, 0, 1, 0, 0, 0, 0, 0]
    assert L.dfusion_mesh_simplify(*good(tri=None, T=0)) == 0
    assert L.dfusion_mesh_simplify(*good(flags=3)) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        simplify_mesh(v, torch.zeros((2, 3), dtype=torch.int64, device="cuda"), 1.0)
    with pytest.raises(ValueError):
        simplify_mesh(v[:, :3], t, 1.0)
    with pytest.raises(capi.DfusionError):
        simplify_mesh(v, t, 0.0)


# ------------------------------------------------------------------------------------------------ the Python mirror
def test_mirror_function_equals_the_restatement():
    mesh = S.mesh_named("noise")
    vd, td = dev_vtx(mesh.vertices), dev_tri(mesh.triangles)
    cell = S.median_edge("noise")
    for kf, kd in ((False, False), (True, False), (False, True), (True, True)):
        want = S.simplified("noise", cell, (KF if kf else 0) | (KD if kd else 0))
        gv, gt, gs, gm, gn = simplify_mesh(vd, td, cell, keep_first=kf, keep_duplicates=kd, return_counts=True)
        assert np.array_equal(u32(gv), want.vertices.view(np.uint32)) and np.array_equal(u32(gt), want.triangles)
        assert np.array_equal(u32(gs), want.vertex_src) and np.array_equal(u32(gm), want.vertex_map) and gn.tolist() == [int(c) for c in want.counts]
        assert gv.shape == (len(want.vertices), 4) and gt.shape == (len(want.triangles), 3) and gt.dtype == torch.int32 and gv.dtype == torch.float32
    assert len(simplify_mesh(vd, td, cell)) == 4 and mesh_ops.simplify_mesh is simplify_mesh
    e = simplify_mesh(vd, td[:0], cell)
    assert e[0].shape == (0, 4) and e[1].shape == (0, 3) and e[2].shape == (0,) and (u32(e[3]) == S.NONE).all() and e[3].shape == (len(mesh.vertices),)
    e = simplify_mesh(vd[:0], td[:0], cell, return_counts=True)
    assert e[3].shape == (0,) and e[4].tolist() == [0] * 8


def test_fetch_mesh_with_a_simplify_cell_on_a_fused_scene():
    from test_gpu_mesh_components import fused_scene
    import mesh_components_ref as M
    S_, vol, cv, wf, intr, ref = fused_scene()
    voxel = float(S_.sc.vs[0])
    v0, t0 = vol.fetchMesh()
    assert np.array_equal(u32(v0), ref.vertices.view(np.uint32)) and np.array_equal(u32(t0), ref.triangles)
    # 0.0: today's bytes, with and without the other arguments
    v1, t1, n1 = vol.fetchMesh(with_normals=True, simplify_cell=0.0)
    assert same_bits(v0, v1) and same_bits(t0, t1) and same_bits(n1, vol.fetchNormals(v0))
    f0, f1 = vol.fetchMesh(min_component_triangles=25), vol.fetchMesh(min_component_triangles=25, simplify_cell=0.0)
    assert same_bits(f0[0], f1[0]) and same_bits(f0[1], f1[1])
    # 2 voxels: the restatement applied to fetchMesh()
    cell = 2 * voxel
    want = S.simplify(ref.vertices, ref.triangles, cell)
    assert 100 < len(want.triangles) < len(ref.triangles) // 3 and want.counts[3] > 1000 and want.counts[6] < len(ref.vertices) // 3
    gv, gt = vol.fetchMesh(simplify_cell=cell)
    assert np.array_equal(u32(gv), want.vertices.view(np.uint32)) and np.array_equal(u32(gt), want.triangles)
    gv, gt, gn = vol.fetchMesh(with_normals=True, simplify_cell=cell)
    assert np.array_equal(u32(gv), want.vertices.view(np.uint32)) and np.array_equal(u32(gt), want.triangles)
    assert gn.shape == gv.shape and same_bits(gn, vol.fetchNormals(gv))
    assert vol.last_mesh_counts_ == (len(ref.vertices), len(ref.triangles))
    # after the component filter
    fv, ft, _ = M.remove_small(ref.vertices, ref.triangles, 25)
    want = S.simplify(fv, ft, cell)
    gv, gt = vol.fetchMesh(min_component_triangles=25, simplify_cell=cell)
    assert np.array_equal(u32(gv), want.vertices.view(np.uint32)) and np.array_equal(u32(gt), want.triangles)
