"""dfusion_mesh_components / dfusion_mesh_filter / dfusion_gather_rows and their Python mirror against the numpy restatement
tests/mesh_components_ref.py: every output and every count, by integer equality."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_components_ref as M
import mesh_ref as R
from dynamicfusion_amd import Intr, capi, frontend, mesh_components, mesh_ops, remove_small_components, synth
from mesh_gpu import dev_tri, ptr, same_bits, u32

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID = 100001
GUARD = 4                                            # guard rows behind every output
G32 = -7                                             # what they hold (0xfffffff9)


def raw_components(tri, V, with_count=True, with_counts=True, tri_dev=None):
    """dfusion_mesh_components into guarded buffers -> (label, triangle_count or None, counts or None) as numpy."""
    td = dev_tri(tri) if tri_dev is None else tri_dev
    T = int(td.shape[0])
    label = torch.full((V + GUARD,), G32, dtype=torch.int32, device="cuda")
    count = torch.full((V + GUARD,), G32, dtype=torch.int32, device="cuda")
    counts = torch.full((4 + GUARD,), 123, dtype=torch.int64, device="cuda")
    capi.check(capi.lib().dfusion_mesh_components(ptr(td) if T else None, T, V, ptr(label), ptr(count) if with_count else None,
                                                  ptr(counts) if with_counts else None, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "dfusion_mesh_components")
    torch.cuda.synchronize()
    assert (label[V:] == G32).all() and (count[V:] == G32).all() and (counts[4:] == 123).all()
    assert with_count or (count == G32).all()
    assert with_counts or (counts == 123).all()
    return u32(label[:V]), u32(count[:V]) if with_count else None, counts[:4].cpu().numpy().astype(np.uint64) if with_counts else None


def check_components(tri, V, **kw):
    label, count, counts = raw_components(tri, V, **kw)
    wl, wc, wn = M.components(tri, V)
    assert np.array_equal(label, wl), int((label != wl).sum())
    assert count is None or np.array_equal(count, wc)
    assert counts is None or np.array_equal(counts, wn), (counts, wn)
    return wl, wc, wn


def raw_filter(tri, V, label, count, min_triangles, keep_largest, tcap, vcap, with_map=True):
    """dfusion_mesh_filter into guarded buffers of the given capacities -> (triangles_out, vertex_src, vertex_map, counts) device tensors,
    guards included."""
    td = dev_tri(tri)
    T = int(td.shape[0])
    ld, cd = torch.from_numpy(label.view(np.int32).copy()).cuda(), torch.from_numpy(count.view(np.int32).copy()).cuda()
    out = torch.full((tcap + GUARD, 3), G32, dtype=torch.int32, device="cuda")
    src = torch.full((vcap + GUARD,), G32, dtype=torch.int32, device="cuda")
    vmap = torch.full((V + GUARD,), G32, dtype=torch.int32, device="cuda")
    counts = torch.full((2 + GUARD,), 123, dtype=torch.int64, device="cuda")
    capi.check(capi.lib().dfusion_mesh_filter(ptr(td) if T else None, T, V, ptr(ld) if V else None, ptr(cd) if V else None, min_triangles,
                                              int(keep_largest), ptr(out) if tcap else None, tcap, ptr(src) if vcap else None, vcap,
                                              ptr(vmap) if with_map else None, ptr(counts), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "dfusion_mesh_filter")
    torch.cuda.synchronize()
    assert (out[tcap:] == G32).all() and (src[vcap:] == G32).all() and (vmap[V:] == G32).all() and (counts[2:] == 123).all()
    return out, src, vmap, counts[:2].cpu().numpy().astype(np.uint64)


def check_filter(tri, V, min_triangles=0, keep_largest=False, components=None):
    """Count-only, then exact capacities: everything equals the restatement."""
    label, count, _ = components if components is not None else M.components(tri, V)
    want_t, want_src, want_map, want_n = M.mesh_filter(tri, V, label, count, min_triangles, keep_largest)
    out, src, vmap, n = raw_filter(tri, V, label, count, min_triangles, keep_largest, 0, 0)
    assert np.array_equal(n, want_n), (n, want_n)
    assert (vmap == G32).all()                                          # counts only: nothing else is written
    kv, kt = int(n[0]), int(n[1])
    out, src, vmap, n = raw_filter(tri, V, label, count, min_triangles, keep_largest, kt, kv)
    assert np.array_equal(n, want_n)
    assert np.array_equal(u32(out[:kt]), want_t) and np.array_equal(u32(src[:kv]), want_src)
    if kt or kv:
        assert np.array_equal(u32(vmap[:V]), want_map)
    else:
        assert (want_map == M.NONE).all() and (vmap == G32).all()       # nothing kept: exact capacities are 0 and 0, counts only again
    return want_t, want_src


def check_both(tri, V, thresholds=(0, 2), largest=(False, True)):
    comps = check_components(tri, V)
    for mt in thresholds:
        for kl in largest:
            check_filter(tri, V, mt, kl, comps)
    return comps


# ------------------------------------------------------------------------------------------------ hand-made cases and wave boundaries
@pytest.mark.parametrize("name,tri,V", M.small_cases(), ids=[c[0] for c in M.small_cases()])
def test_small_cases(name, tri, V):
    label, count, counts = check_both(tri, V, thresholds=(0, 2, 3))
    if name == "no triangle":
        assert counts.tolist() == [0, 5, 0, 0]
    if name == "aaa":
        assert count[4] == 2 and label[6] == 4 and label[2] == 2          # (a, a, a) connects nothing, counts for a's component
    if name.startswith("index"):
        assert counts.tolist() == [2, 0, 1, 2]


def test_two_components_of_equal_size_keep_the_smaller_label():
    cases = {c[0]: c[1:] for c in M.small_cases()}
    for name in ("two equal", "two equal, larger label first"):
        tri, V = cases[name]
        want_t, want_src = check_filter(tri, V, 0, True)
        assert want_src.tolist() == [0, 1, 2, 3] and want_t.tolist() == [[0, 1, 2], [1, 2, 3]]


# ------------------------------------------------------------------------------------------------ labels travel against the index order
@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_strips_of_20000_triangles(order):
    tri, V = M.strip(20000, order)
    label, count, counts = check_components(tri, V)
    assert (label == 0).all() and counts.tolist() == [1, 0, 0, 20000]
    rng = np.random.default_rng(3)
    check_components(tri[rng.permutation(len(tri))], V)                  # and with the triangles themselves in any order
    check_filter(tri, V, 20000, True, (label, count, counts))
    check_filter(tri, V, 20001, False, (label, count, counts))


@pytest.mark.parametrize("min_triangles,kept", [(3, 6000), (4, 0)])
def test_2000_components_of_exactly_3_triangles(min_triangles, kept):
    tri, V = M.islands(2000, 3)
    label, count, counts = check_components(tri, V)
    assert counts.tolist() == [2000, 0, 0, 3]
    want_t, _ = check_filter(tri, V, min_triangles, False, (label, count, counts))
    assert len(want_t) == kept
    check_filter(tri, V, min_triangles, True, (label, count, counts))   # 2000 components tie: label 0 wins


def test_soup_of_100000_triangles_over_70000_vertices():
    tri = M.soup(100000, 70000, 5, p_bad=0.01)
    label, count, counts = check_components(tri, 70000)
    assert counts[2] > 2000 and counts[3] > 65536 and counts[1] > 500 and label.max() > 65536      # nothing may be 16-bit
    for mt, kl in ((0, False), (2, False), (0, True)):
        check_filter(tri, 70000, mt, kl, (label, count, counts))
    sparse = M.soup(30000, 70000, 6)                                     # many components of a few triangles
    check_both(sparse, 70000, thresholds=(0, 2, 5))


# ------------------------------------------------------------------------------------------------ extracted meshes
@pytest.mark.parametrize("min_triangles", M.PLANTED_THRESHOLDS)
def test_planted_sphere_thresholds(min_triangles):
    m, label, count, counts = M.components_of("planted")
    V = len(m.vertices)
    check_components(m.triangles, V)
    want_t, _ = check_filter(m.triangles, V, min_triangles, False, (label, count, counts))
    assert len(want_t) == sum(s for s in M.PLANTED_SIZES if s >= min_triangles)
    check_filter(m.triangles, V, min_triangles, True, (label, count, counts))


@pytest.mark.parametrize("index", [2, 7, 8, 9])
def test_fuzz_meshes_with_unused_vertices_and_tiny_components(index):
    m, label, count, counts = M.components_of(("fuzz", index, 0.1))
    V = len(m.vertices)
    check_components(m.triangles, V)
    assert counts[1] > 0
    for mt, kl in ((0, False), (1, False), (5, False), (100, False), (0, True)):
        check_filter(m.triangles, V, mt, kl, (label, count, counts))


# ------------------------------------------------------------------------------------------------ nullable outputs, scratch, streams
def test_nullable_outputs():
    tri = M.soup(5000, 3000, 9, p_bad=0.02)
    check_components(tri, 3000, with_count=False)                        # the counts from a workspace copy of triangle_count
    check_components(tri, 3000, with_counts=False)
    check_components(tri, 3000, with_count=False, with_counts=False)     # labels only
    label, count, _ = M.components(tri, 3000)
    want = M.mesh_filter(tri, 3000, label, count, 3)
    out, src, vmap, n = raw_filter(tri, 3000, label, count, 3, False, int(want[3][1]), int(want[3][0]), with_map=False)
    assert (vmap == G32).all() and np.array_equal(u32(out[:len(want[0])]), want[0]) and np.array_equal(u32(src[:len(want[1])]), want[1])


def test_repeats_sizes_streams_and_released_scratch():
    small, big = M.soup(300, 200, 21, p_bad=0.03), M.soup(60000, 50000, 22, p_bad=0.01)
    check_both(small, 200)
    check_both(small, 200)                                               # the same call twice
    check_both(big, 50000, thresholds=(0, 3), largest=(False,))          # a large call, then a small one in the same scratch
    check_both(small, 200)
    with torch.cuda.stream(torch.cuda.Stream()):
        check_both(small, 200)
        check_both(big, 50000, thresholds=(3,), largest=(True,))
    assert capi.lib().dfusion_release_scratch() == 0
    check_both(small, 200)


@pytest.mark.parametrize("caps", ["zero", "one", "exact", "one short", "triangles only", "vertices only"])
def test_capacities_keep_their_guards(caps):
    m, label, count, _ = M.components_of("planted")
    V = len(m.vertices)
    want_t, want_src, want_map, want_n = M.mesh_filter(m.triangles, V, label, count, 100)
    kv, kt = len(want_src), len(want_t)
    tcap, vcap = {"zero": (0, 0), "one": (1, 1), "exact": (kt, kv), "one short": (kt - 1, kv - 1), "triangles only": (kt, 0),
                  "vertices only": (0, kv)}[caps]
    out, src, vmap, n = raw_filter(m.triangles, V, label, count, 100, False, tcap, vcap)       # (asserts the guard rows)
    assert np.array_equal(n, want_n)                                     # always the full numbers
    if tcap == kt:
        assert np.array_equal(u32(out[:kt]), want_t)
    if vcap == kv:
        assert np.array_equal(u32(src[:kv]), want_src)
    if caps != "zero":
        assert np.array_equal(u32(vmap[:V]), want_map)                   # V entries whatever the capacities


# ------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("row_bytes", [4, 12, 16])
def test_gather_rows_over_the_planted_spheres_vertex_src(row_bytes):
    m, label, count, _ = M.components_of("planted")
    V = len(m.vertices)
    _, src, _, _ = M.mesh_filter(m.triangles, V, label, count, 100)
    rng = np.random.default_rng(row_bytes)
    rows = {4: rng.integers(0, 256, (V, 4), dtype=np.uint8), 12: rng.standard_normal((V, 3)).astype(F32), 16: m.vertices}[row_bytes]
    n = len(src)
    sd, idx = torch.from_numpy(np.ascontiguousarray(rows)).cuda(), torch.from_numpy(src.view(np.int32).copy()).cuda()
    dst = torch.full((n + GUARD,) + rows.shape[1:], 7, dtype=sd.dtype, device="cuda")
    capi.check(capi.lib().dfusion_gather_rows(ptr(sd), row_bytes, ptr(idx), n, ptr(dst), None), "dfusion_gather_rows")
    torch.cuda.synchronize()
    assert dst[:n].cpu().numpy().tobytes() == rows[src].tobytes() and (dst[n:] == 7).all()
    assert mesh_ops.gather_rows(sd, idx).cpu().numpy().tobytes() == rows[src].tobytes()
    assert capi.lib().dfusion_gather_rows(None, row_bytes, None, 0, None, None) == 0               # n == 0: nothing


# ------------------------------------------------------------------------------------------------ argument checks
def test_every_argument_check():
    L = capi.lib()
    t = dev_tri(np.array([[0, 1, 2]], np.uint32))
    a = torch.zeros(8, dtype=torch.int32, device="cuda")
    b = torch.zeros(8, dtype=torch.int32, device="cuda")
    n = torch.zeros(4, dtype=torch.int64, device="cuda")
    o = torch.zeros((4, 3), dtype=torch.int32, device="cuda")
    big = 1 << 32
    assert L.dfusion_mesh_components(None, 1, 3, ptr(a), ptr(b), ptr(n), None) == INVALID          # triangles
    assert L.dfusion_mesh_components(ptr(t), 1, 3, None, ptr(b), ptr(n), None) == INVALID           # labels
    assert L.dfusion_mesh_components(ptr(t), 1, big, ptr(a), ptr(b), ptr(n), None) == INVALID       # V > 2^32 - 1
    assert L.dfusion_mesh_components(ptr(t), big, 3, ptr(a), ptr(b), ptr(n), None) == INVALID
    assert L.dfusion_mesh_components(ptr(t), 1, 3, ptr(a), None, None, None) == 0                   # both nullable
    good = lambda **kw: [kw.get("tri", ptr(t)), kw.get("T", 1), kw.get("V", 3), kw.get("label", ptr(a)), kw.get("count", ptr(b)), 0, 0,
                         kw.get("out", ptr(o)), kw.get("tcap", 1), kw.get("src", ptr(o)), kw.get("vcap", 3), kw.get("vmap", None),
                         kw.get("counts", ptr(n)), None]
    assert L.dfusion_mesh_filter(*good()) == 0
    for bad in (dict(tri=None), dict(label=None), dict(count=None), dict(counts=None), dict(V=big), dict(T=big), dict(out=None),
                dict(src=None)):
        assert L.dfusion_mesh_filter(*good(**bad)) == INVALID, bad
    assert L.dfusion_mesh_filter(*good(out=None, tcap=0, src=None, vcap=0)) == 0                    # counts only
    for rb in (0, 1, 2, 3, 8, 20, 32):
        assert L.dfusion_gather_rows(ptr(a), rb, ptr(b), 2, ptr(n), None) == INVALID, rb
    assert L.dfusion_gather_rows(None, 4, ptr(b), 2, ptr(n), None) == INVALID
    assert L.dfusion_gather_rows(ptr(a), 4, None, 2, ptr(n), None) == INVALID
    assert L.dfusion_gather_rows(ptr(a), 4, ptr(b), 2, None, None) == INVALID
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        mesh_components(torch.zeros((2, 3), dtype=torch.int64, device="cuda"), 3)
    with pytest.raises(ValueError):
        mesh_ops.gather_rows(torch.zeros((4, 2), dtype=torch.float32, device="cuda"), a)            # rows of 8 bytes
    with pytest.raises(ValueError):
        remove_small_components(torch.zeros((3, 4), device="cuda"), t, attributes=(torch.zeros((2, 4), device="cuda"),))


# ------------------------------------------------------------------------------------------------ the Python mirror
def test_mirror_functions_equal_the_restatement():
    m, label, count, counts = M.components_of("planted")
    V = len(m.vertices)
    td, vd = dev_tri(m.triangles), torch.from_numpy(m.vertices).cuda()
    gl, gc, gn = mesh_components(td, V, return_counts=True)
    assert np.array_equal(u32(gl), label) and np.array_equal(u32(gc), count) and gn.tolist() == [int(c) for c in counts]
    assert len(mesh_components(td, V)) == 2
    rng = np.random.default_rng(8)
    colors, weights = rng.integers(0, 256, (V, 4), dtype=np.uint8), rng.standard_normal(V).astype(F32)
    for mt, kl in ((145, False), (0, True), (9957, False)):
        want_v, want_t, want_src = M.remove_small(m.vertices, m.triangles, mt, kl)
        gv, gt, (ga, gw), gs = remove_small_components(vd, td, mt, kl, attributes=(torch.from_numpy(colors).cuda(), torch.from_numpy(weights).cuda()))
        assert gv.cpu().numpy().tobytes() == want_v.tobytes() and np.array_equal(u32(gt), want_t) and np.array_equal(u32(gs), want_src)
        assert np.array_equal(ga.cpu().numpy(), colors[want_src]) and gw.cpu().numpy().tobytes() == weights[want_src].tobytes()
        assert gv.shape == (len(want_src), 4) and gt.shape == (len(want_t), 3) and gt.dtype == torch.int32
    e = remove_small_components(vd[:0], td[:0], 5)
    assert e[0].shape == (0, 4) and e[1].shape == (0, 3) and e[2] == () and e[3].shape == (0,)


def fused_scene():
    """The fused 32^3 scene of tests/test_gpu_render_mesh.py: volume, colour volume, warp field, the restatement's mesh."""
    import color_ref as CR
    from dynamicfusion_amd import ColorVolume, WarpField
    from test_gpu_color import dense, gpu_volume
    S = CR.scene(32, 80, 60, nodes=64, k=4)
    sc, intr = S.sc, Intr(*S.cfg.intr)
    vol = gpu_volume(S, 2)
    cv = ColorVolume(vol)
    for f in range(3):
        vol.upload(S.vols[f])
        cv.integrate(dense(S.images[f]), dense(sc.dists[f]), sc.cam_poses[f], intr)
    wf = WarpField(k=4, voxel_table=False, weight_table=False)
    wf.init(sc.pos, sigma=sc.sigma, transforms=sc.dqs[2])
    ref = R.extract_mesh(S.vols[2], S.cfg.dims, sc.vs, synth.aff12(sc.pose))
    return S, vol, cv, wf, intr, ref


def test_fetch_mesh_and_render_live_model_on_a_fused_scene():
    import color_ref as CR
    import oracle_lib as O
    import render_ref as RR
    S, vol, cv, wf, intr, ref = fused_scene()
    sc, cfg = S.sc, S.cfg
    sizes = sorted(int(c) for c in M.components(ref.triangles, len(ref.vertices))[1] if c)
    assert len(sizes) >= 3 and sizes[0] < 25 < sizes[-1]                 # the threshold drops something and keeps something
    # with the defaults: today's bits (the unfiltered mesh, twice; explicit defaults are the defaults)
    v0, t0 = vol.fetchMesh()
    assert np.array_equal(u32(v0), ref.vertices.view(np.uint32)) and np.array_equal(u32(t0), ref.triangles)
    v1, t1, n1 = vol.fetchMesh(with_normals=True, min_component_triangles=0, keep_largest=False)
    assert same_bits(v0, v1) and same_bits(t0, t1) and same_bits(n1, vol.fetchNormals(v0))
    for mt, kl in ((25, False), (0, True), (10 ** 9, False)):
        want_v, want_t, _ = M.remove_small(ref.vertices, ref.triangles, mt, kl)
        gv, gt, gn = vol.fetchMesh(with_normals=True, min_component_triangles=mt, keep_largest=kl)
        assert np.array_equal(u32(gv), want_v.view(np.uint32)) and np.array_equal(u32(gt), want_t)
        assert gn.shape == gv.shape and (not len(want_v) or same_bits(gn, vol.fetchNormals(gv))) and vol.last_mesh_counts_ == (len(ref.vertices), len(ref.triangles))
    # renderLiveModelFiltered: the defaults give what renderLiveModel gives, the threshold what the restatements give
    pose = sc.cam_poses[2]
    plain = frontend.renderLiveModel(vol, wf, pose, intr, cfg.cols, cfg.rows, color_volume=cv, k=4)
    zero = frontend.renderLiveModelFiltered(vol, wf, pose, intr, cfg.cols, cfg.rows, color_volume=cv, k=4)
    assert all(same_bits(a, b) for a, b in zip(plain, zero))
    got = frontend.renderLiveModelFiltered(vol, wf, pose, intr, cfg.cols, cfg.rows, color_volume=cv, k=4, min_component_triangles=25)
    want_v, want_t, _ = M.remove_small(ref.vertices, ref.triangles, 25)
    aff = synth.aff12(sc.pose)
    rinv = np.linalg.inv(sc.pose[:3, :3].astype(np.float64)).astype(F32)
    normals = O.extract_normals(sc.ovol(S.vols[2]), aff, rinv, want_v, vol.gradient_delta_factor_)
    colors = CR.fetch(cv.download(), cfg.dims, sc.vs, S.world2vol, want_v)
    wp, wn = O.warp_points(sc.pos, sc.dqs[2], sc.sigma, want_v[:, :3], normals[:, :3], 4)
    warped = np.zeros_like(want_v); warped[:, :3] = wp
    wnormals = np.zeros_like(want_v); wnormals[:, :3] = wn
    world2cam = synth.aff12(np.linalg.inv(np.asarray(pose, np.float64)).astype(F32))
    want = RR.render(warped, want_t, cfg.cols, cfg.rows, cfg.intr, world2cam=world2cam, normals=wnormals, attr=want_v, colors=colors)
    for k, g in zip(("points", "normals", "attr", "colors"), got):
        g = g.cpu().numpy()
        g = g.view(np.uint32) if g.dtype == np.float32 else g
        assert np.array_equal(g, want[k]), (k, int((g != want[k]).any(-1).sum()))
    assert (want["tri"] >= 0).sum() > 500
