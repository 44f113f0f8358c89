"""dfusion_warp_extend / WarpField.extend on the GPU, bit for bit:

  1. the rule: appended positions, transforms, dg_w, n_added and n_winners equal extend_ref (tests/extend_ref.py) -- NaN points,
     points 15+ sigma from every node (the zero-weight fallback), max_new truncation, an all-supported cloud that changes nothing;
  2. the handle after extend (brick lists re-made, only stale table blocks re-made) equals a fresh handle given the grown set
     (set_nodes + build_index): index info, k-NN, warp_points,
     three warped integrates from the same volume (tables on demand, eager, none; cull off; prepare / sweep split) and the solver;
  3. the volume after extend + 2 frames equals the oracle's warped integrate with the grown node set;
  4. exact distance ties: tables over a 32^3 lattice, then growth on lattice sites (the blocks whose build met a tie are re-made);
  5. growth across the node-count dispatch boundaries (5120, 8192) and up to the 65 535-node cap;
  6. a plan prepared before extend is void; two runs give the same bits;
  7. the C++ mirror's WarpField::extend equals the Python path."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

import extend_ref as X
import oracle_lib as O
from dynamicfusion_amd import Intr, TsdfVolume, WarpField, build, capi, synth, upload_u16

pytestmark = pytest.mark.gpu
F32 = np.float32
DF_E_INVALID = 100001

DIMS, SIZE, TRUNC = (64, 64, 64), 1.0, 0.04
POSE = synth.translation(-0.5, -0.5, 0.4)                    # z in [0.4, 1.4]
INTR = (F32(120.0), F32(120.0), F32(64.0), F32(48.0))
COLS, ROWS = 128, 96
RADIUS = 0.08


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, F32)).cuda()


def wall_depth(phase):
    u, v = np.meshgrid(np.arange(COLS), np.arange(ROWS))
    z = 0.9 + 0.05 * np.sin(u / 17.0 + phase) * np.cos(v / 13.0 - phase)
    return np.rint(z * 1000).astype(np.uint16)


def cam(f):
    return synth.rot_y_about(0.02 * f, [0.0, 0.0, 0.9])


def tw(M, f):
    rng = np.random.default_rng(1000 + f)
    return synth.dq_from_twist(rng.uniform(-0.05, 0.05, (M, 3)).astype(F32), rng.uniform(-0.01, 0.01, (M, 3)).astype(F32))


def half_nodes(rng, M=256):
    """A jittered lattice over the volume's x < 0 half only: surface at x > 0.25 m has no node within sigma."""
    n = int(np.ceil((2 * M) ** (1 / 3)))
    s = 1.0 / n
    g = np.stack(np.meshgrid(np.arange(n // 2), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3)
    g = g[rng.permutation(len(g))[:M]]
    pos = (np.array([-0.5, -0.5, 0.4]) + (g + 0.5 + rng.uniform(-0.3, 0.3, g.shape)) * s).astype(F32)
    return pos, np.full(len(pos), 1.5 * s, F32)


def surface_points(rng, n=4000):
    p = np.empty((n, 3), F32)
    p[:, 0] = rng.uniform(-0.45, 0.45, n); p[:, 1] = rng.uniform(-0.45, 0.45, n)
    p[:, 2] = 0.9 + 0.05 * np.sin(p[:, 0] * 3.0) * np.cos(p[:, 1] * 5.0)
    p[::97, 1] = np.nan
    return p


def new_volume(dims=DIMS, size=SIZE, pose=POSE):
    v = TsdfVolume(dims); v.setSize([size] * 3); v.setTruncDist(TRUNC); v.setMaxWeight(64); v.setPose(pose)
    return v


def index_info(wf):
    t, nb, k = C.c_ulonglong(0), C.c_uint(0), C.c_int(0)
    capi.check(capi.lib().dfusion_warp_index_info(wf.handle, C.byref(t), C.byref(nb), C.byref(k)), "dfusion_warp_index_info")
    return t.value, nb.value, k.value


def grown(pos, sigma, dq_last, wf):
    npos, ndq, nsig = (t.cpu().numpy() for t in wf.new_nodes)
    return np.concatenate([pos, npos]), np.concatenate([sigma, nsig]), np.concatenate([dq_last, ndq])


def check_points_equal(A, B, k, queries):
    ia, da = A.KNN(dev(queries), k)
    ib, db = B.KNN(dev(queries), k)
    pa, pb = dev(queries), dev(queries)
    na, nb = dev(np.tile([0.0, 0.0, 1.0], (len(queries), 1))), dev(np.tile([0.0, 0.0, 1.0], (len(queries), 1)))
    A.warp(pa, na, k=k); B.warp(pb, nb, k=k)
    torch.cuda.synchronize()
    assert np.array_equal(ia.cpu().numpy(), ib.cpu().numpy()) and np.array_equal(bits(da.cpu().numpy()), bits(db.cpu().numpy()))
    assert np.array_equal(bits(pa.cpu().numpy()), bits(pb.cpu().numpy())) and np.array_equal(bits(na.cpu().numpy()), bits(nb.cpu().numpy()))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the rule
@pytest.mark.parametrize("indexed", [False, True], ids=["scan", "index"])
@pytest.mark.parametrize("k", [4, 8])
def test_rule_equals_extend_ref(k, indexed):
    rng = np.random.default_rng(7 + k)
    pos, sigma = half_nodes(rng)
    M = len(pos)
    dq = tw(M, 1)
    pts = surface_points(rng)
    far = np.array([[6.0, 0.0, 1.0], [6.0, 3.0, 1.0], [-6.0, -3.0, 2.0]], F32)        # > 15 sigma from every node
    pts = np.concatenate([pts, far, pts[:50]])                   # (repeats lose their cells to the first copies)
    for max_new in (None, 9):
        wf = WarpField(k=k)
        wf.init(pos, sigma=sigma, transforms=tw(M, 0))
        wf.set_transforms(dev(dq))
        if indexed:
            wf.ensure_index(new_volume(), k)
        n, w = wf.extend(dev(pts), RADIUS, sigma=0.07, max_new=max_new)
        torch.cuda.synchronize()
        r_pos, r_dq, r_sig, r_n, r_w = X.extend_ref(pos, dq, sigma, pts, k, RADIUS, 0.07, max_new)
        assert (n, w) == (r_n, r_w) and n > 0
        assert wf.M == M + n
        g_pos, g_dq, g_sig = (t.cpu().numpy() for t in wf.new_nodes)
        assert np.array_equal(bits(g_pos), bits(r_pos)) and np.array_equal(bits(g_sig), bits(r_sig))
        bad = (bits(g_dq) != bits(r_dq)).any(1)
        assert not bad.any(), "%d of %d transforms differ" % (int(bad.sum()), n)
        assert np.isfinite(g_dq).all()
        if max_new is None:
            assert n > 20 and any((g_pos == f).all(1).any() for f in far)     # the far points are nodes, with finite transforms
        else:
            assert n == 9 and w > 9


def test_all_supported_cloud_changes_nothing():
    rng = np.random.default_rng(5)
    pos, sigma = half_nodes(rng)
    M = len(pos)
    intr = Intr(*INTR)
    hs = [WarpField(k=8) for _ in range(2)]
    vols = [new_volume() for _ in range(2)]
    d = upload_u16(O.compute_dists(wall_depth(0.0), np.array(INTR, F32)))
    for h, v in zip(hs, vols):
        h.init(pos, sigma=sigma, transforms=tw(M, 0)); v.clear()
        v.integrate_warped(d, cam(0), intr, h)
    pts = (pos + F32(0.1) * sigma[:, None]).astype(F32)         # every point within its nearest node's sigma
    assert hs[0].extend(dev(pts), RADIUS) == (0, 0)
    assert hs[0].extend(dev(np.zeros((0, 3), F32)), RADIUS) == (0, 0)
    assert hs[0].M == M
    for h, v in zip(hs, vols):
        h.set_transforms(dev(tw(M, 1)))
        v.integrate_warped(d, cam(1), intr, h)
    torch.cuda.synchronize()
    assert np.array_equal(vols[0].download(), vols[1].download())
    check_points_equal(hs[0], hs[1], 8, surface_points(rng, 500)[1:])


def test_invalid_arguments():
    wf = WarpField(k=8)
    wf.init(np.random.default_rng(0).uniform(0, 1, (6, 3)).astype(F32), sigma=0.1)
    L, p, n, w = capi.lib(), dev(np.zeros((4, 3), F32)), C.c_int(0), C.c_int(0)
    for k, r, s, mx in ((8, 0.1, 0.1, 10), (0, 0.1, 0.1, 10), (9, 0.1, 0.1, 10), (4, 0.0, 0.1, 10), (4, float("inf"), 0.1, 10),
                        (4, float("nan"), 0.1, 10), (4, 0.1, float("nan"), 10), (4, 0.1, 0.1, -1)):
        assert L.dfusion_warp_extend(wf.handle, k, C.c_void_p(p.data_ptr()), 4, r, s, mx, None, None, None, C.byref(n), C.byref(w), None) == DF_E_INVALID


# ---------------------------------------------------------------------------------------------------------------------------------
# 2 + 3. the handle after extend == a fresh handle with the grown set
MODES = {
    "on_demand": dict(wf=dict(), integ=dict()),
    "eager": dict(wf=dict(tables_on_demand=False), integ=dict()),
    "no_table": dict(wf=dict(voxel_table=False), integ=dict()),
    "cull_off": dict(wf=dict(), integ=dict(cull=False)),
    "split": dict(wf=dict(), integ=None),
}


def integrate(v, d, f, wf, k, mode):
    if MODES[mode]["integ"] is None:
        v.integrate_warped_prepare(d, cam(f), Intr(*INTR), wf, k=k)
        v.integrate_warped_sweep(wf, sync=False)
    else:
        v.integrate_warped(d, cam(f), Intr(*INTR), wf, k=k, **MODES[mode]["integ"])


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("k", [4, 8])
def test_extend_equals_full_rebuild(k, mode):
    rng = np.random.default_rng(40 + k)
    pos, sigma = half_nodes(rng)
    M = len(pos)
    proj = np.array(INTR, F32)
    dists = [O.compute_dists(wall_depth(0.4 * f), proj) for f in range(6)]
    A = WarpField(k=k, **MODES[mode]["wf"])
    A.init(pos, sigma=sigma, transforms=tw(M, 0))
    va = new_volume(); va.clear()
    for f in range(3):
        A.set_transforms(dev(tw(M, f + 1)))
        integrate(va, upload_u16(dists[f]), f, A, k, mode)
    key = A._index_key
    n, _ = A.extend(dev(surface_points(rng)), RADIUS)
    assert n > 10 and A._index_key == key
    gpos, gsig, gdq = grown(pos, sigma, tw(M, 3), A)
    B = WarpField(k=k, **MODES[mode]["wf"])
    B.init(gpos, sigma=gsig, transforms=gdq)
    vb = new_volume(); vb.upload(va.download())
    B.ensure_index(vb, k)
    assert index_info(A) == index_info(B)
    q = np.concatenate([surface_points(rng, 2000)[1:], gpos[M:] + F32(0.01)]).astype(F32)
    check_points_equal(A, B, k, q)
    start = va.download()
    for f in range(3, 6):
        dq = tw(M + n, f + 1)
        A.set_transforms(dev(dq)); B.set_transforms(dev(dq))
        integrate(va, upload_u16(dists[f]), f, A, k, mode)
        integrate(vb, upload_u16(dists[f]), f, B, k, mode)
        torch.cuda.synchronize()
        a, b = va.download(), vb.download()
        assert (a >> 16).any() and np.array_equal(a, b), "frame %d: %d voxels differ" % (f, int((a != b).sum()))
        if f == 4 and mode == "on_demand":                     # 3. the oracle: two frames after extend, with the grown set
            ref = start.copy()
            vs = np.array([F32(SIZE) / F32(x) for x in DIMS], F32)
            for g in (3, 4):
                O.integrate_warped(dists[g], ref, O.make_volume(ref, DIMS, vs, TRUNC, 64), synth.aff12(POSE),
                                   synth.aff12(synth.affine_inv(cam(g))), proj, gpos, tw(M + n, g + 1), gsig, k)
            assert np.array_equal(a, ref), "oracle: %d voxels differ" % int((a != ref).sum())
    src = surface_points(rng, 1500)[1:]
    dst = (src + F32(0.01)).astype(F32)
    qa, ea = A.energy_data(dev(src), dev(dst), iters=10, k=k)
    qb, eb = B.energy_data(dev(src), dev(dst), iters=10, k=k)
    torch.cuda.synchronize()
    assert np.array_equal(bits(qa.cpu().numpy()), bits(qb.cpu().numpy())) and np.array_equal(bits(ea.cpu().numpy()), bits(eb.cpu().numpy()))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. exact ties: a 32^3 lattice with a missing slab, grown on the missing lattice sites
@pytest.mark.parametrize("on_demand", [True, False], ids=["on_demand", "eager"])
def test_tie_lattice_grown_on_lattice_sites(on_demand):
    """Tables made over a 32^3 lattice (exact ties everywhere) before the growth; the new nodes fill the missing x >= 24/32 columns.  Far
    from them the brick lists do not change, but the rebuilt tie tree orders the equidistant old nodes differently: only the blocks whose
    table build met a tie are re-made, and the handle equals a fresh one."""
    rng = np.random.default_rng(32)
    g = np.stack(np.meshgrid(*[np.arange(32)] * 3, indexing="ij"), -1).reshape(-1, 3)
    g = g[rng.permutation(len(g))]
    have = g[:, 0] < 24
    pos = (g[have] / 32.0).astype(F32)
    sites = (g[~have] / 32.0).astype(F32)
    M = len(pos)
    k = 8
    pose = synth.translation(-0.25, -0.25, -0.25)
    c = rng.integers(0, 31, (6000, 3)) + 0.5
    c[::2, 0] -= 0.5
    q = (c / 32.0).astype(F32)
    cam_pose = synth.translation(0.5, 0.5, -1.0)
    d = upload_u16(O.compute_dists(np.full((ROWS, COLS), 1500, np.uint16), np.array(INTR, F32)))
    A = WarpField(k=k, tables_on_demand=on_demand)
    A.init(pos, sigma=0.02, transforms=tw(M, 0))
    va = new_volume((64, 64, 64), 1.5, pose); va.clear()
    for f in range(2):                                       # tables (and, on the second sweep, blend models) of the old set
        va.integrate_warped(d, cam_pose, Intr(*INTR), A, k=k, cull=False)
    n, w = A.extend(dev(sites), 1.0 / 32, sigma=0.02)
    assert n == w == len(sites)
    B = WarpField(k=k, tables_on_demand=on_demand)
    B.init(np.concatenate([pos, sites]), sigma=0.02, transforms=np.concatenate([tw(M, 0), A.new_nodes[1].cpu().numpy()]))
    vb = new_volume((64, 64, 64), 1.5, pose); vb.upload(va.download())
    B.ensure_index(vb, k)
    assert index_info(A) == index_info(B)
    r_idx, _ = O.knn(np.concatenate([pos, sites]), q, k)
    assert (r_idx != O.knn(np.concatenate([pos, sites]), q, k, brute=True)[0]).any(1).sum() > 1000
    check_points_equal(A, B, k, q)
    ia, _ = A.KNN(dev(q), k)
    assert np.array_equal(ia.cpu().numpy(), r_idx)
    for f in range(3):
        dq = tw(M + n, f + 1)
        for wf, v in ((A, va), (B, vb)):
            wf.set_transforms(dev(dq))
            v.integrate_warped(d, cam_pose, Intr(*INTR), wf, k=k, cull=(f != 1))
        torch.cuda.synchronize()
        a, b = va.download(), vb.download()
        assert (a >> 16).any() and np.array_equal(a, b), "frame %d: %d voxels differ" % (f, int((a != b).sum()))


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. growth across the dispatch boundaries, up to 65 535 nodes
DENSE_DIMS = (96, 96, 96)


@pytest.mark.parametrize("M0,k", [(5000, 4), (8100, 8), (65400, 8)])
def test_growth_across_node_count_boundaries(M0, k):
    rng = np.random.default_rng(M0)
    n = int(np.ceil(M0 ** (1 / 3)))
    g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3)
    g = g[rng.permutation(len(g))[:M0]]
    s = 1.0 / n
    pos = (np.array([-0.5, -0.5, 0.4]) + (g * np.array([0.8, 1.0, 1.0]) + 0.5 + rng.uniform(-0.3, 0.3, g.shape)) * s).astype(F32)
    sigma = np.full(M0, 1.5 * s, F32)
    dq = tw(M0, 0)
    pts = np.empty((3000, 3), F32)
    pts[:, 0] = rng.uniform(0.35, 0.5, 3000); pts[:, 1] = rng.uniform(-0.5, 0.5, 3000); pts[:, 2] = rng.uniform(0.4, 1.4, 3000)
    vol = new_volume(DENSE_DIMS)
    A = WarpField(k=k)
    A.init(pos, sigma=sigma, transforms=dq)
    A.ensure_index(vol, k)
    n_add, w = A.extend(dev(pts), 0.05, sigma=float(1.5 * s))
    r_pos, r_dq, r_sig, r_n, r_w = X.extend_ref(pos, dq, sigma, pts, k, 0.05, float(1.5 * s))
    assert (n_add, w) == (r_n, r_w)
    g_pos, g_dq, _ = (t.cpu().numpy() for t in A.new_nodes)
    assert np.array_equal(bits(g_pos), bits(r_pos)) and np.array_equal(bits(g_dq), bits(r_dq))
    boundary = {5000: 5120, 8100: 8192, 65400: 65535}[M0]
    assert M0 + n_add >= boundary
    if M0 == 65400:
        assert A.M == 65535 and w > n_add
    B = WarpField(k=k)
    B.init(np.concatenate([pos, r_pos]), sigma=np.concatenate([sigma, r_sig]), transforms=np.concatenate([dq, r_dq]))
    vb = new_volume(DENSE_DIMS)
    B.ensure_index(vb, k)
    assert index_info(A) == index_info(B)
    q = np.concatenate([pts[:2000], r_pos + F32(0.004)]).astype(F32)
    check_points_equal(A, B, k, q)
    d = upload_u16(O.compute_dists(wall_depth(0.0), np.array(INTR, F32)))
    dqg = tw(A.M, 1)
    for wf, v in ((A, vol), (B, vb)):
        v.clear(); wf.set_transforms(dev(dqg))
        for _ in range(2):
            v.integrate_warped(d, cam(0), Intr(*INTR), wf, k=k)
    torch.cuda.synchronize()
    a, b = vol.download(), vb.download()
    assert (a >> 16).any() and np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. a prepared plan is void after extend; runs repeat
def test_prepared_plan_is_void_after_extend_and_runs_repeat():
    outs = []
    for rep in range(2):
        rng = np.random.default_rng(77)
        pos, sigma = half_nodes(rng)
        M = len(pos)
        wf = WarpField(k=8)
        wf.init(pos, sigma=sigma, transforms=tw(M, 0))
        v = new_volume(); v.clear()
        d = upload_u16(O.compute_dists(wall_depth(0.0), np.array(INTR, F32)))
        v.integrate_warped(d, cam(0), Intr(*INTR), wf)
        v.integrate_warped_prepare(d, cam(1), Intr(*INTR), wf)
        n, _ = wf.extend(dev(surface_points(rng)), RADIUS)
        assert n > 0
        rc = capi.lib().dfusion_integrate_warped_sweep(v.c_volume(), v.c_slab(), wf.handle, None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == DF_E_INVALID
        wf.set_transforms(dev(tw(wf.M, 2)))
        v.integrate_warped(d, cam(2), Intr(*INTR), wf)
        torch.cuda.synchronize()
        outs.append((v.download(), [t.cpu().numpy() for t in wf.new_nodes]))
    assert np.array_equal(outs[0][0], outs[1][0])
    for a, b in zip(outs[0][1], outs[1][1]):
        assert np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the C++ mirror
def test_cxx_warp_field_extend_equals_python(tmp_path):
    build.build_host()
    rng = np.random.default_rng(9)
    pos, sigma = half_nodes(rng)
    M, k = len(pos), 8
    dq = tw(M, 3)
    pts = surface_points(rng, 3000)
    fin, fout = str(tmp_path / "ext_in.bin"), str(tmp_path / "ext_out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([M, len(pts), k], np.uint32).tobytes()); f.write(np.array([RADIUS, 0.06], F32).tobytes())
        f.write(pos.tobytes()); f.write(dq.tobytes()); f.write(sigma.tobytes()); f.write(pts.tobytes())
    r = subprocess.run([build.HOST_WARP_TESTS, "extend", fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "warp_tests extend ok" in r.stdout, r.stdout + r.stderr
    raw = np.fromfile(fout, np.uint8)
    total, added = raw[:8].view(np.uint32)
    nodes = raw[8:].view(F32).reshape(total, 12)
    wf = WarpField(k=k)
    wf.init(pos, sigma=sigma, transforms=dq)
    n, _ = wf.extend(dev(pts), RADIUS, sigma=0.06)
    assert added == n > 0 and total == M + n
    gpos, gsig, gdq = grown(pos, sigma, dq, wf)
    assert np.array_equal(bits(nodes[:, :3]), bits(gpos)) and np.array_equal(bits(nodes[:, 3:11]), bits(gdq))
    assert np.array_equal(bits(nodes[:, 11]), bits(gsig))
