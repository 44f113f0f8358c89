"""Node sets at every node-count dispatch boundary, up to the C-ABI's 65 535 nodes, against the oracle bit for bit:

  * the data-term solve (dfusion_solver.hip): the CG step kernels df_sv_step_reg_kernel<2 / 5 / 8> and df_sv_step_kernel (M <= 2048,
    <= 5120, <= 8192, larger), W p with a compile-time k (4, 8) and with a run-time one (df_sv_w_apply_kernel<0>: every other k);
  * node packing (dfusion_warp_nodes.hip df_warp_pack_current): the one-workgroup pack + bounds (M <= 8192) and the pack + atomic bounds
    (M > 8192) with the sigma bound forced to "unknown", switched both ways on one handle, and the cull built on those bounds;
  * the brick index's super-brick gather past its LDS list (DF_SUPER_CAP = 1024 candidates: every brick scans all M nodes);
  * 16-bit node ids up to 65 534 in the brick lists, the per-voxel tables, the tie tree and the block models;
  * exact distance ties in a 32^3 lattice, where the tree that orders them is 13 levels deep.
Node sets are made here with numpy (jittered lattices, sigma about twice the spacing), volumes are 64^3 - 96^3 so that the
single-threaded parts of the oracle stay fast."""
import numpy as np
import pytest
import torch

import oracle_lib as O
from dynamicfusion_amd import Intr, TsdfVolume, WarpField, synth, upload_u16

pytestmark = pytest.mark.gpu
F32 = np.float32
SUPER_CAP = 1024                       # DF_SUPER_CAP, dfusion_warp_index.hip


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def jittered_lattice(M, lo, hi, rng, jitter=0.3):
    """M nodes on a jittered cubic lattice filling the box [lo, hi]^3, in a random index order.  Returns (pos, spacing)."""
    n = int(np.ceil(M ** (1 / 3)))
    s = (hi - lo) / n
    g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3)
    g = g[rng.permutation(len(g))[:M]]
    pos = lo + (g + 0.5 + rng.uniform(-jitter, jitter, g.shape)) * s
    return pos.astype(F32), float(s)


def twists(M, rng, rot_amp, trans_amp):
    return synth.dq_from_twist(rng.uniform(-rot_amp, rot_amp, (M, 3)).astype(F32), rng.uniform(-trans_amp, trans_amp, (M, 3)).astype(F32))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the data-term solve at every step-kernel and W-apply dispatch
def solver_problem(M, seed):
    """M nodes, ~3 points per reachable node (some with NaN canonical or live coordinates), 5 nodes far away from every point
    (empty columns of W), smooth target motion plus noise."""
    rng = np.random.default_rng(seed)
    pos, s = jittered_lattice(M, 0.0, 1.0, rng)
    far = rng.choice(M, 5, replace=False)
    pos[far] += F32(40.0)                                     # no point has them among its k nearest
    reach = np.setdiff1d(np.arange(M), far)
    sigma = (2 * s * rng.uniform(0.9, 1.1, M)).astype(F32)
    dq = twists(M, rng, 0.1, 0.01)
    N = 3 * M
    src = (pos[rng.choice(reach, N)] + rng.normal(0, 0.5 * s, (N, 3))).astype(F32)
    dst = (src + 0.02 * np.sin(6 * src) + rng.normal(0, 1e-3, (N, 3))).astype(F32)
    src[7::101] = np.nan
    dst[11::89, 1] = np.nan
    return pos, sigma, dq, src, dst, far


def check_solve(M, k, lam, iters=20, seed=None):
    pos, sigma, dq, src, dst, far = solver_problem(M, seed if seed is not None else M + 7 * k)
    wf = WarpField(k=k)
    wf.init(pos, sigma=sigma, transforms=dq)
    g_dq, g_en = wf.energy_data(torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda(), iters=iters, lam=lam, k=k)
    pts = np.nan_to_num(src[:4000], nan=0.3)
    d_pts = torch.from_numpy(pts.copy()).cuda()
    wf.warp(d_pts, k=k)                                       # energy_data installed the new transforms
    torch.cuda.synchronize()
    r_dq, r_en = O.solve_data_term(pos, dq, sigma, src, dst, k, iters, lam)
    assert r_en[1] < r_en[0]
    assert np.array_equal(bits(g_en.cpu().numpy()), bits(r_en)), (g_en.cpu().numpy(), r_en)
    g = g_dq.cpu().numpy()
    bad = np.nonzero((bits(g) != bits(r_dq)).any(1))[0]
    assert bad.size == 0, "%d of %d node transforms differ, first %s" % (bad.size, M, bad[:8])
    # the rotations are untouched everywhere; the empty columns keep their translations (x = 0 there: only the rounding of
    # re-encoding T0 with the rotation), while the nodes that points reach move
    assert np.array_equal(bits(g[:, :4]), bits(dq[:, :4]))
    t_in, t_out = np.zeros(4, F32), np.zeros(4, F32)
    for n in far:
        O.lib().orc_node_translation(dq[n], t_in); O.lib().orc_node_translation(g[n], t_out)
        assert np.abs(t_out[1:] - t_in[1:]).max() <= 1e-6 * np.abs(t_in[1:]).max() + 1e-10, (n, t_in, t_out)
    assert (np.abs(g[:, 4:] - dq[:, 4:]).max(1)[np.setdiff1d(np.arange(M), far)] > 0).mean() > 0.9     # (k = 1 leaves a few nodes unused)
    ref_pts, _ = O.warp_points(pos, r_dq, sigma, pts, None, k)
    assert np.array_equal(bits(d_pts.cpu().numpy()), bits(ref_pts))


# (M, k, lambda): every M on both sides of the step kernels' thresholds with k = 8; each step kernel with lambda = 0 and 1e-3
@pytest.mark.parametrize("M,k,lam", [(2048, 8, 0.0), (2048, 4, 1e-3),                # df_sv_step_reg_kernel<2>
                                     (2049, 8, 1e-3), (5120, 8, 0.0),                  # <5>
                                     (5121, 8, 0.0), (8192, 8, 1e-3),                  # <8>
                                     (8193, 8, 1e-3), (24576, 8, 0.0), (24576, 4, 1e-3), (65535, 8, 1e-3)])   # df_sv_step_kernel
def test_solve_at_step_kernel_boundaries(M, k, lam):
    check_solve(M, k, lam)


@pytest.mark.parametrize("M", [2000, 9000])
@pytest.mark.parametrize("k", [1, 2, 3, 5, 6, 7])
def test_solve_with_runtime_k(M, k):
    """df_sv_w_apply_kernel<0> (k other than 4 and 8) with the register step kernel and with the general one."""
    check_solve(M, k, 1e-3 if k % 2 else 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. node packing and the cull bounds across M = 8192, one handle
CULL_DIMS, CULL_SIZE, CULL_TRUNC = (64, 64, 64), 1.0, 0.04
CULL_POSE = synth.translation(-0.5, -0.5, 0.5)               # the volume spans z in [0.5, 1.5] in front of the camera at the origin
CULL_INTR = (F32(150.0), F32(150.0), F32(80.0), F32(60.0))
CULL_COLS, CULL_ROWS = 160, 120


def plane_depth(z0, amp, phase):
    """A wavy wall at about z0 metres, every pixel valid."""
    u, v = np.meshgrid(np.arange(CULL_COLS), np.arange(CULL_ROWS))
    z = z0 + amp * np.sin(u / 17.0 + phase) * np.cos(v / 13.0 - phase)
    return np.rint(z * 1000).astype(np.uint16)


DEEP = np.array([0.0, 0.0, 1.38])                            # 0.48 m behind the wall, in the middle of the image


def cull_node_set(M, rng):
    """A jittered lattice filling the volume; the node nearest DEEP gets the last index, the next nearest a random one."""
    pos, s = jittered_lattice(M, -0.5, 0.5, rng)
    pos[:, 2] += F32(1.0)
    near = np.argsort(np.linalg.norm(pos - DEEP, axis=1))[:2]
    pos[[near[0], M - 1]] = pos[[M - 1, near[0]]]
    return pos, np.full(M, 2 * s, F32)


def cull_transforms(M, pos, rng, frame):
    """Small twists, plus what reaches every branch of the bounds kernels:
       frame 0: every rotation with w >= 0 (the rotation bound on), one rotation quaternion of norm 1.5, and the largest translation
                (0.5 m along -z, towards the camera) on the LAST node, which sits deep behind the wall: it pulls the voxels around it
                onto the wall, where they update -- a bound that misses part of the node set (for M > 8192 the last node's index is
                above 8192) or part of the translation (its z component) lets the cull drop them;
       frame 1: one rotation written with w < 0 (the rotation bound off) and a large translation on the node next to it."""
    dq = twists(M, rng, 0.05, 0.005)
    if frame == 0:
        dq[M - 1] = quat_dq([0.05, -0.03, 1.0], [0.2], np.array([[0.002, -0.001, -0.5]], F32))[0]
        s = int(rng.integers(0, M // 2))
        dq[s] = dq[s] * F32(1.5)                              # non-unit rotation quaternion (and its dual part)
    else:
        b = int(np.argsort(np.linalg.norm(pos - DEEP, axis=1))[1])
        dq[b] = quat_dq([0.0, 0.0, 1.0], [0.1], np.array([[0.25, 0.0, -0.1]], F32))[0]
        n = int(rng.integers(0, M))
        dq[n] = -dq[n]                                        # the same transform written with w < 0
    return dq


def quat_dq(axis, angle, t):
    axis = np.asarray(axis, np.float64).reshape(-1, 3); axis = axis / np.linalg.norm(axis, axis=-1, keepdims=True)
    angle = np.asarray(angle, np.float64)
    rotq = np.concatenate([np.cos(angle / 2)[:, None], axis * np.sin(angle / 2)[:, None]], -1).astype(F32)
    half = np.concatenate([np.zeros((len(rotq), 1), F32), F32(0.5) * np.asarray(t, F32)], -1)
    return np.concatenate([rotq, synth.quat_mul(half, rotq)], -1).astype(F32)


def new_cull_volume():
    v = TsdfVolume(CULL_DIMS); v.setSize([CULL_SIZE] * 3); v.setTruncDist(CULL_TRUNC); v.setMaxWeight(64); v.setPose(CULL_POSE)
    return v


def test_pack_paths_and_cull_bounds_on_one_handle():
    rng = np.random.default_rng(2024)
    intr = Intr(*CULL_INTR); proj = np.array(CULL_INTR, F32)
    cam = np.eye(4, dtype=F32)
    vs = np.array([F32(CULL_SIZE) / F32(d) for d in CULL_DIMS], F32)
    frames = [O.compute_dists(plane_depth(0.9, 0.05, ph), proj) for ph in (0.0, 1.3)]
    wf = WarpField(k=8)
    for M in (100, 9000, 50, 9000, 8192, 8193):
        pos, sigma = cull_node_set(M, rng)
        wf.init(pos, sigma=sigma, transforms=twists(M, rng, 0.05, 0.005))     # set_nodes
        vols = [new_cull_volume(), new_cull_volume()]
        cnt = [torch.zeros(1, dtype=torch.int64, device="cuda") for _ in vols]
        ref = np.zeros(CULL_DIMS[::-1], np.uint32)
        n_ref = 0
        for f, dists in enumerate(frames):
            dq = cull_transforms(M, pos, rng, f)
            wf.set_transforms(torch.from_numpy(dq).cuda())                    # the pos == nullptr path
            d = upload_u16(dists)
            vols[0].integrate_warped(d, cam, intr, wf, n_updated=cnt[0])
            vols[1].integrate_warped(d, cam, intr, wf, n_updated=cnt[1], cull=False)
            n_ref += O.integrate_warped(dists, ref, O.make_volume(ref, CULL_DIMS, vs, CULL_TRUNC, 64), synth.aff12(CULL_POSE),
                                        synth.aff12(synth.affine_inv(cam)), proj, pos, dq, sigma, 8)
        a, b = vols[0].download(), vols[1].download()
        print("M = %d: updates %d / %d / %d" % (M, int(cnt[0].item()), int(cnt[1].item()), n_ref))
        assert n_ref > 0
        assert int(cnt[1].item()) == n_ref and np.array_equal(b, ref), "M = %d: no-cull sweep != oracle (%d voxels)" % (M, int((b != ref).sum()))
        assert int(cnt[0].item()) == n_ref and np.array_equal(a, ref), "M = %d: culled sweep != oracle (%d voxels)" % (M, int((a != ref).sum()))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3 + 4. 65 535 nodes: the super-brick gather overflows, and node 65 534 owns a region of the volume
DENSE_DIMS, DENSE_SIZE, DENSE_TRUNC = (96, 96, 96), 1.0, 0.04
DENSE_POSE = synth.translation(-0.5, -0.5, 0.4)              # z in [0.4, 1.4]
DENSE_INTR = (F32(120.0), F32(120.0), F32(64.0), F32(48.0))
DENSE_COLS, DENSE_ROWS = 128, 96
HOLE_C, HOLE_R = np.array([0.02, -0.03, 0.85]), 0.12        # the last node sits alone at the centre of this ball, on the wall


def dense_nodes():
    rng = np.random.default_rng(65535)
    M = 65535
    pos, s = jittered_lattice(M + 4000, -0.5, 0.5, rng)
    pos[:, 2] += F32(0.9)
    pos = pos[np.linalg.norm(pos - HOLE_C, axis=1) > HOLE_R][:M - 1]
    assert len(pos) == M - 1
    pos = np.concatenate([pos, HOLE_C[None].astype(F32)]).astype(F32)
    sigma = np.full(M, 2 * s, F32)
    dq = twists(M, rng, 0.08, 0.01)
    dq[M - 1] = quat_dq([1.0, 0.4, 0.0], [0.3], np.array([[0.01, 0.02, -0.03]], F32))[0]    # a transform of its own
    return pos, sigma, dq, s


@pytest.fixture(scope="module")
def dense():
    pos, sigma, dq, s = dense_nodes()
    vs = np.array([F32(DENSE_SIZE) / F32(d) for d in DENSE_DIMS], F32)
    dists = O.compute_dists(np.rint((0.85 + 0.04 * np.sin(np.arange(DENSE_COLS) / 9.0))[None, :].repeat(DENSE_ROWS, 0) * 1000).astype(np.uint16),
                            np.array(DENSE_INTR, F32))
    return dict(pos=pos, sigma=sigma, dq=dq, s=s, vs=vs, dists=dists)


def new_dense_volume():
    v = TsdfVolume(DENSE_DIMS); v.setSize([DENSE_SIZE] * 3); v.setTruncDist(DENSE_TRUNC); v.setMaxWeight(64); v.setPose(DENSE_POSE)
    return v


def super_brick_gather_lower_bound(pos, k, vs):
    """For every super-brick (4 x 4 x 4 bricks of 8^3 voxels): the number of nodes within D_k(c_S) + 2 d of its centre c_S, d the
    distance to its farthest brick centre.  The kernel's gather radius thrS is that plus r2x, times 1.001, plus 1e-5, so every node
    counted here is gathered."""
    X, Y, Z = DENSE_DIMS
    out = []
    for sz in range(Z // 32):
        for sy in range(Y // 32):
            for sx in range(X // 32):
                cs = (np.array([sx, sy, sz]) * 32 + 15.5) * vs.astype(np.float64) + DENSE_POSE[:3, 3]
                d = np.linalg.norm(12.0 * vs.astype(np.float64))          # brick centres sit 8 b + 3.5: at most 12 voxels per axis from c_S
                r = np.sort(np.linalg.norm(pos.astype(np.float64) - cs, axis=1))
                out.append(int((r <= r[k - 1] + 2 * d).sum()))
    return np.array(out)


@pytest.mark.parametrize("k", [4, 8])
def test_dense_node_set_overflows_the_super_brick_gather(dense, k):
    pos, sigma, dq = dense["pos"], dense["sigma"], dense["dq"]
    n_gather = super_brick_gather_lower_bound(pos, k, dense["vs"])
    print("k = %d: nodes inside the super-bricks' gather radius: min %d, max %d" % (k, n_gather.min(), n_gather.max()))
    assert (n_gather > SUPER_CAP).all()                      # every super-brick takes the overflow branch
    rng = np.random.default_rng(k)
    q = (rng.uniform(0, 1, (30000, 3)) * DENSE_SIZE + DENSE_POSE[:3, 3]).astype(F32)
    r_idx, r_d2 = O.knn(pos, q, k)
    wf = WarpField(k=k)
    wf.init(pos, sigma=sigma, transforms=dq)
    for indexed in (False, True):
        if indexed:
            wf.ensure_index(new_dense_volume(), k)
        idx, d2 = wf.KNN(torch.from_numpy(q).cuda(), k)
        torch.cuda.synchronize()
        assert np.array_equal(idx.cpu().numpy(), r_idx), "indexed = %s" % indexed
        assert np.array_equal(bits(d2.cpu().numpy()), bits(r_d2)), "indexed = %s" % indexed
    # warp with normals, through the index
    nrm = rng.normal(size=q.shape).astype(F32)
    p_d, n_d = torch.from_numpy(q.copy()).cuda(), torch.from_numpy(nrm.copy()).cuda()
    wf.warp(p_d, n_d)
    torch.cuda.synchronize()
    r_p, r_n = O.warp_points(pos, dq, sigma, q, nrm, k)
    assert np.array_equal(bits(p_d.cpu().numpy()), bits(r_p)) and np.array_equal(bits(n_d.cpu().numpy()), bits(r_n))
    # warped integrate: the default sweep and the one without cull, on the same handle, against the oracle
    check_dense_integrate(dense, wf, k, [dict(), dict(cull=False)])


def check_dense_integrate(dense, wf, k, variants):
    pos, sigma, dq = dense["pos"], dense["sigma"], dense["dq"]
    proj = np.array(DENSE_INTR, F32)
    ref = np.zeros(DENSE_DIMS[::-1], np.uint32)
    n_ref = O.integrate_warped(dense["dists"], ref, O.make_volume(ref, DENSE_DIMS, dense["vs"], DENSE_TRUNC, 64), synth.aff12(DENSE_POSE),
                               synth.aff12(np.eye(4, dtype=F32)), proj, pos, dq, sigma, k)
    assert n_ref > 0
    d = upload_u16(dense["dists"])
    for kw in variants:
        v = new_dense_volume()
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        v.integrate_warped(d, np.eye(4, dtype=F32), Intr(*DENSE_INTR), wf, k=k, n_updated=cnt, **kw)
        got = v.download()
        assert int(cnt.item()) == n_ref and np.array_equal(got, ref), "%s: %d voxels differ" % (kw, int((got != ref).sum()))
    return ref


@pytest.mark.parametrize("on_demand", [False, True], ids=["eager", "on-demand"])
def test_last_16_bit_node_id_is_carried_everywhere(dense, on_demand):
    """Node 65 534 is the unique nearest node of every voxel within HOLE_R / 2 of its position: KNN returns it there, and the warped
    integrate over that region (per-voxel tables and block models, made at once or on demand) equals the oracle."""
    pos, sigma, dq = dense["pos"], dense["sigma"], dense["dq"]
    M, k = len(pos), 8
    vs = dense["vs"]
    X, Y, Z = DENSE_DIMS
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    centres = np.stack([xx, yy, zz], -1).reshape(-1, 3) * vs.astype(np.float64) + DENSE_POSE[:3, 3]
    region = np.linalg.norm(centres - HOLE_C, axis=1) < HOLE_R / 2
    assert region.sum() > 500
    r_idx, _ = O.knn(pos, centres[region].astype(F32), k)
    assert (r_idx[:, 0] == M - 1).all()
    wf = WarpField(k=k, tables_on_demand=on_demand)
    wf.init(pos, sigma=sigma, transforms=dq)
    wf.ensure_index(new_dense_volume(), k)
    idx, _ = wf.KNN(torch.from_numpy(centres[region].astype(F32)).cuda(), k)
    torch.cuda.synchronize()
    assert (idx.cpu().numpy()[:, 0] == M - 1).all()
    ref = None
    for rep in range(2):                                      # the second sweep runs with the block models in place
        ref = check_dense_integrate(dense, wf, k, [dict(block_model="now")] if rep == 0 else [dict()])
    assert ((ref.reshape(-1)[region] >> 16) > 0).sum() > 100   # the region is on the wall: its voxels are updated


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. exact ties in a deep tree: a 32^3 lattice of 32 768 nodes
def tie_lattice():
    """Nodes on the lattice j / 32, j = 0..31 per axis (exact in float32), in a random index order; queries at cell centres (8 equidistant
    nodes), face centres (4) and edge midpoints (2).  Every coordinate and squared distance is exact."""
    rng = np.random.default_rng(32)
    g = np.stack(np.meshgrid(*[np.arange(32)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pos = (g[rng.permutation(len(g))] / 32.0).astype(F32)
    n, rows = 6000, np.arange(6000)
    c = rng.integers(0, 31, (n, 3)).astype(np.float64)
    cell = c + 0.5
    face = c + 0.5; face[rows, rng.integers(0, 3, n)] -= 0.5         # one coordinate on the lattice
    edge = c.copy(); edge[rows, rng.integers(0, 3, n)] += 0.5        # two coordinates on the lattice
    q = (np.concatenate([cell, face, edge]) / 32.0).astype(F32)
    return pos, q


@pytest.mark.parametrize("indexed", [False, True], ids=["scan", "brick-index"])
def test_exact_ties_in_a_32_cubed_lattice(indexed):
    pos, q = tie_lattice()
    for k in (4, 8):
        r_idx, r_d2 = O.knn(pos, q, k)
        b_idx, _ = O.knn(pos, q, k, brute=True)
        assert (r_idx != b_idx).any(1).sum() > 1000           # the tree order, not the index order, decides
        wf = WarpField(k=k, voxel_table=False)
        wf.init(pos, sigma=0.06)
        if indexed:
            v = TsdfVolume((64, 64, 64)); v.setSize([1.5] * 3); v.setPose(synth.translation(-0.25, -0.25, -0.25))
            wf.ensure_index(v, k)
        idx, d2 = wf.KNN(torch.from_numpy(q).cuda(), k)
        torch.cuda.synchronize()
        assert np.array_equal(bits(d2.cpu().numpy()), bits(r_d2))
        assert np.array_equal(idx.cpu().numpy(), r_idx), "k = %d: %d queries differ" % (k, int((idx.cpu().numpy() != r_idx).any(1).sum()))
