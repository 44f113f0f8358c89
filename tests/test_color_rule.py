"""The colour volume's rule (include/dfusion.h dfusion_color_*), checked on its numpy restatement tests/color_ref.py by
properties a wrong rule does not pass by luck.  No GPU: tests/test_gpu_color.py then pins the HIP kernels to the restatement."""
from fractions import Fraction

import numpy as np

import color_ref as CR
import mesh_ref as MR

F32 = np.float32
DIMS, COLS, ROWS = 32, 80, 60


def scene():
    return CR.scene(DIMS, COLS, ROWS)


def run(S, color, f, image=None, vf=None, **kw):
    """Frame f's image and dists into `color`, on the TSDF after frame vf (default f)."""
    sc = S.sc
    return CR.integrate(color, S.vols[f if vf is None else vf], S.cfg.dims, sc.vs, sc.trunc, S.images[f] if image is None else image, sc.dists[f], S.vol2world,
                        S.world2cam(f), sc.intr, **kw)


def test_voxels_outside_the_band_unweighted_or_unobserved_keep_their_bytes():
    S = scene()
    rng = np.random.default_rng(5)
    before = rng.integers(0, 256, S.vols[0].shape + (4,), dtype=np.uint8)
    color = before.copy()
    band = 0.6
    n_sel, n_fused, idx, obs = run(S, color, 0, vf=2, band=band)                              # the surface of three poses, seen from the first
    vol = S.vols[2].reshape(-1)
    tsdf = (vol & 0xffff).astype(np.uint16).view(np.float16).astype(np.float64)
    weight = vol >> 16
    changed = np.flatnonzero((color.reshape(-1, 4) != before.reshape(-1, 4)).any(1))
    assert n_fused > 500 and len(changed) > 500
    assert (weight[changed] > 0).all() and (np.abs(tsdf[changed]) < band).all()            # nothing outside the band or without weight moved
    assert (weight == 0).sum() > 1000 and ((weight > 0) & (np.abs(tsdf) >= band)).sum() > 1000   # and both kinds exist
    touched = np.zeros(vol.size, bool)
    touched[idx[obs]] = True
    assert (~obs).sum() > 100                                                                 # selected but not observed: occluded / out of view
    assert np.array_equal(color.reshape(-1, 4)[~touched], before.reshape(-1, 4)[~touched])
    assert n_sel == len(idx) == ((weight > 0) & (np.abs(tsdf) < band)).sum()
    # the weight byte of every observed voxel moved by one (or sits at the cap)
    wb, wa = before.reshape(-1, 4)[idx[obs], 3].astype(int), color.reshape(-1, 4)[idx[obs], 3].astype(int)
    assert np.array_equal(wa, np.minimum(wb + 1, 64))


def test_a_repeated_frame_is_a_fixed_point_and_the_weight_stops_at_the_cap():
    S = scene()
    color = np.zeros(S.vols[0].shape + (4,), np.uint8)
    _, n_fused, idx, obs = run(S, color, 0, max_weight=5)
    first = color.copy()
    assert n_fused > 1000 and (first.reshape(-1, 4)[idx[obs], 3] == 1).all()
    for rep in range(2, 9):
        run(S, color, 0, max_weight=5)
        assert np.array_equal(color[..., :3], first[..., :3])                                 # an average of equal bytes is that byte
        assert (color.reshape(-1, 4)[idx[obs], 3] == min(rep, 5)).all()
    assert (color[..., 3] <= 5).all()


def test_running_average_is_the_exact_rational_rounding():
    rng = np.random.default_rng(11)
    n, steps, cap = 64, 40, 17
    color = np.zeros((n, 4), np.uint8)
    idx = np.arange(n)
    exact = [[0, 0, 0] for _ in range(n)]
    w = [0] * n
    for s in range(steps):
        px = rng.integers(0, 256, (n, 4), dtype=np.uint8)
        if s % 7 == 0:
            px[:, :3] = 255 if s % 14 == 0 else 0                                             # the ends of the range
        CR.fuse(color, idx, px, cap)
        for i in range(n):
            for ch in range(3):
                q = Fraction(exact[i][ch] * w[i] + int(px[i, ch]), w[i] + 1) + Fraction(1, 2)
                exact[i][ch] = q.numerator // q.denominator                                   # round half up
            w[i] = min(w[i] + 1, cap)
        assert np.array_equal(color[:, :3].astype(int), np.array(exact)) and (color[:, 3] == np.array(w)).all()
    assert w[0] == cap


def test_truncation_processes_exactly_the_lowest_indices():
    S = scene()
    full = np.zeros(S.vols[0].shape + (4,), np.uint8)
    n_sel, n_fused, idx, obs = run(S, full, 0)
    cap = n_sel // 3
    part = np.zeros_like(full)
    n_sel2, n_fused2, idx2, obs2 = run(S, part, 0, capacity=cap)
    assert n_sel2 == n_sel and len(idx2) == cap and np.array_equal(idx2, idx[:cap]) and n_fused2 == obs[:cap].sum() > 100
    cut = idx[cap]
    assert np.array_equal(part.reshape(-1, 4)[:cut], full.reshape(-1, 4)[:cut]) and not part.reshape(-1, 4)[cut:].any()
    assert full.reshape(-1, 4)[cut:].any()


def test_half_space_paint_comes_back_exact_on_the_mesh():
    """Three frames of the half-space paint through an identity warp (20 nodes, identity transforms), then the colours of the mesh's
    vertices.  Measured on the restatement, band = 1: all of the 3675 vertices come back with alpha 255 (share 1.0000; asserted >= 0.9)."""
    S = CR.scene(DIMS, COLS, ROWS, nodes=20, k=4)
    sc, cfg = S.sc, S.cfg
    x0 = 0.013
    from dynamicfusion_amd import synth
    nodes = (sc.pos, synth.identity_dq(len(sc.pos)), sc.sigma)
    color = np.zeros(S.vols[0].shape + (4,), np.uint8)
    for f in range(3):
        img = CR.paint_half_space(sc.depths[f], sc.cam_poses[f], cfg.intr, x0)
        n_sel, n_fused, _, _ = run(S, color, f, image=img, nodes=nodes, k=4)
        assert n_fused > 1000
    mesh = MR.extract_mesh(S.vols[2], cfg.dims, sc.vs, S.vol2world)
    got = CR.fetch(color, cfg.dims, sc.vs, S.world2vol, mesh.vertices)
    share = float((got[:, 3] == 255).mean())
    print("vertices %d, alpha 255 share %.4f" % (len(got), share))
    assert len(got) > 3000 and share >= 0.9
    assert set(np.unique(got[:, 3])) <= {0, 255} and not got[got[:, 3] == 0].any()
    # margin: two voxel diagonals plus one pixel's footprint at the vertex's depth (the farthest of the three cameras)
    p = mesh.vertices[:, :3].astype(np.float64)
    depth = np.max([(p - np.asarray(c, np.float64)[:3, 3]) @ np.asarray(c, np.float64)[:3, 2] for c in sc.cam_poses], 0)
    margin = 2 * float(np.linalg.norm(sc.vs.astype(np.float64))) + depth / float(cfg.intr[0])
    far = (got[:, 3] == 255) & (np.abs(p[:, 0] - x0) > margin)
    left, right = far & (p[:, 0] < x0), far & (p[:, 0] > x0)
    assert left.sum() > 500 and right.sum() > 500
    assert (got[left, :3] == np.array(CR.HALF_A, np.uint8)).all() and (got[right, :3] == np.array(CR.HALF_B, np.uint8)).all()


def test_fetch_leaves_out_what_the_rule_leaves_out():
    dims, vs = (8, 4, 4), (F32(0.5), F32(0.25), F32(0.125))
    color = np.zeros((4, 4, 8, 4), np.uint8)
    color[1, 2, 3] = (10, 20, 30, 1)
    color[1, 2, 4] = (110, 220, 30, 9)                                                        # the weight byte gates, it does not weigh
    ident = CR.IDENT12
    pts = np.array([[1.75, 0.5, 0.125, 0], [1.5, 0.5, 0.125, 0], [2.0, 0.5, 0.125, 0], [1.875, 0.5, 0.125, 0],
                    [-3.0, 0.5, 0.125, 0], [np.nan, 0.5, 0.125, 0], [1.75, np.inf, 0.125, 0], [3.9, 0.9, 0.45, 0]], F32)
    got = CR.fetch(color, dims, vs, ident, pts)
    assert got[0].tolist() == [60, 120, 30, 255]                                              # halfway between the two voxels
    assert got[1].tolist() == [10, 20, 30, 255] and got[2].tolist() == [110, 220, 30, 255]
    assert got[3].tolist() == [85, 170, 30, 255]
    assert not got[4:].any()
    # a tap with weight byte 0 is left out, not averaged in as black: one voxel away from a coloured one the colour is still pure
    assert CR.fetch(color, dims, vs, ident, np.array([[1.3, 0.5, 0.125, 0]], F32))[0].tolist() == [10, 20, 30, 255]
    # the last cell: taps beyond the volume are left out
    color[3, 3, 7] = (1, 2, 3, 4)
    assert CR.fetch(color, dims, vs, ident, np.array([[3.6, 0.8, 0.4, 0]], F32))[0].tolist() == [1, 2, 3, 255]
