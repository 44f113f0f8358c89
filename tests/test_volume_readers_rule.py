"""What the volumes of tests/volume_cases.py reach in dfusion_extract_cloud, dfusion_extract_normals and the ray-cast, established
without a GPU: from the numpy restatement of the extractor's per-wave-item crossing count, from the oracle, and -- where oracle/_ref is
built -- from the reference's own kernels compiled for the host.  tests/test_gpu_extract_edges.py and tests/test_gpu_raycast_edges.py
run the kernels on exactly these volumes; every coverage condition they rely on is asserted here."""
import numpy as np
import pytest

import mesh_ref as R
import oracle_lib as O
import volume_cases as VC
from dynamicfusion_amd import synth

F32 = np.float32
live = pytest.mark.skipif(not O.have_refcu(), reason="oracle/_ref/libdfref_cu.so not built (needs the reference's sources)")
CAP = VC.DF_EX_CAP


# ------------------------------------------------------------------------------------------------ the extractor's rounds
CRAFTED = {                      # name: (crossings per item, smallest and largest round sum, total)
    "z_parity": ({256}, 1024, 1024, 16384),
    "z_parity_split": ({257}, 1028, 1028, 16448),
    "z_parity_even_x": ({128}, 512, 512, 8192),
    "checker": ({511, 767}, 2556, 3068, 47040),
}


@pytest.mark.parametrize("name", list(CRAFTED))
def test_crafted_volumes_have_the_stated_rounds(name):
    values, lo, hi, total = CRAFTED[name]
    vol = VC.case(name)
    per, listed = VC.item_counts(vol)
    assert len(per) == 64 and listed.all() and set(per.tolist()) == values and per.sum() == total == VC.named_cloud(name)[1]
    b = VC.round_sum_bounds(vol)
    assert len(b) == 4 and (b[:, 0] == VC.ITEMS_PER_WORKGROUP).all() and b[:, 1].min() == lo and b[:, 2].max() == hi
    if name == "z_parity":          # round 1 fills the buffer exactly and is not flushed (1024 > 1024 is false); round 2 flushes first
        assert lo == hi == CAP
    elif name == "z_parity_even_x":  # two rounds fill it exactly, the third flushes first
        assert 2 * lo == 2 * hi == CAP
    elif name == "z_parity_split":   # every round is `direct`, by the smallest overshoot a round of equal items can have
        assert lo == hi == CAP + VC.ITEMS_PER_ROUND
    else:                            # `direct`, near the most a round can hold: 4 items x 256 voxels x 3 edges
        assert lo > 2 * CAP and hi == 3 * CAP - VC.ITEMS_PER_ROUND


def test_one_past_volume_overflows_the_buffer_by_one_point():
    """Five listed items of 205 crossings in every workgroup: whatever their order, the round of four leaves 820 points buffered and
    the round of one makes s_fill + sum = 1025, the smallest value that must flush."""
    vol = VC.case("one_past")
    per, listed = VC.item_counts(vol)
    groups = listed.reshape(-1, VC.ITEMS_PER_WORKGROUP)
    assert len(per) == 64 and (groups.sum(1) == 5).all() and set(per[listed].tolist()) == {205} and not per[~listed].any()
    assert 4 * 205 <= CAP and 5 * 205 == CAP + 1 and per.sum() == 4 * 5 * 205 == VC.named_cloud("one_past")[1]


@pytest.mark.parametrize("dims", [VC.NOISE_DIMS, VC.BIG_DIMS], ids=["64x48x44", "128x96x86"])
def test_noise_volumes_reach_direct_buffered_and_mixed_rounds(dims):
    for p in (0.0, 0.1, 0.3, 0.6):
        assert VC.item_counts(VC.case("noise_%s" % p, dims))[0].sum() == VC.named_cloud("noise_%s" % p, dims)[1] > 10000
    b = VC.round_sum_bounds(VC.case("noise_0.0", dims))
    print("p_invalid 0: round sums %d .. %d" % (b[:, 1].min(), b[:, 2].max()))
    assert b[:, 1].min() > CAP                                           # every round of four is `direct`
    b = VC.round_sum_bounds(VC.case("noise_0.3", dims))
    print("p_invalid 0.3: round sums %d .. %d" % (b[:, 1].min(), b[:, 2].max()))
    assert b[:, 1].min() > CAP // 4 and b[:, 2].max() < CAP              # every round is buffered ...
    full = b[b[:, 0] == VC.ITEMS_PER_WORKGROUP]
    assert len(full) >= len(b) - 1 and (4 * full[:, 1] > CAP).all()      # ... and the four rounds of a 16-item workgroup overflow the buffer
    b = VC.round_sum_bounds(VC.case("noise_0.1", dims))
    print("p_invalid 0.1: round sums %d .. %d" % (b[:, 1].min(), b[:, 2].max()))
    assert b[:, 1].min() < CAP < b[:, 2].max()                           # both kinds of round occur
    # (stronger than a bound over orders: in address order -- one of the orders -- both kinds do occur)
    per, listed = VC.item_counts(VC.case("noise_0.1", dims))
    assert listed.all()
    rounds = per[:len(per) // 4 * 4].reshape(-1, 4).sum(1)
    assert (rounds > CAP).any() and (rounds <= CAP).any()


def test_restatement_counts_every_extract_case():
    """The per-item restatement's total is O.extract_cloud's count on every volume the GPU tests extract."""
    for index, dims in enumerate(R.FUZZ_DIMS):
        for p in R.FUZZ_P_INVALID:
            vol, _ = R.fuzz_case(index, p)
            n = VC.oracle_cloud(vol, dims)[1]
            assert (VC.item_counts(vol)[0].sum() if dims[2] > 1 else 0) == n
            if dims in ((4, 1, 1), (12, 5, 1)):
                assert n == 0
    for name in ("checker", "z_parity"):
        for dims in ((16, 6, 5), VC.NOISE_DIMS):
            assert VC.item_counts(VC.case(name, dims))[0].sum() == VC.named_cloud(name, dims)[1] > 0
    vol = R.noise_volume((20, 9, 12), 23, 0.1)
    assert VC.item_counts(vol)[0].sum() == VC.oracle_cloud(vol, (20, 9, 12))[1]
    vol = R.noise_volume((24, 11, 13), 19, 0.1)
    assert VC.item_counts(vol)[0].sum() == VC.oracle_cloud(vol, (24, 11, 13), vs=R.ANISO_VS, aff12=synth.aff12(R.rotated_pose()))[1]


def test_noise_clouds_have_normals_past_the_border_gate():
    """At least 40 % of a noise cloud's points have a finite normal (the rest lie within two voxels of a face): the GPU comparison of
    dfusion_extract_normals is not a comparison of NaN with NaN."""
    def share(vol, dims, aff=R.POSE, vs=R.VS):
        rows, _ = VC.oracle_cloud(vol, dims, aff, vs)
        rinv = np.linalg.inv(np.asarray(aff[:9], np.float64).reshape(3, 3)).astype(F32)
        return np.isfinite(O.extract_normals(VC.ovolume(vol, dims, vs), aff, rinv, rows.view(F32), 0.75)[:, :3]).all(1).mean()
    shares = [share(R.fuzz_case(R.FUZZ_DIMS.index((24, 11, 13)), p)[0], (24, 11, 13)) for p in R.FUZZ_P_INVALID]
    shares += [share(VC.case("noise_%s" % p), VC.NOISE_DIMS) for p in (0.0, 0.1, 0.3, 0.6)]
    shares.append(share(R.noise_volume((24, 11, 13), 19, 0.1), (24, 11, 13), synth.aff12(R.rotated_pose()), R.ANISO_VS))
    print("finite shares:", ["%.3f" % s for s in shares])
    assert min(shares) >= 0.4


# ------------------------------------------------------------------------------------------------ the march's window slots
@pytest.mark.parametrize("p", [0.0, 0.1, 0.6])
def test_noise_puts_events_of_both_kinds_on_every_window_slot(p):
    sc = VC.ray_scene()
    _, _, keys = VC.oracle_cast(sc, VC.case("noise_%s" % p), sc.cam_poses[0])
    classes = VC.event_classes(keys)
    ev = keys != VC.NO_EVENT
    first = ((keys[ev] >> 1) < VC.DF_RC_WINDOW).sum() / keys.size
    print("p_invalid %s: pixels per (slot, kind) %s, %.3f in the first window" % (p, classes.tolist(), first))
    assert classes.min() >= 200 and first >= 0.15


def test_back_wall_puts_late_events_on_every_slot_and_lets_rays_leave():
    sc = VC.ray_scene()
    p, _, keys = VC.oracle_cast(sc, VC.case("back_wall"), sc.cam_poses[0])
    ev = keys != VC.NO_EVENT
    late = np.where(ev & ((keys >> 1) >= 16), keys, VC.NO_EVENT)
    classes = VC.event_classes(late)
    print("back wall: late events per (slot, kind) %s, %d rays without an event, first step %d" % (classes.tolist(), (~ev).sum(), (keys[ev] >> 1).min()))
    assert (classes > 0).all() and (~ev).sum() > 0 and np.isfinite(p[..., 0]).sum() > 1000
    assert (keys[ev] >> 1).min() >= 16                                   # nothing before the wall: at least four windows are skipped whole


# ------------------------------------------------------------------------------------------------ the oracle is the reference here
def same_bits_off_nan(got, want):
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


REF_CASES = [("noise", (24, 12, 13), 0.0), ("noise", (24, 12, 13), 0.1), ("noise", VC.NOISE_DIMS, 0.0), ("noise", VC.NOISE_DIMS, 0.1),
             ("back_wall", VC.NOISE_DIMS, 0.1)]


@live
@pytest.mark.parametrize("kind,dims,p", REF_CASES, ids=["%s-%dx%dx%d-%s" % ((k,) + d + (p,)) for k, d, p in REF_CASES])
def test_oracle_equals_the_reference_kernels_on_these_volumes(kind, dims, p):
    vol = R.noise_volume(dims, 7, p) if kind == "noise" else VC.back_wall(dims, VC.BACK_WALL_SEED, p_invalid=p)
    sc = VC.ray_scene(dims)
    cfg = sc.cfg
    ov = sc.ovol(vol)
    aff = synth.aff12(sc.pose)
    cap = 3 * vol.size
    op, n = O.extract_cloud(ov, aff, cap)
    rp, rn = O.refcu_extract_cloud(ov, aff, cap)
    assert n == rn > 500 and np.array_equal(VC.sort_rows(op), VC.sort_rows(rp))
    rinv = np.linalg.inv(sc.pose[:3, :3].astype(np.float64)).astype(F32)
    assert same_bits_off_nan(O.refcu_extract_normals(ov, aff, rinv, op, cfg.gradient_delta_factor)[:, :3],
                             O.extract_normals(ov, aff, rinv, op, cfg.gradient_delta_factor)[:, :3])
    args = (ov, synth.aff12(sc.cam2vol(0)), sc.rinv(0))
    tail = (cfg.cols, cfg.rows, cfg.raycast_step_factor, cfg.gradient_delta_factor)
    wp, wn, _, _ = O.raycast_points(*args, sc.reproj, *tail)
    gp, gn = O.refcu_raycast_points(*args, sc.intr, *tail)
    assert same_bits_off_nan(gp, wp) and same_bits_off_nan(gn, wn) and np.isfinite(wp[..., 0]).sum() > 500
    wd, wdn = O.raycast_depth(*args, sc.reproj, *tail)
    gd, gdn = O.refcu_raycast_depth(*args, sc.intr, *tail)
    assert np.array_equal(gd, wd) and same_bits_off_nan(gdn, wdn)
