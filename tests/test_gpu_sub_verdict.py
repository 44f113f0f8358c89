"""Sub-verdicts of the warped sweep (k = 8): the kept blocks' 4 x 4 x 4 sub-blocks are judged by blend models of their own
(df_sub_verdict_kernel), and the launch plan drops a half layer (8 x 8 x 4 voxels) none of whose four sub-blocks can update.  What is
swept changes, never a bit of the volume: every case compares with the same sweep under DF_WARP_NO_SUB_VERDICT, with no cull at all or
with the CPU oracle, and sees through the swept-voxel counter that half layers were in fact dropped."""
import numpy as np
import pytest
import torch

import oracle_lib as O
from dynamicfusion_amd import Intr, TsdfVolume, WarpField, capi, compute_dists, synth, upload_u16
from scene import Scene
from test_gpu_parity import assert_volume_parity, make_gpu_volume, make_gpu_warp

pytestmark = pytest.mark.gpu
F32 = np.float32

CFG = synth.Config(64, 1.0, cols=160, rows=120, nodes=200, k=8, name="64^3, 200 nodes")
PATHS = (dict(), dict(sub_verdict=False), dict(cull=False))          # the product path, whole blocks only, every voxel


def sweep_frames(sc, frames, kw, slab=None, dqs=None, dists=None, cams=None, prefetch="steady"):
    """One volume and one handle through `frames`: the volume and the swept-voxel count after every frame, the update count, the handle."""
    cfg = sc.cfg
    intr = Intr(*cfg.intr)
    v = make_gpu_volume(sc, slab=slab)
    wf = make_gpu_warp(sc, k=cfg.k)
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    wf.debug_counters(cnt[1:])
    snaps, swept = [], []
    try:
        for f in frames:
            wf.set_transforms(torch.from_numpy(sc.dqs[f] if dqs is None else dqs[f]).cuda())
            before = int(cnt[1].item())
            v.integrate_warped(upload_u16(sc.dists[f]) if dists is None else dists[f], sc.cam_poses[f] if cams is None else cams[f], intr, wf,
                               n_updated=cnt[:1], prefetch=prefetch, **kw)
            snaps.append(v.data().clone()); swept.append(int(cnt[1].item()) - before)
    finally:
        wf.debug_counters(None)
    return snaps, swept, int(cnt[0].item()), wf, v


def test_sub_verdicts_drop_half_layers_and_no_update():
    """64^3, 200 nodes, four moving frames on one handle: the default path, DF_WARP_NO_SUB_VERDICT and DF_WARP_NO_CULL leave the same
    bits after every frame; the sub-verdicts never sweep more, and from the third frame on (the model pass has been over the blocks by
    then) they sweep less: the volume behind the sphere and the back plane is cut at half-layer granularity."""
    sc = Scene(CFG, n_frames=4)
    runs = [sweep_frames(sc, range(4), kw) for kw in PATHS]
    print("swept per frame: sub-verdicts %s, whole blocks %s, no cull %s" % (runs[0][1], runs[1][1], runs[2][1]))
    assert runs[0][2] > 0
    for other in runs[1:]:
        assert other[2] == runs[0][2]
        for f in range(4):
            assert torch.equal(runs[0][0][f], other[0][f]), "volume after frame %d differs" % f
    assert all(a <= b for a, b in zip(runs[0][1], runs[1][1]))
    assert any(a < b for a, b in zip(runs[0][1][2:], runs[1][1][2:]))


def test_odd_shape_against_the_oracle():
    """60 x 52 x 44: blocks, sub-blocks and half layers clipped by the volume at three faces.  Three frames (sub-verdicts from the second:
    models made at the first sweep), every voxel against the CPU oracle."""
    cfg = synth.Config((60, 52, 44), 1.0, cols=160, rows=120, nodes=200, k=8)
    sc = Scene(cfg, n_frames=3)
    snaps, swept, n, _, _ = sweep_frames(sc, range(3), dict(block_model="now"))
    _, swept_blocks, n2, _, _ = sweep_frames(sc, range(3), dict(block_model="now", sub_verdict=False))
    ref = sc.new_volume()
    for f in range(3):
        O.integrate_warped(sc.dists[f], ref, sc.ovol(ref), synth.aff12(sc.pose), synth.aff12(sc.world2cam(f)), sc.intr, sc.pos, sc.dqs[f], sc.sigma, cfg.k)
    print("odd shape: swept %s, whole blocks %s" % (swept, swept_blocks))
    assert_volume_parity(snaps[-1].cpu().numpy().view(np.uint32), ref)
    assert n == n2 > 0 and sum(swept[1:]) < sum(swept_blocks[1:])


def test_slabs_that_cut_half_layers():
    """Own ranges that start and end inside half layers (planes 10 .. 43, then 44 .. 63; three halo planes each side): the planes a slab
    owns equal the unsharded sweep's, the halo planes it stores but does not own keep their cleared value."""
    sc = Scene(CFG, n_frames=3)
    full, _, _, _, _ = sweep_frames(sc, range(3), dict(block_model="now"))
    cleared = make_gpu_volume(sc, slab=(10, 34, 3)).data()[0, 0, 0].item()
    for z0, zn in ((10, 34), (44, 20)):
        for kw in (dict(block_model="now"), dict(block_model="now", sub_verdict=False)):
            snaps, swept, _, _, v = sweep_frames(sc, range(3), kw, slab=(z0, zn, 3))
            got = snaps[-1]
            s0 = v.z_store0
            assert torch.equal(got[z0 - s0:z0 - s0 + zn], full[-1][z0:z0 + zn]), (z0, zn, kw)
            halo = torch.cat([got[:z0 - s0].reshape(-1), got[z0 - s0 + zn:].reshape(-1)])
            assert halo.numel() > 0 and bool((halo == cleared).all()), (z0, zn, kw)
            print("slab %d+%d %s: swept %s" % (z0, zn, kw, swept))


def test_blocks_without_sub_models_beside_modelled_ones():
    """3000 nodes all through a 64^3 volume, denser towards x = 0: most sub-blocks' unions exceed 16 nodes, their blocks get neither codes
    nor sub-models and are swept whole, beside modelled blocks in the same strip items (a strip is four blocks along x).  Bit-equal to
    the sweep with no cull."""
    cfg = synth.Config(64, 1.0, cols=160, rows=120, nodes=3000, k=8)
    rng = np.random.default_rng(11)
    sc = Scene(cfg, n_frames=3, with_nodes=False)
    u = rng.uniform(0.02, 0.98, (cfg.nodes, 3))
    u[:, 0] = u[:, 0] ** 3                                   # thinning out along x: about a tenth of the blocks, most of them at high x, keep every sub-union within 16
    sc.pos = (u * cfg.size + cfg.volume_pose[:3, 3]).astype(F32)
    sc.sigma = np.full(cfg.nodes, 0.06, F32)
    sc.dqs = [synth.node_transforms(cfg, f) for f in range(3)]
    runs = [sweep_frames(sc, range(3), dict(block_model="now", **kw)) for kw in PATHS]
    wf, v = runs[0][3], runs[0][4]
    alive = torch.zeros(8, dtype=torch.int64, device="cuda"); coded = torch.zeros_like(alive)
    wf.alive_blocks_per_layer(v, alive); wf.coded_blocks_per_layer(v, coded)
    print("kept blocks %d, of them with codes (every sub-union fits) %d; swept %s / %s / %s" % (int(alive.sum()), int(coded.sum()), runs[0][1], runs[1][1], runs[2][1]))
    assert 0 < int(coded.sum()) < int(alive.sum())          # both kinds were swept
    assert runs[0][2] > 0
    for other in runs[1:]:
        assert other[2] == runs[0][2]
        for f in range(3):
            assert torch.equal(runs[0][0][f], other[0][f]), "volume after frame %d differs" % f
    assert sum(runs[0][1]) <= sum(runs[1][1])


def test_prepare_and_sweep_with_sub_verdicts():
    """The split API reads the half-layer masks from the plan set its sweep owns: six frames, prepare on a second stream, bit-equal to
    the single call; and a plan whose node set was rewritten twice is refused as before."""
    sc = Scene(CFG, n_frames=6)
    intr = Intr(*CFG.intr)
    dists = [upload_u16(d) for d in sc.dists]
    dqs = [torch.from_numpy(q).cuda() for q in sc.dqs]
    single, swept, n_single, _, _ = sweep_frames(sc, range(6), dict())
    _, swept_blocks, _, _, _ = sweep_frames(sc, range(6), dict(sub_verdict=False))
    assert sum(swept) < sum(swept_blocks)                    # (the sub-verdicts were on in what follows)
    v = make_gpu_volume(sc); wf = make_gpu_warp(sc, k=CFG.k)
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    main, prep = torch.cuda.current_stream(), torch.cuda.Stream()
    for f in range(6):
        if f == 0: prep.wait_stream(main)
        with torch.cuda.stream(prep):
            wf.set_transforms(dqs[f])
            v.integrate_warped_prepare(dists[f], sc.cam_poses[f], intr, wf, prefetch="steady")
        v.integrate_warped_sweep(wf, n_updated=cnt)
        main.synchronize()
        assert torch.equal(v.data(), single[f]), "volume after frame %d differs" % f
    assert int(cnt.item()) == n_single
    torch.cuda.synchronize()
    wf.set_transforms(dqs[0])
    v.integrate_warped_prepare(dists[0], sc.cam_poses[0], intr, wf)
    wf.set_transforms(dqs[1]); wf.set_transforms(dqs[2])      # the second one rewrites the node set the plan reads
    with pytest.raises(capi.DfusionError) as e:
        v.integrate_warped_sweep(wf)
    assert "(code 100001)" in str(e.value)                    # DF_E_INVALID


@pytest.mark.parametrize("side", ["upper_dead", "lower_dead"])
def test_depth_plane_at_a_half_layer_boundary(side):
    """A flat depth image puts the end of the truncation band between planes 35 and 36 of the volume -- the middle of tile layer 4, the
    first layer of the strip items that hold planes 32 .. 63.  Seen from the front, planes 36 .. 63 cannot update: those items keep the
    LOWER half of their first layer only (the sweep's last-plane offset).  Seen from behind, planes 0 .. 35 cannot: the items keep the
    UPPER half of layer 4 and the layers above it (the first-plane offset).  Identity warp, three frames."""
    sc = Scene(CFG, n_frames=3, identity_warp=True)
    intr = Intr(*CFG.intr)
    cam = np.eye(4, dtype=F32)
    if side == "upper_dead": mm = 1009                       # camera at the origin: surface at z = 1.009, band ends at 1.049 < plane 36 = 1.0625
    else:
        cam[0, 0] = cam[2, 2] = -1.0; cam[2, 3] = 2.5        # camera behind the volume, looking back: surface at z = 2.5 - 1.401 = 1.099, band ends at 1.059
        mm = 1401
    depth = np.full((CFG.rows, CFG.cols), mm, np.uint16)
    dists = [compute_dists(upload_u16(depth), intr)] * 3
    cams = [cam] * 3
    runs = [sweep_frames(sc, range(3), dict(block_model="now", **kw), dists=dists, cams=cams) for kw in PATHS]
    print("%s: swept sub-verdicts %s, whole blocks %s, no cull %s" % (side, runs[0][1], runs[1][1], runs[2][1]))
    assert runs[0][2] > 0
    for other in runs[1:]:
        assert other[2] == runs[0][2]
        for f in range(3):
            assert torch.equal(runs[0][0][f], other[0][f]), "volume after frame %d differs" % f
    final = runs[0][0][-1]
    w = (final >> 16) & 0xffff
    dead = w[36:] if side == "upper_dead" else w[:36]
    live = w[32:36] if side == "upper_dead" else w[36:40]
    assert int(dead.sum()) == 0 and int(live.sum()) > 0      # the scene is what the docstring says
    # layer 4 (planes 32 .. 39) is cut in half for the items on the camera's axis: with whole blocks its eight planes are swept
    assert runs[0][1][2] < runs[1][1][2]
