"""The closed non-rigid frame loop (tests/nonrigid_loop.py) on the oracle backend alone, fast case (64^3, 160x120, 7 frames), k = 8 and 4:
the proof that the chosen inputs deserve the non-vacuity conditions tests/test_gpu_nonrigid_loop.py asserts (ICP tracks on every frame,
the solver lowers its energy and moves nodes, the field grows by more than 20 % over at least three frames, the surface stays in view),
that the oracle loop repeats bit for bit, and -- where oracle/_ref is built -- that the loop's warped integrates and the k-NN of the
solver's points are those of the reference's own classes (ref_integrate_warped, nanoflann), not only of their restatement."""
import numpy as np
import pytest

import nonrigid_loop as NL
import oracle_lib as O
from dynamicfusion_amd import synth

F32 = np.float32
_runs = {}


def oracle_run(k):
    if k not in _runs:
        case = NL.FAST.with_k(k)
        be = NL.OracleBackend(case)
        be.keep_inputs = True
        _runs[k] = (case, be, NL.run(be, case))
    return _runs[k]


@pytest.mark.parametrize("k", [8, 4])
def test_inputs_deserve_the_nonvacuity_conditions(k):
    case, _, rec = oracle_run(k)
    s = NL.summary(rec, case)
    print("k = %d:" % k, s)
    assert NL.nonvacuity(rec, case) == []
    assert s["frames"] == case.frames and 100 <= s["M0"] <= 300


def test_long_case_inputs_deserve_the_nonvacuity_conditions():
    case = NL.LONG
    rec = NL.run(NL.OracleBackend(case), case)
    s = NL.summary(rec, case)
    print("long:", s)
    assert NL.nonvacuity(rec, case) == []
    assert s["frames"] >= 12


def test_the_scene_deforms():
    """The depth offset is a few millimetres, smooth, and different from frame to frame."""
    offs = [NL.surface_offset_mm(NL.FAST, f) for f in range(NL.FAST.frames)]
    assert all(np.abs(o).max() <= 4 for o in offs) and np.abs(offs[0]).max() == 0
    assert all(np.abs(offs[f]).max() >= 2 for f in range(1, NL.FAST.frames) if abs(np.sin(0.6 * f)) > 0.5)
    assert all((offs[f] != offs[f - 1]).mean() > 0.2 for f in range(1, NL.FAST.frames))
    assert all(np.abs(np.diff(o, axis=1)).max() <= 1 and np.abs(np.diff(o, axis=0)).max() <= 1 for o in offs)


@pytest.mark.parametrize("k", [8, 4])
def test_two_runs_give_identical_bits(k):
    case, _, rec = oracle_run(k)
    again = NL.run(NL.OracleBackend(case), case)
    assert NL.first_difference(rec, again) is None


def test_first_difference_names_frame_and_stage():
    """The comparison can fail, and says where: an oracle that drops its second warp differs first at frame 1's warp2 (the solver has
    moved nodes by then); everything before it is still equal."""
    case, _, rec = oracle_run(8)
    msg = NL.first_difference(rec, NL.run(NL.OracleBackend(case, skip_second_warp=True), case))
    assert msg is not None and msg.startswith("frame 1, stage warp2, points:"), msg
    assert NL.first_difference(rec[:5], rec[:4]) is not None


@pytest.mark.skipif(not O.have_ref(), reason="the reference's nanoflann (oracle/_ref) is not built")
@pytest.mark.parametrize("k", [8, 4])
def test_loop_stages_equal_the_reference_classes(k):
    case, be, rec = oracle_run(k)
    cfg = case.cfg
    vs, trunc = NL._geometry(cfg)
    assert len(be.integrate_inputs) == case.frames - 1 == len(be.solver_points)
    for frame, dists, world2cam, pos, dq, sig, before in be.integrate_inputs:
        vol = before.copy()
        n, _ = O.ref_integrate_warped(dists, vol, cfg.dims, vs, trunc, cfg.max_weight, synth.aff12(cfg.volume_pose), synth.aff12(world2cam),
                                      np.array(cfg.intr, F32), pos, dq, sig, k, 0, 0, cfg.dims[2])
        want = NL.stage(rec, frame, "integrate_warped")
        bad = int((vol != want["volume"]).sum())
        assert bad == 0 and n == int(want["updated"]), "frame %d: %d voxels differ from the reference's classes (updates %d / %d)" % (
            frame, bad, n, int(want["updated"]))
    for frame, pos, pts in be.solver_points:
        q = pts[np.isfinite(pts).all(1)]
        assert len(q) > 1000
        i1, d1 = O.knn(pos, q, k)
        i2, d2 = O.knn(pos, q, k, use_ref=True)
        assert np.array_equal(i1, i2) and np.array_equal(d1.view(np.uint32), d2.view(np.uint32)), "frame %d: the solver's k-NN differs" % frame
