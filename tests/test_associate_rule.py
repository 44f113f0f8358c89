"""The projective data association's rule on its numpy restatement alone (tests/associate_ref.py): the proof that the inputs of
tests/test_gpu_associate.py and tests/test_gpu_nonrigid_loop_assoc.py deserve those tests.

Planted sphere (160 x 120, radius 0.2 m at 1 m, model = canonical + t0, live sphere moved by t0 + (4, 2, -3) mm, depth rounded to mm),
dist_thres 0.05, cos 30 degrees, occlusion test off: projective pairing finds the live sample about one pixel footprint from the true
correspondence where index pairing is centimetres off.  Closed loop (FAST, oracle backends): the association keeps the loop honest,
keeps at least 90 % of the index-valid pairs, lowers E_data before the solve at least tenfold, and every rejection status occurs."""
import numpy as np

import associate_loop as AL
import associate_ref as AR
import nonrigid_loop as NL

F32 = np.float32
_loops = {}


def _planted_medians(t0):
    s = AR.planted(t0)
    live, st, cnt = AR.associate(s["points"], s["normals"], s["live_points"], s["live_normals"], AR.INTR, AR.DIST_THRES, AR.MIN_COSINE, -1.0)
    finite = int(np.isfinite(s["points"]).all(1).sum())
    proj = float(np.median(AR.pair_error_mm(live, s["truth"])))
    index = float(np.median(AR.pair_error_mm(AR.index_pairs(s["points"], s["live_points"]), s["truth"])))
    print("t0 = %s: projective median %.3f mm, index median %.3f mm, paired %d of %d finite, counts %s" % (
        t0, proj, index, int(cnt[0]), finite, cnt.tolist()))
    assert int(cnt.sum()) == len(s["points"]) and int(cnt[1]) == len(s["points"]) - finite and int(cnt[4]) == 0
    assert np.array_equal(np.isfinite(live).all(1), st == 0)
    return proj, index, int(cnt[0]), finite


def test_planted_sphere_projective_pairing_beats_index_pairing():
    proj, index, paired, finite = _planted_medians((0.03, 0.0, 0.0))
    assert proj <= index / 3.0
    assert paired >= 0.9 * finite


def test_planted_sphere_without_drift_projective_pairing_is_no_worse():
    proj, index, paired, finite = _planted_medians((0.0, 0.0, 0.0))
    assert proj <= 1.1 * index
    assert paired >= 0.9 * finite


def test_occlusion_keeps_the_front_surface():
    """Two copies of the model, the second 5 cm behind: with margin 0.02 the far copy is occluded wherever the near copy hits its
    pixel, and the near copy pairs as it did alone."""
    s = AR.planted((0.03, 0.0, 0.0))
    p, n = s["points"], s["normals"]
    both = np.concatenate([p, p + np.array([0, 0, 0.05], F32)]).astype(F32)
    l1, st1, _ = AR.associate(p, n, s["live_points"], s["live_normals"], AR.INTR, 0.2, AR.MIN_COSINE, 0.02)
    l2, st2, cnt2 = AR.associate(both, np.concatenate([n, n]), s["live_points"], s["live_normals"], AR.INTR, 0.2, AR.MIN_COSINE, 0.02)
    assert np.array_equal(st2[:len(p)], st1) and np.array_equal(l2[:len(p)].view(np.uint32), l1.view(np.uint32))
    far = st2[len(p):]
    assert int((far == 4).sum()) > 1000


def _loop(associate):
    if associate not in _loops:
        be = AL.AssocOracleBackend(NL.FAST, associate=associate)
        _loops[associate] = (be, NL.run(be, NL.FAST))
    return _loops[associate]


def test_closed_loop_with_association_deserves_the_gpu_test():
    case = NL.FAST
    be, rec = _loop(True)
    _, rec_index = _loop(False)
    assert NL.nonvacuity(rec, case) == []
    assert NL.nonvacuity(rec_index, case) == []
    seen = np.zeros(8, np.int64)
    for f in range(1, case.frames):
        a = be.assoc[f]
        e_assoc, e_index = AL.energy_before(rec, f), AL.energy_before(rec_index, f)
        print("frame %d: counts %s, index-valid %d, E_data before %.4g (index loop %.4g, ratio %.1f)" % (
            f, a["counts"].tolist(), a["index_valid"], e_assoc, e_index, e_index / e_assoc))
        assert int(a["counts"].sum()) == case.cfg.cols * case.cfg.rows
        assert a["counts"][0] >= 0.9 * a["index_valid"]
        assert e_assoc * 10.0 <= e_index
        seen += a["counts"] > 0
    assert all(seen[s] >= 1 for s in (3, 4, 5, 6, 7)), seen.tolist()
