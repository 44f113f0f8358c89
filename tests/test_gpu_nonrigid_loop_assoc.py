"""The closed non-rigid frame loop (tests/nonrigid_loop.py, FAST: 64^3, 160 x 120, 7 frames, extend inside) with the projective data
association in front of the solve (tests/associate_loop.py): the GPU backend calls frontend.associateProjective between two
dfusion_transform_points, the oracle backend the numpy restatement tests/associate_ref.py (dist_thres 0.03, cos 30 degrees, margin
0.02).  Every recorded stage of every frame is equal bit for bit, and so is, per frame, what the association itself gave: live_out and
status bit for bit, the counts, and the copy taken back into the solver's frame (through _bits_nan: its NaNs went through float
arithmetic).  tests/test_associate_rule.py proves on the oracle alone that these inputs reach every rejection status."""
import numpy as np
import pytest

import associate_loop as AL
import nonrigid_loop as NL

pytestmark = pytest.mark.gpu


def test_fast_case_with_projective_association_equals_the_restatement_at_every_stage():
    case = NL.FAST
    oracle = AL.AssocOracleBackend(case)
    want = NL.run(oracle, case)
    assert NL.nonvacuity(want, case) == [], "the inputs no longer deserve the test"
    be = AL.AssocGpuBackend(case)
    got = NL.run(be, case)
    msg = NL.first_difference(got, want)
    print("%s: %s" % (case.name, NL.summary(got, case) if msg is None else None))
    assert sorted(be.assoc) == sorted(oracle.assoc) == list(range(1, case.frames))
    for f in range(1, case.frames):
        g, w = be.assoc[f], oracle.assoc[f]
        print("frame %d: counts %s" % (f, g["counts"].tolist()))
        assert np.array_equal(g["live"], w["live"]), "frame %d: %d live_out rows differ" % (f, int((g["live"] != w["live"]).any(1).sum()))
        assert np.array_equal(g["status"], w["status"]), "frame %d: statuses differ" % f
        assert np.array_equal(g["counts"], w["counts"]), "frame %d: counts %s against %s" % (f, g["counts"].tolist(), w["counts"].tolist())
        assert np.array_equal(g["back"], w["back"]), "frame %d: the copy taken back differs" % f
        assert g["index_valid"] == w["index_valid"] and g["counts"][0] > 0
    assert msg is None, "GPU against the restatement: " + msg
    assert NL.nonvacuity(got, case) == []
