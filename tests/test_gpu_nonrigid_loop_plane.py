"""The closed non-rigid frame loop (tests/nonrigid_loop.py, FAST: 64^3, 160 x 120, 7 frames, extend inside) with the projective data
association in front of the solve and the POINT-TO-PLANE solve behind it (tests/plane_loop.py): the GPU backend calls
frontend.associateProjective and WarpField.solve_plane, the oracle backend the numpy restatements tests/associate_ref.py and
tests/solver_plane_ref.py.  Every recorded stage of every frame is equal bit for bit, and so is what the association gave per frame.
tests/test_solver_plane_rule.py proves on the oracle side alone that the solve moves nodes and lowers its energy in every frame, and
that the transforms are not the point-to-point loop's."""
import numpy as np
import pytest

import nonrigid_loop as NL
import plane_loop as PL

pytestmark = pytest.mark.gpu


def test_fast_case_with_association_and_the_plane_solve_equals_the_restatement_at_every_stage():
    case = NL.FAST
    want, oracle = PL.run_oracle_loop(case)
    assert NL.nonvacuity(want, case) == [], "the inputs no longer deserve the test"
    be = PL.PlaneGpuBackend(case)
    got = NL.run(be, case)
    msg = NL.first_difference(got, want)
    print("%s: %s" % (case.name, NL.summary(got, case) if msg is None else None))
    assert sorted(be.assoc) == sorted(oracle.assoc) == list(range(1, case.frames))
    for f in range(1, case.frames):
        g, w = be.assoc[f], oracle.assoc[f]
        for item in ("live", "status", "counts", "back"):
            assert np.array_equal(g[item], w[item]), "frame %d: the association's %s differs" % (f, item)
        assert g["counts"][0] > 0
    assert msg is None, "GPU against the restatement: " + msg
    assert NL.nonvacuity(got, case) == []
