"""The closed non-rigid frame loop (tests/nonrigid_loop.py, FAST: 64^3, 160 x 120, 7 frames, extend inside) with the projective data
association in front of the solve and the solve with node ROTATIONS as unknowns behind it (tests/rigid_loop.py): the GPU backend calls
frontend.associateProjective and WarpField.solve_rigid on the unwarped canonical points and normals, the oracle backend the numpy
restatements tests/associate_ref.py and tests/solver_rigid_ref.py.  Every recorded stage of every frame is equal bit for bit, and so is
what the association gave per frame; in every frame the solve turns nodes."""
import numpy as np
import pytest

import nonrigid_loop as NL
import rigid_loop as RL

pytestmark = pytest.mark.gpu


def test_fast_case_with_association_and_the_rigid_solve_equals_the_restatement_at_every_stage():
    case = NL.FAST
    want, oracle = RL.run_oracle_loop(case)
    assert NL.nonvacuity(want, case) == [], "the inputs no longer deserve the test"
    be = RL.RigidGpuBackend(case)
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
    for f in range(1, case.frames):
        assert RL.rotations_changed(got, f) >= 1, "frame %d: no node's rotation differs from its seed" % f
