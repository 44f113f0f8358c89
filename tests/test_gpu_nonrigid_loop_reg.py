"""The closed non-rigid frame loop (tests/nonrigid_loop.py) with the REGULARISED warp solve: the GPU backend calls WarpField.solve, the
oracle backend the numpy restatement tests/solver_reg_ref.py, kg = 4 and lambda_reg = 1, everything else as in
tests/test_gpu_nonrigid_loop.py.  The FAST case (64^3, 160 x 120, 7 frames, the field grown by extend inside the loop, so the graph is
dropped and rebuilt on the way): every recorded stage of every frame equal bit for bit, and the transforms differ from the
unregularised loop's by frame 2 -- the term is live in the loop."""
import numpy as np
import pytest

import nonrigid_loop as NL
import solver_reg_ref as R

pytestmark = pytest.mark.gpu
KG, LAMBDA_REG = 4, 1.0


class RegGpuBackend(NL.GpuBackend):
    def solve(self, canonical, live, frame):
        dq, en = self.wf.solve(canonical, live, iters=self.case.iters, lam=self.case.lam, reg_neighbours=KG, reg_lambda=LAMBDA_REG)
        return en.cpu().numpy()


class RegOracleBackend(NL.OracleBackend):
    def solve(self, canonical, live, frame):
        self.dq, en = R.solve(self.pos, self.dq, self.sig, canonical, live, self.k, self.case.iters, self.case.lam, KG, LAMBDA_REG)
        return en


def test_fast_case_with_regularisation_equals_the_restatement_at_every_stage():
    case = NL.FAST
    want = NL.run(RegOracleBackend(case), case)
    assert NL.nonvacuity(want, case) == [], "the inputs no longer deserve the test"
    be = RegGpuBackend(case)
    got = NL.run(be, case)
    msg = NL.first_difference(got, want)
    print("%s: %s; kept blocks %s" % (case.name, NL.summary(got, case) if msg is None else None, be.kept))
    assert msg is None, "GPU against the restatement: " + msg
    assert NL.nonvacuity(got, case) == []
    en = NL.stage(got, 2, "solve")["energy"].view(np.float32)
    assert en.shape == (4,) and en[2] > 0                      # the graph had something to say
    # against the unregularised loop (the oracle's: tests/test_gpu_nonrigid_loop.py shows the GPU equals it)
    plain = NL.run(NL.OracleBackend(case), case)
    differs = [f for f in (1, 2) if NL.stage(got, f, "solve")["dq"].shape != NL.stage(plain, f, "solve")["dq"].shape
               or not np.array_equal(NL.stage(got, f, "solve")["dq"], NL.stage(plain, f, "solve")["dq"])]
    assert differs, "the regularised transforms equal the unregularised loop's up to frame 2"
