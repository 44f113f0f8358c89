"""The closed non-rigid frame loop (tests/nonrigid_loop.py) with the ROBUST warp solve: the GPU backend calls WarpField.solve_robust, the
oracle backend the numpy restatement tests/solver_robust_ref.py; kg = 4, lambda_reg = 1, 2 rounds, tukey_c = 0.05, huber_delta = 0.01,
everything else as in tests/test_gpu_nonrigid_loop_reg.py.  The FAST case (64^3, 160 x 120, 7 frames, extend inside): every recorded
stage of every frame equal bit for bit.  On the oracle's record alone: by frame 2 a point has weight 0 (the loop pairs points by pixel,
so the depth edges are gross outliers), and the transforms differ from the regularised-only loop's."""
import numpy as np
import pytest

import nonrigid_loop as NL
import solver_robust_ref as RR
from test_gpu_nonrigid_loop_reg import KG, LAMBDA_REG, RegOracleBackend

pytestmark = pytest.mark.gpu
ROUNDS, TUKEY_C, HUBER_DELTA = 2, 0.05, 0.01


class RobustGpuBackend(NL.GpuBackend):
    def solve(self, canonical, live, frame):
        dq, en = self.wf.solve_robust(canonical, live, iters=self.case.iters, lam=self.case.lam, reg_neighbours=KG, reg_lambda=LAMBDA_REG,
                                      rounds=ROUNDS, tukey_c=TUKEY_C, huber_delta=HUBER_DELTA)
        return en.cpu().numpy()


class RobustOracleBackend(NL.OracleBackend):
    def __init__(self, case):
        super().__init__(case)
        self.rejected = {}                         # frame -> number of points with weight exactly 0 after the last round

    def solve(self, canonical, live, frame):
        self.dq, en, pw, _ = RR.solve_robust(self.pos, self.dq, self.sig, canonical, live, self.k, self.case.iters, self.case.lam, KG,
                                             LAMBDA_REG, ROUNDS, TUKEY_C, HUBER_DELTA)
        valid = ~(np.isnan(canonical).any(1) | np.isnan(live).any(1))
        self.rejected[frame] = int((pw[valid] == 0).sum())
        return en


def test_fast_case_with_the_robust_solve_equals_the_restatement_at_every_stage():
    case = NL.FAST
    oracle = RobustOracleBackend(case)
    want = NL.run(oracle, case)
    assert NL.nonvacuity(want, case) == [], "the inputs no longer deserve the test"
    # conditions on the inputs, from the oracle's record alone
    print("points with weight 0 per frame:", oracle.rejected)
    assert max(oracle.rejected[1], oracle.rejected[2]) >= 1, "no point was rejected by frame 2"
    reg = NL.run(RegOracleBackend(case), case)
    differs = [f for f in (1, 2) if NL.stage(want, f, "solve")["dq"].shape != NL.stage(reg, f, "solve")["dq"].shape
               or not np.array_equal(NL.stage(want, f, "solve")["dq"], NL.stage(reg, f, "solve")["dq"])]
    assert differs, "the robust transforms equal the regularised-only loop's up to frame 2"
    be = RobustGpuBackend(case)
    got = NL.run(be, case)
    msg = NL.first_difference(got, want)
    print("%s: %s; kept blocks %s" % (case.name, NL.summary(got, case) if msg is None else None, be.kept))
    assert msg is None, "GPU against the restatement: " + msg
    assert NL.nonvacuity(got, case) == []
