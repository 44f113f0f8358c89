"""Backends of the closed non-rigid loop (tests/nonrigid_loop.py) with the projective association in front of the solve
(tests/associate_loop.py) and the POINT-TO-PLANE warp solve behind it, the way the device-resident branch of KinFu::dynamicfusion runs
with warp_projective_association and warp_point_to_plane.  The loop holds the warped normals in the ray-cast's (the camera's) frame and
the solver's points are inverse_pose * that frame, so the normals are taken there first: dfusion_transform_points with the inverse
pose's rotation and no translation.  The GPU backend calls WarpField.solve_plane, the oracle backend the numpy restatement
tests/solver_plane_ref.py; kg = 4, lambda_reg = 1, one round, quadratic penalties.  The association's backends end in their base's solve,
so the plane solves sit between the two in the method resolution order."""
import numpy as np

import associate_loop as AL
import nonrigid_loop as NL
import solver_plane_ref as P
from dynamicfusion_amd import synth

F32 = np.float32
KG, LAMBDA_REG = 4, 1.0


def inverse_rotation12(pose):
    aff = np.array(synth.aff12(synth.affine_inv(pose)), F32)
    aff[9:] = 0
    return aff


class _OraclePlaneSolve(NL.OracleBackend):
    def solve(self, canonical, live, frame):
        self.dq, en, _, _ = P.solve_plane(self.pos, self.dq, self.sig, canonical, live, self.plane_normals, self.k, self.case.iters,
                                          self.case.lam, KG, LAMBDA_REG)
        return en


class PlaneOracleBackend(AL.AssocOracleBackend, _OraclePlaneSolve):
    def solve(self, canonical, live, frame):
        self.plane_normals = np.ascontiguousarray(NL.transform_ref(self.last_wn, inverse_rotation12(self.last_pose)))
        return super().solve(canonical, live, frame)


class _GpuPlaneSolve(NL.GpuBackend):
    def solve(self, canonical, live, frame):
        dq, en = self.wf.solve_plane(canonical, live, self.plane_normals, iters=self.case.iters, lam=self.case.lam, reg_neighbours=KG,
                                     reg_lambda=LAMBDA_REG)
        return en.cpu().numpy()


class PlaneGpuBackend(AL.AssocGpuBackend, _GpuPlaneSolve):
    def solve(self, canonical, live, frame):
        self.plane_normals = self._packed(self.last_wn, inverse_rotation12(self.last_pose))
        return super().solve(canonical, live, frame)


def run_oracle_loop(case=NL.FAST):
    """The oracle side alone: (record, backend)."""
    be = PlaneOracleBackend(case)
    return NL.run(be, case), be
