"""Backends of the closed non-rigid loop (tests/nonrigid_loop.py) with the projective association in front of the solve
(tests/associate_loop.py) and the warp solve with node ROTATIONS as unknowns behind it (dfusion_warp_solve_rigid).  That
solve warps the model points itself, so it gets what the loop's first warp of the frame was handed -- the UNWARPED canonical points and
normals, kept from before that warp -- while the association still pairs the warped points, as in tests/plane_loop.py.  The loop holds
the normals in the ray-cast's (the camera's) frame and the points in inverse_pose * that frame, so the normals are taken there first:
dfusion_transform_points with the inverse pose's rotation and no translation.  The GPU backend calls WarpField.solve_rigid, the oracle
backend the numpy restatement tests/solver_rigid_ref.py; kg = 4, lambda_reg = 1, lambda_rot = lambda, one round, quadratic penalties."""
import numpy as np

import associate_loop as AL
import nonrigid_loop as NL
import solver_rigid_ref as G
from plane_loop import KG, LAMBDA_REG, inverse_rotation12

F32 = np.float32


class _KeepUnwarped:
    """What the frame's FIRST warp was handed, copied before it ran."""

    def warp(self, pts, nrm, frame):
        if getattr(self, "unwarped_frame", None) != frame:
            self.unwarped_frame, self.unwarped = frame, (self.copy_of(pts), self.copy_of(nrm))
        return super().warp(pts, nrm, frame)


class _OracleRigidSolve(NL.OracleBackend):
    def solve(self, canonical, live, frame):
        self.dq, en, _, _ = G.solve_rigid(self.pos, self.dq, self.sig, self.rigid_points, live, self.rigid_normals, self.k, self.case.iters,
                                          self.case.lam, self.case.lam, KG, LAMBDA_REG)
        return en


class RigidOracleBackend(_KeepUnwarped, AL.AssocOracleBackend, _OracleRigidSolve):
    copy_of = staticmethod(np.copy)

    def solve(self, canonical, live, frame):
        self.rigid_points = self.unwarped[0]
        self.rigid_normals = np.ascontiguousarray(NL.transform_ref(self.unwarped[1], inverse_rotation12(self.last_pose)))
        return super().solve(canonical, live, frame)


class _GpuRigidSolve(NL.GpuBackend):
    def solve(self, canonical, live, frame):
        dq, en = self.wf.solve_rigid(self.rigid_points, live, self.rigid_normals, iters=self.case.iters, lam=self.case.lam, lam_rot=self.case.lam,
                                     reg_neighbours=KG, reg_lambda=LAMBDA_REG)
        return en.cpu().numpy()


class RigidGpuBackend(_KeepUnwarped, AL.AssocGpuBackend, _GpuRigidSolve):
    @staticmethod
    def copy_of(t):
        return t.clone()

    def solve(self, canonical, live, frame):
        self.rigid_points = self.unwarped[0]
        self.rigid_normals = self._packed(self.unwarped[1], inverse_rotation12(self.last_pose))
        return super().solve(canonical, live, frame)


def run_oracle_loop(case=NL.FAST):
    """The oracle side alone: (record, backend)."""
    be = RigidOracleBackend(case)
    return NL.run(be, case), be


def rotations_changed(rec, frame):
    """The number of nodes whose rotation after the frame's solve is not the one it went in with (the node items of the stage before:
    frame 0's init_field, or the last frame's extend)."""
    before = NL.stage(rec, frame - 1, "extend" if frame > 1 else "init_field")["dq"]
    after = NL.stage(rec, frame, "solve")["dq"]
    assert before.shape == after.shape
    return int((before.reshape(-1, 8)[:, :4] != after.reshape(-1, 8)[:, :4]).any(1).sum())
