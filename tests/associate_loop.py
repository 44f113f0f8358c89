"""Backends of the closed non-rigid loop (tests/nonrigid_loop.py) that put the projective data association in front of the solve, the
way the device-resident branch of KinFu::dynamicfusion does with warp_projective_association: the warped points go into the camera
frame (transform_points with the camera pose), are associated against the live level-0 maps with the warped normals as the loop holds
them, and the result goes back with the inverse pose -- both sides of the solve are then in one frame.  The backends keep the last
pose (the one the frame's ray-cast ran at), the live level-0 maps and the last warped normals, and record per frame what the
association gave: assoc[frame] = dict(live, status, counts, back, index_valid)."""
import numpy as np

import associate_ref as AR
import nonrigid_loop as NL
from dynamicfusion_amd import synth

F32 = np.float32
DIST_THRES, MIN_COSINE, MARGIN = 0.03, float(F32(np.cos(np.deg2rad(30.0)))), 0.02


class AssocOracleBackend(NL.OracleBackend):
    def __init__(self, case, associate=True):
        super().__init__(case)
        self.associate, self.assoc = bool(associate), {}

    def front_end(self, depth):
        d, p, n = super().front_end(depth)
        self.live_p, self.live_n = p[0], n[0]
        return d, p, n

    def raycast(self, cam_pose):
        self.last_pose = cam_pose
        return super().raycast(cam_pose)

    def warp(self, pts, nrm, frame):
        out = super().warp(pts, nrm, frame)
        self.last_wn = out[1]
        return out

    def solve(self, canonical, live, frame):
        index_valid = int((np.isfinite(canonical).all(1) & np.isfinite(live).all(1)).sum())
        if self.associate:
            cam = np.ascontiguousarray(NL.transform_ref(canonical, synth.aff12(self.last_pose)))
            lv, st, cnt = AR.associate(cam, self.last_wn, self.live_p, self.live_n, self.intr, DIST_THRES, MIN_COSINE, MARGIN)
            live = np.ascontiguousarray(NL.transform_ref(lv, synth.aff12(synth.affine_inv(self.last_pose))))
            self.assoc[frame] = dict(live=NL._bits(lv), status=st, counts=cnt.astype(np.int64), back=NL._bits_nan(live),
                                     index_valid=index_valid)
        return super().solve(canonical, live, frame)


class AssocGpuBackend(NL.GpuBackend):
    def __init__(self, case):
        super().__init__(case)
        self.assoc = {}

    def front_end(self, depth):
        d, p, n = super().front_end(depth)
        self.live_p, self.live_n = p[0], n[0]
        return d, p, n

    def raycast(self, cam_pose):
        self.last_pose = cam_pose
        return super().raycast(cam_pose)

    def warp(self, pts, nrm, frame):
        out = super().warp(pts, nrm, frame)
        self.last_wn = out[1]
        return out

    def _packed(self, pts, aff12):
        """dfusion_transform_points on a packed set, as an N x 1 image."""
        from dynamicfusion_amd import capi
        n = int(pts.shape[0])
        out = self.torch.empty((n, 3), dtype=self.torch.float32, device="cuda")
        capi.check(capi.lib().dfusion_transform_points(pts.data_ptr(), n * 12, 3, out.data_ptr(), n * 12, 3, n, 1, capi.floats(aff12),
                                                       self.main.cuda_stream), "dfusion_transform_points")
        return out

    def solve(self, canonical, live, frame):
        from dynamicfusion_amd import frontend
        index_valid = int((self.torch.isfinite(canonical).all(1) & self.torch.isfinite(live).all(1)).sum().item())
        cam = self._packed(canonical, synth.aff12(self.last_pose))
        lv, st, cnt = frontend.associateProjective(self.intr, cam, self.last_wn, self.live_p, self.live_n, DIST_THRES, MIN_COSINE, MARGIN,
                                                   return_status=True, return_counts=True)
        back = self._packed(lv, synth.aff12(synth.affine_inv(self.last_pose)))
        self.assoc[frame] = dict(live=NL._bits(lv.cpu().numpy()), status=st.cpu().numpy(), counts=cnt.cpu().numpy(),
                                 back=NL._bits_nan(back.cpu().numpy()), index_valid=index_valid)
        return super().solve(canonical, back, frame)


def energy_before(rec, frame):
    return float(NL.stage(rec, frame, "solve")["energy"].view(F32)[0])
