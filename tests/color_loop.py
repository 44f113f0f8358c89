"""Backends of the closed non-rigid loop (tests/nonrigid_loop.py) that fuse a colour image after every integrate, the way KinFu does with
KinFuParams::integrate_color and warped_fusion: frame 0 rigidly after the rigid integrate, every later frame through the warp field
after the warped integrate, with the frame's own dists and pose.  The GPU side goes through ColorVolume on the loop's one volume and one
warp-field handle; the oracle side through the numpy restatement tests/color_ref.py on the oracle loop's own volume and nodes.  Both
record colors[frame] (the colour volume's bytes) and counts[frame] = (selected, fused).  The image of frame f is the 5 cm checker painted
from the loop's depth frame f at the synthetic camera pose (images(case))."""
import numpy as np

import color_ref as CR
import nonrigid_loop as NL
from dynamicfusion_amd import synth

F32 = np.float32
MAX_WEIGHT = 3                         # so that the cap engages within the 7 frames


def images(case):
    return [CR.paint_checker(d, synth.camera_pose(case.cfg, f * case.cam_step), case.cfg.intr) for f, d in enumerate(NL.depth_frames(case))]


class ColorOracleBackend(NL.OracleBackend):
    def __init__(self, case):
        super().__init__(case)
        self.images = images(case)
        self.color = np.zeros(self.vol.shape + (4,), np.uint8)
        self.colors, self.counts = {}, {}

    def _fuse(self, dists, cam_pose, frame, nodes):
        n_sel, n_fused, _, _ = CR.integrate(self.color, self.vol, self.cfg.dims, self.vs, self.trunc, self.images[frame], np.ascontiguousarray(dists),
                                            synth.aff12(self.pose), synth.aff12(synth.affine_inv(cam_pose)), self.intr, nodes=nodes, k=self.k,
                                            max_weight=MAX_WEIGHT)
        self.colors[frame], self.counts[frame] = self.color.copy(), (n_sel, n_fused)

    def integrate(self, dists, cam_pose):
        n = super().integrate(dists, cam_pose)
        self._fuse(dists, cam_pose, 0, None)
        return n

    def integrate_warped(self, dists, cam_pose, frame):
        n = super().integrate_warped(dists, cam_pose, frame)
        self._fuse(dists, cam_pose, frame, (self.pos, self.dq, self.sig))
        return n


class ColorGpuBackend(NL.GpuBackend):
    def __init__(self, case, **kw):
        super().__init__(case, **kw)
        from dynamicfusion_amd import ColorVolume
        self.images = [self.torch.from_numpy(im).cuda() for im in images(case)]
        self.cv = ColorVolume(self.v)
        self.colors, self.counts = {}, {}

    def _fuse(self, dists, cam_pose, frame, wf):
        c = self.cv.integrate(self.images[frame], dists, cam_pose, self.intr, warp_field=wf, max_weight=MAX_WEIGHT, return_counts=True)
        self.colors[frame], self.counts[frame] = self.cv.download().copy(), tuple(c.tolist())

    def integrate(self, dists, cam_pose):
        n = super().integrate(dists, cam_pose)
        self._fuse(dists, cam_pose, 0, None)
        return n

    def integrate_warped(self, dists, cam_pose, frame):
        n = super().integrate_warped(dists, cam_pose, frame)
        self._fuse(dists, cam_pose, frame, self.wf)
        return n
