"""ColorVolume: the colour of the fused surface (include/dfusion.h dfusion_color_*; no reference counterpart -- the reference's
KinFu::operator() accepts a colour image and drops it).

A ColorVolume belongs to a TsdfVolume and shares its dims, stored planes and pose: 4 bytes a voxel {c0, c1, c2, w}, the three channels
in the byte order of the images it is given.  integrate() looks every near-surface voxel up where the rigid pose -- or the warp field --
puts it in the live frame and keeps an integer running average; fetchColors() reads the colours of points (fetchCloud / fetchMesh
vertices) back.  All compute is in libdfusion_hip.so.
"""
import ctypes as C

import numpy as np
import torch

from . import capi
from .synth import aff12, affine_inv, affine_mul
from .tsdf_volume import BGRA, U16, _flat, _image, _ptr, _stream

F32 = np.float32


class ColorVolume:
    def __init__(self, tsdf_volume):
        self.volume = tsdf_volume
        X, Y, _ = tsdf_volume.getDims()
        self.data_ = torch.empty((tsdf_volume.z_store_n, Y, X, 4), dtype=torch.uint8, device=tsdf_volume.device)
        self.clear()

    def data(self):
        return self.data_

    def clear(self):
        capi.check(capi.lib().dfusion_color_clear(_ptr(self.data_), self.volume.c_volume(), self.volume.c_slab(), _stream()),
                   "dfusion_color_clear")

    def default_capacity(self):
        """Voxels a frame can colour when the caller names no capacity: a sixteenth of the slab's own voxels (the band |tsdf| < 1 of a
        surface crossing the volume a few times holds a few per cent of them), at least 65536, never more than there are."""
        X, Y, _ = self.volume.getDims()
        n = X * Y * self.volume.z_own_n
        return max(1, min(n, max(n // 16, 65536)))

    def integrate(self, image, dists, camera_pose, intr, warp_field=None, k=None, band=1.0, max_weight=64, capacity=None, return_counts=False):
        """image: uint8 [rows, cols, 4] device tensor (the 4th byte is ignored), dists: the frame's dists image (u16 [rows, cols]).  Call
        it after the frame's depth integrate: the TSDF volume is read as it is.  warp_field: the voxels go through its warp (k nearest
        nodes, default warp_field.k) as in TsdfVolume.integrate_warped -- through the brick lists if the field holds an index for >= k
        neighbours (integrate_warped builds one), else by scanning the nodes: the same bytes; None: rigid.  Nothing synchronises.
        return_counts: device int64 [2] = (voxels selected, voxels fused); selected > capacity means the highest-index voxels were
        left out."""
        vol = self.volume
        ip, ipitch, rows, cols = _image(image, BGRA)
        dp, dpitch = vol._same_size(_image(dists, U16), rows, cols)
        cam_inv = affine_inv(np.asarray(camera_pose, F32))
        if warp_field is None:
            world2cam, handle, k = cam_inv, None, 0
        else:
            k = warp_field.k if k is None else int(k)
            world2cam, handle = affine_mul(cam_inv, warp_field.warp_to_live_), warp_field.handle
        capacity = self.default_capacity() if capacity is None else int(capacity)
        counts = torch.empty(2, dtype=torch.int64, device=vol.device) if return_counts else None
        capi.check(capi.lib().dfusion_color_integrate(
            ip, ipitch, dp, dpitch, cols, rows, vol.c_volume(), vol.c_slab(), _ptr(self.data_), capi.floats(aff12(vol.pose_)),
            capi.floats(aff12(world2cam)), intr.as_proj(), handle, k, float(band), int(max_weight), capacity,
            C.c_void_p(counts.data_ptr()) if return_counts else None, C.c_void_p(counts.data_ptr() + 8) if return_counts else None,
            _stream()), "dfusion_color_integrate")
        return counts

    def fetchColors(self, points):
        """points: float32 [n, 4] device tensor (fetchCloud / fetchMesh vertices, world frame) -> uint8 [n, 4]: the three channels and
        255, or four zeros where no coloured voxel surrounds the point."""
        vol = self.volume
        if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 4:
            raise ValueError("points must be float32 [n, 4], got %s %s" % (points.dtype, tuple(points.shape)))
        n = int(points.shape[0])
        out = torch.empty((n, 4), dtype=torch.uint8, device=vol.device)
        world2vol = np.linalg.inv(vol.pose_.astype(np.float64)).astype(F32)
        capi.check(capi.lib().dfusion_color_fetch(_ptr(self.data_), vol.c_volume(), vol.c_slab(), capi.floats(aff12(world2vol)),
                                                  _flat(points) if n else None, n, _ptr(out) if n else None, _stream()),
                   "dfusion_color_fetch")
        return out

    # ---- convenience for tests
    def download(self):
        """uint8 numpy [z_store_n, Y, X, 4]: c0, c1, c2, weight."""
        return self.data_.detach().cpu().numpy()

    def upload(self, arr_u8):
        self.data_.copy_(torch.from_numpy(np.ascontiguousarray(arr_u8, np.uint8)).reshape(self.data_.shape))
