"""Host-side mirror of the reference's depth front-end and projective ICP:
kfusion::cuda::{depthBilateralFilter, depthTruncation, depthBuildPyramid, computeNormalsAndMaskDepth, computePointNormals,
resizeDepthNormals, resizePointsNormals} (kfusion/src/imgproc.cpp:10-150) and kfusion::cuda::ProjectiveICP
(kfusion/src/projective_icp.cpp:64-213) over the C-ABI.  Images are device tensors: depth int16 [rows, cols] (u16 bits),
points / normals float32 [rows, cols, 4].
"""
import math

import numpy as np
import torch

from . import capi
from .synth import aff12
from .tsdf_volume import BGRA, F4, F32, U16, Intr, _flat, _image, _ptr, _stream


def intr_level(intr, level):
    """Intr::operator()(level), precomp.cpp:10-14."""
    div = 1 << level
    return Intr(F32(intr.fx) / F32(div), F32(intr.fy) / F32(div), F32(intr.cx) / F32(div), F32(intr.cy) / F32(div))


def _new_depth(rows, cols, device):
    return torch.empty((rows, cols), dtype=torch.int16, device=device)


def _new_image4(rows, cols, device):
    return torch.empty((rows, cols, 4), dtype=torch.float32, device=device)


def _sized(t, kind, rows, cols):
    """(ptr, pitch) of an output / second input image that must be rows x cols."""
    p, pitch, r, c = _image(t, kind)
    if (r, c) != (rows, cols):
        raise ValueError("image is %dx%d, expected %dx%d" % (r, c, rows, cols))
    return p, pitch


def depthBilateralFilter(depth, kernel_size, sigma_spatial, sigma_depth, out=None):
    sp, spitch, rows, cols = _image(depth, U16)
    if out is None:
        out = _new_depth(rows, cols, depth.device)
    dp, dpitch = _sized(out, U16, rows, cols)
    capi.check(capi.lib().dfusion_bilateral_filter(sp, spitch, dp, dpitch, cols, rows, int(kernel_size),
                                                   float(sigma_spatial), float(sigma_depth), _stream()), "dfusion_bilateral_filter")
    return out


def depthTruncation(depth, threshold):
    dp, pitch, rows, cols = _image(depth, U16)
    capi.check(capi.lib().dfusion_truncate_depth(dp, pitch, cols, rows, float(threshold), _stream()), "dfusion_truncate_depth")
    return depth


def cloudToDepth(cloud, out=None):
    """cuda::cloudToDepth (imgproc.cpp:98-103): depth mm = points.z * 1000 (a NaN point -- a ray-cast miss -- gives 0)."""
    cp, cpitch, rows, cols = _image(cloud, F4)
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.int16, device=cloud.device)
    dp, dpitch = _sized(out, U16, rows, cols)
    capi.check(capi.lib().dfusion_cloud_to_depth(cp, cpitch, dp, dpitch, cols, rows, _stream()), "dfusion_cloud_to_depth")
    return out


def depthBuildPyramid(depth, sigma_depth, out=None):
    sp, spitch, rows, cols = _image(depth, U16)
    if out is None:
        out = _new_depth(rows // 2, cols // 2, depth.device)
    dp, dpitch = _sized(out, U16, rows // 2, cols // 2)
    capi.check(capi.lib().dfusion_depth_pyramid(sp, spitch, cols, rows, dp, dpitch, float(sigma_depth),
                                                _stream()), "dfusion_depth_pyramid")
    return out


def computeNormalsAndMaskDepth(intr, depth, normals=None):
    dp, dpitch, rows, cols = _image(depth, U16)
    if normals is None:
        normals = _new_image4(rows, cols, depth.device)
    np_, npitch = _sized(normals, F4, rows, cols)
    capi.check(capi.lib().dfusion_compute_normals_mask_depth(dp, dpitch, np_, npitch, cols, rows, intr.as_proj(),
                                                             _stream()), "dfusion_compute_normals_mask_depth")
    return normals


def computePointNormals(intr, depth, points=None, normals=None):
    dp, dpitch, rows, cols = _image(depth, U16)
    if points is None:
        points = _new_image4(rows, cols, depth.device)
    if normals is None:
        normals = _new_image4(rows, cols, depth.device)
    pp, ppitch = _sized(points, F4, rows, cols)
    np_, npitch = _sized(normals, F4, rows, cols)
    capi.check(capi.lib().dfusion_compute_point_normals(dp, dpitch, pp, ppitch, np_, npitch, cols,
                                                        rows, intr.as_proj(), _stream()), "dfusion_compute_point_normals")
    return points, normals


def resizeDepthNormals(depth, normals, d=None, n=None):
    dp, dpitch, rows, cols = _image(depth, U16)
    np_, npitch = _sized(normals, F4, rows, cols)
    d = _new_depth(rows // 2, cols // 2, depth.device) if d is None else d
    n = _new_image4(rows // 2, cols // 2, depth.device) if n is None else n
    odp, odpitch = _sized(d, U16, rows // 2, cols // 2)
    onp, onpitch = _sized(n, F4, rows // 2, cols // 2)
    capi.check(capi.lib().dfusion_resize_depth_normals(dp, dpitch, np_, npitch, cols, rows, odp,
                                                       odpitch, onp, onpitch, _stream()), "dfusion_resize_depth_normals")
    return d, n


def resizePointsNormals(points, normals, p=None, n=None):
    pp, ppitch, rows, cols = _image(points, F4)
    np_, npitch = _sized(normals, F4, rows, cols)
    p = _new_image4(rows // 2, cols // 2, points.device) if p is None else p
    n = _new_image4(rows // 2, cols // 2, points.device) if n is None else n
    opp, oppitch = _sized(p, F4, rows // 2, cols // 2)
    onp, onpitch = _sized(n, F4, rows // 2, cols // 2)
    capi.check(capi.lib().dfusion_resize_points_normals(pp, ppitch, np_, npitch, cols, rows, opp,
                                                        oppitch, onp, onpitch, _stream()),
               "dfusion_resize_points_normals")
    return p, n


def renderImage(src, normals, intr, light_pose, image=None):
    """kfusion::cuda::renderImage (imgproc.cpp:152-186): Phong view of a points image (float32 [rows, cols, 4]) or a depth image
    (int16 [rows, cols]) with its normals; image: uint8 [rows, cols, 4] BGRA (device)."""
    np_, npitch, rows, cols = _image(normals, F4)
    if image is None:
        image = torch.empty((rows, cols, 4), dtype=torch.uint8, device=normals.device)
    ip, ipitch = _sized(image, BGRA, rows, cols)
    light = capi.floats(light_pose)
    if src.dtype == torch.float32:
        sp, spitch = _sized(src, F4, rows, cols)
        capi.check(capi.lib().dfusion_render_image_points(sp, spitch, np_, npitch, cols, rows, light, ip,
                                                          ipitch, _stream()), "dfusion_render_image_points")
    else:
        sp, spitch = _sized(src, U16, rows, cols)
        capi.check(capi.lib().dfusion_render_image_depth(sp, spitch, np_, npitch, cols, rows, intr.as_proj(), light,
                                                         ip, ipitch, _stream()), "dfusion_render_image_depth")
    return image


def renderTangentColors(normals, image=None):
    """kfusion::cuda::renderTangentColors (imgproc.cpp:193-201)."""
    np_, npitch, rows, cols = _image(normals, F4)
    if image is None:
        image = torch.empty((rows, cols, 4), dtype=torch.uint8, device=normals.device)
    ip, ipitch = _sized(image, BGRA, rows, cols)
    capi.check(capi.lib().dfusion_render_tangent_colors(np_, npitch, cols, rows, ip, ipitch, _stream()),
               "dfusion_render_tangent_colors")
    return image


def associateProjective(intr, points, normals, live_points, live_normals, dist_thres, min_cosine, occlusion_margin=-1.0,
                        return_status=False, return_counts=False):
    """Projective data association for the warp solve (include/dfusion.h dfusion_associate_projective): every predicted point
    (device [N, 3], camera frame of the live image; `normals` [N, 3] or None together with `live_normals`) is paired with the sample
    of `live_points` (float32 [rows, cols, 4]) at the pixel it projects to.  Returns live [N, 3] -- rejected points are all-NaN
    (0x7fffffff), which the solvers skip -- then, if asked for, status (uint8 [N]: 0 paired, 1 invalid, 2 behind, 3 outside,
    4 occluded, 5 hole, 6 far, 7 normal) and counts (int64 [8], points per status), all device tensors.  occlusion_margin < 0
    switches the occlusion test off."""
    if (normals is None) != (live_normals is None):
        raise ValueError("normals and live_normals go together")
    lp, lpitch, rows, cols = _image(live_points, F4)
    lnp, lnpitch = _sized(live_normals, F4, rows, cols) if live_normals is not None else (None, 0)
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("points %s %s, expected float32 [N, 3]" % (points.dtype, tuple(points.shape)))
    n = int(points.shape[0])
    if normals is not None and (normals.dtype != torch.float32 or tuple(normals.shape) != (n, 3)):
        raise ValueError("normals %s %s, expected float32 [%d, 3]" % (normals.dtype, tuple(normals.shape), n))
    if n == 0:
        normals, lnp = None, None                       # (an empty tensor has no address: nothing is read either way)
    dev = live_points.device
    live = torch.empty((n, 3), dtype=torch.float32, device=dev)
    status = torch.empty(n, dtype=torch.uint8, device=dev) if return_status else None
    counts = torch.empty(8, dtype=torch.int64, device=dev) if return_counts else None
    capi.check(capi.lib().dfusion_associate_projective(
        _flat(points), _flat(normals) if normals is not None else None, n, lp, lpitch, lnp, lnpitch, cols, rows, intr.as_proj(),
        float(dist_thres), float(min_cosine), float(occlusion_margin), _ptr(live), _ptr(status) if return_status else None,
        _ptr(counts) if return_counts else None, _stream()), "dfusion_associate_projective")
    out = (live,) + ((status,) if return_status else ()) + ((counts,) if return_counts else ())
    return out[0] if len(out) == 1 else out


def renderMesh(intr, vertices, triangles, cols, rows, world2cam=None, normals=None, attr=None, colors=None, max_extent=16,
               return_tri=False, return_counts=False):
    """A z-buffered rasteriser (include/dfusion.h dfusion_render_mesh): the mesh `vertices` (float32 [V, 4]) / `triangles` (int32 [T, 3],
    uint32 bits) -- fetchMesh's, or its vertices after WarpField.warp -- seen by the camera `intr` of cols x rows pixels.  world2cam: a
    4x4 pose or 12 floats, None = the vertices are in the camera frame.  Per-vertex normals / attr (float32 [V, 4]) and colors
    (uint8 [V, 4]) are interpolated as given (no rotation).  -> (points, normals, attr, colors): float32 [rows, cols, 4] images and a
    uint8 [rows, cols, 4] one, None where the input is; a miss is all-NaN (0x7fffffff) / four 0 bytes.  Then, if asked for, tri
    (int32 [rows, cols], -1 = miss) and counts (int64 [6]: triangles drawn / invalid / degenerate / stretched / off-screen, covered
    pixels).  Device tensors; nothing synchronises."""
    def per_vertex(t, dtype, name):
        if t is None:
            return None
        if t.dtype != dtype or tuple(t.shape) != (nv, 4):
            raise ValueError("%s %s %s, expected %s [%d, 4]" % (name, t.dtype, tuple(t.shape), dtype, nv))
        return _flat(t) if nv else None

    if vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 4:
        raise ValueError("vertices %s %s, expected float32 [V, 4]" % (vertices.dtype, tuple(vertices.shape)))
    if triangles.dtype != torch.int32 or triangles.dim() != 2 or triangles.shape[1] != 3:
        raise ValueError("triangles %s %s, expected int32 [T, 3]" % (triangles.dtype, tuple(triangles.shape)))
    nv, nt = int(vertices.shape[0]), int(triangles.shape[0])
    cols, rows = int(cols), int(rows)
    if cols <= 0 or rows <= 0:
        raise ValueError("image of %d x %d pixels" % (cols, rows))
    dev = vertices.device
    if world2cam is not None:
        w = np.asarray(world2cam, np.float32)
        world2cam = capi.floats(aff12(w) if w.shape == (4, 4) else w.reshape(12))
    points = _new_image4(rows, cols, dev)
    out_n = _new_image4(rows, cols, dev) if normals is not None else None
    out_a = _new_image4(rows, cols, dev) if attr is not None else None
    out_c = torch.empty((rows, cols, 4), dtype=torch.uint8, device=dev) if colors is not None else None
    tri = torch.empty((rows, cols), dtype=torch.int32, device=dev) if return_tri else None
    counts = torch.empty(6, dtype=torch.int64, device=dev) if return_counts else None
    capi.check(capi.lib().dfusion_render_mesh(
        _flat(vertices) if nv else None, nv, _flat(triangles) if nt else None, nt, world2cam, per_vertex(normals, torch.float32, "normals"),
        per_vertex(attr, torch.float32, "attr"), per_vertex(colors, torch.uint8, "colors"), cols, rows, intr.as_proj(), int(max_extent),
        _ptr(points), cols * 16, _ptr(out_n) if out_n is not None and nv else None, cols * 16, _ptr(out_a) if out_a is not None and nv else None,
        cols * 16, _ptr(out_c) if out_c is not None and nv else None, cols * 4, _ptr(tri) if return_tri else None, cols * 4,
        _ptr(counts) if return_counts else None, _stream()), "dfusion_render_mesh")
    if not nv:                                          # (no per-vertex array has an address: the images are all misses)
        for t in (out_n, out_a):
            if t is not None:
                t.copy_(points)
        if out_c is not None:
            out_c.zero_()
    out = (points, out_n, out_a, out_c) + ((tri,) if return_tri else ()) + ((counts,) if return_counts else ())
    return out


def renderLiveModel(volume, warp_field, camera_pose, intr, cols, rows, color_volume=None, k=None):
    """The prediction of the live frame: the canonical mesh of `volume` (fetchMesh with normals), coloured by `color_volume`
    (fetchColors at the canonical vertices; None: no colour image), warped by `warp_field` (copies of the vertices and normals, k
    nearest nodes, default warp_field.k) and rendered into the camera at `camera_pose` (inverted in f64), with the canonical vertices
    as the attribute.  -> (points, normals, canonical points, colours) images as renderMesh gives them; the normals stay in the frame
    the warp leaves them in."""
    return _render_live_mesh(volume.fetchMesh(with_normals=True), warp_field, camera_pose, intr, cols, rows, color_volume, k)


def renderLiveModelFiltered(volume, warp_field, camera_pose, intr, cols, rows, color_volume=None, k=None, min_component_triangles=0,
                            keep_largest=False):
    """renderLiveModel without the floaters: the mesh's connected pieces of fewer than min_component_triangles triangles (with
    keep_largest: all but the largest) are dropped first -- fetchMesh's arguments -- so the colours are fetched and the warp runs
    for the kept vertices only.  At the defaults: renderLiveModel's calls exactly."""
    mesh = volume.fetchMesh(with_normals=True, min_component_triangles=min_component_triangles, keep_largest=keep_largest)
    return _render_live_mesh(mesh, warp_field, camera_pose, intr, cols, rows, color_volume, k)


def _render_live_mesh(mesh, warp_field, camera_pose, intr, cols, rows, color_volume, k):
    vertices, triangles, normals = mesh
    colors = color_volume.fetchColors(vertices) if color_volume is not None else None
    nv = int(vertices.shape[0])
    p3, n3 = vertices[:, :3].contiguous(), normals[:, :3].contiguous()
    if nv:
        warp_field.warp(p3, n3, k)
    warped = torch.zeros((nv, 4), dtype=torch.float32, device=vertices.device)
    wnormals = torch.zeros((nv, 4), dtype=torch.float32, device=vertices.device)
    warped[:, :3] = p3
    wnormals[:, :3] = n3
    world2cam = np.linalg.inv(np.asarray(camera_pose, np.float64).reshape(4, 4)).astype(np.float32)
    return renderMesh(intr, warped, triangles, cols, rows, world2cam=world2cam, normals=wnormals, attr=vertices, colors=colors)


def unpack_icp_sums(sums):
    """StreamHelper::get (projective_icp.cpp:43-61): 27 floats -> symmetric A (6x6) and b (6)."""
    A = np.zeros((6, 6), F32)
    b = np.zeros(6, F32)
    shift = 0
    for i in range(6):
        for j in range(i, 7):
            v = sums[shift]
            shift += 1
            if j == 6:
                b[i] = v
            else:
                A[i, j] = A[j, i] = v
    return A, b


def rodrigues_affine(r):
    """cv::Affine3f(rvec, t) (projective_icp.cpp:162 `Affine3f Tinc(Vec3f(r.val), Vec3f(r.val+3))`): Rodrigues rotation of
    r[0:3], translation r[3:6].  OpenCV is not in the reference tree; evaluated here in f64 and rounded to f32."""
    rvec = np.asarray(r[:3], np.float64)
    theta = float(np.linalg.norm(rvec))
    R = np.eye(3)
    if theta >= np.finfo(np.float64).eps:
        c, s = math.cos(theta), math.sin(theta)
        k = rvec / theta
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = c * np.eye(3) + (1 - c) * np.outer(k, k) + s * K
    T = np.eye(4, dtype=F32)
    T[:3, :3] = R.astype(F32)
    T[:3, 3] = np.asarray(r[3:6], F32)
    return T


class ProjectiveICP:
    """kfusion::cuda::ProjectiveICP (projective_icp.cpp:64-213).  The device part (correspondences + the 27 sums) is the
    HIP kernel pair behind dfusion_icp_sums_*; the 6x6 solve is host side as in the reference (cv::solve DECOMP_SVD there,
    numpy f64 here -- OpenCV's Jacobi SVD is a third-party algorithm outside the reference tree, so the pose is matched to
    tolerance, not bit for bit; the sums are)."""
    MAX_PYRAMID_LEVELS = 4

    def __init__(self):
        self.angle_thres_ = float(F32(20.0) * F32(0.017453293))      # deg2rad(20.f), projective_icp.cpp:66
        self.dist_thres_ = 0.1
        self.setIterationsNum([10, 5, 4, 0])
        self._ws = None
        self._sums = None
        self.last_accepted = None

    def setIterationsNum(self, iters):
        iters = list(iters)[:self.MAX_PYRAMID_LEVELS]
        self.iters_ = iters + [0] * (self.MAX_PYRAMID_LEVELS - len(iters))

    def setDistThreshold(self, d):
        self.dist_thres_ = float(d)

    def setAngleThreshold(self, a):
        self.angle_thres_ = float(a)

    def getUsedLevelsNum(self):
        i = self.MAX_PYRAMID_LEVELS - 1
        while i >= 0 and not self.iters_[i]:
            i -= 1
        return i + 1

    def thresholds(self):
        """ComputeIcpHelper ctor (projective_icp.cpp:11-15): (dist2_thres, min_cosine) as floats."""
        return float(F32(self.dist_thres_) * F32(self.dist_thres_)), float(F32(math.cos(F32(self.angle_thres_))))

    def sums(self, level_intr, curr, ncurr, prev, nprev, affine, depth_variant=False):
        """One ComputeIcpHelper::operator() call: returns the 27 sums (numpy f32)."""
        kind = U16 if depth_variant else F4
        np_, nppitch, rows, cols = _image(nprev, F4)
        cp, cpitch = _sized(curr, kind, rows, cols)
        ncp, ncpitch = _sized(ncurr, F4, rows, cols)
        pp, ppitch = _sized(prev, kind, rows, cols)
        need = capi.lib().dfusion_icp_workspace_floats(cols, rows)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(max(need, 27 * 1200 + 27), dtype=torch.float32, device=nprev.device)
        if self._sums is None:
            self._sums = torch.empty(27, dtype=torch.float32, device=nprev.device)
        acc = torch.zeros(1, dtype=torch.int32, device=nprev.device)
        d2, mc = self.thresholds()
        L = capi.lib()
        fn = L.dfusion_icp_sums_depth if depth_variant else L.dfusion_icp_sums_points
        capi.check(fn(cp, cpitch, ncp, ncpitch, pp, ppitch, np_, nppitch, cols, rows, capi.floats(aff12(affine)), level_intr.as_proj(), d2, mc,
                      self._ws.data_ptr(), self._sums.data_ptr(), acc.data_ptr(), _stream()),
                   "dfusion_icp_sums_depth" if depth_variant else "dfusion_icp_sums_points")
        out = self._sums.cpu().numpy().copy()                      # cudaStreamSynchronize + pinned copy in the reference (:45)
        self.last_accepted = int(acc.item())
        return out

    def estimateTransformDevice(self, intr, curr_pyr, ncurr_pyr, prev_pyr, nprev_pyr, depth_variant=False):
        """The same loop as ONE enqueue (dfusion_icp_estimate): sums, 6x6 solve and pose update all on the GPU, one read-back at the
        end.  Returns (ok, affine 4x4 f32 curr -> prev)."""
        n = self.getUsedLevelsNum()
        levels = (capi.DfIcpLevel * n)()
        kind = U16 if depth_variant else F4
        for l in range(n):
            np_, nppitch, rows, cols = _image(nprev_pyr[l], F4)
            cp, cpitch = _sized(curr_pyr[l], kind, rows, cols)
            ncp, ncpitch = _sized(ncurr_pyr[l], F4, rows, cols)
            pp, ppitch = _sized(prev_pyr[l], kind, rows, cols)
            levels[l] = capi.DfIcpLevel(cp.value, cpitch, ncp.value, ncpitch, pp.value, ppitch, np_.value, nppitch, cols, rows, self.iters_[l])
        rows0, cols0 = nprev_pyr[0].shape[:2]
        need = capi.lib().dfusion_icp_workspace_floats(cols0, rows0) + 27
        dev = nprev_pyr[0].device
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(max(need, 27 * 1200 + 27), dtype=torch.float32, device=dev)
        state = torch.empty(13, dtype=torch.float32, device=dev)
        d2, mc = self.thresholds()
        capi.check(capi.lib().dfusion_icp_estimate(levels, n, 1 if depth_variant else 0, intr.as_proj(), d2, mc, self._ws.data_ptr(), state.data_ptr(),
                                                   _stream()), "dfusion_icp_estimate")
        st = state.cpu().numpy()
        affine = np.eye(4, dtype=F32)
        affine[:3, :3] = st[:9].reshape(3, 3)
        affine[:3, 3] = st[9:12]
        return bool(st[12] != 0), affine

    def estimateTransform(self, intr, curr_pyr, ncurr_pyr, prev_pyr, nprev_pyr, depth_variant=False):
        """projective_icp.cpp:129-213 with the reference's control flow (one host solve per iteration).  Returns (ok, affine 4x4 f32
        curr -> prev)."""
        affine = np.eye(4, dtype=F32)
        for level in range(self.getUsedLevelsNum() - 1, -1, -1):
            li = intr_level(intr, level)                           # setLevelIntr, projective_icp.cpp:17-23
            for _ in range(self.iters_[level]):
                s = self.sums(li, curr_pyr[level], ncurr_pyr[level], prev_pyr[level], nprev_pyr[level], affine, depth_variant)
                A, b = unpack_icp_sums(s)
                det = float(np.linalg.det(A.astype(np.float64)))   # cv::determinant(A), :150
                if abs(det) < 1e-15 or math.isnan(det):
                    return False, affine
                r = np.linalg.solve(A.astype(np.float64), b.astype(np.float64))     # cv::solve(A, b, r, DECOMP_SVD), :159
                affine = (rodrigues_affine(r).astype(np.float64) @ affine.astype(np.float64)).astype(F32)   # Tinc * affine, :163
        return True, affine
