"""The closed non-rigid frame loop -- KinFu::operator() + KinFu::dynamicfusion (kinfu.cpp:220-304, :344-400) with the warp field
grown every frame (dfusion_warp_extend) -- written ONCE over a small backend interface, in the style of frontend_ref.icp_loop, with
two backends that each feed themselves:

  GpuBackend     dynamicfusion_amd.frontend, TsdfVolume, WarpField (one handle for the whole sequence), capi.dfusion_transform_points
  OracleBackend  oracle_lib (bilateral ... solve_data_term), extend_ref.extend_ref, transform_ref (numpy)

run(backend, case) returns the stage record: after every stage of every frame the stage's outputs as numpy arrays (float images as
their bits).  first_difference(a, b) names the first (frame, stage, item) whose bits differ: up to there both loops had equal inputs,
so that stage is the culprit.  nonvacuity(record, case) lists which of the conditions that keep the loop honest (ICP tracks, the
solver moves nodes, the field grows, ...) a record misses; they are conditions on the chosen INPUTS, proven on the oracle alone by
tests/test_oracle_nonrigid_loop.py.

Per frame (parameters of KinFuParams::default_params_dynamicfusion unless the Case says otherwise):
  front end   bilateral filter, 3-level depth pyramid, point normals per level
  frame 0     rigid integrate at the first pose, ray-cast -> prev pyramids, warp field <- every s-th finite point of the cloud
  frames >= 1 ICP (3 levels, host 6x6 solve) -> pose; ray-cast at it; cloud and normals -> packed float3 through transform_points
              (the cloud with the inverse pose, kinfu.cpp:353-383); warp; solve the data term against the live points of level 0; warp;
              extend with the un-warped cloud; compute_dists + warped integrate at the ICP pose; ray-cast -> resized pyramids (next prev)

The scene of synth.depth_frame is rigid, so a smooth frame-dependent offset of a few millimetres (surface_offset_mm) is added to every
depth frame: without it the solver would only absorb ICP error.
"""
import numpy as np

import extend_ref
import oracle_lib as O
from dynamicfusion_amd import synth
from frontend_ref import BILATERAL, icp_loop, level_intr, thresholds

F32 = np.float32
LEVELS = 3
DF_E_INVALID = 100001


class Case:
    """One closed-loop configuration: the volume / image sizes and everything the loop needs that the reference leaves open."""

    def __init__(self, name, dims, cols, rows, k, frames, cam_step, node_stride, sigma, radius, max_new, iters=4, lam=1e-3,
                 amp_mm=4.0, seed=17):
        self.name, self.k, self.frames, self.cam_step = name, int(k), int(frames), int(cam_step)
        self.cfg = synth.Config(dims, 1.0, cols=cols, rows=rows, nodes=0, k=k)
        self.node_stride = int(node_stride)     # s of WarpField::init: every s-th finite point of frame 0's cloud is a node
        self.sigma = float(F32(sigma))          # dg_w of every node, initial and added: small enough to leave unsupported surface
        self.radius = float(F32(radius))        # extend: decimation cell
        self.max_new = int(max_new)             # extend: cap per frame, so that growth goes on over several frames
        self.iters, self.lam = int(iters), float(lam)
        self.amp_mm, self.seed = float(amp_mm), int(seed)

    def with_k(self, k):
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.k = int(k)
        return c


FAST = Case("fast", 64, 160, 120, k=8, frames=7, cam_step=2, node_stride=97, sigma=0.05, radius=0.06, max_new=14)
LONG = Case("long", 128, 320, 240, k=8, frames=13, cam_step=2, node_stride=389, sigma=0.05, radius=0.06, max_new=10)


def surface_offset_mm(case, frame):
    """int32 [rows, cols]: a smooth standing wave over the pixel grid whose amplitude and phase move with the frame number."""
    cfg = case.cfg
    rng = np.random.RandomState(case.seed)
    fu, fv = rng.uniform(1.0, 2.0, 2)
    pu, pv = rng.uniform(0.0, 2 * np.pi, 2)
    u, v = np.meshgrid(np.arange(cfg.cols, dtype=np.float64) / cfg.cols, np.arange(cfg.rows, dtype=np.float64) / cfg.rows)
    wave = np.sin(2 * np.pi * fu * u + pu + 0.35 * frame) * np.cos(2 * np.pi * fv * v + pv - 0.2 * frame)
    return np.rint(case.amp_mm * np.sin(0.6 * frame) * wave).astype(np.int32)


def depth_frames(case):
    out = []
    for f in range(case.frames):
        d = synth.depth_frame(case.cfg, f * case.cam_step)
        moved = np.clip(d.astype(np.int32) + surface_offset_mm(case, f), 1, 65535).astype(np.uint16)
        out.append(np.where(d > 0, moved, 0).astype(np.uint16))
    return out


def transform_ref(pts, aff):
    """numpy float32 restatement of dfusion_transform_points: R(i,0)*x + R(i,1)*y + R(i,2)*z + t(i), products summed left to right;
    aff None = plain re-striding."""
    x, y, z = pts[..., 0], pts[..., 1], pts[..., 2]
    if aff is None:
        return np.stack([x, y, z], -1)
    R, t = aff[:9].reshape(3, 3), aff[9:]
    with np.errstate(invalid="ignore"):
        return np.stack([((R[i, 0] * x + R[i, 1] * y) + R[i, 2] * z) + t[i] for i in range(3)], -1).astype(F32)


def _geometry(cfg):
    vs = np.array([F32(cfg.size) / F32(d) for d in cfg.dims], F32)
    trunc = float(max(F32(cfg.trunc_dist), F32(2.1) * max(vs)))                  # tsdf_volume.cpp:68-73
    return vs, trunc


# ------------------------------------------------------------------------------------------------------------------ oracle backend
class OracleBackend:
    """Images are numpy arrays; the node set is three numpy arrays."""
    name = "oracle"

    def __init__(self, case, skip_second_warp=False):
        cfg = self.cfg = case.cfg
        self.case, self.k = case, case.k
        self.intr = np.array(cfg.intr, F32)
        self.reproj = np.array([F32(1) / F32(cfg.intr[0]), F32(1) / F32(cfg.intr[1]), cfg.intr[2], cfg.intr[3]], F32)
        self.vs, self.trunc = _geometry(cfg)
        self.pose = cfg.volume_pose
        X, Y, Z = cfg.dims
        self.vol = np.zeros((Z, Y, X), np.uint32)
        self.d2t, self.mc = thresholds()
        self.pos = self.dq = self.sig = None
        self.skip_second_warp = skip_second_warp     # a deliberately wrong loop, to show that the comparison can fail and says where
        self.warps = 0
        self.integrate_inputs = []             # (frame, dists, world2cam, pos, dq, sigma, volume before) for the reference-classes leg
        self.solver_points = []                # (frame, pos, canonical points of the solve)
        self.keep_inputs = False

    def _ovol(self):
        return O.make_volume(self.vol, self.cfg.dims, self.vs, self.trunc, self.cfg.max_weight)

    # images
    def np_u16(self, a): return np.ascontiguousarray(a)
    def np_f32(self, a): return np.ascontiguousarray(a, F32)

    def front_end(self, depth):
        d = [O.bilateral(depth, **BILATERAL)]
        for i in range(1, LEVELS):
            d.append(O.depth_pyramid(d[-1], BILATERAL["sigma_depth"]))
        pn = [O.compute_point_normals(d[i], level_intr(self.intr, i)) for i in range(LEVELS)]
        return d, [p for p, _ in pn], [n for _, n in pn]

    def compute_dists(self, depth):
        return O.compute_dists(np.ascontiguousarray(depth), self.intr)

    def integrate(self, dists, cam_pose):
        vol2cam = synth.affine_mul(synth.affine_inv(cam_pose), self.pose)
        return O.integrate(dists, self.vol, self._ovol(), synth.aff12(vol2cam), self.intr)

    def raycast(self, cam_pose):
        cam2vol = synth.affine_mul(synth.affine_inv(self.pose), cam_pose)
        rinv = np.linalg.inv(cam2vol[:3, :3].astype(np.float64)).astype(F32)
        p, n, _, _ = O.raycast_points(self._ovol(), synth.aff12(cam2vol), rinv, self.reproj, self.cfg.cols, self.cfg.rows,
                                      self.cfg.raycast_step_factor, self.cfg.gradient_delta_factor)
        return p, n

    def resize(self, points, normals):
        return O.resize_points_normals(points, normals)

    def icp(self, curr, ncurr, prev, nprev):
        ok, aff, _ = icp_loop(lambda lv, li, a: O.icp_sums(curr[lv], ncurr[lv], prev[lv], nprev[lv], synth.aff12(a), li,
                                                           self.d2t, self.mc)[0], self.intr)
        return ok, aff

    def transform(self, image4, aff12):
        return np.ascontiguousarray(transform_ref(image4, aff12).reshape(-1, 3))

    # warp field
    def init_field(self, pos):
        self.pos = np.ascontiguousarray(pos, F32)
        self.dq = synth.identity_dq(len(pos))
        self.sig = np.full(len(pos), self.case.sigma, F32)

    def nodes(self):
        return self.pos.copy(), self.dq.copy(), self.sig.copy()

    def warp(self, pts, nrm, frame):
        self.warps += 1
        if self.skip_second_warp and self.warps % 2 == 0:
            return pts, nrm
        return O.warp_points(self.pos, self.dq, self.sig, pts, nrm, self.k)

    def solve(self, canonical, live, frame):
        if self.keep_inputs:
            self.solver_points.append((frame, self.pos.copy(), canonical.copy()))
        self.dq, en = O.solve_data_term(self.pos, self.dq, self.sig, canonical, live, self.k, self.case.iters, self.case.lam)
        return en

    def extend(self, pts, frame):
        npos, ndq, nsig, n, w = extend_ref.extend_ref(self.pos, self.dq, self.sig, pts, self.k, self.case.radius, self.case.sigma,
                                                      self.case.max_new)
        if n:
            self.pos, self.dq, self.sig = (np.concatenate([self.pos, npos]), np.concatenate([self.dq, ndq]),
                                           np.concatenate([self.sig, nsig]))
        return n, w

    def integrate_warped(self, dists, cam_pose, frame):
        world2cam = synth.affine_inv(cam_pose)                     # warp_to_live_ stays the identity (warp_field.cpp:26)
        if self.keep_inputs:
            self.integrate_inputs.append((frame, dists.copy(), world2cam, self.pos.copy(), self.dq.copy(), self.sig.copy(), self.vol.copy()))
        return O.integrate_warped(dists, self.vol, self._ovol(), synth.aff12(self.pose), synth.aff12(world2cam), self.intr,
                                  self.pos, self.dq, self.sig, self.k)

    def volume(self):
        return self.vol.copy()

    def extras(self, frame):
        return {}


# --------------------------------------------------------------------------------------------------------------------- GPU backend
class GpuBackend:
    """Images are device tensors; ONE WarpField handle and one TsdfVolume for the whole sequence.

    split: the warped integrate as integrate_warped_prepare on a second stream + integrate_warped_sweep, the prepare issued after the
    solver and the extend of its own frame.  The split run also shows the voiding rules of include/dfusion.h on the way: on the frames of
    `void_frames` a plan is prepared BEFORE the solver; the solver's write-back is the first transforms update since (the plan stays good),
    a set_transforms on top is the second (the sweep must refuse); and a plan prepared before an extend that adds nodes must be refused
    too.  The refused plans are replaced by a fresh prepare, and the results must still be the oracle's.
    cull_off: a second volume swept with cull=False through the same handle after every frame's sweep (volume2())."""
    name = "gpu"

    def __init__(self, case, tables_on_demand=True, split=False, prefetch=True, cull_off=False, void_frames=(2, 4)):
        import torch
        from dynamicfusion_amd import Intr, TsdfVolume, WarpField
        self.torch = torch
        cfg = self.cfg = case.cfg
        self.case, self.k = case, case.k
        self.intr = Intr(*cfg.intr)
        self.split, self.prefetch, self.void_frames = split, prefetch, tuple(void_frames)
        _, trunc = _geometry(cfg)

        def volume():
            v = TsdfVolume(cfg.dims)
            v.setSize([cfg.size] * 3); v.setTruncDist(cfg.trunc_dist); v.setMaxWeight(cfg.max_weight); v.setPose(cfg.volume_pose)
            v.setRaycastStepFactor(cfg.raycast_step_factor); v.setGradientDeltaFactor(cfg.gradient_delta_factor)
            assert v.getTruncDist() == trunc
            return v
        self.v = volume()
        self.v2 = volume() if cull_off else None
        self.wf = WarpField(k=case.k, tables_on_demand=tables_on_demand)
        self.cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.main = torch.cuda.current_stream()
        self.side = torch.cuda.Stream() if split else None
        self.voided = {"second_update": 0, "extend": 0}           # refusals seen (split runs)
        self.pending = None
        self.kept, self.coded = [], []

    def np_u16(self, t): return t.detach().cpu().numpy().view(np.uint16)
    def np_f32(self, t): return t.detach().cpu().numpy()

    def front_end(self, depth):
        from dynamicfusion_amd import frontend, upload_u16
        d = [frontend.depthBilateralFilter(upload_u16(depth), BILATERAL["ksz"], BILATERAL["sigma_spatial"], BILATERAL["sigma_depth"])]
        for i in range(1, LEVELS):
            d.append(frontend.depthBuildPyramid(d[-1], BILATERAL["sigma_depth"]))
        pn = [frontend.computePointNormals(frontend.intr_level(self.intr, i), d[i]) for i in range(LEVELS)]
        return d, [p for p, _ in pn], [n for _, n in pn]

    def compute_dists(self, depth):
        from dynamicfusion_amd import compute_dists, upload_u16
        return compute_dists(depth if self.torch.is_tensor(depth) else upload_u16(depth), self.intr)

    def integrate(self, dists, cam_pose):
        self.cnt.zero_()
        self.v.integrate(dists, cam_pose, self.intr, n_updated=self.cnt)
        if self.v2 is not None:
            self.v2.integrate(dists, cam_pose, self.intr)
        return int(self.cnt.item())

    def raycast(self, cam_pose):
        p = self.torch.empty((self.cfg.rows, self.cfg.cols, 4), dtype=self.torch.float32, device="cuda")
        n = self.torch.empty_like(p)
        self.v.raycast(cam_pose, self.intr, p, n)
        return p, n

    def resize(self, points, normals):
        from dynamicfusion_amd import frontend
        return frontend.resizePointsNormals(points, normals)

    def icp(self, curr, ncurr, prev, nprev):
        from dynamicfusion_amd import frontend
        return frontend.ProjectiveICP().estimateTransform(self.intr, curr, ncurr, prev, nprev)

    def transform(self, image4, aff12):
        from dynamicfusion_amd import capi
        rows, cols = image4.shape[:2]
        out = self.torch.empty((rows * cols, 3), dtype=self.torch.float32, device="cuda")
        capi.check(capi.lib().dfusion_transform_points(image4.data_ptr(), cols * 16, 4, out.data_ptr(), cols * 12, 3, cols, rows,
                                                       capi.floats(aff12) if aff12 is not None else None,
                                                       self.main.cuda_stream), "dfusion_transform_points")
        return out

    def init_field(self, pos):
        self.wf.init(pos, sigma=self.case.sigma)
        self.wf.set_point_tiling(self.cfg.cols)                    # the point sets of the loop are images (kfusion_hip.cpp dynamicfusion)

    def nodes(self):
        pos, _, sig = self.wf._keep
        return pos.cpu().numpy().reshape(-1, 3), self.wf._dq.cpu().numpy().reshape(-1, 8), sig.cpu().numpy().reshape(-1)

    def warp(self, pts, nrm, frame):
        pts, nrm = pts.clone(), nrm.clone()
        self.wf.warp(pts, nrm)
        return pts, nrm

    def _prepare(self, dists, cam_pose):
        self.side.wait_stream(self.main)                           # the caller orders everything but sweeps against the handle's other calls
        with self.torch.cuda.stream(self.side):
            self.v.integrate_warped_prepare(dists, cam_pose, self.intr, self.wf, prefetch=self.prefetch)
        self.main.wait_stream(self.side)

    def _sweep_refused(self):
        from dynamicfusion_amd import capi
        rc = capi.lib().dfusion_integrate_warped_sweep(self.v.c_volume(), self.v.c_slab(), self.wf.handle, None, self.main.cuda_stream)
        return rc == DF_E_INVALID

    def early_plan(self, dists, cam_pose, frame):
        """Split runs, on the frames of void_frames: a plan made before this frame's solver."""
        self.pending = None
        if self.split and frame in self.void_frames:
            self._prepare(dists, cam_pose)
            self.pending = (dists, cam_pose)

    def solve(self, canonical, live, frame):
        dq, en = self.wf.energy_data(canonical, live, iters=self.case.iters, lam=self.case.lam)
        if self.pending is not None and frame == self.void_frames[0]:
            self.wf.set_transforms(dq)                             # the second update since the prepare (the solver's was the first)
            assert self._sweep_refused(), "frame %d: a plan survived two transforms updates" % frame
            self.voided["second_update"] += 1
            self.pending = None
        return en.cpu().numpy()

    def extend(self, pts, frame):
        # (a pending plan is one transforms update old here: still good)
        n, w = self.wf.extend(pts, self.case.radius, sigma=self.case.sigma, max_new=self.case.max_new)
        if self.pending is not None and n > 0:
            assert self._sweep_refused(), "frame %d: a plan survived an extend that added %d nodes" % (frame, n)
            self.voided["extend"] += 1
        self.pending = None
        return n, w

    def integrate_warped(self, dists, cam_pose, frame):
        torch = self.torch
        self.cnt.zero_()
        if self.split:
            self._prepare(dists, cam_pose)
            self.v.integrate_warped_sweep(self.wf, n_updated=self.cnt)
        else:
            self.v.integrate_warped(dists, cam_pose, self.intr, self.wf, n_updated=self.cnt, sync=False, prefetch=self.prefetch)
        nl = self.cfg.dims[2] // 8
        a = torch.zeros(nl, dtype=torch.int64, device="cuda"); c = torch.zeros_like(a)
        self.wf.alive_blocks_per_layer(self.v, a); self.wf.coded_blocks_per_layer(self.v, c)
        self.kept.append(int(a.sum().item())); self.coded.append(int(c.sum().item()))
        if self.v2 is not None:
            self.v2.integrate_warped(dists, cam_pose, self.intr, self.wf, cull=False, sync=False, prefetch=self.prefetch)
        torch.cuda.synchronize()
        return int(self.cnt.item())

    def volume(self):
        return self.v.download().copy()

    def volume2(self):
        return self.v2.download().copy()

    def extras(self, frame):
        return {}


# --------------------------------------------------------------------------------------------------------------------- the loop
def _bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a.view(np.uint32).copy()
    return a.copy()


def _bits_nan(a):
    """Bits of a float array whose NaNs went through float arithmetic (transform_points on ray-cast misses): the payload of such a NaN is
    the hardware's (tests/test_gpu_pitched_images.py), so every NaN is recorded as one pattern; everything else bit for bit."""
    a = np.ascontiguousarray(a, F32)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


def run(be, case, depths=None, on_frame=None):
    """Drives `be` through case.frames frames.  Returns the stage record: a list of (frame, stage, {item: numpy array})."""
    depths = depth_frames(case) if depths is None else depths
    rec = []

    def put(frame, stage, **items):
        rec.append((frame, stage, {k: np.asarray(v) for k, v in items.items()}))

    def put_pyr(frame, stage, pts, nrm, depth=None):
        items = {}
        for i in range(LEVELS):
            items["points%d" % i] = _bits(be.np_f32(pts[i])); items["normals%d" % i] = _bits(be.np_f32(nrm[i]))
            if depth is not None:
                items["depth%d" % i] = be.np_u16(depth[i]).copy()
        put(frame, stage, **items)

    def cast_pyramids(frame, stage, pose):
        p, n = be.raycast(pose)
        pp, nn = [p], [n]
        for i in range(1, LEVELS):
            a, b = be.resize(pp[-1], nn[-1])
            pp.append(a); nn.append(b)
        put_pyr(frame, stage, pp, nn)
        return pp, nn

    pose = synth.camera_pose(case.cfg, 0)
    prev = None
    for f in range(case.frames):
        d_pyr, p_pyr, n_pyr = be.front_end(depths[f])
        put_pyr(f, "front_end", p_pyr, n_pyr, d_pyr)
        if f == 0:
            dists = be.compute_dists(depths[f])                    # kinfu.cpp:226: frame 0 fuses the raw depth
            put(f, "dists", dists=be.np_u16(dists))
            n = be.integrate(dists, pose)
            put(f, "integrate", volume=be.volume(), updated=n, pose=_bits(pose))
            prev = cast_pyramids(f, "raycast_next", pose)
            cloud = be.np_f32(prev[0][0]).reshape(-1, 4)[:, :3]
            seeds = cloud[np.isfinite(cloud).all(1)][::case.node_stride]       # WarpField::init(cv::Mat), warp_field.cpp:49-60
            be.init_field(seeds)
            put(f, "init_field", **_node_items(be))
            if on_frame: on_frame(f, be)
            continue

        ok, aff = be.icp(p_pyr, n_pyr, prev[0], prev[1])
        pose = synth.affine_mul(pose, aff)                          # poses_.back() * affine, kinfu.cpp:277
        put(f, "icp", ok=bool(ok), affine=_bits(aff), pose=_bits(pose))
        if not ok:
            break
        cp, cn = be.raycast(pose)
        put(f, "raycast", points=_bits(be.np_f32(cp)), normals=_bits(be.np_f32(cn)))
        finite = float(np.isfinite(be.np_f32(cp)[..., 0]).mean())
        canonical = be.transform(cp, synth.aff12(synth.affine_inv(pose)))
        normals = be.transform(cn, None)
        live = be.transform(p_pyr[0], None)
        put(f, "transform_points", canonical=_bits_nan(be.np_f32(canonical)), normals=_bits_nan(be.np_f32(normals)),
            live=_bits_nan(be.np_f32(live)), finite=finite)
        dists = be.compute_dists(d_pyr[0])                          # kinfu.cpp:344-400 fuses the filtered depth
        put(f, "dists", dists=be.np_u16(dists))
        if hasattr(be, "early_plan"):
            be.early_plan(dists, pose, f)
        w1p, w1n = be.warp(canonical, normals, f)
        put(f, "warp1", points=_bits_nan(be.np_f32(w1p)), normals=_bits_nan(be.np_f32(w1n)))
        dq_before = be.nodes()[1]
        en = be.solve(w1p, live, f)                                 # optimiseWarpData(canonical (warped), ..., live, ...), kinfu.cpp:389
        put(f, "solve", energy=_bits(en), moved=int((_bits(be.nodes()[1][:, 4:]) != _bits(dq_before[:, 4:])).any(1).sum()),
            **_node_items(be))
        w2p, w2n = be.warp(w1p, w1n, f)                             # kinfu.cpp:391
        put(f, "warp2", points=_bits_nan(be.np_f32(w2p)), normals=_bits_nan(be.np_f32(w2n)))
        n_added, n_winners = be.extend(canonical, f)
        put(f, "extend", n_added=n_added, n_winners=n_winners, **_node_items(be))
        n = be.integrate_warped(dists, pose, f)
        put(f, "integrate_warped", volume=be.volume(), updated=n)
        prev = cast_pyramids(f, "raycast_next", pose)
        if on_frame: on_frame(f, be)
    return rec


def _node_items(be):
    pos, dq, sig = be.nodes()
    return dict(M=len(pos), pos=_bits(pos), dq=_bits(dq), sigma=_bits(sig))


def first_difference(a, b):
    """None, or a message naming the first (frame, stage, item) where two stage records differ, with the count of differing elements."""
    for (fa, sa, ia), (fb, sb, ib) in zip(a, b):
        if (fa, sa) != (fb, sb):
            return "the records diverge: frame %d stage %s against frame %d stage %s" % (fa, sa, fb, sb)
        if sorted(ia) != sorted(ib):
            return "frame %d, stage %s: items %s against %s" % (fa, sa, sorted(ia), sorted(ib))
        for key in ia:
            x, y = ia[key], ib[key]
            if x.shape != y.shape:
                return "frame %d, stage %s, %s: shape %s against %s" % (fa, sa, key, x.shape, y.shape)
            if x.dtype != y.dtype:
                return "frame %d, stage %s, %s: dtype %s against %s" % (fa, sa, key, x.dtype, y.dtype)
            bad = int((x != y).sum())
            if bad:
                return "frame %d, stage %s, %s: %d of %d elements differ" % (fa, sa, key, bad, x.size)
    if len(a) != len(b):
        return "one record has %d stages, the other %d" % (len(a), len(b))
    return None


def stage(rec, frame, name):
    for f, s, items in rec:
        if f == frame and s == name:
            return items
    raise KeyError((frame, name))


def summary(rec, case):
    """The figures of a run: frames, node counts, the frames that added nodes, update counts, finite share of the ray-casts."""
    frames = sorted({f for f, _, _ in rec})
    last = frames[-1]
    return dict(frames=len(frames), M0=int(stage(rec, 0, "init_field")["M"]), M=int(stage(rec, last, "extend")["M"]),
                added={f: int(stage(rec, f, "extend")["n_added"]) for f in frames[1:]},
                updated=[int(stage(rec, f, "integrate_warped" if f else "integrate")["updated"]) for f in frames],
                finite=[float(stage(rec, f, "transform_points")["finite"]) for f in frames[1:]])


def nonvacuity(rec, case):
    """The conditions (on the inputs) without which a loop that does nothing would pass; returns the list of those `rec` misses."""
    miss = []
    frames = sorted({f for f, _, _ in rec})
    if frames != list(range(case.frames)):
        return ["the loop stopped after frame %d" % frames[-1]]
    for f in frames[1:]:
        if not bool(stage(rec, f, "icp")["ok"]):
            miss.append("frame %d: ICP not ok" % f)
        en = stage(rec, f, "solve")["energy"].view(F32)
        if not en[1] < en[0]:
            miss.append("frame %d: energy %g -> %g" % (f, en[0], en[1]))
        if int(stage(rec, f, "solve")["moved"]) < 1:
            miss.append("frame %d: the solver moved no node" % f)
        if float(stage(rec, f, "transform_points")["finite"]) < 0.2:
            miss.append("frame %d: %.3f of the ray-cast finite" % (f, float(stage(rec, f, "transform_points")["finite"])))
    s = summary(rec, case)
    for f, n in enumerate(s["updated"]):
        if n <= 0:
            miss.append("frame %d: update count %d" % (f, n))
    grew = [f for f, n in s["added"].items() if n > 0 and f > 1]
    if len(grew) < 3:
        miss.append("nodes were added after frame 1 on frames %s only" % grew)
    if s["M"] < 1.2 * s["M0"]:
        miss.append("M %d -> %d: less than 20 %% growth" % (s["M0"], s["M"]))
    if not 100 <= s["M0"] <= 300:
        miss.append("the field starts with %d nodes" % s["M0"])
    # blend models are made from the second sweep over the tables on (frame 2's): an extend that adds nodes on a frame >= 3 runs the
    # in-place table update with models present
    if not [f for f in grew if f >= 3]:
        miss.append("no extend added nodes after the second warped sweep")
    return miss
