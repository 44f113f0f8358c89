"""Every image entry point of the C-ABI on pitched and offset images (include/dfusion.h: row y starts at base + y * pitch, the pitch a
byte count of the caller's choice).  Each image is a column window [:, x0:x0+cols] of a wider buffer filled with a sentinel bit pattern,
and the images of one call all have DIFFERENT pitches and column offsets, so a kernel that reads one image with another's pitch, writes
whole pitch-wide rows or ignores x0 is caught.  Every test asserts (a) the valid region equals the oracle on the dense copy bit for bit,
(b) every padding byte still holds the sentinel, (c) the result equals the same call on dense tensors.  The gate tests put the dists
pitch at the 32-bit address gates of the rigid sweep (rows * pitch < 2^31) and of the pipelined warped sweep (pitch < 2^24,
rows * pitch < 2^32)."""
import numpy as np
import pytest
import torch

import oracle_lib as O
from dynamicfusion_amd import Intr, capi, compute_dists, frontend, synth
from frontend_ref import BILATERAL, level_intr, thresholds
from nonrigid_loop import transform_ref as _transform_ref      # the numpy restatement of dfusion_transform_points
from scene import Scene
from test_gpu_parity import _filled, assert_volume_parity, make_gpu_volume, make_gpu_warp

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID = 100001
FULL = synth.Config(64, 1.0, cols=640, rows=480, nodes=0, k=4)
RAGGED = synth.Config(64, 1.0, cols=203, rows=117, nodes=0, k=4)
VOL = synth.Config(64, 1.0, cols=203, rows=117, nodes=100, k=4, name="64^3 ragged")

# kind -> (dtype, channels, bytes per pixel, bits dtype, sentinel bits)
KINDS = {"u16": (torch.int16, None, 2, torch.int16, -0x5A5B),           # 0xA5A5
         "f4": (torch.float32, 4, 16, torch.int32, -0x5A5A5A5B),        # 0xA5A5A5A5 in every float
         "bgra": (torch.uint8, 4, 4, torch.uint8, 0xA5)}


class Padded:
    """A [rows, cols(, 4)] image at pixel column x0 of a sentinel-filled buffer whose rows are `pitch` bytes
    (default: (x0 + cols) * bpp + pad)."""

    def __init__(self, rows, cols, kind, pad=0, x0=0, pitch=None):
        dtype, ch, bpp, _, sent = KINDS[kind]
        pitch = (x0 + cols) * bpp + pad if pitch is None else pitch
        assert pitch % bpp == 0 and pitch >= (x0 + cols) * bpp
        self.rows, self.cols, self.x0, self.pitch, self.kind, self.sent = rows, cols, x0, pitch, kind, sent
        self.buf = torch.empty((rows, pitch // bpp) + ((ch,) if ch else ()), dtype=dtype, device="cuda")
        self.bits().fill_(sent)
        self.t = self.buf[:, x0:x0 + cols]

    def bits(self):
        return self.buf.view(KINDS[self.kind][3])

    def padding_intact(self):
        torch.cuda.synchronize()
        b, x1 = self.bits(), self.x0 + self.cols
        for r0 in range(0, self.rows, 16):
            blk = b[r0:r0 + 16]
            if bool((blk[:, :self.x0] != self.sent).any()) or bool((blk[:, x1:] != self.sent).any()):
                return False
        return True

    def np(self):
        a = self.t.contiguous().cpu().numpy()
        return a.view(np.uint16) if self.kind == "u16" else a


def padded(arr, kind, pad=0, x0=0, pitch=None):
    """numpy image (uint16 [r, c] / float32 [r, c, 4] / uint8 [r, c, 4]) -> Padded holding it."""
    p = Padded(arr.shape[0], arr.shape[1], kind, pad, x0, pitch)
    src = np.ascontiguousarray(arr)
    p.t.copy_(torch.from_numpy(src.view(np.int16) if kind == "u16" else src).cuda())
    return p


def dense(arr):
    a = np.ascontiguousarray(arr)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, ref):
    """bit-equal numpy images (got may be a tensor)"""
    if isinstance(got, torch.Tensor):
        got = got.contiguous().cpu().numpy()
        got = got.view(np.uint16) if got.dtype == np.int16 else got
    return got.shape == ref.shape and np.array_equal(bits(got), bits(ref))


def check(outs, refs, dense_outs):
    """(a) oracle, (b) padding, (c) dense call, for a list of Padded outputs."""
    for i, (p, r, d) in enumerate(zip(outs, refs, dense_outs)):
        assert same(p.np(), r), "output %d differs from the oracle" % i
        assert p.padding_intact(), "output %d: padding written" % i
        assert same(p.np(), d if isinstance(d, np.ndarray) else d.contiguous().cpu().numpy().view(r.dtype)), "output %d differs from the dense call" % i


# ---------------------------------------------------------------------------------------------------------------- front end
@pytest.mark.parametrize("cfg", [FULL, RAGGED], ids=["640x480", "203x117"])
def test_front_end_pitched(cfg):
    intr = Intr(*cfg.intr); intr_np = np.array(cfg.intr, F32)
    depth = synth.depth_frame(cfg, 0)
    R, Cc = cfg.rows, cfg.cols
    ksz, ss, sd = BILATERAL["ksz"], BILATERAL["sigma_spatial"], BILATERAL["sigma_depth"]
    # bilateral: src +2 bytes at x0 = 3, dst +66 at x0 = 1
    src = padded(depth, "u16", 2, 3); dst = Padded(R, Cc, "u16", 66, 1)
    frontend.depthBilateralFilter(src.t, ksz, ss, sd, out=dst.t)
    f = O.bilateral(depth, **BILATERAL)
    check([dst, src], [f, depth], [frontend.depthBilateralFilter(dense(depth), ksz, ss, sd), depth])
    # truncation in place: +4096 bytes at x0 = 5
    tr = padded(f, "u16", 4096, 5)
    frontend.depthTruncation(tr.t, 1.2)
    check([tr], [O.truncate_depth(f, 1.2)], [frontend.depthTruncation(dense(f), 1.2)])
    # pyramid: src +66 at x0 = 1, dst +4096 at x0 = 7
    ps = padded(f, "u16", 66, 1); pd = Padded(R // 2, Cc // 2, "u16", 4096, 7)
    frontend.depthBuildPyramid(ps.t, sd, out=pd.t)
    check([pd, ps], [O.depth_pyramid(f, sd), f], [frontend.depthBuildPyramid(dense(f), sd), f])
    # normals + depth mask: depth +2 at x0 = 3 (written in place), normals float4 +16 at x0 = 1
    md = padded(f, "u16", 2, 3); mn = Padded(R, Cc, "f4", 16, 1)
    frontend.computeNormalsAndMaskDepth(intr, md.t, normals=mn.t)
    cm, cn = O.compute_normals_mask_depth(f, intr_np)
    dd = dense(f); dn = frontend.computeNormalsAndMaskDepth(intr, dd)
    check([md, mn], [cm, cn], [dd, dn])
    # points + normals: depth +66 at x0 = 1, points +1024 at x0 = 1, normals dense
    pnd = padded(f, "u16", 66, 1); pp = Padded(R, Cc, "f4", 1024, 1); pn = Padded(R, Cc, "f4")
    frontend.computePointNormals(intr, pnd.t, points=pp.t, normals=pn.t)
    cp, cpn = O.compute_point_normals(f, intr_np)
    gp, gn = frontend.computePointNormals(intr, dense(f))
    check([pp, pn, pnd], [cp, cpn, f], [gp, gn, f])
    # resizeDepthNormals: four images, four pitches
    rd_in = padded(cm, "u16", 4096, 5); rn_in = padded(cn, "f4", 16, 1)
    rd_out = Padded(R // 2, Cc // 2, "u16", 2, 3); rn_out = Padded(R // 2, Cc // 2, "f4", 1024, 2)
    frontend.resizeDepthNormals(rd_in.t, rn_in.t, d=rd_out.t, n=rn_out.t)
    cd2, cn2 = O.resize_depth_normals(cm, cn)
    gd2, gn2 = frontend.resizeDepthNormals(dense(cm), dense(cn))
    check([rd_out, rn_out, rd_in, rn_in], [cd2, cn2, cm, cn], [gd2, gn2, cm, cn])
    # resizePointsNormals: points +1024 at x0 = 1, normals dense, outputs +16 at x0 = 1 and +1024 at x0 = 3
    rp_in = padded(cp, "f4", 1024, 1); rq_in = padded(cpn, "f4")
    rp_out = Padded(R // 2, Cc // 2, "f4", 16, 1); rq_out = Padded(R // 2, Cc // 2, "f4", 1024, 3)
    frontend.resizePointsNormals(rp_in.t, rq_in.t, p=rp_out.t, n=rq_out.t)
    cp2, cq2 = O.resize_points_normals(cp, cpn)
    gp2, gq2 = frontend.resizePointsNormals(dense(cp), dense(cpn))
    check([rp_out, rq_out, rp_in], [cp2, cq2, cp], [gp2, gq2, cp])
    # cloudToDepth: cloud +16 at x0 = 1, depth +66 at x0 = 1
    cc = padded(cp, "f4", 16, 1); cdp = Padded(R, Cc, "u16", 66, 1)
    frontend.cloudToDepth(cc.t, out=cdp.t)
    check([cdp, cc], [O.cloud_to_depth(cp), cp], [frontend.cloudToDepth(dense(cp)), cp])


@pytest.mark.parametrize("cfg", [FULL, RAGGED], ids=["640x480", "203x117"])
def test_renders_pitched(cfg):
    intr = Intr(*cfg.intr); intr_np = np.array(cfg.intr, F32)
    f = O.bilateral(synth.depth_frame(cfg, 0), **BILATERAL)
    pts, nrm = O.compute_point_normals(f, intr_np)
    md, mn = O.compute_normals_mask_depth(f, intr_np)
    R, Cc = cfg.rows, cfg.cols
    light = (0.4, -0.3, 0.2)
    # points +16 at x0 = 1, normals +1024 at x0 = 1, image +12 bytes at x0 = 3
    p, n, img = padded(pts, "f4", 16, 1), padded(nrm, "f4", 1024, 1), Padded(R, Cc, "bgra", 12, 3)
    frontend.renderImage(p.t, n.t, intr, light, image=img.t)
    ref = O.render_points(pts, nrm, light)
    assert len(np.unique(ref[..., 0])) > 30
    check([img, p, n], [ref, pts, nrm], [frontend.renderImage(dense(pts), dense(nrm), intr, light), pts, nrm])
    # depth +66 at x0 = 1, normals dense, image +4096 at x0 = 1
    d, dn, img2 = padded(md, "u16", 66, 1), padded(mn, "f4"), Padded(R, Cc, "bgra", 4096, 1)
    frontend.renderImage(d.t, dn.t, intr, light, image=img2.t)
    check([img2, d], [O.render_depth(md, mn, intr_np, light), md], [frontend.renderImage(dense(md), dense(mn), intr, light), md])
    # tangent colours: normals +16 at x0 = 2, image +8 at x0 = 2
    tn, timg = padded(nrm, "f4", 16, 2), Padded(R, Cc, "bgra", 8, 2)
    frontend.renderTangentColors(tn.t, image=timg.t)
    check([timg, tn], [O.render_tangent_colors(nrm), nrm], [frontend.renderTangentColors(dense(nrm)), nrm])


# ---------------------------------------------------------------------------------------------------------------- ICP
def _icp_inputs(cfg):
    intr_np = np.array(cfg.intr, F32)
    d0, d1 = synth.depth_frame(cfg, 0), synth.depth_frame(cfg, 6)
    out = []
    for d in (d1, d0):                           # curr, prev
        lv = [O.bilateral(d, **BILATERAL)]
        for i in range(1, 3):
            lv.append(O.depth_pyramid(lv[-1], BILATERAL["sigma_depth"]))
        out.append(lv)
    pn = [[O.compute_point_normals(lv[i], level_intr(intr_np, i)) for i in range(3)] for lv in out]
    mk = [[O.compute_normals_mask_depth(lv[i], level_intr(intr_np, i)) for i in range(3)] for lv in out]
    return pn, mk


# per image of a level: (kind, pad bytes, x0) -- curr, ncurr, prev, nprev all different
ICP_LAYOUT = {"points": [("f4", 16, 1), ("f4", 0, 0), ("f4", 1024, 2), ("f4", 48, 1)],
              "depth": [("u16", 2, 3), ("f4", 16, 1), ("u16", 4096, 1), ("f4", 1024, 0)]}


@pytest.mark.parametrize("variant", ["points", "depth"])
@pytest.mark.parametrize("cfg", [FULL, RAGGED], ids=["640x480", "203x117"])
def test_icp_pitched(cfg, variant):
    intr = Intr(*cfg.intr); intr_np = np.array(cfg.intr, F32)
    (pc, pp), (mc, mp) = _icp_inputs(cfg)
    dv = variant == "depth"
    # per level: curr, ncurr, prev, nprev as numpy
    lv = [(mc[i][0], mc[i][1], mp[i][0], mp[i][1]) if dv else (pc[i][0], pc[i][1], pp[i][0], pp[i][1]) for i in range(3)]
    icp = frontend.ProjectiveICP()
    d2t, mcos = icp.thresholds()
    assert (d2t, mcos) == thresholds()
    est = synth.rot_y_about(np.deg2rad(0.4), (0.05, -0.02, 1.0)).astype(F32)
    pads = []
    for level in range(3):
        imgs = [padded(a, k, pad + 2 * level * (k == "u16"), x0) for a, (k, pad, x0) in zip(lv[level], ICP_LAYOUT[variant])]
        pads.append(imgs)
        li = frontend.intr_level(intr, level)
        g = icp.sums(li, *[p.t for p in imgs], est, depth_variant=dv)
        g_acc = icp.last_accepted
        c, acc = O.icp_sums(*lv[level], synth.aff12(est), level_intr(intr_np, level), d2t, mcos, depth_variant=dv)
        gd = icp.sums(li, *[dense(a) for a in lv[level]], est, depth_variant=dv)
        assert g_acc == acc == icp.last_accepted and acc > 100, level
        assert np.array_equal(bits(g), bits(c)) and np.array_equal(bits(g), bits(gd)), "level %d sums" % level
        assert all(p.padding_intact() for p in imgs)
    # the single-enqueue loop: every level's four pitches through DfIcpLevel -- pose bit-equal to the dense run
    ok_p, aff_p = icp.estimateTransformDevice(intr, *[[pads[l][j].t for l in range(3)] for j in range(4)], depth_variant=dv)
    ok_d, aff_d = icp.estimateTransformDevice(intr, *[[dense(lv[l][j]) for l in range(3)] for j in range(4)], depth_variant=dv)
    assert ok_p == ok_d and np.array_equal(bits(aff_p), bits(aff_d))
    assert (ok_p and not np.array_equal(aff_p, np.eye(4, dtype=F32))) or dv


# ---------------------------------------------------------------------------------------------------------------- transform_points
@pytest.mark.parametrize("rows,cols", [(117, 203), (1, 1000)], ids=["203x117", "rows1"])
@pytest.mark.parametrize("sin,sout", [(3, 3), (4, 3), (3, 4)])
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "copy"])
def test_transform_points_pitched(rows, cols, sin, sout, affine):
    rng = np.random.default_rng(rows * 10 + sin * 3 + sout)
    pts = rng.uniform(-2, 2, (rows, cols, sin)).astype(F32)
    pts.reshape(-1, sin)[::37, 1] = np.nan                                  # NaN points go through the arithmetic like any other
    aff = synth.aff12(synth.affine_mul(synth.translation(0.1, -0.2, 0.3), synth.rot_y_about(0.3, (0.2, 0.0, 1.0)))) if affine else None
    ref = _transform_ref(pts, aff)
    if sout == 4:
        ref = np.concatenate([ref, np.zeros((rows, cols, 1), F32)], -1)
    SENT = -0x5A5A5A5B
    def buf(stride, pad):
        w = cols * stride + pad // 4
        b = torch.empty((rows, w), dtype=torch.int32, device="cuda").fill_(SENT)
        return b, w * 4
    ib, ipitch = buf(sin, 20)
    ib.view(torch.float32)[:, :cols * sin] = torch.from_numpy(pts.reshape(rows, -1)).cuda()
    ob, opitch = buf(sout, 1028)
    L = capi.lib()
    aff_c = capi.floats(aff) if affine else None
    assert L.dfusion_transform_points(ib.data_ptr(), ipitch, sin, ob.data_ptr(), opitch, sout, cols, rows, aff_c, None) == 0
    # the same call dense
    dinp = torch.from_numpy(pts).cuda(); dout = torch.empty((rows, cols, sout), dtype=torch.float32, device="cuda")
    assert L.dfusion_transform_points(dinp.data_ptr(), cols * sin * 4, sin, dout.data_ptr(), cols * sout * 4, sout, cols, rows, aff_c, None) == 0
    torch.cuda.synchronize()
    got = ob[:, :cols * sout].contiguous().cpu().numpy().view(F32).reshape(rows, cols, sout)
    nan = np.isnan(ref)                                                     # (a NaN's payload is the hardware's: compare the mask)
    assert nan.any() and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(ref)[~nan])
    assert np.array_equal(bits(dout.cpu().numpy()), bits(got))
    assert bool((ob[:, cols * sout:] == SENT).all()) and bool((ib[:, cols * sin:] == SENT).all())
    # a pitch shorter than cols * stride * 4: refused
    assert L.dfusion_transform_points(ib.data_ptr(), cols * sin * 4 - 2, sin, ob.data_ptr(), opitch, sout, cols, rows, aff_c, None) == INVALID
    assert L.dfusion_transform_points(ib.data_ptr(), ipitch, sin, ob.data_ptr(), cols * sout * 4 - 2, sout, cols, rows, aff_c, None) == INVALID


# ---------------------------------------------------------------------------------------------------------------- volume
def test_compute_dists_and_project_and_remove_pitched():
    sc = Scene(VOL, n_frames=1)
    intr = Intr(*VOL.intr)
    R, Cc = VOL.rows, VOL.cols
    dep = padded(sc.depths[0], "u16", 66, 1); dst = Padded(R, Cc, "u16", 4096, 3)
    compute_dists(dep.t, intr, dists=dst.t)
    check([dst, dep], [sc.dists[0], sc.depths[0]], [compute_dists(dense(sc.depths[0]), intr), sc.depths[0]])
    # dfusion_project_and_remove: in +2 at x0 = 3, out +4096 at x0 = 1
    rng = np.random.default_rng(5)
    n = 20000
    pts = np.zeros((n, 4), F32)
    pts[:, 0] = rng.uniform(-0.9, 0.9, n); pts[:, 1] = rng.uniform(-0.7, 0.7, n); pts[:, 2] = rng.uniform(0.3, 1.6, n)
    pts[::101, 1] = np.nan
    exp_pts, exp_dists, exp_ro, exp_n = O.project_and_remove(sc.dists[0], pts, sc.intr)
    assert 1000 < exp_n < n
    din, dout = padded(sc.dists[0], "u16", 2, 3), padded(sc.dists[0], "u16", 4096, 1)
    dense_out = dense(sc.dists[0])
    results = []
    for a, b in ((din.t, dout.t), (dense(sc.dists[0]), dense_out)):
        dp = torch.from_numpy(pts).cuda(); ro = torch.empty(n, dtype=torch.float32, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        rc = capi.lib().dfusion_project_and_remove(a.data_ptr(), a.stride(0) * 2, b.data_ptr(), b.stride(0) * 2, Cc, R, dp.data_ptr(), n,
                                                   capi.floats(sc.intr), ro.data_ptr(), cnt.data_ptr(), None)
        assert rc == 0
        results.append((dp, ro, int(cnt.item())))
    check([dout, din], [exp_dists, sc.dists[0]], [dense_out, sc.dists[0]])
    for dp, ro, cnt in results:
        assert cnt == exp_n and same(dp, exp_pts) and same(ro, exp_ro)
    # the mirror's psdf on a strided dists view (snapshot dense, removal into the view)
    vol = make_gpu_volume(sc)
    pv = padded(sc.dists[0], "u16", 66, 1)
    ro, pr = vol.psdf(torch.from_numpy(pts[:, :3].copy()).cuda(), pv.t, intr, return_points=True)
    check([pv], [exp_dists], [exp_dists])
    assert same(ro, exp_ro) and same(pr, exp_pts)


def test_integrate_rigid_and_warped_pitched():
    sc = Scene(VOL, n_frames=2)
    intr = Intr(*VOL.intr)
    rigid, warped, split = make_gpu_volume(sc), make_gpu_volume(sc), make_gpu_volume(sc)
    rigid_d, warped_d = make_gpu_volume(sc), make_gpu_volume(sc)
    wf, wf_s, wf_d = make_gpu_warp(sc), make_gpu_warp(sc), make_gpu_warp(sc)
    ref_r, ref_w = sc.new_volume(), sc.new_volume()
    for f in range(2):
        p = padded(sc.dists[f], "u16", 66 if f else 4096, 5 if f else 1)
        d = dense(sc.dists[f])
        rigid.integrate(p.t, sc.cam_poses[f], intr)
        rigid_d.integrate(d, sc.cam_poses[f], intr)
        O.integrate(sc.dists[f], ref_r, sc.ovol(ref_r), synth.aff12(sc.vol2cam(f)), sc.intr)
        for w in (wf, wf_s, wf_d):
            w.set_transforms(torch.from_numpy(sc.dqs[f]).cuda())
        warped.integrate_warped(p.t, sc.cam_poses[f], intr, wf)
        split.integrate_warped_prepare(p.t, sc.cam_poses[f], intr, wf_s)
        split.integrate_warped_sweep(wf_s, sync=True)
        warped_d.integrate_warped(d, sc.cam_poses[f], intr, wf_d)
        O.integrate_warped(sc.dists[f], ref_w, sc.ovol(ref_w), synth.aff12(sc.pose), synth.aff12(sc.world2cam(f)), sc.intr, sc.pos,
                           sc.dqs[f], sc.sigma, VOL.k)
        assert p.padding_intact()
    assert_volume_parity(rigid.download(), ref_r)
    assert_volume_parity(warped.download(), ref_w)
    assert_volume_parity(split.download(), ref_w)
    assert torch.equal(rigid.data(), rigid_d.data()) and torch.equal(warped.data(), warped_d.data())


def test_raycasts_pitched():
    sc = Scene(VOL, n_frames=2, with_nodes=False)
    vol, ref = _filled(sc)
    intr = Intr(*VOL.intr)
    R, Cc = VOL.rows, VOL.cols
    rp, rn, _, stats = O.raycast_points(sc.ovol(ref), synth.aff12(sc.cam2vol(1)), sc.rinv(1), sc.reproj, Cc, R,
                                        VOL.raycast_step_factor, VOL.gradient_delta_factor)
    assert stats[1] > 0.2 * Cc * R
    rd, rdn = O.raycast_depth(sc.ovol(ref), synth.aff12(sc.cam2vol(1)), sc.rinv(1), sc.reproj, Cc, R, VOL.raycast_step_factor,
                              VOL.gradient_delta_factor)
    dp, dn = dense(np.zeros((R, Cc, 4), F32)), dense(np.zeros((R, Cc, 4), F32))
    vol.raycast(sc.cam_poses[1], intr, dp, dn)
    # points +16 at x0 = 1, normals +1024 at x0 = 2
    pp, pn = Padded(R, Cc, "f4", 16, 1), Padded(R, Cc, "f4", 1024, 2)
    vol.raycast(sc.cam_poses[1], intr, pp.t, pn.t)
    check([pp, pn], [rp, rn], [dp, dn])
    # depth +2 at x0 = 3, normals +16 at x0 = 1
    dd, ddn = dense(np.zeros((R, Cc), np.uint16)), dense(np.zeros((R, Cc, 4), F32))
    vol.raycast(sc.cam_poses[1], intr, dd, ddn)
    pd, pdn = Padded(R, Cc, "u16", 2, 3), Padded(R, Cc, "f4", 16, 1)
    vol.raycast(sc.cam_poses[1], intr, pd.t, pdn.t)
    check([pd, pdn], [rd, rdn], [dd, ddn])
    # the two-stage cast on one slab: march (dense keys), shade into points +1024 at x0 = 1 and normals dense-plus-one-pixel
    k64 = torch.empty((R, Cc), dtype=torch.int64, device="cuda")
    vol.raycast_march(sc.cam_poses[1], intr, k64)
    sp, sn = Padded(R, Cc, "f4", 1024, 1), Padded(R, Cc, "f4", 16, 0)
    vol.raycast_shade(sc.cam_poses[1], intr, k64, sp.t, sn.t)
    dsp, dsn = dense(np.zeros((R, Cc, 4), F32)), dense(np.zeros((R, Cc, 4), F32))
    vol.raycast_shade(sc.cam_poses[1], intr, k64, dsp, dsn)
    check([sp, sn], [rp, rn], [dsp, dsn])
    # points of keys over a row band: normals band +16 at x0 = 1 (a band of a padded image), points band +1024 at x0 = 2
    r0, nr = 37, 50
    nb = padded(rn, "f4", 16, 1)
    band_n = nb.t[r0:r0 + nr]
    band_p = Padded(nr, Cc, "f4", 1024, 2)
    vol.raycast_points_of_keys(sc.cam_poses[1], intr, k64, band_n, band_p.t, r0, nr)
    band_d = dense(np.zeros((nr, Cc, 4), F32))
    vol.raycast_points_of_keys(sc.cam_poses[1], intr, k64, dense(rn[r0:r0 + nr]), band_d, r0, nr)
    check([band_p, nb], [rp[r0:r0 + nr], rn], [band_d, rn])


# ---------------------------------------------------------------------------------------------------------------- validation
def test_every_pitch_is_validated():
    """Each image argument of each entry point: the call succeeds with pitch = cols * bpp and returns DF_E_INVALID with 2 bytes less;
    the mirror refuses what the ABI cannot express."""
    cfg = synth.Config(64, 1.0, cols=64, rows=48, nodes=100, k=4)
    sc = Scene(cfg, n_frames=1)
    intr = Intr(*cfg.intr)
    R, Cc = cfg.rows, cfg.cols
    L = capi.lib()
    vol = make_gpu_volume(sc)
    wf = make_gpu_warp(sc)
    d16 = [dense(sc.dists[0]) for _ in range(4)]
    f4 = [dense(np.zeros((R, Cc, 4), F32)) for _ in range(4)]
    img = torch.zeros((R, Cc, 4), dtype=torch.uint8, device="cuda")
    h16 = [torch.zeros((R // 2, Cc // 2), dtype=torch.int16, device="cuda")] + [torch.zeros((R // 2, Cc // 2, 4), dtype=torch.float32, device="cuda")
                                                                                 for _ in range(2)]
    vol.integrate_warped(d16[0], sc.cam_poses[0], intr, wf)          # (builds the index the direct calls below need)
    cv, proj, reproj = vol.c_volume(), intr.as_proj(), intr.as_reproj()
    aff, rinv = vol._raycast_args(sc.cam_poses[0])
    v2c = capi.floats(synth.aff12(sc.vol2cam(0)))
    v2w, w2c = capi.floats(synth.aff12(sc.pose)), capi.floats(synth.aff12(sc.world2cam(0)))
    k64 = torch.empty((R, Cc), dtype=torch.int64, device="cuda")
    vol.raycast_march(sc.cam_poses[0], intr, k64)
    ws = torch.empty(L.dfusion_icp_workspace_floats(Cc, R) + 64, dtype=torch.float32, device="cuda")
    sums = torch.empty(27, dtype=torch.float32, device="cuda")
    state = torch.empty(13, dtype=torch.float32, device="cuda")
    eye = capi.floats(synth.aff12(np.eye(4, dtype=F32)))
    light = capi.floats([0.0, 0.0, 0.0])
    p = lambda t: t.data_ptr()
    U, F, B, UH, FH = 2 * Cc, 16 * Cc, 4 * Cc, Cc, 8 * Cc        # bound of each kind (UH / FH: the half-size outputs)

    def icp_est(pitches, depth):
        lvl = (capi.DfIcpLevel * 1)()
        c, n = (d16 if depth else f4), f4
        lvl[0] = capi.DfIcpLevel(p(c[0]), pitches[0], p(n[1]), pitches[1], p(c[2]), pitches[2], p(n[3]), pitches[3], Cc, R, 2)
        return L.dfusion_icp_estimate(lvl, 1, 1 if depth else 0, proj, 0.01, 0.9, p(ws), p(state), None)

    calls = {
        "dfusion_compute_dists": ([U, U], lambda a, b: L.dfusion_compute_dists(p(d16[0]), a, p(d16[1]), b, Cc, R, proj, None)),
        "dfusion_project_and_remove": ([U, U], lambda a, b: L.dfusion_project_and_remove(p(d16[0]), a, p(d16[1]), b, Cc, R, p(f4[0]), 16, proj,
                                                                                          None, None, None)),
        "dfusion_integrate": ([U], lambda a: L.dfusion_integrate(p(d16[0]), a, Cc, R, cv, None, v2c, proj, None, None)),
        "dfusion_integrate_ex": ([U], lambda a: L.dfusion_integrate_ex(p(d16[0]), a, Cc, R, cv, None, v2c, proj, 0, None, None, None)),
        "dfusion_integrate_warped": ([U], lambda a: L.dfusion_integrate_warped(p(d16[0]), a, Cc, R, cv, None, v2w, w2c, proj, wf.handle, 4, 0,
                                                                                None, None)),
        "dfusion_integrate_warped_prepare": ([U], lambda a: L.dfusion_integrate_warped_prepare(p(d16[0]), a, Cc, R, cv, None, v2w, w2c, proj,
                                                                                                wf.handle, 4, 0, None)),
        "dfusion_raycast_points": ([F, F], lambda a, b: L.dfusion_raycast_points(cv, None, aff, rinv, reproj, p(f4[0]), a, p(f4[1]), b, Cc, R,
                                                                                  0.75, 0.5, None, None)),
        "dfusion_raycast_depth": ([U, F], lambda a, b: L.dfusion_raycast_depth(cv, None, aff, rinv, reproj, p(d16[2]), a, p(f4[1]), b, Cc, R,
                                                                                0.75, 0.5, None)),
        "dfusion_raycast_shade": ([F, F], lambda a, b: L.dfusion_raycast_shade(cv, None, aff, rinv, reproj, p(k64), p(f4[0]), a, p(f4[1]), b,
                                                                                Cc, R, 0.5, None)),
        "dfusion_raycast_points_of_keys": ([F, F], lambda a, b: L.dfusion_raycast_points_of_keys(aff, rinv, reproj, p(k64), p(f4[1]), a,
                                                                                                  p(f4[2]), b, Cc, R, None)),
        "dfusion_raycast_points_of_keys_rows": ([F, F], lambda a, b: L.dfusion_raycast_points_of_keys_rows(aff, rinv, reproj, p(k64), p(f4[1]), a,
                                                                                                            p(f4[2]), b, Cc, R, 8, 20, None)),
        "dfusion_bilateral_filter": ([U, U], lambda a, b: L.dfusion_bilateral_filter(p(d16[0]), a, p(d16[3]), b, Cc, R, 7, 4.5, 0.04, None)),
        "dfusion_truncate_depth": ([U], lambda a: L.dfusion_truncate_depth(p(d16[3]), a, Cc, R, 1.2, None)),
        "dfusion_cloud_to_depth": ([F, U], lambda a, b: L.dfusion_cloud_to_depth(p(f4[0]), a, p(d16[3]), b, Cc, R, None)),
        "dfusion_depth_pyramid": ([U, UH], lambda a, b: L.dfusion_depth_pyramid(p(d16[0]), a, Cc, R, p(h16[0]), b, 0.04, None)),
        "dfusion_compute_normals_mask_depth": ([U, F], lambda a, b: L.dfusion_compute_normals_mask_depth(p(d16[3]), a, p(f4[3]), b, Cc, R, proj,
                                                                                                          None)),
        "dfusion_compute_point_normals": ([U, F, F], lambda a, b, c: L.dfusion_compute_point_normals(p(d16[0]), a, p(f4[2]), b, p(f4[3]), c, Cc, R,
                                                                                                      proj, None)),
        "dfusion_resize_depth_normals": ([U, F, UH, FH], lambda a, b, c, d: L.dfusion_resize_depth_normals(p(d16[0]), a, p(f4[1]), b, Cc, R,
                                                                                                            p(h16[0]), c, p(h16[1]), d, None)),
        "dfusion_resize_points_normals": ([F, F, FH, FH], lambda a, b, c, d: L.dfusion_resize_points_normals(p(f4[0]), a, p(f4[1]), b, Cc, R,
                                                                                                              p(h16[1]), c, p(h16[2]), d, None)),
        "dfusion_render_image_points": ([F, F, B], lambda a, b, c: L.dfusion_render_image_points(p(f4[0]), a, p(f4[1]), b, Cc, R, light, p(img), c,
                                                                                                  None)),
        "dfusion_render_image_depth": ([U, F, B], lambda a, b, c: L.dfusion_render_image_depth(p(d16[0]), a, p(f4[1]), b, Cc, R, proj, light,
                                                                                                p(img), c, None)),
        "dfusion_render_tangent_colors": ([F, B], lambda a, b: L.dfusion_render_tangent_colors(p(f4[1]), a, Cc, R, p(img), b, None)),
        "dfusion_transform_points": ([4 * 4 * Cc, 3 * 4 * Cc], lambda a, b: L.dfusion_transform_points(p(f4[0]), a, 4, p(f4[2]), b, 3, Cc, R, eye,
                                                                                                        None)),
        "dfusion_icp_sums_points": ([F, F, F, F], lambda a, b, c, d: L.dfusion_icp_sums_points(p(f4[0]), a, p(f4[1]), b, p(f4[2]), c, p(f4[3]), d,
                                                                                                Cc, R, eye, proj, 0.01, 0.9, p(ws), p(sums),
                                                                                                None, None)),
        "dfusion_icp_sums_depth": ([U, F, U, F], lambda a, b, c, d: L.dfusion_icp_sums_depth(p(d16[0]), a, p(f4[1]), b, p(d16[2]), c, p(f4[3]),
                                                                                              d, Cc, R, eye, proj, 0.01, 0.9, p(ws), p(sums),
                                                                                              None, None)),
        "dfusion_icp_estimate(points)": ([F, F, F, F], lambda *a: icp_est(a, False)),
        "dfusion_icp_estimate(depth)": ([U, F, U, F], lambda *a: icp_est(a, True)),
    }
    for name, (bounds, call) in calls.items():
        assert call(*bounds) == 0, name
        torch.cuda.synchronize()
        for i in range(len(bounds)):
            short = list(bounds); short[i] -= 2
            assert call(*short) == INVALID, "%s: pitch %d" % (name, i)
    assert L.dfusion_raycast_shade(cv, None, aff, rinv, reproj, p(k64), None, 0, p(f4[1]), F, Cc, R, 0.5, None) == 0   # NULL points: no pitch
    torch.cuda.synchronize()
    # the mirror: a transposed depth, a float4 view not on a pixel boundary, a wrong dtype
    with pytest.raises(ValueError):
        compute_dists(dense(np.zeros((Cc, R), np.uint16)).t(), intr)
    raw = torch.zeros((R, Cc * 4 + 8), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        frontend.renderTangentColors(raw[:, 1:1 + 4 * Cc].unflatten(1, (Cc, 4)))
    with pytest.raises(ValueError):
        frontend.depthBilateralFilter(d16[0].to(torch.int32), 7, 4.5, 0.04)
    with pytest.raises(ValueError):
        vol.integrate(d16[0].float(), sc.cam_poses[0], intr)


# ---------------------------------------------------------------------------------------------------------------- 32-bit address gates
GATES = {
    # image: (pitch bytes, rows) -- rigid short forms need rows * pitch < 2^31; the pipelined warped sweep pitch < 2^24 and rows * pitch < 2^32
    "A": ((1 << 24) - 64, 127),     # both on
    "B": ((1 << 24) - 64, 200),     # rigid short forms off; pipelined sweep on, dists offsets above 2^31
    "C": ((1 << 24) + 64, 128),     # both off (pitch >= 2^24)
    "D": ((1 << 24) - 64, 273),     # both off (rows * pitch >= 2^32): the generic sweep; its last 16 rows start above 2^32 (4.6 GB)
}


@pytest.mark.parametrize("image,k", [("A", 4), ("B", 4), ("C", 4), ("D", 4), ("B", 8)], ids=["A-k4", "B-k4", "C-k4", "D-k4", "B-k8"])
def test_integrate_at_the_address_gates(image, k):
    pitch, rows = GATES[image]
    cfg = synth.Config(64, 1.0, cols=160, rows=rows, nodes=100, k=k)
    fx = cfg.intr[0]
    cfg.intr = (fx, fx * rows / 120.0, cfg.intr[2], rows / 2.0)      # the same vertical field of view as 120 rows: every row sees the volume
    sc = Scene(cfg, n_frames=1)
    intr = Intr(*cfg.intr)
    dists = sc.dists[0]
    ref_r, ref_w = sc.new_volume(), sc.new_volume()
    O.integrate(dists, ref_r, sc.ovol(ref_r), synth.aff12(sc.vol2cam(0)), sc.intr)
    O.integrate_warped(dists, ref_w, sc.ovol(ref_w), synth.aff12(sc.pose), synth.aff12(sc.world2cam(0)), sc.intr, sc.pos, sc.dqs[0], sc.sigma, k)
    # the last 16 rows matter: without them the oracle's volumes differ (so the largest offsets are read)
    cut = dists.copy(); cut[-16:] = 0
    cut_r, cut_w = sc.new_volume(), sc.new_volume()
    O.integrate(cut, cut_r, sc.ovol(cut_r), synth.aff12(sc.vol2cam(0)), sc.intr)
    O.integrate_warped(cut, cut_w, sc.ovol(cut_w), synth.aff12(sc.pose), synth.aff12(sc.world2cam(0)), sc.intr, sc.pos, sc.dqs[0], sc.sigma, k)
    assert not np.array_equal(cut_r, ref_r) and not np.array_equal(cut_w, ref_w)
    if image == "D":                         # (what a 32-bit row offset would wrap: every one of the last 16 rows)
        assert (rows - 16) * pitch >= 1 << 32
    rigid, warped = make_gpu_volume(sc), make_gpu_volume(sc)
    wf = make_gpu_warp(sc, k=k)
    torch.cuda.empty_cache()
    img = padded(dists, "u16", x0=1, pitch=pitch)                    # one image at a time (up to 4.6 GB)
    assert img.t.stride(0) * 2 == pitch and img.t.data_ptr() % 4 == 2
    try:
        rigid.integrate(img.t, sc.cam_poses[0], intr)
        warped.integrate_warped(img.t, sc.cam_poses[0], intr, wf)
        torch.cuda.synchronize()
        assert img.padding_intact()
    finally:
        del img
        torch.cuda.empty_cache()
    assert_volume_parity(rigid.download(), ref_r)
    assert_volume_parity(warped.download(), ref_w)
    rigid_d, warped_d = make_gpu_volume(sc), make_gpu_volume(sc)
    wf_d = make_gpu_warp(sc, k=k)
    rigid_d.integrate(dense(dists), sc.cam_poses[0], intr)
    warped_d.integrate_warped(dense(dists), sc.cam_poses[0], intr, wf_d)
    assert torch.equal(rigid.data(), rigid_d.data()) and torch.equal(warped.data(), warped_d.data())
