"""frontend.renderLiveModel after four frames of the closed non-rigid loop (tests/nonrigid_loop.py, FAST's configuration: 64^3,
160 x 120, extend inside, colour fused after every integrate) on the loop's one volume, colour volume and warp-field handle, against the
same composition made on the CPU from the oracle loop's state: mesh_ref.extract_mesh, the oracle's fetchNormals, color_ref.fetch, the
oracle's warp and render_ref.render.  Points, normals, canonical points and colours are equal bit for bit."""
import numpy as np
import pytest

import color_loop as CL
import color_ref as CR
import mesh_ref as MR
import nonrigid_loop as NL
import oracle_lib as O
import render_ref as RR
from dynamicfusion_amd import frontend, synth

pytestmark = pytest.mark.gpu
F32 = np.float32
CASE = NL.Case("fast4", 64, 160, 120, k=8, frames=4, cam_step=2, node_stride=97, sigma=0.05, radius=0.06, max_new=14)


def last_pose(rec):
    bits = [items["pose"] for f, stage, items in rec if stage == "icp"][-1]
    return np.ascontiguousarray(bits).view(F32).reshape(4, 4)


def cpu_composition(ob, pose):
    """renderLiveModel's four steps from the oracle backend's volume, colour volume and nodes."""
    cfg = ob.cfg
    aff = synth.aff12(ob.pose)
    m = MR.extract_mesh(ob.vol, cfg.dims, ob.vs, aff)
    rinv = np.linalg.inv(ob.pose[:3, :3].astype(np.float64)).astype(F32)
    normals = O.extract_normals(ob._ovol(), aff, rinv, m.vertices, cfg.gradient_delta_factor)
    world2vol = synth.aff12(np.linalg.inv(ob.pose.astype(np.float64)).astype(F32))
    colors = CR.fetch(ob.color, cfg.dims, ob.vs, world2vol, m.vertices)
    wp, wn = O.warp_points(ob.pos, ob.dq, ob.sig, m.vertices[:, :3], normals[:, :3], ob.k)
    warped = np.zeros_like(m.vertices); warped[:, :3] = wp
    wnormals = np.zeros_like(m.vertices); wnormals[:, :3] = wn
    world2cam = synth.aff12(np.linalg.inv(pose.astype(np.float64)).astype(F32))
    return m, RR.render(warped, m.triangles, cfg.cols, cfg.rows, cfg.intr, world2cam=world2cam, normals=wnormals, attr=m.vertices, colors=colors)


def test_render_live_model_after_the_closed_loop_equals_the_cpu_composition():
    ob = CL.ColorOracleBackend(CASE)
    want_rec = NL.run(ob, CASE)
    be = CL.ColorGpuBackend(CASE)
    got_rec = NL.run(be, CASE)
    msg = NL.first_difference(got_rec, want_rec)
    assert msg is None, msg                                              # both loops are in the same state
    pose = last_pose(got_rec)
    assert np.array_equal(pose.view(np.uint32), last_pose(want_rec).view(np.uint32)) and not np.array_equal(pose, np.eye(4, dtype=F32))
    m, want = cpu_composition(ob, pose)
    cfg = CASE.cfg
    got = frontend.renderLiveModel(be.v, be.wf, pose, be.intr, cfg.cols, cfg.rows, color_volume=be.cv)
    assert be.v.last_mesh_counts_ == (len(m.vertices), len(m.triangles))
    for k, g in zip(("points", "normals", "attr", "colors"), got):
        g = g.cpu().numpy()
        g = g.view(np.uint32) if g.dtype == np.float32 else g
        assert np.array_equal(g, want[k]), (k, int((g != want[k]).any(-1).sum()))
    hit = want["tri"] >= 0
    print("mesh %d vertices %d triangles, counts %s" % (len(m.vertices), len(m.triangles), want["counts"]))
    assert len(m.triangles) > 10000 and hit.sum() > 8000 and want["counts"][0] > 5000
    # the warp field moved the surface: canonical point and live point differ under most pixels, by millimetres (measured: median 4.0 mm)
    p, a = want["points"].view(F32)[hit][:, :3], want["attr"].view(F32)[hit][:, :3]
    pw = (p.astype(np.float64) @ pose[:3, :3].astype(np.float64).T + pose[:3, 3]) - a
    d = np.linalg.norm(pw, axis=1)
    assert 1e-4 < np.median(d) < 0.02
    assert len(np.unique(want["colors"][hit][:, :3], axis=0)) > 10       # the checker paint came through
    assert np.isfinite(want["normals"].view(F32)[hit]).all(-1).mean() > 0.8
    # without a colour volume there is no colour image, and the rest is the same
    plain = frontend.renderLiveModel(be.v, be.wf, pose, be.intr, cfg.cols, cfg.rows)
    assert plain[3] is None and all(np.array_equal(x.cpu().numpy().view(np.uint32), y.cpu().numpy().view(np.uint32)) for x, y in zip(plain[:3], got[:3]))
