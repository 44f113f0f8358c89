"""dfusion_extract_mesh / TsdfVolume.fetchMesh (dynamicfusion_amd/csrc/dfusion_mesh.hip) against the numpy restatement of the rule,
tests/mesh_ref.py: vertices as uint32 bits, triangles exactly, both in the rule's order."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import mesh_ref as R
import oracle_lib as O
from dynamicfusion_amd import TsdfVolume, WarpField, build, capi, mesh_io, synth

pytestmark = pytest.mark.gpu
F32 = np.float32


def pose44(aff12):
    T = np.eye(4, dtype=F32)
    T[:3, :3] = np.asarray(aff12[:9], F32).reshape(3, 3)
    T[:3, 3] = aff12[9:]
    return T


def gpu_volume(vol_u32, dims, aff12=R.IDENT, slab=None, vs=R.VS):
    """A TsdfVolume whose voxel size is vs exactly (mesh_ref.VS: 3 / 256 per voxel), holding vol_u32's stored planes."""
    v = TsdfVolume(dims, slab=slab)
    v.setSize([float(F32(d) * vs[i]) for i, d in enumerate(dims)])
    assert np.array_equal(v.getVoxelSize().view(np.uint32), np.array(vs, F32).view(np.uint32))
    v.setPose(pose44(aff12))
    v.upload(vol_u32[v.z_store0:v.z_store0 + v.z_store_n])
    return v


def assert_same_mesh(vertices, triangles, ref):
    gv, gt = vertices.cpu().numpy(), triangles.cpu().numpy().view(np.uint32)
    assert gv.shape == ref.vertices.shape and gt.shape == ref.triangles.shape, (gv.shape, gt.shape, ref.vertices.shape, ref.triangles.shape)
    assert np.array_equal(gv.view(np.uint32), ref.vertices.view(np.uint32))
    assert np.array_equal(gt, ref.triangles)


@pytest.mark.parametrize("name,vol,dims,aff", [("sphere", R.sphere_volume, R.SPHERE_DIMS, R.IDENT), ("torus", R.torus_volume, R.TORUS_DIMS, R.IDENT),
                                               ("cut", R.cut_sphere_volume, R.SPHERE_DIMS, R.IDENT), ("hand", R.handmade_volume, R.HAND_DIMS, R.POSE)],
                         ids=["sphere32", "torus48x40x32", "cut_sphere32", "handmade16"])
def test_mesh_equals_restatement(name, vol, dims, aff):
    v = gpu_volume(vol(), dims, aff)
    vertices, triangles = v.fetchMesh()
    ref = R.mesh_of(name)
    assert v.last_mesh_counts_ == (len(ref.vertices), len(ref.triangles)) and len(ref.triangles) > 500
    assert_same_mesh(vertices, triangles, ref)


def test_scene_volume_at_a_rotated_pose():
    sc, ref_vol = R.scene_small()
    pose = R.rotated_pose()
    v = TsdfVolume(sc.cfg.dims)
    v.setSize([sc.cfg.size] * 3)
    v.setPose(pose)
    v.upload(ref_vol)
    ref = R.extract_mesh(ref_vol, sc.cfg.dims, sc.vs, synth.aff12(pose))
    assert len(ref.triangles) > 10000
    assert_same_mesh(*v.fetchMesh(), ref)


def raw_call(v, vcap, tcap, guard=4):
    """dfusion_extract_mesh with the given capacities into buffers followed by `guard` rows of guard words -> (vertices, triangles, counts)."""
    vb = torch.full((vcap + guard, 4), -7.0, dtype=torch.float32, device="cuda")
    tb = torch.full((tcap + guard, 3), -7, dtype=torch.int32, device="cuda")
    counts = torch.full((2,), 123, dtype=torch.int64, device="cuda")
    capi.check(capi.lib().dfusion_extract_mesh(v.c_volume(), v.c_slab(), capi.floats(synth.aff12(v.getPose())), C.c_void_p(vb.data_ptr()) if vcap else None, vcap,
                                               C.c_void_p(tb.data_ptr()) if tcap else None, tcap, C.c_void_p(counts.data_ptr()), None), "dfusion_extract_mesh")
    torch.cuda.synchronize()
    return vb, tb, tuple(int(c) for c in counts.tolist())


def test_empty_volume_and_count_only():
    v = TsdfVolume(R.SPHERE_DIMS)
    vertices, triangles = v.fetchMesh()
    assert v.last_mesh_counts_ == (0, 0) and vertices.shape == (0, 4) and triangles.shape == (0, 3)
    assert raw_call(v, 0, 0)[2] == (0, 0)                               # counts are WRITTEN (they held 123)
    v = gpu_volume(R.torus_volume(), R.TORUS_DIMS)
    ref = R.mesh_of("torus")
    _, _, counts = raw_call(v, 0, 0)                                     # count-only: null arrays
    assert counts == (len(ref.vertices), len(ref.triangles))
    vb, tb, counts_full = raw_call(v, counts[0], counts[1])
    assert counts_full == counts
    assert_same_mesh(vb[:counts[0]], tb[:counts[1]], ref)
    assert (vb[counts[0]:] == -7).all() and (tb[counts[1]:] == -7).all()
    L = capi.lib()
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    aff = capi.floats(R.IDENT)
    assert L.dfusion_extract_mesh(v.c_volume(), None, aff, None, 5, None, 0, C.c_void_p(cnt.data_ptr()), None) == 100001     # capacity without an array
    assert L.dfusion_extract_mesh(v.c_volume(), None, aff, None, 0, None, 0, None, None) == 100001
    assert L.dfusion_extract_mesh(capi.DfVolume(), None, aff, None, 0, None, 0, C.c_void_p(cnt.data_ptr()), None) == 100001


@pytest.mark.parametrize("short", ["vertices", "triangles", "both"])
def test_capacity_one_short_writes_nothing_past_it(short):
    v = gpu_volume(R.sphere_volume(), R.SPHERE_DIMS)
    ref = R.mesh_of("sphere")
    nv, nt = len(ref.vertices), len(ref.triangles)
    vcap = nv - (short != "triangles")
    tcap = nt - (short != "vertices")
    vb, tb, counts = raw_call(v, vcap, tcap)
    assert counts == (nv, nt)                                            # still the full counts
    assert (vb[vcap:] == -7).all() and (tb[tcap:] == -7).all()


SLABS = {"4 slabs": [(0, 8), (8, 8), (16, 8), (24, 8)], "uneven": [(0, 5), (5, 13), (18, 3), (21, 11)]}


@pytest.mark.parametrize("split", list(SLABS), ids=["4x8", "5_13_3_11"])
def test_slab_meshes(split):
    vol, dims = R.torus_volume(), R.TORUS_DIMS
    full = R.mesh_of("torus")

    def soup(m_v, m_t):                                                  # triangles as triples of vertex positions, sorted
        t = m_v[:, :3].view(np.uint32)[m_t.astype(np.int64)].reshape(-1, 9)
        return t[np.lexsort(t.T[::-1])]
    parts = []
    for z0, zn in SLABS[split]:
        v = gpu_volume(vol, dims, slab=(z0, zn, 1))                      # 1 halo plane
        ref = R.extract_mesh(vol[v.z_store0:v.z_store0 + v.z_store_n], dims, R.VS, R.IDENT, slab=(v.z_store0, v.z_store_n, z0, zn))
        vertices, triangles = v.fetchMesh()
        assert_same_mesh(vertices, triangles, ref)
        parts.append(soup(vertices.cpu().numpy(), triangles.cpu().numpy().view(np.uint32)))
    assert sum(len(p) for p in parts) == len(full.triangles)
    allp = np.concatenate(parts)
    assert np.array_equal(allp[np.lexsort(allp.T[::-1])], soup(full.vertices, full.triangles))


def test_fetch_mesh_with_normals():
    v = gpu_volume(R.sphere_volume(), R.SPHERE_DIMS)
    vertices, triangles, normals = v.fetchMesh(with_normals=True)
    ref = R.mesh_of("sphere")
    assert_same_mesh(vertices, triangles, ref)
    ovol = O.make_volume(R.sphere_volume(), R.SPHERE_DIMS, np.array(R.VS, F32), v.getTruncDist(), v.getMaxWeight())
    rn = O.extract_normals(ovol, R.IDENT, np.eye(3, dtype=F32), ref.vertices, v.getGradientDeltaFactor())
    gn = normals.cpu().numpy()
    assert np.array_equal(np.isnan(gn), np.isnan(rn)) and np.array_equal(gn.view(np.uint32), rn.view(np.uint32))
    # the gradient normal of a vertex agrees with the face normals of the triangles around it.  Measured (restatement + oracle on the
    # CPU, and the same here since both are bit-equal): every normal is finite (4980 of 4980) and 1.000 of them have a positive dot
    # product with every adjacent face normal; asserted with a small margin below that
    fn, _ = R.face_normals(ref.vertices, ref.triangles)
    t = ref.triangles.astype(np.int64)
    finite = np.isfinite(gn[:, 0])
    good = np.ones(len(gn), bool)
    for q in range(3):
        bad = ~((gn[t[:, q], :3].astype(np.float64) * fn).sum(1) > 0)
        good[t[bad, q]] = False
    print("finite %d of %d, agreeing fraction %.4f" % (finite.sum(), len(gn), good[finite].mean()))
    assert finite.mean() > 0.99 and good[finite].mean() >= 0.99


def test_vertices_through_an_identity_warp_keep_their_bits():
    v = gpu_volume(R.sphere_volume(), R.SPHERE_DIMS)
    vertices, _ = v.fetchMesh()
    p = vertices[:, :3].contiguous()
    nodes = p[::50].cpu().numpy()
    wf = WarpField(k=4)
    wf.init(nodes, sigma=0.05)
    q = p.clone()
    wf.warp(q)
    torch.cuda.synchronize()
    assert len(nodes) >= 4 and np.array_equal(q.cpu().numpy().view(np.uint32), p.cpu().numpy().view(np.uint32))


def test_headless_frame_mesh_writes_the_python_mirrors_ply(tmp_path):
    from scene import Scene
    cfg = synth.Config(64, 1.0, cols=160, rows=120, nodes=0, k=4)
    frames = 2
    sc = Scene(cfg, n_frames=frames, with_nodes=False)
    _, app = build.build_host()
    fin, fout, ply = str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(tmp_path / "cxx.ply")
    with open(fin, "wb") as f:
        f.write(synth.aff12(sc.pose).tobytes())
        f.write(np.asarray(cfg.intr, F32).tobytes())
        for i in range(frames):
            f.write(sc.depths[i].tobytes())
            f.write(synth.aff12(sc.cam_poses[i]).tobytes())
    r = subprocess.run([app, "mesh", ply, str(cfg.dims[0]), str(cfg.size), str(cfg.cols), str(cfg.rows), str(frames), "0", str(cfg.k), fin, fout],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    nv = int(np.prod(cfg.dims))
    vol = np.fromfile(fout, np.uint32, count=nv).reshape(cfg.dims[2], cfg.dims[1], cfg.dims[0])     # the volume the harness fused from those frames
    v = TsdfVolume(cfg.dims)
    v.setSize([cfg.size] * 3)
    v.setPose(sc.pose)
    v.upload(vol)
    vertices, triangles = v.fetchMesh()
    assert triangles.shape[0] > 10000
    mine = str(tmp_path / "py.ply")
    mesh_io.write_ply(mine, vertices, triangles)
    assert open(ply, "rb").read() == open(mine, "rb").read()
    assert os.path.getsize(ply) > 13 * triangles.shape[0]
