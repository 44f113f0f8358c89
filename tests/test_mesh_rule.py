"""The mesh rule of dfusion_extract_mesh (include/dfusion.h; marching tetrahedra on the Kuhn subdivision), checked on its numpy
restatement tests/mesh_ref.py by properties no wrong rule passes by luck: closed, consistently oriented, right Euler characteristic.
No GPU: tests/test_gpu_mesh.py then pins the HIP kernels to the restatement bit for bit."""
import numpy as np

import mesh_ref as R
import oracle_lib as O
from dynamicfusion_amd import mesh_io, synth


def near_surface_corners_are_valid(vol, dist):
    """Every corner of a cell the surface passes through lies within sqrt(3) voxels of it: |tsdf| <= 0.44 < 1, so the cell is meshed."""
    _, valid, _ = R.decode(vol)
    near = np.abs(dist) <= np.sqrt(3.0)
    assert near.sum() > 1000 and valid[near].all()
    assert np.abs(np.clip(dist[near] / 4.0, -1, 1)).max() <= 0.44


def assert_closed_oriented(mesh, euler):
    und, use, fwd = R.edge_use(mesh.triangles)
    assert (use == 2).all() and (fwd == 1).all()                     # every edge in exactly two triangles, once in each direction
    V, E, F = len(mesh.vertices), len(und), len(mesh.triangles)
    assert V - E + F == euler, (V, E, F)
    assert len(np.unique(mesh.triangles)) == V                        # no vertex unreferenced
    assert mesh.triangles.max() < V


def test_case_table_orientation_depends_on_case_and_parity_only():
    N, _, _, FLIP = R.case_table()
    assert [int(n) for n in N[0]] == [0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0]
    for t, p in enumerate(R.PERMS):
        assert (N[t] == N[0]).all()
        want = FLIP[0] ^ bool(R.perm_parity(p))
        assert (FLIP[t] == want)[N[0] > 0].all()


def test_sphere_is_a_closed_oriented_sphere():
    near_surface_corners_are_valid(R.sphere_volume(), R.sphere_dist(R.SPHERE_DIMS, R.SPHERE_C, R.SPHERE_R))
    m = R.mesh_of("sphere")
    assert len(m.triangles) > 1000
    assert_closed_oriented(m, 2)
    n, cen = R.face_normals(m.vertices, m.triangles)
    centre = np.array(R.SPHERE_C) * np.array(R.VS, np.float64)
    assert ((n * (cen - centre)).sum(1) > 0).all()


def test_torus_is_a_closed_oriented_torus():
    near_surface_corners_are_valid(R.torus_volume(), R.torus_dist(R.TORUS_DIMS))
    m = R.mesh_of("torus")
    assert len(m.triangles) > 1000
    assert_closed_oriented(m, 0)
    n, cen = R.face_normals(m.vertices, m.triangles)
    vs = float(R.VS[0])
    c = cen / vs - np.array(R.TORUS_C)
    ring = np.hypot(c[:, 0], c[:, 1])
    core = np.stack([c[:, 0] / ring * R.TORUS_R, c[:, 1] / ring * R.TORUS_R, np.zeros(len(c))], 1)     # nearest point of the tube's axis
    assert ((n * (c - core)).sum(1) > 0).all()


def test_cut_sphere_is_open_only_on_the_volume_faces():
    m = R.mesh_of("cut")
    und, use, fwd = R.edge_use(m.triangles)
    assert use.max() == 2 and (fwd[use == 2] == 1).all() and (use == 1).sum() > 50
    X, Y, Z = R.SPHERE_DIMS
    lo = np.array([0.5 * float(v) for v in R.VS])
    hi = np.array([(d - 0.5) * float(v) for d, v in zip((X, Y, Z), R.VS)])
    p = m.vertices[:, :3].astype(np.float64)
    a, b = p[und[use == 1, 0]], p[und[use == 1, 1]]
    on_face = ((np.abs(a - lo) < 1e-9) & (np.abs(b - lo) < 1e-9)) | ((np.abs(a - hi) < 1e-9) & (np.abs(b - hi) < 1e-9))
    assert on_face.any(1).all()                                       # both ends on one boundary plane of the voxel centres


def test_handmade_volume_zeros_and_invalid_blocks():
    vol = R.handmade_volume()
    half = vol & 0xffff
    assert (half == 0).any() and (half == 0x8000).any()               # +0 and -0, both outside
    m = R.mesh_of("hand")
    assert len(m.triangles) > 500 and not np.isnan(m.vertices).any()
    _, valid, inside = R.decode(vol)
    z, y, x, s = m.owner.T
    off = np.array(R.OFFS)[s]
    assert valid[z, y, x].all() and valid[z + off[:, 2], y + off[:, 1], x + off[:, 0]].all()     # no edge to an invalid voxel has a vertex
    assert not inside[8].any() and (inside[z, y, x] != inside[z + off[:, 2], y + off[:, 1], x + off[:, 0]]).all()
    und, use, fwd = R.edge_use(m.triangles)
    assert use.max() == 2 and (fwd[use == 2] == 1).all()
    openv = R.open_edge_vertices(m, R.HAND_DIMS)
    once = und[use == 1]
    assert len(once) > 20 and openv[once].all()                       # open only along the volume's sides and the invalid blocks
    interior = ~openv
    assert interior.sum() > 100                                       # and there is a closed part to speak of
    # the surface lies on the lattice plane z = 8 of the volume frame: undo the pose
    aff = R.POSE.astype(np.float64)
    local = (m.vertices[:, :3].astype(np.float64) - aff[9:]) @ aff[:9].reshape(3, 3)
    assert np.abs(local[:, 2] - 8.5 * float(R.VS[2])).max() < 1e-6


def test_axis_edge_vertices_are_the_oracles_cloud():
    sc, ref = R.scene_small()
    aff = synth.aff12(R.rotated_pose())
    m = R.extract_mesh(ref, sc.cfg.dims, sc.vs, aff)
    cloud, n = O.extract_cloud(sc.ovol(ref), aff, 1 << 22)
    assert n == cloud.shape[0] > 1000
    axis = set(map(bytes, np.ascontiguousarray(m.vertices[np.isin(m.owner[:, 3], [0, 1, 3])]).view(np.uint32)))
    assert all(bytes(p) in axis for p in np.ascontiguousarray(cloud).view(np.uint32))
    und, use, _ = R.edge_use(m.triangles)
    assert use.max() == 2


def test_write_ply_round_trip(tmp_path):
    m = R.mesh_of("hand")
    nrm = np.arange(len(m.vertices) * 4, dtype=np.float32).reshape(-1, 4)
    for normals in (None, nrm):
        path = tmp_path / "m.ply"
        mesh_io.write_ply(str(path), m.vertices, m.triangles, normals)
        raw = path.read_bytes()
        head, body = raw.split(b"end_header\n", 1)
        lines = head.decode("ascii").split("\n")
        assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
        nv = int([l for l in lines if l.startswith("element vertex")][0].split()[-1])
        nf = int([l for l in lines if l.startswith("element face")][0].split()[-1])
        props = [l.split()[-1] for l in lines if l.startswith("property float")]
        assert (nv, nf) == (len(m.vertices), len(m.triangles))
        assert props == (["x", "y", "z"] if normals is None else ["x", "y", "z", "nx", "ny", "nz"])
        assert "property list uchar int vertex_indices" in lines
        vb = nv * 4 * len(props)
        want_v = m.vertices[:, :3] if normals is None else np.concatenate([m.vertices[:, :3], nrm[:, :3]], 1)
        assert body[:vb] == np.ascontiguousarray(want_v, "<f4").tobytes()
        faces = np.frombuffer(body[vb:], dtype=np.uint8).reshape(nf, 13)
        assert (faces[:, 0] == 3).all()
        assert np.ascontiguousarray(faces[:, 1:]).tobytes() == m.triangles.astype("<u4").tobytes()


# ---- the volumes that tests/test_gpu_mesh_edges.py meshes on the GPU: what they reach, shown here without the kernel
def fuzz_set():
    return [(R.FUZZ_DIMS[i], p) + R.fuzz_case(i, p) for i in range(len(R.FUZZ_DIMS)) for p in R.FUZZ_P_INVALID]


def test_noise_volume_holds_what_it_says():
    vol = R.noise_volume((16, 16, 16), 18, 0.1)
    half, weight = vol & 0xffff, vol >> 16
    tsdf = half.astype(np.uint16).view(np.float16).astype(np.float32)
    assert np.isfinite(tsdf).all() and np.abs(tsdf).max() <= 1 and weight.max() <= 127
    frac = lambda m: float(m.mean())
    assert 0.03 < frac((half == 0) | (half == 0x8000)) < 0.07 and (half == 0).any() and (half == 0x8000).any()
    assert 0.01 < frac(half == 0xbc00) < 0.03 and 0.03 < frac(half == 0x3c00) < 0.07 and 0.07 < frac(weight == 0) < 0.13
    clean = R.noise_volume((16, 16, 16), 18, 0.0)
    assert R.decode(clean)[1].all()


def test_fuzz_set_reaches_every_corner_pattern_and_every_edge_mask():
    patterns, masks = set(), set()
    for dims, p, vol, m in fuzz_set():
        assert np.isfinite(m.vertices).all()
        assert m.vertices.shape[0] > 0, (dims, p)
        patterns |= set(int(c) for c in np.unique(m.cell_patterns))
        X, Y, Z = dims
        z, y, x, s = m.owner.T
        per_voxel = np.zeros(X * Y * Z, np.int64)
        np.bitwise_or.at(per_voxel, (z * Y + y) * X + x, 1 << s)
        masks |= set(int(c) for c in np.unique(per_voxel))
    assert patterns == set(range(256))
    assert masks == set(range(128))


def test_fuzz_volumes_without_cells_have_vertices_and_no_triangles():
    for dims, p, vol, m in fuzz_set():
        if dims in ((4, 1, 1), (8, 1, 5), (12, 5, 1)):
            assert len(m.vertices) > 0 and len(m.triangles) == 0, (dims, p)
    assert max(len(m.triangles) for _, _, _, m in fuzz_set()) > 5000


def test_checker_fills_the_lane_table_with_every_lane():
    dims = (16, 6, 5)
    m = R.extract_mesh(R.checker_volume(dims), dims, R.VS, R.IDENT)
    n4 = 16 * 6 * 5 // 4
    assert R.lanes_with_a_vertex(m) == n4 == 120 and len(m.vertices) > n4 and len(m.triangles) > 0


def test_one_vertex_per_lane_fills_the_lane_table_with_every_vertex():
    dims = (16, 6, 5)
    m = R.extract_mesh(R.one_vertex_per_lane_volume(dims), dims, R.VS, R.IDENT)
    assert R.lanes_with_a_vertex(m) == len(m.vertices) == 36 and len(m.triangles) == 0


def test_banded_mesh_is_the_mesh_of_the_whole_volume():
    dims, bands = (16, 8, 40), [(0, 5), (17, 6), (33, 7)]
    noise = R.noise_volume(dims, 7, 0.1)
    vol = np.zeros_like(noise)
    for z0, n in bands:
        vol[z0:z0 + n] = noise[z0:z0 + n]
    whole = R.extract_mesh(vol, dims, R.VS, R.POSE)
    banded = R.banded_mesh(vol, dims, R.VS, R.POSE, bands)
    assert len(whole.triangles) > 1000 and len(np.unique(whole.owner[:, 0] // 16)) == 3         # every band has vertices
    assert np.array_equal(banded.vertices.view(np.uint32), whole.vertices.view(np.uint32))
    assert np.array_equal(banded.triangles, whole.triangles)


def test_anisotropic_voxel_sizes_cannot_be_permuted_unseen():
    import itertools
    base = R.extract_mesh(R.torus_volume(), R.TORUS_DIMS, R.ANISO_VS, R.IDENT).vertices.view(np.uint32)
    assert len(set(float(v) for v in R.ANISO_VS)) == 3
    for perm in itertools.permutations(range(3)):
        if perm == (0, 1, 2):
            continue
        other = R.extract_mesh(R.torus_volume(), R.TORUS_DIMS, [R.ANISO_VS[i] for i in perm], R.IDENT).vertices.view(np.uint32)
        assert other.shape == base.shape and not np.array_equal(other, base), perm
