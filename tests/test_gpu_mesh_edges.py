"""dfusion_extract_mesh outside the smooth 32^3 .. 64^3 volumes of tests/test_gpu_mesh.py: noise that reaches every corner pattern and every
per-voxel edge mask, anisotropic voxels, volume shapes at the unit boundaries, a compact lane table that is exactly full, more than one scan
tile, more than one pass of the count kernel's grid, workspace reuse and streams, slab and capacity edges.  The reference of every
comparison is tests/mesh_ref.extract_mesh (tests/test_mesh_rule.py shows, without the kernel, what these volumes reach): vertices as
uint32 bits, triangles exactly."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mesh_ref as R
import oracle_lib as O
from dynamicfusion_amd import capi, synth
from test_gpu_mesh import assert_same_mesh, gpu_volume, raw_call

pytestmark = pytest.mark.gpu
F32 = np.float32


def assert_guards_intact(vb, tb, vcap, tcap):
    assert (vb[vcap:] == -7).all() and (tb[tcap:] == -7).all()


# ---- 1. noise at every shape where a lane, a row or an item ends differently
@pytest.mark.parametrize("p_invalid", R.FUZZ_P_INVALID, ids=["all_valid", "p_invalid_0.1"])
@pytest.mark.parametrize("index", range(len(R.FUZZ_DIMS)), ids=["%dx%dx%d" % d for d in R.FUZZ_DIMS])
def test_noise_volume_equals_restatement(index, p_invalid):
    vol, ref = R.fuzz_case(index, p_invalid)
    v = gpu_volume(vol, R.FUZZ_DIMS[index], R.POSE)
    vertices, triangles = v.fetchMesh()
    assert v.last_mesh_counts_ == (len(ref.vertices), len(ref.triangles))
    assert_same_mesh(vertices, triangles, ref)


# ---- 2. three different voxel sizes (tests/test_mesh_rule.py: permuting them changes the torus's vertices)
def test_anisotropic_torus_with_normals():
    pose = R.rotated_pose()
    aff = synth.aff12(pose)
    v = gpu_volume(R.torus_volume(), R.TORUS_DIMS, aff, vs=R.ANISO_VS)
    vertices, triangles, normals = v.fetchMesh(with_normals=True)
    ref = R.extract_mesh(R.torus_volume(), R.TORUS_DIMS, R.ANISO_VS, aff)
    assert len(ref.triangles) > 500
    assert_same_mesh(vertices, triangles, ref)
    ovol = O.make_volume(R.torus_volume(), R.TORUS_DIMS, np.array(R.ANISO_VS, F32), v.getTruncDist(), v.getMaxWeight())
    rinv = np.linalg.inv(pose[:3, :3].astype(np.float64)).astype(F32)
    rn = O.extract_normals(ovol, aff, rinv, ref.vertices, v.getGradientDeltaFactor())
    gn = normals.cpu().numpy()
    assert np.isfinite(rn[:, 0]).mean() > 0.99
    assert np.array_equal(np.isnan(gn), np.isnan(rn)) and np.array_equal(gn.view(np.uint32), rn.view(np.uint32))


def test_anisotropic_noise():
    dims, aff = (24, 11, 13), synth.aff12(R.rotated_pose())
    vol = R.noise_volume(dims, 19, 0.1)
    ref = R.extract_mesh(vol, dims, R.ANISO_VS, aff)
    assert len(ref.triangles) > 500
    assert_same_mesh(*gpu_volume(vol, dims, aff, vs=R.ANISO_VS).fetchMesh(), ref)


# ---- 3. the compact lane table exactly full: qcap = min(vertex_capacity, n4) entries, and `fits` is q0 + popc(lanes) <= qcap
# (64, 48, 44): 528 wave-items, so the emit launch has 9 waves in 3 workgroups that take their entries from the one counter
@pytest.mark.parametrize("dims", [(16, 6, 5), (64, 48, 44)], ids=["16x6x5", "64x48x44"])
@pytest.mark.parametrize("kind", ["checker", "one_vertex_per_lane"])
def test_lane_table_exactly_full(kind, dims):
    vol = R.checker_volume(dims) if kind == "checker" else R.one_vertex_per_lane_volume(dims)
    ref = R.extract_mesh(vol, dims, R.VS, R.POSE)
    nv, nt, n4, entries = len(ref.vertices), len(ref.triangles), dims[0] * dims[1] * dims[2] // 4, R.lanes_with_a_vertex(ref)
    if kind == "checker":
        assert entries == n4 and nv > n4 and nt > 0                      # qcap == n4, and every lane holds an entry
    else:
        assert entries == nv and nv < n4 and nt == 0                     # qcap == nv, and every entry-holding lane holds one vertex
    assert min(nv, n4) == entries and (dims == (16, 6, 5) or (n4 + 63) // 64 >= 64)      # the table has exactly as many entries as are taken
    v = gpu_volume(vol, dims, R.POSE)
    vb, tb, counts = raw_call(v, nv, nt)
    assert counts == (nv, nt)
    assert_same_mesh(vb[:nv], tb[:nt], ref)
    assert_guards_intact(vb, tb, nv, nt)


# ---- 4. more than one tile of the scan
# hipcub::DeviceScan::ExclusiveSum hands rocprim::default_config to rocprim::exclusive_scan.  rocprim has no tuned scan configuration for
# gfx950, so default_scan_config<950, unsigned long long> is default_scan_config_base<unsigned long long>: block size 256, items per thread
# max(1, 16 / (sizeof(value) / sizeof(int))) = 8 -- a tile of 2048 items (both figures confirmed by a static_assert compiled for gfx950).
# At most 2048 items take the single-block kernel; more go through the look-back scan, one tile per workgroup.  Three tiles need
# n_items + 1 > 4096, that is more than 4095 * 256 = 1 048 320 voxels: 128 x 96 x 86 = 1 056 768 voxels are 4128 items, 4129 counts, tiles of
# 2048 + 2048 + 33.
SCAN_TILE = 2048
BIG_DIMS = (128, 96, 86)


@functools.lru_cache(None)
def big_noise():
    """(volume, its mesh at POSE) of the three-tile noise volume; shared, read-only."""
    vol = R.noise_volume(BIG_DIMS, 4, 0.1)
    return vol, R.extract_mesh(vol, BIG_DIMS, R.VS, R.POSE)


def test_three_scan_tiles():
    n_items = (BIG_DIMS[0] * BIG_DIMS[1] * BIG_DIMS[2] // 4 + 63) // 64
    assert 2 * SCAN_TILE < n_items + 1 <= 3 * SCAN_TILE
    vol, ref = big_noise()
    v = gpu_volume(vol, BIG_DIMS, R.POSE)
    vertices, triangles = v.fetchMesh()
    assert v.last_mesh_counts_ == (len(ref.vertices), len(ref.triangles)) and len(ref.triangles) > 1000000
    assert_same_mesh(vertices, triangles, ref)


# ---- 5. more than one pass of the count kernel's grid
# The count launch has at most 256 * 32 = 8192 workgroups, each of which takes 1024 lane-items (4 voxels each) per trip of its loop: one
# trip covers 8192 * 1024 = 8 388 608 lane-items = 33 554 432 voxels = 512 planes of 256 x 256.  256 x 256 x 516 = 33 816 576 voxels are
# 8 454 144 lane-items, 65 536 = four planes more: the second trip starts at plane 512, inside the last band.
def test_second_trip_of_the_count_grid():
    dims, bands = (256, 256, 516), [(0, 4), (250, 3), (508, 8)]
    X, Y, Z = dims
    n4, one_trip = X * Y * Z // 4, 256 * 32 * 1024
    assert X * Y * Z == 33816576 and n4 - one_trip == 4 * X * Y // 4 and 508 * X * Y // 4 < one_trip < n4
    vol = np.zeros((Z, Y, X), np.uint32)
    for i, (z0, n) in enumerate(bands):
        vol[z0:z0 + n] = R.noise_volume((X, Y, n), 30 + i, 0.1)
    ref = R.banded_mesh(vol, dims, R.VS, R.POSE, bands)
    v = gpu_volume(vol, dims, R.POSE)
    vertices, triangles = v.fetchMesh()
    assert v.last_mesh_counts_ == (len(ref.vertices), len(ref.triangles)) and len(ref.triangles) > 1000000
    assert_same_mesh(vertices, triangles, ref)


# ---- 6. the workspace is the per-(device, stream) scratch, and its lane table is not zeroed between calls
def test_small_call_over_a_stale_table_and_the_same_call_twice():
    vol, ref = big_noise()
    big = gpu_volume(vol, BIG_DIMS, R.POSE)
    first = big.fetchMesh()
    assert big.last_mesh_counts_ == (len(ref.vertices), len(ref.triangles))
    small_vol, small_ref = R.fuzz_case(R.FUZZ_DIMS.index((20, 3, 9)), 0.1)
    small = gpu_volume(small_vol, (20, 3, 9), R.POSE)
    assert_same_mesh(*small.fetchMesh(), small_ref)                      # the big call's table entries lie under this one
    second = big.fetchMesh()
    assert torch.equal(first[0].view(torch.int32), second[0].view(torch.int32)) and torch.equal(first[1], second[1])
    assert_same_mesh(*second, ref)


def test_fresh_stream_then_the_default_stream():
    ref = R.mesh_of("torus")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        v = gpu_volume(R.torus_volume(), R.TORUS_DIMS)
        vertices, triangles = v.fetchMesh()
        s.synchronize()
        assert_same_mesh(vertices, triangles, ref)
    torch.cuda.synchronize()
    assert_same_mesh(*v.fetchMesh(), ref)


# ---- 7. slab edges
SLAB_DIMS = (20, 9, 12)


@functools.lru_cache(None)
def slab_noise():
    vol = R.noise_volume(SLAB_DIMS, 23, 0.1)
    return vol, R.extract_mesh(vol, SLAB_DIMS, R.VS, R.POSE)


def slab_mesh(z0, zn):
    """(GPU vertices, triangles as numpy) of the slab [z0, z0 + zn) with 1 halo plane where one exists, compared with the restatement's."""
    vol, _ = slab_noise()
    v = gpu_volume(vol, SLAB_DIMS, R.POSE, slab=(z0, zn, 1))
    ref = R.extract_mesh(vol[v.z_store0:v.z_store0 + v.z_store_n], SLAB_DIMS, R.VS, R.POSE, slab=(v.z_store0, v.z_store_n, z0, zn))
    vertices, triangles = v.fetchMesh()
    assert v.last_mesh_counts_ == (len(ref.vertices), len(ref.triangles))
    assert_same_mesh(vertices, triangles, ref)
    return vertices.cpu().numpy(), triangles.cpu().numpy().view(np.uint32)


def test_slab_that_owns_no_plane_has_in_plane_vertices_only():
    vertices, triangles = slab_mesh(5, 0)
    assert len(vertices) > 50 and len(triangles) == 0


@pytest.mark.parametrize("z0,zn", [(5, 1), (0, 1), (8, 4), (11, 1)], ids=["one_plane", "one_plane_bottom", "top", "one_plane_top"])
def test_slab_edges(z0, zn):
    vertices, triangles = slab_mesh(z0, zn)
    assert len(vertices) > 50 and (len(triangles) > 0) == (z0 + 1 < SLAB_DIMS[2])


def test_three_slabs_are_the_whole_as_triangle_soup():
    def soup(m_v, m_t):                                                  # triangles as triples of vertex positions, sorted
        t = m_v[:, :3].view(np.uint32)[m_t.astype(np.int64)].reshape(-1, 9)
        return t[np.lexsort(t.T[::-1])]
    _, full = slab_noise()
    parts = [soup(*slab_mesh(z0, zn)) for z0, zn in [(0, 5), (5, 1), (6, 6)]]
    assert sum(len(p) for p in parts) == len(full.triangles) > 500
    allp = np.concatenate(parts)
    assert np.array_equal(allp[np.lexsort(allp.T[::-1])], soup(full.vertices, full.triangles))


def test_slab_without_the_plane_above_it_is_refused():
    vol, _ = slab_noise()
    v = gpu_volume(vol, SLAB_DIMS, R.POSE, slab=(2, 4, 0))               # planes 2 .. 5 stored; the cells of plane 5 want plane 6
    assert v.z_own0 + v.z_own_n < SLAB_DIMS[2] and v.z_store0 + v.z_store_n == v.z_own0 + v.z_own_n
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    assert capi.lib().dfusion_extract_mesh(v.c_volume(), v.c_slab(), capi.floats(R.POSE), None, 0, None, 0, C.c_void_p(cnt.data_ptr()), None) == 100001
    torch.cuda.synchronize()


# ---- 8. capacities far short: contents unspecified, nothing past either capacity, full counts
@pytest.mark.parametrize("case", ["1_1", "nv_0", "0_nt", "half_nv_nt", "nv_half_nt"])
def test_capacities_far_short(case):
    index = R.FUZZ_DIMS.index((16, 16, 16))
    vol, ref = R.fuzz_case(index, 0.0)
    nv, nt = len(ref.vertices), len(ref.triangles)
    assert nv > 1000 and nt > 1000
    vcap, tcap = {"1_1": (1, 1), "nv_0": (nv, 0), "0_nt": (0, nt), "half_nv_nt": (nv // 2, nt), "nv_half_nt": (nv, nt // 2)}[case]
    v = gpu_volume(vol, (16, 16, 16), R.POSE)
    vb, tb, counts = raw_call(v, vcap, tcap)                             # (raises unless the call returns 0)
    assert counts == (nv, nt)
    assert_guards_intact(vb, tb, vcap, tcap)
