"""dfusion_extract_cloud and dfusion_extract_normals outside the thin shells that `integrate` makes: noise at every shape where a lane,
a row or a wave-item ends differently, volumes crafted so that a workgroup's LDS buffer is filled exactly, flushed in mid-list or
bypassed (tests/volume_cases.py; tests/test_volume_readers_rule.py shows without the kernel which rounds they make), capacities short
of the cloud on both write paths, a second call appending behind the first, slab edges, the normals' border gate and points that are
not numbers.  Through the C-ABI into buffers followed by guard rows; clouds as sorted rows of uint32 against O.extract_cloud, counts
exactly; normals bit for bit against O.extract_normals of the same points in the same order."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_ref as R
import oracle_lib as O
import volume_cases as VC
from dynamicfusion_amd import capi, synth
from test_gpu_mesh import gpu_volume

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD, SENTINEL = 4, -7.0
DF_E_INVALID = 100001
ROTATED = synth.aff12(R.rotated_pose())


def ptr(t):
    return C.c_void_p(t.data_ptr())


def new_buffer(rows):
    return torch.full((max(rows, 1) + GUARD, 4), SENTINEL, dtype=torch.float32, device="cuda")


def extract(v, aff, capacity, buf=None, count=None, stream=None):
    """dfusion_extract_cloud into `buf` (default: max(capacity, 1) rows + GUARD rows, all SENTINEL) -> (return code, buffer as numpy, count)."""
    buf = new_buffer(capacity) if buf is None else buf
    count = torch.zeros(1, dtype=torch.int64, device="cuda") if count is None else count
    rc = capi.lib().dfusion_extract_cloud(v.c_volume(), v.c_slab(), capi.floats(aff), ptr(buf), capacity, ptr(count), stream)
    torch.cuda.synchronize()
    return rc, buf.cpu().numpy(), int(count.item())


def assert_untouched(rows):
    assert (rows == SENTINEL).all()


def assert_cloud(v, aff, ref_sorted, n):
    """One call with capacity n: the count, the set, and nothing behind it."""
    rc, got, count = extract(v, aff, n)
    assert rc == 0 and count == n
    assert np.array_equal(VC.sort_rows(got[:n]), ref_sorted)
    assert_untouched(got[n:])
    return got[:n]


def multiset_contained(got, ref):
    """Every row of `got` (uint32 [m, 4]) occurs in `ref` at least as often."""
    u, inv = np.unique(np.concatenate([ref, got]), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    return bool((np.bincount(inv[len(ref):], minlength=len(u)) <= np.bincount(inv[:len(ref)], minlength=len(u))).all())


def gpu_normals(v, aff, points, n):
    """dfusion_extract_normals of the first n rows of the device tensor `points` -> numpy [n, 4]; GUARD rows behind the output stay."""
    out = new_buffer(n)
    rinv = np.linalg.inv(np.asarray(aff[:9], np.float64).reshape(3, 3)).astype(F32)
    capi.check(capi.lib().dfusion_extract_normals(v.c_volume(), v.c_slab(), capi.floats(aff), capi.floats(rinv.reshape(-1)), ptr(points), n,
                                                  v.getGradientDeltaFactor(), ptr(out), None), "dfusion_extract_normals")
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert n >= 1
    assert_untouched(out[n:])
    return out[:n]


def oracle_normals(v, vol, dims, vs, aff, points):
    rinv = np.linalg.inv(np.asarray(aff[:9], np.float64).reshape(3, 3)).astype(F32)
    return O.extract_normals(VC.ovolume(vol, dims, vs), aff, rinv, points, v.getGradientDeltaFactor())


def assert_normals(v, vol, dims, vs, aff, cloud, min_finite=None):
    """The normals of the GPU's own points, in its order, are the oracle's: same bits off NaN, NaN where the oracle has NaN."""
    n = len(cloud)
    got = gpu_normals(v, aff, torch.from_numpy(np.ascontiguousarray(cloud)).cuda(), n)
    want = oracle_normals(v, vol, dims, vs, aff, cloud)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    if min_finite is not None:
        assert np.isfinite(want[:, :3]).all(1).mean() >= min_finite


# ---- 1. noise at every shape where a lane, a row or an item ends differently, and at sizes with many workgroups
@pytest.mark.parametrize("p_invalid", R.FUZZ_P_INVALID, ids=["all_valid", "p_invalid_0.1"])
@pytest.mark.parametrize("index", range(len(R.FUZZ_DIMS)), ids=["%dx%dx%d" % d for d in R.FUZZ_DIMS])
def test_noise_shapes_equal_oracle(index, p_invalid):
    dims = R.FUZZ_DIMS[index]
    vol, _ = R.fuzz_case(index, p_invalid)
    ref, n = VC.oracle_cloud(vol, dims)
    assert (n == 0) == (dims[2] == 1)                                    # 4x1x1 and 12x5x1: no plane is scanned
    v = gpu_volume(vol, dims, R.POSE)
    cloud = assert_cloud(v, R.POSE, ref, n)
    if dims == (24, 11, 13):
        assert_normals(v, vol, dims, R.VS, R.POSE, cloud, min_finite=0.4)


@pytest.mark.parametrize("p_invalid", [0.0, 0.1, 0.3, 0.6])
@pytest.mark.parametrize("dims", [VC.NOISE_DIMS, VC.BIG_DIMS], ids=["64x48x44", "128x96x86"])
def test_noise_of_many_workgroups_equals_oracle(dims, p_invalid):
    """p_invalid 0: every round is `direct`; 0.3: every round is buffered, with a flush in mid-list; 0.1: both (the rule test)."""
    name = "noise_%s" % p_invalid
    ref, n = VC.named_cloud(name, dims)
    v = gpu_volume(VC.case(name, dims), dims, R.POSE)
    cloud = assert_cloud(v, R.POSE, ref, n)
    if dims == VC.NOISE_DIMS:
        assert_normals(v, VC.case(name, dims), dims, R.VS, R.POSE, cloud, min_finite=0.4)


def test_anisotropic_voxels_at_a_rotated_pose():
    dims = (24, 11, 13)
    vol = R.noise_volume(dims, 19, 0.1)
    ref, n = VC.oracle_cloud(vol, dims, aff12=ROTATED, vs=R.ANISO_VS)
    v = gpu_volume(vol, dims, ROTATED, vs=R.ANISO_VS)
    cloud = assert_cloud(v, ROTATED, ref, n)
    assert n > 1000
    assert_normals(v, vol, dims, R.ANISO_VS, ROTATED, cloud, min_finite=0.4)


# ---- 2. the crafted rounds: buffer exactly full, flushed in mid-list, one point past it, bypassed by 4 points and by two buffers' worth
@pytest.mark.parametrize("name,total", [("z_parity", 16384), ("z_parity_split", 16448), ("z_parity_even_x", 8192), ("checker", 47040),
                                        ("one_past", 4100)])
def test_crafted_rounds(name, total):
    ref, n = VC.named_cloud(name)
    assert n == total
    v = gpu_volume(VC.case(name), VC.CRAFTED_DIMS, R.POSE)
    cloud = assert_cloud(v, R.POSE, ref, n)
    assert_normals(v, VC.case(name), VC.CRAFTED_DIMS, R.VS, R.POSE, cloud)


@pytest.mark.parametrize("dims", [(16, 6, 5), VC.NOISE_DIMS], ids=["16x6x5", "64x48x44"])
@pytest.mark.parametrize("name", ["checker", "z_parity"])
def test_crafted_volumes_at_other_shapes(name, dims):
    ref, n = VC.named_cloud(name, dims)
    v = gpu_volume(VC.case(name, dims), dims, R.POSE)
    cloud = assert_cloud(v, R.POSE, ref, n)
    if dims == VC.NOISE_DIMS:
        assert_normals(v, VC.case(name, dims), dims, R.VS, R.POSE, cloud)


# ---- 3. capacities: the count is always n, nothing is written at or behind `capacity` on either write path
CAPACITY_CASES = {"buffered": ("z_parity", VC.CRAFTED_DIMS), "direct": ("z_parity_split", VC.CRAFTED_DIMS), "both": ("noise_0.1", VC.NOISE_DIMS)}


@pytest.mark.parametrize("which", ["0", "1", "half", "n-1", "n", "n+3"])
@pytest.mark.parametrize("path", list(CAPACITY_CASES))
def test_capacities(path, which):
    name, dims = CAPACITY_CASES[path]
    ref, n = VC.named_cloud(name, dims)
    cap = {"0": 0, "1": 1, "half": n // 2, "n-1": n - 1, "n": n, "n+3": n + 3}[which]
    v = gpu_volume(VC.case(name, dims), dims, R.POSE)
    rc, got, count = extract(v, R.POSE, cap)                            # (capacity 0 still gets a buffer: the ABI refuses a null one)
    assert rc == 0 and count == n
    written = min(n, cap)
    assert_untouched(got[written:])
    rows = np.ascontiguousarray(got[:written]).view(np.uint32)
    assert multiset_contained(rows, ref)
    if cap >= n:
        assert np.array_equal(VC.sort_rows(got[:n]), ref)


# ---- 4. *count is incremented: a second call appends behind the first
def test_second_call_appends_behind_the_first():
    ref1, n1 = VC.named_cloud("z_parity")
    ref2, n2 = VC.named_cloud("noise_0.1", VC.NOISE_DIMS)
    buf = new_buffer(n1 + n2)
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    rc, got, c = extract(gpu_volume(VC.case("z_parity"), VC.CRAFTED_DIMS, R.POSE), R.POSE, n1 + n2, buf, count)
    assert rc == 0 and c == n1
    rc, got, c = extract(gpu_volume(VC.case("noise_0.1", VC.NOISE_DIMS), VC.NOISE_DIMS, R.POSE), R.POSE, n1 + n2, buf, count)
    assert rc == 0 and c == n1 + n2
    assert np.array_equal(VC.sort_rows(got[:n1]), ref1)
    assert np.array_equal(VC.sort_rows(got[n1:n1 + n2]), ref2)
    assert np.array_equal(VC.sort_rows(got[:n1 + n2]), VC.sort_rows(np.concatenate([ref1, ref2])))
    assert_untouched(got[n1 + n2:])


# ---- 5. slab edges
SLAB_DIMS = (20, 9, 12)


def slab_volume():
    return R.noise_volume(SLAB_DIMS, 23, 0.1)


def slab_cloud(z0, zn):
    """The GPU's cloud (sorted rows) of the slab that owns [z0, z0 + zn), stored with one halo plane where one exists; compared with the oracle's."""
    vol = slab_volume()
    v = gpu_volume(vol, SLAB_DIMS, R.POSE, slab=(z0, zn, 1))
    ref, n = VC.oracle_cloud(np.ascontiguousarray(vol[v.z_store0:v.z_store0 + v.z_store_n]), SLAB_DIMS,
                             slab=(v.z_store0, v.z_store_n, z0, zn))
    assert_cloud(v, R.POSE, ref, n)
    return ref


@pytest.mark.parametrize("z0,zn,empty", [(5, 1, False), (0, 1, False), (8, 4, False), (11, 1, True), (5, 0, True)],
                         ids=["one_plane", "one_plane_bottom", "top_clamped_at_Z-1", "top_plane_alone", "owns_no_plane"])
def test_slab_edges(z0, zn, empty):
    assert (len(slab_cloud(z0, zn)) == 0) == empty


def test_three_uneven_slabs_are_the_whole():
    whole, n = VC.oracle_cloud(slab_volume(), SLAB_DIMS)
    parts = np.concatenate([slab_cloud(z0, zn) for z0, zn in [(0, 5), (5, 1), (6, 6)]])
    assert len(parts) == n > 1000 and np.array_equal(VC.sort_rows(parts), whole)


def test_slab_without_the_plane_above_it_is_refused():
    v = gpu_volume(slab_volume(), SLAB_DIMS, R.POSE, slab=(2, 4, 0))     # planes 2 .. 5 stored; the +z edges of plane 5 want plane 6
    assert v.z_own0 + v.z_own_n < SLAB_DIMS[2] and v.z_store0 + v.z_store_n == v.z_own0 + v.z_own_n
    count = torch.full((1,), 123, dtype=torch.int64, device="cuda")
    rc, got, c = extract(v, R.POSE, 100, count=count)
    assert rc == DF_E_INVALID and c == 123
    assert_untouched(got)


# ---- 6. the normals' border gate, points that are not numbers, and the ends of the launch
@pytest.mark.parametrize("dims", [(24, 11, 13), VC.NOISE_DIMS], ids=["24x11x13", "64x48x44"])
def test_normals_border_gate(dims):
    """Identity pose: the point g * voxel_size has nearest voxel g.  NaN at g = 1 and dim - 2, the oracle's value at 2 and dim - 3."""
    vol = R.noise_volume(dims, 7, 0.0)
    v = gpu_volume(vol, dims, R.IDENT)
    pts, gate = [], []
    for axis in range(3):
        for g in (1, 2, dims[axis] - 3, dims[axis] - 2):
            p = [F32(d // 2) * R.VS[i] for i, d in enumerate(dims)]
            p[axis] = F32(g) * R.VS[axis]
            assert int(np.rint(F32(p[axis]) * (F32(1) / R.VS[axis]))) == g
            pts.append(p + [0.0]); gate.append(g in (1, dims[axis] - 2))
    pts, gate = np.array(pts, F32), np.array(gate)
    got = gpu_normals(v, R.IDENT, torch.from_numpy(pts).cuda(), len(pts))
    want = oracle_normals(v, vol, dims, R.VS, R.IDENT, pts)
    assert np.isnan(got[gate, :3]).all() and np.isnan(want[gate, :3]).all()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    assert np.isfinite(want[~gate, :3]).all(1).sum() >= 6               # (the open side of the gate is exercised)


@pytest.mark.parametrize("aff", [R.IDENT, ROTATED], ids=["identity", "rotated"])
def test_normals_of_points_that_are_not_numbers_are_nan(aff):
    dims = (24, 11, 13)
    vol = R.noise_volume(dims, 7, 0.0)
    v = gpu_volume(vol, dims, aff)
    c = np.array([float(F32(d // 2) * R.VS[i]) for i, d in enumerate(dims)])                # the central voxel, in the volume frame
    centre = (np.asarray(aff[:9], np.float64).reshape(3, 3) @ c + np.asarray(aff[9:], np.float64)).astype(F32)
    pts = [list(centre) + [0.0]]
    for axis in range(3):
        for bad in (np.nan, np.inf, -np.inf, 1e30, -1e30):
            p = list(centre) + [0.0]
            p[axis] = bad
            pts.append(p)
    pts = np.array(pts, F32)
    got = gpu_normals(v, aff, torch.from_numpy(pts).cuda(), len(pts))
    assert np.isfinite(got[0]).all()                                     # (the same point with nothing wrong in it has a normal)
    assert np.isnan(got[1:, :3]).all()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_normals_launch_ends(n):
    ref, total = VC.named_cloud("noise_0.1", VC.NOISE_DIMS)
    pts = np.ascontiguousarray(ref[total // 3:total // 3 + 300].view(F32))
    vol = VC.case("noise_0.1", VC.NOISE_DIMS)
    v = gpu_volume(vol, VC.NOISE_DIMS, R.POSE)
    got = gpu_normals(v, R.POSE, torch.from_numpy(pts).cuda(), n)       # (300 points lie in the input: rows n .. 299 must not be read out)
    want = oracle_normals(v, vol, VC.NOISE_DIMS, R.VS, R.POSE, pts[:n])
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


# ---- 7. the same call twice, and on a fresh stream
def test_same_case_twice_and_on_a_fresh_stream():
    ref, n = VC.named_cloud("noise_0.1", VC.NOISE_DIMS)
    v = gpu_volume(VC.case("noise_0.1", VC.NOISE_DIMS), VC.NOISE_DIMS, R.POSE)
    assert_cloud(v, R.POSE, ref, n)
    assert_cloud(v, R.POSE, ref, n)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        buf, count = new_buffer(n), torch.zeros(1, dtype=torch.int64, device="cuda")
        rc, got, c = extract(v, R.POSE, n, buf, count, stream=C.c_void_p(s.cuda_stream))
    assert rc == 0 and c == n and np.array_equal(VC.sort_rows(got[:n]), ref)
    assert_untouched(got[n:])
    assert_cloud(v, R.POSE, ref, n)
