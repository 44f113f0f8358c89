"""numpy restatement of dfusion_extract_mesh's rule (include/dfusion.h): marching tetrahedra on the Kuhn subdivision.
f32 arithmetic in the stated order, vectorised over edges and cells; the case table is generated here, geometrically, from the
rule's wording -- nothing is taken from the HIP source.  Also the analytic / hand-made volumes the mesh tests share."""
import functools
import itertools

import numpy as np

F32 = np.float32
PERMS = list(itertools.permutations(range(3)))        # lexicographic: xyz, xzy, yxz, yzx, zxy, zyx
OFFS = [(d & 1, (d >> 1) & 1, (d >> 2) & 1) for d in range(1, 8)]     # slot s = d - 1 -> (dx, dy, dz)


# ------------------------------------------------------------------------------------------------ case table
def perm_parity(p):
    return sum(1 for i in range(3) for j in range(i + 1, 3) if p[i] > p[j]) & 1


@functools.lru_cache(None)
def case_table():
    """-> N [6, 16] triangles of tetrahedron t in case m (bit i: local corner i inside); CORNER, SLOT [6, 16, 2, 3]: the owner (cell
    corner code dx + 2 dy + 4 dz) and slot of each triangle vertex, already oriented; FLIP [6, 16] whether the rule's order was turned."""
    N = np.zeros((6, 16), np.int64)
    CORNER = np.zeros((6, 16, 2, 3), np.int64)
    SLOT = np.zeros((6, 16, 2, 3), np.int64)
    FLIP = np.zeros((6, 16), bool)
    lam = 0.3                                           # a point on the open edge (not the midpoint): the orientation cannot depend on it
    for t, (a, b, c) in enumerate(PERMS):
        e = np.eye(3)
        corners = [np.zeros(3), e[a], e[a] + e[b], np.ones(3)]
        for m in range(16):
            ins = [i for i in range(4) if (m >> i) & 1]
            outs = [i for i in range(4) if not (m >> i) & 1]
            if len(ins) in (0, 4):
                continue
            if len(ins) in (1, 3):
                i = ins[0] if len(ins) == 1 else outs[0]
                j, k, l = outs if len(ins) == 1 else ins
                tris = [[(i, j), (i, k), (i, l)]]
            else:
                (i, j), (k, l) = ins, outs
                tris = [[(i, k), (i, l), (j, l)], [(i, k), (j, l), (j, k)]]

            def point(pair):
                u, v = pair
                u, v = (u, v) if (m >> u) & 1 else (v, u)                   # from the inside end
                return corners[u] + lam * (corners[v] - corners[u])
            direction = np.mean([corners[i] for i in outs], 0) - np.mean([corners[i] for i in ins], 0)
            signs = []
            for tri in tris:
                p0, p1, p2 = (point(pr) for pr in tri)
                signs.append(float(np.dot(np.cross(p1 - p0, p2 - p0), direction)))
            assert all(abs(s) > 1e-9 for s in signs) and len({s > 0 for s in signs}) == 1      # both triangles of a quad turn together
            flip = signs[0] < 0
            FLIP[t, m] = flip
            N[t, m] = len(tris)
            for r, tri in enumerate(tris):
                if flip:
                    tri = [tri[0], tri[2], tri[1]]
                for q, (u, v) in enumerate(tri):
                    lo, hi = min(u, v), max(u, v)
                    d = (corners[hi] - corners[lo]).astype(int)
                    cc = corners[lo].astype(int)
                    CORNER[t, m, r, q] = cc[0] + 2 * cc[1] + 4 * cc[2]
                    SLOT[t, m, r, q] = d[0] + 2 * d[1] + 4 * d[2] - 1
    return N, CORNER, SLOT, FLIP


# ------------------------------------------------------------------------------------------------ f32 helpers
def fma32(a, b, c):
    """fmaf(a, b, c) on f32 arrays, exactly: the product is exact in f64, the sum is rounded to ODD in f64 (53 >= 2 * 24 + 2 bits), so
    the final rounding to f32 is the only one that counts."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64).copy()
    fix = (err != 0) & ((bits & 1) == 0) & np.isfinite(s)
    away = (err > 0) == (s > 0)                         # the exact sum lies farther from zero than s
    bits[fix & away] += 1
    bits[fix & ~away] -= 1
    return bits.view(np.float64).astype(F32)


def aff_mul(aff12, V):
    """dfusion_device.h aff_mul: R v + t with dot(a, b) = fmaf(a.x, b.x, fmaf(a.y, b.y, a.z * b.z))."""
    aff12 = np.asarray(aff12, F32).reshape(-1)
    out = np.empty_like(V)
    for i in range(3):
        r = [np.full(V.shape[0], aff12[3 * i + j], F32) for j in range(3)]
        out[:, i] = fma32(r[0], V[:, 0], fma32(r[1], V[:, 1], r[2] * V[:, 2])) + aff12[9 + i]
    return out


def decode(vol_u32):
    half = (vol_u32 & 0xffff).astype(np.uint16)
    tsdf = half.view(np.float16).astype(F32)
    valid = ((vol_u32 >> 16) != 0) & (half != 0x3c00)
    return tsdf, valid, valid & (tsdf < 0)


# ------------------------------------------------------------------------------------------------ the rule
class Mesh:
    pass


def extract_mesh(vol_u32, dims, vs, aff12, slab=None):
    """vol_u32 [z_store_n, Y, X] (the stored planes); slab = (z_store0, z_store_n, z_own0, z_own_n) or None.
    -> Mesh: vertices f32 [n, 4], triangles uint32 [m, 3]; owner [n, 4] (z, y, x, slot; z global) of every vertex; meshed [nz-1.., ..],
    cell_patterns (the 8-bit corner pattern of every meshed cell) and z0 (the first owner plane) for the property tests."""
    X, Y, Z = dims
    z_store0, z_store_n, z_own0, z_own_n = slab if slab is not None else (0, Z, 0, Z)
    z_end = min(z_own0 + z_own_n, Z - 1)
    assert z_end <= z_store0 + z_store_n - 1
    vsx, vsy, vsz = (F32(v) for v in vs)
    out = Mesh()
    out.z0 = z_own0
    if z_end < z_own0:
        out.vertices, out.triangles = np.zeros((0, 4), F32), np.zeros((0, 3), np.uint32)
        out.owner, out.meshed = np.zeros((0, 4), np.int64), np.zeros((0, Y - 1, X - 1), bool)
        out.cell_patterns = np.zeros(0, np.int64)
        return out
    P = np.ascontiguousarray(vol_u32[z_own0 - z_store0:z_end - z_store0 + 1])
    nz = P.shape[0]
    tsdf, valid, inside = decode(P)
    carry = np.zeros((nz, Y, X, 7), bool)
    for s, (dx, dy, dz) in enumerate(OFFS):
        A = (slice(0, nz - dz), slice(0, Y - dy), slice(0, X - dx))
        B = (slice(dz, nz), slice(dy, Y), slice(dx, X))
        carry[A + (s,)] = valid[A] & valid[B] & (inside[A] != inside[B])
    zz, yy, xx, ss = np.nonzero(carry)                                  # C order: ascending (linear voxel index, slot)
    vid = np.full(carry.shape, -1, np.int64)
    vid[zz, yy, xx, ss] = np.arange(zz.size)
    off = np.array(OFFS)[ss]
    Fa = np.abs(tsdf[zz, yy, xx])
    Fn = np.abs(tsdf[zz + off[:, 2], yy + off[:, 1], xx + off[:, 0]])
    d_inv = F32(1) / (Fa + Fn)
    V = np.stack([(xx.astype(F32) + F32(0.5)) * vsx, (yy.astype(F32) + F32(0.5)) * vsy, ((zz + z_own0).astype(F32) + F32(0.5)) * vsz], 1)
    for c, step in enumerate((vsx, vsy, vsz)):
        on = off[:, c] == 1
        Vn = V[:, c] + step
        V[:, c] = np.where(on, (V[:, c] * Fn + Vn * Fa) * d_inv, V[:, c])
    out.vertices = np.zeros((zz.size, 4), F32)
    out.vertices[:, :3] = aff_mul(aff12, V)
    out.owner = np.stack([zz + z_own0, yy, xx, ss], 1)

    # cells
    meshed = np.ones((nz - 1, Y - 1, X - 1), bool)
    in8 = np.zeros(meshed.shape, np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        S = (slice(dz, nz - 1 + dz), slice(dy, Y - 1 + dy), slice(dx, X - 1 + dx))
        meshed &= valid[S]
        in8 |= inside[S].astype(np.int64) << c
    out.meshed = meshed
    cz, cy, cx = np.nonzero(meshed)                                     # ascending linear cell index
    cin = in8[cz, cy, cx]
    out.cell_patterns = cin                                            # the inside / outside corner pattern of every meshed cell
    N, CORNER, SLOT, _ = case_table()
    tri = np.full((cz.size, 6, 2, 3), -1, np.int64)
    for t, (a, b, _c) in enumerate(PERMS):
        v = [0, 1 << a, (1 << a) | (1 << b), 7]
        m = sum(((cin >> v[i]) & 1) << i for i in range(4))
        for r in range(2):
            have = N[t, m] > r
            for q in range(3):
                cc, s = CORNER[t, m, r, q], SLOT[t, m, r, q]
                idx = vid[cz + (cc >> 2), cy + ((cc >> 1) & 1), cx + (cc & 1), s]
                assert (idx[have] >= 0).all()                           # every tetrahedron edge with a sign change carries a vertex
                tri[:, t, r, q] = np.where(have, idx, -1)
    tri = tri.reshape(-1, 3)
    out.triangles = tri[tri[:, 0] >= 0].astype(np.uint32)
    return out


# ------------------------------------------------------------------------------------------------ topology helpers
def edge_use(triangles):
    """-> (undirected edges [E, 2] sorted pairs, times each is used, times used in the direction lo -> hi)."""
    t = triangles.astype(np.int64)
    d = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    und = np.sort(d, 1)
    fwd = d[:, 0] < d[:, 1]
    und_u, inv = np.unique(und, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    return und_u, np.bincount(inv, minlength=len(und_u)), np.bincount(inv, weights=fwd, minlength=len(und_u)).astype(np.int64)


def face_normals(vertices, triangles):
    p = vertices[:, :3].astype(np.float64)
    t = triangles.astype(np.int64)
    return np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]]), (p[t[:, 0]] + p[t[:, 1]] + p[t[:, 2]]) / 3


def open_edge_vertices(mesh, dims):
    """bool per vertex: its lattice edge touches a cell that is not meshed (or lies outside the meshed range) -- where a mesh may be open."""
    X, Y, _ = dims
    nzc = mesh.meshed.shape[0]
    pad = np.zeros((nzc + 2, Y + 1, X + 1), bool)                        # pad[z + 1, y + 1, x + 1] = meshed[z, y, x]
    pad[1:-1, 1:-1, 1:-1] = mesh.meshed
    z, y, x, s = mesh.owner.T
    z = z - mesh.z0
    off = np.array(OFFS)[s]
    touch = np.zeros(z.size, bool)
    for bz, by, bx in itertools.product((0, 1), repeat=3):               # the cells q with q <= p and p + d <= q + 1
        ok = ((off[:, 2] == 0) | (bz == 0)) & ((off[:, 1] == 0) | (by == 0)) & ((off[:, 0] == 0) | (bx == 0))
        touch |= ok & ~pad[z - bz + 1, y - by + 1, x - bx + 1]
    return touch


# ------------------------------------------------------------------------------------------------ volumes
VS = tuple(F32(3.0) / F32(256) for _ in range(3))
IDENT = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F32)
POSE = np.array([0.8, -0.6, 0, 0.6, 0.8, 0, 0, 0, 1, 0.25, -0.5, 1.0], F32)     # a rotation about z and a translation (exercises aff)


def pack(dist_voxels):
    """tsdf = clip(dist / (4 voxels), -1, 1) as half, weight 1."""
    half = np.clip(dist_voxels / 4.0, -1, 1).astype(np.float16).view(np.uint16)
    return half.astype(np.uint32) | np.uint32(1 << 16)


def centres(dims):
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z) + 0.5, np.arange(Y) + 0.5, np.arange(X) + 0.5, indexing="ij")
    return x, y, z


SPHERE_DIMS, SPHERE_C, SPHERE_R = (32, 32, 32), (15.8, 16.7, 16.2), 9.4
TORUS_DIMS, TORUS_C, TORUS_R, TORUS_r = (48, 40, 32), (24.1, 20.2, 16.3), 11.6, 4.7
CUT_C, CUT_R = (5.3, 27.6, 14.9), 11.3


def sphere_dist(dims, c, r):
    x, y, z = centres(dims)
    return np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r


@functools.lru_cache(None)
def sphere_volume():
    return pack(sphere_dist(SPHERE_DIMS, SPHERE_C, SPHERE_R))


@functools.lru_cache(None)
def cut_sphere_volume():
    return pack(sphere_dist(SPHERE_DIMS, CUT_C, CUT_R))


def torus_dist(dims):
    x, y, z = centres(dims)
    ring = np.sqrt((x - TORUS_C[0]) ** 2 + (y - TORUS_C[1]) ** 2) - TORUS_R
    return np.sqrt(ring ** 2 + (z - TORUS_C[2]) ** 2) - TORUS_r


@functools.lru_cache(None)
def torus_volume():
    return pack(torus_dist(TORUS_DIMS))


HAND_DIMS = (16, 16, 16)


@functools.lru_cache(None)
def handmade_volume():
    """The surface exactly on the lattice plane z = 8 (tsdf +0 and -0 there, both outside), cut by the volume's sides, with a block of
    weight-0 voxels and a block of tsdf == 1 voxels astride it."""
    X, Y, Z = HAND_DIMS
    z = np.arange(Z, dtype=np.float64)[:, None, None] * np.ones((Z, Y, X))
    v = pack(z - 8.0)
    assert ((v[8] & 0xffff) == 0).all() and (v[12] & 0xffff == 0x3c00).all() and (v[4] & 0xffff == 0xbc00).all()
    v[8, :, ::2] |= 0x8000                                              # -0 in every other column
    v[6:10, 3:6, 3:6] &= 0xffff                                         # weight 0
    v[7:9, 9:12, 10:13] = (1 << 16) | 0x3c00                            # tsdf == 1
    return v


@functools.lru_cache(None)
def mesh_of(name):
    """The restatement's mesh of a named volume, computed once per process and shared (do not modify)."""
    vol, dims, aff = {"sphere": (sphere_volume, SPHERE_DIMS, IDENT), "cut": (cut_sphere_volume, SPHERE_DIMS, IDENT),
                      "torus": (torus_volume, TORUS_DIMS, IDENT), "hand": (handmade_volume, HAND_DIMS, POSE)}[name]
    return extract_mesh(vol(), dims, VS, aff)


@functools.lru_cache(None)
def scene_small():
    """(Scene, packed volume) of the 64^3 scene after 2 oracle-integrated frames (as tests/test_gpu_extract.py builds it); shared, read-only."""
    import oracle_lib as O
    from dynamicfusion_amd import synth
    from scene import Scene
    cfg = synth.Config(64, 1.0, cols=160, rows=120, nodes=100, k=4, name="64^3 small")
    sc = Scene(cfg, n_frames=2, with_nodes=False)
    ref = sc.new_volume()
    for f in range(2):
        O.integrate(sc.dists[f], ref, sc.ovol(ref), synth.aff12(sc.vol2cam(f)), sc.intr)
    return sc, ref


def rotated_pose():
    """A volume pose with a rotation about a skew axis and a translation (4x4 float32)."""
    ax = np.array([0.3, -0.5, 0.81]); ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    th = 0.7
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T[:3, 3] = [-0.4, 0.3, 0.9]
    return T.astype(F32)


# ------------------------------------------------------------------------------------------------ volumes that reach every lane state
ANISO_VS = (F32(3.0) / F32(256), F32(5.0) / F32(256), F32(7.0) / F32(512))
FUZZ_DIMS = [(4, 1, 1), (4, 2, 2), (4, 7, 3), (8, 1, 5), (12, 5, 1), (20, 3, 9), (36, 7, 5), (260, 3, 2), (16, 16, 16), (24, 11, 13)]
FUZZ_P_INVALID = (0.0, 0.1)


def noise_volume(dims, seed, p_invalid):
    """Every voxel on its own: half tsdf uniform in [-1, 1] (a draw that rounds to +1.0, which would not be valid, is the half below
    it), about 5 % of the voxels +0 or -0 (outside both), 2 % -1.0 (valid, inside), p_invalid / 2 of them +1.0 (not valid); weights
    1 .. 127, p_invalid of them 0.  No NaN, no |tsdf| > 1: the pipeline stores neither.  -> uint32 [Z, Y, X]."""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    half = rng.uniform(-1.0, 1.0, (Z, Y, X)).astype(np.float16).view(np.uint16)
    half[half == 0x3c00] = 0x3bff
    u = rng.random((Z, Y, X))
    half[u < 0.025] = 0x0000
    half[(u >= 0.025) & (u < 0.05)] = 0x8000
    half[(u >= 0.05) & (u < 0.07)] = 0xbc00
    half[(u >= 0.07) & (u < 0.07 + p_invalid / 2)] = 0x3c00
    weight = rng.integers(1, 128, (Z, Y, X)).astype(np.uint32)
    weight[rng.random((Z, Y, X)) < p_invalid] = 0
    return half.astype(np.uint32) | (weight << np.uint32(16))


@functools.lru_cache(None)
def fuzz_case(index, p_invalid):
    """(volume, its mesh at POSE) of FUZZ_DIMS[index], seed 10 + index; shared, read-only."""
    vol = noise_volume(FUZZ_DIMS[index], 10 + index, p_invalid)
    return vol, extract_mesh(vol, FUZZ_DIMS[index], VS, POSE)


def checker_volume(dims):
    """Inside iff x + y + z is odd, |tsdf| = 0.5, weight 1: every axis edge and every body diagonal carries a vertex, so every lane has one."""
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    half = np.where((x + y + z) & 1, 0xb800, 0x3800).astype(np.uint32)
    return half | np.uint32(1 << 16)


def one_vertex_per_lane_volume(dims):
    """On even y and even z only: voxels x = 0 (mod 4) outside, x = 1 (mod 4) inside; everything else has weight 0.  A lane of such a
    row has exactly one vertex (its first x edge), every other lane none, and no cell is meshed."""
    X, Y, Z = dims
    vol = np.zeros((Z, Y, X), np.uint32)
    vol[::2, ::2, 0::4] = (1 << 16) | 0x3800
    vol[::2, ::2, 1::4] = (1 << 16) | 0xb800
    return vol


def lanes_with_a_vertex(mesh):
    """The number of lanes (4 x-adjacent voxels, x0 = 0 mod 4) that own at least one vertex."""
    z, y, x, _ = mesh.owner.T
    return len(np.unique(np.stack([z, y, x >> 2], 1), axis=0))


def banded_mesh(vol, dims, vs, aff, bands):
    """The mesh of a volume that is valid only inside the z-bands (z0, n), ascending, with at least one all-invalid plane between two
    of them: the meshes of the bands, each extracted as a slab of its own (plus the invalid plane above it, which the slab rule wants
    stored), concatenated with the vertex indices offset.  vol: the whole volume [Z, Y, X].  -> Mesh with vertices and triangles only."""
    Z = dims[2]
    vertices, triangles, nv, top = [], [], 0, 0
    for z0, n in bands:
        store_n = min(n + 1, Z - z0)
        assert z0 >= top and z0 + n <= Z
        assert not decode(vol[top:z0])[1].any() and not decode(vol[z0 + n:z0 + store_n])[1].any()
        m = extract_mesh(vol[z0:z0 + store_n], dims, vs, aff, slab=(z0, store_n, z0, n))
        vertices.append(m.vertices)
        triangles.append((m.triangles.astype(np.int64) + nv).astype(np.uint32))
        nv += len(m.vertices)
        top = z0 + n
    assert not decode(vol[top:])[1].any()
    out = Mesh()
    out.vertices, out.triangles = np.concatenate(vertices), np.concatenate(triangles)
    return out
