"""dfusion_render_mesh / frontend.renderMesh (dynamicfusion_amd/csrc/dfusion_render.hip) against the numpy restatement of the rule,
tests/render_ref.py: the point, normal, attribute and colour images, the triangle image and the counts, bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import render_ref as RR
from dynamicfusion_amd import Intr, capi, frontend, synth

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID = 100001
KEYS = ("points", "normals", "attr", "colors", "tri")
UNIT = (1.0, 1.0, 0.0, 0.0)                      # u = x / z, v = y / z: a vertex at z = 1 projects to its own (x, y)
GUARD = 2                                        # guard rows above and below a pitched output


def dressed(v, seed=5):
    """Random per-vertex normals, attribute and colours for the vertices v [V, 4]."""
    rng = np.random.RandomState(seed)
    n = rng.standard_normal((len(v), 4)).astype(F32)
    a = rng.uniform(-2, 2, (len(v), 4)).astype(F32)
    c = rng.randint(0, 256, (len(v), 4)).astype(np.uint8)
    return n, a, c


def _image(rows, cols, ch, dtype, pad):
    """-> (buffer, interior view): dense, or the interior of a wider and taller sentinel-filled buffer."""
    shape = (rows, cols) + ((ch,) if ch else ())
    if pad is None:
        t = torch.empty(shape, dtype=dtype, device="cuda")
        return t, t
    x0, extra = pad
    buf = torch.full((rows + 2 * GUARD, x0 + cols + extra) + ((ch,) if ch else ()), 0x55, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + rows, x0:x0 + cols]


def _pitch(view):
    return view.stride(0) * view.element_size()


def gpu_render(v, t, cols, rows, intr, w2c=None, nrm=None, att=None, col=None, ext=16, pad=None, outputs=KEYS, counts=True):
    """One dfusion_render_mesh call on numpy inputs -> dict of numpy outputs (bits), as render_ref.render names them."""
    dev = lambda a, dt: None if a is None or not len(a) else torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    tv = dev(v, F32)
    tt = dev(None if t is None else np.asarray(t, np.uint32).view(np.int32), np.int32)
    tn, ta, tc = dev(nrm, F32), dev(att, F32), dev(col, np.uint8)
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    want_out = {"points": True, "normals": nrm is not None and "normals" in outputs, "attr": att is not None and "attr" in outputs,
                "colors": col is not None and "colors" in outputs, "tri": "tri" in outputs}
    spec = {"points": (4, torch.float32), "normals": (4, torch.float32), "attr": (4, torch.float32), "colors": (4, torch.uint8), "tri": (0, torch.int32)}
    bufs, views = {}, {}
    for i, k in enumerate(KEYS):
        if want_out[k]:
            bufs[k], views[k] = _image(rows, cols, spec[k][0], spec[k][1], None if pad is None else (pad[0] + i, pad[1] + 2 * i))
    cnt = torch.full((6,), -7, dtype=torch.int64, device="cuda") if counts else None
    arg = lambda k: (ptr(views.get(k)), _pitch(views[k]) if k in views else 0)
    rc = capi.lib().dfusion_render_mesh(
        ptr(tv), len(v), ptr(tt), 0 if t is None else len(t), None if w2c is None else capi.floats(w2c), ptr(tn), ptr(ta), ptr(tc), cols, rows,
        capi.floats(intr), int(ext), *arg("points"), *arg("normals"), *arg("attr"), *arg("colors"), *arg("tri"), ptr(cnt),
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    capi.check(rc, "dfusion_render_mesh")
    torch.cuda.synchronize()
    out = {}
    for k in KEYS:
        if k in views:
            a = views[k].cpu().numpy()
            out[k] = np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a
            if pad is not None:                                          # nothing outside the image changed
                views[k].fill_(0x55)
                assert bool((bufs[k] == 0x55).all()), k
        else:
            out[k] = None
    out["counts"] = cnt.cpu().numpy().astype(np.uint64) if counts else None
    return out


def check(v, t, cols, rows, intr, w2c=None, nrm=None, att=None, col=None, ext=16, **kw):
    want = RR.render(v, t, cols, rows, intr, world2cam=w2c, normals=nrm, attr=att, colors=col, max_extent=ext)
    got = gpu_render(v, t, cols, rows, intr, w2c, nrm, att, col, ext, **kw)
    for k in KEYS + ("counts",):
        if got[k] is not None:
            assert want[k] is not None and np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))
    return want


# ------------------------------------------------------------------------------------------------ hand-made triangles, 8 x 6
def V(*rows):
    return np.array([list(r) + [0.0] * (4 - len(r)) for r in rows], F32)


BELOW = float(np.nextafter(F32(65536), F32(0)))
DENORM = float(np.float32(1e-41))
HAND = {
    # name: (vertices, triangles, expected statuses at max_extent 4 or None, expected covered pixels or None)
    "vertex-on-sample-and-edges-through-samples": (V((2, 1, 1), (5, 1, 1), (2, 4, 1)), [(0, 1, 2)], [0], 10),
    "clockwise": (V((2, 1, 1), (5, 1, 1), (2, 4, 1)), [(0, 2, 1)], [0], 10),
    "shared-edge-coplanar-equal-z": (V((2, 1, 1), (5, 1, 1), (2, 4, 1), (5, 4, 1)), [(1, 3, 2), (0, 1, 2)], [0, 0], 16),
    "overlap-near-first": (V((1, 1, 1), (6, 1, 1), (1, 5, 1), (2, 2, 2), (14, 2, 2), (2, 12, 2)), [(0, 1, 2), (3, 4, 5)], [3, 3], None),
    "overlap-near-last": (V((1, 1, 1), (6, 1, 1), (1, 5, 1), (2, 2, 2), (14, 2, 2), (2, 12, 2)), [(3, 4, 5), (0, 1, 2)], [3, 3], None),
    "collinear-and-repeated": (V((1, 1, 1), (3, 3, 1), (5, 5, 1)), [(0, 1, 2), (0, 0, 1), (2, 2, 2)], [2, 2, 2], 0),
    "extent-exactly-4-and-one-unit-more": (V((1, 1, 1), (5, 1, 1), (1, 5, 1), (5.0625, 1, 1), (1, 5.0625, 1)),
                                           [(0, 1, 2), (0, 3, 2), (0, 1, 4)], [0, 3, 3], 15),
    "box-partly-negative": (V((-1.5, -1.2, 1), (2.3, -0.5, 1), (0.2, 2.7, 1), (-0.99, -0.99, 1), (-0.1, -0.99, 1), (-0.99, -0.1, 1)),
                            [(0, 1, 2), (3, 4, 5)], [0, 4], None),
    "box-wholly-outside": (V((-5, -5, 1), (-3, -5, 1), (-4, -3, 1), (8, 1, 1), (10, 1, 1), (9, 3, 1), (1, 6, 1), (3, 6, 1), (2, 8, 1), (7, 5, 1), (7.5, 5.5, 1), (8, 5, 1)),
                           [(0, 1, 2), (3, 4, 5), (6, 7, 8), (9, 10, 11)], [4, 4, 4, 0], 1),
    "u-just-below-and-at-65536": (V((1, 1, 1), (2, 1, 1), (BELOW, 1, 1), (65536, 1, 1), (1, -BELOW, 1), (1, -65536, 1), (1, 2, 1)),
                                  [(0, 6, 2), (0, 1, 3), (0, 1, 4), (0, 1, 5)], [3, 1, 3, 1], 0),
    "z-zero-negative-denormal": (V((1, 1, 1), (4, 1, 1), (1, 4, 1), (0, 0, 0.0), (0, 0, -0.0), (1, 1, -1), (0, 0, DENORM), (3, 3, DENORM)),
                                 [(0, 1, 3), (0, 1, 4), (0, 1, 5), (1, 2, 6), (0, 1, 7), (0, 1, 2)], [1, 1, 1, 0, 1, 0], None),
    "nan-and-inf": (np.concatenate([V((1, 1, 1), (4, 1, 1), (1, 4, 1))] +
                                   [V(tuple(bad if c == i else 1.0 for c in range(3))) for i in range(3) for bad in (np.nan, np.inf, -np.inf)]),
                    [(0, 1, 3 + j) for j in range(9)] + [(0, 1, 2)], [1] * 9 + [0], 10),
    "index-V-and-ffffffff": (V((2, 1, 1), (5, 1, 1), (2, 4, 1)), [(0, 1, 3), (0xffffffff, 1, 2), (0, 0xffffffff, 0xffffffff), (0, 1, 2)], [1, 1, 1, 0], 10),
    "larger-than-the-image": (V((-10, -10, 1), (50, -10, 1), (-10, 50, 1)), [(0, 1, 2)], [3], 0),
}


@pytest.mark.parametrize("ext", [1, 4, 16, 64])
@pytest.mark.parametrize("name", sorted(HAND))
def test_handmade_triangles(name, ext):
    v, t, statuses, covered = HAND[name]
    t = np.array(t, np.uint32)
    n, a, c = dressed(v)
    want = check(v, t, 8, 6, UNIT, nrm=n, att=a, col=c, ext=ext)
    if ext == 4:
        if statuses is not None:
            assert want["status"].tolist() == statuses
        if covered is not None:
            assert int(want["counts"][5]) == covered
    if name == "larger-than-the-image" and ext == 64:
        assert want["status"].tolist() == [0] and int(want["counts"][5]) == 48
    if name == "shared-edge-coplanar-equal-z":
        diag = [(y, x) for y, x in ((1, 5), (2, 4), (3, 3), (4, 2))]
        if ext >= 4:
            assert all(want["tri"][p] == 0 for p in diag)                # both cover the shared edge at equal z: the lower index wins
    if name.startswith("overlap") and ext >= 16:
        near = 0 if name.endswith("first") else 1
        assert want["tri"][2, 2] == near and (want["tri"] == 1 - near).sum() > 3


def test_handmade_triangles_in_one_mesh():
    vs, ts, off = [], [], 0
    for name in sorted(HAND):
        v, t = HAND[name][0], np.array(HAND[name][1], np.int64)
        ts.append(np.where(t >= len(v), np.where(t == len(v), -1, t), t + off))      # (the out-of-range indices stay out of range)
        vs.append(v)
        off += len(v)
    v, t = np.concatenate(vs), np.concatenate(ts)
    t[t == -1] = len(v)
    n, a, c = dressed(v)
    for ext in (4, 64):
        want = check(v, t.astype(np.uint32), 8, 6, UNIT, nrm=n, att=a, col=c, ext=ext)
        assert set(np.unique(want["status"])) == {0, 1, 2, 3, 4}


# ------------------------------------------------------------------------------------------------ random sets
def random_triangles(n, cols, rows, seed, size=3.0, bad=0.02):
    """n triangles of about `size` pixels around random centres from 4 pixels outside the image inwards, at depths 0.5-3 m, in camera space for
    the returned intrinsics; a share `bad` of the vertices is broken (NaN, behind, far off) and of the indices out of range."""
    rng = np.random.RandomState(seed)
    intr = (37.5, 36.25, cols / 2 - 0.37, rows / 2 + 0.21)
    c = np.stack([rng.uniform(-4, cols + 4, n), rng.uniform(-4, rows + 4, n)], 1)
    p = c[:, None] + rng.uniform(-size, size, (n, 3, 2)) * rng.choice([0.1, 1.0, 2.5], (n, 1, 1))
    snap = rng.random_sample(n) < 0.15                                   # vertices on sample points: ties, edges through samples, area 0
    p[snap] = np.rint(p[snap])
    z = rng.choice([0.5, 1.0, 1.5, 2.0, 3.0], (n, 1)) + rng.uniform(-0.2, 0.2, (n, 3)) * (rng.random_sample((n, 1)) < 0.7)
    v = np.zeros((n * 3, 4), F32)
    v[:, 0] = ((p[..., 0].ravel() - intr[2]) / intr[0] * z.ravel()).astype(F32)
    v[:, 1] = ((p[..., 1].ravel() - intr[3]) / intr[1] * z.ravel()).astype(F32)
    v[:, 2] = z.ravel().astype(F32)
    brk = rng.random_sample(n * 3) < bad
    v[brk, rng.randint(0, 3, brk.sum())] = rng.choice([np.nan, np.inf, -1.0, 0.0, 1e9], brk.sum()).astype(F32)
    t = np.arange(n * 3, dtype=np.int64).reshape(n, 3)
    share = rng.random_sample(n) < 0.3                                   # triangles that share vertices with their predecessor
    t[1:][share[1:], 0] = t[:-1][share[1:], 1]
    oob = rng.random_sample(n) < bad / 2
    t[oob, rng.randint(0, 3, oob.sum())] = rng.choice([n * 3, n * 3 + 1, 0xffffffff], oob.sum())
    return v, t.astype(np.uint32), intr


@pytest.mark.parametrize("n", [63, 64, 65])
def test_wave_boundaries(n):
    v, t, intr = random_triangles(n, 16, 12, seed=n, bad=0.0)
    z = 0.25                                                             # the last triangle is the nearest, over the middle of the image
    t[-1] = (3 * n - 3, 3 * n - 2, 3 * n - 1)
    for i, (px, py) in enumerate(((5.0, 3.0), (11.0, 4.0), (7.0, 9.0))):
        v[3 * n - 3 + i, :3] = ((px - intr[2]) / intr[0] * z, (py - intr[3]) / intr[1] * z, z)
    nr, a, c = dressed(v)
    want = check(v, t, 16, 12, intr, nrm=nr, att=a, col=c, ext=16)
    assert want["counts"][0] > n // 3 and want["counts"][5] > 20 and (want["tri"] == n - 1).sum() > 10


def test_100000_random_triangles_reach_every_status():
    v, t, intr = random_triangles(100000, 64, 48, seed=11, size=1.2)
    nr, a, c = dressed(v)
    want = check(v, t, 64, 48, intr, nrm=nr, att=a, col=c, ext=4)
    cnt = want["counts"]
    assert all(cnt[s] > 100 for s in range(5)) and int(cnt[:5].sum()) == 100000 and cnt[5] == 64 * 48
    # and many triangles pile on a pixel: the drawn ones cover some 40 times the image
    assert cnt[0] > 20000


def test_4096_triangles_over_one_pixel():
    rng = np.random.RandomState(3)
    n = 4096
    z = rng.choice([0.75, 1.0, 1.0, 1.25, 2.0], n)
    tie = rng.randint(0, n, 40)
    z[tie] = 0.5                                                         # 40 copies of the nearest triangle: the lowest index wins
    p = np.array([[2.5, 1.5], [4.5, 2.5], [2.5, 3.5]])[None] + rng.uniform(-0.1, 0.1, (n, 3, 2))
    p[tie] = p[tie[0]]
    v = np.zeros((n * 3, 4), F32)
    v[:, 0] = (p[..., 0] * z[:, None]).ravel(); v[:, 1] = (p[..., 1] * z[:, None]).ravel(); v[:, 2] = np.repeat(z, 3)
    t = np.arange(n * 3, dtype=np.uint32).reshape(n, 3)
    nr, a, c = dressed(v)
    want = check(v, t, 8, 6, UNIT, nrm=nr, att=a, col=c, ext=4)
    assert want["tri"][2, 3] == tie.min() and want["counts"][0] == n and want["counts"][5] >= 2


# ------------------------------------------------------------------------------------------------ the sphere scenes of the rule test
@functools.lru_cache(None)
def sphere_scene():
    cfg = synth.Config(32, 1.0, cols=80, rows=60)
    v, t, n = RR.sphere_mesh(0.2, (0.0, 0.0, 1.0))
    v2, t2, n2 = RR.sphere_mesh(0.5, (0.0, 0.0, 1.8))
    return cfg, v, t, n, np.concatenate([v, v2]), np.concatenate([t, t2 + np.uint32(len(v))]), np.concatenate([n, n2])


@pytest.mark.parametrize("ext", [1, 16])
def test_sphere_scenes(ext):
    cfg, v, t, n, vv, tt, nn = sphere_scene()
    col = dressed(vv)[2]
    one = check(v, t, cfg.cols, cfg.rows, cfg.intr, nrm=n, att=v, col=col[:len(v)], ext=ext)
    two = check(vv, tt, cfg.cols, cfg.rows, cfg.intr, nrm=nn, att=vv, col=col, ext=ext)
    assert one["counts"][5] > 600 and two["counts"][5] > one["counts"][5]
    # from a turned and shifted camera
    pose = synth.rot_y_about(np.deg2rad(9.0), (0.0, 0.0, 1.0)).astype(np.float64)
    pose[:3, 3] += (0.02, -0.03, 0.05)
    w2c = synth.aff12(np.linalg.inv(pose).astype(F32))
    turned = check(vv, tt, cfg.cols, cfg.rows, cfg.intr, w2c=w2c, nrm=nn, att=vv, col=col, ext=ext)
    assert turned["counts"][5] > 600 and not np.array_equal(turned["tri"], two["tri"])


# ------------------------------------------------------------------------------------------------ a fused scene's mesh, warped and coloured
def test_warped_coloured_mesh_of_a_fused_scene():
    import color_ref as CR
    from dynamicfusion_amd import ColorVolume, WarpField
    from test_gpu_color import dense, gpu_volume
    S = CR.scene(32, 80, 60, nodes=64, k=4)
    sc, intr = S.sc, Intr(*S.cfg.intr)
    vol = gpu_volume(S, 2)
    cv = ColorVolume(vol)
    for f in range(3):
        vol.upload(S.vols[f])
        cv.integrate(dense(S.images[f]), dense(sc.dists[f]), sc.cam_poses[f], intr)
    wf = WarpField(k=4, voxel_table=False, weight_table=False)
    wf.init(sc.pos, sigma=sc.sigma, transforms=sc.dqs[2])
    verts, tris, normals = vol.fetchMesh(with_normals=True)
    colors = cv.fetchColors(verts)
    p3, n3 = verts[:, :3].contiguous(), normals[:, :3].contiguous()
    wf.warp(p3, n3, 4)
    warped, wn = torch.zeros_like(verts), torch.zeros_like(normals)
    warped[:, :3] = p3; wn[:, :3] = n3
    w2c = sc.world2cam(2)
    got = frontend.renderMesh(intr, warped, tris, 80, 60, world2cam=w2c, normals=wn, attr=verts, colors=colors, return_tri=True, return_counts=True)
    want = RR.render(warped.cpu().numpy(), tris.cpu().numpy().view(np.uint32), 80, 60, S.cfg.intr, world2cam=synth.aff12(w2c),
                     normals=wn.cpu().numpy(), attr=verts.cpu().numpy(), colors=colors.cpu().numpy())
    for k, g in zip(KEYS, got[:5]):
        g = g.cpu().numpy()
        assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, want[k]), k
    assert np.array_equal(got[5].cpu().numpy().astype(np.uint64), want["counts"])
    hit = want["tri"] >= 0
    assert len(tris) > 1000 and hit.sum() > 500 and want["counts"][0] > 500
    assert len(np.unique(want["colors"][hit][:, :3], axis=0)) > 3         # the checker paint, interpolated
    # the attribute is the canonical point under the pixel: where the warp moves it, point and attribute differ
    assert not np.array_equal(want["attr"][hit], want["points"][hit])


# ------------------------------------------------------------------------------------------------ the call's edges
def small_set():
    v, t, intr = random_triangles(3000, 40, 30, seed=29)
    return (v, t, intr) + dressed(v)


def test_each_optional_output_absent():
    v, t, intr, n, a, c = small_set()
    for outputs in (("points",), ("points", "normals"), ("points", "attr"), ("points", "colors"), ("points", "tri"), ("points", "attr", "colors", "tri")):
        check(v, t, 40, 30, intr, nrm=n, att=a, col=c, ext=8, outputs=outputs)
    check(v, t, 40, 30, intr, nrm=n, att=a, col=c, ext=8, counts=False)
    check(v, t, 40, 30, intr, ext=8)                                     # no per-vertex input at all
    check(v, t, 40, 30, intr, nrm=n, ext=8, outputs=("points", "normals", "tri"))


@pytest.mark.parametrize("pad", [(1, 3), (4, 0), (0, 5)])
def test_pitched_and_offset_outputs_keep_their_guards(pad):
    v, t, intr, n, a, c = small_set()
    check(v, t, 40, 30, intr, nrm=n, att=a, col=c, ext=8, pad=pad)
    check(v, t, 1, 1, intr, nrm=n, att=a, col=c, ext=8, pad=pad)


def test_empty_meshes_are_all_misses():
    v, t, intr, n, a, c = small_set()
    for vv, tt in ((v[:0], t[:0]), (v, t[:0]), (v[:0], t)):
        got = gpu_render(vv, tt, 40, 30, intr, None, n[:len(vv)], a[:len(vv)], c[:len(vv)], 8, outputs=("points", "tri"))
        assert (got["points"] == 0x7fffffff).all() and (got["tri"] == -1).all() and got["counts"].tolist() == [0] * 6
        want = RR.render(vv, tt, 40, 30, intr, max_extent=8)
        assert np.array_equal(want["points"], got["points"]) and want["counts"].tolist() == [0] * 6
    e4 = torch.empty((0, 4), dtype=torch.float32, device="cuda")
    out = frontend.renderMesh(Intr(*intr), e4, torch.empty((0, 3), dtype=torch.int32, device="cuda"), 40, 30, normals=e4, attr=e4,
                              colors=torch.empty((0, 4), dtype=torch.uint8, device="cuda"), return_tri=True, return_counts=True)
    assert all((o[..., :].cpu().numpy().view(np.uint32) == 0x7fffffff).all() for o in out[:3])
    assert (out[3] == 0).all() and (out[4] == -1).all() and out[5].tolist() == [0] * 6


def test_repeats_sizes_streams_and_released_scratch():
    v, t, intr, n, a, c = small_set()
    bv, bt, bintr = random_triangles(20000, 320, 240, seed=31, size=6.0)
    first = check(v, t, 40, 30, intr, nrm=n, att=a, col=c, ext=8)
    again = check(v, t, 40, 30, intr, nrm=n, att=a, col=c, ext=8)     # the same call twice
    assert np.array_equal(first["keys"], again["keys"])
    check(bv, bt, 320, 240, bintr, ext=16)                               # a large image, then a small one in the same scratch
    check(v, t, 40, 30, intr, nrm=n, att=a, col=c, ext=8)
    check(v, t, 7, 5, intr, ext=8)
    with torch.cuda.stream(torch.cuda.Stream()):
        check(v, t, 40, 30, intr, nrm=n, att=a, col=c, ext=8)
        check(bv, bt, 320, 240, bintr, ext=16)
    assert capi.lib().dfusion_release_scratch() == 0
    check(v, t, 40, 30, intr, nrm=n, att=a, col=c, ext=8)


def test_frontend_mirror_equals_the_restatement():
    v, t, intr, n, a, c = small_set()
    dev = lambda x: torch.from_numpy(x).cuda()
    got = frontend.renderMesh(Intr(*intr), dev(v), dev(t.view(np.int32)), 40, 30, normals=dev(n), attr=dev(a), colors=dev(c), return_tri=True,
                              return_counts=True)
    want = RR.render(v, t, 40, 30, intr, normals=n, attr=a, colors=c)      # (default max_extent 16 on both sides)
    for k, g in zip(KEYS, got[:5]):
        g = g.cpu().numpy()
        assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, want[k]), k
    assert got[5].tolist() == [int(x) for x in want["counts"]]
    pts, no_n, no_a, no_c = frontend.renderMesh(Intr(*intr), dev(v), dev(t.view(np.int32)), 40, 30)
    assert no_n is None and no_a is None and no_c is None and np.array_equal(pts.cpu().numpy().view(np.uint32), want["points"])
    with pytest.raises(ValueError):
        frontend.renderMesh(Intr(*intr), dev(v)[:, :3], dev(t.view(np.int32)), 40, 30)
    with pytest.raises(ValueError):
        frontend.renderMesh(Intr(*intr), dev(v), dev(t.view(np.int32)), 40, 30, normals=dev(n)[:-1])


def test_every_argument_check():
    L = capi.lib()
    v, t, intr, n, a, c = small_set()
    tv, tt = torch.from_numpy(v).cuda(), torch.from_numpy(t.view(np.int32)).cuda()
    tn, tc = torch.from_numpy(n).cuda(), torch.from_numpy(c).cuda()
    img = torch.empty((30, 40, 4), dtype=torch.float32, device="cuda")
    img8 = torch.empty((30, 40, 4), dtype=torch.uint8, device="cuda")
    P = lambda x: C.c_void_p(x.data_ptr())
    good = dict(v=P(tv), V=len(v), t=P(tt), T=len(t), w2c=None, n=P(tn), a=P(tn), c=P(tc), cols=40, rows=30, intr=capi.floats(intr), ext=16,
                po=P(img), pp=640, no=None, np_=0, ao=None, ap=0, co=None, cp=0, to=None, tp=0, cnt=None)

    def call(**kw):
        g = dict(good, **kw)
        return L.dfusion_render_mesh(g["v"], g["V"], g["t"], g["T"], g["w2c"], g["n"], g["a"], g["c"], g["cols"], g["rows"], g["intr"], g["ext"],
                                     g["po"], g["pp"], g["no"], g["np_"], g["ao"], g["ap"], g["co"], g["cp"], g["to"], g["tp"], g["cnt"], None)

    assert call() == 0
    assert call(v=None) == INVALID and call(t=None) == INVALID
    assert call(v=None, V=0) == 0 and call(t=None, T=0) == 0
    assert call(intr=None) == INVALID and call(po=None) == INVALID
    assert call(cols=0) == INVALID and call(rows=0) == INVALID and call(cols=-1) == INVALID
    assert call(pp=639) == INVALID and call(pp=624) == INVALID           # shorter than a row
    assert call(pp=648) == INVALID                                       # long enough, not a multiple of 16
    assert call(po=C.c_void_p(img.data_ptr() + 4)) == INVALID            # a misaligned base
    assert call(no=P(img), np_=639) == INVALID and call(ao=P(img), ap=632) == INVALID
    assert call(co=P(img8), cp=159) == INVALID and call(co=P(img8), cp=162) == INVALID and call(to=P(img8), tp=158) == INVALID
    assert call(ext=0) == INVALID and call(ext=65) == INVALID and call(ext=-3) == INVALID and call(ext=1) == 0 and call(ext=64) == 0
    assert call(V=1 << 32) == INVALID and call(T=1 << 32) == INVALID
    for i in range(4):
        for bad in (np.nan, np.inf, -np.inf):
            assert call(intr=capi.floats([bad if j == i else x for j, x in enumerate(intr)])) == INVALID
    assert call(intr=capi.floats((0.0,) + tuple(intr[1:]))) == INVALID and call(intr=capi.floats((intr[0], -0.0) + tuple(intr[2:]))) == INVALID
    assert call(no=P(img), np_=640, n=None) == INVALID and call(ao=P(img), ap=640, a=None) == INVALID and call(co=P(img8), cp=160, c=None) == INVALID
    assert call(no=P(img), np_=640) == 0 and call(co=P(img8), cp=160) == 0
    torch.cuda.synchronize()
