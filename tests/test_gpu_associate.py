"""dfusion_associate_projective against its numpy restatement (tests/associate_ref.py), bit for bit: live_out, status and counts.
Scenes and hand-made sets that reach every status and every boundary of the rule, then the call forms (tiny N, NULL normals, NULL
status / counts, pitched and offset live images, repeated calls, stale scratch, a fresh stream) and every argument check."""
import ctypes as C

import numpy as np
import pytest
import torch

import associate_ref as AR
from dynamicfusion_amd import Intr, capi, frontend
from test_gpu_pitched_images import padded

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID = 100001
GUARD = 7                     # elements in front of and behind every output, which must keep their sentinel


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_associate(points, normals, lp, ln, intr, dist, mc, margin, want_status=True, want_counts=True, lp_t=None, ln_t=None):
    """One call through the C-ABI with guarded outputs.  Returns (live bits [N, 3], status or None, counts or None)."""
    n = len(points)
    rows, cols = lp.shape[:2]
    lp_t = _dev(lp) if lp_t is None else lp_t
    ln_t = (_dev(ln) if ln is not None else None) if ln_t is None else ln_t
    room = lambda a: np.concatenate([np.asarray(a, F32).reshape(-1, 3), np.zeros((1, 3), F32)])     # (never a NULL pointer, also for N = 0)
    p_t = _dev(room(points))
    n_t = _dev(room(normals)) if normals is not None else None
    live = torch.full((n + 2 * GUARD, 3), 12345.0, dtype=torch.float32, device="cuda")
    st = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    cnt = torch.full((8 + 2 * GUARD,), -77, dtype=torch.int64, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    lpp, lpitch, r, c = frontend._image(lp_t, frontend.F4)
    assert (r, c) == (rows, cols)
    lnp, lnpitch = frontend._sized(ln_t, frontend.F4, rows, cols) if ln_t is not None else (None, 0)
    rc = capi.lib().dfusion_associate_projective(
        ptr(p_t), ptr(n_t), n, lpp, lpitch, lnp, lnpitch, cols, rows, capi.floats(intr), float(dist), float(mc), float(margin),
        C.c_void_p(live[GUARD:].data_ptr()), C.c_void_p(st[GUARD:].data_ptr()) if want_status else None,
        C.c_void_p(cnt[GUARD:].data_ptr()) if want_counts else None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    live_h, st_h, cnt_h = live.cpu().numpy(), st.cpu().numpy(), cnt.cpu().numpy()
    assert (live_h[:GUARD] == 12345.0).all() and (live_h[GUARD + n:] == 12345.0).all(), "live_out written out of bounds"
    assert (st_h[:GUARD] == 0xA5).all() and (st_h[GUARD + n:] == 0xA5).all(), "status written out of bounds"
    assert (cnt_h[:GUARD] == -77).all() and (cnt_h[GUARD + 8:] == -77).all(), "counts written out of bounds"
    if not want_status:
        assert (st_h == 0xA5).all()
    if not want_counts:
        assert (cnt_h == -77).all()
    return (live_h[GUARD:GUARD + n].view(np.uint32), st_h[GUARD:GUARD + n] if want_status else None,
            cnt_h[GUARD:GUARD + 8] if want_counts else None)


def check(points, normals, lp, ln, intr, dist, mc, margin, **kw):
    """GPU == restatement on all three outputs; returns the restatement's (status, counts)."""
    want_live, want_st, want_cnt = AR.associate(points, normals, lp, ln, intr, dist, mc, margin)
    live, st, cnt = gpu_associate(points, normals, lp, ln, intr, dist, mc, margin, **kw)
    bad = int((live != want_live.view(np.uint32)).any(1).sum())
    assert bad == 0, "%d of %d live_out rows differ" % (bad, len(want_st))
    if st is not None:
        assert np.array_equal(st, want_st), "%d statuses differ" % int((st != want_st).sum())
    if cnt is not None:
        assert np.array_equal(cnt.astype(np.uint64), want_cnt), (cnt.tolist(), want_cnt.tolist())
        assert int(cnt.sum()) == len(want_st)
    return want_st, want_cnt


# ------------------------------------------------------------------------------------------------------------------ scenes
@pytest.mark.parametrize("t0", [(0.03, 0.0, 0.0), (0.0, 0.0, 0.0), (-0.02, 0.015, 0.01)])
@pytest.mark.parametrize("margin", [-1.0, 0.02])
def test_planted_sphere(t0, margin):
    s = AR.planted(t0)
    st, cnt = check(s["points"], s["normals"], s["live_points"], s["live_normals"], AR.INTR, AR.DIST_THRES, AR.MIN_COSINE, margin)
    assert len(st) == 19200 and cnt[0] > 2000 and cnt[1] > 10000


# The hand-made sets live on an 8 x 6 image with fx = fy = 4, cx = cy = 0: a point (x, y, z) falls on u = 4 x / z, v = 4 y / z, so
# quarters at z = 1 hit pixel corners exactly.  The live sample of pixel (ui, vi) is ((ui + 0.5) / 4, (vi + 0.5) / 4, 1) unless a test
# plants another one; the live normal is (0, 0, 1).
HC, HR, HINTR = 8, 6, (4.0, 4.0, 0.0, 0.0)


def hand_maps():
    u, v = np.meshgrid(np.arange(HC, dtype=F32), np.arange(HR, dtype=F32))
    lp = np.zeros((HR, HC, 4), F32); ln = np.zeros((HR, HC, 4), F32)
    lp[..., 0] = (u + F32(0.5)) / F32(4); lp[..., 1] = (v + F32(0.5)) / F32(4); lp[..., 2] = 1
    ln[..., 2] = 1
    return lp, ln


def up(x):
    return np.nextafter(F32(x), F32(np.inf))


def test_hand_made_projection_bounds_and_invalid_inputs():
    lp, ln = hand_maps()
    nan, inf = F32(np.nan), F32(np.inf)
    pts = [(0, 0, 1), (-0.0, -0.0, 1), (2, 0, 1), (np.nextafter(F32(2), F32(0)), 0, 1), (0, 1.5, 1), (0, np.nextafter(F32(1.5), F32(0)), 1),
           (-1e-3, 0, 1), (0, -1e-3, 1), (0.25, 0.25, 0.0), (0.25, 0.25, -0.0), (0.25, 0.25, -1.0), (0.25, 0.25, 1e-42), (1e-42, 0, 1e-42)]
    want = [0, 0, 3, 0, 3, 0, 3, 3, 2, 2, 2, 3, 0]
    for c in range(3):
        for bad in (nan, inf, -inf):
            p = [0.25, 0.25, 1.0]; p[c] = bad
            pts.append(tuple(p)); want.append(1)
    pts = np.array(pts, F32)
    st, cnt = check(pts, None, lp, None, HINTR, 10.0, 0.5, -1.0)
    assert st.tolist() == want
    # with normals: a bad normal is status 1 whatever the point is (behind and outside included); a good one changes nothing
    nrm = np.tile(np.array([0, 0, 1], F32), (len(pts), 1))
    st2, _ = check(pts, nrm, lp, ln, HINTR, 10.0, 0.5, -1.0)
    assert st2.tolist() == want
    pp, nn = [], []
    for base in ((0.25, 0.25, 1.0), (0.25, 0.25, -1.0), (2, 0, 1)):
        for c in range(3):
            for bad in (nan, inf, -inf):
                n = [0.0, 0.0, 1.0]; n[c] = bad
                pp.append(base); nn.append(tuple(n))
    st3, cnt3 = check(np.array(pp, F32), np.array(nn, F32), lp, ln, HINTR, 10.0, 0.5, -1.0)
    assert (st3 == 1).all() and cnt3[1] == len(pp)


def test_hand_made_hole_distance_and_normal_thresholds():
    lp, ln = hand_maps()
    # pixel (1, 1): d = (-0.125, 0, 0), d^2 == dist_thres^2 exactly -> kept; pixel (2, 1): one ulp farther -> far; pixel (3, 1): a hole
    lp[1, 1, :3] = (0.375, 0.25, 1); lp[1, 2, :3] = (up(0.625), 0.25, 1); lp[1, 3, :3] = np.nan
    lp[1, 4, :3] = (0.125, np.nan, 1)                          # only q.x decides the hole: NaN elsewhere is a NaN distance, which is kept
    pts = np.array([(0.25, 0.25, 1), (0.5, 0.25, 1), (0.75, 0.25, 1), (1.0, 0.25, 1)], F32)
    st, _ = check(pts, None, lp, None, HINTR, 0.125, 0.5, -1.0)
    assert st.tolist() == [0, 6, 5, 0]
    # normals: |dot| == min_cosine kept (both signs), one ulp below rejected, a NaN live normal rejected
    lp, ln = hand_maps()
    ln[1, 1, :3] = (0, 0, 0.5); ln[1, 2, :3] = (0, 0, np.nextafter(F32(0.5), F32(0))); ln[1, 3, :3] = (np.nan, 0, 1); ln[1, 4, :3] = (0, 0, -0.5)
    ln[1, 5, :3] = (0, 0, np.nan)
    pts = np.array([(0.25 * i + 0.125, 0.375, 1) for i in range(1, 6)], F32)
    nrm = np.tile(np.array([0, 0, 1], F32), (len(pts), 1))
    st, _ = check(pts, nrm, lp, ln, HINTR, 10.0, 0.5, -1.0)
    assert st.tolist() == [0, 7, 7, 0, 7]


def test_hand_made_occlusion_margins():
    lp, ln = hand_maps()
    z1 = up(1.25)
    a, b, c = F32(0.3125), F32(0.5625), F32(0.8125)                                # u = 1.25, 2.25, 3.25 (v = 1.25) at any depth
    pts = np.array([(a, a, 1), (a * F32(1.25), a * F32(1.25), 1.25),               # pixel (1, 1): exactly the margin behind -> kept
                    (b, a, 1), (b * z1, a * z1, z1),                               # pixel (2, 1): one ulp more -> occluded
                    (c, a, 1), (c, a, 1), (c * up(1), a * up(1), up(1))], F32)     # pixel (3, 1): a tie, and one ulp behind it
    st, _ = check(pts, None, lp, None, HINTR, 10.0, 0.5, 0.25)
    assert st.tolist() == [0, 0, 0, 4, 0, 0, 0]
    st, _ = check(pts, None, lp, None, HINTR, 10.0, 0.5, 0.0)                      # margin 0 keeps the exact tie only
    assert st.tolist() == [0, 4, 0, 4, 0, 0, 4]
    st, cnt = check(pts, None, lp, None, HINTR, 10.0, 0.5, -0.5)                   # a negative margin: the test is off
    assert st.tolist() == [0] * 7 and cnt[4] == 0
    # points that fail tests 1-3 never occlude: a NaN-normal point in front of a good one
    nrm = np.tile(np.array([0, 0, 1], F32), (2, 1)); nrm[0, 0] = np.nan
    st, _ = check(np.array([(0.15625, 0.15625, 0.5), (0.3125, 0.3125, 1)], F32), nrm, lp, ln, HINTR, 10.0, 0.5, 0.25)
    assert st.tolist() == [1, 0]


def test_4096_points_on_one_pixel():
    rng = np.random.RandomState(3)
    lp, ln = hand_maps()
    z = rng.uniform(0.8, 1.2, 4096).astype(F32)
    pts = np.stack([F32(0.3125) * z, F32(0.3125) * z, z], 1).astype(F32)
    nrm = np.tile(np.array([0, 0, 1], F32), (4096, 1))
    st, cnt = check(pts, nrm, lp, ln, HINTR, 10.0, 0.5, 0.01)
    assert cnt[0] + cnt[4] == 4096 and cnt[0] > 50 and cnt[4] > 3000
    check(pts, nrm, lp, ln, HINTR, 10.0, 0.5, 0.0)


def random_set(n, seed=11):
    """Random points over a 64 x 48 image, some outside it, behind the camera or not finite; live maps with holes and NaN normals."""
    rng = np.random.RandomState(seed)
    cols, rows, intr = 64, 48, (50.0, 50.0, 31.5, 23.5)
    u, v = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    z = 1.0 + 0.2 * np.sin(u / 9.0) * np.cos(v / 7.0)
    lp = np.zeros((rows, cols, 4), F32); ln = np.zeros((rows, cols, 4), F32)
    lp[..., 0] = (u - intr[2]) / intr[0] * z; lp[..., 1] = (v - intr[3]) / intr[1] * z; lp[..., 2] = z
    nl = rng.normal(size=(rows, cols, 3)) * 0.4 + np.array([0, 0, -1.0])
    ln[..., :3] = nl / np.linalg.norm(nl, axis=-1, keepdims=True)
    holes = rng.uniform(size=(rows, cols)) < 0.05
    lp[holes] = np.nan; ln[holes] = np.nan
    ln[rng.uniform(size=(rows, cols)) < 0.01, 0] = np.nan
    pu, pv = rng.uniform(-4, cols + 4, n), rng.uniform(-4, rows + 4, n)
    pz = 1.0 + 0.2 * np.sin(pu / 9.0) * np.cos(pv / 7.0) + rng.normal(size=n) * 0.08
    pz[rng.uniform(size=n) < 0.01] *= -1
    pts = np.stack([(pu - intr[2]) / intr[0] * pz, (pv - intr[3]) / intr[1] * pz, pz], 1).astype(F32)
    pn = rng.normal(size=(n, 3)) * 0.4 + np.array([0, 0, -1.0])
    nrm = (pn / np.linalg.norm(pn, axis=-1, keepdims=True)).astype(F32)
    pts[rng.uniform(size=n) < 0.005, rng.randint(0, 3)] = np.nan
    nrm[rng.uniform(size=n) < 0.005, rng.randint(0, 3)] = np.inf
    return pts, nrm, lp, ln, intr


def test_100000_random_points_reach_every_status():
    pts, nrm, lp, ln, intr = random_set(100000)
    st, cnt = check(pts, nrm, lp, ln, intr, 0.15, 0.6, 0.05)
    assert (cnt > 0).all(), cnt.tolist()


def test_more_points_than_one_walk_of_the_resolve_grid():
    """The resolve kernel runs at most 512 workgroups of 256 lanes: beyond 131 072 points a workgroup walks more than one chunk and
    carries its status counts along (one more than a whole number of chunks, and a wave's worth more)."""
    pts, nrm, lp, ln, intr = random_set(131072 + 65, seed=29)
    for n in (131072, 131073, 131072 + 65):
        st, cnt = check(pts[:n], nrm[:n], lp, ln, intr, 0.15, 0.6, 0.05)
    assert (cnt > 0).all()


# ------------------------------------------------------------------------------------------------------------------ call forms
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_point_counts(n):
    pts, nrm, lp, ln, intr = random_set(400, seed=5)
    check(pts[:n], nrm[:n], lp, ln, intr, 0.15, 0.6, 0.05)
    check(pts[:n], nrm[:n], lp, ln, intr, 0.15, 0.6, -1.0)


def test_no_points():
    pts, nrm, lp, ln, intr = random_set(8, seed=5)
    live, st, cnt = gpu_associate(pts[:0], nrm[:0], lp, ln, intr, 0.15, 0.6, 0.05)
    assert live.shape == (0, 3) and cnt.tolist() == [0] * 8
    for nr, l in ((None, None), (_dev(nrm[:0]), _dev(ln))):
        out = frontend.associateProjective(Intr(*intr), _dev(pts[:0]), nr, _dev(lp), l, 0.15, 0.6, return_counts=True)
        assert out[0].shape == (0, 3) and out[1].cpu().tolist() == [0] * 8


def test_without_normals_and_without_status_or_counts():
    pts, nrm, lp, ln, intr = random_set(5000, seed=7)
    st, cnt = check(pts, None, lp, None, intr, 0.15, 0.6, 0.05)
    assert cnt[7] == 0 and cnt[6] > 0
    for ws, wc in ((False, True), (True, False), (False, False)):
        check(pts, nrm, lp, ln, intr, 0.15, 0.6, 0.05, want_status=ws, want_counts=wc)


def test_python_wrapper_returns_what_was_asked_for():
    pts, nrm, lp, ln, intr = random_set(3000, seed=9)
    want_live, want_st, want_cnt = AR.associate(pts, nrm, lp, ln, intr, 0.15, 0.6, 0.05)
    I = Intr(*intr)
    args = (I, _dev(pts), _dev(nrm), _dev(lp), _dev(ln), 0.15, 0.6, 0.05)
    live = frontend.associateProjective(*args)
    assert isinstance(live, torch.Tensor) and np.array_equal(live.cpu().numpy().view(np.uint32), want_live.view(np.uint32))
    live, st = frontend.associateProjective(*args, return_status=True)
    assert np.array_equal(st.cpu().numpy(), want_st)
    live, cnt = frontend.associateProjective(*args, return_counts=True)
    assert np.array_equal(cnt.cpu().numpy().astype(np.uint64), want_cnt)
    live, st, cnt = frontend.associateProjective(*args, return_status=True, return_counts=True)
    assert np.array_equal(st.cpu().numpy(), want_st) and np.array_equal(cnt.cpu().numpy().astype(np.uint64), want_cnt)
    off = frontend.associateProjective(I, _dev(pts), _dev(nrm), _dev(lp), _dev(ln), 0.15, 0.6)          # the default margin: test off
    assert np.array_equal(off.cpu().numpy().view(np.uint32), AR.associate(pts, nrm, lp, ln, intr, 0.15, 0.6, -1.0)[0].view(np.uint32))
    with pytest.raises(ValueError):
        frontend.associateProjective(I, _dev(pts), None, _dev(lp), _dev(ln), 0.15, 0.6)


def test_pitched_and_offset_live_images():
    pts, nrm, lp, ln, intr = random_set(20000, seed=13)
    a = padded(lp, "f4", 48, 3); b = padded(ln, "f4", 4096, 1)                     # different pitches and column offsets
    check(pts, nrm, lp, ln, intr, 0.15, 0.6, 0.05, lp_t=a.t, ln_t=b.t)
    assert a.padding_intact() and b.padding_intact()
    assert np.array_equal(a.np().view(np.uint32), lp.view(np.uint32)) and np.array_equal(b.np().view(np.uint32), ln.view(np.uint32))


def test_repeated_calls_stale_scratch_and_a_fresh_stream():
    pts, nrm, lp, ln, intr = random_set(30000, seed=17)
    check(pts, nrm, lp, ln, intr, 0.15, 0.6, 0.05)
    check(pts, nrm, lp, ln, intr, 0.15, 0.6, 0.05)                                 # the same call again on the same stream
    s = AR.planted((0.03, 0.0, 0.0))                                               # a larger image, then a small one: the scratch is stale
    check(s["points"], s["normals"], s["live_points"], s["live_normals"], AR.INTR, AR.DIST_THRES, AR.MIN_COSINE, 0.02)
    hl, hn = hand_maps()
    hp = np.array([(0.3125, 0.3125, 1), (0.390625, 0.390625, 1.25), (0.46875, 0.46875, 1.5)], F32)
    st, _ = check(hp, None, hl, None, HINTR, 10.0, 0.5, 0.25)
    assert st.tolist() == [0, 0, 4]
    check(pts[:100], nrm[:100], lp, ln, intr, 0.15, 0.6, 0.05)
    with torch.cuda.stream(torch.cuda.Stream()):
        check(pts, nrm, lp, ln, intr, 0.15, 0.6, 0.05)
        check(hp, None, hl, None, HINTR, 10.0, 0.5, 0.25)
    assert capi.lib().dfusion_release_scratch() == 0
    check(pts, nrm, lp, ln, intr, 0.15, 0.6, 0.05)


def test_argument_checks():
    pts, nrm, lp, ln, intr = random_set(64, seed=19)
    L = capi.lib()
    p, n, a, b = _dev(pts), _dev(nrm), _dev(lp), _dev(ln)
    out = torch.empty((64, 3), dtype=torch.float32, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    rows, cols = lp.shape[:2]
    base = dict(points=P(p), normals=P(n), N=64, lp=P(a), lpp=cols * 16, ln=P(b), lnp=cols * 16, cols=cols, rows=rows,
                intr=capi.floats(intr), dist=0.15, mc=0.6, margin=0.05, out=P(out))

    def call(**kw):
        k = dict(base); k.update(kw)
        return L.dfusion_associate_projective(k["points"], k["normals"], k["N"], k["lp"], k["lpp"], k["ln"], k["lnp"], k["cols"], k["rows"],
                                              k["intr"], k["dist"], k["mc"], k["margin"], k["out"], None, None, None)
    assert call() == 0
    for bad in (dict(N=-1), dict(cols=0), dict(rows=0), dict(cols=-3), dict(rows=-1), dict(points=None), dict(lp=None), dict(out=None),
                dict(intr=None), dict(normals=None), dict(ln=None), dict(lpp=cols * 16 - 1), dict(lnp=cols * 16 - 16), dict(lpp=0),
                dict(dist=-0.01), dict(dist=float("nan")), dict(mc=float("nan"))):
        assert call(**bad) == INVALID, bad
    assert call(normals=None, ln=None, lnp=0) == 0                                 # both NULL: no normal test
    assert call(dist=0.0) == 0 and call(mc=-1.0) == 0 and call(mc=2.0) == 0 and call(margin=float("nan")) == 0
    assert call(N=0, points=None, out=None) == 0                                   # nothing to read or write
    assert call(N=0, cols=0) == INVALID
    torch.cuda.synchronize()
