"""The warp-field extension rule without a GPU: extend_ref's decimation against a brute-force loop, the support test against a
brute-force k-NN, and the interfaces that carry dfusion_warp_extend (C-ABI export, ctypes binding, Python and C++ mirrors)."""
import ctypes as C
import os

import numpy as np

import extend_ref as X
import oracle_lib as O
from dynamicfusion_amd import WarpField, build, capi

F32 = np.float32


def brute_winners(points, candidate, radius):
    seen, out = set(), []
    for i, p in enumerate(np.asarray(points, F32)):
        if not candidate[i]:
            continue
        f = [F32(p[a]) / F32(radius) for a in range(3)]
        if not all(abs(x) < F32(2.0 ** 30) for x in f):        # (False for NaN)
            continue
        c = tuple(int(np.floor(x)) for x in f)
        if c not in seen:
            seen.add(c)
            out.append(i)
    return np.array(out, np.int64)


def cloud(rng, n, radius):
    p = rng.uniform(-1.0, 1.0, (n, 3)).astype(F32)
    p[::7] = (np.round(p[::7] / radius) * radius).astype(F32)    # on cell borders (up to the rounding of the product)
    p[3::11] = (rng.integers(-20, 20, (len(p[3::11]), 3)) * F32(radius)).astype(F32)
    p[5::13, 1] = np.nan
    p[6::29, 2] = np.inf
    p[8::31, 0] = F32(-3e9) * F32(radius)                        # beyond 2^30 cells
    return p


def test_decimation_matches_a_brute_force_loop():
    rng = np.random.default_rng(11)
    for radius in (0.05, 0.125, 0.3):
        p = cloud(rng, 3000, radius)
        cand = rng.random(len(p)) < 0.6
        got = X.decimate(p, cand, radius)
        want = brute_winners(p, cand, radius)
        assert np.array_equal(got, want), radius
        assert np.all(np.diff(got) > 0)
        assert want.size > 50


def test_cells_take_negative_coordinates_to_lower_cells():
    valid, c = X.cells(np.array([[-0.01, 0.0, 0.099], [-0.1, 0.1, -0.2], [np.nan, 0, 0]], F32), 0.1)
    assert valid.tolist() == [True, True, False]
    assert c[0].tolist() == [-1, 0, 0] and c[1].tolist() == [-1, 1, -2]


def test_support_test_and_rule_against_brute_force_knn():
    rng = np.random.default_rng(3)
    pos = rng.uniform(-0.5, 0.5, (200, 3)).astype(F32)
    sigma = rng.uniform(0.03, 0.08, 200).astype(F32)
    dq = np.tile(np.array([1, 0, 0, 0, 0, 0, 0, 0], F32), (200, 1))
    pts = rng.uniform(-1.0, 1.0, (1500, 3)).astype(F32)
    pts[::17, 0] = np.nan
    for k in (4, 8):
        mask, idx, d2 = X.unsupported(pos, sigma, pts, k)
        fin = np.isfinite(pts).all(1)
        bd = ((pts[:, None, :] - pos[None]) ** 2).sum(-1)
        order = np.argsort(bd, 1, kind="stable")[:, :k]
        assert np.array_equal(np.sort(idx[fin], 1), np.sort(order[fin], 1))
        near = pos[order]
        dd = (pts[:, None, :] - near).astype(F32)
        d2b = (dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1]) + dd[..., 2] * dd[..., 2]
        want = fin & (d2b >= sigma[order] * sigma[order]).all(1)
        assert np.array_equal(mask, want)
        new_pos, new_dq, new_sig, n, w = X.extend_ref(pos, dq, sigma, pts, k, 0.1, 0.05, max_new=7)
        assert n == 7 and w > 7 and np.array_equal(new_pos.view(np.uint32), pts[X.decimate(pts, mask, 0.1)[:7]].view(np.uint32))
        assert np.isfinite(new_dq).all() and (new_sig == F32(0.05)).all()


def test_zero_weight_fallback_copies_the_nearest_transform():
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F32)
    dq = np.array([[np.cos(0.1 * i), np.sin(0.1 * i), 0, 0, 0, 0.1 * i, 0, 0] for i in range(4)], F32)
    sigma = np.full(4, 0.01, F32)
    new_pos, new_dq, _, n, w = X.extend_ref(pos, dq, sigma, np.array([[5.0, 0, 0], [0.5, 0.5, 0.5]], F32), 4, 0.5, 0.02)
    assert n == 2 and w == 2
    assert np.array_equal(new_dq[0], dq[1])                      # (5, 0, 0): nearest node 1, all weights 0
    assert np.array_equal(new_dq[1], dq[O.knn(pos, new_pos[1:], 4)[0][0, 0]])


def test_library_exports_dfusion_warp_extend():
    L = C.CDLL(build.build_library())
    assert hasattr(L, "dfusion_warp_extend")
    assert "dfusion_warp_extend" in capi.SYMBOLS
    hdr = open(os.path.join(build.REPO_DIR, "include", "dfusion.h")).read()
    assert "int dfusion_warp_extend(DfWarpField *wf," in hdr
    assert callable(getattr(WarpField, "extend", None))
    cxx = open(os.path.join(build.HOST_DIR, "include", "kfusion", "warp_field.hpp")).read()
    assert "int extend(const std::vector<Vec3f>& points, float radius, float sigma);" in cxx
