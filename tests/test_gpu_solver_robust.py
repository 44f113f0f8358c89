"""GPU parity of the robust warp solve (dfusion_warp_solve_robust) against the numpy restatement
tests/solver_robust_ref.py, which tests/test_solver_robust_rule.py checks on the CPU: the transforms, the four energies and the last
round's point and edge weights bit for bit across the node-count, neighbour-count, graph, round and penalty settings that change a
dispatch; the off switches; huge thresholds; all outliers; the graph cache; NaN points; argument checks; one handle through all three
entry points at changing sizes; how many energies the data-term entry point writes; the C++ mirror.

The grid is a covering design, not the full product (108 solves, the M = 8193 ones seconds each on the CPU side): every M meets every
penalty setting, every M meets every k, and kg = 0 / 4 and rounds = 1 / 3 each occur with every M, every k and every penalty setting
that has a meaning there (Huber needs edges)."""
import subprocess

import numpy as np
import pytest
import torch

import solver_robust_ref as RR
from dynamicfusion_amd import build, capi
from solver_cases import (DF_E_INVALID, HUBER_DELTA, ITERS, LAM, LREG, MODES, N, TUKEY_C, assert_same, bits, dev, field, lcg_problem, outlier_problem,
                          problem, random_nodes, shared_problem)

pytestmark = pytest.mark.gpu
F32 = np.float32


def run_gpu(wf, src, dst, k, kg, lreg, rounds, c, delta, iters=ITERS, lam=LAM):
    out = wf.solve_robust(dev(src), dev(dst), iters=iters, lam=lam, reg_neighbours=kg, reg_lambda=lreg, rounds=rounds, tukey_c=c,
                          huber_delta=delta, k=k, return_weights=True)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in out]


GRID = [
    # M,    k, kg, rounds, mode
    (40,    8, 4, 3, "both"),
    (40,    4, 0, 3, "tukey"),
    (40,    3, 4, 1, "huber"),
    (40,    8, 4, 1, "tukey"),
    (2049,  8, 4, 1, "both"),
    (2049,  4, 4, 3, "huber"),
    (2049,  3, 0, 1, "tukey"),
    (2049,  3, 4, 3, "tukey"),
    (8193,  8, 0, 3, "tukey"),
    (8193,  4, 4, 1, "both"),
    (8193,  3, 4, 3, "huber"),
    (8193,  8, 4, 1, "huber"),
    (40,    4, 4, 3, "both"),
    (2049,  8, 0, 3, "tukey"),
    (8193,  3, 0, 1, "tukey"),
]


@pytest.mark.parametrize("M,k,kg,rounds,mode", GRID, ids=["M%d-k%d-kg%d-r%d-%s" % c for c in GRID])
def test_matches_the_restatement_bit_for_bit(M, k, kg, rounds, mode):
    pos, sigma, dq, src, dst = shared_problem(M)
    c, delta = MODES[mode]
    wf = field(pos, sigma, dq, k)
    got = run_gpu(wf, src, dst, k, kg, LREG, rounds, c, delta)
    d = {}
    want = RR.solve_robust(pos, dq, sigma, src, dst, k, ITERS, LAM, kg, LREG, rounds, c, delta, details=d)
    pw, ew = want[2], want[3]
    print("M %d k %d kg %d rounds %d %s: energies gpu %s restatement %s; points with weight 0: %d, in (0, 1): %d; edges below 1: %s" % (
        M, k, kg, rounds, mode, got[1], want[1], int((pw == 0).sum()), int(((pw > 0) & (pw < 1)).sum()),
        None if ew is None else int((ew < 1).sum())))
    if c:                                                # the inputs use both branches of both weight functions
        assert (pw == 0).sum() > 100 and ((pw > 0) & (pw < 1)).sum() > 100
    if delta:
        assert (ew < 1).any() and (ew == 1).any()
    assert_same(got, want, "gpu against the restatement")
    assert np.array_equal(bits(wf._dq.cpu().numpy()), bits(want[0]))


def chained(pos, sigma, dq, src, dst, kg, lreg, rounds, iters=ITERS):
    wf = field(pos, sigma, dq)
    ens = []
    for _ in range(rounds):
        out, en = wf.solve(dev(src), dev(dst), iters=iters, lam=LAM, reg_neighbours=kg, reg_lambda=lreg)
        ens.append(en.cpu().numpy())
    torch.cuda.synchronize()
    return out.cpu().numpy(), np.array([ens[0][0], ens[-1][1], ens[0][2], ens[-1][3]], F32)


@pytest.mark.parametrize("rounds", [1, 3])
def test_off_switches_give_the_plain_solves_bits(rounds):
    pos = random_nodes(100)
    sigma, dq, src, dst = outlier_problem(pos)
    for kg, lreg in ((4, LREG), (0, 0.0), (4, 0.0)):
        want_dq, want_en = chained(pos, sigma, dq, src, dst, kg, lreg, rounds)
        g_dq, g_en, g_pw, g_ew = run_gpu(field(pos, sigma, dq), src, dst, 8, kg, lreg, rounds, 0.0, 0.0)
        assert np.array_equal(bits(g_dq), bits(want_dq)) and np.array_equal(bits(g_en), bits(want_en))
        assert (g_pw == 1).all() and (g_ew is None if not (kg and lreg) else (g_ew == 1).all())


def test_huge_thresholds_give_the_quadratic_rounds_through_the_weighted_path():
    pos = random_nodes(100)
    sigma, dq, src, dst = outlier_problem(pos)
    want_dq, _ = chained(pos, sigma, dq, src, dst, 4, LREG, 3)
    got = run_gpu(field(pos, sigma, dq), src, dst, 8, 4, LREG, 3, 1e6, 1e6)
    assert (got[2] == 1).all() and (got[3] == 1).all()
    assert np.array_equal(bits(got[0]), bits(want_dq))
    assert_same(got, RR.solve_robust(pos, dq, sigma, src, dst, 8, ITERS, LAM, 4, LREG, 3, 1e6, 1e6), "huge thresholds")


@pytest.mark.parametrize("rounds", [1, 3])
def test_all_outliers_leave_the_translations_alone(rounds):
    """omega = 0 everywhere and no graph: delta = 0 exactly, and a round writes what a 0-step solve writes (the write-back re-encodes
    the translation, which is not the identity on the bits -- so R rounds are R chained 0-step solves)."""
    pos = random_nodes(100)
    sigma, dq, src, dst = problem(pos, N)
    far = (src + F32([0.5, -0.4, 0.3])).astype(F32)                       # every residual past c (the transforms move a point by centimetres)
    got = run_gpu(field(pos, sigma, dq), src, far, 8, 0, 0.0, rounds, TUKEY_C, 0.0)
    assert (got[2][np.isfinite(src).all(1) & np.isfinite(far).all(1)] == 0).all()
    wf = field(pos, sigma, dq)
    for _ in range(rounds):
        zero_step, _ = wf.energy_data(dev(src), dev(far), iters=0, lam=LAM)
    torch.cuda.synchronize()
    assert np.array_equal(bits(got[0]), bits(zero_step.cpu().numpy()))
    d = {}
    assert_same(got, RR.solve_robust(pos, dq, sigma, src, far, 8, ITERS, LAM, 0, 0.0, rounds, TUKEY_C, 0.0, details=d), "all outliers")
    assert not any(x.any() for x in d["x"])


def test_the_cached_graph_is_only_read():
    pos = random_nodes(300)
    sigma, dq, src, dst = outlier_problem(pos)
    wf = field(pos, sigma, dq)
    nbr0, alpha0 = (t.cpu().numpy() for t in wf.node_graph(4))
    got = run_gpu(wf, src, dst, 8, 4, LREG, 3, TUKEY_C, HUBER_DELTA)
    assert (got[3] < 1).any()
    nbr1, alpha1 = (t.cpu().numpy() for t in wf.node_graph(4))
    assert np.array_equal(nbr0, nbr1) and np.array_equal(bits(alpha0), bits(alpha1))
    wf.set_transforms(dev(dq))
    a_dq, a_en = wf.solve(dev(src), dev(dst), iters=ITERS, lam=LAM, reg_neighbours=4, reg_lambda=LREG)
    b_dq, b_en = field(pos, sigma, dq).solve(dev(src), dev(dst), iters=ITERS, lam=LAM, reg_neighbours=4, reg_lambda=LREG)
    torch.cuda.synchronize()
    assert np.array_equal(bits(a_dq.cpu().numpy()), bits(b_dq.cpu().numpy())) and np.array_equal(bits(a_en.cpu().numpy()), bits(b_en.cpu().numpy()))


def test_nan_points_have_no_influence():
    pos = random_nodes(100)
    sigma, dq, src, dst = outlier_problem(pos)
    nan = np.isnan(src).any(1) | np.isnan(dst).any(1)
    assert 30 < nan.sum() < 100
    a = run_gpu(field(pos, sigma, dq), src, dst, 8, 4, LREG, 2, TUKEY_C, HUBER_DELTA)
    src2, dst2 = src.copy(), dst.copy()
    with np.errstate(invalid="ignore"):
        src2[nan] = src2[nan] * F32(3) + F32(1); dst2[nan] = dst2[nan] - F32(2)      # (NaN components stay NaN, the others move)
    b = run_gpu(field(pos, sigma, dq), src2, dst2, 8, 4, LREG, 2, TUKEY_C, HUBER_DELTA)
    assert_same(a, b, "NaN points with other finite components")
    assert (a[2][nan] == 1).all()                        # e0 = 0 for a skipped point: the rule gives weight 1 (and the point has no entry)
    assert_same(a, RR.solve_robust(pos, dq, sigma, src, dst, 8, ITERS, LAM, 4, LREG, 2, TUKEY_C, HUBER_DELTA), "NaN points")


def test_invalid_arguments():
    L = capi.lib()
    pos = random_nodes(5)
    wf = field(pos, np.full(5, 0.4, F32), k=4)
    pts = dev(np.random.default_rng(1).uniform(-1, 1, (64, 3)).astype(F32))
    dq = torch.empty((5, 8), dtype=torch.float32, device="cuda"); en = torch.zeros(4, dtype=torch.float32, device="cuda")
    pw = torch.empty(64, dtype=torch.float32, device="cuda"); ew = torch.empty((5, 7), dtype=torch.float32, device="cuda")

    def call(kg=2, lreg=1.0, rounds=2, c=0.05, delta=0.01, k=4, n=64, iters=3, lam=0.0, edge=None, points=pts):
        return L.dfusion_warp_solve_robust(wf.handle, k, points.data_ptr() if points is not None else None, pts.data_ptr(), n, iters, lam, kg,
                                           lreg, rounds, c, delta, dq.data_ptr(), en.data_ptr(), pw.data_ptr(), edge, None)
    nan = float("nan")
    # what dfusion_warp_solve refuses
    for bad in (dict(kg=-1), dict(kg=8), dict(kg=5), dict(kg=7, lreg=0.0), dict(lreg=-1.0), dict(lreg=nan), dict(kg=0, lreg=nan),
                dict(k=0), dict(k=9), dict(k=6), dict(n=0), dict(iters=-1), dict(lam=-1.0), dict(lam=nan), dict(points=None)):
        assert call(**bad) == DF_E_INVALID, bad
    # its own
    for bad in (dict(rounds=0), dict(rounds=-3), dict(c=-0.05), dict(c=nan), dict(delta=-0.01), dict(delta=nan),
                dict(kg=0, edge=ew.data_ptr()), dict(lreg=0.0, edge=ew.data_ptr())):
        assert call(**bad) == DF_E_INVALID, bad
    assert L.dfusion_warp_solve_robust(None, 4, pts.data_ptr(), pts.data_ptr(), 64, 3, 0.0, 2, 1.0, 2, 0.05, 0.01, None, None, None, None, None) == DF_E_INVALID
    assert call() == 0 and call(kg=4, edge=ew.data_ptr()) == 0 and call(kg=0, lreg=0.0, c=0.0, delta=0.0, rounds=1) == 0
    assert L.dfusion_warp_solve_robust(wf.handle, 4, pts.data_ptr(), pts.data_ptr(), 64, 3, 0.0, 2, 1.0, 2, 0.05, 0.01, None, None, None, None, None) == 0
    torch.cuda.synchronize()


def test_one_handle_serves_every_entry_point_while_its_workspace_grows_and_shrinks():
    """The three entry points carve one workspace on the handle.  Calls of different shapes in a row (N = 300 / 3001, with and without
    the graph's and the penalties' pieces) must each give the bits of the same call on a fresh handle: nothing a differently shaped call
    left behind is read."""
    pos = random_nodes(40)
    sigma, dq, src, dst = outlier_problem(pos)
    small, large = (dev(src[:300]), dev(dst[:300])), (dev(src), dev(dst))
    kw = dict(iters=ITERS, lam=LAM, k=4)
    graph = dict(reg_neighbours=2, reg_lambda=LREG)
    steps = [
        lambda wf: wf.energy_data(*small, **kw),
        lambda wf: wf.solve_robust(*large, rounds=2, tukey_c=TUKEY_C, huber_delta=HUBER_DELTA, return_weights=True, **graph, **kw),
        lambda wf: wf.solve(*small, **graph, **kw),
        lambda wf: wf.solve_robust(*small, rounds=1, tukey_c=0.0, huber_delta=0.0, return_weights=True, **graph, **kw),
        lambda wf: wf.energy_data(*large, **kw),
    ]

    def run(wf, step):
        wf.set_transforms(dev(dq))
        out = step(wf)
        torch.cuda.synchronize()
        return [bits(t.cpu().numpy()) for t in out]
    one = field(pos, sigma, dq, 4)
    got = [run(one, step) for step in steps]
    for i, step in enumerate(steps):
        want = run(field(pos, sigma, dq, 4), step)
        assert len(got[i]) == len(want)
        for j, (g, w) in enumerate(zip(got[i], want)):
            assert np.array_equal(g, w), "call %d, output %d: the shared handle against a fresh one" % (i + 1, j)
    assert [len(g) for g in got] == [2, 4, 2, 4, 2]
    assert (got[1][2] == 0).any() and (got[1][3] != bits(F32(1))).any()        # both penalties were live in call 2
    assert np.array_equal(got[3][0], got[2][0]) and np.array_equal(got[3][1], got[2][1])   # all off, one round: the plain solve
    assert (got[3][2] == bits(F32(1))).all() and (got[3][3] == bits(F32(1))).all()


def test_the_data_term_entry_point_writes_two_energies():
    L = capi.lib()
    pos = random_nodes(5)
    wf = field(pos, np.full(5, 0.4, F32), k=4)
    src = np.random.default_rng(1).uniform(-1, 1, (64, 3)).astype(F32)
    pts, live = dev(src), dev(src + F32(0.01))
    dq = torch.empty((5, 8), dtype=torch.float32, device="cuda"); en = torch.full((4,), -7.0, dtype=torch.float32, device="cuda")
    assert L.dfusion_warp_solve_data_term(wf.handle, 4, pts.data_ptr(), live.data_ptr(), 64, 3, 0.0, dq.data_ptr(), en.data_ptr(), None) == 0
    torch.cuda.synchronize()
    e = en.cpu().numpy()
    assert e[0] > 0 and 0 <= e[1] < e[0] and (e[2:] == -7).all(), e
    assert L.dfusion_warp_solve(wf.handle, 4, pts.data_ptr(), live.data_ptr(), 64, 3, 0.0, 0, 1.0, dq.data_ptr(), en.data_ptr(), None) == 0
    torch.cuda.synchronize()
    e = en.cpu().numpy()
    assert e[0] > 0 and (bits(e[2:]) == 0).all(), e


# ------------------------------------------------------------------------------------------------ the C++ mirror
def test_cxx_mirror_prints_the_python_mirrors_bits():
    build.build_host()
    r = subprocess.run([build.HOST_WARP_SOLVE, "robust"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [[int(w, 16) for w in line.split()] for line in r.stdout.strip().splitlines()]
    got_dq, got_en = np.array(lines[:-1], np.uint32), np.array(lines[-1], np.uint32)
    pos, dq, sigma, src, dst = lcg_problem()
    want_dq, want_en, pw, ew = run_gpu(field(pos, sigma, dq), src, dst, 8, 4, 1.0, 3, 0.04, 0.01, iters=20, lam=1e-3)
    assert got_dq.shape == (50, 8)
    assert np.array_equal(got_dq, bits(want_dq)) and np.array_equal(got_en, bits(want_en))
    assert (pw == 0).any() and (ew < 1).any()            # both penalties were live on the app's problem
    plain, _ = field(pos, sigma, dq).solve(dev(src), dev(dst), iters=20, lam=1e-3, reg_neighbours=4, reg_lambda=1.0)
    assert not np.array_equal(got_dq, bits(plain.cpu().numpy()))
