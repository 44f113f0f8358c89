"""GPU parity of the point-to-plane warp solve (dfusion_warp_solve_plane) against the numpy restatement
tests/solver_plane_ref.py, which tests/test_solver_plane_rule.py checks on the CPU: the transforms, the four energies and the last
round's point and edge weights bit for bit across the node-count, neighbour-count, graph, round and penalty settings that change a
dispatch (every coupled step kernel and every projecting W p kernel is new code); all points invalid; N around one workgroup;
convergence before the steps run out; normals that are not unit; the same call twice; one handle through the older entry points and
this one at changing sizes; a fresh stream; the argument checks; the C++ mirror.

The grid is a covering design, not the full product: every M meets every penalty setting and every k, and kg = 0 / 4 and rounds = 1 / 3
each occur with every M, every k and every penalty setting that has a meaning there (Huber needs edges)."""
import subprocess

import numpy as np
import pytest
import torch

import solver_plane_ref as P
from dynamicfusion_amd import build, capi
from solver_cases import (DF_E_INVALID, HUBER_DELTA, ITERS, LAM, LREG, MODES, N, TUKEY_C, assert_same, bits, dev, field, lcg_normals, lcg_problem,
                          random_nodes, seeded_normals)
from solver_cases import shared_plane_problem as shared_problem

pytestmark = pytest.mark.gpu
F32 = np.float32


def run_gpu(wf, src, dst, nrm, k, kg, lreg, rounds, c, delta, iters=ITERS, lam=LAM):
    out = wf.solve_plane(dev(src), dev(dst), dev(nrm), iters=iters, lam=lam, reg_neighbours=kg, reg_lambda=lreg, rounds=rounds, tukey_c=c,
                         huber_delta=delta, k=k, return_weights=True)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in out]


GRID = [
    # M,    k, kg, rounds, mode        step kernel
    (40,    8, 4, 3, "both"),        # register-resident, 2 elements a thread
    (40,    4, 0, 1, "off"),
    (40,    3, 4, 1, "huber"),
    (40,    4, 0, 3, "tukey"),
    (2049,  4, 4, 1, "both"),        # 5 elements a thread
    (2049,  3, 4, 3, "off"),
    (2049,  8, 4, 3, "huber"),
    (2049,  8, 0, 1, "tukey"),
    (5121,  3, 0, 3, "tukey"),       # 8 elements a thread
    (5121,  8, 4, 1, "off"),
    (5121,  4, 4, 3, "both"),
    (5121,  8, 4, 1, "huber"),
    (8193,  8, 0, 1, "off"),         # the general step kernel
    (8193,  4, 4, 1, "huber"),
    (8193,  3, 4, 3, "both"),
    (8193,  8, 0, 3, "tukey"),
]


@pytest.mark.parametrize("M,k,kg,rounds,mode", GRID, ids=["M%d-k%d-kg%d-r%d-%s" % c for c in GRID])
def test_matches_the_restatement_bit_for_bit(M, k, kg, rounds, mode):
    pos, sigma, dq, src, dst, nrm = shared_problem(M)
    c, delta = MODES[mode]
    wf = field(pos, sigma, dq, k)
    got = run_gpu(wf, src, dst, nrm, k, kg, LREG, rounds, c, delta)
    d = {}
    want = P.solve_plane(pos, dq, sigma, src, dst, nrm, k, ITERS, LAM, kg, LREG, rounds, c, delta, details=d)
    pw, ew = want[2], want[3]
    print("M %d k %d kg %d rounds %d %s: energies gpu %s restatement %s; steps %s; points with weight 0: %d, in (0, 1): %d; edges below 1: %s" % (
        M, k, kg, rounds, mode, got[1], want[1], d["steps"], int((pw == 0).sum()), int(((pw > 0) & (pw < 1)).sum()),
        None if ew is None else int((ew < 1).sum())))
    assert d["steps"] == [ITERS] * rounds and any(x.any() for x in d["x"])       # every step ran, and moved nodes
    bad = ~np.isfinite(nrm).all(1)
    assert bad.sum() > 20 and (d["keys"][bad] == M).all()                       # the inputs use the normals' validity rule
    if c:                                                # and both branches of both weight functions
        assert (pw == 0).sum() > 100 and ((pw > 0) & (pw < 1)).sum() > 100
    if delta:
        assert (ew < 1).any() and (ew == 1).any()
    assert_same(got, want, "gpu against the restatement")
    assert np.array_equal(bits(wf._dq.cpu().numpy()), bits(want[0]))


def test_it_is_not_the_point_to_point_solve():
    pos, sigma, dq, src, dst, nrm = shared_problem(40)
    a = run_gpu(field(pos, sigma, dq), src, dst, nrm, 8, 4, LREG, 1, 0.0, 0.0)
    b_dq, b_en = field(pos, sigma, dq).solve(dev(src), dev(dst), iters=ITERS, lam=LAM, reg_neighbours=4, reg_lambda=LREG)
    torch.cuda.synchronize()
    assert not np.array_equal(bits(a[0]), bits(b_dq.cpu().numpy()))
    assert a[1][0] < b_en.cpu().numpy()[0]               # |n . e|^2 <= |e|^2 for unit normals
    assert np.array_equal(bits(a[1][2]), bits(b_en.cpu().numpy()[2]))           # E_reg before the solve is the same term


def test_all_points_invalid():
    """Every normal NaN: no entry, r0 = 0 without a graph, so the recurrence never starts and a round writes what a 0-step solve writes."""
    pos, sigma, dq, src, dst, _ = shared_problem(40)
    nrm = np.full((N, 3), np.nan, F32)
    for kg, rounds in ((0, 2), (4, 1)):
        got = run_gpu(field(pos, sigma, dq), src, dst, nrm, 8, kg, LREG, rounds, TUKEY_C, 0.0)
        d = {}
        want = P.solve_plane(pos, dq, sigma, src, dst, nrm, 8, ITERS, LAM, kg, LREG, rounds, TUKEY_C, 0.0, details=d)
        assert (d["keys"] == 40).all() and want[1][0] == 0 and (want[2] == 1).all()
        assert_same(got, want, "all points invalid, kg %d" % kg)
        if kg == 0:
            assert d["steps"] == [0, 0]
            wf = field(pos, sigma, dq)
            for _ in range(rounds):
                zero_step, _ = wf.energy_data(dev(src), dev(dst), iters=0, lam=LAM)
            torch.cuda.synchronize()
            assert np.array_equal(bits(got[0]), bits(zero_step.cpu().numpy()))


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_point_counts_around_one_workgroup(n):
    pos, sigma, dq, src, dst, nrm = shared_problem(40)
    src, dst, nrm = src[1:n + 1], dst[1:n + 1], nrm[1:n + 1]                    # (point 0 is a NaN point)
    assert np.isfinite(src[0]).all() and np.isfinite(dst[0]).all() and np.isfinite(nrm[0]).all()
    got = run_gpu(field(pos, sigma, dq), src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, HUBER_DELTA)
    assert_same(got, P.solve_plane(pos, dq, sigma, src, dst, nrm, 8, ITERS, LAM, 4, LREG, 2, TUKEY_C, HUBER_DELTA), "N = %d" % n)


def test_convergence_before_the_steps_run_out():
    """400 steps asked for at M = 40: the recurrence freezes long before (|r|^2 <= 1e-10 |r0|^2) and the kernels of the remaining steps
    return at once -- the restatement stops there, and the bits are its bits."""
    pos, sigma, dq, src, dst, nrm = shared_problem(40)
    d = {}
    want = P.solve_plane(pos, dq, sigma, src, dst, nrm, 8, 400, LAM, 4, LREG, 2, TUKEY_C, 0.0, details=d)
    print("steps taken per round:", d["steps"])
    assert all(0 < s < 400 for s in d["steps"])
    got = run_gpu(field(pos, sigma, dq), src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, 0.0, iters=400)
    assert_same(got, want, "early out")


def test_normals_are_used_as_given():
    pos, sigma, dq, src, dst, nrm = shared_problem(40)
    scale = np.random.default_rng(3).uniform(0.2, 3.0, (N, 1)).astype(F32)
    with np.errstate(invalid="ignore"):
        scaled = (nrm * scale).astype(F32)
    got = run_gpu(field(pos, sigma, dq), src, dst, scaled, 8, 4, LREG, 2, TUKEY_C, HUBER_DELTA)
    assert_same(got, P.solve_plane(pos, dq, sigma, src, dst, scaled, 8, ITERS, LAM, 4, LREG, 2, TUKEY_C, HUBER_DELTA), "non-unit normals")
    unit = run_gpu(field(pos, sigma, dq), src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, HUBER_DELTA)
    assert not np.array_equal(bits(got[0]), bits(unit[0]))                      # nothing normalised them


def test_the_same_call_twice_gives_the_same_bits():
    pos, sigma, dq, src, dst, nrm = shared_problem(2049)
    wf = field(pos, sigma, dq)
    a = run_gpu(wf, src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, HUBER_DELTA)
    wf.set_transforms(dev(dq))
    b = run_gpu(wf, src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, HUBER_DELTA)
    assert_same(a, b, "second call on the handle")
    assert_same(a, run_gpu(field(pos, sigma, dq), src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, HUBER_DELTA), "a fresh handle")


def test_one_handle_serves_every_entry_point_while_its_workspace_grows_and_shrinks():
    """The entry points carve one workspace on the handle, and the plane solve adds a piece to it.  Calls of different shapes in a row
    must each give the bits of the same call on a fresh handle: nothing a differently shaped call left behind is read."""
    pos, sigma, dq, src, dst, nrm = shared_problem(40)
    small, large = (dev(src[:300]), dev(dst[:300])), (dev(src), dev(dst))
    n_small, n_large = dev(nrm[:300]), dev(nrm)
    kw = dict(iters=ITERS, lam=LAM, k=4)
    graph = dict(reg_neighbours=2, reg_lambda=LREG)
    steps = [
        lambda wf: wf.solve(*small, **graph, **kw),
        lambda wf: wf.solve_plane(*large, n_large, rounds=2, tukey_c=TUKEY_C, huber_delta=HUBER_DELTA, return_weights=True, **graph, **kw),
        lambda wf: wf.solve_robust(*small, rounds=2, tukey_c=TUKEY_C, huber_delta=HUBER_DELTA, return_weights=True, **graph, **kw),
        lambda wf: wf.solve_plane(*small, n_small, **kw),
        lambda wf: wf.solve(*large, **graph, **kw),
        lambda wf: wf.solve_plane(*large, n_large, rounds=1, tukey_c=TUKEY_C, return_weights=True, **kw),
        lambda wf: wf.energy_data(*small, **kw),
    ]

    def run(wf, step):
        wf.set_transforms(dev(dq))
        out = step(wf)
        torch.cuda.synchronize()
        return [None if t is None else bits(t.cpu().numpy()) for t in out]
    one = field(pos, sigma, dq, 4)
    got = [run(one, step) for step in steps]
    for i, step in enumerate(steps):
        want = run(field(pos, sigma, dq, 4), step)
        assert len(got[i]) == len(want)
        for j, (g, w) in enumerate(zip(got[i], want)):
            assert (g is None and w is None) or np.array_equal(g, w), "call %d, output %d: the shared handle against a fresh one" % (i + 1, j)
    assert [len(g) for g in got] == [2, 4, 4, 2, 2, 4, 2]
    assert (got[1][2] == 0).any() and (got[1][3] != bits(F32(1))).any()        # both penalties were live in call 2


def test_a_fresh_stream():
    pos, sigma, dq, src, dst, nrm = shared_problem(40)
    want = run_gpu(field(pos, sigma, dq), src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, HUBER_DELTA)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        wf = field(pos, sigma, dq)
        out = wf.solve_plane(dev(src), dev(dst), dev(nrm), iters=ITERS, lam=LAM, reg_neighbours=4, reg_lambda=LREG, rounds=2, tukey_c=TUKEY_C,
                             huber_delta=HUBER_DELTA, return_weights=True)
        s.synchronize()
        got = [t.cpu().numpy() for t in out]
    torch.cuda.synchronize()
    assert_same(got, want, "a fresh stream against the default stream")


def test_invalid_arguments():
    L = capi.lib()
    pos = random_nodes(5)
    wf = field(pos, np.full(5, 0.4, F32), k=4)
    pts = dev(np.random.default_rng(1).uniform(-1, 1, (64, 3)).astype(F32))
    nrm = dev(seeded_normals(64, marked=False))
    dq = torch.empty((5, 8), dtype=torch.float32, device="cuda"); en = torch.zeros(4, dtype=torch.float32, device="cuda")
    pw = torch.empty(64, dtype=torch.float32, device="cuda"); ew = torch.empty((5, 7), dtype=torch.float32, device="cuda")
    here = object()

    def call(kg=2, lreg=1.0, rounds=2, c=0.05, delta=0.01, k=4, n=64, iters=3, lam=0.0, edge=None, points=here, live=here, normals=here, handle=here):
        p = [pts.data_ptr() if a is here else a for a in (points, live)]
        return L.dfusion_warp_solve_plane(wf.handle if handle is here else handle, k, p[0], p[1], nrm.data_ptr() if normals is here else normals, n,
                                          iters, lam, kg, lreg, rounds, c, delta, dq.data_ptr(), en.data_ptr(), pw.data_ptr(), edge, None)
    nan = float("nan")
    # what dfusion_warp_solve refuses
    for bad in (dict(kg=-1), dict(kg=8), dict(kg=5), dict(kg=7, lreg=0.0), dict(lreg=-1.0), dict(lreg=nan), dict(kg=0, lreg=nan),
                dict(k=0), dict(k=9), dict(k=6), dict(n=0), dict(n=-4), dict(iters=-1), dict(lam=-1.0), dict(lam=nan), dict(points=None),
                dict(live=None), dict(handle=None)):
        assert call(**bad) == DF_E_INVALID, bad
    # what dfusion_warp_solve_robust adds
    for bad in (dict(rounds=0), dict(rounds=-3), dict(c=-0.05), dict(c=nan), dict(delta=-0.01), dict(delta=nan),
                dict(kg=0, edge=ew.data_ptr()), dict(lreg=0.0, edge=ew.data_ptr())):
        assert call(**bad) == DF_E_INVALID, bad
    # its own
    assert call(normals=None) == DF_E_INVALID
    assert call() == 0 and call(kg=4, edge=ew.data_ptr()) == 0 and call(kg=0, lreg=0.0, c=0.0, delta=0.0, rounds=1) == 0
    assert L.dfusion_warp_solve_plane(wf.handle, 4, pts.data_ptr(), pts.data_ptr(), nrm.data_ptr(), 64, 3, 0.0, 2, 1.0, 2, 0.05, 0.01, None, None,
                                      None, None, None) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the C++ mirror
def test_cxx_mirror_prints_the_restatements_bits():
    build.build_host()
    r = subprocess.run([build.HOST_WARP_SOLVE, "plane"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [[int(w, 16) for w in line.split()] for line in r.stdout.strip().splitlines()]
    got_dq, got_en = np.array(lines[:-1], np.uint32), np.array(lines[-1], np.uint32)
    pos, dq, sigma, src, dst = lcg_problem()
    nrm = lcg_normals(len(src))
    want_dq, want_en, pw, ew = P.solve_plane(pos, dq, sigma, src, dst, nrm, 8, 20, 1e-3, 4, 1.0, 3, 0.02, 0.01)
    assert got_dq.shape == (50, 8)
    assert np.array_equal(got_dq, bits(want_dq)) and np.array_equal(got_en, bits(want_en))
    assert (pw == 0).any() and ((pw > 0) & (pw < 1)).any() and (ew < 1).any()   # both penalties were live on the app's problem
    robust, _ = field(pos, sigma, dq).solve_robust(dev(src), dev(dst), iters=20, lam=1e-3, reg_neighbours=4, reg_lambda=1.0, rounds=3,
                                                   tukey_c=0.02, huber_delta=0.01)
    assert not np.array_equal(got_dq, bits(robust.cpu().numpy()))               # the mirror's switch did switch
