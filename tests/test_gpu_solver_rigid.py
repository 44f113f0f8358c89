"""GPU parity of the warp solve with node rotations as unknowns (dfusion_warp_solve_rigid) against the numpy restatement
tests/solver_rigid_ref.py, which tests/test_solver_rigid_rule.py checks on the CPU: the transforms, the four energies and the last
round's point and edge weights bit for bit across the node-count, neighbour-count, graph, normal, round and penalty settings that change
a dispatch (the step kernels are dispatched on 2 M entries); all points invalid; N around one workgroup; convergence before the steps
run out; the same call twice; one handle through the older entry points and this one at changing sizes, which keep their bits; a fresh
stream; with brick lists and without an index; the argument checks; the C++ mirror.

The grid is a covering design, not the full product: every M meets every penalty setting and every k, and kg = 0 / 4, rounds = 1 / 3
and normals given / None each occur with every M, every k and every penalty setting that has a meaning there (Huber needs edges)."""
import numpy as np
import pytest
import torch

import solver_plane_ref as P
import solver_rigid_ref as G
import solver_robust_ref as RR
from dynamicfusion_amd import WarpField, capi
from solver_cases import (DF_E_INVALID, HUBER_DELTA, ITERS, LAM, LREG, LROT, MODES, N, TUKEY_C, assert_same, bits, dev, field, lcg_normals, lcg_problem,
                          random_nodes, seeded_normals)
from solver_cases import shared_plane_problem as shared_problem
from test_gpu_ties import index_volume

pytestmark = pytest.mark.gpu
F32 = np.float32


def run_gpu(wf, src, dst, nrm, k, kg, lreg, rounds, c, delta, iters=ITERS, lam=LAM, lrot=LROT):
    out = wf.solve_rigid(dev(src), dev(dst), None if nrm is None else dev(nrm), iters=iters, lam=lam, lam_rot=lrot, reg_neighbours=kg,
                         reg_lambda=lreg, rounds=rounds, tukey_c=c, huber_delta=delta, k=k, return_weights=True)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in out]


def restated(pos, dq, sigma, src, dst, nrm, k, kg, lreg, rounds, c, delta, iters=ITERS, lam=LAM, lrot=LROT, details=None):
    return G.solve_rigid(pos, dq, sigma, src, dst, nrm, k, iters, lam, lrot, kg, lreg, rounds, c, delta, details=details)


GRID = [
    # M,    k, kg, rounds, mode, normals     step kernel, on 2 M entries
    (40,    8, 4, 3, "both", True),        # register-resident, 2 elements a thread
    (40,    4, 0, 1, "off", False),
    (40,    3, 4, 1, "huber", True),
    (40,    4, 0, 3, "tukey", False),
    (1025,  4, 4, 1, "both", False),       # 5 elements a thread
    (1025,  3, 4, 3, "off", True),
    (1025,  8, 4, 3, "huber", False),
    (1025,  8, 0, 1, "tukey", True),
    (2561,  3, 0, 3, "tukey", True),       # 8 elements a thread
    (2561,  8, 4, 1, "off", False),
    (2561,  4, 4, 3, "both", True),
    (2561,  8, 4, 1, "huber", True),
    (4097,  8, 0, 1, "off", True),         # the general step kernel
    (4097,  4, 4, 1, "huber", False),
    (4097,  3, 4, 3, "both", False),
    (4097,  8, 0, 3, "tukey", False),
]


@pytest.mark.parametrize("M,k,kg,rounds,mode,normals", GRID, ids=["M%d-k%d-kg%d-r%d-%s-%s" % (c[:5] + ("plane" if c[5] else "point",)) for c in GRID])
def test_matches_the_restatement_bit_for_bit(M, k, kg, rounds, mode, normals):
    pos, sigma, dq, src, dst, nrm = shared_problem(M)
    nrm = nrm if normals else None
    c, delta = MODES[mode]
    wf = field(pos, sigma, dq, k)
    got = run_gpu(wf, src, dst, nrm, k, kg, LREG, rounds, c, delta)
    d = {}
    want = restated(pos, dq, sigma, src, dst, nrm, k, kg, LREG, rounds, c, delta, details=d)
    pw, ew = want[2], want[3]
    print("M %d k %d kg %d rounds %d %s normals %s: energies gpu %s restatement %s; steps %s; points with weight 0: %d, in (0, 1): %d; "
          "edges below 1: %s" % (M, k, kg, rounds, mode, normals, got[1], want[1], d["steps"], int((pw == 0).sum()),
                                 int(((pw > 0) & (pw < 1)).sum()), None if ew is None else int((ew < 1).sum())))
    assert d["steps"] == [ITERS] * rounds                                # every step ran ...
    assert all(x[:M].any() and x[M:].any() for x in d["x"])              # ... and turned and moved nodes
    assert (bits(want[0][:, :4]) != bits(dq[:, :4])).any()               # the rotations are not the seeds
    if normals:
        bad = ~np.isfinite(nrm).all(1)
        assert bad.sum() > 20 and (d["keys"][bad] == M).all()            # the inputs use the normals' validity rule
    if c:                                                                # and both branches of both weight functions
        assert (pw == 0).sum() > 100 and ((pw > 0) & (pw < 1)).sum() > 100
    if delta:
        assert (ew < 1).any() and (ew == 1).any()
    assert_same(got, want, "gpu against the restatement")
    assert np.array_equal(bits(wf._dq.cpu().numpy()), bits(want[0]))


def test_it_is_not_the_translation_only_solve():
    pos, sigma, dq, src, dst, nrm = shared_problem(40)
    a = run_gpu(field(pos, sigma, dq), src, dst, nrm, 8, 4, LREG, 1, 0.0, 0.0)
    b = field(pos, sigma, dq).solve_plane(dev(src), dev(dst), dev(nrm), iters=ITERS, lam=LAM, reg_neighbours=4, reg_lambda=LREG)
    torch.cuda.synchronize()
    b_dq = b[0].cpu().numpy()
    assert np.array_equal(bits(b_dq[:, :4]), bits(dq[:, :4]))            # the older solve keeps every rotation
    assert (bits(a[0][:, :4]) != bits(dq[:, :4])).any(1).sum() > 30      # this one turns the nodes


def test_all_points_invalid():
    """Every normal NaN: no entry, r0 = 0 without a graph, so the recurrence never starts and every node keeps its eight floats."""
    pos, sigma, dq, src, dst, _ = shared_problem(40)
    nrm = np.full((N, 3), np.nan, F32)
    for kg, rounds in ((0, 2), (4, 1)):
        got = run_gpu(field(pos, sigma, dq), src, dst, nrm, 8, kg, LREG, rounds, TUKEY_C, 0.0)
        d = {}
        want = restated(pos, dq, sigma, src, dst, nrm, 8, kg, LREG, rounds, TUKEY_C, 0.0, details=d)
        assert (d["keys"] == 40).all() and want[1][0] == 0 and (want[2] == 1).all()
        assert_same(got, want, "all points invalid, kg %d" % kg)
        if kg == 0:
            assert d["steps"] == [0, 0] and np.array_equal(bits(got[0]), bits(dq))


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_point_counts_around_one_workgroup(n):
    pos, sigma, dq, src, dst, nrm = shared_problem(40)
    src, dst, nrm = src[1:n + 1], dst[1:n + 1], nrm[1:n + 1]                    # (point 0 is a NaN point)
    assert np.isfinite(src[0]).all() and np.isfinite(dst[0]).all() and np.isfinite(nrm[0]).all()
    got = run_gpu(field(pos, sigma, dq), src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, HUBER_DELTA)
    assert_same(got, restated(pos, dq, sigma, src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, HUBER_DELTA), "N = %d" % n)


def test_convergence_before_the_steps_run_out():
    """400 steps asked for at M = 40, damped so that the recurrence freezes before (|r|^2 <= 1e-10 |r0|^2) and the kernels of the
    remaining steps return at once -- the restatement stops there, and the bits are its bits."""
    pos, sigma, dq, src, dst, nrm = shared_problem(40)
    d = {}
    want = restated(pos, dq, sigma, src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, 0.0, iters=400, lam=1e-2, lrot=1e-1, details=d)
    print("steps taken per round:", d["steps"])
    assert all(0 < s < 400 for s in d["steps"])
    got = run_gpu(field(pos, sigma, dq), src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, 0.0, iters=400, lam=1e-2, lrot=1e-1)
    assert_same(got, want, "early out")


def test_the_same_call_twice_gives_the_same_bits():
    pos, sigma, dq, src, dst, nrm = shared_problem(1025)
    wf = field(pos, sigma, dq)
    a = run_gpu(wf, src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, HUBER_DELTA)
    wf.set_transforms(dev(dq))
    b = run_gpu(wf, src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, HUBER_DELTA)
    assert_same(a, b, "second call on the handle")
    assert_same(a, run_gpu(field(pos, sigma, dq), src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, HUBER_DELTA), "a fresh handle")


def test_one_handle_serves_every_entry_point_and_the_older_ones_keep_their_bits():
    """The entry points carve one workspace on the handle, and this solve adds pieces to it and doubles others.  Calls of different shapes
    in a row must each give the bits of the same call on a fresh handle -- solve_plane and solve_robust behind solve_rigid included, and
    those two are the restatements' bits as before."""
    pos, sigma, dq, src, dst, nrm = shared_problem(40)
    small, large = (dev(src[:300]), dev(dst[:300])), (dev(src), dev(dst))
    n_small, n_large = dev(nrm[:300]), dev(nrm)
    kw = dict(iters=ITERS, lam=LAM, k=4)
    graph = dict(reg_neighbours=2, reg_lambda=LREG)
    robust = dict(rounds=2, tukey_c=TUKEY_C, huber_delta=HUBER_DELTA, return_weights=True)
    steps = [
        lambda wf: wf.solve(*small, **graph, **kw),
        lambda wf: wf.solve_rigid(*large, n_large, lam_rot=LROT, **robust, **graph, **kw),
        lambda wf: wf.solve_plane(*large, n_large, **robust, **graph, **kw),
        lambda wf: wf.solve_robust(*small, **robust, **graph, **kw),
        lambda wf: wf.solve_rigid(*small, None, lam_rot=LROT, **kw),
        lambda wf: wf.solve_plane(*small, n_small, **kw),
        lambda wf: wf.solve_rigid(*large, None, lam_rot=LROT, rounds=1, tukey_c=TUKEY_C, return_weights=True, **kw),
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
    assert [len(g) for g in got] == [2, 4, 4, 4, 2, 2, 4, 2]
    assert (got[1][2] == 0).any() and (got[1][3] != bits(F32(1))).any()        # both penalties were live in call 2
    plane = P.solve_plane(pos, dq, sigma, src, dst, nrm, 4, ITERS, LAM, 2, LREG, 2, TUKEY_C, HUBER_DELTA)
    rob = RR.solve_robust(pos, dq, sigma, src[:300], dst[:300], 4, ITERS, LAM, 2, LREG, 2, TUKEY_C, HUBER_DELTA)
    for g, w in zip(got[2], plane):
        assert np.array_equal(g, bits(w)), "solve_plane behind solve_rigid"
    for g, w in zip(got[3], rob):
        assert np.array_equal(g, bits(w)), "solve_robust behind solve_rigid"


def test_a_fresh_stream():
    pos, sigma, dq, src, dst, nrm = shared_problem(40)
    want = run_gpu(field(pos, sigma, dq), src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, HUBER_DELTA)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        wf = field(pos, sigma, dq)
        out = wf.solve_rigid(dev(src), dev(dst), dev(nrm), iters=ITERS, lam=LAM, lam_rot=LROT, reg_neighbours=4, reg_lambda=LREG, rounds=2,
                             tukey_c=TUKEY_C, huber_delta=HUBER_DELTA, return_weights=True)
        s.synchronize()
        got = [t.cpu().numpy() for t in out]
    torch.cuda.synchronize()
    assert_same(got, want, "a fresh stream against the default stream")


def test_with_brick_lists_and_without_an_index():
    """The k-NN and the warp of every round take the brick lists when the handle has an index: the same bits."""
    pos, sigma, dq, src, dst, nrm = shared_problem(1025)
    want = run_gpu(field(pos, sigma, dq), src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, HUBER_DELTA)
    wf = WarpField(k=8, voxel_table=False)
    wf.init(pos, sigma=sigma, transforms=dq)
    wf.ensure_index(index_volume(origin=(-1.0, -1.0, -1.0)), 8)
    assert_same(run_gpu(wf, src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, HUBER_DELTA), want, "brick lists against the scan")


def test_invalid_arguments():
    L = capi.lib()
    pos = random_nodes(5)
    wf = field(pos, np.full(5, 0.4, F32), k=4)
    pts = dev(np.random.default_rng(1).uniform(-1, 1, (64, 3)).astype(F32))
    nrm = dev(seeded_normals(64, marked=False))
    dq = torch.empty((5, 8), dtype=torch.float32, device="cuda"); en = torch.zeros(4, dtype=torch.float32, device="cuda")
    pw = torch.empty(64, dtype=torch.float32, device="cuda"); ew = torch.empty((5, 7), dtype=torch.float32, device="cuda")
    here = object()

    def call(kg=2, lreg=1.0, rounds=2, c=0.05, delta=0.01, k=4, n=64, iters=3, lam=0.0, lrot=0.0, edge=None, points=here, live=here, normals=here,
             handle=here):
        p = [pts.data_ptr() if a is here else a for a in (points, live)]
        return L.dfusion_warp_solve_rigid(wf.handle if handle is here else handle, k, p[0], p[1], nrm.data_ptr() if normals is here else normals, n,
                                          iters, lam, lrot, kg, lreg, rounds, c, delta, dq.data_ptr(), en.data_ptr(), pw.data_ptr(), edge, None)
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
    assert call(lrot=-1e-3) == DF_E_INVALID and call(lrot=nan) == DF_E_INVALID
    assert call() == 0 and call(normals=None) == 0 and call(kg=4, edge=ew.data_ptr()) == 0 and call(lrot=0.5) == 0
    assert call(kg=0, lreg=0.0, c=0.0, delta=0.0, rounds=1) == 0
    assert L.dfusion_warp_solve_rigid(wf.handle, 4, pts.data_ptr(), pts.data_ptr(), nrm.data_ptr(), 64, 3, 0.0, 0.0, 2, 1.0, 2, 0.05, 0.01, None,
                                      None, None, None, None) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the C++ mirror
def test_cxx_mirror_prints_the_restatements_bits():
    """host/apps/warp_solve.cpp rigid: the plane mode's seeded problem through WarpField::setNodeRotations + energy_data."""
    import subprocess
    from dynamicfusion_amd import build
    build.build_host()
    r = subprocess.run([build.HOST_WARP_SOLVE, "rigid"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [[int(w, 16) for w in line.split()] for line in r.stdout.strip().splitlines()]
    got_dq, got_en = np.array(lines[:-1], np.uint32), np.array(lines[-1], np.uint32)
    pos, dq, sigma, src, dst = lcg_problem()
    nrm = lcg_normals(len(src))
    want_dq, want_en, pw, ew = G.solve_rigid(pos, dq, sigma, src, dst, nrm, 8, 20, 1e-3, 0.01, 4, 1.0, 3, 0.02, 0.01)
    assert got_dq.shape == (50, 8)
    assert np.array_equal(got_dq, bits(want_dq)) and np.array_equal(got_en, bits(want_en))
    assert (bits(want_dq[:, :4]) != bits(dq.reshape(-1, 8)[:, :4])).any(1).sum() > 25      # the mirror's switch did switch: nodes turned
    plane, _ = field(pos, sigma, dq).solve_plane(dev(src), dev(dst), dev(nrm), iters=20, lam=1e-3, reg_neighbours=4, reg_lambda=1.0, rounds=3,
                                                 tukey_c=0.02, huber_delta=0.01)
    assert not np.array_equal(got_dq, bits(plane.cpu().numpy()))
