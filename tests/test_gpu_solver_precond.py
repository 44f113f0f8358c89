"""GPU parity of the warp solve with rotations under the 6x6 node-block preconditioner (dfusion_warp_set_preconditioner)
against the numpy restatement tests/solver_precond_ref.py, which tests/test_solver_precond_rule.py checks on the CPU: the transforms, the
four energies and the last round's point and edge weights bit for bit at every node count where the preconditioned step kernel changes
its variant (2 M <= 2, 5, 8 x 1024 and beyond) and at M = k, over the penalty settings, graph on and off, one round and three, with
normals and without, on the planted cap and over the node hierarchy; the setting changes the solve and lowers the energy the frame
loop's budget reaches; off is off, bit for bit, and the translation-only solves never see it; the setting survives extend; the
argument checks.

The grid is a covering design: every M meets kg = 0 and 4, and both data terms, round counts and all penalty settings occur at the
register-resident variants and at the general one."""
import ctypes

import numpy as np
import pytest
import torch

import solver_hier_ref as H
import solver_precond_ref as PC
from dynamicfusion_amd import capi
from solver_cases import DF_E_INVALID, HUBER_DELTA, ITERS, LAM, LREG, LROT, MODES, TUKEY_C, assert_same, bits, dev, field, random_nodes
from solver_cases import shared_plane_problem as shared_problem
from test_solver_rigid_rule import TURN, planted_turn

pytestmark = pytest.mark.gpu
F32 = np.float32


def run_gpu(wf, src, dst, nrm, k, kg, lreg, rounds, c, delta, iters=ITERS, lam=LAM, lrot=LROT):
    out = wf.solve_rigid(dev(src), dev(dst), None if nrm is None else dev(nrm), iters=iters, lam=lam, lam_rot=lrot, reg_neighbours=kg,
                         reg_lambda=lreg, rounds=rounds, tukey_c=c, huber_delta=delta, k=k, return_weights=True)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in out]


def restated(pos, dq, sigma, src, dst, nrm, k, kg, lreg, rounds, c, delta, iters=ITERS, lam=LAM, lrot=LROT, details=None, precond=1):
    return PC.solve_rigid(pos, dq, sigma, src, dst, nrm, k, iters, lam, lrot, kg, lreg, rounds, c, delta, details=details, precond=precond)


def pc_field(pos, sigma, dq, k=8):
    wf = field(pos, sigma, dq, k)
    wf.set_preconditioner(1)
    assert wf.preconditioner == 1
    return wf


GRID = [
    # M,    k, kg, rounds, mode, normals     the preconditioned step, by nodes
    (8,     8, 4, 3, "both", True),        # M = k: every list holds every valid point, about 3000 entries (the thread stride wraps)
    (8,     8, 0, 1, "tukey", False),
    (257,   8, 4, 1, "huber", False),      # one node a thread, two workgroups of nodes in the graph kernels
    (257,   4, 0, 3, "off", True),
    (1024,  8, 4, 3, "off", False),        # the last M with one node a thread
    (1024,  8, 0, 1, "tukey", True),
    (1025,  4, 4, 1, "both", True),        # three nodes a thread
    (1025,  8, 0, 3, "off", False),
    (2560,  8, 4, 1, "tukey", True),       # the last M with three
    (2560,  3, 0, 3, "tukey", False),
    (2561,  8, 4, 3, "huber", True),       # four nodes a thread
    (2561,  8, 0, 1, "off", False),
    (4096,  8, 4, 1, "off", True),         # the last M with four
    (4096,  4, 0, 3, "tukey", False),
    (4097,  8, 4, 3, "both", False),       # the general kernel; many lists shorter than a wave, some empty
    (4097,  8, 0, 1, "off", True),
]


@pytest.mark.parametrize("M,k,kg,rounds,mode,normals", GRID, ids=["M%d-k%d-kg%d-r%d-%s-%s" % (c[:5] + ("plane" if c[5] else "point",)) for c in GRID])
def test_matches_the_restatement_bit_for_bit(M, k, kg, rounds, mode, normals):
    pos, sigma, dq, src, dst, nrm = shared_problem(M)
    nrm = nrm if normals else None
    c, delta = MODES[mode]
    wf = pc_field(pos, sigma, dq, k)
    got = run_gpu(wf, src, dst, nrm, k, kg, LREG, rounds, c, delta)
    d = {}
    want = restated(pos, dq, sigma, src, dst, nrm, k, kg, LREG, rounds, c, delta, details=d)
    lens = np.bincount(d["lists"].node, minlength=M)
    print("M %d k %d kg %d rounds %d %s normals %s: energies gpu %s restatement %s; steps %s; lists %d .. %d entries, %d empty; factored %s" % (
        M, k, kg, rounds, mode, normals, got[1], want[1], d["steps"], lens.min(), lens.max(), int((lens == 0).sum()), [int(f.sum()) for f in d["factored"]]))
    assert all(s > 0 for s in d["steps"]) and all(x[:M].any() and x[M:].any() for x in d["x"])
    assert all(f.sum() > M // 2 for f in d["factored"])                 # the blocks are in use
    if M == 8:
        assert lens.min() > 2560                                         # more than ten trips of the thread stride
    if M == 4097:
        assert (lens < 64).sum() > 1000
    assert_same(got, want, "gpu against the restatement")
    assert np.array_equal(bits(wf._dq.cpu().numpy()), bits(want[0]))
    plain = PC.G.solve_rigid(pos, dq, sigma, src, dst, nrm, k, ITERS, LAM, LROT, kg, LREG, rounds, c, delta) if M <= 257 else None
    if plain is not None:                                                # and they are not the plain solve's bits
        assert not np.array_equal(bits(plain[0]), bits(want[0]))


@pytest.mark.parametrize("normals", [False, True], ids=["point", "plane"])
def test_the_planted_cap(normals):
    """The off-centre planted turn (M 60, N 1500) at the TURN setting with the frame loop's 40 steps and 3 rounds."""
    pos, dq, sigma, src, live, nrm, _ = planted_turn()
    nrm = nrm if normals else None
    args = (8, TURN["kg"], TURN["lreg"], 3, 0.0, 0.0)
    kw = dict(iters=40, lam=TURN["lam"], lrot=TURN["lam_rot"])
    got = run_gpu(pc_field(pos, sigma, dq), src, live, nrm, *args, **kw)
    d = {}
    want = restated(pos, dq, sigma, src, live, nrm, *args, details=d, **kw)
    print("planted cap, normals %s: energies %s, steps %s" % (normals, want[1], d["steps"]))
    assert_same(got, want, "planted cap")


def test_over_the_node_hierarchy():
    pos, sigma, dq, src, dst, nrm = shared_problem(257)
    setting = (2, 0.5, 2.0)
    wf = pc_field(pos, sigma, dq)
    wf.set_graph_hierarchy(*setting)
    got = run_gpu(wf, src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, HUBER_DELTA)
    with H.hierarchy(*setting):
        want = restated(pos, dq, sigma, src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, HUBER_DELTA)
    flat = restated(pos, dq, sigma, src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, HUBER_DELTA)
    assert H.levels(pos, 4, *setting)[3] >= 1 and not np.array_equal(bits(flat[0]), bits(want[0]))
    assert_same(got, want, "over the hierarchy")


def test_convergence_before_the_steps_run_out():
    """400 steps asked for: the recurrence freezes on r.z <= 1e-10 (r.z)_0 long before, the kernels of the remaining steps return at once."""
    pos, sigma, dq, src, dst, nrm = shared_problem(257)
    d = {}
    want = restated(pos, dq, sigma, src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, 0.0, iters=400, lam=1e-2, lrot=1e-1, details=d)
    print("steps taken per round:", d["steps"])
    assert all(0 < s < 400 for s in d["steps"])
    got = run_gpu(pc_field(pos, sigma, dq), src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, 0.0, iters=400, lam=1e-2, lrot=1e-1)
    assert_same(got, want, "early out")


def test_a_node_without_entries_and_edges_under_zero_damping():
    """Its block is empty, its first pivot 0: the identity, and the node keeps its eight floats."""
    pos, sigma, dq, src, dst, _ = shared_problem(257)
    pos = pos.copy(); pos[37] = F32([30, 30, 30])
    got = run_gpu(pc_field(pos, sigma, dq), src, dst, None, 8, 0, 0.0, 2, 0.0, 0.0, lam=0.0, lrot=0.0)
    d = {}
    want = restated(pos, dq, sigma, src, dst, None, 8, 0, 0.0, 2, 0.0, 0.0, lam=0.0, lrot=0.0, details=d)
    assert not d["factored"][0][37] and d["factored"][0].sum() == 256
    assert_same(got, want, "an unconstrained node")
    assert np.array_equal(bits(got[0][37]), bits(dq[37]))


def test_the_setting_changes_the_solve_and_reaches_a_lower_energy():
    """The planted turn with the frame loop's budget, 40 steps and 3 rounds, on the same inputs: mode 1 gives other transforms than
    mode 0 and a lower E_data after the solve."""
    pos, dq, sigma, src, live, _, _ = planted_turn()
    args = (8, TURN["kg"], TURN["lreg"], 3, 0.0, 0.0)
    kw = dict(iters=40, lam=TURN["lam"], lrot=TURN["lam_rot"])
    plain = run_gpu(field(pos, sigma, dq), src, live, None, *args, **kw)
    wf = field(pos, sigma, dq)
    assert wf.preconditioner == 0
    wf.set_preconditioner(1)
    pre = run_gpu(wf, src, live, None, *args, **kw)
    print("E_data before / after: plain %s, node blocks %s" % (plain[1][:2], pre[1][:2]))
    assert not np.array_equal(bits(plain[0]), bits(pre[0]))
    assert bits(plain[1][0]) == bits(pre[1][0])
    assert pre[1][1] < plain[1][1] < plain[1][0]


def test_off_means_off():
    """Switched on and off again: the bits of a handle that never had the setting.  And with the setting on, solve, solve_robust and
    solve_plane return what they return without it."""
    pos, sigma, dq, src, dst, nrm = shared_problem(257)
    never = run_gpu(field(pos, sigma, dq), src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, HUBER_DELTA)
    wf = pc_field(pos, sigma, dq)
    on = run_gpu(wf, src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, HUBER_DELTA)
    wf.set_preconditioner(0)
    assert wf.preconditioner == 0
    wf.set_transforms(dev(dq))
    off = run_gpu(wf, src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, HUBER_DELTA)
    assert_same(off, never, "on, then off")
    assert not np.array_equal(bits(on[0]), bits(never[0]))
    assert_same(never, restated(pos, dq, sigma, src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, HUBER_DELTA, precond=0), "mode 0 against the plain restatement")
    kw = dict(iters=ITERS, lam=LAM, reg_neighbours=4, reg_lambda=LREG)
    rob = dict(rounds=2, tukey_c=TUKEY_C, huber_delta=HUBER_DELTA, return_weights=True)
    calls = [lambda w: w.solve(dev(src), dev(dst), **kw), lambda w: w.solve_robust(dev(src), dev(dst), **kw, **rob),
             lambda w: w.solve_plane(dev(src), dev(dst), dev(nrm), **kw, **rob)]
    for i, call in enumerate(calls):
        a, b = call(field(pos, sigma, dq)), call(pc_field(pos, sigma, dq))
        torch.cuda.synchronize()
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert np.array_equal(bits(x.cpu().numpy()), bits(y.cpu().numpy())), "translation-only solve %d under mode 1" % i


def test_the_setting_survives_extend_and_set_nodes():
    rng = np.random.default_rng(31)
    pos = rng.uniform(-0.5, 0.5, (120, 3)).astype(F32)
    _, sigma, dq, src, dst, nrm = shared_problem(257)
    sigma, dq = np.full(120, 0.15, F32), dq[:120]
    wf = pc_field(pos, sigma, dq)
    n_added, _ = wf.extend(dev(rng.uniform(-1, 1, (4000, 3)).astype(F32)), 0.3, sigma=0.15)
    torch.cuda.synchronize()
    assert n_added > 10 and wf.preconditioner == 1
    gpos, gdq, gsig = (t.cpu().numpy() for t in wf._keep)
    gpos, gdq, gsig = gpos.reshape(-1, 3), gdq.reshape(-1, 8), gsig.reshape(-1)
    got = run_gpu(wf, src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, HUBER_DELTA)
    d = {}
    want = restated(gpos, gdq, gsig, src, dst, nrm, 8, 4, LREG, 2, TUKEY_C, HUBER_DELTA, details=d)
    assert len(gpos) == 120 + n_added and all(s > 0 for s in d["steps"])
    assert_same(got, want, "after extend")
    wf.init(pos, sigma=sigma, transforms=dq)                            # new nodes on the same handle
    wf.set_transforms(dev(dq))
    assert wf.preconditioner == 1


def test_invalid_arguments():
    L = capi.lib()
    wf = field(random_nodes(40), np.full(40, 0.4, F32))
    mode = ctypes.c_int(-7)
    for bad in (-1, 2, 3, 1 << 20):
        assert L.dfusion_warp_set_preconditioner(wf.handle, bad) == DF_E_INVALID
    assert L.dfusion_warp_set_preconditioner(None, 1) == DF_E_INVALID and L.dfusion_warp_set_preconditioner(None, 0) == DF_E_INVALID
    assert L.dfusion_warp_preconditioner(None, ctypes.byref(mode)) == DF_E_INVALID and L.dfusion_warp_preconditioner(wf.handle, None) == DF_E_INVALID
    assert mode.value == -7
    assert L.dfusion_warp_preconditioner(wf.handle, ctypes.byref(mode)) == 0 and mode.value == 0        # the refused calls changed nothing
    assert L.dfusion_warp_set_preconditioner(wf.handle, 1) == 0
    assert L.dfusion_warp_set_preconditioner(wf.handle, 2) == DF_E_INVALID
    assert L.dfusion_warp_preconditioner(wf.handle, ctypes.byref(mode)) == 0 and mode.value == 1
    with pytest.raises(Exception):
        wf.set_preconditioner(-1)
    assert wf.preconditioner == 1
