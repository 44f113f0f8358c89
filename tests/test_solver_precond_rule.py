"""The rule of the 6x6 node-block preconditioner of the warp solve with rotations, on the CPU: tests/solver_precond_ref.py
-- the numpy restatement the GPU is compared with bit for bit in tests/test_gpu_solver_precond.py -- builds the diagonal blocks of the
round's normal matrix, needs at most half of the plain recurrence's steps, ends at the same solution, gets further inside the frame
loop's budget of steps, and treats nodes it cannot factor as the rule says."""
import numpy as np

import oracle_lib as O
import solver_precond_ref as PC
import solver_rigid_ref as G
from dynamicfusion_amd import synth
from solver_cases import bits, random_problem
from test_solver_rigid_rule import CENTRE, DENSE, DENSE_MEASURED, TURN, cross_matrix, dense_rigid, planted_turn, turn_errors

F32 = np.float32


# ------------------------------------------------------------------------------------------------ (1) the blocks
def dense_matrix(d, M, lam, lam_rot, lreg, plane):
    """The float64 normal matrix and right-hand side of the first round as test_solver_rigid_rule.dense_rigid builds them (unknown
    3 i + c = omega_i, 3 M + 3 i + c = tau_i), from the restatement's own f32 quantities; `plane`: every point's three rows replaced by
    the one row n'^T J."""
    w, wn, keys, Gr = d["w"].astype(np.float64), d["wn"].astype(np.float64), d["keys"], d["graph"]
    a, q, e = d["a"][0].astype(np.float64), d["q"][0].astype(np.float64), d["e"][0].astype(np.float64)
    N, k = w.shape
    J = np.zeros((N, 3, 6 * M))
    rows = np.arange(N)
    ax, eye = cross_matrix(a), np.eye(3)
    for j in range(k):
        ok = keys[:, j] < M
        n = np.where(ok, keys[:, j], 0)
        om = np.where(ok[:, None, None], w[:, j, None, None] * cross_matrix(q[n]) - wn[:, j, None, None] * ax, 0.0)
        tau = np.where(ok[:, None, None], w[:, j, None, None] * eye, 0.0)
        for r in range(3):
            for c in range(3):
                J[rows, r, 3 * n + c] += om[:, r, c]
                J[rows, r, 3 * M + 3 * n + c] += tau[:, r, c]
    if plane:
        nw = d["nw"][0].astype(np.float64)
        J = np.einsum("vr,vrc->vc", nw, J)
        e = (nw * e).sum(1)
    J = J.reshape(-1, 6 * M)
    A = J.T @ J + np.diag(np.r_[np.full(3 * M, lam_rot), np.full(3 * M, lam)])
    rhs = J.T @ e.reshape(-1)
    alpha, head, tail = Gr.alpha.reshape(-1).astype(np.float64), Gr.nbr.reshape(-1), Gr.tail
    b, g = d["b"][0].astype(np.float64), d["g"][0].astype(np.float64)
    bx = cross_matrix(b)
    D = np.zeros((len(head), 3, 6 * M))
    for ed in range(len(head)):
        i, j = tail[ed], head[ed]
        D[ed][:, 3 * M + 3 * i:3 * M + 3 * i + 3] += eye
        D[ed][:, 3 * M + 3 * j:3 * M + 3 * j + 3] -= eye
        D[ed][:, 3 * i:3 * i + 3] -= bx[ed]
    A += lreg * np.einsum("e,erc,erd->cd", alpha, D, D)
    rhs -= lreg * np.einsum("e,erc,er->c", alpha, D, g)
    return A, rhs


def diagonal_blocks(A, M):
    """[M, 6, 6]: rows and columns (omega_n, tau_n) of A for every node n."""
    out = np.empty((M, 6, 6))
    for n in range(M):
        ix = np.r_[3 * n:3 * n + 3, 3 * M + 3 * n:3 * M + 3 * n + 3]
        out[n] = A[np.ix_(ix, ix)]
    return out


def test_blocks_are_the_diagonal_blocks_of_the_dense_matrix():
    """The off-centre planted turn at the TURN setting.  Point-to-point: the restatement's f32 blocks against the diagonal blocks of the
    float64 matrix, whose solution is checked to be dense_rigid's; then the plane form against the matrix with rows n'^T J.  Bound: 1e-4 x
    the block's largest entry (a list has at most 1500 entries, so n 2^-24 sum|terms| stays under it)."""
    pos, dq, sigma, src, live, normals, _ = planted_turn()
    M = len(pos)
    lam, lrot, lreg = float(F32(TURN["lam"])), float(F32(TURN["lam_rot"])), TURN["lreg"]
    for nrm in (None, normals):
        d = {}
        PC.solve_rigid(pos, dq, sigma, src, live, nrm, 8, 0, TURN["lam"], TURN["lam_rot"], TURN["kg"], lreg, 1, details=d)
        A, rhs = dense_matrix(d, M, lam, lrot, lreg, nrm is not None)
        if nrm is None:
            want = dense_rigid(d, M, lam, lrot, lreg)
            assert np.abs(np.linalg.solve(A, rhs).reshape(2 * M, 3) - want).max() <= 1e-9 * np.abs(want).max()
        want = diagonal_blocks(A, M)
        got = PC.full_blocks(d["blocks"][0].astype(np.float64))
        rel = np.abs(got - want).max((1, 2)) / np.abs(want).max((1, 2))
        print("%s: largest |block - dense| / largest entry = %.3g; factored %d of %d" % (
            "point-to-plane" if nrm is not None else "point-to-point", rel.max(), d["factored"][0].sum(), M))
        assert rel.max() <= 1e-4
        assert d["factored"][0].all()
        Lo, _ = PC.cholesky(d["blocks"][0])                             # and the factor is the block's: L L^T = B
        back = np.einsum("nik,njk->nij", Lo.astype(np.float64), Lo.astype(np.float64))
        assert (np.abs(back - got).max((1, 2)) <= 1e-5 * np.abs(got).max((1, 2))).all()


# ------------------------------------------------------------------------------------------------ (2) fewer steps
# measured on the CPU (x86-64, glibc exp) with the restatements: (plain steps, preconditioned steps) of one round, point-to-point
STEPS_MEASURED_TURN = (505, 73)
STEPS_MEASURED_RANDOM = (407, 72)


def steps_of(problem, setting, iters):
    pos, dq, sigma, src, live = problem
    plain, pre = {}, {}
    G.solve_rigid(pos, dq, sigma, src, live, None, 8, iters, *setting, 1, details=plain)
    PC.solve_rigid(pos, dq, sigma, src, live, None, 8, iters, *setting, 1, details=pre)
    return plain["steps"][0], pre["steps"][0]


def test_the_planted_turn_needs_at_most_half_the_steps():
    """One round on the off-centre planted turn, TURN setting, neither recurrence cut off.  Measured: STEPS_MEASURED_TURN."""
    plain, pre = steps_of(planted_turn()[:5], (TURN["lam"], TURN["lam_rot"], TURN["kg"], TURN["lreg"]), 1500)
    print("planted turn: plain %d steps, node blocks %d steps, ratio %.2f" % (plain, pre, plain / pre))
    assert 0 < plain < 1500 and 0 < pre < 1500
    assert 2 * pre <= plain


def test_a_random_problem_needs_at_most_half_the_steps():
    """random_problem(150, 3001, nans=False), kg 4, lambda 1e-3, lambda_rot 1e-2.  Measured: STEPS_MEASURED_RANDOM."""
    plain, pre = steps_of(random_problem(150, 3001, nans=False), (1e-3, 1e-2, 4, 1.0), 1500)
    print("random problem: plain %d steps, node blocks %d steps, ratio %.2f" % (plain, pre, plain / pre))
    assert 0 < plain < 1500 and 0 < pre < 1500
    assert 2 * pre <= plain


# ------------------------------------------------------------------------------------------------ (3) the same solution
DENSE_MEASURED_PRECOND = 3.68e-5                         # largest |X - dense|, one converged round with the node blocks, measured on the CPU


def test_converged_round_meets_the_dense_normal_equations():
    """test_solver_rigid_rule's dense comparison with the blocks on: the bound is the plain solve's, 4 x its DENSE_MEASURED."""
    pos, dq, sigma, src, live, _, _ = planted_turn()
    d = {}
    PC.solve_rigid(pos, dq, sigma, src, live, None, 8, 400, DENSE["lam"], DENSE["lam_rot"], 4, DENSE["lreg"], 1, details=d)
    want = dense_rigid(d, len(pos), float(F32(DENSE["lam"])), float(F32(DENSE["lam_rot"])), DENSE["lreg"])
    err = float(np.abs(d["x"][0].astype(np.float64) - want).max())
    print("dense solve with node blocks: max |X - dense| = %.3g, steps %s" % (err, d["steps"]))
    assert d["steps"][0] < 400
    assert err <= 4 * DENSE_MEASURED                     # (measured: DENSE_MEASURED_PRECOND)


# ------------------------------------------------------------------------------------------------ (4) inside the frame loop's budget
# (largest |y - live| in metres, largest normal angle in degrees) after 3 rounds of 40 steps on the centred turn, measured on the CPU
BUDGET_MEASURED_PLAIN = (1.17e-2, 4.64)
BUDGET_MEASURED_PRECOND = (1.23e-6, 4.98e-4)


def test_the_planted_turn_inside_the_frame_loops_budget():
    """40 steps a round and 3 rounds, KinFuParams' budget, on the turn about the sphere's centre (which the field can hold exactly: what
    is left is the solver's error).  Measured: BUDGET_MEASURED_PLAIN and BUDGET_MEASURED_PRECOND; asserted: the blocks leave less of
    both."""
    pos, dq, sigma, src, live, normals, true_normals = planted_turn(CENTRE)
    out = {}
    for mode in (0, 1):
        d = {}
        r_dq, en, _, _ = PC.solve_rigid(pos, dq, sigma, src, live, None, 8, 40, TURN["lam"], TURN["lam_rot"], TURN["kg"], TURN["lreg"], 3, details=d,
                                        precond=mode)
        out[mode] = turn_errors(pos, r_dq, sigma, src, live, normals, true_normals)
        print("3 rounds of 40 steps, preconditioner %d: |y - live| %.3g m, normal %.3g deg, energies %s, steps %s" % ((mode,) + out[mode] + (en, d["steps"])))
    assert out[1][0] < out[0][0] and out[1][1] < out[0][1]


# ------------------------------------------------------------------------------------------------ (5) degenerate nodes
def test_a_node_without_entries_and_edges_under_zero_damping_takes_the_identity():
    pos, dq, sigma, src, dst = random_problem(100, 2000)
    pos = pos.copy(); pos[37] = F32([30, 30, 30])                       # no point has it among its 8 nearest
    d = {}
    out, en, _, _ = PC.solve_rigid(pos, dq, sigma, src, dst, None, 8, 12, 0.0, 0.0, 0, 0.0, 2, details=d)
    assert not (d["keys"] == 37).any()
    for rnd in range(2):
        assert not d["blocks"][rnd][37].any()                           # an empty block: its first pivot is 0
        assert not d["factored"][rnd][37] and d["factored"][rnd].sum() == len(pos) - 1
    assert np.array_equal(bits(out[37]), bits(dq.reshape(-1, 8)[37]))
    assert (bits(out) != bits(dq.reshape(-1, 8))).any(1).sum() == len(pos) - 1
    assert np.isfinite(out).all() and en[1] < en[0]


def test_a_nan_or_a_rank_deficient_block_gives_the_identity_for_that_node_only():
    pos, dq, sigma, src, dst = random_problem(40, 600, nans=False)
    d = {}
    PC.solve_rigid(pos, dq, sigma, src, dst, None, 8, 0, 1e-3, 1e-3, 4, 1.0, 1, details=d)
    B = d["blocks"][0].copy()
    B[5, PC.up(1, 4)] = np.nan                                          # a NaN off the diagonal
    B[9, PC.up(3, 3)] = np.inf                                          # an infinite pivot
    B[11] = 0
    for i in (3, 4, 5):
        B[11, PC.up(i, i)] = 1                                          # translations alone: the rotation block has rank 0
    fac = PC.cholesky(B)
    assert (np.flatnonzero(~fac[1]) == [5, 9, 11]).all()
    r = np.random.default_rng(3).normal(0, 1, (80, 3)).astype(F32)
    z = PC.apply(fac, r)
    assert np.isfinite(z).all()
    for n in (5, 9, 11):
        assert np.array_equal(bits(z[n]), bits(r[n])) and np.array_equal(bits(z[40 + n]), bits(r[40 + n]))
    good = np.flatnonzero(fac[1])
    full = PC.full_blocks(B.astype(np.float64))
    r6 = np.concatenate([r[:40], r[40:]], 1).astype(np.float64)
    z6 = np.concatenate([z[:40], z[40:]], 1).astype(np.float64)
    for n in good:                                                      # and elsewhere z is the block's solve
        assert np.abs(full[n] @ z6[n] - r6[n]).max() <= 1e-3 * np.abs(r6[n]).max()


def test_a_field_that_explains_the_live_points_is_left_alone():
    """live = warp(canonical) exactly: r0 = 0, so z0 = 0 and r.z = 0: the recurrence never starts and every node keeps its eight floats."""
    pos, dq, sigma, src, _ = random_problem(100, 2000, nans=False)
    normals = np.random.default_rng(8).normal(0, 1, src.shape).astype(F32)
    for transforms, kg in ((dq, 0), (synth.identity_dq(len(pos)), 4)):
        live, _ = O.warp_points(pos, transforms, sigma, src, None, 8)
        for nrm in (None, normals):
            d = {}
            out, en, _, _ = PC.solve_rigid(pos, transforms, sigma, src, live, nrm, 8, 25, 1e-3, 1e-3, kg, 1.0, 2, details=d)
            assert d["steps"] == [0, 0] and not d["r0"][0].any() and not d["r0"][1].any()
            assert np.array_equal(bits(out), bits(transforms))
            assert bits(en[0]) == bits(en[1]) and bits(en[2]) == bits(en[3]) and en[0] == 0


def test_mode_zero_is_the_plain_restatement():
    pos, dq, sigma, src, dst = random_problem(40, 600)
    a = PC.solve_rigid(pos, dq, sigma, src, dst, None, 8, 6, 1e-3, 1e-2, 4, 1.0, 2, 0.05, 0.03, precond=0)
    b = G.solve_rigid(pos, dq, sigma, src, dst, None, 8, 6, 1e-3, 1e-2, 4, 1.0, 2, 0.05, 0.03)
    c = PC.solve_rigid(pos, dq, sigma, src, dst, None, 8, 6, 1e-3, 1e-2, 4, 1.0, 2, 0.05, 0.03)
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y))
    assert not np.array_equal(bits(c[0]), bits(b[0]))
