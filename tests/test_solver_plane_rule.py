"""The rule of the point-to-plane warp solve, on the CPU: tests/solver_plane_ref.py -- the numpy restatement the GPU is
compared with bit for bit in tests/test_gpu_solver_plane.py -- gives the point-to-point restatement's x translations when every normal is
(1, 0, 0), ignores a planted tangential slip that the point-to-point solve turns into node motion, meets a dense float64 solve of its own
normal equations (one round, and three re-weighted rounds with Tukey on), and treats NaN, infinite and zero normals as the rule says."""
import numpy as np

import associate_loop as AL
import nonrigid_loop as NL
import plane_loop as PL
import solver_plane_ref as P
import solver_reg_ref as R
from solver_cases import bits, planted_slip, random_problem

F32 = np.float32


# ------------------------------------------------------------------------------------------------ (1) degenerate normals
def test_normals_along_x_give_the_point_to_point_x_translations():
    """n = (1, 0, 0): rho = e0x, b = (rho, 0, 0), the y and z parts of every CG vector stay 0 and add nothing to a dot product, so the one
    coupled recurrence is the point-to-point solve's x recurrence."""
    pos, dq, sigma, src, dst = random_problem(100, 2000)
    normals = np.tile(F32([1, 0, 0]), (len(src), 1))
    dr, d = {}, {}
    R.solve(pos, dq, sigma, src, dst, 8, 25, 1e-3, kg=0, details=dr)
    got_dq, got_en, pw, ew = P.solve_plane(pos, dq, sigma, src, dst, normals, 8, 25, 1e-3, details=d)
    x = d["x"][0]                                                        # (the translation updates themselves: a decoded transform mixes
    assert np.abs(x[:, 0]).max() > 1e-3                                  # the components through the node's rotation)
    assert np.array_equal(x[:, 0], dr["x"][:, 0])
    assert not x[:, 1:].any()
    assert np.array_equal(got_dq[:, :4], dq.reshape(-1, 8)[:, :4])
    e0x = d["e0"][0][:, :1]
    assert bits(got_en[0]) == bits(R.strided_sum1024(e0x * e0x)[0])
    assert got_en[1] < got_en[0] and (pw == 1).all() and ew is None


# ------------------------------------------------------------------------------------------------ (2) the planted slip
LAM = 1e-3


def tangential(v, n):
    n = n.astype(np.float64)
    return v - (v * n).sum(1, keepdims=True) * n


def slip_errors(dq_out, w, keys, planted, blend, normals):
    """(largest node error against the planted field, largest tangential point error |W x - blend| perpendicular to n), float64."""
    x = R.node_translation(dq_out)[:, 1:].astype(np.float64)             # identity start: T = delta
    wx = np.einsum("nk,nkc->nc", w.astype(np.float64), x[keys])
    return float(np.abs(x - planted).max()), float(np.linalg.norm(tangential(wx - blend, normals), axis=1).max())


# measured on the CPU (x86-64, glibc exp) with the restatements, 400 steps, lam = 1e-3: {kg, lambda_reg: (largest node error of the
# plane solve, of the point-to-point solve, largest tangential point error of the plane solve, of the point-to-point solve)}, metres
SLIP_MEASURED = {
    (0, 0.0): (7.22e-5, 2.91e-3, 7.84e-5, 1.11e-2),
    (4, 0.01): (5.43e-5, 2.90e-3, 8.10e-5, 1.11e-2),
}


def run_slip(kg, lreg):
    pos, dq, sigma, src, live, normals, planted, blend = planted_slip()
    d = {}
    p_dq, p_en, _, _ = P.solve_plane(pos, dq, sigma, src, live, normals, 8, 400, LAM, kg, lreg, details=d)
    q_dq, q_en = R.solve(pos, dq, sigma, src, live, 8, 400, LAM, kg, lreg)
    args = (d["w"], d["keys"], planted, blend, normals)
    return slip_errors(p_dq, *args), slip_errors(q_dq, *args), p_en, q_en, d


def check_slip(kg, lreg):
    (pn, pt), (qn, qt), p_en, q_en, d = run_slip(kg, lreg)
    print("planted slip kg %d lambda_reg %g: node error plane %.3g point-to-point %.3g; tangential point error plane %.3g "
          "point-to-point %.3g; energies plane %s point-to-point %s; steps %s" % (kg, lreg, pn, qn, pt, qt, p_en, q_en, d["steps"]))
    m_pn, m_qn, m_pt, m_qt = SLIP_MEASURED[(kg, lreg)]
    assert p_en[1] < p_en[0]
    assert pn <= 4 * m_pn and pt <= 4 * m_pt                            # the margin DESIGN.md 12 uses for float32 conjugate gradients
    assert qn >= m_qn / 4 and qt >= m_qt / 4
    assert pn <= qn / 10 and pt <= qt / 10                              # the condition: the slip does not reach the nodes


def test_planted_slip_does_not_move_the_nodes():
    """The data-only solve.  Measured: SLIP_MEASURED[(0, 0.0)]."""
    check_slip(0, 0.0)


def test_planted_slip_does_not_move_the_nodes_with_regularisation():
    """kg = 4, lambda_reg = 0.01.  Measured: SLIP_MEASURED[(4, 0.01)]."""
    check_slip(4, 0.01)


# ------------------------------------------------------------------------------------------------ (3) dense float64
def dense_plane(d, M, lam, lreg, rounds, c):
    """The same rounds in float64 on the dense 3M x 3M normal matrix: the row of point v is J_v = n_v^T (w_v1 I .. w_vk I) at its nodes'
    columns; A = J^T Omega J + lam I + lreg (L x I3), rhs = J^T Omega rho - lreg b; numpy.linalg.solve.  From the restatement's own f32
    w, alpha, normals and first e0 and g (the rotations are fixed, so a round's g is the first g moved by the translations so far);
    the Tukey weights from the float64 rho."""
    w, keys, G, n = d["w"].astype(np.float64), d["keys"], d["graph"], d["normals"].astype(np.float64)
    e_first, g_first = d["e0"][0].astype(np.float64), d["g"][0].astype(np.float64)
    N, k = w.shape
    W = np.zeros((N, M))
    for j in range(k):
        ok = keys[:, j] < M
        np.add.at(W, (np.flatnonzero(ok), keys[ok, j]), w[ok, j])
    J = (W[:, :, None] * n[:, None, :]).reshape(N, 3 * M)               # column 3 i + c
    alpha, head, tail = G.alpha.reshape(-1).astype(np.float64), G.nbr.reshape(-1), G.tail
    Lg = np.zeros((M, M))
    for ed in range(len(head)):
        i, j, a = tail[ed], head[ed], alpha[ed]
        Lg[i, i] += a; Lg[j, j] += a; Lg[i, j] -= a; Lg[j, i] -= a
    total = np.zeros((M, 3))
    for _ in range(rounds):
        rho = ((e_first - W @ total) * n).sum(1)
        s = rho * rho
        om = np.where(s < c * c, (1 - s / (c * c)) ** 2, 0.0) if c else np.ones(N)
        g = g_first + total[tail] - total[head]
        A = J.T @ (om[:, None] * J) + lam * np.eye(3 * M) + lreg * np.kron(Lg, np.eye(3))
        breg = np.zeros((M, 3))
        np.add.at(breg, tail, alpha[:, None] * g); np.add.at(breg, head, -alpha[:, None] * g)
        rhs = J.T @ (om * rho) - lreg * breg.reshape(-1)
        total = total + np.linalg.solve(A, rhs).reshape(M, 3)
    return total


TUKEY_C_DENSE = 0.012
DENSE_MEASURED = 4.51e-6       # largest |delta - dense|, one quadratic round of 400 steps, measured on the CPU (see the docstring below)
DENSE_IRLS_MEASURED = 2.99e-8     # the same over 3 rounds with Tukey on


def test_converged_solve_meets_the_dense_normal_equations():
    """The planted slip with kg = 4, lambda_reg = 1, 400 steps, against the 180 x 180 float64 system.
    Measured on the CPU (x86-64, glibc exp): largest |delta - dense| = DENSE_MEASURED; asserted: 4 x that."""
    pos, dq, sigma, src, live, normals, planted, _ = planted_slip()
    d = {}
    r_dq, _, _, _ = P.solve_plane(pos, dq, sigma, src, live, normals, 8, 400, LAM, 4, 1.0, details=d)
    want = dense_plane(d, len(pos), float(F32(LAM)), 1.0, 1, 0.0)
    err = float(np.abs(d["x"][0].astype(np.float64) - want).max())
    print("dense solve: max |delta - dense| = %.3g, max |delta| = %.3g, steps %s" % (err, np.abs(want).max(), d["steps"]))
    assert np.abs(want).max() > 1e-3
    assert err <= 4 * DENSE_MEASURED


def test_converged_rounds_meet_a_dense_float64_irls():
    """The same with 3 rounds and tukey_c = 1.2 cm, which puts part of the points' rho (up to 9.9 mm) into the weight's slope and none
    past it.  Measured on the CPU: largest |accumulated delta - dense| = DENSE_IRLS_MEASURED; asserted: 4 x that."""
    pos, dq, sigma, src, live, normals, planted, _ = planted_slip()
    d = {}
    r_dq, _, pw, _ = P.solve_plane(pos, dq, sigma, src, live, normals, 8, 400, LAM, 4, 1.0, 3, TUKEY_C_DENSE, 0.0, details=d)
    want = dense_plane(d, len(pos), float(F32(LAM)), 1.0, 3, float(F32(TUKEY_C_DENSE)))
    got = R.node_translation(r_dq)[:, 1:].astype(np.float64)             # (the field starts at the identity: T = the accumulated delta)
    err = float(np.abs(got - want).max())
    first = d["omega"][0]
    print("dense IRLS: max |delta - dense| = %.3g, max |delta| = %.3g; first round's weights in (0, 1): %d, smallest %.3g" % (
        err, np.abs(want).max(), int(((first > 0) & (first < 1)).sum()), first.min()))
    assert ((first > 0) & (first < 1)).any()
    assert np.abs(want).max() > 1e-3
    assert err <= 4 * DENSE_IRLS_MEASURED


# ------------------------------------------------------------------------------------------------ (4) NaN, infinite and zero normals
def test_nan_and_infinite_normals_skip_the_point_and_a_zero_normal_changes_nothing():
    pos, dq, sigma, src, dst = random_problem(100, 2000)
    rng = np.random.default_rng(4)
    normals = rng.normal(0, 1, (len(src), 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(F32)
    ok = np.isfinite(src).all(1) & np.isfinite(dst).all(1)
    bad = np.flatnonzero(ok)[[3, 40, 500, 900]]
    zero = np.flatnonzero(ok)[[7, 300]]
    marked = normals.copy()
    marked[bad[0], 0] = np.nan; marked[bad[1], 2] = np.inf; marked[bad[2], 1] = -np.inf; marked[bad[3]] = np.nan
    marked[zero] = 0
    d = {}
    got = P.solve_plane(pos, dq, sigma, src, dst, marked, 8, 12, 1e-3, 4, 1.0, 2, 0.05, 0.0, details=d)
    assert (d["keys"][bad] == len(pos)).all() and not d["w"][bad].any() and not d["e0"][0][bad].any()
    assert (d["keys"][zero] < len(pos)).all() and d["w"][zero].any() and d["e0"][0][zero].any() and not d["rho"][0][zero].any()
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    # the same solve with those points taken out by the older rule (a NaN live point) ...
    dst2 = dst.copy(); dst2[bad] = np.nan
    want = P.solve_plane(pos, dq, sigma, src, dst2, normals_with(normals, zero), 8, 12, 1e-3, 4, 1.0, 2, 0.05, 0.0)
    for g, w in zip(got, want):
        assert np.array_equal(bits(g), bits(w))
    # ... and where a zero-normal point's live position is does not matter: rho = +-0 whatever e0 is
    dst3 = dst.copy(); dst3[zero] += F32(0.5)
    moved = P.solve_plane(pos, dq, sigma, src, dst3, marked, 8, 12, 1e-3, 4, 1.0, 2, 0.05, 0.0)
    for g, w in zip(got[:3], moved[:3]):
        assert np.array_equal(g, w)


def normals_with(normals, zero):
    n = normals.copy()
    n[zero] = 0
    return n


# ------------------------------------------------------------------------------------------------ (5) the closed loop's oracle side moves
def test_the_loops_oracle_side_moves_nodes_every_frame():
    """tests/test_gpu_nonrigid_loop_plane.py compares the GPU loop with an oracle loop whose solve is this restatement, stage by stage.
    That is only worth something if the solve does something there: on the oracle side alone, every frame's solve moves at least one
    node and lowers the data energy (and the loop's other conditions hold), the last frame has points with a usable normal and points
    whose normal is NaN, and the transforms are not those of the same loop with the point-to-point solve."""
    case = NL.FAST
    rec, be = PL.run_oracle_loop(case)
    assert NL.nonvacuity(rec, case) == []
    for f in range(1, case.frames):
        st = NL.stage(rec, f, "solve")
        en = st["energy"].view(F32)
        print("frame %d: nodes moved %d, energies %s" % (f, int(st["moved"]), en))
        assert int(st["moved"]) >= 1 and en[1] < en[0]
    ok = np.isfinite(be.plane_normals).all(1)
    assert ok.sum() > 1000 and (~ok).sum() > 1000

    class RegSolve(NL.OracleBackend):
        def solve(self, canonical, live, frame):
            self.dq, en = R.solve(self.pos, self.dq, self.sig, canonical, live, self.k, self.case.iters, self.case.lam, PL.KG, PL.LAMBDA_REG)
            return en

    class AssocReg(AL.AssocOracleBackend, RegSolve):
        pass
    ptp = NL.run(AssocReg(case), case)
    assert not np.array_equal(NL.stage(rec, 1, "solve")["dq"], NL.stage(ptp, 1, "solve")["dq"])
