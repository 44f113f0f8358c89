"""The rule of the robust warp solve, on the CPU: tests/solver_robust_ref.py -- the numpy restatement the GPU is compared with
bit for bit in tests/test_gpu_solver_robust.py -- gives the regularised restatement's bits with both thresholds off, rejects exactly the
planted outliers of a planted problem and recovers its field better than the quadratic solve, and meets a dense float64 IRLS."""
import numpy as np

import solver_reg_ref as R
import solver_robust_ref as RR
from dynamicfusion_amd import synth
from solver_cases import bits, random_problem

F32 = np.float32


# ------------------------------------------------------------------------------------------------ (a) off switches
def test_thresholds_off_one_round_is_the_regularised_restatement():
    pos, dq, sigma, src, dst = random_problem(100, 2000)
    for kg, lreg in ((4, 1.0), (0, 0.0)):
        want_dq, want_en = R.solve(pos, dq, sigma, src, dst, 8, 25, 1e-3, kg, lreg)
        got_dq, got_en, pw, ew = RR.solve_robust(pos, dq, sigma, src, dst, 8, 25, 1e-3, kg, lreg, rounds=1)
        assert np.array_equal(bits(got_dq), bits(want_dq)) and np.array_equal(bits(got_en), bits(want_en))
        assert (pw == 1).all() and (ew is None if kg == 0 else (ew == 1).all())


def test_thresholds_off_three_rounds_are_three_chained_solves():
    pos, dq, sigma, src, dst = random_problem(100, 2000)
    cur, ens = dq, []
    for _ in range(3):
        cur, en = R.solve(pos, cur, sigma, src, dst, 8, 6, 1e-3, 4, 1.0)
        ens.append(en)
    got_dq, got_en, _, _ = RR.solve_robust(pos, dq, sigma, src, dst, 8, 6, 1e-3, 4, 1.0, rounds=3)
    assert np.array_equal(bits(got_dq), bits(cur))
    assert np.array_equal(bits(got_en), bits([ens[0][0], ens[2][1], ens[0][2], ens[2][3]]))
    assert not np.array_equal(bits(ens[0]), bits(ens[2]))                # (the rounds did move on)


# ------------------------------------------------------------------------------------------------ (b) the planted problem
TUKEY_C, HUBER_DELTA, ROUNDS = 0.05, 0.01, 5
LAM, LREG = 1e-3, 1.0


def planted_problem():
    """M = 60 nodes with identity transforms, N = 1500 points, k = 8.  A smooth translation field is planted on the nodes; an inlier's
    live point is its canonical point moved by exactly the field's blend sum_i w_vi T_i (so the planted field has zero data residual on
    the inliers); every tenth point's live position is displaced by a further 0.25 m in a seeded direction.  The field's amplitude is
    scaled so that no inlier moves more than 1 cm (a point's weights sum to more than 1)."""
    M, N, k = 60, 1500, 8
    rng = np.random.default_rng(101)
    pos = rng.uniform(-1, 1, (M, 3)).astype(F32)
    sigma = rng.uniform(0.3, 0.6, M).astype(F32)
    dq = synth.identity_dq(M)
    src = rng.uniform(-1, 1, (N, 3)).astype(F32)
    w, keys, _, _ = R.setup(pos, dq, sigma, src, src, k)
    shape = np.stack([np.sin(1.5 * pos[:, 0] + 0.3), np.cos(1.2 * pos[:, 1] - 0.5), np.sin(pos[:, 2] + pos[:, 0])], 1)
    shape = shape / np.linalg.norm(shape, axis=1).max()
    blend = np.einsum("nk,nkc->nc", w.astype(np.float64), shape[keys])
    amp = 0.0099 / max(1.0, float(np.linalg.norm(blend, axis=1).max()))
    planted = amp * shape                                                # float64 [M, 3], |T_i| <= 1 cm
    dst = src.astype(np.float64) + amp * blend
    outlier = np.zeros(N, bool); outlier[::10] = True
    d = rng.normal(0, 1, (N, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    dst[outlier] += 0.25 * d[outlier]
    return pos, dq, sigma, src, dst.astype(F32), planted, outlier


ROBUST_MEASURED = 1.59e-4      # largest node error of the robust solve against the planted field (metres), measured on the CPU
QUADRATIC_MEASURED = 2.87e-2   # the same of the quadratic solve (5 chained rounds)


def node_error(dq_out, planted):
    return float(np.abs(R.node_translation(dq_out)[:, 1:].astype(np.float64) - planted).max())


def test_planted_outliers_are_rejected_and_the_field_recovered():
    """Measured on the CPU (x86-64, glibc exp), 100 steps a round, lam = 1e-3, lambda_reg = 1: the robust solve's largest node error
    is ROBUST_MEASURED, the quadratic solve's QUADRATIC_MEASURED (see the constants).  Asserted: robust <= 4 x, quadratic >= 1/4 x (the margin
    DESIGN.md 12 uses for float32 conjugate gradients against a dense solve)."""
    pos, dq, sigma, src, dst, planted, outlier = planted_problem()
    d = {}
    r_dq, r_en, pw, ew = RR.solve_robust(pos, dq, sigma, src, dst, 8, 100, LAM, 4, LREG, ROUNDS, TUKEY_C, HUBER_DELTA, details=d)
    first = np.sqrt(RR.sq_norm(d["e0"][0]).astype(np.float64))
    assert first[~outlier].max() <= 0.01 < TUKEY_C and first[outlier].min() >= 0.24 > TUKEY_C       # the construction
    w1 = d["omega"][0]
    assert (w1[outlier] == 0).all() and (w1[~outlier] > 0).all()
    assert (pw[outlier] == 0).all() and (pw[~outlier] > 0).all()         # and they stay rejected
    q_dq, q_en, _, _ = RR.solve_robust(pos, dq, sigma, src, dst, 8, 100, LAM, 4, LREG, ROUNDS, 0.0, 0.0)
    e_rob, e_quad = node_error(r_dq, planted), node_error(q_dq, planted)
    print("planted problem: node error robust %.3g, quadratic %.3g; energies robust %s quadratic %s" % (e_rob, e_quad, r_en, q_en))
    assert r_en[1] < r_en[0]
    assert e_rob < e_quad
    assert e_rob <= 4 * ROBUST_MEASURED
    assert e_quad >= QUADRATIC_MEASURED / 4


# ------------------------------------------------------------------------------------------------ (c) dense float64 IRLS
def dense_irls(d, M, lam, lreg, rounds, c, delta):
    """The same rounds in float64 on dense matrices: weights from the float64 residuals, each round's weighted normal equations by
    numpy.linalg.solve.  From the restatement's own f32 w, alpha and first e0 and g (the rotations are fixed, so a round's
    g is the first g moved by the translations so far)."""
    w, keys, G = d["w"].astype(np.float64), d["keys"], d["graph"]
    e_first, g_first = d["e0"][0].astype(np.float64), d["g"][0].astype(np.float64)
    N, k = w.shape
    W = np.zeros((N, M))
    for j in range(k):
        ok = keys[:, j] < M
        np.add.at(W, (np.flatnonzero(ok), keys[ok, j]), w[ok, j])
    alpha, head, tail = G.alpha.reshape(-1).astype(np.float64), G.nbr.reshape(-1), G.tail
    total = np.zeros((M, 3))
    for _ in range(rounds):
        e = e_first - W @ total
        s = (e * e).sum(1)
        om = np.where(s < c * c, (1 - s / (c * c)) ** 2, 0.0)
        g = g_first + total[tail] - total[head]
        sg = (g * g).sum(1)
        with np.errstate(divide="ignore"):
            a = alpha * np.where(sg <= delta * delta, 1.0, delta / np.sqrt(sg))
        A = W.T @ (om[:, None] * W) + lam * np.eye(M)
        rhs = W.T @ (om[:, None] * e)
        for ed in range(len(head)):
            i, j = tail[ed], head[ed]
            A[i, i] += lreg * a[ed]; A[j, j] += lreg * a[ed]; A[i, j] -= lreg * a[ed]; A[j, i] -= lreg * a[ed]
            rhs[i] -= lreg * a[ed] * g[ed]; rhs[j] += lreg * a[ed] * g[ed]
        total = total + np.linalg.solve(A, rhs)
    return total


HUBER_DELTA_DENSE = 5e-4
DENSE_IRLS_MEASURED = 1.71e-8  # largest |delta - dense| measured on the CPU (see the docstring below)


def test_converged_rounds_meet_a_dense_float64_irls():
    """The planted problem, 5 rounds of 400 steps, against the dense float64 IRLS: the translations accumulated over the rounds.
    huber_delta is 0.5 mm here, not 1 cm: the planted field is so smooth that no edge difference reaches 1 cm, and the comparison
    should cross Huber's linear zone too (asserted below).
    Measured on the CPU (x86-64, glibc exp): largest |delta - dense| = DENSE_IRLS_MEASURED; asserted: 4 x that."""
    pos, dq, sigma, src, dst, planted, _ = planted_problem()
    d = {}
    r_dq, _, _, _ = RR.solve_robust(pos, dq, sigma, src, dst, 8, 400, LAM, 4, LREG, ROUNDS, TUKEY_C, HUBER_DELTA_DENSE, details=d)
    want = dense_irls(d, len(pos), float(F32(LAM)), float(F32(LREG)), ROUNDS, float(F32(TUKEY_C)), float(F32(HUBER_DELTA_DENSE)))
    got = R.node_translation(r_dq)[:, 1:].astype(np.float64)             # (the field starts at the identity: T = the accumulated delta)
    err = float(np.abs(got - want).max())
    print("dense IRLS: max |delta - dense| = %.3g, max |delta| = %.3g" % (err, np.abs(want).max()))
    assert np.abs(want).max() > 1e-3
    print("edges past delta per round:", [int((w < 1).sum()) for w in d["omega_e"]])
    assert any((w < 1).any() for w in d["omega_e"]), "no edge ever left the quadratic zone: Huber untested"
    assert err <= 4 * DENSE_IRLS_MEASURED
