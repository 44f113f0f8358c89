"""The rule of the regularised warp solve, on the CPU: tests/solver_reg_ref.py -- the numpy restatement the GPU is compared
with bit for bit in tests/test_gpu_solver_reg.py -- is pinned to the committed oracle where the two overlap (kg = 0), checked against an
independent dense float64 solve of the same normal equations where they do not, and shown to do what the term is for."""
import numpy as np
import pytest

import oracle_lib as O
import solver_reg_ref as R
from dynamicfusion_amd import synth
from solver_cases import bits, random_problem

F32 = np.float32


# ------------------------------------------------------------------------------------------------ pinned to the oracle
@pytest.mark.parametrize("M,N,k,iters,lam", [(100, 2000, 8, 25, 0.0), (257, 1503, 4, 25, 1e-3)], ids=["k8", "k4-damped-ragged"])
def test_without_graph_the_restatement_is_the_oracle(M, N, k, iters, lam):
    pos, dq, sigma, src, dst = random_problem(M, N)
    want_dq, want_en = O.solve_data_term(pos, dq, sigma, src, dst, k, iters, lam)
    got_dq, got_en = R.solve(pos, dq, sigma, src, dst, k, iters, lam, kg=0)
    assert want_en[1] < 0.5 * want_en[0]
    assert np.array_equal(bits(got_en[:2]), bits(want_en))
    assert np.array_equal(bits(got_dq), bits(want_dq))
    assert got_en[2] == 0 and got_en[3] == 0


# ------------------------------------------------------------------------------------------------ against a dense float64 solve
def dense_delta(d, M, lam, lreg):
    """The normal equations (W^T W + lam I + lreg L) delta = W^T e0 - lreg b as a dense float64 matrix, from the restatement's own f32
    w, alpha and g; numpy.linalg.solve."""
    w, keys, e0, G, g = d["w"].astype(np.float64), d["keys"], d["e0"].astype(np.float64), d["graph"], d["g"].astype(np.float64)
    N, k = w.shape
    W = np.zeros((N, M))
    for j in range(k):
        ok = keys[:, j] < M
        np.add.at(W, (np.flatnonzero(ok), keys[ok, j]), w[ok, j])
    A = W.T @ W + lam * np.eye(M)
    rhs = W.T @ e0
    alpha, head, tail = G.alpha.reshape(-1).astype(np.float64), G.nbr.reshape(-1), G.tail
    for e in range(len(head)):
        i, j, a = tail[e], head[e], alpha[e]
        A[i, i] += lreg * a; A[j, j] += lreg * a; A[i, j] -= lreg * a; A[j, i] -= lreg * a
        rhs[i] -= lreg * a * g[e]; rhs[j] += lreg * a * g[e]
    return np.linalg.solve(A, rhs)


DENSE_MEASURED = 4.6e-6        # largest |delta - dense| measured on the CPU (see the docstring below)


def test_converged_solve_meets_the_dense_normal_equations():
    """M = 60, N = 1500, k = 8, kg = 4, lam = 1e-3, lambda_reg = 1, 400 steps against numpy.linalg.solve in float64.
    Measured on the CPU (x86-64, glibc exp): largest |delta - dense| = 4.6e-6 with |delta| up to 7.3e-2 (the
    data-only solve of the same problem, which is the oracle's bit for bit, is 2.8e-5 off its own dense solve: float32 conjugate gradients
    on a matrix whose weights span many orders of magnitude); asserted: 4 x that."""
    M, lam, lreg = 60, 1e-3, 1.0
    pos, dq, sigma, src, dst = random_problem(M, 1500)
    d = {}
    R.solve(pos, dq, sigma, src, dst, 8, 400, lam, kg=4, lambda_reg=lreg, details=d)
    want = dense_delta(d, M, float(F32(lam)), float(F32(lreg)))
    err = float(np.abs(d["x"].astype(np.float64) - want).max())
    print("dense solve: max |delta - dense| = %.3g, max |delta| = %.3g" % (err, np.abs(want).max()))
    assert np.abs(want).max() > 1e-2
    assert err <= 4 * DENSE_MEASURED


# ------------------------------------------------------------------------------------------------ behaviour
def test_unobserved_nodes_follow_their_neighbours():
    pos = np.zeros((20, 3), F32); pos[:, 0] = np.arange(20, dtype=F32) * F32(0.1)
    sigma = np.full(20, 0.1, F32)
    dq = synth.identity_dq(20)
    rng = np.random.default_rng(3)
    src = np.stack([rng.uniform(-0.05, 1.15, 600), rng.uniform(-0.02, 0.02, 600), rng.uniform(-0.02, 0.02, 600)], 1).astype(F32)
    dst = (src + F32([0.02, 0, 0])).astype(F32)
    d0, d1 = {}, {}
    R.solve(pos, dq, sigma, src, dst, 4, 200, 0.0, kg=0, details=d0)
    assert d0["keys"].max() <= 15, "the points must not reach nodes 16..19"
    assert not d0["x"][16:].any()                                   # no data entry: an empty row, delta exactly 0
    assert d0["x"][11, 0] > 0.002                                   # (the weights of a point sum to more than 1: a node gets part of the shift)
    R.solve(pos, dq, sigma, src, dst, 4, 200, 0.0, kg=2, lambda_reg=1.0, details=d1)
    print("delta_x, data only:", d0["x"][:, 0], "\ndelta_x, regularised:", d1["x"][:, 0])
    assert d1["x"][11, 0] > 0.002 and (d1["x"][16:, 0] > 0.5 * d1["x"][11, 0]).all(), d1["x"][:, 0]


def test_rigid_field_has_no_regularisation_energy():
    """Every node carries the same transform, so g_e = T(v_j) - T(v_j) is dq_transform evaluated twice on identical inputs: exactly 0,
    and E_reg before is exactly 0.  A uniform translation keeps the field rigid: E_reg after stays small against the data energy."""
    rng = np.random.default_rng(5)
    M = 40
    pos = rng.uniform(-0.5, 0.5, (M, 3)).astype(F32)
    sigma = np.full(M, 0.4, F32)
    one = synth.dq_from_twist(F32([[0.2, -0.1, 0.15]]), F32([[0.01, 0.02, -0.01]]))
    dq = np.repeat(one, M, 0)
    src = rng.uniform(-0.5, 0.5, (1500, 3)).astype(F32)
    warped, _ = O.warp_points(pos, dq, sigma, src, None, 8)
    dst = (warped + F32([0.01, -0.02, 0.015])).astype(F32)
    d = {}
    _, en = R.solve(pos, dq, sigma, warped, dst, 8, 100, 1e-3, kg=4, lambda_reg=1.0, details=d)
    assert not d["g"].any()
    assert en[2] == 0
    assert en[0] > 0 and en[3] <= 1e-3 * en[0], en


# ------------------------------------------------------------------------------------------------ the graph rule
def test_graph_of_eight_nodes_with_seven_neighbours_is_complete():
    pos = np.random.default_rng(1).uniform(-1, 1, (8, 3)).astype(F32)
    nbr, alpha = R.node_graph(pos, np.linspace(0.1, 0.8, 8).astype(F32), 7)
    for i in range(8):
        assert sorted(nbr[i].tolist()) == [j for j in range(8) if j != i]
    assert np.array_equal(alpha, np.maximum(np.linspace(0.1, 0.8, 8).astype(F32)[:, None], np.linspace(0.1, 0.8, 8).astype(F32)[nbr]))


def test_graph_with_a_duplicated_position():
    pos = np.random.default_rng(2).uniform(-1, 1, (30, 3)).astype(F32)
    pos[17] = pos[4]
    kg = 3
    idx, _ = O.knn(pos, pos, kg + 1)
    nbr, _ = R.node_graph(pos, np.full(30, 0.3, F32), kg)
    for i in range(30):
        row = idx[i].tolist()
        if i in row:                                     # the entry that is i goes, the rest keep their order: kg distinct other nodes
            assert nbr[i].tolist() == [j for j in row if j != i]
            assert i not in nbr[i] and len(set(nbr[i].tolist())) == kg
        else:                                            # i ranked out: the last entry goes
            assert nbr[i].tolist() == row[:kg]
    assert 17 in nbr[4] and 4 in nbr[17]


def test_graph_on_a_lattice_follows_the_knn_tie_order():
    ax = np.arange(4, dtype=F32) * F32(0.25)
    pos = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3).astype(F32)
    kg = 4
    idx, d2 = O.knn(pos, pos, kg + 1)
    assert (d2[:, 1] == d2[:, 2]).all()                  # exact ties at every node
    nbr, _ = R.node_graph(pos, np.full(64, 0.3, F32), kg)
    for i in range(64):
        assert idx[i, 0] == i and nbr[i].tolist() == idx[i, 1:].tolist()
