"""CPU side of tests/test_gpu_node_counts.py: the oracle's nanoflann replay against the reference's own nanoflann on a deep tree full
of exact ties, and the oracle's data-term solve (which the GPU equals bit for bit) against a float64 solution of the damped normal
equations (W^T W + lambda I) delta = W^T e0 at node counts on the far side of each of the GPU step kernels' thresholds."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as sla

import oracle_lib as O
from dynamicfusion_amd import synth
from test_gpu_node_counts import tie_lattice

F32 = np.float32


@pytest.mark.skipif(not O.have_ref(), reason="the reference's nanoflann (oracle/_ref) is not built")
def test_tie_order_in_a_32_cubed_lattice_equals_reference_nanoflann():
    pos, q = tie_lattice()
    for k in (4, 8):
        a_idx, a_d2 = O.knn(pos, q, k)
        r_idx, r_d2 = O.knn(pos, q, k, use_ref=True)
        b_idx, _ = O.knn(pos, q, k, brute=True)
        assert (a_idx != b_idx).any(1).sum() > 1000           # ties decided by the tree walk, not by index order
        assert np.array_equal(a_d2.view(np.uint32), r_d2.view(np.uint32))
        assert np.array_equal(a_idx, r_idx), "k = %d: %d queries differ" % (k, int((a_idx != r_idx).any(1).sum()))


# ---- float64 check of the damped solve
LAM = 1e-3
KAPPA_MAX = 15.0


def damped_problem(M, seed):
    """Nodes on a jittered lattice (spacing s), sigma = 0.35 s, three points per node scattered 0.15 s around it, non-trivial starting
    transforms, a smooth target motion plus noise.  sigma is small against the spacing so that W^T W is diagonally dominant and the
    damped matrix well conditioned (kappa <= KAPPA_MAX, checked below); the weights still reach the neighbouring nodes."""
    rng = np.random.default_rng(seed)
    n = int(np.ceil(M ** (1 / 3)))
    s = 0.02
    g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3)[rng.permutation(n ** 3)[:M]]
    pos = ((g + rng.uniform(-0.2, 0.2, g.shape)) * s).astype(F32)
    sigma = np.full(M, 0.35 * s, F32)
    dq = synth.dq_from_twist(rng.uniform(-0.1, 0.1, (M, 3)).astype(F32), rng.uniform(-0.005, 0.005, (M, 3)).astype(F32))
    src = (np.repeat(pos, 3, 0) + rng.normal(0, 0.15 * s, (3 * M, 3))).astype(F32)
    dst = (src + 0.03 * np.sin(20 * src) + rng.normal(0, 1e-3, src.shape)).astype(F32)
    return pos, sigma, dq, src, dst


def translations(dq):
    out = np.zeros((len(dq), 4), F32)
    for j in range(len(dq)):
        O.lib().orc_node_translation(dq[j], out[j])
    return out[:, 1:].astype(np.float64)


@pytest.mark.parametrize("M", [2049, 5121, 8193])
def test_damped_solve_matches_float64_normal_equations(M):
    k = 8
    pos, sigma, dq, src, dst = damped_problem(M, M)
    N = len(src)
    # W in float64: the k nearest nodes (exhaustive scan), weights exp(-d^2 / 2 sigma^2) from float64 distances
    idx, _ = O.knn(pos, src, k, brute=True)
    d2 = ((src[:, None, :].astype(np.float64) - pos[idx].astype(np.float64)) ** 2).sum(-1)
    w = np.exp(-d2 / (2 * sigma[idx].astype(np.float64) ** 2))
    W = sp.csr_matrix((w.ravel(), idx.ravel(), np.arange(0, N * k + 1, k)), shape=(N, M))
    T0 = translations(dq)
    e0 = (dst.astype(np.float64) - src.astype(np.float64)) - W @ T0
    A = (W.T @ W + LAM * sp.identity(M)).tocsc()
    b = W.T @ e0
    delta = sla.spsolve(A, b)
    lmax = sla.eigsh(A, 1, which="LA", return_eigenvectors=False)[0]
    lmin = sla.eigsh(A, 1, sigma=0, which="LM", return_eigenvectors=False)[0]
    kappa = lmax / lmin
    assert kappa <= KAPPA_MAX, kappa
    # The CG stops a component once |r| <= 1e-5 |r0| (SV_REL_TOL2 = 1e-10 on the squares), and |d - d*| / |d*| <= kappa |r| / |b|; twice
    # that covers the float32 arithmetic: tol = 2 kappa 1e-5 <= 3e-4.
    tol = 2 * kappa * 1e-5
    # the damping matters at this tolerance: the undamped least-squares solution would fail it
    undamped = sla.spsolve((W.T @ W).tocsc(), b)
    assert (np.linalg.norm(undamped - delta, axis=0) / np.linalg.norm(delta, axis=0) > tol).all()

    iters = 120
    out, en = O.solve_data_term(pos, dq, sigma, src, dst, k, iters, LAM)
    out_more, en_more = O.solve_data_term(pos, dq, sigma, src, dst, k, iters + 1, LAM)
    assert np.array_equal(out, out_more) and np.array_equal(en, en_more)      # the relative-residual test stopped the solve
    d_o = translations(out) - T0
    rel = np.linalg.norm(d_o - delta, axis=0) / np.linalg.norm(delta, axis=0)
    print("M = %d: kappa %.2f, tol %.2g, relative error per component %s" % (M, kappa, tol, rel))
    assert (rel <= tol).all(), rel
    E0 = float((e0 ** 2).sum())
    assert abs(float(en[0]) - E0) <= 1e-5 * E0
    res_o = e0 - W @ d_o
    f_o = float((res_o ** 2).sum() + LAM * (d_o ** 2).sum())
    f_star = float(((e0 - W @ delta) ** 2).sum() + LAM * (delta ** 2).sum())
    assert f_star <= f_o <= f_star * (1 + 1e-3)
    E1 = float((res_o ** 2).sum())
    assert abs(float(en[1]) - E1) <= 1e-4 * E1
