"""numpy float32 restatement of the robust warp solve (dfusion_warp_solve_robust) on solver_reg_ref's pieces, operation for
operation: `rounds` rounds of the regularised solve, each with Tukey weights on the points (multiplied into the node-major entry
weights) and Huber weights on the graph edges (multiplied into a copy of alpha), both taken at the transforms the round starts from.

    solve_robust(pos, dq, sigma, canonical, live, k, iters, lam, kg, lambda_reg, rounds, tukey_c, huber_delta)
        -> (dq_out [M, 8], energy [4], point_weights [N], edge_weights [M, kg] or None)
"""
import copy

import numpy as np

import solver_reg_ref as R

F32 = np.float32


def residual_at(w, keys, node_t, canonical, live):
    """df_sv_round_e0_kernel: e0 from the stored entries at the translations node_t -- df_sv_setup_kernel's sums in slot order."""
    M = len(node_t)
    valid = keys[:, 0] < M
    s = np.zeros((len(w), 3), F32)
    for j in range(w.shape[1]):
        t = node_t[np.where(valid, keys[:, j], 0)]
        s = np.where(valid[:, None], s + w[:, j, None] * t[:, 1:], s)
    with np.errstate(invalid="ignore"):
        return np.where(valid[:, None], (live - canonical) - s, F32(0)).astype(F32)


def sq_norm(e):
    return ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]).astype(F32)


def tukey_weights(e, c2):
    with np.errstate(invalid="ignore", over="ignore"):
        s = sq_norm(e)
        u = F32(1) - s / c2
        return np.where(s < c2, u * u, F32(0)).astype(F32)


def tukey_energy(e, c2):
    with np.errstate(invalid="ignore", over="ignore"):
        s = sq_norm(e)
        u = F32(1) - s / c2
        third = c2 / F32(3)
        val = np.where(s < c2, third * (F32(1) - (u * u) * u), third).astype(F32)
    return R.strided_sum1024(val[:, None])[0]


def huber_weights(g, delta, d2):
    s = sq_norm(g)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s <= d2, F32(1), delta / np.sqrt(s)).astype(F32)


def huber_energy(G, g, x, delta, d2):
    h = (g + x[G.tail]) - x[G.nbr.reshape(-1)] if x is not None else g
    s = sq_norm(h)
    with np.errstate(invalid="ignore"):
        val = (G.alpha.reshape(-1) * np.where(s <= d2, s, (F32(2) * delta) * np.sqrt(s) - d2)).astype(F32)
    return R.strided_sum1024(val[:, None])[0]


def solve_robust(pos, dq, sigma, canonical, live, k, iters, lam=0.0, kg=0, lambda_reg=0.0, rounds=3, tukey_c=0.0, huber_delta=0.0,
                 details=None):
    """`details` (a dict) receives w, keys, lists, and per round the lists e0, omega, omega_e, g, x (= delta), dq."""
    pos, dq, sigma, canonical, live = R.f32(pos), R.f32(dq).reshape(-1, 8), R.f32(sigma), R.f32(canonical), R.f32(live)
    M, N = len(pos), len(canonical)
    assert rounds >= 1
    lam, lreg = F32(lam), F32(lambda_reg)
    c, delta = F32(tukey_c), F32(huber_delta)
    c2, d2 = c * c, delta * delta
    reg = kg > 0 and lreg != 0
    tukey, huber = c != 0, bool(reg and delta != 0)
    # once per call
    w, keys, e0, node_t = R.setup(pos, dq, sigma, canonical, live, k)
    lists = R.NodeLists(keys, w, M, k)
    G = R.Graph(pos, sigma, kg) if reg else None
    en = np.zeros(4, F32)
    omega, omega_e = np.ones(N, F32), (np.ones(M * kg, F32) if reg else None)
    log = dict(e0=[], omega=[], omega_e=[], x=[], dq=[], g=[])
    zero = F32(0)
    for rnd in range(rounds):
        if rnd:
            node_t = R.node_translation(dq)
            e0 = residual_at(w, keys, node_t, canonical, live)
        L, Gw = lists, G
        if tukey:
            omega = tukey_weights(e0, c2)
            L = copy.copy(lists)
            L.w = (omega[lists.pt] * lists.w).astype(F32)
        if rnd == 0:
            en[0] = tukey_energy(e0, c2) if tukey else R.energy_sum(e0)
        r = L.apply(e0)
        if reg:
            vj = pos[G.nbr.reshape(-1)]
            g = R.dq_transform(dq[G.tail], vj) - R.dq_transform(dq[G.nbr.reshape(-1)], vj)
            if huber:
                omega_e = huber_weights(g, delta, d2)
                Gw = copy.copy(G)
                Gw.alpha = (G.alpha.reshape(-1) * omega_e).astype(F32).reshape(G.alpha.shape)
            r = r - lreg * Gw.node_sums(g)
            if rnd == 0:
                en[2] = huber_energy(G, g, None, delta, d2) if huber else G.energy(g, np.zeros((M, 3), F32))
        x = np.zeros((M, 3), F32)
        p = r.copy()
        rr = R.strided_sum1024(r * r)
        rr0 = rr.copy()
        with np.errstate(divide="ignore", invalid="ignore"):
            for _ in range(iters):
                if not (rr > 0).any():
                    break
                q = L.apply(R.w_apply(w, keys, M, p), lam, p)
                if reg:
                    q = q + lreg * Gw.node_sums(Gw.edge_diff(p))
                pq = R.strided_sum1024(p * q)
                alpha = np.where((pq > 0) & (rr > 0), rr / pq, zero).astype(F32)
                x = x + alpha * p
                r = r - alpha * q
                rn = R.strided_sum1024(r * r)
                beta = np.where((alpha != 0) & (rr > 0), rn / rr, zero).astype(F32)
                p = r + beta * p
                rr = np.where((alpha != 0) & (rn > F32(1.0e-10) * rr0), rn, zero).astype(F32)
        if rnd == rounds - 1:
            e1 = e0 - R.w_apply(w, keys, M, x)
            en[1] = tukey_energy(e1, c2) if tukey else R.energy_sum(e1)
            if reg:
                en[3] = huber_energy(G, g, x, delta, d2) if huber else G.energy(g, x)
        T = np.concatenate([np.zeros((M, 1), F32), node_t[:, 1:] + x], 1)
        dq = np.concatenate([dq[:, :4], R.q_mul(F32(0.5) * T, dq[:, :4])], 1).astype(F32)
        log["e0"].append(e0); log["omega"].append(omega.copy()); log["x"].append(x); log["dq"].append(dq)
        log["omega_e"].append(None if omega_e is None else omega_e.copy()); log["g"].append(g if reg else None)
    if details is not None:
        details.update(w=w, keys=keys, lists=lists, graph=G, **log)
    return dq, en, omega, (omega_e.reshape(M, kg) if reg else None)
