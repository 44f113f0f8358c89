"""numpy float32 restatement of the point-to-plane warp solve (dfusion_warp_solve_plane) on solver_reg_ref's and
solver_robust_ref's pieces, operation for operation: the robust rounds with the residual of every point taken along its normal,
rho = (nx ex + ny ey) + nz ez, the right-hand side W^T Omega (n rho), the operator W^T Omega N N^T W and ONE conjugate-gradient recurrence
over the 3M vector (every dot product the three per-component sums combined as (s0 + s1) + s2).

    solve_plane(pos, dq, sigma, canonical, live, normals, k, iters, lam, kg, lambda_reg, rounds, tukey_c, huber_delta)
        -> (dq_out [M, 8], energy [4], point_weights [N], edge_weights [M, kg] or None)
"""
import copy

import numpy as np

import solver_reg_ref as R
import solver_robust_ref as RR

F32 = np.float32


def dot_n(n, e):
    """(nx ex + ny ey) + nz ez per row."""
    return ((n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2]).astype(F32)


def plane_setup(pos, dq, sigma, canonical, live, normals, k):
    """df_sv_setup_kernel<true>: R.setup's rule, and a point whose normal has a NaN or infinite component is invalid too (a NaN canonical
    point is what R.setup turns into key M, weights 0 and e0 = 0).  Returns R.setup's tuple and the normals with the invalid points' set
    to 0 (the kernels never use those)."""
    bad = ~np.isfinite(normals).all(1)
    canonical = canonical.copy()
    canonical[bad] = np.nan
    w, keys, e0, node_t = R.setup(pos, dq, sigma, canonical, live, k)
    n = np.where((keys[:, 0] < len(pos))[:, None], normals, F32(0)).astype(F32)
    return w, keys, e0, node_t, n


def rho_of(n, e, valid):
    """df_sv_plane_rho_kernel: n . e, 0 for an invalid point."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(valid, dot_n(n, e), F32(0)).astype(F32)


def tukey_weights(rho, c2):
    with np.errstate(invalid="ignore", over="ignore"):
        s = rho * rho
        u = F32(1) - s / c2
        return np.where(s < c2, u * u, F32(0)).astype(F32)


def data_energy(rho, tukey, c2):
    """df_sv_point_energy_kernel: one value per point, thread-strided, then the 1024-tree."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = (rho * rho).astype(F32)
        if tukey:
            u = F32(1) - s / c2
            third = c2 / F32(3)
            s = np.where(s < c2, third * (F32(1) - (u * u) * u), third).astype(F32)
    return R.strided_sum1024(s[:, None])[0]


def sum3(v):
    """A dot product of the coupled recurrence: the per-component sums (thread-strided, 1024-tree), then (s0 + s1) + s2."""
    s = R.strided_sum1024(v)
    return F32((s[0] + s[1]) + s[2])


def project(n, u, valid):
    """df_sv_w_apply_kernel<K, true>'s store: n (n . u), 0 for an invalid point."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = dot_n(n, u)
        return np.where(valid[:, None], n * d[:, None], F32(0)).astype(F32)


def solve_plane(pos, dq, sigma, canonical, live, normals, k, iters, lam=0.0, kg=0, lambda_reg=0.0, rounds=1, tukey_c=0.0, huber_delta=0.0,
                details=None):
    """`details` (a dict) receives w, keys, lists, graph, normals (as used) and per round the lists e0, rho, omega, omega_e, g,
    x (= delta), dq, steps (the CG steps taken before the recurrence froze)."""
    pos, dq, sigma, canonical, live = R.f32(pos), R.f32(dq).reshape(-1, 8), R.f32(sigma), R.f32(canonical), R.f32(live)
    normals = R.f32(normals)
    M, N = len(pos), len(canonical)
    assert rounds >= 1 and normals.shape == (N, 3)
    lam, lreg = F32(lam), F32(lambda_reg)
    c, delta = F32(tukey_c), F32(huber_delta)
    c2, d2 = c * c, delta * delta
    reg = kg > 0 and lreg != 0
    tukey, huber = c != 0, bool(reg and delta != 0)
    w, keys, e0, node_t, n = plane_setup(pos, dq, sigma, canonical, live, normals, k)
    valid = keys[:, 0] < M
    lists = R.NodeLists(keys, w, M, k)
    G = R.Graph(pos, sigma, kg) if reg else None
    en = np.zeros(4, F32)
    omega, omega_e = np.ones(N, F32), (np.ones(M * kg, F32) if reg else None)
    log = dict(e0=[], rho=[], omega=[], omega_e=[], x=[], dq=[], g=[], steps=[])
    zero = F32(0)
    for rnd in range(rounds):
        if rnd:
            node_t = R.node_translation(dq)
            e0 = RR.residual_at(w, keys, node_t, canonical, live)
        rho = rho_of(n, e0, valid)
        b = (n * rho[:, None]).astype(F32)
        L, Gw = lists, G
        if tukey:
            omega = tukey_weights(rho, c2)
            L = copy.copy(lists)
            L.w = (omega[lists.pt] * lists.w).astype(F32)
        if rnd == 0:
            en[0] = data_energy(rho, tukey, c2)
        r = L.apply(b)
        if reg:
            vj = pos[G.nbr.reshape(-1)]
            g = R.dq_transform(dq[G.tail], vj) - R.dq_transform(dq[G.nbr.reshape(-1)], vj)
            if huber:
                omega_e = RR.huber_weights(g, delta, d2)
                Gw = copy.copy(G)
                Gw.alpha = (G.alpha.reshape(-1) * omega_e).astype(F32).reshape(G.alpha.shape)
            r = r - lreg * Gw.node_sums(g)
            if rnd == 0:
                en[2] = RR.huber_energy(G, g, None, delta, d2) if huber else G.energy(g, np.zeros((M, 3), F32))
        x = np.zeros((M, 3), F32)
        p = r.copy()
        rr = sum3(r * r)
        rr0 = rr
        steps = 0
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            for _ in range(iters):
                if not rr > 0:                       # frozen: the remaining steps change nothing
                    break
                steps += 1
                q = L.apply(project(n, R.w_apply(w, keys, M, p), valid), lam, p)
                if reg:
                    q = q + lreg * Gw.node_sums(Gw.edge_diff(p))
                pq = sum3(p * q)
                alpha = F32(rr / pq) if (pq > 0 and rr > 0) else zero
                x = x + alpha * p
                r = r - alpha * q
                rn = sum3(r * r)
                beta = F32(rn / rr) if (alpha != 0 and rr > 0) else zero
                p = r + beta * p
                rr = rn if (alpha != 0 and rn > F32(1.0e-10) * rr0) else zero
        if rnd == rounds - 1:
            e1 = e0 - R.w_apply(w, keys, M, x)
            en[1] = data_energy(rho_of(n, e1, valid), tukey, c2)
            if reg:
                en[3] = RR.huber_energy(G, g, x, delta, d2) if huber else G.energy(g, x)
        T = np.concatenate([np.zeros((M, 1), F32), node_t[:, 1:] + x], 1)
        dq = np.concatenate([dq[:, :4], R.q_mul(F32(0.5) * T, dq[:, :4])], 1).astype(F32)
        log["e0"].append(e0); log["rho"].append(rho); log["omega"].append(omega.copy()); log["x"].append(x); log["dq"].append(dq)
        log["omega_e"].append(None if omega_e is None else omega_e.copy()); log["g"].append(g if reg else None); log["steps"].append(steps)
    if details is not None:
        details.update(w=w, keys=keys, lists=lists, graph=G, normals=n, **log)
    return dq, en, omega, (omega_e.reshape(M, kg) if reg else None)
