"""numpy float32 restatement of the warp solve with node rotations as unknowns (dfusion_warp_solve_rigid), operation for
operation, on the pieces of solver_reg_ref / solver_robust_ref / solver_plane_ref: Gauss-Newton rounds against the DQB warp the rest of
the pipeline applies (oracle_lib.warp_points), six unknowns a node (omega about the node's warped position, tau), the Jacobian of that
blend -- the node translations under the unnormalised weights w, the rotation under wn = w / S_v -- and ONE conjugate-gradient
recurrence over the 3-component array of 2M entries (omega_n at entry n, tau_n at entry M + n).

    solve_rigid(pos, dq, sigma, canonical, live, normals, k, iters, lam, lam_rot, kg, lambda_reg, rounds, tukey_c, huber_delta)
        -> (dq_out [M, 8], energy [4], point_weights [N], edge_weights [M, kg] or None)
"""
import copy

import numpy as np

import oracle_lib as O
import solver_plane_ref as P
import solver_reg_ref as R
import solver_robust_ref as RR

F32 = np.float32
_quiet = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


def warp(pos, dq, sigma, canonical, normals, k):
    """y and n': copies of the points and the normals through the point path with an identity warp_to_live."""
    y, n = O.warp_points(pos, dq, sigma, canonical, normals, k)
    return y, n


def node_centres(pos, dq):
    """c_n = dq_transform(rot_n, dual_n, pos_n)."""
    return R.dq_transform(dq, pos).astype(F32)


def rigid_setup(pos, sigma, canonical, live, normals, y, nw, k):
    """Once per call: (w [N, k] the blend weights, wn [N, k] = w / S_v, keys [N, k] (M = invalid point))."""
    M, N = len(pos), len(canonical)
    idx, d2 = O.knn(pos, canonical, k)
    valid = ~(np.isnan(canonical).any(1) | np.isnan(live).any(1))
    if normals is not None:
        valid &= np.isfinite(normals).all(1) & np.isfinite(nw).all(1)
    valid &= np.isfinite(y).all(1)
    w = np.zeros((N, k), F32)
    S = np.zeros(N, F32)
    with np.errstate(**_quiet):
        for j in range(k):
            sg = sigma[np.where(valid, idx[:, j], 0)]
            arg = (-d2[:, j] / (F32(2) * sg * sg)).astype(np.float64)
            w[:, j] = np.where(valid, R._exp(np.where(valid, arg, 0.0)).astype(np.float64).astype(F32), F32(0))
            S = S + w[:, j]
        valid &= ~(S == 0)
        wn = np.where(valid[:, None], w / S[:, None], F32(0)).astype(F32)
        w = np.where(valid[:, None], w, F32(0)).astype(F32)
    keys = np.where(valid[:, None], idx, M).astype(np.int64)
    return w, wn, keys


def blend_translation(w, keys, node_t):
    """T_v = sum_i w_vi t_i in slot order (df_sv_setup_kernel's sums): what the warp adds to the turned point."""
    M = len(node_t)
    s = np.zeros((len(w), 3), F32)
    for j in range(w.shape[1]):
        ok = keys[:, j] < M
        t = node_t[np.where(ok, keys[:, j], 0)]
        s = np.where(ok[:, None], s + w[:, j, None] * t[:, 1:], s)
    return s


def j_apply(w, wn, keys, M, a, q, p, nw, valid):
    """u = J p, one point a row, slot order: st = st + w (p_tau_n - (p_om_n x q_n)), sr = sr + wn p_om_n, u = st + (sr x a_v); with
    normals projected on n'."""
    N, k = wn.shape
    pom, ptau = p[:M], p[M:]
    st, sr = np.zeros((N, 3), F32), np.zeros((N, 3), F32)
    with np.errstate(**_quiet):
        for j in range(k):
            ok = keys[:, j] < M
            n = np.where(ok, keys[:, j], 0)
            h = ptau[n] - R.cross3(pom[n], q[n])
            st = np.where(ok[:, None], st + w[:, j, None] * h, st)
            sr = np.where(ok[:, None], sr + wn[:, j, None] * pom[n], sr)
        s = st + R.cross3(sr, a)
        if nw is not None:
            s = P.project(nw, s, valid)
    return s.astype(F32)


def jt_apply(L, M, a, q, u, lam=None, lam_rot=None, p=None):
    """J^T u (+ damping): a node's six sums over its list -- w u, then wn (a_v x u) -- thread-strided, then the 256-tree; the omega part
    is the second minus q_n x the first.  -> [2M, 3]"""
    part = np.zeros((M, 6, 256), F32)
    with np.errstate(**_quiet):
        for sel in L.sel:
            n, t, v = L.node[sel], L.thread[sel], L.pt[sel]
            uv = u[v]
            part[n, :, t] = part[n, :, t] + np.concatenate([L.w[sel, None] * uv, L.wn[sel, None] * R.cross3(a[v], uv)], 1)
        out = R.tree(part, 256)
        tau = out[:, :3]
        om = out[:, 3:] - R.cross3(q, tau)
        if p is not None:
            om, tau = om + F32(lam_rot) * p[:M], tau + F32(lam) * p[M:]
    return np.concatenate([om, tau]).astype(F32)


def edge_values(G, pos, dq, c):
    """g_e = T_i v_j - c_j and b_e = T_i v_j - c_i for the edge e = (i -> j)."""
    head = G.nbr.reshape(-1)
    Tij = R.dq_transform(dq[G.tail], pos[head])
    return (Tij - c[head]).astype(F32), (Tij - c[G.tail]).astype(F32)


def reg_sums(G, b, d):
    """[2M, 3]: the omega accumulators (+ alpha_e (b_e x d_e) over the outgoing edges in slot order), then the tau accumulators
    (Graph.node_sums of d)."""
    a = G.alpha.reshape(-1)
    om = np.zeros((G.M, 3), F32)
    with np.errstate(**_quiet):
        bxd = R.cross3(b, d)
        for s in range(G.kg):
            e = np.arange(G.M) * G.kg + s
            om = om + a[e, None] * bxd[e]
        return np.concatenate([om, G.node_sums(d)]).astype(F32)


def edge_step(G, b, p):
    """d_e = (p_tau_i + (p_om_i x b_e)) - p_tau_j."""
    M = G.M
    with np.errstate(**_quiet):
        return ((p[M:][G.tail] + R.cross3(p[:M][G.tail], b)) - p[M:][G.nbr.reshape(-1)]).astype(F32)


def write_back(dq, node_t, c, x):
    """The transforms a round writes: a node whose six update components are all exactly 0 keeps its eight floats."""
    M = len(dq)
    om, tau = x[:M], x[M:]
    with np.errstate(**_quiet):
        qo = R.q_normalize(np.concatenate([np.ones((M, 1), F32), F32(0.5) * om], 1).astype(F32))
        r1 = R.q_mul(qo, R.q_normalize(dq[:, :4])).astype(F32)
        zero_dual = np.zeros((M, 4), F32)
        t1 = (R.dq_transform(np.concatenate([qo, zero_dual], 1), node_t[:, 1:] - c) + c) + tau
        T = np.concatenate([np.zeros((M, 1), F32), t1], 1).astype(F32)
        new = np.concatenate([r1, R.q_mul(F32(0.5) * T, r1)], 1).astype(F32)
    keep = ~(x[:M] != 0).any(1) & ~(x[M:] != 0).any(1)
    return np.where(keep[:, None], dq, new).astype(F32)


def solve_rigid(pos, dq, sigma, canonical, live, normals, k, iters, lam=0.0, lam_rot=0.0, kg=0, lambda_reg=0.0, rounds=1, tukey_c=0.0,
                huber_delta=0.0, details=None):
    """`normals` None: the point-to-point data term.  `details` (a dict) receives wn, keys, lists, graph and per round the lists y, nw, c,
    e, rho, omega, omega_e, g, b, r0, x, dq, steps (the CG steps taken before the recurrence froze), and y_after / nw_after: the warp
    behind the last write-back."""
    pos, dq, sigma, canonical, live = R.f32(pos), R.f32(dq).reshape(-1, 8), R.f32(sigma), R.f32(canonical), R.f32(live)
    plane = normals is not None
    if plane:
        normals = R.f32(normals)
    M, N = len(pos), len(canonical)
    assert rounds >= 1 and (not plane or normals.shape == (N, 3))
    lam, lrot, lreg = F32(lam), F32(lam_rot), F32(lambda_reg)
    cc, delta = F32(tukey_c), F32(huber_delta)
    c2, d2 = cc * cc, delta * delta
    reg = kg > 0 and lreg != 0
    tukey, huber = cc != 0, bool(reg and delta != 0)
    G = R.Graph(pos, sigma, kg) if reg else None
    en = np.zeros(4, F32)
    omega, omega_e = np.ones(N, F32), (np.ones(M * kg, F32) if reg else None)
    log = dict(y=[], nw=[], c=[], q=[], a=[], e=[], rho=[], omega=[], omega_e=[], g=[], b=[], r0=[], x=[], dq=[], steps=[])
    zero = F32(0)

    def data_energy(e, rho):
        if plane:
            return P.data_energy(rho, tukey, c2)
        return RR.tukey_energy(e, c2) if tukey else R.energy_sum(e)

    def residual(y, nw):
        with np.errstate(**_quiet):
            e = np.where(valid[:, None], live - y, F32(0)).astype(F32)
        return e, (P.rho_of(nw, e, valid) if plane else None)

    def reg_energy(g):
        return RR.huber_energy(G, g, None, delta, d2) if huber else G.energy(g, np.zeros((M, 3), F32))

    for rnd in range(rounds):
        y, nw = warp(pos, dq, sigma, canonical, normals, k)
        if rnd == 0:
            w, wn, keys = rigid_setup(pos, sigma, canonical, live, normals, y, nw, k)
            valid = keys[:, 0] < M
            lists = R.NodeLists(keys, w, M, k)
            lists.wn = R.NodeLists(keys, wn, M, k).w
        node_t = R.node_translation(dq)
        c = node_centres(pos, dq)
        q = (c - node_t[:, 1:]).astype(F32)
        with np.errstate(**_quiet):
            a = np.where(valid[:, None], y - blend_translation(w, keys, node_t), F32(0)).astype(F32)
        e, rho = residual(y, nw)
        with np.errstate(**_quiet):
            rhs = np.where(valid[:, None], nw * rho[:, None], F32(0)).astype(F32) if plane else e
        L, Gw = lists, G
        if tukey:
            omega = P.tukey_weights(rho, c2) if plane else RR.tukey_weights(e, c2)
            L = copy.copy(lists)
            L.w, L.wn = (omega[lists.pt] * lists.w).astype(F32), (omega[lists.pt] * lists.wn).astype(F32)
        if rnd == 0:
            en[0] = data_energy(e, rho)
        r = jt_apply(L, M, a, q, rhs)
        g = b = None
        if reg:
            g, b = edge_values(G, pos, dq, c)
            if huber:
                omega_e = RR.huber_weights(g, delta, d2)
                Gw = copy.copy(G)
                Gw.alpha = (G.alpha.reshape(-1) * omega_e).astype(F32).reshape(G.alpha.shape)
            with np.errstate(**_quiet):
                r = (r - lreg * reg_sums(Gw, b, g)).astype(F32)
            if rnd == 0:
                en[2] = reg_energy(g)
        r0 = r.copy()
        x = np.zeros((2 * M, 3), F32)
        p = r.copy()
        rr = P.sum3(r * r)
        rr0 = rr
        steps = 0
        with np.errstate(**_quiet):
            for _ in range(iters):
                if not rr > 0:                       # frozen: the remaining steps change nothing
                    break
                steps += 1
                Ap = jt_apply(L, M, a, q, j_apply(w, wn, keys, M, a, q, p, nw if plane else None, valid), lam, lrot, p)
                if reg:
                    Ap = (Ap + lreg * reg_sums(Gw, b, edge_step(Gw, b, p))).astype(F32)
                pq = P.sum3(p * Ap)
                alpha = F32(rr / pq) if (pq > 0 and rr > 0) else zero
                x = x + alpha * p
                r = r - alpha * Ap
                rn = P.sum3(r * r)
                beta = F32(rn / rr) if (alpha != 0 and rr > 0) else zero
                p = r + beta * p
                rr = rn if (alpha != 0 and rn > F32(1.0e-10) * rr0) else zero
        dq = write_back(dq, node_t, c, x)
        for name, val in (("y", y), ("nw", nw), ("c", c), ("q", q), ("a", a), ("e", e), ("rho", rho), ("omega", omega.copy()), ("g", g), ("b", b), ("r0", r0),
                          ("omega_e", None if omega_e is None else omega_e.copy()), ("x", x), ("dq", dq), ("steps", steps)):
            log[name].append(val)
    y, nw = warp(pos, dq, sigma, canonical, normals, k)
    e, rho = residual(y, nw)
    en[1] = data_energy(e, rho)
    if reg:
        en[3] = reg_energy(edge_values(G, pos, dq, node_centres(pos, dq))[0])
    if details is not None:
        details.update(w=w, wn=wn, keys=keys, lists=lists, graph=G, valid=valid, y_after=y, nw_after=nw, e_after=e, **log)
    return dq, en, omega, (omega_e.reshape(M, kg) if reg else None)
