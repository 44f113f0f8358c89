"""numpy float32 restatement of the 6x6 node-block Jacobi preconditioner of the warp solve with rotations (dfusion_warp_set_preconditioner,
DESIGN.md 21), operation for operation, on the pieces of solver_rigid_ref: per round the diagonal 6x6 block of every node of the normal
matrix J^T Omega J + lambda_reg L + damping (unknown order omega_n, tau_n), its Cholesky factor in f32, and ONE preconditioned
conjugate-gradient recurrence over the 6M unknowns in which z = B^-1 r is two triangular substitutions per node.

    solve_rigid(pos, dq, sigma, canonical, live, normals, k, iters, lam, lam_rot, kg, lambda_reg, rounds, tukey_c, huber_delta, precond=1)
        -> (dq_out [M, 8], energy [4], point_weights [N], edge_weights [M, kg] or None)

precond = 0 is solver_rigid_ref.solve_rigid itself.

The block of node n, as 21 upper-triangle entries in row-major order (UP[i][j], i <= j; 0..2 = omega x y z, 3..5 = tau x y z).  Every
product is rounded before it is added.
  data   per entry (v, n) of the node's list, thread-strided and then the 256-tree (df_sv_rigid_jt_apply_kernel's walk), with w, wn the
         entry's weights, w', wn' their Tukey-scaled copies (the same numbers without Tukey), q = q_n, a = a_v:
             m = w q - wn a,   m' = w' q - wn' a
         point-to-point, ten sums:   P_cd += m'_c m_d (c <= d: xx xy xz yy yz zz),   K_c += w' m_c,   T += w' w;  then
             OO = [[Pyy + Pzz, -Pxy, -Pxz], [., Pxx + Pzz, -Pyz], [., ., Pxx + Pyy]],  OT = [[0, Kz, -Ky], [-Kz, 0, Kx], [Ky, -Kx, 0]],  TT = T I
         point-to-plane, 21 sums, n' the warped normal:   h = (n' x m, w n'),  h' = (n' x m', w' n'),   B_ij += h'_i h_j (i <= j)
  graph  (kg > 0) over the outgoing edges in slot order, alpha' the (Huber-scaled) edge weight, b = b_e:
             Q_cd += (alpha' b_c) b_d (c <= d),   KB_c += alpha' b_c,   AT += alpha';   then over the incoming edges in ascending edge id AT += alpha';
         OO entries + lambda_reg * (Qyy + Qzz, -Qxy, -Qxz, Qxx + Qzz, -Qyz, Qxx + Qyy),  OT off-diagonal + lambda_reg * (-KBz, KBy, KBz, -KBx, -KBy, KBx)
         in row order, TT diagonal + lambda_reg * AT
  damping  + lambda_rot on the diagonal of OO, + lambda on the diagonal of TT.
Cholesky B = L L^T by rows: for i, for j <= i:  s = B_ji; for k < j: s = s - L_ik L_jk;  L_ii = sqrt(s) (the pivot s must be > 0 and
finite), L_ij = s / L_jj.  A node with a failed pivot has the identity as its preconditioner.  z = B^-1 r:  y_i = (r_i - sum_k<i L_ik y_k) /
L_ii upwards, z_i = (y_i - sum_k>i L_ki z_k) / L_ii downwards, k ascending in both.
A dot product of the recurrence: thread t of 1024 owns nodes t, t + 1024, ...; per node and component it adds the omega product, then the
tau product; then the 1024-tree per component and (s0 + s1) + s2.
"""
import copy

import numpy as np

import solver_plane_ref as P
import solver_reg_ref as R
import solver_rigid_ref as G
import solver_robust_ref as RR

F32 = np.float32
_quiet = G._quiet


def up(i, j):
    """Index of entry (i, j), i <= j, among the 21 upper-triangle entries in row-major order."""
    return i * 6 - i * (i - 1) // 2 + (j - i)


def data_sums(lists, L, M, a, q, nw):
    """The node sums of the data term: [M, 10] (point-to-point, nw None) or [M, 21] (point-to-plane)."""
    S = 10 if nw is None else 21
    part = np.zeros((M, S, 256), F32)
    with np.errstate(**_quiet):
        for sel in lists.sel:
            n, t, v = lists.node[sel], lists.thread[sel], lists.pt[sel]
            w, wn, ws, wns = lists.w[sel, None], lists.wn[sel, None], L.w[sel, None], L.wn[sel, None]
            m = w * q[n] - wn * a[v]
            ms = ws * q[n] - wns * a[v]
            if nw is None:
                terms = [ms[:, 0] * m[:, 0], ms[:, 0] * m[:, 1], ms[:, 0] * m[:, 2], ms[:, 1] * m[:, 1], ms[:, 1] * m[:, 2], ms[:, 2] * m[:, 2],
                         ws[:, 0] * m[:, 0], ws[:, 0] * m[:, 1], ws[:, 0] * m[:, 2], ws[:, 0] * w[:, 0]]
            else:
                nv = nw[v]
                h = np.concatenate([R.cross3(nv, m), w * nv], 1)
                hs = np.concatenate([R.cross3(nv, ms), ws * nv], 1)
                terms = [hs[:, i] * h[:, j] for i in range(6) for j in range(i, 6)]
            part[n, :, t] = part[n, :, t] + np.stack(terms, 1).astype(F32)
        return R.tree(part, 256).astype(F32)


def _rotation_part(B, Pm, scale=None):
    """OO entries from the six sums xx xy xz yy yz zz of Pm [M, 6]: set (scale None) or + scale * value."""
    xx, xy, xz, yy, yz, zz = (Pm[:, i] for i in range(6))
    for (i, j), val in (((0, 0), yy + zz), ((0, 1), -xy), ((0, 2), -xz), ((1, 1), xx + zz), ((1, 2), -yz), ((2, 2), xx + yy)):
        B[:, up(i, j)] = val if scale is None else B[:, up(i, j)] + scale * val


def blocks(lists, L, M, a, q, nw, Gw, b, lam, lam_rot, lreg):
    """[M, 21]: every node's block (module docstring).  Gw None: no graph term."""
    s = data_sums(lists, L, M, a, q, nw)
    with np.errstate(**_quiet):
        if nw is None:
            B = np.zeros((M, 21), F32)
            _rotation_part(B, s[:, :6])
            kx, ky, kz = s[:, 6], s[:, 7], s[:, 8]
            for (i, j), val in (((0, 4), kz), ((0, 5), -ky), ((1, 3), -kz), ((1, 5), kx), ((2, 3), ky), ((2, 4), -kx)):
                B[:, up(i, j)] = val
            for i in (3, 4, 5):
                B[:, up(i, i)] = s[:, 9]
        else:
            B = s.copy()
        if Gw is not None:
            al = Gw.alpha.reshape(-1)
            Q, KB, AT = np.zeros((M, 6), F32), np.zeros((M, 3), F32), np.zeros(M, F32)
            for sl in range(Gw.kg):
                e = np.arange(M) * Gw.kg + sl
                ab = al[e, None] * b[e]
                be = b[e]
                Q = Q + np.stack([ab[:, 0] * be[:, 0], ab[:, 0] * be[:, 1], ab[:, 0] * be[:, 2], ab[:, 1] * be[:, 1], ab[:, 1] * be[:, 2],
                                  ab[:, 2] * be[:, 2]], 1)
                KB = KB + ab
                AT = AT + al[e]
            for r in range(int(Gw.in_deg.max()) if M else 0):
                n = np.flatnonzero(Gw.in_deg > r)
                AT[n] = AT[n] + al[Gw.in_edge[Gw.in_off[n] + r]]
            _rotation_part(B, Q, lreg)
            for (i, j), val in (((0, 4), -KB[:, 2]), ((0, 5), KB[:, 1]), ((1, 3), KB[:, 2]), ((1, 5), -KB[:, 0]), ((2, 3), -KB[:, 1]), ((2, 4), KB[:, 0])):
                B[:, up(i, j)] = B[:, up(i, j)] + lreg * val
            for i in (3, 4, 5):
                B[:, up(i, i)] = B[:, up(i, i)] + lreg * AT
        for i in (0, 1, 2):
            B[:, up(i, i)] = B[:, up(i, i)] + lam_rot
        for i in (3, 4, 5):
            B[:, up(i, i)] = B[:, up(i, i)] + lam
    return B.astype(F32)


def full_blocks(B):
    """[M, 21] -> [M, 6, 6] symmetric."""
    out = np.zeros((len(B), 6, 6), B.dtype)
    for i in range(6):
        for j in range(i, 6):
            out[:, i, j] = out[:, j, i] = B[:, up(i, j)]
    return out


def cholesky(B):
    """-> (L [M, 6, 6] lower, ok [M]): ok False where a pivot is not > 0 or not finite (that node's preconditioner is the identity)."""
    M = len(B)
    Lo = np.zeros((M, 6, 6), F32)
    ok = np.ones(M, bool)
    with np.errstate(**_quiet):
        for i in range(6):
            for j in range(i + 1):
                s = B[:, up(j, i)].copy()
                for k in range(j):
                    s = s - Lo[:, i, k] * Lo[:, j, k]
                if i == j:
                    ok &= (s > 0) & np.isfinite(s)
                    Lo[:, i, i] = np.sqrt(s)
                else:
                    Lo[:, i, j] = s / Lo[:, j, j]
    return Lo, ok


def apply(fac, r):
    """z = B^-1 r for r [2M, 3] (omega rows, then tau rows); the identity where the factorisation failed."""
    Lo, ok = fac
    M = len(ok)
    r6 = np.concatenate([r[:M], r[M:]], 1)
    y, z = np.zeros((M, 6), F32), np.zeros((M, 6), F32)
    with np.errstate(**_quiet):
        for i in range(6):
            t = r6[:, i].copy()
            for k in range(i):
                t = t - Lo[:, i, k] * y[:, k]
            y[:, i] = t / Lo[:, i, i]
        for i in range(5, -1, -1):
            t = y[:, i].copy()
            for k in range(i + 1, 6):
                t = t - Lo[:, k, i] * z[:, k]
            z[:, i] = t / Lo[:, i, i]
    z = np.where(ok[:, None], z, r6).astype(F32)
    return np.concatenate([z[:, :3], z[:, 3:]]).astype(F32)


def node_dot(u, v):
    """A dot product of the preconditioned recurrence over [2M, 3] arrays (module docstring)."""
    M = len(u) // 2
    with np.errstate(**_quiet):
        prod = (u * v).astype(F32)
        part = np.zeros((1024, 3), F32)
        for lo in range(0, M, 1024):
            n = min(M, lo + 1024) - lo
            part[:n] = part[:n] + prod[lo:lo + n]
            part[:n] = part[:n] + prod[M + lo:M + lo + n]
        s = R.tree(np.ascontiguousarray(part.T), 1024)
        return F32((s[0] + s[1]) + s[2])


def solve_rigid(pos, dq, sigma, canonical, live, normals, k, iters, lam=0.0, lam_rot=0.0, kg=0, lambda_reg=0.0, rounds=1, tukey_c=0.0,
                huber_delta=0.0, details=None, precond=1):
    """solver_rigid_ref.solve_rigid with the node blocks as preconditioner.  `details` receives what that one's does and per round
    `blocks` [M, 21] and `factored` [M] (False: the identity)."""
    if not precond:
        return G.solve_rigid(pos, dq, sigma, canonical, live, normals, k, iters, lam, lam_rot, kg, lambda_reg, rounds, tukey_c, huber_delta, details)
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
    Gr = R.Graph(pos, sigma, kg) if reg else None
    en = np.zeros(4, F32)
    omega, omega_e = np.ones(N, F32), (np.ones(M * kg, F32) if reg else None)
    log = dict(y=[], nw=[], c=[], q=[], a=[], e=[], rho=[], omega=[], omega_e=[], g=[], b=[], r0=[], x=[], dq=[], steps=[], blocks=[], factored=[])
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
        return RR.huber_energy(Gr, g, None, delta, d2) if huber else Gr.energy(g, np.zeros((M, 3), F32))

    for rnd in range(rounds):
        y, nw = G.warp(pos, dq, sigma, canonical, normals, k)
        if rnd == 0:
            w, wn, keys = G.rigid_setup(pos, sigma, canonical, live, normals, y, nw, k)
            valid = keys[:, 0] < M
            lists = R.NodeLists(keys, w, M, k)
            lists.wn = R.NodeLists(keys, wn, M, k).w
        node_t = R.node_translation(dq)
        c = G.node_centres(pos, dq)
        q = (c - node_t[:, 1:]).astype(F32)
        with np.errstate(**_quiet):
            a = np.where(valid[:, None], y - G.blend_translation(w, keys, node_t), F32(0)).astype(F32)
        e, rho = residual(y, nw)
        with np.errstate(**_quiet):
            rhs = np.where(valid[:, None], nw * rho[:, None], F32(0)).astype(F32) if plane else e
        L, Gw = lists, Gr
        if tukey:
            omega = P.tukey_weights(rho, c2) if plane else RR.tukey_weights(e, c2)
            L = copy.copy(lists)
            L.w, L.wn = (omega[lists.pt] * lists.w).astype(F32), (omega[lists.pt] * lists.wn).astype(F32)
        if rnd == 0:
            en[0] = data_energy(e, rho)
        r = G.jt_apply(L, M, a, q, rhs)
        g = b = None
        if reg:
            g, b = G.edge_values(Gr, pos, dq, c)
            if huber:
                omega_e = RR.huber_weights(g, delta, d2)
                Gw = copy.copy(Gr)
                Gw.alpha = (Gr.alpha.reshape(-1) * omega_e).astype(F32).reshape(Gr.alpha.shape)
            with np.errstate(**_quiet):
                r = (r - lreg * G.reg_sums(Gw, b, g)).astype(F32)
            if rnd == 0:
                en[2] = reg_energy(g)
        B = blocks(lists, L, M, a, q, nw if plane else None, Gw, b, lam, lrot, lreg)
        fac = cholesky(B)
        r0 = r.copy()
        x = np.zeros((2 * M, 3), F32)
        z = apply(fac, r)
        p = z.copy()
        rz = node_dot(r, z)
        rz0 = rz
        steps = 0
        with np.errstate(**_quiet):
            for _ in range(iters):
                if not rz > 0:                       # frozen: the remaining steps change nothing
                    break
                steps += 1
                Ap = G.jt_apply(L, M, a, q, G.j_apply(w, wn, keys, M, a, q, p, nw if plane else None, valid), lam, lrot, p)
                if reg:
                    Ap = (Ap + lreg * G.reg_sums(Gw, b, G.edge_step(Gw, b, p))).astype(F32)
                pq = node_dot(p, Ap)
                alpha = F32(rz / pq) if (pq > 0 and rz > 0) else zero
                x = x + alpha * p
                r = r - alpha * Ap
                z = apply(fac, r)
                rn = node_dot(r, z)
                beta = F32(rn / rz) if (alpha != 0 and rz > 0) else zero
                p = z + beta * p
                rz = rn if (alpha != 0 and rn > F32(1.0e-10) * rz0) else zero
        dq = G.write_back(dq, node_t, c, x)
        for name, val in (("y", y), ("nw", nw), ("c", c), ("q", q), ("a", a), ("e", e), ("rho", rho), ("omega", omega.copy()), ("g", g), ("b", b), ("r0", r0),
                          ("omega_e", None if omega_e is None else omega_e.copy()), ("x", x), ("dq", dq), ("steps", steps), ("blocks", B),
                          ("factored", fac[1])):
            log[name].append(val)
    y, nw = G.warp(pos, dq, sigma, canonical, normals, k)
    e, rho = residual(y, nw)
    en[1] = data_energy(e, rho)
    if reg:
        en[3] = reg_energy(G.edge_values(Gr, pos, dq, G.node_centres(pos, dq))[0])
    if details is not None:
        details.update(w=w, wn=wn, keys=keys, lists=lists, graph=Gr, valid=valid, y_after=y, nw_after=nw, e_after=e, **log)
    return dq, en, omega, (omega_e.reshape(M, kg) if reg else None)
