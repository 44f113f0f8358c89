"""numpy float32 restatement of the warp solver with the regularisation term (dfusion_warp_solve), operation for
operation: every product and every sum is rounded to float32 where the kernels of dynamicfusion_amd/csrc/dfusion_solver.hip round it, and
every sum runs in their order (thread-strided partial sums, the 256- and 1024-trees, slot order, ascending edge ids).  With kg = 0 it is
oracle/dfusion_frontend_oracle.c's orc_solve_data_term (tests/test_solver_reg_rule.py pins that bit for bit); the k-NN is the oracle's.

    solve(pos, dq, sigma, canonical, live, k, iters, lam, kg, lambda_reg) -> (dq_out [M, 8], energy [4])
    node_graph(pos, sigma, kg) -> (nbr int32 [M, kg], alpha [M, kg])
"""
import math

import numpy as np

import oracle_lib as O

F32 = np.float32
_exp = np.frompyfunc(math.exp, 1, 1)          # the C library's double exp, as the oracle calls it


def f32(a):
    return np.ascontiguousarray(a, F32)


# ---------------------------------------------------------------------------------------------- quaternions (dfusion_device.h)
def q_mul(a, b):
    aw, ax, ay, az = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bw, bx, by, bz = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([((aw * bw) - (ax * bx) - (ay * by) - (az * bz)),
                     ((aw * bx) + (ax * bw) + (ay * bz) - (az * by)),
                     ((aw * by) - (ax * bz) + (ay * bw) + (az * bx)),
                     ((aw * bz) + (ax * by) - (ay * bx) + (az * bw))], -1)


def q_conj(a):
    return a * np.array([1, -1, -1, -1], F32)


def q_normalize(a):
    """quaternion.hpp:211-228: (1.0 / norm) * q with a double scalar, rounded per component."""
    n = np.sqrt((a[..., 0] * a[..., 0]) + (a[..., 1] * a[..., 1]) + (a[..., 2] * a[..., 2]) + (a[..., 3] * a[..., 3]))
    inv = 1.0 / n.astype(np.float64)
    return (inv[..., None] * a.astype(np.float64)).astype(F32)


def node_translation(dq):
    """dual_quaternion.hpp:120-125 getTranslation(): (w, x, y, z)."""
    return q_mul(F32(2) * dq[..., 4:], q_conj(q_normalize(dq[..., :4])))


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def dq_transform(dq, p):
    """dq_transform of dfusion_device.h (dual_quaternion.hpp:204-210 + quaternion.hpp:124-130) for rows of dq [.., 8] and p [.., 3]."""
    rn = q_normalize(dq[..., :4])
    t = q_mul(F32(2) * dq[..., 4:], q_conj(rn))
    qv = rn[..., 1:]
    inner = cross3(qv, p) + p * rn[..., :1]
    p = p + cross3(qv * F32(2), inner)
    return p + t[..., 1:]


# ---------------------------------------------------------------------------------------------- the fixed sum orders
def tree(part, width):
    """part [.., width]: pairs (t, t + s), s = width / 2 .. 1."""
    part = part.copy()
    s = width // 2
    while s >= 1:
        part[..., :s] = part[..., :s] + part[..., s:2 * s]
        s //= 2
    return part[..., 0]


def strided_sum1024(v):
    """v [n, C]: thread t of 1024 owns rows t, t + 1024, ... (summed in that order from 0), then the 1024-tree.  -> [C]"""
    n, C = v.shape
    rounds = max(1, -(-n // 1024))
    pad = np.zeros((rounds * 1024, C), F32)
    pad[:n] = v
    pad = pad.reshape(rounds, 1024, C)
    part = np.zeros((1024, C), F32)
    for r in range(rounds):
        part = part + pad[r]            # (a padded +0 changes nothing: a partial is never -0)
    return tree(np.ascontiguousarray(part.T), 1024)


def energy_sum(e):
    """df_sv_energy_kernel over rows of three components."""
    s = strided_sum1024(e * e)
    return (s[0] + s[1]) + s[2]


class NodeLists:
    """W^T as the kernels walk it: the valid entries sorted stably by node, 256 threads a node."""

    def __init__(self, keys, w, M, k):
        flat = keys.reshape(-1)
        valid = np.flatnonzero(flat < M)
        order = valid[np.argsort(flat[valid], kind="stable")]
        node = flat[order].astype(np.int64)
        cnt = np.bincount(node, minlength=M)
        off = np.concatenate([[0], np.cumsum(cnt)])
        rank = np.arange(len(order)) - off[node]
        self.M = M
        self.pt = order // k
        self.w = w.reshape(-1)[order]
        self.node, self.thread, self.round = node, rank % 256, rank // 256
        self.rounds = int(self.round.max()) + 1 if len(order) else 0
        self.sel = [np.flatnonzero(self.round == r) for r in range(self.rounds)]

    def apply(self, u, lam=None, p=None):
        part = np.zeros((self.M, 3, 256), F32)
        for sel in self.sel:
            n, t = self.node[sel], self.thread[sel]
            part[n, :, t] = part[n, :, t] + self.w[sel, None] * u[self.pt[sel]]
        out = tree(part, 256)
        if p is not None:
            out = out + F32(lam) * p
        return out


def w_apply(w, keys, M, p):
    N, k = w.shape
    s = np.zeros((N, 3), F32)
    for j in range(k):
        ok = keys[:, j] < M
        n = np.where(ok, keys[:, j], 0)
        s = np.where(ok[:, None], s + w[:, j, None] * p[n], s)
    return s


# ---------------------------------------------------------------------------------------------- the node graph
def node_graph(pos, sigma, kg):
    """Node i's kg nearest other nodes: the (kg + 1)-NN of its position in nanoflann's tie order without the entry whose id is i -- or
    without the last entry when none is.  alpha = max(sigma_i, sigma_j)."""
    pos, sigma = f32(pos), f32(sigma)
    M = len(pos)
    assert 1 <= kg <= 7 and M >= kg + 1
    idx, _ = O.knn(pos, pos, kg + 1)
    nbr = np.empty((M, kg), np.int32)
    for i in range(M):
        row = idx[i].tolist()
        drop = row.index(i) if i in row else kg
        nbr[i] = row[:drop] + row[drop + 1:]
    alpha = np.maximum(sigma[:, None], sigma[nbr])
    return nbr, alpha


class Graph:
    def __init__(self, pos, sigma, kg):
        self.nbr, self.alpha = node_graph(pos, sigma, kg)
        self.M, self.kg = len(pos), kg
        head = self.nbr.reshape(-1)
        self.tail = np.repeat(np.arange(self.M), kg)
        self.in_edge = np.argsort(head, kind="stable")           # per head node: ascending edge ids
        self.in_off = np.concatenate([[0], np.cumsum(np.bincount(head, minlength=self.M))])
        self.in_deg = np.diff(self.in_off)

    def node_sums(self, d):
        """d [M * kg, 3] edge values -> acc [M, 3]: + alpha_e d_e over the outgoing edges in slot order, then - alpha_e d_e over the
        incoming edges in ascending edge id; every product rounded before it is added."""
        a = self.alpha.reshape(-1)
        acc = np.zeros((self.M, 3), F32)
        for s in range(self.kg):
            e = np.arange(self.M) * self.kg + s
            acc = acc + a[e, None] * d[e]
        for r in range(int(self.in_deg.max()) if self.M else 0):
            n = np.flatnonzero(self.in_deg > r)
            e = self.in_edge[self.in_off[n] + r]
            acc[n] = acc[n] - a[e, None] * d[e]
        return acc

    def edge_diff(self, p):
        return p[self.tail] - p[self.nbr.reshape(-1)]

    def energy(self, g, x):
        h = (g + x[self.tail]) - x[self.nbr.reshape(-1)]
        s = strided_sum1024(self.alpha.reshape(-1, 1) * (h * h))
        return (s[0] + s[1]) + s[2]


# ---------------------------------------------------------------------------------------------- the solve
def setup(pos, dq, sigma, canonical, live, k):
    """df_sv_setup_kernel: (w [N, k], keys [N, k] (M = invalid), e0 [N, 3], node_t [M, 4])."""
    M, N = len(pos), len(canonical)
    node_t = node_translation(dq)
    idx, d2 = O.knn(pos, canonical, k)
    valid = ~(np.isnan(canonical).any(1) | np.isnan(live).any(1))
    keys = np.where(valid[:, None], idx, M).astype(np.int64)
    w = np.zeros((N, k), F32)
    s = np.zeros((N, 3), F32)
    with np.errstate(all="ignore"):                  # (the k-NN of a NaN point holds anything: masked by `valid`)
        for j in range(k):
            sg = sigma[np.where(valid, idx[:, j], 0)]
            arg = (-d2[:, j] / (F32(2) * sg * sg)).astype(np.float64)
            wj = np.where(valid, _exp(np.where(valid, arg, 0.0)).astype(np.float64).astype(F32), F32(0)).astype(F32)
            w[:, j] = wj
            t = node_t[np.where(valid, idx[:, j], 0)]
            s = np.where(valid[:, None], s + wj[:, None] * t[:, 1:], s)
        e0 = np.where(valid[:, None], (live - canonical) - s, F32(0)).astype(F32)
    return w, keys, e0, node_t


def solve(pos, dq, sigma, canonical, live, k, iters, lam=0.0, kg=0, lambda_reg=0.0, details=None):
    """Returns (dq_out [M, 8], energy [E_data before, E_data after, E_reg before, E_reg after]).  `details` (a dict) receives the
    pieces: w, keys, e0, x (= delta), and with regularisation graph and g."""
    pos, dq, sigma, canonical, live = f32(pos), f32(dq).reshape(-1, 8), f32(sigma), f32(canonical), f32(live)
    M = len(pos)
    lam, lreg = F32(lam), F32(lambda_reg)
    reg = kg > 0 and lreg != 0
    w, keys, e0, node_t = setup(pos, dq, sigma, canonical, live, k)
    lists = NodeLists(keys, w, M, k)
    en = np.zeros(4, F32)
    en[0] = energy_sum(e0)
    r = lists.apply(e0)
    if reg:
        G = Graph(pos, sigma, kg)
        vj = pos[G.nbr.reshape(-1)]
        g = dq_transform(dq[G.tail], vj) - dq_transform(dq[G.nbr.reshape(-1)], vj)
        r = r - lreg * G.node_sums(g)
        en[2] = G.energy(g, np.zeros((M, 3), F32))
    x = np.zeros((M, 3), F32)
    p = r.copy()
    rr = strided_sum1024(r * r)
    rr0 = rr.copy()
    zero = F32(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        for _ in range(iters):
            if not (rr > 0).any():                   # every component frozen: the remaining steps change nothing
                break
            q = lists.apply(w_apply(w, keys, M, p), lam, p)
            if reg:
                q = q + lreg * G.node_sums(G.edge_diff(p))
            pq = strided_sum1024(p * q)
            alpha = np.where((pq > 0) & (rr > 0), rr / pq, zero).astype(F32)
            x = x + alpha * p
            r = r - alpha * q
            rn = strided_sum1024(r * r)
            beta = np.where((alpha != 0) & (rr > 0), rn / rr, zero).astype(F32)
            p = r + beta * p
            rr = np.where((alpha != 0) & (rn > F32(1.0e-10) * rr0), rn, zero).astype(F32)
    en[1] = energy_sum(e0 - w_apply(w, keys, M, x))
    if reg:
        en[3] = G.energy(g, x)
    # encodeTranslation (dual_quaternion.hpp:82-85): 0.5 * (0, T) * rotation_
    T = np.concatenate([np.zeros((M, 1), F32), node_t[:, 1:] + x], 1)
    out = np.concatenate([dq[:, :4], q_mul(F32(0.5) * T, dq[:, :4])], 1).astype(F32)
    if details is not None:
        details.update(w=w, keys=keys, e0=e0, x=x, lists=lists)
        if reg:
            details.update(graph=G, g=g)
    return out, en
