"""numpy restatement of the warp-field extension rule (include/dfusion.h dfusion_warp_extend), on the oracle's k-NN and DQB.

    unsupported p : p finite, M >= k, and d2_i >= sigma_i * sigma_i (f32) for each of p's k nearest nodes (O.knn: nanoflann's order)
    cell of p     : (int)floorf(p / radius) per axis, f32 division; |p / radius| >= 2^30 on an axis -> p takes no part
    winner        : the lowest unsupported point index of its cell; winners are appended in increasing index, at most
                    min(max_new, 65535 - M) of them
    new node      : vertex = p, dg_w = sigma_new, transform = O.dqb(p) over the old nodes -- or, when all k weights
                    (float)exp((double)(-d2 / (2 sigma sigma))) are 0, the transform of p's nearest node
"""
import numpy as np

import oracle_lib as O

F32 = np.float32
CELL_LIM = F32(2.0 ** 30)
MAX_NODES = 65535


def cells(points, radius):
    """(valid [N] bool, cell [N,3] int64): the grid cell of every point and whether it may take part at all."""
    p = np.ascontiguousarray(points, F32).reshape(-1, 3)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        f = p / F32(radius)
        valid = (np.abs(f) < CELL_LIM).all(1)
    c = np.zeros(p.shape, np.int64)
    c[valid] = np.floor(f[valid]).astype(np.int64)
    return valid, c


def decimate(points, candidate, radius):
    """Indices (ascending) of the points that win their cell: the lowest candidate index per cell."""
    valid, c = cells(points, radius)
    ids = np.nonzero(np.asarray(candidate, bool) & valid)[0]
    if ids.size == 0:
        return ids.astype(np.int64)
    _, first = np.unique(c[ids], axis=0, return_index=True)     # first occurrence = lowest index (ids ascending)
    return np.sort(ids[first])


def weights(d2, s):
    d2, s = np.asarray(d2, F32), np.asarray(s, F32)
    return np.exp(((-d2) / ((F32(2) * s) * s)).astype(np.float64)).astype(F32)


def unsupported(pos, sigma, points, k):
    """(mask [N], idx [N,k], d2 [N,k]) for finite points; the k-NN of non-finite points is that of the origin and never used."""
    p = np.ascontiguousarray(points, F32).reshape(-1, 3)
    fin = np.isfinite(p).all(1)
    q = np.where(fin[:, None], p, F32(0))
    idx, d2 = O.knn(pos, q, k)
    s = np.asarray(sigma, F32)[idx]
    return fin & (d2 >= s * s).all(1), idx, d2


def extend_ref(pos, dq, sigma, points, k, radius, sigma_new, max_new=None):
    """Returns (new_pos [n,3], new_dq [n,8], new_sigma [n], n_added, n_winners)."""
    pos, dq, sigma = np.asarray(pos, F32).reshape(-1, 3), np.asarray(dq, F32).reshape(-1, 8), np.asarray(sigma, F32).reshape(-1)
    p = np.ascontiguousarray(points, F32).reshape(-1, 3)
    M = pos.shape[0]
    cap = MAX_NODES - M if max_new is None else min(int(max_new), MAX_NODES - M)
    if p.shape[0] == 0:
        return np.zeros((0, 3), F32), np.zeros((0, 8), F32), np.zeros(0, F32), 0, 0
    mask, idx, d2 = unsupported(pos, sigma, p, k)
    win = decimate(p, mask, radius)
    take = win[:max(cap, 0)]
    n = take.size
    new_pos = p[take].copy()
    new_dq = O.dqb(pos, dq, sigma, new_pos, k) if n else np.zeros((0, 8), F32)
    zero = (weights(d2[take], sigma[idx[take]]) == 0).all(1)
    new_dq[zero] = dq[idx[take][zero, 0]]
    return new_pos, new_dq, np.full(n, sigma_new, F32), int(n), int(win.size)
