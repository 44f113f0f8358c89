"""numpy float32 restatement of the hierarchical node graph of the regularised warp solves (dfusion_warp_set_graph_hierarchy, DESIGN.md
13; dynamicfusion_amd/csrc/dfusion_warp_graph.hip), operation for operation:

    levels(pos, kg, L, radius, beta) -> (members, top int32 [M], sizes int32 [9], effective)
    hier_graph(pos, sigma, kg, L, radius, beta) -> (nbr int32 [M, kg], alpha [M, kg])
    HierGraph(pos, sigma, kg, L, radius, beta): solver_reg_ref.Graph over those edges
    with hierarchy(L, radius, beta): ...    # solver_reg_ref.Graph is HierGraph with this setting: the four solve restatements
                                            # (solver_reg_ref, solver_robust_ref, solver_plane_ref, solver_rigid_ref) run over it unchanged

With an effective depth of 0 the graph is solver_reg_ref.node_graph's (the flat graph, the oracle's k-NN)."""
import contextlib

import numpy as np

import solver_reg_ref as R

F32 = np.float32
MAX_LEVELS = 8
CELL_LIM = F32(2.0 ** 30)


def cell_edges(L, radius, beta):
    """c_1 = radius, c_{l+1} = f32(c_l * beta), up to the first that is not finite."""
    out, c = [], F32(radius)
    with np.errstate(over="ignore"):
        for _ in range(L):
            if not np.isfinite(c):
                break
            out.append(c)
            c = F32(c * F32(beta))
    return out


def decimate(pos, members, c):
    """The members of the next level: among `members` (ascending node ids) the lowest id of every cell floorf(p / c); a node with a
    non-finite coordinate or |p / c| >= 2^30 on an axis takes no part."""
    with np.errstate(all="ignore"):
        f = pos[members] / F32(c)                          # IEEE f32 division
        ok = (np.abs(f) < CELL_LIM).all(1)                 # (NaN and inf fail this)
        cell = np.floor(np.where(ok[:, None], f, F32(0))).astype(np.int64)
    seen, keep = set(), []
    for m in np.flatnonzero(ok):
        key = (int(cell[m, 0]), int(cell[m, 1]), int(cell[m, 2]))
        if key not in seen:
            seen.add(key)
            keep.append(int(members[m]))
    return np.array(keep, np.int64)


def levels(pos, kg, L, radius, beta):
    """(members: [S_0 .. S_L] ascending node ids (empty where the cell edge overflowed), top int32 [M] clamped to the effective depth,
    sizes int32 [9], effective depth L')."""
    pos = R.f32(pos)
    M = len(pos)
    assert 1 <= kg <= 7 and 1 <= L <= MAX_LEVELS and M >= kg + 1
    members = [np.arange(M, dtype=np.int64)]
    for c in cell_edges(L, radius, beta):
        members.append(decimate(pos, members[-1], c))
    while len(members) < L + 1:
        members.append(np.zeros(0, np.int64))
    sizes = np.zeros(MAX_LEVELS + 1, np.int32)
    sizes[:L + 1] = [len(m) for m in members]
    eff = max(l for l in range(L + 1) if sizes[l] >= kg + 1)
    top = np.zeros(M, np.int32)
    for l in range(1, eff + 1):
        top[members[l]] = l
    return members, top, sizes, eff


def nearest(pos, queries, cands, kg):
    """[len(queries), kg]: per query node its kg nearest of `cands` (ascending node ids) without itself, by (d2, node id); d2 =
    (dx dx + dy dy) + dz dz in f32, query minus candidate; NaN after every finite d2, in id order."""
    out = np.empty((len(queries), kg), np.int32)
    with np.errstate(all="ignore"):
        for a in range(0, len(queries), 256):
            q = queries[a:a + 256]
            d = pos[q][:, None, :] - pos[cands][None, :, :]
            dd = d * d
            d2 = (dd[..., 0] + dd[..., 1]) + dd[..., 2]
            for r, i in enumerate(q):
                order = np.argsort(d2[r], kind="stable")       # (stable: ties and the NaNs at the end stay in id order)
                order = order[cands[order] != i]
                out[a + r] = cands[order[:kg]]
    return out


def hier_graph(pos, sigma, kg, L, radius, beta):
    pos, sigma = R.f32(pos), R.f32(sigma)
    members, top, _, eff = levels(pos, kg, L, radius, beta)
    if eff == 0:
        return R.node_graph(pos, sigma, kg)
    target = np.minimum(top + 1, eff)
    nbr = np.empty((len(pos), kg), np.int32)
    for t in range(1, eff + 1):
        q = np.flatnonzero(target == t)
        nbr[q] = nearest(pos, q, members[t], kg)
    return nbr, np.maximum(sigma[:, None], sigma[nbr])


class HierGraph(R.Graph):
    def __init__(self, pos, sigma, kg, L, radius, beta):
        self.nbr, self.alpha = hier_graph(pos, sigma, kg, L, radius, beta)
        self.M, self.kg = len(pos), kg
        head = self.nbr.reshape(-1)                                  # the transpose: as solver_reg_ref.Graph makes it
        self.tail = np.repeat(np.arange(self.M), kg)
        self.in_edge = np.argsort(head, kind="stable")
        self.in_off = np.concatenate([[0], np.cumsum(np.bincount(head, minlength=self.M))])
        self.in_deg = np.diff(self.in_off)


@contextlib.contextmanager
def hierarchy(L, radius, beta=4.0):
    """Inside, solver_reg_ref.Graph(pos, sigma, kg) is the hierarchical graph of this setting (L = 0: untouched)."""
    if L == 0:
        yield
        return
    flat = R.Graph
    R.Graph = lambda pos, sigma, kg: HierGraph(pos, sigma, kg, L, radius, beta)
    try:
        yield
    finally:
        R.Graph = flat


def chain(M=120, step=0.025, n=1500, reach=0.5, shift=0.02):
    """The behaviour case: M nodes `step` apart along x (dg_w = step, identity transforms); n points over the first `reach` metres, a
    little off the axis, all moved by `shift` along x."""
    pos = np.zeros((M, 3), F32)
    pos[:, 0] = np.arange(M, dtype=F32) * F32(step)
    rng = np.random.default_rng(5)
    src = np.stack([rng.uniform(0, reach, n), rng.uniform(-0.01, 0.01, n), rng.uniform(-0.01, 0.01, n)], 1).astype(F32)
    dst = src.copy()
    dst[:, 0] += F32(shift)
    dq = np.zeros((M, 8), F32)
    dq[:, 0] = 1
    return pos, dq, np.full(M, step, F32), src, dst
