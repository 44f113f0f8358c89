"""GPU parity of the hierarchical node graph (dfusion_warp_set_graph_hierarchy, dfusion_warp_graph_levels) with the numpy
restatement tests/solver_hier_ref.py, which tests/test_solver_hier_rule.py checks on the CPU: the levels (top, sizes, effective depth) and
the edges (ids and alpha bits), then all 8 M floats of the transforms, the energies and the weights of the four regularised solves over
that graph, bit for bit; the fallback to the flat graph; the LDS tile edge of the subset k-NN; the graph's lifetime across extend; the
off switch; argument checks."""
import numpy as np
import pytest
import torch

import solver_hier_ref as H
import solver_plane_ref as P
import solver_reg_ref as R
import solver_rigid_ref as G
import solver_robust_ref as RR
from dynamicfusion_amd import capi
from solver_cases import (DF_E_INVALID, HUBER_DELTA, ITERS, LAM, LREG, LROT, TUKEY_C, assert_same, bits, dev, field, problem, random_nodes,
                          seeded_normals)

pytestmark = pytest.mark.gpu
F32 = np.float32
NPTS = 1503


# ------------------------------------------------------------------------------------------------ node sets and settings
def lattice():
    ax = np.arange(4, dtype=F32) * F32(0.25)
    return np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3).astype(F32)


def two_cells():
    pos = np.random.default_rng(2).uniform(0.1, 0.8, (6, 3)).astype(F32)
    pos[::2, 0] += F32(0.9)
    return pos


def with_nan():
    pos = np.random.default_rng(6).uniform(-1, 1, (40, 3)).astype(F32)
    pos[0, 1] = np.nan
    return pos


_tile = {}


def tile_edge(target):
    """400 random nodes and the first radius of a fixed scan at which the restatement counts `target` members in S_1."""
    if target not in _tile:
        pos = random_nodes(400, seed=target)
        for radius in np.linspace(0.40, 0.15, 4001).astype(F32):
            if len(H.decimate(pos, np.arange(400), radius)) == target:
                break
        else:
            raise AssertionError("no radius of the scan gives |S_1| = %d" % target)
        _tile[target] = (pos, float(radius))
    return _tile[target]


# name: (nodes, k, kg, (levels, radius, beta), expected effective depth or None)
CASES = {
    "chain": (lambda: H.chain()[0], 4, 4, (4, 0.05, 4.0), 2),
    "M6-fallback": (two_cells, 4, 4, (3, 0.9, 4.0), 0),
    "one-cell": (lambda: np.random.default_rng(3).uniform(0.1, 0.9, (50, 3)).astype(F32), 8, 4, (4, 1.0, 4.0), 0),
    "lattice": (lattice, 8, 4, (2, 0.5, 2.0), 1),
    "duplicate": (lambda: np.random.default_rng(3).uniform(-1, 1, (30, 3)).astype(F32)[np.r_[0:30, 4]], 8, 3, (2, 0.5, 2.0), None),
    "nan": (with_nan, 8, 4, (2, 0.5, 2.0), None),
    "S1-255": (lambda: tile_edge(255)[0], 8, 4, lambda: (2, tile_edge(255)[1], 3.0), 2),
    "S1-256": (lambda: tile_edge(256)[0], 8, 4, lambda: (2, tile_edge(256)[1], 3.0), 2),
    "S1-257": (lambda: tile_edge(257)[0], 8, 7, lambda: (2, tile_edge(257)[1], 3.0), 2),
    "M2049": (lambda: random_nodes(2049), 8, 4, (3, 0.2, 2.5), 3),
    "M8193": (lambda: random_nodes(8193), 8, 4, (8, 0.15, 2.5), None),
}
SOLVES = ["solve", "robust", "plane", "rigid"]
_made = {}


def case(name):
    """(pos, k, kg, setting, sigma, dq, src, dst, normals, reference graph), made once per case.  Nobody writes to it."""
    if name not in _made:
        nodes, k, kg, setting, eff = CASES[name]
        pos = nodes()
        setting = setting() if callable(setting) else setting
        if name == "chain":
            _, dq, sigma, src, dst = H.chain()
        else:
            sigma, dq, src, dst = problem(pos, NPTS)
        graph = H.HierGraph(pos, sigma, kg, *setting)
        _made[name] = (pos, k, kg, setting, sigma, dq, src, dst, seeded_normals(len(src)), graph, eff)
    return _made[name]


def hier_field(pos, sigma, dq, k, setting):
    wf = field(pos, sigma, dq, k)
    wf.set_graph_hierarchy(*setting)
    return wf


@pytest.mark.parametrize("name", list(CASES))
def test_levels_and_graph_equal_the_restatement(name):
    pos, k, kg, setting, sigma, dq, _, _, _, graph, want_eff = case(name)
    M = len(pos)
    wf = hier_field(pos, sigma, dq, k, setting)
    nbr, alpha = wf.node_graph(kg)
    top, sizes, eff = wf.graph_levels(kg)
    torch.cuda.synchronize()
    members, r_top, r_sizes, r_eff = H.levels(pos, kg, *setting)
    print("%s: M %d, sizes %s, effective %d, largest in-degree %d" % (name, M, r_sizes.tolist(), r_eff, int(graph.in_deg.max())))
    assert want_eff is None or r_eff == want_eff
    if name.startswith("S1-"):
        assert r_sizes[1] == int(name[3:])
    if name == "M8193":
        assert (r_sizes[1:9] > 0).all() and r_eff == 8       # eight levels made; from the fifth on a node per sign octant
    assert np.array_equal(sizes.cpu().numpy(), r_sizes) and int(eff.item()) == r_eff
    assert np.array_equal(top.cpu().numpy(), r_top)
    assert np.array_equal(nbr.cpu().numpy(), graph.nbr)
    assert np.array_equal(bits(alpha.cpu().numpy()), bits(graph.alpha))
    flat, flat_alpha = field(pos, sigma, dq, k).node_graph(kg)
    torch.cuda.synchronize()
    if r_eff == 0:                                           # the fallback: the flat graph of the same node set, bit for bit
        assert np.array_equal(nbr.cpu().numpy(), flat.cpu().numpy()) and np.array_equal(bits(alpha.cpu().numpy()), bits(flat_alpha.cpu().numpy()))
    else:
        assert not np.array_equal(nbr.cpu().numpy(), flat.cpu().numpy())
    if name == "nan":
        assert 0 not in members[1] and r_top[0] == 0 and graph.nbr[0].tolist() == members[1][:4].tolist()


def run_gpu(wf, kind, src, dst, nrm, k, kg, iters, lreg):
    kw = dict(iters=iters, lam=LAM, reg_neighbours=kg, reg_lambda=lreg, k=k)
    rob = dict(rounds=2, tukey_c=TUKEY_C, huber_delta=HUBER_DELTA, return_weights=True)
    if kind == "solve":
        out = wf.solve(dev(src), dev(dst), **kw) + (None, None)
    elif kind == "robust":
        out = wf.solve_robust(dev(src), dev(dst), **kw, **rob)
    elif kind == "plane":
        out = wf.solve_plane(dev(src), dev(dst), dev(nrm), **kw, **rob)
    else:
        out = wf.solve_rigid(dev(src), dev(dst), dev(nrm), lam_rot=LROT, **kw, **rob)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in out]


def restated(kind, pos, dq, sigma, src, dst, nrm, k, kg, iters, lreg):
    if kind == "solve":
        return R.solve(pos, dq, sigma, src, dst, k, iters, LAM, kg, lreg) + (None, None)
    if kind == "robust":
        return RR.solve_robust(pos, dq, sigma, src, dst, k, iters, LAM, kg, lreg, 2, TUKEY_C, HUBER_DELTA)
    if kind == "plane":
        return P.solve_plane(pos, dq, sigma, src, dst, nrm, k, iters, LAM, kg, lreg, 2, TUKEY_C, HUBER_DELTA)
    return G.solve_rigid(pos, dq, sigma, src, dst, nrm, k, iters, LAM, LROT, kg, lreg, 2, TUKEY_C, HUBER_DELTA)


def same(got, want, what):
    if got[2] is None:                                       # the plain solve has no weights
        assert np.array_equal(bits(got[1]), bits(want[1])), what + ": energies %s against %s" % (got[1], want[1])
        assert np.array_equal(bits(got[0]), bits(want[0])), what + ": transforms"
    else:
        assert_same(got, want, what)


@pytest.mark.parametrize("kind", SOLVES)
@pytest.mark.parametrize("name", list(CASES))
def test_solves_match_the_restatement_bit_for_bit(name, kind):
    pos, k, kg, setting, sigma, dq, src, dst, nrm, graph, _ = case(name)
    iters, lreg = (50, 100.0) if name == "chain" and kind == "solve" else (ITERS, LREG)
    wf = hier_field(pos, sigma, dq, k, setting)
    got = run_gpu(wf, kind, src, dst, nrm, k, kg, iters, lreg)
    flat = R.Graph
    R.Graph = lambda *a: graph                               # the case's reference graph, made once (H.hierarchy makes it per solve)
    try:
        want = restated(kind, pos, dq, sigma, src, dst, nrm, k, kg, iters, lreg)
    finally:
        R.Graph = flat
    print("%s %s: energies gpu %s restatement %s" % (name, kind, got[1], want[1]))
    assert np.isfinite(want[1]).all() and (want[1][2] > 0 or name == "chain")      # (the chain starts rigid: no E_reg before)
    same(got, want, name + " " + kind)
    if name == "chain" and kind == "solve":                  # what the hierarchy is for, on the GPU's own bits
        x = R.node_translation(got[0])[:, 1]                # (identity transforms before: the translation is delta)
        assert (x[30:] > 0.8 * x[10]).all() and x[10] > 0.005


def test_graph_follows_extend_with_the_setting_kept():
    """A regularised solve builds the hierarchy; extend adds nodes and drops it, the setting stays: the next graph is that of a fresh
    handle given the grown set and the same setting, and the restatement's."""
    k, kg, setting = 8, 4, (3, 0.25, 2.0)
    rng = np.random.default_rng(31)
    pos = rng.uniform(-0.5, 0.5, (120, 3)).astype(F32)
    sigma, dq, src, dst = problem(pos, NPTS)
    sigma = np.full(120, 0.15, F32)
    wf = hier_field(pos, sigma, dq, k, setting)
    wf.solve(dev(src), dev(dst), iters=5, lam=1e-3, reg_neighbours=kg, reg_lambda=1.0)           # the graph of 120 nodes is cached now
    n_added, _ = wf.extend(dev(rng.uniform(-1, 1, (4000, 3)).astype(F32)), 0.3, sigma=0.15)
    assert n_added > 10
    torch.cuda.synchronize()
    gpos, gdq, gsig = (t.cpu().numpy() for t in wf._keep)
    gpos, gdq, gsig = gpos.reshape(-1, 3), gdq.reshape(-1, 8), gsig.reshape(-1)
    fresh = hier_field(gpos, gsig, gdq, k, setting)
    a, b = wf.node_graph(kg) + wf.graph_levels(kg), fresh.node_graph(kg) + fresh.graph_levels(kg)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert np.array_equal(x.cpu().numpy().view(np.uint32), y.cpu().numpy().view(np.uint32))
    want = H.HierGraph(gpos, gsig, kg, *setting)
    _, r_top, r_sizes, r_eff = H.levels(gpos, kg, *setting)
    assert r_eff >= 2 and r_sizes[0] == 120 + n_added
    assert np.array_equal(a[0].cpu().numpy(), want.nbr) and np.array_equal(bits(a[1].cpu().numpy()), bits(want.alpha))
    assert np.array_equal(a[2].cpu().numpy(), r_top) and np.array_equal(a[3].cpu().numpy(), r_sizes) and int(a[4].item()) == r_eff
    a_dq, a_en = wf.solve(dev(src), dev(dst), iters=10, lam=1e-3, reg_neighbours=kg, reg_lambda=1.0)
    torch.cuda.synchronize()
    with H.hierarchy(*setting):
        r_dq, r_en = R.solve(gpos, gdq, gsig, src, dst, k, 10, 1e-3, kg, 1.0)
    assert np.array_equal(bits(a_dq.cpu().numpy()), bits(r_dq)) and np.array_equal(bits(a_en.cpu().numpy()), bits(r_en))


@pytest.mark.parametrize("kind", SOLVES)
def test_levels_zero_is_the_flat_graph_and_its_solves(kind):
    """Switched on, used, and switched off again: the flat graph and the flat solves, against solver_reg_ref and its kin as they stand."""
    pos = random_nodes(257)
    sigma, dq, src, dst = problem(pos, NPTS)
    nrm = seeded_normals(NPTS)
    wf = hier_field(pos, sigma, dq, 8, (3, 0.3, 2.0))
    h_nbr, _ = wf.node_graph(4)
    wf.set_graph_hierarchy(0, 0.3)
    nbr, alpha = wf.node_graph(4)
    top, sizes, eff = wf.graph_levels(4)
    torch.cuda.synchronize()
    r_nbr, r_alpha = R.node_graph(pos, sigma, 4)
    assert np.array_equal(nbr.cpu().numpy(), r_nbr) and np.array_equal(bits(alpha.cpu().numpy()), bits(r_alpha))
    assert not np.array_equal(h_nbr.cpu().numpy(), r_nbr)
    assert not top.cpu().numpy().any() and sizes.cpu().numpy().tolist() == [257] + [0] * 8 and int(eff.item()) == 0
    got = run_gpu(wf, kind, src, dst, nrm, 8, 4, ITERS, LREG)
    same(got, restated(kind, pos, dq, sigma, src, dst, nrm, 8, 4, ITERS, LREG), "levels = 0, " + kind)
    # a handle that never heard of the hierarchy reports the same levels
    top, sizes, eff = field(pos, sigma, dq).graph_levels(4)
    torch.cuda.synchronize()
    assert not top.cpu().numpy().any() and sizes.cpu().numpy().tolist() == [257] + [0] * 8 and int(eff.item()) == 0


def test_invalid_arguments():
    L = capi.lib()
    pos = random_nodes(300)
    sigma = np.full(300, 0.4, F32)
    wf = hier_field(pos, sigma, None, 8, (2, 0.3, 2.0))
    want, _ = wf.node_graph(4)
    nan, inf = float("nan"), float("inf")
    for levels, radius, beta in ((-1, 0.3, 2.0), (9, 0.3, 2.0), (2, 0.0, 2.0), (2, -1.0, 2.0), (2, nan, 2.0), (2, inf, 2.0), (2, 0.3, 0.5),
                                 (2, 0.3, nan), (2, 0.3, inf)):
        assert L.dfusion_warp_set_graph_hierarchy(wf.handle, levels, radius, beta) == DF_E_INVALID
    assert L.dfusion_warp_set_graph_hierarchy(None, 2, 0.3, 2.0) == DF_E_INVALID
    got, _ = wf.node_graph(4)                                # the handle is as it was: the same hierarchy
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())
    assert np.array_equal(got.cpu().numpy(), H.hier_graph(pos, sigma, 4, 2, 0.3, 2.0)[0])
    assert L.dfusion_warp_set_graph_hierarchy(wf.handle, 8, 0.3, 1.0) == 0           # the ends of the ranges
    top = torch.empty(300, dtype=torch.int32, device="cuda")
    for kg in (0, 8):
        assert L.dfusion_warp_graph_levels(wf.handle, kg, top.data_ptr(), None, None, None) == DF_E_INVALID
    assert L.dfusion_warp_graph_levels(None, 4, top.data_ptr(), None, None, None) == DF_E_INVALID
    small = field(random_nodes(5), np.full(5, 0.4, F32), k=4)
    assert L.dfusion_warp_graph_levels(small.handle, 5, None, None, None, None) == DF_E_INVALID      # M < kg + 1
    assert L.dfusion_warp_graph_levels(wf.handle, 4, None, None, None, None) == 0                     # every pointer may be null
    torch.cuda.synchronize()
    _, _, r_sizes, r_eff = H.levels(pos, 4, 8, 0.3, 1.0)      # beta = 1: eight equal levels
    _, sizes, eff = wf.graph_levels(4)
    torch.cuda.synchronize()
    assert np.array_equal(sizes.cpu().numpy(), r_sizes) and int(eff.item()) == r_eff == 8 and len(set(r_sizes[1:].tolist())) == 1
