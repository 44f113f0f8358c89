"""The rule of the hierarchical node graph, on the CPU: tests/solver_hier_ref.py -- the numpy restatement the GPU is
compared with bit for bit in tests/test_gpu_solver_hier.py -- checked property by property (nesting, lowest index wins, the effective
depth, the (d2, index) order, duplicates, NaN), against an independent dense float64 solve of the normal equations over its edges, and
shown to do what the hierarchy is for: carry a correction along a long unobserved chain in few conjugate-gradient steps."""
import numpy as np
import pytest

import solver_hier_ref as H
import solver_reg_ref as R
from solver_cases import bits, random_problem

F32 = np.float32


def lattice():
    ax = np.arange(4, dtype=F32) * F32(0.25)
    return np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3).astype(F32)


# ------------------------------------------------------------------------------------------------ the levels
def test_levels_are_nested_and_the_lowest_index_of_a_cell_wins():
    pos = np.random.default_rng(1).uniform(-1, 1, (500, 3)).astype(F32)
    members, top, sizes, eff = H.levels(pos, 4, 3, 0.2, 2.0)
    assert eff == 3 and sizes[0] == 500 and (sizes[4:] == 0).all()
    assert sizes[0] > sizes[1] > sizes[2] > sizes[3] >= 5
    for l, c in zip((1, 2, 3), (F32(0.2), F32(0.4), F32(0.8))):
        assert (np.diff(members[l]) > 0).all() and np.isin(members[l], members[l - 1]).all()
        cell = np.floor(pos / c).astype(np.int64)
        below = members[l - 1]
        for i in members[l]:                                 # no node of the level below with a lower index shares the cell
            same = below[(cell[below] == cell[i]).all(1)]
            assert same.min() == i
        assert len({tuple(cell[i]) for i in members[l]}) == len({tuple(cell[i]) for i in below}) == sizes[l]
    for i in range(500):
        assert top[i] == max(l for l in range(4) if i in members[l])


@pytest.mark.parametrize("n_cells,want", [(4, 0), (5, 1)], ids=["kg", "kg+1"])
def test_effective_depth_needs_kg_plus_one_members(n_cells, want):
    """kg = 4: a level of 4 members cannot give a node 4 other targets, a level of 5 can."""
    pos = np.zeros((40, 3), F32)
    pos[:, 0] = (np.arange(40) % n_cells) + F32(0.25) + F32(0.01) * (np.arange(40) // n_cells)      # n_cells unit cells along x
    members, top, sizes, eff = H.levels(pos, 4, 2, 1.0, 100.0)
    assert sizes[1] == n_cells and sizes[2] == 1             # (level 2: everything in the cell [0, 100))
    assert eff == want
    assert (top == 0).all() if want == 0 else (np.flatnonzero(top == 1).tolist() == list(range(n_cells)))


def test_depth_zero_is_the_flat_graph_bit_for_bit():
    pos = np.random.default_rng(2).uniform(0.1, 0.8, (6, 3)).astype(F32)
    pos[::2, 0] += F32(0.9)                                  # two cells of edge 0.9: no level has 5 members
    sigma = np.linspace(0.1, 0.6, 6).astype(F32)
    _, _, sizes, eff = H.levels(pos, 4, 3, 0.9, 4.0)
    assert eff == 0 and sizes[1] == 2 and sizes[2] == 1
    nbr, alpha = H.hier_graph(pos, sigma, 4, 3, 0.9, 4.0)
    f_nbr, f_alpha = R.node_graph(pos, sigma, 4)
    assert np.array_equal(nbr, f_nbr) and np.array_equal(bits(alpha), bits(f_alpha))
    # all nodes in one cell: the same
    pos = np.random.default_rng(3).uniform(0.1, 0.9, (50, 3)).astype(F32)
    nbr, _ = H.hier_graph(pos, np.full(50, 0.3, F32), 4, 4, 1.0, 4.0)
    assert np.array_equal(nbr, R.node_graph(pos, np.full(50, 0.3, F32), 4)[0])


def test_overflowing_cell_edge_empties_the_levels_above():
    pos = np.random.default_rng(4).uniform(-1, 1, (100, 3)).astype(F32)
    _, _, sizes, eff = H.levels(pos, 2, 4, 0.1, 3e38)
    assert sizes[1] > 50 and sizes[2] == 8 and (sizes[3:] == 0).all() and eff == 2     # c_2 = 3e37: a cell per sign octant; c_3 = inf


# ------------------------------------------------------------------------------------------------ the edges
def test_lattice_with_exact_ties_follows_d2_then_index():
    pos = lattice()
    kg = 4
    members, top, sizes, eff = H.levels(pos, kg, 2, 0.5, 2.0)
    assert sizes[1] == 8 and sizes[2] == 1 and eff == 1
    nbr, _ = H.hier_graph(pos, np.full(64, 0.3, F32), kg, 2, 0.5, 2.0)
    S1 = members[1]
    ties = 0
    for i in range(64):
        cand = [j for j in S1 if j != i]
        d2 = [float(((pos[i] - pos[j]).astype(F32) ** 2).sum()) for j in cand]      # (exact on this lattice: multiples of 1/16)
        want = [j for _, j in sorted(zip(d2, cand))][:kg]
        assert nbr[i].tolist() == want
        ties += sorted(d2)[kg - 1] == sorted(d2)[kg]
    assert ties > 10                                         # the order of equals decided entries


def test_duplicated_position():
    pos = np.random.default_rng(3).uniform(-1, 1, (30, 3)).astype(F32)[np.r_[0:30, 4]]
    members, top, _, eff = H.levels(pos, 3, 2, 0.5, 2.0)
    assert eff >= 1 and top[30] == 0 and top[4] >= 1         # the copy shares the cell at every level and has the higher index
    nbr, _ = H.hier_graph(pos, np.full(31, 0.3, F32), 3, 2, 0.5, 2.0)
    assert nbr[30, 0] == 4                                   # distance 0 to its original, a member of S_1
    assert all(i not in nbr[i] and len(set(nbr[i].tolist())) == 3 for i in range(31))


def test_nan_position_is_no_member_and_gets_targets_in_range():
    pos = np.random.default_rng(6).uniform(-1, 1, (40, 3)).astype(F32)
    pos[0, 1] = np.nan
    pos[7] = np.inf
    members, top, _, eff = H.levels(pos, 4, 2, 0.5, 2.0)
    assert eff >= 1 and 0 not in members[1] and 7 not in members[1] and top[0] == 0 and top[7] == 0
    nbr, _ = H.hier_graph(pos, np.full(40, 0.3, F32), 4, 2, 0.5, 2.0)
    assert nbr.min() >= 0 and nbr.max() < 40
    assert nbr[0].tolist() == members[1][:4].tolist()        # every d2 NaN: index order
    for i in range(40):
        assert i not in nbr[i] and len(set(nbr[i].tolist())) == 4


def test_hierarchy_context_stands_in_for_the_flat_graph_and_leaves():
    pos = lattice()
    sigma = np.full(64, 0.3, F32)
    with H.hierarchy(2, 0.5, 2.0):
        made = R.Graph(pos, sigma, 4)
    assert isinstance(made, H.HierGraph) and np.array_equal(made.nbr, H.hier_graph(pos, sigma, 4, 2, 0.5, 2.0)[0])
    assert type(R.Graph(pos, sigma, 4)) is R.Graph
    with H.hierarchy(0, 0.5):
        assert type(R.Graph(pos, sigma, 4)) is R.Graph


# ------------------------------------------------------------------------------------------------ against a dense float64 solve
def dense_delta(d, M, lam, lreg):
    """(W^T W + lam I + lreg L) delta = W^T e0 - lreg b as a dense float64 matrix, from the restatement's own f32 w, alpha and g, over
    whatever edges d["graph"] holds; numpy.linalg.solve."""
    w, keys, e0, G, g = d["w"].astype(np.float64), d["keys"], d["e0"].astype(np.float64), d["graph"], d["g"].astype(np.float64)
    N, k = w.shape
    W = np.zeros((N, M))
    for j in range(k):
        ok = keys[:, j] < M
        np.add.at(W, (np.flatnonzero(ok), keys[ok, j]), w[ok, j])
    A = W.T @ W + lam * np.eye(M)
    rhs = W.T @ e0
    L = np.zeros((M, M))
    for e, (i, j, a) in enumerate(zip(G.tail, G.nbr.reshape(-1), G.alpha.reshape(-1).astype(np.float64))):
        L[i, i] += a; L[j, j] += a; L[i, j] -= a; L[j, i] -= a
        rhs[i] -= lreg * a * g[e]; rhs[j] += lreg * a * g[e]
    return np.linalg.solve(A + lreg * L, rhs)


DENSE_MEASURED = 4.0e-6        # largest |delta - dense| measured on the CPU (see the docstring below)


def test_converged_hierarchical_solve_meets_the_dense_normal_equations():
    """test_solver_reg_rule's problem (M = 60, N = 1500, k = 8, kg = 4, lam = 1e-3, lambda_reg = 1, 400 steps) over the hierarchy
    (2 levels, radius 0.5, beta 2).  Measured on the CPU (x86-64, glibc exp): largest |delta - dense| = 3.97e-6 with |delta| up to 6.7e-2 (the flat graph's
    is 4.6e-6, tests/test_solver_reg_rule.py); asserted: 4 x that."""
    M, lam, lreg = 60, 1e-3, 1.0
    pos, dq, sigma, src, dst = random_problem(M, 1500)
    d = {}
    with H.hierarchy(2, 0.5, 2.0):
        R.solve(pos, dq, sigma, src, dst, 8, 400, lam, kg=4, lambda_reg=lreg, details=d)
    assert isinstance(d["graph"], H.HierGraph)
    assert not np.array_equal(d["graph"].nbr, R.node_graph(pos, sigma, 4)[0])
    want = dense_delta(d, M, float(F32(lam)), float(F32(lreg)))
    err = float(np.abs(d["x"].astype(np.float64) - want).max())
    print("dense solve: max |delta - dense| = %.3g, max |delta| = %.3g" % (err, np.abs(want).max()))
    assert np.abs(want).max() > 1e-2
    assert err <= 4 * DENSE_MEASURED


# ------------------------------------------------------------------------------------------------ behaviour
def test_a_correction_crosses_the_chain_in_fifty_steps_only_over_the_hierarchy():
    """120 nodes 25 mm apart (dg_w 0.025), 1500 points over the first 0.5 m moved 20 mm along the chain; k = 4, kg = 4, lambda_reg = 100,
    50 steps; the k-NN is the oracle's.  delta_x at node 10 / 60 / 119:
        flat graph                                 0.0088 / 0.0000 / 0.0000
        hierarchy (4 levels, radius 0.05, beta 4)  0.0089 / 0.0090 / 0.0090
    (a brute-force k-NN on another draw of the points gave 0.0085 / 0 / 0 and 0.0087 / 0.0088 / 0.0088: neither moves the picture)."""
    pos, dq, sigma, src, dst = H.chain()
    d0, d1 = {}, {}
    R.solve(pos, dq, sigma, src, dst, 4, 50, 0.0, kg=4, lambda_reg=100.0, details=d0)
    with H.hierarchy(4, 0.05, 4.0):
        R.solve(pos, dq, sigma, src, dst, 4, 50, 0.0, kg=4, lambda_reg=100.0, details=d1)
    flat, hier = d0["x"][:, 0], d1["x"][:, 0]
    print("delta_x at 10 / 60 / 119: flat %.4f / %.4f / %.4f, hierarchy %.4f / %.4f / %.4f" % (
        flat[10], flat[60], flat[119], hier[10], hier[60], hier[119]))
    assert flat[10] > 0.005 and hier[10] > 0.005
    assert abs(flat[119]) < 0.1 * flat[10]
    assert (hier[30:] > 0.8 * hier[10]).all()
