"""GPU parity of the regularised warp solve (dfusion_warp_solve, dfusion_warp_node_graph) against the numpy restatement
tests/solver_reg_ref.py, which tests/test_solver_reg_rule.py ties to the committed oracle: the node graph (ids and alpha bits), all 8 M
floats of the transforms and all four energies bit for bit at every node-count dispatch boundary and with a hub node; the off switch;
the graph's lifetime across extend and set_nodes; reproducibility; argument checks; the C++ mirror."""
import subprocess

import numpy as np
import pytest
import torch

import solver_reg_ref as R
from dynamicfusion_amd import build, capi
from solver_cases import DF_E_INVALID, bits, dev, field, lcg_problem, problem, random_nodes

pytestmark = pytest.mark.gpu
F32 = np.float32


# ------------------------------------------------------------------------------------------------ node sets
def lattice():
    ax = np.arange(4, dtype=F32) * F32(0.25)
    return np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3).astype(F32)


def star():
    """300 nodes on the unit sphere and one at the centre."""
    rng = np.random.default_rng(23)
    p = rng.normal(0, 1, (300, 3))
    p = (p / np.linalg.norm(p, axis=1, keepdims=True)).astype(F32)
    return np.concatenate([p, np.zeros((1, 3), F32)]).astype(F32)


def pile():
    """A hub that does exist: 200 nodes at ONE position among 101 others.  With kg = 1 a pile node's two nearest are two pile nodes at
    distance 0 in nanoflann's tie order, the same two for every query there; a node that is neither of them is ranked out and takes the
    first (drop-last rule), so the first-ranked pile node collects an incoming list of about 200 edges.  (The star cannot do that: a node
    whose nearest other node is the centre keeps every other such node more than 60 degrees away as seen from the centre -- at most 12
    in three dimensions, the kissing number -- so its centre has in-degree <= 12 whatever the radius.)"""
    pos = np.random.default_rng(29).uniform(-1, 1, (301, 3)).astype(F32)
    pos[50:250] = pos[50]
    return pos


GRAPH_SETS = {
    "M8-kg7": lambda: (np.random.default_rng(1).uniform(-1, 1, (8, 3)).astype(F32), 7),
    "M100-kg4": lambda: (np.random.default_rng(2).uniform(-1, 1, (100, 3)).astype(F32), 4),
    "lattice": lambda: (lattice(), 4),
    "duplicate": lambda: (np.random.default_rng(3).uniform(-1, 1, (30, 3)).astype(F32)[np.r_[0:30, 4]], 3),
    "star": lambda: (star(), 1),
    "pile": lambda: (pile(), 1),
}


@pytest.mark.parametrize("name", list(GRAPH_SETS))
def test_graph_equals_the_restatement(name):
    pos, kg = GRAPH_SETS[name]()
    M = len(pos)
    sigma = np.random.default_rng(7).uniform(0.2, 0.6, M).astype(F32)
    wf = field(pos, sigma)
    nbr, alpha = wf.node_graph(kg)
    torch.cuda.synchronize()
    r_nbr, r_alpha = R.node_graph(pos, sigma, kg)
    assert np.array_equal(nbr.cpu().numpy(), r_nbr)
    assert np.array_equal(bits(alpha.cpu().numpy()), bits(r_alpha))
    if name == "duplicate":
        assert (pos[30] == pos[4]).all() and 30 in r_nbr[4] and 4 in r_nbr[30]
    deg = np.bincount(r_nbr.reshape(-1), minlength=M)
    print("%s: largest in-degree %d" % (name, deg.max()))
    if name == "pile":
        assert deg.max() >= 150                          # a long incoming list


# ------------------------------------------------------------------------------------------------ the solve
SOLVE_CASES = [
    ("baseline", lambda: random_nodes(100), 5003, 8, 4, 40, 0.0, 0.5),
    ("damped-kg7", lambda: random_nodes(257), 5003, 4, 7, 25, 1e-3, 2.0),
    ("M2048", lambda: random_nodes(2048), 3001, 8, 4, 12, 1e-3, 1.0),
    ("M2049", lambda: random_nodes(2049), 3001, 8, 4, 12, 1e-3, 1.0),
    ("M8193", lambda: random_nodes(8193), 3001, 8, 4, 12, 1e-3, 1.0),
    ("star", star, 2000, 8, 1, 12, 1e-3, 1.0),
    ("pile", pile, 2000, 8, 1, 12, 1e-3, 1.0),
]


@pytest.mark.parametrize("name,nodes,N,k,kg,iters,lam,lreg", SOLVE_CASES, ids=[c[0] for c in SOLVE_CASES])
def test_solve_matches_the_restatement_bit_for_bit(name, nodes, N, k, kg, iters, lam, lreg):
    pos = nodes()
    M = len(pos)
    sigma, dq, src, dst = problem(pos, N)
    wf = field(pos, sigma, dq, k)
    g_dq, g_en = wf.solve(dev(src), dev(dst), iters=iters, lam=lam, reg_neighbours=kg, reg_lambda=lreg)
    torch.cuda.synchronize()
    d = {}
    r_dq, r_en = R.solve(pos, dq, sigma, src, dst, k, iters, lam, kg, lreg, details=d)
    g_dq, g_en = g_dq.cpu().numpy(), g_en.cpu().numpy()
    print("%s: M %d, energies gpu %s restatement %s, nodes without data %d, largest in-degree %d" % (
        name, M, g_en, r_en, int((np.bincount(d["keys"][d["keys"] < M], minlength=M) == 0).sum()), int(d["graph"].in_deg.max())))
    assert r_en[2] > 0 and np.isfinite(r_en).all() and r_en[1] < r_en[0]
    assert np.array_equal(bits(g_en), bits(r_en))
    assert np.array_equal(bits(g_dq), bits(r_dq))
    if M == 8193:
        assert (np.bincount(d["keys"][d["keys"] < M], minlength=M) == 0).sum() > 100         # nodes that only the graph moves
    if name == "pile":
        assert d["graph"].in_deg.max() >= 150            # the hub: one thread walks a long incoming list
    # the handle carries the new transforms
    assert np.array_equal(bits(wf._dq.cpu().numpy()), bits(r_dq))


def test_off_switch_returns_energy_data_bits():
    pos = random_nodes(100)
    sigma, dq, src, dst = problem(pos, 5003)
    want_dq, want_en = field(pos, sigma, dq).energy_data(dev(src), dev(dst), iters=20, lam=1e-3)
    for kg, lreg in ((0, 1.0), (4, 0.0)):
        got_dq, got_en = field(pos, sigma, dq).solve(dev(src), dev(dst), iters=20, lam=1e-3, reg_neighbours=kg, reg_lambda=lreg)
        torch.cuda.synchronize()
        assert np.array_equal(bits(got_dq.cpu().numpy()), bits(want_dq.cpu().numpy()))
        assert np.array_equal(bits(got_en.cpu().numpy()[:2]), bits(want_en.cpu().numpy()))
        assert np.array_equal(bits(got_en.cpu().numpy()[2:]), np.zeros(2, np.uint32))
    # the C entry point itself writes the two zeros (WarpField.solve hands it a zeroed tensor)
    wf = field(pos, sigma, dq)
    out = torch.empty((100, 8), dtype=torch.float32, device="cuda"); en = torch.full((4,), 7.0, dtype=torch.float32, device="cuda")
    s, d = dev(src), dev(dst)
    assert capi.lib().dfusion_warp_solve(wf.handle, 8, s.data_ptr(), d.data_ptr(), 5003, 20, 1e-3, 4, 0.0, out.data_ptr(), en.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(en.cpu().numpy()), np.concatenate([bits(want_en.cpu().numpy()), np.zeros(2, np.uint32)]))


def test_graph_follows_extend_and_set_nodes():
    """A regularised solve builds the graph; extend adds nodes, set_nodes replaces them: the next solve must use the new set's graph --
    equal to a fresh handle's and to the restatement, bit for bit."""
    k, kg = 8, 4
    rng = np.random.default_rng(31)
    pos = rng.uniform(-0.5, 0.5, (120, 3)).astype(F32)
    sigma, dq, src, dst = problem(pos, 3001)
    sigma = np.full(120, 0.15, F32)
    wf = field(pos, sigma, dq)
    wf.solve(dev(src), dev(dst), iters=5, lam=1e-3, reg_neighbours=kg, reg_lambda=1.0)           # the graph of 120 nodes is cached now
    cloud = rng.uniform(-1, 1, (4000, 3)).astype(F32)
    n_added, _ = wf.extend(dev(cloud), 0.3, sigma=0.15)
    assert n_added > 10
    torch.cuda.synchronize()
    gpos, gdq, gsig = (t.cpu().numpy() for t in wf._keep)
    gpos, gdq, gsig = gpos.reshape(-1, 3), gdq.reshape(-1, 8), gsig.reshape(-1)
    a_dq, a_en = wf.solve(dev(src), dev(dst), iters=10, lam=1e-3, reg_neighbours=kg, reg_lambda=1.0)
    b_dq, b_en = field(gpos, gsig, gdq).solve(dev(src), dev(dst), iters=10, lam=1e-3, reg_neighbours=kg, reg_lambda=1.0)
    torch.cuda.synchronize()
    r_dq, r_en = R.solve(gpos, gdq, gsig, src, dst, k, 10, 1e-3, kg, 1.0)
    for got_dq, got_en in ((a_dq, a_en), (b_dq, b_en)):
        assert np.array_equal(bits(got_dq.cpu().numpy()), bits(r_dq)) and np.array_equal(bits(got_en.cpu().numpy()), bits(r_en))
    # set_nodes: another node set of the SAME size on the grown handle
    pos2 = rng.uniform(-1, 1, gpos.shape).astype(F32)
    wf.init(pos2, sigma=gsig, transforms=gdq)
    c_dq, c_en = wf.solve(dev(src), dev(dst), iters=10, lam=1e-3, reg_neighbours=kg, reg_lambda=1.0)
    d_dq, d_en = field(pos2, gsig, gdq).solve(dev(src), dev(dst), iters=10, lam=1e-3, reg_neighbours=kg, reg_lambda=1.0)
    torch.cuda.synchronize()
    r_dq, r_en = R.solve(pos2, gdq, gsig, src, dst, k, 10, 1e-3, kg, 1.0)
    for got_dq, got_en in ((c_dq, c_en), (d_dq, d_en)):
        assert np.array_equal(bits(got_dq.cpu().numpy()), bits(r_dq)) and np.array_equal(bits(got_en.cpu().numpy()), bits(r_en))
    # set_transforms leaves the graph alone: the same solve from the same transforms again gives the same bits
    wf.set_transforms(dev(gdq))
    e_dq, e_en = wf.solve(dev(src), dev(dst), iters=10, lam=1e-3, reg_neighbours=kg, reg_lambda=1.0)
    torch.cuda.synchronize()
    assert np.array_equal(bits(e_dq.cpu().numpy()), bits(r_dq)) and np.array_equal(bits(e_en.cpu().numpy()), bits(r_en))


def test_two_runs_give_identical_bits():
    pos = random_nodes(2000, seed=41)
    sigma, dq, src, dst = problem(pos, 40001)
    outs = []
    for _ in range(2):
        g_dq, g_en = field(pos, sigma, dq).solve(dev(src), dev(dst), iters=30, lam=1e-3, reg_neighbours=4, reg_lambda=1.0)
        torch.cuda.synchronize()
        outs.append((g_dq.cpu().numpy(), g_en.cpu().numpy()))
    assert np.array_equal(bits(outs[0][0]), bits(outs[1][0])) and np.array_equal(bits(outs[0][1]), bits(outs[1][1]))
    assert outs[0][1][1] < outs[0][1][0]


def test_invalid_arguments():
    L = capi.lib()
    pos = random_nodes(5)
    wf = field(pos, np.full(5, 0.4, F32), k=4)
    pts = dev(np.random.default_rng(1).uniform(-1, 1, (64, 3)).astype(F32))
    dq = torch.empty((5, 8), dtype=torch.float32, device="cuda"); en = torch.zeros(4, dtype=torch.float32, device="cuda")

    def call(kg, lreg):
        return L.dfusion_warp_solve(wf.handle, 4, pts.data_ptr(), pts.data_ptr(), 64, 3, 0.0, kg, lreg, dq.data_ptr(), en.data_ptr(), None)
    assert call(-1, 1.0) == DF_E_INVALID
    assert call(8, 1.0) == DF_E_INVALID
    assert call(5, 1.0) == DF_E_INVALID and call(7, 0.0) == DF_E_INVALID         # M = 5 < kg + 1
    assert call(2, -1.0) == DF_E_INVALID
    assert call(2, float("nan")) == DF_E_INVALID
    assert call(0, float("nan")) == DF_E_INVALID
    assert call(4, 1.0) == 0 and call(0, 0.0) == 0                                # M = kg + 1 is enough
    nbr = torch.empty((5, 7), dtype=torch.int32, device="cuda")
    for kg in (0, 5, 8):
        assert L.dfusion_warp_node_graph(wf.handle, kg, nbr.data_ptr(), None, None) == DF_E_INVALID
    assert L.dfusion_warp_node_graph(wf.handle, 4, None, None, None) == DF_E_INVALID
    assert L.dfusion_warp_node_graph(wf.handle, 4, nbr.data_ptr(), None, None) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the C++ mirror
@pytest.mark.parametrize("kg,lreg", [(4, 1.0), (0, 0.0)], ids=["regularised", "off"])
def test_cxx_mirror_prints_the_python_mirrors_bits(kg, lreg):
    build.build_host()
    r = subprocess.run([build.HOST_WARP_SOLVE, "reg", str(kg), str(lreg)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.array([[int(w, 16) for w in line.split()] for line in r.stdout.strip().splitlines()], np.uint32)
    pos, dq, sigma, src, dst = lcg_problem()
    wf = field(pos, sigma, dq)
    if kg:
        want, _ = wf.solve(dev(src), dev(dst), iters=20, lam=1e-3, reg_neighbours=kg, reg_lambda=lreg)
    else:
        want, _ = wf.energy_data(dev(src), dev(dst), iters=20, lam=1e-3)
    torch.cuda.synchronize()
    assert got.shape == (50, 8)
    assert np.array_equal(got, bits(want.cpu().numpy()))
    if kg:                                               # and the term did something: the data-only answer differs
        plain, _ = field(pos, sigma, dq).energy_data(dev(src), dev(dst), iters=20, lam=1e-3)
        assert not np.array_equal(got, bits(plain.cpu().numpy()))
