"""The rule of the warp solve with node rotations as unknowns, on the CPU: tests/solver_rigid_ref.py -- the numpy
restatement the GPU is compared with bit for bit in tests/test_gpu_solver_rigid.py -- recovers a planted rigid turn that the
translation-only solve cannot, meets a dense float64 solve of its own normal equations, leaves a field that already explains the live
points bit for bit alone, and treats invalid inputs and unconstrained nodes as the rule says."""
import numpy as np

import oracle_lib as O
import solver_plane_ref as P
import solver_reg_ref as R
import solver_rigid_ref as G
from dynamicfusion_amd import synth
from solver_cases import bits, planted_slip, random_problem

F32 = np.float32


# ------------------------------------------------------------------------------------------------ (1) the planted rigid turn
TURN_DEG = 5.0
TURN_AXIS = np.array([0.0, 1.0, 0.0])
# Two points off the cap for the axis to pass through.  The blend the pipeline applies turns a point by the blended rotation and adds
# the node translations under UNNORMALISED weights: y = R_v p + sum_i w_vi t_i, and the weight sums S_v differ from point to point (3 to
# 6 here).  A turn about the sphere's centre, the frame's origin, needs a rotation and no translation, so the field can hold it exactly
# and what is left after the solve is the solver's error: that is the planted turn the conditions below are set on.  A turn about any
# other point also needs the ONE translation (I - R) a0 at every point, which no node translations can deliver through differing S_v; what
# is left there is the blend's error, measured and pinned in the second test.
CENTRE, OFF_CENTRE = np.array([0.0, 0.0, 0.0]), np.array([0.3, -0.2, 0.1])
TURN = dict(iters=400, lam=1e-3, lam_rot=1e-3, kg=4, lreg=1.0, rounds=3)           # DESIGN.md 16's damping, the GPU tests' lambda_reg


def planted_turn(point=OFF_CENTRE):
    """DESIGN.md 16's cap (60 nodes, 1500 points on the 60 degree cap of the unit sphere, sigma in [0.3, 0.6], k = 8, identity
    transforms, normals = the points); the live points and the expected normals are the canonical ones turned 5 degrees about the y
    direction through `point`."""
    pos, dq, sigma, src, _, normals, _, _ = planted_slip()
    ang = np.deg2rad(TURN_DEG)
    K = np.array([[0, -TURN_AXIS[2], TURN_AXIS[1]], [TURN_AXIS[2], 0, -TURN_AXIS[0]], [-TURN_AXIS[1], TURN_AXIS[0], 0]])
    rot = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    live = ((src.astype(np.float64) - point) @ rot.T + point).astype(F32)
    return pos, dq, sigma, src, live, normals, normals.astype(np.float64) @ rot.T


def turn_errors(pos, dq, sigma, src, live, normals, true_normals, k=8):
    """(largest |y - live|, largest angle in degrees between the warped and the true normal), float64, with the oracle's warp.  The
    warped normal is the normal turned by the blend's rotation: the point path adds the blend's translation to a normal as it does to a
    point (as the reference does), which says nothing about its direction."""
    y, _ = O.warp_points(pos, dq, sigma, src, None, k)
    blend = O.dqb(pos, dq, sigma, src, k)
    turned = R.dq_transform(np.concatenate([blend[:, :4], np.zeros((len(src), 4), F32)], 1), normals).astype(np.float64)
    cos = (turned * true_normals).sum(1) / (np.linalg.norm(turned, axis=1) * np.linalg.norm(true_normals, axis=1))
    return float(np.linalg.norm(y.astype(np.float64) - live, axis=1).max()), float(np.degrees(np.arccos(np.clip(cos, -1, 1))).max())


def run_turn(point):
    """solve_rigid (point-to-point: on a sphere the residual along the normal does not see a turn, or the part of one, that slides the
    cap in itself) over 3 rounds and the translation-only solver_plane_ref on the same pairs: ((rigid errors), (translation-only errors),
    rigid energies, details)."""
    pos, dq, sigma, src, live, normals, true_normals = planted_turn(point)
    d = {}
    r_dq, r_en, _, _ = G.solve_rigid(pos, dq, sigma, src, live, None, 8, TURN["iters"], TURN["lam"], TURN["lam_rot"], TURN["kg"], TURN["lreg"],
                                     TURN["rounds"], details=d)
    t_dq, t_en, _, _ = P.solve_plane(pos, dq, sigma, src, live, normals, 8, TURN["iters"], TURN["lam"], TURN["kg"], TURN["lreg"], TURN["rounds"])
    args = (sigma, src, live, normals, true_normals)
    rigid, trans = turn_errors(pos, r_dq, *args), turn_errors(pos, t_dq, *args)
    print("planted turn about %s: rigid |y - live| %.3g m, normal %.3g deg, energies %s, steps %s; translations only %.3g m, %.3g deg, "
          "energies %s" % ((point.tolist(),) + rigid + (r_en, d["steps"]) + trans + (t_en,)))
    assert d["valid"].all() and len(d["valid"]) == 1500
    assert r_en[1] < r_en[0]
    return rigid, trans, r_en, d


# measured on the CPU (x86-64, glibc exp) with the restatements: (largest |y - live| in metres, largest normal angle in degrees)
TURN_MEASURED_RIGID = (8.84e-7, 3.41e-4)
TURN_MEASURED_TRANSLATIONS = (9.03e-2, 5.00)
OFF_CENTRE_MEASURED_RIGID = (3.34e-3, 0.965)
OFF_CENTRE_MEASURED_TRANSLATIONS = (9.55e-2, 5.00)
OFF_CENTRE_MEASURED_PLANE_FORM = (9.77e-2, 5.04)          # solve_rigid WITH the normals: the residual along the normal


def test_planted_rigid_turn():
    """The turn about the sphere's centre.  Measured: TURN_MEASURED_RIGID (2.4e-2 m and 0.29 degrees, 8.6e-5 and 9.4e-3, 8.8e-7 and 3.4e-4
    after rounds 1, 2, 3: Gauss-Newton's convergence) and TURN_MEASURED_TRANSLATIONS (the translation-only solve cannot turn a normal).
    Asserted: rigid at most 4 x its values, translations-only at least a quarter of its values, and the rigid normal error at most a
    tenth of the translation-only one."""
    rigid, trans, _, _ = run_turn(CENTRE)
    assert rigid[0] <= 4 * TURN_MEASURED_RIGID[0] and rigid[1] <= 4 * TURN_MEASURED_RIGID[1]
    assert trans[0] >= TURN_MEASURED_TRANSLATIONS[0] / 4 and trans[1] >= TURN_MEASURED_TRANSLATIONS[1] / 4
    assert rigid[1] <= trans[1] / 10


def test_planted_turn_about_an_off_centre_axis_leaves_the_blends_error():
    """The same turn about the axis through OFF_CENTRE.  Measured: OFF_CENTRE_MEASURED_RIGID and OFF_CENTRE_MEASURED_TRANSLATIONS; the
    rounds have converged (1.007, 0.9659, 0.9650, 0.9650 degrees after rounds 1 to 4), and float64 Gauss-Newton rounds on the dense
    system of test (2) end at the same 3.34e-3 m and 0.9650 degrees, so this is the minimum of the energy, not the recurrence
    (lambda_reg = 1e4 reaches 0.51 degrees, no graph 0.97): the least-squares fit trades part of the rotation against the translation
    the blend cannot deliver.  The issue's tenth of the translation-only normal error (0.50 degrees) is NOT attainable for a rigid
    motion in general with this blend: 0.965 / 5.00 = 0.19.  Asserted: both solves within the 4 x margin of their values, and the rigid
    solve ahead on both.  The plane form of the rigid solve (with the normals) is pinned too, OFF_CENTRE_MEASURED_PLANE_FORM: on a sphere
    the residual along the normal does not see the part of the turn that slides the cap in itself, so it does no better than the
    translation-only plane solve there."""
    rigid, trans, _, _ = run_turn(OFF_CENTRE)
    pos, dq, sigma, src, live, normals, true_normals = planted_turn(OFF_CENTRE)
    f_dq, f_en, _, _ = G.solve_rigid(pos, dq, sigma, src, live, normals, 8, TURN["iters"], TURN["lam"], TURN["lam_rot"], TURN["kg"], TURN["lreg"],
                                     TURN["rounds"])
    form = turn_errors(pos, f_dq, sigma, src, live, normals, true_normals)
    print("plane form of the rigid solve: |y - live| %.3g m, normal %.3g deg, energies %s" % (form + (f_en,)))
    assert f_en[1] < f_en[0]
    assert form[0] >= OFF_CENTRE_MEASURED_PLANE_FORM[0] / 4 and form[1] >= OFF_CENTRE_MEASURED_PLANE_FORM[1] / 4
    assert form[0] <= 4 * OFF_CENTRE_MEASURED_PLANE_FORM[0] and form[1] <= 4 * OFF_CENTRE_MEASURED_PLANE_FORM[1]
    assert rigid[0] <= 4 * OFF_CENTRE_MEASURED_RIGID[0] and rigid[1] <= 4 * OFF_CENTRE_MEASURED_RIGID[1]
    assert trans[0] >= OFF_CENTRE_MEASURED_TRANSLATIONS[0] / 4 and trans[1] >= OFF_CENTRE_MEASURED_TRANSLATIONS[1] / 4
    assert rigid[0] < trans[0] and rigid[1] < trans[1]


# ------------------------------------------------------------------------------------------------ (2) dense float64
def cross_matrix(v):
    """[v]x with [v]x o = v x o, for rows of v.  -> [.., 3, 3]"""
    z = np.zeros(len(v))
    return np.stack([np.stack([z, -v[:, 2], v[:, 1]], 1), np.stack([v[:, 2], z, -v[:, 0]], 1), np.stack([-v[:, 1], v[:, 0], z], 1)], 1)


def dense_rigid(d, M, lam, lam_rot, lreg, normalised_blend=False):
    """The first round in float64 on the dense 6M x 6M normal matrix, from the restatement's own f32 w, wn, a, q, e, b, g and alpha.
    Unknown 3 i + c is omega_i's component c, 3 M + 3 i + c is tau_i's.  The rows of point v: w_vi I at tau_i, w_vi [q_i]x - wn_vi [a_v]x
    at omega_i; of edge e = (i -> j): I at tau_i, -[b_e]x at omega_i, -I at tau_j.
    normalised_blend: the data rows of the usual linear-blend-skinning Jacobian instead, wn_vi I at tau_i and -wn_vi [y_v - c_i]x at
    omega_i -- right for a blend over normalised weights, which the pipeline's is not."""
    w, wn, keys, G_ = d["w"].astype(np.float64), d["wn"].astype(np.float64), d["keys"], d["graph"]
    a, q, e = d["a"][0].astype(np.float64), d["q"][0].astype(np.float64), d["e"][0].astype(np.float64)
    y, cen = d["y"][0].astype(np.float64), d["c"][0].astype(np.float64)
    N, k = w.shape
    J = np.zeros((N, 3, 6 * M))
    rows = np.arange(N)
    ax, eye = cross_matrix(a), np.eye(3)
    for j in range(k):
        ok = keys[:, j] < M
        n = np.where(ok, keys[:, j], 0)
        om = np.where(ok[:, None, None], w[:, j, None, None] * cross_matrix(q[n]) - wn[:, j, None, None] * ax, 0.0)
        tau = np.where(ok[:, None, None], w[:, j, None, None] * eye, 0.0)
        if normalised_blend:
            om = np.where(ok[:, None, None], -wn[:, j, None, None] * cross_matrix(y - cen[n]), 0.0)
            tau = np.where(ok[:, None, None], wn[:, j, None, None] * eye, 0.0)
        for r in range(3):                                             # (a point's k nodes differ: no index pair repeats)
            for c in range(3):
                J[rows, r, 3 * n + c] += om[:, r, c]
                J[rows, r, 3 * M + 3 * n + c] += tau[:, r, c]
    J = J.reshape(3 * N, 6 * M)
    A = J.T @ J + np.diag(np.r_[np.full(3 * M, lam_rot), np.full(3 * M, lam)])
    rhs = J.T @ e.reshape(-1)
    alpha, head, tail = G_.alpha.reshape(-1).astype(np.float64), G_.nbr.reshape(-1), G_.tail
    b, g = d["b"][0].astype(np.float64), d["g"][0].astype(np.float64)
    bx = cross_matrix(b)
    D = np.zeros((len(head), 3, 6 * M))
    for ed in range(len(head)):
        i, j = tail[ed], head[ed]
        D[ed][:, 3 * M + 3 * i:3 * M + 3 * i + 3] += eye
        D[ed][:, 3 * M + 3 * j:3 * M + 3 * j + 3] -= eye
        D[ed][:, 3 * i:3 * i + 3] -= bx[ed]
    A += lreg * np.einsum("e,erc,erd->cd", alpha, D, D)
    rhs -= lreg * np.einsum("e,erc,er->c", alpha, D, g)
    return np.linalg.solve(A, rhs).reshape(2 * M, 3)


DENSE = dict(lam=1e-2, lam_rot=1e-1, lreg=1.0)       # damped enough that the recurrence reaches |r|^2 <= 1e-10 |r0|^2 within 400 steps
DENSE_MEASURED = 3.73e-4                                 # largest |X - dense|, one round of 400 steps, measured on the CPU


def test_converged_round_meets_the_dense_normal_equations():
    """The off-centre planted turn, point-to-point, kg = 4, one round of 400 steps against the 360 x 360 float64 system.
    Measured on the CPU (x86-64, glibc exp): largest |X - dense| = DENSE_MEASURED; asserted: 4 x that."""
    pos, dq, sigma, src, live, normals, _ = planted_turn()
    d = {}
    G.solve_rigid(pos, dq, sigma, src, live, None, 8, 400, DENSE["lam"], DENSE["lam_rot"], 4, DENSE["lreg"], 1, details=d)
    want = dense_rigid(d, len(pos), float(F32(DENSE["lam"])), float(F32(DENSE["lam_rot"])), DENSE["lreg"])
    err = float(np.abs(d["x"][0].astype(np.float64) - want).max())
    print("dense solve: max |X - dense| = %.3g, max |omega| = %.3g, max |tau| = %.3g, steps %s" % (
        err, np.abs(want[:60]).max(), np.abs(want[60:]).max(), d["steps"]))
    assert d["steps"][0] < 400                           # converged, not cut off
    assert np.abs(want[:60]).max() > 1e-2 and np.abs(want[60:]).max() > 1e-2
    assert err <= 4 * DENSE_MEASURED


def test_the_normalised_linear_blend_jacobian_diverges_on_this_blend():
    """Why the rule does not take the usual Jacobian over normalised weights.  Exact Gauss-Newton rounds on the off-centre planted turn
    (each round's dense float64 system solved with numpy, the update written back by the restatement's write_back, the true residual
    from the oracle's warp): with the rule's Jacobian E_data = sum |live - y|^2 falls round by round; with the normalised one, whose
    translation columns are wrong by the weight sum S_v (3 to 6 here), it rises without bound."""
    pos, dq, sigma, src, live, normals, _ = planted_turn()
    energies = {}
    for normalised in (False, True):
        cur, en = dq.reshape(-1, 8).copy(), []
        for rnd in range(4):
            d = {}
            G.solve_rigid(pos, cur, sigma, src, live, None, 8, 0, TURN["lam"], TURN["lam_rot"], 4, TURN["lreg"], 1, details=d)
            en.append(float((d["e"][0].astype(np.float64) ** 2).sum()))
            if rnd < 3:
                X = dense_rigid(d, len(pos), TURN["lam"], TURN["lam_rot"], TURN["lreg"], normalised_blend=normalised).astype(F32)
                cur = G.write_back(cur, R.node_translation(cur), d["c"][0], X)
        energies[normalised] = en
    print("E_data over exact rounds: the rule's Jacobian %s; the normalised blend's %s" % (energies[False], energies[True]))
    good, bad = energies[False], energies[True]
    assert good[0] == bad[0]
    assert good[1] < good[0] and good[2] < good[1] and good[3] < 1e-3 * good[0]
    assert bad[1] > bad[0] and bad[2] > bad[1] and bad[3] > 100 * bad[0]


# ------------------------------------------------------------------------------------------------ (3) the fixed point
def test_a_field_that_explains_the_live_points_is_left_alone():
    """live = warp(canonical) exactly: e = 0, r0 = 0, the recurrence never starts (SV_ACTIVE = 0 after the init), every node keeps its
    eight floats and both energy pairs are equal -- with seeded transforms and no graph, and with a graph over identity transforms."""
    pos, dq, sigma, src, _ = random_problem(100, 2000, nans=False)
    normals = np.random.default_rng(8).normal(0, 1, src.shape).astype(F32)
    for transforms, kg in ((dq, 0), (synth.identity_dq(len(pos)), 4)):
        live, _ = O.warp_points(pos, transforms, sigma, src, None, 8)
        for nrm in (None, normals):
            d = {}
            out, en, _, _ = G.solve_rigid(pos, transforms, sigma, src, live, nrm, 8, 25, 1e-3, 1e-3, kg, 1.0, 2, details=d)
            assert d["steps"] == [0, 0] and not d["r0"][0].any() and not d["r0"][1].any()
            assert np.array_equal(bits(out), bits(transforms))
            assert bits(en[0]) == bits(en[1]) and bits(en[2]) == bits(en[3]) and en[0] == 0


# ------------------------------------------------------------------------------------------------ (4) invalid inputs
def test_invalid_normals_and_weightless_points_are_skipped():
    pos, dq, sigma, src, dst = random_problem(100, 2000)
    rng = np.random.default_rng(4)
    normals = rng.normal(0, 1, (len(src), 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(F32)
    ok = np.isfinite(src).all(1) & np.isfinite(dst).all(1)
    bad = np.flatnonzero(ok)[[3, 40, 500, 900]]
    marked = normals.copy()
    marked[bad[0], 0] = np.nan; marked[bad[1], 2] = np.inf; marked[bad[2], 1] = -np.inf; marked[bad[3]] = np.nan
    d = {}
    args = (8, 12, 1e-3, 1e-3, 4, 1.0, 2, 0.05, 0.0)
    got = G.solve_rigid(pos, dq, sigma, src, dst, marked, *args, details=d)
    assert (d["keys"][bad] == len(pos)).all() and not d["w"][bad].any() and not d["wn"][bad].any() and not d["e"][0][bad].any()
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    dst2 = dst.copy(); dst2[bad] = np.nan                               # the same solve with those points taken out by the older rule
    want = G.solve_rigid(pos, dq, sigma, src, dst2, normals, *args)
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(bits(g), bits(w))
    # a point so far from its nodes that every weight underflows to 0: S_v = 0, invalid (its wn would be 0 / 0)
    far = np.flatnonzero(ok)[[11, 700]]
    src3, dst3 = src.copy(), dst.copy()
    src3[far] += F32(40); dst3[far] += F32(40)
    d3 = {}
    got3 = G.solve_rigid(pos, dq, sigma, src3, dst3, normals, *args, details=d3)
    assert (d3["keys"][far] == len(pos)).all() and np.isfinite(got3[0]).all() and np.isfinite(d3["wn"]).all()
    dst4 = dst.copy(); dst4[far] = np.nan
    want3 = G.solve_rigid(pos, dq, sigma, src, dst4, normals, *args)
    for g, w in zip(got3[:2], want3[:2]):
        assert np.array_equal(bits(g), bits(w))


# ------------------------------------------------------------------------------------------------ (5) an unconstrained node
def test_a_node_without_entries_and_without_edges_keeps_its_eight_floats():
    pos, dq, sigma, src, dst = random_problem(100, 2000)
    pos = pos.copy(); pos[37] = F32([30, 30, 30])                       # no point has it among its 8 nearest
    d = {}
    out, en, _, _ = G.solve_rigid(pos, dq, sigma, src, dst, None, 8, 12, 1e-3, 1e-3, 0, 0.0, 2, details=d)
    assert not (d["keys"] == 37).any()
    assert np.array_equal(bits(out[37]), bits(dq.reshape(-1, 8)[37]))
    moved = (bits(out) != bits(dq.reshape(-1, 8))).any(1)
    assert moved.sum() == len(pos) - 1                                   # every other node turned and moved
    assert (bits(out[:, :4]) != bits(dq.reshape(-1, 8)[:, :4])).any(1).sum() == len(pos) - 1


# ------------------------------------------------------------------------------------------------ (6) the closed loop's oracle side turns nodes
def test_the_loops_oracle_side_turns_nodes_every_frame():
    """tests/test_gpu_nonrigid_loop_rigid.py compares the GPU loop with an oracle loop whose solve is this restatement, stage by stage.
    On the oracle side alone: the loop's conditions hold, every frame's solve lowers the TRUE data energy (the warp behind the
    write-back) and changes the rotation of at least one node, and the transforms are not the plane loop's."""
    import nonrigid_loop as NL
    import plane_loop as PL
    import rigid_loop as RL
    case = NL.FAST
    rec, be = RL.run_oracle_loop(case)
    assert NL.nonvacuity(rec, case) == []
    for f in range(1, case.frames):
        st = NL.stage(rec, f, "solve")
        en = st["energy"].view(F32)
        turned = RL.rotations_changed(rec, f)
        print("frame %d: nodes moved %d, turned %d, energies %s" % (f, int(st["moved"]), turned, en))
        assert turned >= 1 and en[1] < en[0]
    plane, _ = PL.run_oracle_loop(case)
    assert not np.array_equal(NL.stage(rec, 1, "solve")["dq"], NL.stage(plane, 1, "solve")["dq"])
