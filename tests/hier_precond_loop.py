"""Backends of the closed non-rigid loop (tests/nonrigid_loop.py) with the association in front of the solve with node rotations
(tests/rigid_loop.py), regularised over the HIERARCHICAL node graph (dfusion_warp_set_graph_hierarchy) and with the 6x6
node-block preconditioner (dfusion_warp_set_preconditioner).  The GPU backend makes both settings ONCE, right after
init_field, and never again: the field then grows on six consecutive frames, and the graph, its transpose and the blocks have to follow
on the one handle.  The oracle backend calls the numpy restatement tests/solver_precond_ref.py inside solver_hier_ref.hierarchy on its
own nodes.  kg, lambda_reg, lambda, lambda_rot and the step count are rigid_loop's.  The two solves replace rigid_loop's at the end of
the method resolution order, behind the association.

LEVELS = 2, RADIUS = 0.08, BETA = 4 on the FAST case (k = 8, one quadratic round): the level sizes are 102 / 32 / 12 after init_field
and 186 / 72 / 16 after the last extend, and both levels are effective on every frame, so the radius needed no lowering (per frame, and
for k = 4 with the robust penalties; rigid_loop's own field, solved over the flat graph, ends at 186 / 75 / 17).

Beside the stage record both backends keep, per frame (0: after init_field, f >= 1: after the frame's extend),
    graph[f] = dict(nbr, alpha (bits), top, sizes, effective, preconditioner)
the GPU side from WarpField.node_graph / graph_levels / preconditioner, the oracle side from solver_hier_ref.hier_graph / levels on its
nodes.  The oracle backend also keeps what the non-vacuity conditions need: flat_rows[f], the number of nodes whose neighbour row is not
the flat solver_reg_ref.node_graph's, and with compare_plain, plain[f] = dict(differs, energy, energy_plain): whether the frame's
transforms differ in bits from those of precond = 0 on the same inputs, and both energy vectors.  On the last frame the GPU backend makes
the frame's solve twice more on a second handle given the loop handle's nodes and the same two settings (repeat = the three results)."""
import numpy as np

import nonrigid_loop as NL
import rigid_loop as RL
import solver_hier_ref as H
import solver_precond_ref as PC
import solver_reg_ref as R
from plane_loop import KG, LAMBDA_REG
from solver_cases import HUBER_DELTA, TUKEY_C

F32 = np.float32
LEVELS, RADIUS, BETA = 2, 0.08, 4.0
PRECOND = 1


class Setting:
    """The penalties of a loop: (a) one quadratic round, (b) two rounds with Tukey and Huber on."""

    def __init__(self, rounds=1, tukey_c=0.0, huber_delta=0.0):
        self.rounds, self.tukey_c, self.huber_delta = int(rounds), float(tukey_c), float(huber_delta)


QUADRATIC = Setting()
ROBUST = Setting(2, TUKEY_C, HUBER_DELTA)


def graph_items(nbr, alpha, top, sizes, effective, preconditioner):
    return dict(nbr=np.asarray(nbr, np.int32), alpha=NL._bits(np.asarray(alpha, F32)), top=np.asarray(top, np.int32),
                sizes=np.asarray(sizes, np.int32).reshape(-1), effective=int(np.asarray(effective).reshape(-1)[0]),
                preconditioner=int(preconditioner))


# ------------------------------------------------------------------------------------------------------------------ oracle
class _OracleHierPrecondSolve(RL._OracleRigidSolve):
    def solve(self, canonical, live, frame):
        s = self.setting
        args = (self.pos, self.dq, self.sig, self.rigid_points, live, self.rigid_normals, self.k, self.case.iters, self.case.lam, self.case.lam,
                KG, LAMBDA_REG, s.rounds, s.tukey_c, s.huber_delta)
        with H.hierarchy(LEVELS, RADIUS, BETA):
            dq, en, _, _ = PC.solve_rigid(*args, precond=PRECOND)
            if self.compare_plain:
                dq0, en0, _, _ = PC.solve_rigid(*args, precond=0)
                self.plain[frame] = dict(differs=not np.array_equal(NL._bits(dq), NL._bits(dq0)), energy=en.copy(), energy_plain=en0.copy())
        self.dq = dq
        return en


class HierPrecondOracleBackend(RL.RigidOracleBackend, _OracleHierPrecondSolve):
    def __init__(self, case, setting=QUADRATIC, compare_plain=False):
        super().__init__(case)
        self.setting, self.compare_plain = setting, bool(compare_plain)
        self.graph, self.flat_rows, self.plain = {}, {}, {}

    def _keep_graph(self, frame):
        nbr, alpha = H.hier_graph(self.pos, self.sig, KG, LEVELS, RADIUS, BETA)
        _, top, sizes, eff = H.levels(self.pos, KG, LEVELS, RADIUS, BETA)
        self.graph[frame] = graph_items(nbr, alpha, top, sizes, eff, PRECOND)
        self.flat_rows[frame] = int((nbr != R.node_graph(R.f32(self.pos), R.f32(self.sig), KG)[0]).any(1).sum())

    def init_field(self, pos):
        super().init_field(pos)
        self._keep_graph(0)

    def extend(self, pts, frame):
        out = super().extend(pts, frame)
        self._keep_graph(frame)
        return out


# --------------------------------------------------------------------------------------------------------------------- GPU
class _GpuHierPrecondSolve(RL._GpuRigidSolve):
    def _call(self, wf, live):
        s = self.setting
        dq, en = wf.solve_rigid(self.rigid_points, live, self.rigid_normals, iters=self.case.iters, lam=self.case.lam, lam_rot=self.case.lam,
                                reg_neighbours=KG, reg_lambda=LAMBDA_REG, rounds=s.rounds, tukey_c=s.tukey_c, huber_delta=s.huber_delta)
        return NL._bits(dq.cpu().numpy()), NL._bits(en.cpu().numpy())

    def solve(self, canonical, live, frame):
        last = frame == self.case.frames - 1
        if last:
            from dynamicfusion_amd import WarpField
            pos, _, sig = self.wf._keep
            dq0 = self.wf._dq.clone()
            twin = WarpField(k=self.k)
            twin.set_nodes(pos.clone(), dq0.clone(), sig.clone())
            twin.set_point_tiling(self.cfg.cols)
            twin.set_graph_hierarchy(LEVELS, RADIUS, BETA)
            twin.set_preconditioner(PRECOND)
        mine = self._call(self.wf, live)
        if last:
            first = self._call(twin, live)
            twin.set_transforms(dq0)
            self.repeat = (mine, first, self._call(twin, live))
        return mine[1].view(F32)


class HierPrecondGpuBackend(RL.RigidGpuBackend, _GpuHierPrecondSolve):
    def __init__(self, case, setting=QUADRATIC):
        super().__init__(case)
        self.setting = setting
        self.graph, self.repeat = {}, None

    def _keep_graph(self, frame):
        nbr, alpha = self.wf.node_graph(KG)
        top, sizes, eff = self.wf.graph_levels(KG)
        self.graph[frame] = graph_items(nbr.cpu().numpy(), alpha.cpu().numpy(), top.cpu().numpy(), sizes.cpu().numpy(), eff.cpu().numpy(),
                                        self.wf.preconditioner)

    def init_field(self, pos):
        super().init_field(pos)
        self.wf.set_graph_hierarchy(LEVELS, RADIUS, BETA)          # once, here: the settings have to survive every extend
        self.wf.set_preconditioner(PRECOND)
        self._keep_graph(0)

    def extend(self, pts, frame):
        out = super().extend(pts, frame)
        self._keep_graph(frame)
        return out


# --------------------------------------------------------------------------------------------------------------------- checks
def run_oracle_loop(case=NL.FAST, setting=QUADRATIC, compare_plain=True):
    """The oracle side alone: (record, backend)."""
    be = HierPrecondOracleBackend(case, setting, compare_plain)
    return NL.run(be, case), be


def graph_difference(got, want):
    """None, or a message naming the first (frame, item) of two backends' graph records that differs."""
    if sorted(got) != sorted(want):
        return "graphs kept on frames %s against %s" % (sorted(got), sorted(want))
    for f in sorted(want):
        for item in ("sizes", "effective", "top", "nbr", "alpha", "preconditioner"):
            g, w = np.asarray(got[f][item]), np.asarray(want[f][item])
            if g.shape != w.shape or g.dtype != w.dtype:
                return "frame %d, %s: %s %s against %s %s" % (f, item, g.dtype, g.shape, w.dtype, w.shape)
            if not np.array_equal(g, w):
                return "frame %d, %s: %d of %d elements differ" % (f, item, int((g != w).sum()), w.size)
    return None


def level_sizes(be):
    """{frame: [|S_0|, .., |S_LEVELS|]} of a backend's graph records."""
    return {f: [int(x) for x in be.graph[f]["sizes"][:LEVELS + 1]] for f in sorted(be.graph)}


def nonvacuity(rec, be, case):
    """The conditions of the issue on the ORACLE's record and backend; returns the list of those missed."""
    miss = list(NL.nonvacuity(rec, case))
    if sorted(be.graph) != list(range(case.frames)):
        return miss + ["graphs kept on frames %s" % sorted(be.graph)]
    for f in range(case.frames):
        if be.graph[f]["effective"] < 2:
            miss.append("frame %d: %d effective levels (sizes %s)" % (f, be.graph[f]["effective"], level_sizes(be)[f]))
        if be.flat_rows[f] < 1:
            miss.append("frame %d: every neighbour row is the flat graph's" % f)
    for f in range(1, case.frames):
        if RL.rotations_changed(rec, f) < 1:
            miss.append("frame %d: no node's rotation differs from its seed" % f)
    if be.compare_plain and not any(p["differs"] for p in be.plain.values()):
        miss.append("on every frame the transforms are those of precond = 0")
    return miss
