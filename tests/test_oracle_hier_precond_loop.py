"""The closed non-rigid frame loop with the hierarchical graph and the node-block preconditioner (tests/hier_precond_loop.py) on the
oracle backend alone, case (a): FAST, k = 8, one quadratic round.  The proof, on a machine without a GPU, that the inputs deserve what
tests/test_gpu_nonrigid_loop_hier_precond.py asserts: the loop's own conditions hold, every frame has 2 effective levels and a graph that
is not the flat one, every solve turns nodes and differs in bits from the solve without the preconditioner.  The figures of the run are
pinned: the node counts, the update counts and the level sizes per frame.

The preconditioner's effect at the loop's budget (4 steps, one round), measured on the restatement on the same inputs per frame: the
data energy after the solve is lower with the node blocks than without on every frame (0.0085 against 0.0146 on frame 1, 0.0086 against
0.0233 on frame 6; all frames in DESIGN.md 25), and so is E_data + lambda_reg E_reg."""
import numpy as np
import pytest

import hier_precond_loop as HP
import nonrigid_loop as NL

F32 = np.float32
SIZES = {0: [102, 32, 12], 1: [116, 42, 14], 2: [130, 51, 14], 3: [144, 56, 14], 4: [158, 60, 14], 5: [172, 67, 15], 6: [186, 72, 16]}
UPDATED = [142696, 142960, 141850, 137554, 137271, 139773, 139616]


@pytest.fixture(scope="module")
def loop():
    rec, be = HP.run_oracle_loop(NL.FAST, HP.QUADRATIC, compare_plain=True)
    return NL.FAST, rec, be


def test_inputs_deserve_the_nonvacuity_conditions(loop):
    case, rec, be = loop
    assert HP.nonvacuity(rec, be, case) == []
    assert all(be.plain[f]["differs"] for f in range(1, case.frames))


def test_the_figures_of_the_run(loop):
    case, rec, be = loop
    s = NL.summary(rec, case)
    print(s, HP.level_sizes(be))
    assert (s["frames"], s["M0"], s["M"]) == (7, 102, 186)
    assert s["added"] == {f: 14 for f in range(1, 7)}
    assert s["updated"] == UPDATED
    assert all(0.5 < x < 0.55 for x in s["finite"])
    assert HP.level_sizes(be) == SIZES
    assert all(be.graph[f]["effective"] == 2 and be.graph[f]["preconditioner"] == 1 for f in range(case.frames))
    for f in range(case.frames):
        top = be.graph[f]["top"]
        assert [int((top >= l).sum()) for l in range(3)] == SIZES[f]


def test_the_graph_is_rebuilt_on_every_frame(loop):
    """What a stale level would be: the graph of frame f is not that of frame f - 1 with rows appended -- old nodes change their
    neighbours when the field grows."""
    case, _, be = loop
    for f in range(1, case.frames):
        old, new = be.graph[f - 1]["nbr"], be.graph[f]["nbr"]
        assert len(new) == len(old) + 14
        assert (new[:len(old)] != old).any(1).sum() >= 1, "frame %d: no old node changed a neighbour" % f


def test_the_preconditioner_lowers_the_energy_at_this_budget(loop):
    case, _, be = loop
    for f in range(1, case.frames):
        pre, plain = be.plain[f]["energy"], be.plain[f]["energy_plain"]
        print("frame %d: E_data, E_reg after: node blocks %.6f %.6f, none %.6f %.6f" % (f, pre[1], pre[3], plain[1], plain[3]))
        assert pre[0] == plain[0] and pre[2] == plain[2]                     # the same inputs
        assert pre[1] < plain[1] < plain[0]
        assert pre[1] + F32(HP.LAMBDA_REG) * pre[3] < plain[1] + F32(HP.LAMBDA_REG) * plain[3]
