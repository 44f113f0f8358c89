"""The closed non-rigid frame loop (tests/nonrigid_loop.py, FAST: 64^3, 160 x 120, 7 frames, extend inside) with the association in
front of the solve with node rotations, regularised over the hierarchical node graph and preconditioned with the 6x6 node blocks
(tests/hier_precond_loop.py).  The GPU backend sets the hierarchy (2 levels, radius 0.08, beta 4) and the preconditioner once after
init_field; the field then grows by 14 nodes on each of six frames.  Every recorded stage of every frame is equal to the restatement's
bit for bit, and so are, after init_field and after every extend, the graph (neighbours, alpha), the levels (top, sizes, effective) and
the preconditioner setting the handle reports.  On the last frame the same solve on a second handle that was given the loop handle's
nodes and settings gives the loop handle's bits, twice.

(a) k = 8, one round, quadratic penalties; (b) k = 4, two rounds with Tukey and Huber on (solver_cases.TUKEY_C, HUBER_DELTA): the
blocks carry the scaled weights.  The conditions on the inputs (hier_precond_loop.nonvacuity) are taken from the oracle's record alone."""
import numpy as np
import pytest

import hier_precond_loop as HP
import nonrigid_loop as NL

pytestmark = pytest.mark.gpu
CASES = {"a": (NL.FAST, HP.QUADRATIC), "b": (NL.FAST.with_k(4), HP.ROBUST)}


@pytest.fixture(scope="module", params=sorted(CASES))
def loops(request):
    """(case, the oracle's record and backend, the GPU's record and backend): each loop runs once per case."""
    case, setting = CASES[request.param]
    want, oracle = HP.run_oracle_loop(case, setting, compare_plain=True)
    be = HP.HierPrecondGpuBackend(case, setting)
    got = NL.run(be, case)
    return case, want, oracle, got, be


def test_the_inputs_deserve_the_test(loops):
    case, want, oracle, _, _ = loops
    print("level sizes per frame:", HP.level_sizes(oracle), "rows off the flat graph:", oracle.flat_rows)
    assert HP.nonvacuity(want, oracle, case) == []


def test_every_stage_equals_the_restatement(loops):
    case, want, oracle, got, be = loops
    msg = NL.first_difference(got, want)
    print("%s: %s" % (case.name, NL.summary(got, case) if msg is None else None))
    assert msg is None, "GPU against the restatement: " + msg
    assert NL.nonvacuity(got, case) == []
    assert sorted(be.assoc) == sorted(oracle.assoc) == list(range(1, case.frames))
    for f in range(1, case.frames):
        for item in ("live", "status", "counts", "back"):
            assert np.array_equal(be.assoc[f][item], oracle.assoc[f][item]), "frame %d: the association's %s differs" % (f, item)


def test_graph_levels_and_setting_follow_every_extend(loops):
    case, _, oracle, _, be = loops
    msg = HP.graph_difference(be.graph, oracle.graph)
    assert msg is None, "the handle's graph against the restatement on the oracle's nodes: " + msg
    assert all(be.graph[f]["preconditioner"] == HP.PRECOND and be.graph[f]["effective"] == 2 for f in range(case.frames))


def test_a_second_handle_with_the_same_state_repeats_the_last_solve(loops):
    case, want, _, _, be = loops
    assert be.repeat is not None
    (dq, en), first, second = be.repeat
    for name, (d, e) in (("first", first), ("second", second)):
        assert np.array_equal(d, dq), "last frame, %s call on the second handle: %d transform words differ" % (name, int((d != dq).sum()))
        assert np.array_equal(e, en), "last frame, %s call on the second handle: energies %s against %s" % (name, e.view(np.float32), en.view(np.float32))
    last = NL.stage(want, case.frames - 1, "solve")
    assert np.array_equal(dq, last["dq"]) and np.array_equal(en, last["energy"])
