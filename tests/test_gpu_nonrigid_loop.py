"""The closed non-rigid frame loop on the GPU against the oracle, stage by stage (tests/nonrigid_loop.py):

    depth -> bilateral -> pyramid -> point normals -> ICP -> ray-cast -> transform_points -> warp -> solve the data term -> warp ->
    extend -> compute_dists -> warped integrate -> ray-cast -> resize

Both backends run free, each feeding itself, on ONE warp-field handle and one volume for the whole sequence; every recorded stage of every
frame -- images, pose, node set {pos, dq, sigma}, energies, n_added / n_winners, update count, the whole volume -- must be equal bit for
bit.  The first stage that differs names the culprit, because its inputs were still equal.  The cases vary what drives the handle's
state machine, not its arithmetic: k = 8 / 4, tables on demand / eager, the single call / prepare on a second stream + sweep (which also
shows that a pending plan is void after a second transforms update -- the solver's write-back being the first -- and after an extend
that adds nodes), and a 13-frame 128^3 case that runs past the second-sweep blend models, the third-sweep codes and the every-8th-sweep
prefetch probe, with default and with steady prefetch and a second volume swept with cull off through the same handle.

tests/test_oracle_nonrigid_loop.py proves on the CPU that the inputs satisfy the non-vacuity conditions asserted here.

Measured wall time of this file on an MI355X host: 5.6 s for the 10 cases (the long case 2.0 s, of which its one oracle run 1.1 s on the
host's 16 cores; a fast case 0.05 - 0.5 s)."""
import time

import numpy as np
import pytest

import nonrigid_loop as NL

pytestmark = pytest.mark.gpu
_oracle = {}


def oracle_record(case):
    """The oracle loop depends on the case's sizes and k only: one run serves every GPU configuration of it."""
    key = (case.name, case.k)
    if key not in _oracle:
        rec = NL.run(NL.OracleBackend(case), case)
        assert NL.nonvacuity(rec, case) == [], "the inputs no longer deserve the test"
        _oracle[key] = rec
    return _oracle[key]


def check(case, be, on_frame=None):
    t0 = time.time()
    want = oracle_record(case)
    t1 = time.time()
    got = NL.run(be, case, on_frame=on_frame)
    msg = NL.first_difference(got, want)
    s = NL.summary(got, case) if msg is None else None
    print("%s k=%d: oracle %.1f s, gpu %.1f s; %s; kept blocks %s, coded %s" % (case.name, case.k, t1 - t0, time.time() - t1, s, be.kept, be.coded))
    assert msg is None, "GPU against oracle: " + msg
    assert NL.nonvacuity(got, case) == []
    return got


@pytest.mark.parametrize("call", ["single", "split"])
@pytest.mark.parametrize("tables", ["on_demand", "eager"])
@pytest.mark.parametrize("k", [8, 4])
def test_fast_case_equals_oracle_at_every_stage(k, tables, call):
    case = NL.FAST.with_k(k)
    be = NL.GpuBackend(case, tables_on_demand=(tables == "on_demand"), split=(call == "split"))
    check(case, be)
    if call == "split":
        # the voiding rules of include/dfusion.h were met on the way (the asserts are in GpuBackend): a plan prepared before the solver
        # and followed by the solver's write-back plus one set_transforms, and a plan prepared before an extend that added nodes
        assert be.voided["second_update"] == 1 and be.voided["extend"] >= 1, be.voided


@pytest.mark.parametrize("prefetch", [True, "steady"], ids=["default_prefetch", "steady_prefetch"])
def test_long_case_equals_oracle_at_every_stage(prefetch):
    case = NL.LONG
    assert case.frames >= 12 and case.k == 8 and case.cfg.dims == (128, 128, 128) and (case.cfg.cols, case.cfg.rows) == (320, 240)
    be = NL.GpuBackend(case, prefetch=prefetch, cull_off=True)

    def culled_equals_unculled(f, be):
        a, b = be.volume(), be.volume2()
        assert np.array_equal(a, b), "frame %d: %d voxels of the cull-off volume differ" % (f, int((a != b).sum()))

    check(case, be, on_frame=culled_equals_unculled)
    assert len(be.coded) == case.frames - 1
    first = next((i for i, c in enumerate(be.coded) if c > 0), None)
    assert first is not None and all(c > 0 for c in be.coded[first:]), "coded blocks per frame: %s" % be.coded
    assert all(kept > 0 for kept in be.kept)
