"""The mesh tail of the closed non-rigid loop (tests/mesh_tail_loop.py) on the oracle backend alone: the proof, on a machine without a
GPU, that the loop's fused surface on frames 3 and 6 deserves what tests/test_gpu_nonrigid_loop_mesh_tail.py compares -- the conditions
of mesh_tail_loop.nonvacuity hold and the figures are the pinned ones."""
import pytest

import mesh_tail_loop as MT
import nonrigid_loop as NL
from test_gpu_nonrigid_loop_mesh_tail import CASE, FIGURES


@pytest.fixture(scope="module")
def loop():
    return MT.run(MT.TailOracleBackend(CASE), CASE, MT.oracle_tail)


@pytest.mark.parametrize("frame", MT.TAIL_FRAMES)
def test_the_fused_surface_deserves_the_tail(loop, frame):
    rec, tails = loop
    assert NL.nonvacuity(rec, CASE) == []
    fig = MT.figures(tails[frame])
    print("frame %d: %s" % (frame, fig))
    assert MT.nonvacuity(fig) == []
    assert fig == FIGURES[frame]


def test_the_comparison_can_fail_and_says_where(loop):
    """A tail whose filtered normals were gathered by the NEW index instead of vertex_src differs first at step 3's normals."""
    _, tails = loop
    want = tails[MT.TAIL_FRAMES[0]]
    assert MT.first_difference({k: v for k, v in want.items() if not k.startswith(MT.ORACLE_ONLY)}, want) is None
    wrong = dict(want)
    wrong["3.normals"] = want["1.normals"][:len(want["3.vertex_src"])]
    msg = MT.first_difference(wrong, want)
    assert msg is not None and msg.startswith("3.normals:"), msg
