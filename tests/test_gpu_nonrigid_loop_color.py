"""The closed non-rigid frame loop (tests/nonrigid_loop.py, FAST: 64^3, 160 x 120, 7 frames, extend inside) with the frame's colour image
fused after every integrate (tests/color_loop.py): the GPU backend through ColorVolume on the loop's volume and warp-field handle, the
oracle backend through the numpy restatement tests/color_ref.py on its own volume and nodes.  The colour volume of every frame is equal
bit for bit, and so are the counts; every other recorded stage equals the run WITHOUT colour, on both sides: the colour reads the
geometry and the warp field and changes neither."""
import numpy as np
import pytest

import color_loop as CL
import nonrigid_loop as NL

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("call", ["single", "split"])
def test_fast_case_with_colour_equals_the_restatement_at_every_frame(call):
    case = NL.FAST
    oracle = CL.ColorOracleBackend(case)
    want = NL.run(oracle, case)
    assert NL.nonvacuity(want, case) == [], "the inputs no longer deserve the test"
    plain = NL.run(NL.OracleBackend(case), case)
    assert NL.first_difference(want, plain) is None                       # the restatement's colour leaves the oracle loop alone
    be = CL.ColorGpuBackend(case, split=(call == "split"))
    got = NL.run(be, case)
    msg = NL.first_difference(got, plain)
    assert msg is None, "GPU with colour against the loop without: " + msg
    assert sorted(be.colors) == sorted(oracle.colors) == list(range(case.frames))
    for f in range(case.frames):
        g, w = be.colors[f], oracle.colors[f]
        print("frame %d: selected, fused %s" % (f, be.counts[f]))
        assert be.counts[f] == oracle.counts[f] and be.counts[f][1] > 1000, (f, be.counts[f], oracle.counts[f])
        assert np.array_equal(g, w), "frame %d: %d voxels differ" % (f, int((g != w).any(-1).sum()))
    last = be.colors[case.frames - 1]
    assert last[..., 3].max() == CL.MAX_WEIGHT and (last[..., 3] == CL.MAX_WEIGHT).sum() > 1000
    assert len(np.unique(last[last[..., 3] > 0][:, :3], axis=0)) > 2       # averages across checker cells exist
    assert NL.nonvacuity(got, case) == []
