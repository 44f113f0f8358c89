"""The warp solve with node rotations through kfusion::KinFu (KinFuParams::warp_solve_rotations, kinfu_headless's mode word `rigid`)
together with the projective association: 4 frames at 64^3 / 160 x 120.  The device-resident branch hands the solve copies of the
canonical points and normals from before the first warp.  It tracks on every frame; frame 0 and frame 1's association -- which runs
before the first solve -- are what they are without the flag; from frame 1 on the node transforms and the fused volume differ from the
plane run's and from the flag-off run's; and the flag-off run gives the same frames twice (what it computes is pinned against the
oracle by the older C++ tests, which run without the flag)."""
import re
import subprocess

import numpy as np
import pytest

from dynamicfusion_amd import build, synth

pytestmark = pytest.mark.gpu
F32 = np.float32
FRAMES = 4


def run(cfg, fin, fout, mode):
    r = subprocess.run([build.HOST_KINFU_APP, str(cfg.cols), str(cfg.rows), str(FRAMES), str(cfg.dims[0]), str(cfg.size), fin, fout, mode],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(fout, np.uint8)
    tracked = raw[:FRAMES * 52].reshape(FRAMES, 52)[:, :4].copy().view(np.int32).ravel()
    assert list(tracked) == [0] + [1] * (FRAMES - 1), r.stdout + r.stderr           # (frame 0 only seeds the model, kinfu.cpp:246-265)
    trace = {int(m.group(1)): (m.group(2), m.group(3)) for m in re.finditer(r"trace frame (\d+) volume ([0-9a-f]+) nodes ([0-9a-f]+)", r.stderr)}
    counts = {int(m.group(1)): [int(x) for x in m.group(2).split()]
              for m in re.finditer(r"assoc frame (\d+) tracked \d+ counts ((?:\d+ ?){8})", r.stderr)}
    assert sorted(trace) == sorted(counts) == list(range(FRAMES)), r.stderr
    return raw[FRAMES * 52 + 8:].view(np.uint32).copy(), trace, counts


def test_cxx_kinfu_with_the_rigid_solve(tmp_path):
    cfg = synth.Config(64, 1.0, cols=160, rows=120, nodes=0, k=8)
    build.build_host()
    fin, fout = str(tmp_path / "kin.bin"), str(tmp_path / "kout.bin")
    with open(fin, "wb") as f:
        f.write(np.asarray(cfg.intr, F32).tobytes())
        for i in range(FRAMES):
            f.write(synth.depth_frame(cfg, 2 * i).tobytes())
    r_vol, r_trace, r_counts = run(cfg, fin, fout, "warped-assoc-rigid-trace")
    p_vol, p_trace, p_counts = run(cfg, fin, fout, "warped-assoc-plane-trace")
    q_vol, q_trace, q_counts = run(cfg, fin, fout, "warped-assoc-trace")
    q2_vol, q2_trace, q2_counts = run(cfg, fin, fout, "warped-assoc-trace")
    print(r_trace, p_trace, q_trace, r_counts)
    assert q_trace == q2_trace and q_counts == q2_counts and np.array_equal(q_vol, q2_vol)     # the flag off: the same frames
    assert r_trace[0] == q_trace[0] == p_trace[0] and r_counts[1] == q_counts[1] and r_counts[1][0] > 0
    for f in range(1, FRAMES):
        for name, other in (("plane", p_trace), ("flag-off", q_trace)):
            assert r_trace[f][1] != other[f][1], "frame %d: the rigid solve left the %s run's transforms" % (f, name)
            assert r_trace[f][0] != other[f][0], "frame %d: the rigid solve left the %s run's volume" % (f, name)
        assert sum(r_counts[f]) == cfg.cols * cfg.rows and r_counts[f][0] > 0
    assert not np.array_equal(r_vol, p_vol) and not np.array_equal(r_vol, q_vol)
