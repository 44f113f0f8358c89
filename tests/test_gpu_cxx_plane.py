"""The point-to-plane warp solve through kfusion::KinFu (KinFuParams::warp_point_to_plane, kinfu_headless's mode word `plane`) together
with the projective association: 4 frames at 64^3 / 160 x 120.  It tracks on every frame; frame 1's association -- which runs before the
first solve -- counts what it counts without the flag; from frame 1 on the node transforms differ from the point-to-point run's, and so
does the fused volume."""
import re
import subprocess

import numpy as np
import pytest

from dynamicfusion_amd import build, synth

pytestmark = pytest.mark.gpu
F32 = np.float32


def test_cxx_kinfu_with_the_plane_solve(tmp_path):
    cfg = synth.Config(64, 1.0, cols=160, rows=120, nodes=0, k=8)
    frames = 4
    build.build_host()
    fin, fout = str(tmp_path / "kin.bin"), str(tmp_path / "kout.bin")
    with open(fin, "wb") as f:
        f.write(np.asarray(cfg.intr, F32).tobytes())
        for i in range(frames):
            f.write(synth.depth_frame(cfg, 2 * i).tobytes())
    out = {}
    for mode in ("warped-assoc-plane-trace", "warped-assoc-trace"):
        r = subprocess.run([build.HOST_KINFU_APP, str(cfg.cols), str(cfg.rows), str(frames), str(cfg.dims[0]), str(cfg.size), fin, fout, mode],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = np.fromfile(fout, np.uint8)
        tracked = raw[:frames * 52].reshape(frames, 52)[:, :4].copy().view(np.int32).ravel()
        assert list(tracked) == [0] + [1] * (frames - 1), r.stdout + r.stderr       # (frame 0 only seeds the model, kinfu.cpp:246-265)
        nodes = {int(m.group(1)): m.group(2) for m in re.finditer(r"trace frame (\d+) volume [0-9a-f]+ nodes ([0-9a-f]+)", r.stderr)}
        counts = {int(m.group(1)): [int(x) for x in m.group(2).split()]
                  for m in re.finditer(r"assoc frame (\d+) tracked \d+ counts ((?:\d+ ?){8})", r.stderr)}
        assert sorted(nodes) == sorted(counts) == list(range(frames)), r.stderr
        out[mode] = (raw[frames * 52 + 8:].view(np.uint32), nodes, counts)
    (p_vol, p_nodes, p_counts), (q_vol, q_nodes, q_counts) = out["warped-assoc-plane-trace"], out["warped-assoc-trace"]
    print(p_nodes, q_nodes, p_counts)
    assert p_nodes[0] == q_nodes[0] and p_counts[1] == q_counts[1] and p_counts[1][0] > 0
    for f in range(1, frames):
        assert p_nodes[f] != q_nodes[f], "frame %d: the plane solve left the point-to-point solve's transforms" % f
        assert sum(p_counts[f]) == cfg.cols * cfg.rows and p_counts[f][0] > 0
    assert not np.array_equal(p_vol, q_vol)
