"""The projective data association through the C++ mirror: the `associate` app (kfusion::cuda::associateProjective) against the numpy
restatement bit for bit, and kfusion::KinFu with KinFuParams::warp_projective_association through kinfu_headless (mode word `assoc`):
4 frames at 64^3 / 160 x 120, it tracks on every frame, pairs points on every frame >= 1 and fuses a different volume than the same
input without the association."""
import re
import subprocess

import numpy as np
import pytest

import associate_ref as AR
from dynamicfusion_amd import build, synth
from test_gpu_associate import random_set

pytestmark = pytest.mark.gpu
F32 = np.float32


def run_associate(tmp_path, points, normals, lp, ln, intr, dist, mc, margin):
    build.build_host()
    fin, fout = str(tmp_path / "assoc_in.bin"), str(tmp_path / "assoc_out.bin")
    n = len(points)
    rows, cols = lp.shape[:2]
    with open(fin, "wb") as f:
        f.write(np.array([n, cols, rows, 0 if normals is None else 1], np.int32).tobytes())
        f.write(np.array(list(intr) + [dist, mc, margin], F32).tobytes())
        f.write(np.ascontiguousarray(points, F32).tobytes())
        if normals is not None:
            f.write(np.ascontiguousarray(normals, F32).tobytes())
        f.write(np.ascontiguousarray(lp, F32).tobytes())
        if normals is not None:
            f.write(np.ascontiguousarray(ln, F32).tobytes())
    r = subprocess.run([build.HOST_ASSOCIATE, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(fout, np.uint8)
    assert raw.size == 12 * n + n + 64
    return raw[:12 * n].view(np.uint32).reshape(n, 3), raw[12 * n:13 * n], raw[13 * n:].view(np.uint64)


@pytest.mark.parametrize("with_normals", [True, False])
def test_cxx_associate_app_equals_the_restatement(tmp_path, with_normals):
    pts, nrm, lp, ln, intr = random_set(20000, seed=23)
    if not with_normals:
        nrm = ln = None
    for margin in (0.05, -1.0):
        want_live, want_st, want_cnt = AR.associate(pts, nrm, lp, ln, intr, 0.15, 0.6, margin)
        live, st, cnt = run_associate(tmp_path, pts, nrm, lp, ln, intr, 0.15, 0.6, margin)
        assert np.array_equal(live, want_live.view(np.uint32)) and np.array_equal(st, want_st) and np.array_equal(cnt, want_cnt)
        assert want_cnt[0] > 100


def test_cxx_kinfu_with_projective_association(tmp_path):
    cfg = synth.Config(64, 1.0, cols=160, rows=120, nodes=0, k=8)
    frames = 4
    build.build_host()
    fin, fout = str(tmp_path / "kin.bin"), str(tmp_path / "kout.bin")
    with open(fin, "wb") as f:
        f.write(np.asarray(cfg.intr, F32).tobytes())
        for i in range(frames):
            f.write(synth.depth_frame(cfg, 2 * i).tobytes())
    out = {}
    for mode in ("warped-assoc-trace", "warped"):
        r = subprocess.run([build.HOST_KINFU_APP, str(cfg.cols), str(cfg.rows), str(frames), str(cfg.dims[0]), str(cfg.size), fin, fout, mode],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = np.fromfile(fout, np.uint8)
        tracked = raw[:frames * 52].reshape(frames, 52)[:, :4].copy().view(np.int32).ravel()
        assert list(tracked) == [0] + [1] * (frames - 1), r.stdout + r.stderr       # (frame 0 only seeds the model, kinfu.cpp:246-265)
        out[mode] = (raw[frames * 52 + 8:].view(np.uint32), r.stderr)
    counts = {int(m.group(1)): [int(x) for x in m.group(2).split()]
              for m in re.finditer(r"assoc frame (\d+) tracked \d+ counts ((?:\d+ ?){8})", out["warped-assoc-trace"][1])}
    print(counts)
    assert sorted(counts) == list(range(frames))
    assert counts[0] == [0] * 8                                                     # frame 0 runs no association
    for f in range(1, frames):
        assert sum(counts[f]) == cfg.cols * cfg.rows and counts[f][0] > 0, (f, counts[f])
    assert "assoc frame" not in out["warped"][1]
    assert not np.array_equal(out["warped-assoc-trace"][0], out["warped"][0])
