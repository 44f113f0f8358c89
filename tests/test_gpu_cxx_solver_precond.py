"""The C++ mirror's switch for the node-block preconditioner (kfusion::WarpField::setPreconditioner): host/apps/warp_solve
`rigid ... pcg` prints the bits the Python mirror leaves on the same seeded problem with set_preconditioner(1) -- and not the plain
solve's, which the app prints as before without the word; and kinfu_headless with `rigid-pcg` runs KinFuParams::warp_precondition
through KinFu."""
import re
import subprocess

import numpy as np
import pytest
import torch

from dynamicfusion_amd import build, synth
from solver_cases import bits, dev, field, lcg_normals, lcg_problem

pytestmark = pytest.mark.gpu


def python_mirror(pcg, hier=False):
    pos, dq, sigma, src, dst = lcg_problem()
    nrm = dev(lcg_normals(len(src)))
    wf = field(pos, sigma, dq)
    if hier:
        wf.set_graph_hierarchy(2, 0.5, 2.0)
    if pcg:
        wf.set_preconditioner(1)
    out = wf.solve_rigid(dev(src), dev(dst), nrm, iters=20, lam=1e-3, lam_rot=0.01, reg_neighbours=4, reg_lambda=1.0, rounds=3, tukey_c=0.02,
                         huber_delta=0.01)
    torch.cuda.synchronize()
    return bits(out[0].cpu().numpy()), bits(out[1].cpu().numpy())


def app(*words):
    build.build_host()
    r = subprocess.run([build.HOST_WARP_SOLVE] + list(words), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [[int(w, 16) for w in line.split()] for line in r.stdout.strip().splitlines()]
    return np.array(lines[:-1], np.uint32), np.array(lines[-1], np.uint32)


@pytest.mark.parametrize("words", [("rigid", "pcg"), ("rigid", "hier", "pcg"), ("rigid", "4", "1", "3", "0.02", "0.01", "pcg")], ids=" ".join)
def test_cxx_mirror_with_pcg_prints_the_python_mirrors_bits(words):
    got_dq, got_en = app(*words)
    want_dq, want_en = python_mirror(True, "hier" in words)
    assert got_dq.shape == (50, 8)
    assert np.array_equal(got_dq, want_dq) and np.array_equal(got_en, want_en)
    plain_dq, _ = python_mirror(False, "hier" in words)      # and the word did something
    assert not np.array_equal(got_dq, plain_dq)


def test_without_the_word_the_app_prints_what_it_printed():
    got_dq, got_en = app("rigid")
    want_dq, want_en = python_mirror(False)
    assert np.array_equal(got_dq, want_dq) and np.array_equal(got_en, want_en)


def test_cxx_kinfu_with_the_preconditioner(tmp_path):
    """KinFuParams::warp_precondition through kinfu_headless's word `pcg` beside `rigid`: 3 frames at 64^3 / 160 x 120.  Every frame
    tracks; frame 0 has no solve and is what it is without the word; from frame 1 on the node transforms differ from the plain
    recurrence's; and the word gives the same frames twice."""
    frames = 3
    cfg = synth.Config(64, 1.0, cols=160, rows=120, nodes=0, k=8)
    build.build_host()
    fin, fout = str(tmp_path / "kin.bin"), str(tmp_path / "kout.bin")
    with open(fin, "wb") as f:
        f.write(np.asarray(cfg.intr, np.float32).tobytes())
        for i in range(frames):
            f.write(synth.depth_frame(cfg, 2 * i).tobytes())

    def run(mode):
        r = subprocess.run([build.HOST_KINFU_APP, str(cfg.cols), str(cfg.rows), str(frames), str(cfg.dims[0]), str(cfg.size), fin, fout, mode],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        tracked = np.fromfile(fout, np.uint8)[:frames * 52].reshape(frames, 52)[:, :4].copy().view(np.int32).ravel()
        assert list(tracked) == [0] + [1] * (frames - 1), r.stdout + r.stderr
        trace = {int(m.group(1)): m.group(3) for m in re.finditer(r"trace frame (\d+) volume ([0-9a-f]+) nodes ([0-9a-f]+)", r.stderr)}
        assert sorted(trace) == list(range(frames)), r.stderr
        return trace
    pcg, again, plain = run("warped-rigid-pcg-trace"), run("warped-rigid-pcg-trace"), run("warped-rigid-trace")
    print(pcg, plain)
    assert pcg == again
    assert pcg[0] == plain[0]
    for f in range(1, frames):
        assert pcg[f] != plain[f], "frame %d: the preconditioner left the plain recurrence's transforms" % f
