"""The C++ mirror's switch for the hierarchical node graph (kfusion::WarpField::setRegularisationHierarchy): host/apps/
warp_solve with the word `hier` prints, for each of the four solves, the bits the Python mirror leaves on the same seeded problem with
set_graph_hierarchy(2, 0.5, 2) -- and not the flat graph's; and kinfu_headless with `hier` runs KinFuParams::warp_reg_levels through KinFu."""
import re
import subprocess

import numpy as np
import pytest
import torch

import solver_hier_ref as H
from dynamicfusion_amd import build, synth
from solver_cases import bits, dev, field, lcg_normals, lcg_problem

pytestmark = pytest.mark.gpu
SETTING = (2, 0.5, 2.0)


def python_mirror(mode, hier):
    pos, dq, sigma, src, dst = lcg_problem()
    nrm = dev(lcg_normals(len(src)))
    wf = field(pos, sigma, dq)
    if hier:
        wf.set_graph_hierarchy(*SETTING)
    kw = dict(iters=20, lam=1e-3, reg_neighbours=4, reg_lambda=1.0)
    if mode == "reg":
        out = wf.solve(dev(src), dev(dst), **kw)
    elif mode == "robust":
        out = wf.solve_robust(dev(src), dev(dst), rounds=3, tukey_c=0.04, huber_delta=0.01, **kw)
    elif mode == "plane":
        out = wf.solve_plane(dev(src), dev(dst), nrm, rounds=3, tukey_c=0.02, huber_delta=0.01, **kw)
    else:
        out = wf.solve_rigid(dev(src), dev(dst), nrm, lam_rot=0.01, rounds=3, tukey_c=0.02, huber_delta=0.01, **kw)
    torch.cuda.synchronize()
    return bits(out[0].cpu().numpy()), bits(out[1].cpu().numpy())


@pytest.mark.parametrize("mode", ["reg", "robust", "plane", "rigid"])
def test_cxx_mirror_with_hier_prints_the_python_mirrors_bits(mode):
    build.build_host()
    r = subprocess.run([build.HOST_WARP_SOLVE, mode, "hier"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [[int(w, 16) for w in line.split()] for line in r.stdout.strip().splitlines()]
    got_dq = np.array(lines if mode == "reg" else lines[:-1], np.uint32)
    want_dq, want_en = python_mirror(mode, True)
    assert got_dq.shape == (50, 8)
    assert np.array_equal(got_dq, want_dq)
    if mode != "reg":                                        # (`reg` prints no energies)
        assert np.array_equal(np.array(lines[-1], np.uint32), want_en)
    flat_dq, _ = python_mirror(mode, False)                  # and the word did something: the flat graph's answer differs
    assert not np.array_equal(got_dq, flat_dq)


def test_the_mirrors_setting_has_two_effective_levels():
    pos = lcg_problem()[0]
    _, _, sizes, eff = H.levels(pos, 4, *SETTING)
    assert eff == 2 and sizes[1] > sizes[2] >= 5


def test_arguments_with_hier_after_them():
    build.build_host()
    a = subprocess.run([build.HOST_WARP_SOLVE, "reg", "4", "1", "hier"], capture_output=True, text=True, timeout=120)
    b = subprocess.run([build.HOST_WARP_SOLVE, "reg", "hier"], capture_output=True, text=True, timeout=120)
    assert a.returncode == 0 and b.returncode == 0 and a.stdout == b.stdout and len(a.stdout.splitlines()) == 50


def test_cxx_kinfu_with_the_hierarchy(tmp_path):
    """KinFuParams::warp_reg_levels through kinfu_headless's word `hier`, beside `rigid` (which switches the term on at 4 neighbours,
    weight 1): 3 frames at 64^3 / 160 x 120.  Every frame tracks; frame 0 has no solve and is what it is without the word; from frame 1
    on the node transforms differ from the flat graph's run; and the word gives the same frames twice."""
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
    hier, again, flat = run("warped-rigid-hier-trace"), run("warped-rigid-hier-trace"), run("warped-rigid-trace")
    print(hier, flat)
    assert hier == again
    assert hier[0] == flat[0]
    for f in range(1, frames):
        assert hier[f] != flat[f], "frame %d: the hierarchy left the flat graph's transforms" % f
