#!/usr/bin/env python3
"""Cost and effect of the 6x6 node-block preconditioner of the solve with rotations against the plain recurrence, in one
process, at the headline solve size (2000 surface nodes of synth.make_nodes, k = 8, the 307 200-point frame, kg = 4, lambda_reg = 1,
lambda = lambda_rot = 1e-3, point-to-point, one round) and at 8000 nodes:
  * a conjugate-gradient step each way: (time of a solve with 40 steps - time of one with 10) / 30;
  * what a round costs beside its steps each way (time of the 10-step solve - 10 steps), and the difference: the block assembly, the
    Cholesky factors and the preconditioned init in place of the plain one;
  * the steps each recurrence takes until it freezes (|r|^2 <= 1e-10 |r0|^2 plain, r.z <= 1e-10 (r.z)_0 preconditioned): the smallest
    `iters` whose transforms are those of a solve with CAP steps, by bisection (a frozen recurrence ignores further steps);
  * the wall time of a solve with exactly that many steps each way, and steps x step + round as the model of it.
Wall times around a device synchronise, medians of REPEATS after two warm-up rounds, the two modes alternating.  Prints one JSON line.
Usage: tools/solver_precond_probe.py [REPEATS] [--out FILE]"""
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, REPO)
from dynamicfusion_amd import WarpField, capi, synth  # noqa: E402

out = None
if "--out" in sys.argv:
    i = sys.argv.index("--out"); out = sys.argv[i + 1]; del sys.argv[i:i + 2]
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
KG, LREG, LAM, LROT, LO, HI, CAP = 4, 1.0, 1e-3, 1e-3, 10, 40, 6000
med = lambda a: float(np.median(a))  # noqa: E731


def sync_ms(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def surface(M):
    cfg = synth.Config(512, 3.0, nodes=M, k=8)
    pos, sigma = synth.make_nodes(cfg)
    rng = np.random.default_rng(5); N = cfg.cols * cfg.rows
    src = (pos[rng.integers(0, len(pos), N)] + rng.normal(0, 0.03, (N, 3))).astype(np.float32)
    dst = (src + 0.01 * np.sin(5 * src)).astype(np.float32)
    wf = WarpField(k=8); wf.init(pos, sigma=sigma)
    dq0 = wf._keep[1].clone()
    d_src, d_dst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()

    def solve(mode, iters):
        wf.set_preconditioner(mode)
        wf.set_transforms(dq0)                                   # every solve starts from the same transforms
        return wf.solve_rigid(d_src, d_dst, None, iters=iters, lam=LAM, lam_rot=LROT, reg_neighbours=KG, reg_lambda=LREG, rounds=1)

    res = {"nodes": int(len(pos)), "points": int(N), "k": 8, "kg": KG, "lambda": LAM, "lambda_rot": LROT, "lambda_reg": LREG}
    steps = {}
    for mode in (0, 1):
        ref, en = solve(mode, CAP)
        ref = ref.cpu().numpy().view(np.uint32)
        lo, hi = 0, CAP
        while lo < hi:
            mid = (lo + hi) // 2
            if np.array_equal(solve(mode, mid)[0].cpu().numpy().view(np.uint32), ref):
                hi = mid
            else:
                lo = mid + 1
        steps[mode] = lo
        res["steps_%d" % mode] = lo if lo < CAP else None
        res["energy_%d" % mode] = en.cpu().tolist()
    times = {(mode, it): [] for mode in (0, 1) for it in (LO, HI, "conv")}
    for rep in range(reps + 2):
        for mode in (0, 1):
            for it in (LO, HI, "conv"):
                ms, _ = sync_ms(lambda: solve(mode, steps[mode] if it == "conv" else it))
                if rep >= 2:
                    times[(mode, it)].append(ms)
    for mode in (0, 1):
        step_us = 1e3 * (med(times[(mode, HI)]) - med(times[(mode, LO)])) / (HI - LO)
        round_ms = med(times[(mode, LO)]) - LO * step_us / 1e3
        res["step_us_%d" % mode], res["round_ms_%d" % mode] = step_us, round_ms
        res["solve_ms_%d" % mode] = {str(it): med(times[(mode, it)]) for it in (LO, HI, "conv")}
        res["solve_raw_ms_%d" % mode] = {str(it): times[(mode, it)] for it in (LO, HI, "conv")}
        res["model_ms_%d" % mode] = steps[mode] * step_us / 1e3 + round_ms
    res["step_ratio"] = res["step_us_1"] / res["step_us_0"]
    res["round_extra_ms"] = res["round_ms_1"] - res["round_ms_0"]
    res["converged_ratio"] = res["solve_ms_1"]["conv"] / res["solve_ms_0"]["conv"]
    return res


res = {"library": os.path.relpath(capi.library_path(), REPO), "repeats": reps, "cap": CAP, "surface": [surface(M) for M in (2000, 8000)]}
line = json.dumps(res)
print(line)
if out:
    with open(out, "w") as f:
        f.write(line + "\n")
