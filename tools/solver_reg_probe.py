#!/usr/bin/env python3
"""Cost of the regularisation term in the warp solve at the headline size: 2000 nodes, k = 8, the 307 200-point frame.
Per conjugate-gradient step: (time of a solve with 40 steps - time of one with 10) / 30, for the data-only solve (energy_data) and for
the regularised one (solve, kg = 4, lambda_reg = 1); and the one-off graph build (node_graph on a handle that has just been given its
nodes).  Wall times around a device synchronise, medians of REPEATS after two warm-up rounds, the two solves alternating.
--lib FILE measures another build of the library (an older one has only the data-only solve).  Prints one JSON line.
Usage: tools/solver_reg_probe.py [REPEATS] [--lib FILE] [--out FILE]"""
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, REPO)
from dynamicfusion_amd import WarpField, capi, synth  # noqa: E402

out = lib = None
if "--out" in sys.argv:
    i = sys.argv.index("--out"); out = sys.argv[i + 1]; del sys.argv[i:i + 2]
if "--lib" in sys.argv:
    i = sys.argv.index("--lib"); lib = sys.argv[i + 1]; del sys.argv[i:i + 2]
    capi._lib = capi.load(lib, strict=False)
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
KG, LREG, LO, HI = 4, 1.0, 10, 40
have_reg = not getattr(capi.lib().dfusion_warp_solve, "missing", False)

cfg = synth.CONFIGS["512"]
pos, sigma = synth.make_nodes(cfg)
rng = np.random.default_rng(5); N = cfg.cols * cfg.rows
src = (pos[rng.integers(0, len(pos), N)] + rng.normal(0, 0.03, (N, 3))).astype(np.float32)
dst = (src + 0.01 * np.sin(5 * src)).astype(np.float32)
d_src, d_dst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
wf = WarpField(k=8); wf.init(pos, sigma=sigma)
dq0 = wf._keep[1].clone()


def sync_ms(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def solve_ms(reg, iters):
    wf.set_transforms(dq0)                                   # every solve starts from the same transforms
    if reg:
        return sync_ms(lambda: wf.solve(d_src, d_dst, iters=iters, reg_neighbours=KG, reg_lambda=LREG))
    return sync_ms(lambda: wf.energy_data(d_src, d_dst, iters=iters))


kinds = [False, True] if have_reg else [False]
t = {(reg, it): [] for reg in kinds for it in (LO, HI)}
energy = {}
for rep in range(reps + 2):
    for reg in kinds:
        for it in (LO, HI):
            ms, (_, en) = solve_ms(reg, it)
            if rep >= 2:
                t[(reg, it)].append(ms)
            energy["%s_%d" % ("reg" if reg else "data", it)] = [float(x) for x in en.cpu().numpy()]
graph = []
if have_reg:
    for rep in range(reps + 2):
        wf.set_nodes(*wf._keep)                              # drops the graph
        ms, _ = sync_ms(lambda: wf.node_graph(KG))
        if rep >= 2:
            graph.append(ms)
med = lambda a: float(np.median(a))  # noqa: E731
res = {"library": lib or capi.library_path(), "nodes": int(len(pos)), "points": int(N), "k": 8, "kg": KG, "repeats": reps,
       "data_step_us": 1e3 * (med(t[(False, HI)]) - med(t[(False, LO)])) / (HI - LO),
       "data_solve_ms": {str(it): med(t[(False, it)]) for it in (LO, HI)}, "energy": energy}
if have_reg:
    res.update(reg_step_us=1e3 * (med(t[(True, HI)]) - med(t[(True, LO)])) / (HI - LO),
               reg_solve_ms={str(it): med(t[(True, it)]) for it in (LO, HI)}, graph_build_ms=med(graph), graph_build_raw_ms=graph)
res["raw_ms"] = {"%s_%d" % ("reg" if reg else "data", it): v for (reg, it), v in t.items()}
line = json.dumps(res)
print(line)
if out:
    with open(out, "w") as f:
        f.write(line + "\n")
