#!/usr/bin/env python3
"""Cost and effect of the hierarchical node graph against the flat one, at 2000 and 8000 nodes, kg = 4:
  * the one-off graph build (node_graph on a handle that has just been given its nodes), hierarchical against flat, on surface nodes
    (synth.make_nodes of the headline scene), the hierarchy at 3 levels, radius = dg_w, beta 4;
  * a regularised conjugate-gradient step over each graph, on those nodes with the 307 200-point frame: (time of a solve with 40 steps -
    time of one with 10) / 30, and the largest in-degree of each graph (one thread per node walks its incoming edges);
  * on a chain of that many nodes 25 mm apart (dg_w 0.025, 1500 points over the first 0.5 m moved 20 mm along it, k = 4, lambda_reg = 100;
    hierarchy: 8 levels, radius 0.05, beta 4) the steps each graph needs: the first entry n of a ladder (x 1.5 a rung) at which delta_x
    over the rim nodes -- those past the points -- differs from the rung before by less than 1 % of its largest value.
Wall times around a device synchronise, medians of REPEATS after two warm-up rounds, the two graphs alternating.  Prints one JSON line.
Usage: tools/solver_hier_probe.py [REPEATS] [--out FILE]"""
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
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
KG, LREG, LO, HI = 4, 1.0, 10, 40
LADDER = [10]
while LADDER[-1] < 20000:
    LADDER.append(int(LADDER[-1] * 1.5 + 0.5))
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
    setting = (3, float(sigma[0]), 4.0)
    wf = WarpField(k=8); wf.init(pos, sigma=sigma)
    dq0 = wf._keep[1].clone()
    d_src, d_dst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    res = {"nodes": int(M), "points": int(N), "k": 8, "kg": KG, "hierarchy": setting}
    build = {"flat": [], "hier": []}
    step = {(g, it): [] for g in ("flat", "hier") for it in (LO, HI)}
    for rep in range(reps + 2):
        for g in ("flat", "hier"):
            wf.set_nodes(*wf._keep)                              # drops the graph
            wf.set_graph_hierarchy(*(setting if g == "hier" else (0, 1.0)))
            ms, (nbr, _) = sync_ms(lambda: wf.node_graph(KG))
            if rep >= 2:
                build[g].append(ms)
            if rep == 0:
                res[g + "_max_in_degree"] = int(torch.bincount(nbr.reshape(-1).long(), minlength=M).max().item())
                if g == "hier":
                    _, sizes, eff = wf.graph_levels(KG)
                    res["sizes"], res["effective"] = sizes.cpu().tolist(), int(eff.item())
            for it in (LO, HI):
                wf.set_transforms(dq0)                           # every solve starts from the same transforms
                ms, _ = sync_ms(lambda: wf.solve(d_src, d_dst, iters=it, reg_neighbours=KG, reg_lambda=LREG))
                if rep >= 2:
                    step[(g, it)].append(ms)
    for g in ("flat", "hier"):
        res[g + "_build_ms"] = med(build[g]); res[g + "_build_raw_ms"] = build[g]
        res[g + "_step_us"] = 1e3 * (med(step[(g, HI)]) - med(step[(g, LO)])) / (HI - LO)
        res[g + "_solve_ms"] = {str(it): med(step[(g, it)]) for it in (LO, HI)}
    return res


def chain(M):
    pos = np.zeros((M, 3), np.float32); pos[:, 0] = np.arange(M, dtype=np.float32) * np.float32(0.025)
    rng = np.random.default_rng(5)
    src = np.stack([rng.uniform(0, 0.5, 1500), rng.uniform(-0.01, 0.01, 1500), rng.uniform(-0.01, 0.01, 1500)], 1).astype(np.float32)
    dst = src.copy(); dst[:, 0] += np.float32(0.02)
    d_src, d_dst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    wf = WarpField(k=4); wf.init(pos, sigma=0.025)
    dq0 = wf._keep[1].clone()
    rim = slice(24, M)                                           # nodes 0.1 m and more past the last point
    res = {"nodes": int(M), "hierarchy": (8, 0.05, 4.0)}
    for g in ("flat", "hier"):
        wf.set_graph_hierarchy(*((8, 0.05, 4.0) if g == "hier" else (0, 1.0)))
        if g == "hier":
            _, sizes, eff = wf.graph_levels(KG)
            res["sizes"], res["effective"] = sizes.cpu().tolist(), int(eff.item())
        before, found = None, None
        for n in LADDER:
            wf.set_transforms(dq0)
            dq, _ = wf.solve(d_src, d_dst, iters=n, reg_neighbours=KG, reg_lambda=100.0)
            d = dq.cpu().numpy().astype(np.float64)
            x = 2.0 * (d[:, 5] * d[:, 0] - d[:, 4] * d[:, 1])[rim]   # translation x of (rotation, dual) at the identity rotation
            if before is not None and np.abs(x).max() > 0 and np.abs(x - before).max() < 0.01 * np.abs(x).max():
                found = n
                break
            before = x
        res[g + "_steps"] = found
        res[g + "_delta_x_first_last"] = [float(x[0]), float(x[-1])]
    return res


res = {"library": os.path.relpath(capi.library_path(), REPO), "repeats": reps, "surface": [surface(M) for M in (2000, 8000)], "chain": [chain(M) for M in (2000, 8000)]}
line = json.dumps(res)
print(line)
if out:
    with open(out, "w") as f:
        f.write(line + "\n")
