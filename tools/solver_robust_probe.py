#!/usr/bin/env python3
"""Cost of the robust warp solve at the headline size: 2000 nodes, k = 8, kg = 4, the 307 200-point frame.
Wall times around a device synchronise, medians of REPEATS after two warm-up rounds:
  the 40-step regularised solve (WarpField.solve) on this tree and, with --parent-lib FILE, on another build of the library;
  the robust solve (tukey_c = 0.05, huber_delta = 0.01) at 1, 2 and 3 rounds of 40 steps;
  the quadratic rounds through the same entry point (both thresholds 0) at 2 and 3 rounds: a round's own work without the weights;
  the robust solve with 0 steps at 2 and 3 rounds: what a round costs beyond its conjugate-gradient steps (e0, Tukey, list scale, edge
  values, Huber, right-hand side, write-back).
Every measurement runs in a child process of its own (one library per process); this tree and the parent library alternate, SESSIONS
times each; every row the parent library has is timed there too, and the summary sets the two side by side
(rows_against_parent).  Writes one JSON line to --out (default profiles/solver_robust_probe.json).
Usage: tools/solver_robust_probe.py [REPEATS] [--parent-lib FILE] [--out FILE] [--sessions N]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, REPO)
KG, LREG, ITERS, TUKEY_C, HUBER_DELTA = 4, 1.0, 40, 0.05, 0.01


def opt(name, default=None):
    if name in sys.argv:
        i = sys.argv.index(name); v = sys.argv[i + 1]; del sys.argv[i:i + 2]
        return v
    return default


def child(lib, reps):
    import torch
    from dynamicfusion_amd import WarpField, capi, synth
    if lib:
        capi._lib = capi.load(lib, strict=False)
    have = not getattr(capi.lib().dfusion_warp_solve_robust, "missing", False)
    cfg = synth.CONFIGS["512"]
    pos, sigma = synth.make_nodes(cfg)
    rng = np.random.default_rng(5); N = cfg.cols * cfg.rows
    src = (pos[rng.integers(0, len(pos), N)] + rng.normal(0, 0.03, (N, 3))).astype(np.float32)
    dst = (src + 0.01 * np.sin(5 * src)).astype(np.float32)
    dst[::10] += np.float32(0.25)                            # every tenth pair a gross outlier
    d_src, d_dst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    wf = WarpField(k=8); wf.init(pos, sigma=sigma)
    dq0 = wf._keep[1].clone()

    def ms(fn):
        wf.set_transforms(dq0)                               # every solve starts from the same transforms
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def robust(rounds, iters, c, delta):
        return lambda: wf.solve_robust(d_src, d_dst, iters=iters, reg_neighbours=KG, reg_lambda=LREG, rounds=rounds, tukey_c=c,
                                       huber_delta=delta)
    runs = {"solve_40": lambda: wf.solve(d_src, d_dst, iters=ITERS, reg_neighbours=KG, reg_lambda=LREG)}
    if have:
        for r in (1, 2, 3):
            runs["robust_%d" % r] = robust(r, ITERS, TUKEY_C, HUBER_DELTA)
        for r in (2, 3):
            runs["quadratic_rounds_%d" % r] = robust(r, ITERS, 0.0, 0.0)
            runs["robust_0_steps_%d" % r] = robust(r, 0, TUKEY_C, HUBER_DELTA)
    t = {name: [] for name in runs}
    for rep in range(reps + 2):
        for name, fn in runs.items():
            v = ms(fn)
            if rep >= 2:
                t[name].append(v)
    print(json.dumps({"library": lib or capi.library_path(), "nodes": int(len(pos)), "points": int(N), "raw_ms": t}))


def main():
    out = opt("--out", os.path.join(REPO, "profiles", "solver_robust_probe.json"))
    parent = opt("--parent-lib")
    sessions = int(opt("--sessions", "2"))
    if "--child" in sys.argv:
        sys.argv.remove("--child")
        return child(opt("--lib"), int(sys.argv[1]))
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    med = lambda a: float(np.median(a))  # noqa: E731
    res = {"repeats": reps, "sessions": sessions, "k": 8, "kg": KG, "iters": ITERS, "tukey_c": TUKEY_C, "huber_delta": HUBER_DELTA,
           "tree": [], "parent": []}
    for _ in range(sessions):
        for which, lib in (("parent", parent), ("tree", None)):
            if which == "parent" and not parent:
                continue
            cmd = [sys.executable, os.path.abspath(__file__), "--child", str(reps)] + (["--lib", lib] if lib else [])
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit("%s child failed (%d):\n%s%s" % (which, r.returncode, r.stdout, r.stderr))
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            rec["median_ms"] = {k: med(v) for k, v in rec["raw_ms"].items()}
            rec["library"] = "this tree" if which == "tree" else "parent"
            res["nodes"], res["points"] = rec["nodes"], rec["points"]
            res[which].append(rec)
    m = res["tree"][-1]["median_ms"]
    solves = [s["median_ms"]["solve_40"] for s in res["tree"] + res["parent"]]
    base = med([s["median_ms"]["solve_40"] for s in (res["parent"] or res["tree"])])
    res["summary"] = {
        "solve_40_ms_tree": [s["median_ms"]["solve_40"] for s in res["tree"]],
        "solve_40_ms_parent": [s["median_ms"]["solve_40"] for s in res["parent"]],
        "solve_40_spread_ms": max(solves) - min(solves),
        "robust_ms": {str(r): m["robust_%d" % r] for r in (1, 2, 3)},
        "round_ms_robust": m["robust_3"] - m["robust_2"],
        "round_ms_quadratic": m["quadratic_rounds_3"] - m["quadratic_rounds_2"],
        "round_beyond_cg_ms": m["robust_0_steps_3"] - m["robust_0_steps_2"],
        "round_beyond_cg_over_parent_solve": (m["robust_0_steps_3"] - m["robust_0_steps_2"]) / base,
    }
    if parent:
        # every row on both libraries: the session medians, and whether this tree's lies within the parent's own session-to-session
        # spread, widened by that spread once more on either side (two sessions are a small sample of it)
        rows = {}
        for name in res["parent"][0]["median_ms"]:
            p = [s["median_ms"][name] for s in res["parent"]]
            t = [s["median_ms"][name] for s in res["tree"]]
            spread = max(p) - min(p)
            rows[name] = {"parent_ms": p, "tree_ms": t, "tree_median_ms": med(t), "allowed_ms": [min(p) - spread, max(p) + spread],
                          "within": bool(min(p) - spread <= med(t) <= max(p) + spread)}
        res["summary"]["rows_against_parent"] = rows
    line = json.dumps(res)
    print(json.dumps(res["summary"]))
    with open(out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
