#!/usr/bin/env python3
"""Cost of the warp solve with node rotations at the headline size: 2000 nodes, k = 8, kg = 4, the 307 200-point frame.
Wall times around a device synchronise, medians of REPEATS after two warm-up rounds:
  the point-to-plane solve (WarpField.solve_plane, one round, quadratic penalties) at 40 and at 0 steps on this tree and, with
  --parent-lib FILE, on another build of the library;
  the rigid solve (WarpField.solve_rigid, with the normals, one round, quadratic penalties) at 40 and at 0 steps on this tree.
A conjugate-gradient step is (40 steps - 0 steps) / 40; the 0-step call is what a round costs around its steps (for the rigid solve: two
warps of the points, the k-NN, the lists, the write-back).  Every measurement runs in a child process of its own (one library per
process); this tree and the parent library alternate, SESSIONS times each.  The summary says whether this tree's `solve_plane` and
`solve_rigid` lie within the parent's own range across its processes, and within that range widened by its width on either side, and on which side it
lies when outside; it gives the rigid step as a ratio to the parent's plane step.
Writes one JSON line to --out (default profiles/solver_rigid_probe.json).
Usage: tools/solver_rigid_probe.py [REPEATS] [--parent-lib FILE] [--out FILE] [--sessions N]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, REPO)
KG, LREG, ITERS = 4, 1.0, 40


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
    have = not getattr(capi.lib().dfusion_warp_solve_rigid, "missing", False)
    cfg = synth.CONFIGS["512"]
    pos, sigma = synth.make_nodes(cfg)
    rng = np.random.default_rng(5); N = cfg.cols * cfg.rows
    src = (pos[rng.integers(0, len(pos), N)] + rng.normal(0, 0.03, (N, 3))).astype(np.float32)
    dst = (src + 0.01 * np.sin(5 * src)).astype(np.float32)
    nrm = rng.normal(0, 1, (N, 3)); nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    d_src, d_dst, d_nrm = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda(), torch.from_numpy(nrm).cuda()
    wf = WarpField(k=8); wf.init(pos, sigma=sigma)
    dq0 = wf._keep[1].clone()

    def ms(fn):
        wf.set_transforms(dq0)                               # every solve starts from the same transforms
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    runs = {}
    for iters in (ITERS, 0):
        runs["plane_%d" % iters] = lambda iters=iters: wf.solve_plane(d_src, d_dst, d_nrm, iters=iters, reg_neighbours=KG, reg_lambda=LREG)
        if have:
            runs["rigid_%d" % iters] = lambda iters=iters: wf.solve_rigid(d_src, d_dst, d_nrm, iters=iters, reg_neighbours=KG, reg_lambda=LREG)
    t = {name: [] for name in runs}
    for rep in range(reps + 2):
        for name, fn in runs.items():
            v = ms(fn)
            if rep >= 2:
                t[name].append(v)
    print(json.dumps({"library": lib or capi.library_path(), "nodes": int(len(pos)), "points": int(N), "raw_ms": t}))


def summarise(res, parent):
    """The figures of the run side by side, and for `solve_plane` and `solve_rigid` where this tree's median lies against the parent's processes: inside
    their own range [min, max] ("within_parent_range"), inside that range widened by its width on either side (a few sessions are a
    small sample of it; "within_widened_range"), and on which side when outside."""
    med = lambda a: float(np.median(a))  # noqa: E731

    def col(recs, table, name):
        return [s[table][name] for s in recs]
    summary = {
        "plane_40_ms_tree": col(res["tree"], "median_ms", "plane_40"), "plane_40_ms_parent": col(res["parent"], "median_ms", "plane_40"),
        "rigid_40_ms_tree": col(res["tree"], "median_ms", "rigid_40"), "rigid_0_ms_tree": col(res["tree"], "median_ms", "rigid_0"),
        "plane_0_ms_tree": col(res["tree"], "median_ms", "plane_0"),
        "plane_step_us_tree": col(res["tree"], "step_us", "plane"), "plane_step_us_parent": col(res["parent"], "step_us", "plane"),
        "rigid_step_us_tree": col(res["tree"], "step_us", "rigid"),
    }
    if parent:
        for name, table, key in (("plane_40_ms", "median_ms", "plane_40"), ("plane_step_us", "step_us", "plane"),
                                 ("rigid_40_ms", "median_ms", "rigid_40"), ("rigid_step_us", "step_us", "rigid")):
            p, t = col(res["parent"], table, key), med(col(res["tree"], table, key))
            spread = max(p) - min(p)
            summary[name + "_against_parent"] = {
                "parent_range": [min(p), max(p)], "tree_median": t, "within_parent_range": bool(min(p) <= t <= max(p)),
                "widened_range": [min(p) - spread, max(p) + spread], "within_widened_range": bool(min(p) - spread <= t <= max(p) + spread),
                "side": "inside" if min(p) <= t <= max(p) else ("faster" if t < min(p) else "slower")}
        summary["rigid_step_over_parent_plane_step"] = med(summary["rigid_step_us_tree"]) / med(summary["plane_step_us_parent"])
    return summary


def main():
    out = opt("--out", os.path.join(REPO, "profiles", "solver_rigid_probe.json"))
    parent = opt("--parent-lib")
    sessions = int(opt("--sessions", "2"))
    if "--child" in sys.argv:
        sys.argv.remove("--child")
        return child(opt("--lib"), int(sys.argv[1]))
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    med = lambda a: float(np.median(a))  # noqa: E731
    res = {"repeats": reps, "sessions": sessions, "k": 8, "kg": KG, "iters": ITERS, "tree": [], "parent": []}
    for _ in range(sessions):
        for which, lib in (("parent", parent), ("tree", None)):
            if which == "parent" and not parent:
                continue
            cmd = [sys.executable, os.path.abspath(__file__), "--child", str(reps)] + (["--lib", lib] if lib else [])
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit("%s child failed (%d):\n%s%s" % (which, r.returncode, r.stdout, r.stderr))
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            m = rec["median_ms"] = {k: med(v) for k, v in rec["raw_ms"].items()}
            rec["step_us"] = {name: (m[name + "_%d" % ITERS] - m[name + "_0"]) / ITERS * 1e3 for name in ("plane", "rigid") if name + "_0" in m}
            rec["library"] = "this tree" if which == "tree" else "parent"
            res["nodes"], res["points"] = rec["nodes"], rec["points"]
            res[which].append(rec)

    res["summary"] = summary = summarise(res, bool(parent))
    print(json.dumps(summary))
    with open(out, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
