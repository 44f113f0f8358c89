#!/usr/bin/env python3
"""Cost of the projective data association at the headline frame: 640 x 480, 307 200 points.
  call    dfusion_associate_projective timed by HIP events, medians of REPEATS after two warm-up calls, with the occlusion test on
          (fill + splat + resolve) and off (resolve alone).  Inputs: the live maps of a synthetic depth frame, the predicted points
          those of the frame two camera steps on (so that points leave the image, hit holes and fail the gates).
  frame   kinfu_headless ms / frame (its own figure: KinFu::operator(), frames 2.., wall clock) in mode `warped` and `warped-assoc`
          on this tree and, with --parent-host DIR (a directory holding the parent commit's dynamicfusion_amd/host/kinfu_headless and
          its libraries in the same layout), in mode `warped` there too: parent and tree alternate, SESSIONS times each, and which of
          the two goes first alternates from session to session.
--call-only stops after the first part (the workload of a kernel trace).  Writes one JSON line to --out (default
profiles/associate_probe.json).
Usage: tools/associate_probe.py [REPEATS] [--parent-host DIR] [--out FILE] [--sessions N] [--frames N] [--call-only]"""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, REPO)
DIST_THRES, ANGLE_DEG, MARGIN = 0.05, 30.0, 0.02


def opt(name, default=None):
    if name in sys.argv:
        i = sys.argv.index(name); v = sys.argv[i + 1]; del sys.argv[i:i + 2]
        return v
    return default


def time_call(reps):
    import torch
    from dynamicfusion_amd import Intr, frontend, synth, upload_u16
    cfg = synth.Config(256, 1.0, cols=640, rows=480, nodes=0, k=8)
    intr = Intr(*cfg.intr)
    maps = [frontend.computePointNormals(intr, upload_u16(synth.depth_frame(cfg, f))) for f in (0, 2)]
    live_p, live_n = maps[0]
    pts = maps[1][0][..., :3].reshape(-1, 3).contiguous()
    nrm = maps[1][1][..., :3].reshape(-1, 3).contiguous()
    mc = float(np.cos(np.deg2rad(ANGLE_DEG)))
    out = {"points": int(pts.shape[0])}
    for name, margin in (("occlusion_on", MARGIN), ("occlusion_off", -1.0)):
        t = []
        for rep in range(reps + 2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            res = frontend.associateProjective(intr, pts, nrm, live_p, live_n, DIST_THRES, mc, margin, return_counts=True)
            b.record()
            torch.cuda.synchronize()
            if rep >= 2:
                t.append(a.elapsed_time(b))
        out[name] = {"raw_ms": t, "median_ms": float(np.median(t)), "counts": res[1].cpu().tolist()}
    return out


def time_frames(app, mode, fin, cols, rows, frames, dims):
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([app, str(cols), str(rows), str(frames), str(dims), "1.0", fin, os.path.join(d, "out.bin"), mode],
                           capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.exit("%s %s failed (%d):\n%s%s" % (app, mode, r.returncode, r.stdout, r.stderr))
    return float(re.search(r"([0-9.]+) ms/frame", r.stdout).group(1))


def main():
    out = opt("--out", os.path.join(REPO, "profiles", "associate_probe.json"))
    parent = opt("--parent-host")
    sessions = int(opt("--sessions", "4"))
    frames = int(opt("--frames", "40"))
    call_only = "--call-only" in sys.argv
    if call_only:
        sys.argv.remove("--call-only")
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    from dynamicfusion_amd import build, synth
    build.build_host()
    res = {"repeats": reps, "sessions": sessions, "frames": frames, "dist_thres": DIST_THRES, "angle_deg": ANGLE_DEG, "margin": MARGIN,
           "call": time_call(reps)}
    if call_only:
        print(json.dumps(res["call"]))
        with open(out, "w") as f:
            f.write(json.dumps(res) + "\n")
        return
    cfg = synth.Config(256, 1.0, cols=640, rows=480, nodes=0, k=8)
    with tempfile.TemporaryDirectory() as d:
        fin = os.path.join(d, "in.bin")
        with open(fin, "wb") as f:
            f.write(np.asarray(cfg.intr, np.float32).tobytes())
            for i in range(frames):
                f.write(synth.depth_frame(cfg, 2 * i).tobytes())
        rows = {"tree_warped": [], "tree_warped_assoc": [], "parent_warped": []}
        for s in range(sessions):
            order = ["parent_warped", "tree_warped"] if s % 2 == 0 else ["tree_warped", "parent_warped"]
            for which in order:
                if which == "parent_warped" and not parent:
                    continue
                app = os.path.join(parent, "dynamicfusion_amd", "host", "kinfu_headless") if which == "parent_warped" else build.HOST_KINFU_APP
                rows[which].append(time_frames(app, "warped", fin, cfg.cols, cfg.rows, frames, cfg.dims[0]))
            rows["tree_warped_assoc"].append(time_frames(build.HOST_KINFU_APP, "warped-assoc", fin, cfg.cols, cfg.rows, frames, cfg.dims[0]))
    med = lambda a: float(np.median(a)) if a else None  # noqa: E731
    res["frame_ms"] = rows
    res["summary"] = {"call_ms_occlusion_on": res["call"]["occlusion_on"]["median_ms"], "call_ms_occlusion_off": res["call"]["occlusion_off"]["median_ms"],
                      "frame_ms_tree_warped": med(rows["tree_warped"]), "frame_ms_tree_warped_assoc": med(rows["tree_warped_assoc"]),
                      "frame_ms_parent_warped": med(rows["parent_warped"])}
    if parent:
        p = rows["parent_warped"]
        res["summary"]["parent_spread_ms"] = [min(p), max(p)]
        res["summary"]["unflagged_within_parent_spread"] = bool(min(p) <= med(rows["tree_warped"]) <= max(p))
    print(json.dumps(res["summary"]))
    with open(out, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
