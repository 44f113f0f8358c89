#!/usr/bin/env python3
"""Cost of growing the warp field (WarpField.extend, include/dfusion.h dfusion_warp_extend) at a bench config, against the full
rebuild that bench.py's frame_nodes_changed_ms measures (set_nodes + index + the frame).  Each repeat, on one handle in its steady
state: extend with ~NEW nodes (points 3 sigma off randomly chosen nodes, max_new = NEW), then the next frame (integrate + ray cast);
and the rebuild path: set_nodes of the (grown) set + ensure_index, then the same frame.  Wall times with a device synchronisation
around each part.  Prints one JSON line; --out FILE also writes it there.
Usage: tools/extend_probe.py [CONFIG] [REPEATS] [NEW] [--out FILE]"""
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, REPO)
from dynamicfusion_amd import Intr, TsdfVolume, WarpField, compute_dists, synth, upload_u16  # noqa: E402

out = None
if "--out" in sys.argv:
    i = sys.argv.index("--out"); out = sys.argv[i + 1]; del sys.argv[i:i + 2]
name = sys.argv[1] if len(sys.argv) > 1 else "512"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
new = int(sys.argv[3]) if len(sys.argv) > 3 else 50
cfg = synth.CONFIGS[name]; intr = Intr(*cfg.intr)
vol = TsdfVolume(cfg.dims); vol.setSize([cfg.size] * 3); vol.setTruncDist(cfg.trunc_dist); vol.setMaxWeight(cfg.max_weight); vol.setPose(cfg.volume_pose)
vol.setRaycastStepFactor(cfg.raycast_step_factor); vol.setGradientDeltaFactor(cfg.gradient_delta_factor); vol.clear()
pos, sigma = synth.make_nodes(cfg)
sigma = np.broadcast_to(np.asarray(sigma, np.float32), (len(pos),)).copy()
wf = WarpField(k=cfg.k); wf.init(pos, sigma=sigma, transforms=synth.node_transforms(cfg, 0))
dists = compute_dists(upload_u16(synth.depth_frame(cfg, 0)), intr)
cam = synth.camera_pose(cfg, 0)
pts = torch.empty((cfg.rows, cfg.cols, 4), dtype=torch.float32, device="cuda"); nrm = torch.empty_like(pts)
rng = np.random.default_rng(0)


def frame():
    vol.integrate_warped(dists, cam, intr, wf, sync=False)
    vol.raycast(cam, intr, pts, nrm)


def sync_ms(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


for _ in range(3):
    frame()
ext, ext_frame, reb, reb_frame, added = [], [], [], [], []
for _ in range(reps):
    if wf.M + new > 65535:
        break
    src = rng.integers(0, wf.M, 4 * new)
    d = rng.normal(size=(4 * new, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    keep_pos, _, keep_sig = (t.cpu().numpy() for t in wf._keep)
    cand = (keep_pos.reshape(-1, 3)[src] + 3.0 * keep_sig[src, None] * d).astype(np.float32)
    t, (n, _) = sync_ms(lambda: wf.extend(torch.from_numpy(cand).cuda(), float(np.median(keep_sig)), max_new=new))
    ext.append(t); added.append(n)
    wf.set_transforms(wf._keep[1])
    ext_frame.append(sync_ms(frame)[0])
    frame()
    t, _ = sync_ms(lambda: (wf.set_nodes(*wf._keep), wf.ensure_index(vol, cfg.k)))
    reb.append(t)
    reb_frame.append(sync_ms(frame)[0])
    frame()
med = lambda a: float(np.median(a)) if a else None  # noqa: E731
res = {"config": name, "nodes_start": int(len(pos)), "nodes_end": int(wf.M), "added_per_call": added,
       "extend_ms": med(ext), "extend_next_frame_ms": med(ext_frame), "extend_plus_frame_ms": med([a + b for a, b in zip(ext, ext_frame)]),
       "rebuild_ms": med(reb), "rebuild_next_frame_ms": med(reb_frame), "rebuild_plus_frame_ms": med([a + b for a, b in zip(reb, reb_frame)]),
       "raw": {"extend": ext, "extend_frame": ext_frame, "rebuild": reb, "rebuild_frame": reb_frame}}
line = json.dumps(res)
print(line)
if out:
    with open(out, "w") as f:
        f.write(line + "\n")
