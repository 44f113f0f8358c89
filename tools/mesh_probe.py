#!/usr/bin/env python3
"""Times dfusion_extract_mesh on the headline volume (512^3 after a few warped frames, as bench.py primes it) beside fetchCloud's
kernel in the same process: medians of 5, HIP events.  usage: mesh_probe.py [config=512] [frames=5] [out.json=profiles/mesh_probe.json]"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from dynamicfusion_amd import Intr, TsdfVolume, WarpField, capi, compute_dists, synth, upload_u16  # noqa: E402


def median_ms(fn, n=5, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), out


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "512"
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(REPO, "profiles", "mesh_probe.json")
    cfg = synth.CONFIGS[name]
    intr = Intr(*cfg.intr)
    vol = TsdfVolume(cfg.dims)
    vol.setSize([cfg.size] * 3); vol.setTruncDist(cfg.trunc_dist); vol.setMaxWeight(cfg.max_weight); vol.setPose(cfg.volume_pose)
    pos, sigma = synth.make_nodes(cfg)
    wf = WarpField(k=cfg.k)
    wf.init(pos, sigma=sigma, transforms=synth.node_transforms(cfg, 0))
    for f in range(frames):
        wf.set_transforms(torch.from_numpy(synth.node_transforms(cfg, f)).cuda())
        vol.integrate_warped(compute_dists(upload_u16(synth.depth_frame(cfg, f)), intr), synth.camera_pose(cfg, f), intr, wf)
    torch.cuda.synchronize()
    L, st = capi.lib(), torch.cuda.current_stream().cuda_stream
    aff = capi.floats(synth.aff12(vol.getPose()))
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    count_only = lambda: capi.check(L.dfusion_extract_mesh(vol.c_volume(), None, aff, None, 0, None, 0, counts.data_ptr(), st))
    count_only()
    nv, nt = (int(c) for c in counts.tolist())
    vb = torch.empty((max(nv, 1), 4), dtype=torch.float32, device="cuda")
    tb = torch.empty((max(nt, 1), 3), dtype=torch.int32, device="cuda")
    full = lambda: capi.check(L.dfusion_extract_mesh(vol.c_volume(), None, aff, vb.data_ptr(), nv, tb.data_ptr(), nt, counts.data_ptr(), st))
    cbuf = torch.empty((1 << 22, 4), dtype=torch.float32, device="cuda")
    ccnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    cloud = lambda: capi.check(L.dfusion_extract_cloud(vol.c_volume(), None, aff, cbuf.data_ptr(), cbuf.shape[0], ccnt.data_ptr(), st))
    ms_cloud, all_cloud = median_ms(cloud)
    ms_count, all_count = median_ms(count_only)
    ms_full, all_full = median_ms(full)
    ccnt.zero_(); cloud()
    nvox = float(np.prod(cfg.dims))
    res = {"config": cfg.name, "device": torch.cuda.get_device_name(0), "frames": frames, "vertices": nv, "triangles": nt, "cloud_points": int(ccnt.item()),
           "extract_cloud_ms": ms_cloud, "mesh_count_only_ms": ms_count, "mesh_full_ms": ms_full,
           "count_only_over_cloud": ms_count / ms_cloud, "full_over_cloud": ms_full / ms_cloud,
           "count_only_scan_GBps": 4 * nvox / (ms_count * 1e-3) / 1e9, "samples_ms": {"cloud": all_cloud, "count_only": all_count, "full": all_full},
           "how": "medians of 5 after 2 warm-up calls, HIP events around one call each, one process"}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
