#!/usr/bin/env python3
"""Times the colour volume on the headline configuration (512^3, 640 x 480, 2000 nodes, k = 8, the volume primed with a few warped frames
on the bench's sweep poses, as tools/mesh_probe.py primes it): ColorVolume.integrate through the warp field, and its parts; fetchColors
on the mesh's vertices; and, as yardsticks in the same process, back to back, integrate_warped and fetchCloud's kernel.  Medians of 5,
HIP events.

The parts of integrate are separated by what a call can be told to leave out, not by a profiler:
  select  = a rigid call with band = 2^-20 (count, scan, totals; the list and fuse launches find nothing to do)
  fuse    = a rigid call with the real band, minus select (the list kernel's writes and the fuse kernel)
  warp    = the call through the warp field, minus the rigid call (the NaN fill and dfusion_warp_points over the capacity)
and the call through the warp field is repeated with the capacity cut to the band's size, which shows what the unused capacity costs.
usage: color_probe.py [config=512] [frames=5] [out.json=profiles/color_probe.json]"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from dynamicfusion_amd import ColorVolume, Intr, TsdfVolume, WarpField, capi, compute_dists, synth, upload_u16  # noqa: E402


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
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(REPO, "profiles", "color_probe.json")
    cfg = synth.CONFIGS[name]
    intr = Intr(*cfg.intr)
    vol = TsdfVolume(cfg.dims)
    vol.setSize([cfg.size] * 3); vol.setTruncDist(cfg.trunc_dist); vol.setMaxWeight(cfg.max_weight); vol.setPose(cfg.volume_pose)
    pos, sigma = synth.make_nodes(cfg)
    wf = WarpField(k=cfg.k)
    wf.init(pos, sigma=sigma, transforms=synth.node_transforms(cfg, 0))
    for f in range(frames):
        wf.set_transforms(torch.from_numpy(synth.node_transforms(cfg, f)).cuda())
        dists = compute_dists(upload_u16(synth.depth_frame(cfg, f)), intr)
        vol.integrate_warped(dists, synth.camera_pose(cfg, f), intr, wf)
    torch.cuda.synchronize()
    pose = synth.camera_pose(cfg, frames - 1)
    # an image whose content does not matter to the clock: a colour ramp over the pixels
    yy, xx = np.meshgrid(np.arange(cfg.rows), np.arange(cfg.cols), indexing="ij")
    image = torch.from_numpy(np.stack([xx & 255, yy & 255, (xx + yy) & 255, np.full_like(xx, 255)], -1).astype(np.uint8)).cuda()
    cv = ColorVolume(vol)
    cap = cv.default_capacity()
    counts = cv.integrate(image, dists, pose, intr, warp_field=wf, return_counts=True)
    n_selected, n_fused = (int(c) for c in counts.tolist())
    counts_r = cv.integrate(image, dists, pose, intr, return_counts=True)
    L, st = capi.lib(), torch.cuda.current_stream().cuda_stream
    aff = capi.floats(synth.aff12(vol.getPose()))
    cbuf = torch.empty((1 << 22, 4), dtype=torch.float32, device="cuda")
    ccnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    cloud = lambda: capi.check(L.dfusion_extract_cloud(vol.c_volume(), None, aff, cbuf.data_ptr(), cbuf.shape[0], ccnt.data_ptr(), st))
    sweep = lambda: vol.integrate_warped(dists, pose, intr, wf, sync=False)
    full = lambda: cv.integrate(image, dists, pose, intr, warp_field=wf)
    rigid = lambda: cv.integrate(image, dists, pose, intr)
    select = lambda: cv.integrate(image, dists, pose, intr, band=2.0 ** -20)
    tight_cap = (n_selected + 5119) // 5120 * 5120                      # the band's size, known after the first call
    tight = lambda: cv.integrate(image, dists, pose, intr, warp_field=wf, capacity=tight_cap)
    res = {"config": cfg.name, "device": torch.cuda.get_device_name(0), "frames": frames, "nodes": int(len(pos)), "k": cfg.k,
           "capacity": cap, "selected": n_selected, "fused_warped": n_fused, "fused_rigid": int(counts_r[1].item()), "samples_ms": {}}
    # back to back, the yardsticks between the colour calls
    for key, fn in (("extract_cloud_ms", cloud), ("color_select_ms", select), ("integrate_warped_ms", sweep), ("color_integrate_warped_ms", full),
                    ("color_integrate_rigid_ms", rigid), ("color_integrate_warped_tight_capacity_ms", tight), ("extract_cloud_again_ms", cloud)):
        res[key], res["samples_ms"][key] = median_ms(fn)
    vertices, triangles = vol.fetchMesh()
    res["vertices"] = int(vertices.shape[0])
    res["fetch_colors_ms"], res["samples_ms"]["fetch_colors_ms"] = median_ms(lambda: cv.fetchColors(vertices))
    colors = cv.fetchColors(vertices)
    res["vertices_with_colour"] = int((colors[:, 3] == 255).sum().item())
    res["color_fuse_ms"] = res["color_integrate_rigid_ms"] - res["color_select_ms"]
    res["color_warp_ms"] = res["color_integrate_warped_ms"] - res["color_integrate_rigid_ms"]
    res["tight_capacity"] = tight_cap
    res["select_over_cloud"] = res["color_select_ms"] / res["extract_cloud_ms"]
    res["select_scan_GBps"] = 4 * float(np.prod(cfg.dims)) / (res["color_select_ms"] * 1e-3) / 1e9
    res["color_over_integrate_warped"] = res["color_integrate_warped_ms"] / res["integrate_warped_ms"]
    res["how"] = ("medians of 5 after 2 warm-up calls, HIP events around one call each, one process; select / fuse / warp are differences of "
                  "whole calls (see the tool's docstring), not kernel times")
    print(json.dumps(res))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
