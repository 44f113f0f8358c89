#!/usr/bin/env python3
"""Times the mesh rasteriser on the headline configuration (512^3, 640 x 480, 2000 nodes, k = 8, the volume primed with a few warped
frames on the bench's sweep poses, as tools/mesh_probe.py primes it): frontend.renderMesh alone on the warped mesh with every output, its
points-only form, and the whole frontend.renderLiveModel (fetchMesh + fetchNormals, fetchColors, warp, render); beside them, as
yardsticks in the same process, the ray-cast of the canonical volume from the same pose and fetchMesh.  Medians of 5 after two warm-up
calls, HIP events.  The three launches of a render are timed one by one under rocprofv3 --kernel-trace --stats, not here.
usage: render_probe.py [config=512] [frames=5] [out.json=profiles/render_probe.json]"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from dynamicfusion_amd import ColorVolume, Intr, TsdfVolume, WarpField, compute_dists, frontend, synth, upload_u16  # noqa: E402


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
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(REPO, "profiles", "render_probe.json")
    cfg = synth.CONFIGS[name]
    intr = Intr(*cfg.intr)
    vol = TsdfVolume(cfg.dims)
    vol.setSize([cfg.size] * 3); vol.setTruncDist(cfg.trunc_dist); vol.setMaxWeight(cfg.max_weight); vol.setPose(cfg.volume_pose)
    vol.setRaycastStepFactor(cfg.raycast_step_factor); vol.setGradientDeltaFactor(cfg.gradient_delta_factor)
    pos, sigma = synth.make_nodes(cfg)
    wf = WarpField(k=cfg.k)
    wf.init(pos, sigma=sigma, transforms=synth.node_transforms(cfg, 0))
    cv = ColorVolume(vol)
    yy, xx = np.meshgrid(np.arange(cfg.rows), np.arange(cfg.cols), indexing="ij")
    image = torch.from_numpy(np.stack([xx & 255, yy & 255, (xx + yy) & 255, np.full_like(xx, 255)], -1).astype(np.uint8)).cuda()
    for f in range(frames):
        wf.set_transforms(torch.from_numpy(synth.node_transforms(cfg, f)).cuda())
        dists = compute_dists(upload_u16(synth.depth_frame(cfg, f)), intr)
        vol.integrate_warped(dists, synth.camera_pose(cfg, f), intr, wf)
        cv.integrate(image, dists, synth.camera_pose(cfg, f), intr, warp_field=wf)
    torch.cuda.synchronize()
    pose = synth.camera_pose(cfg, frames - 1)
    world2cam = np.linalg.inv(pose.astype(np.float64)).astype(np.float32)

    vertices, triangles, normals = vol.fetchMesh(with_normals=True)
    colors = cv.fetchColors(vertices)
    p3, n3 = vertices[:, :3].contiguous(), normals[:, :3].contiguous()
    wf.warp(p3, n3)
    warped, wnormals = torch.zeros_like(vertices), torch.zeros_like(normals)
    warped[:, :3] = p3; wnormals[:, :3] = n3
    out = frontend.renderMesh(intr, warped, triangles, cfg.cols, cfg.rows, world2cam=world2cam, normals=wnormals, attr=vertices, colors=colors,
                              return_counts=True)
    counts = [int(c) for c in out[4].tolist()]
    rp = torch.empty((cfg.rows, cfg.cols, 4), dtype=torch.float32, device="cuda")
    rn = torch.empty_like(rp)
    vol.raycast(pose, intr, rp, rn)
    torch.cuda.synchronize()
    cast = ~torch.isnan(rp[..., 0])
    hit = ~torch.isnan(out[0][..., 0])

    render_all = lambda: frontend.renderMesh(intr, warped, triangles, cfg.cols, cfg.rows, world2cam=world2cam, normals=wnormals, attr=vertices,
                                             colors=colors)
    render_points = lambda: frontend.renderMesh(intr, warped, triangles, cfg.cols, cfg.rows, world2cam=world2cam)
    live = lambda: frontend.renderLiveModel(vol, wf, pose, intr, cfg.cols, cfg.rows, color_volume=cv)
    raycast = lambda: vol.raycast(pose, intr, rp, rn)
    mesh = lambda: vol.fetchMesh()
    res = {"config": cfg.name, "device": torch.cuda.get_device_name(0), "frames": frames, "nodes": int(len(pos)), "k": cfg.k,
           "cols": cfg.cols, "rows": cfg.rows, "vertices": int(vertices.shape[0]), "triangles": int(triangles.shape[0]), "max_extent": 16,
           "triangles_drawn": counts[0], "triangles_invalid": counts[1], "triangles_degenerate": counts[2], "triangles_stretched": counts[3],
           "triangles_off_screen": counts[4], "pixels_covered": counts[5], "raycast_hits": int(cast.sum().item()),
           "raycast_hits_covered": int((cast & hit).sum().item()), "samples_ms": {}}
    for key, fn in (("raycast_ms", raycast), ("render_mesh_ms", render_all), ("render_mesh_points_only_ms", render_points), ("fetch_mesh_ms", mesh),
                    ("render_live_model_ms", live), ("raycast_again_ms", raycast)):
        res[key], res["samples_ms"][key] = median_ms(fn)
    res["render_over_raycast"] = res["render_mesh_ms"] / res["raycast_ms"]
    res["live_model_over_raycast"] = res["render_live_model_ms"] / res["raycast_ms"]
    res["how"] = ("medians of 5 after 2 warm-up calls, HIP events around one call each, one process; fetch_mesh_ms and render_live_model_ms "
                  "include the host read-back of the mesh counts and the mirrors' allocations")
    print(json.dumps(res))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
