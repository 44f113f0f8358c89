#!/usr/bin/env python3
"""Times dfusion_mesh_ray_hits on the mesh of the headline volume (512^3 after a few warped frames, compacted: the mesh and the protocol
of tools/mesh_closest_probe.py): the 307 200 pinhole rays of the 640 x 480 headline camera at the last frame's pose, nearest hit and
any-hit, and visible_points of the mesh's own vertices from that camera.  Times are medians of 5 after two warm-ups, HIP events, in one
process; the build alone is the call with ONE ray.  Beside them, for orientation only, renderMesh's time (profiles/render_probe.json) and
the closest-point query times (profiles/mesh_closest_probe.json) as those files hold them.  No time here is a pass condition.
usage: mesh_rays_probe.py [config=512] [frames=5] [out.json=profiles/mesh_rays_probe.json]"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from dynamicfusion_amd import Intr, TsdfVolume, WarpField, capi, compute_dists, mesh_ops, synth, upload_u16  # noqa: E402
from mesh_probe import median_ms  # noqa: E402


def timed_rays(L, st, vertices, triangles, origins, directions, t_max, any_hit):
    """One dfusion_mesh_ray_hits call of the rays against the mesh, timed; beside it the same call with one ray (the build)."""
    nv, nt, nr = int(vertices.shape[0]), int(triangles.shape[0]), int(origins.shape[0])
    tri = torch.empty(nr, dtype=torch.int32, device="cuda")
    hit = torch.empty((nr, 4), dtype=torch.float32, device="cuda")
    counts = torch.zeros(8, dtype=torch.int64, device="cuda")
    call = lambda n: capi.check(L.dfusion_mesh_ray_hits(vertices.data_ptr(), nv, triangles.data_ptr(), nt, origins.data_ptr(), directions.data_ptr(), n,
                                                        0.0, t_max, 1 if any_hit else 0, tri.data_ptr(), None if any_hit else hit.data_ptr(), None,
                                                        counts.data_ptr(), st))
    ms_build, all_build = median_ms(lambda: call(1))
    ms_all, all_all = median_ms(lambda: call(nr))
    c = [int(x) for x in counts.tolist()]
    return {"triangles": nt, "rays": nr, "any_hit": any_hit, "t_max": t_max, "build_ms": ms_build, "build_and_walk_ms": ms_all, "walk_ms": ms_all - ms_build,
            "counts": dict(zip(mesh_ops.RAY_COUNT_NAMES, c)), "triangle_tests_per_ray": c[6] / max(nr, 1), "nodes_visited_per_ray": c[7] / max(nr, 1),
            "samples_ms": {"build": all_build, "build_and_walk": all_all}}


def recorded(path, *keys):
    try:
        x = json.load(open(os.path.join(REPO, "profiles", path)))
        for k in keys:
            x = x[k]
        return x
    except (OSError, KeyError, ValueError):
        return None


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "512"
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(REPO, "profiles", "mesh_rays_probe.json")
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
    raw_vertices, raw_triangles = vol.fetchMesh()
    vertices, triangles, _, _ = mesh_ops.remove_small_components(raw_vertices, raw_triangles)
    pose = np.asarray(synth.camera_pose(cfg, frames - 1), np.float64).reshape(4, 4)      # camera to world
    eye = pose[:3, 3].astype(np.float32)
    v, u = np.meshgrid(np.arange(cfg.rows), np.arange(cfg.cols), indexing="ij")
    cam = np.stack([(u - intr.cx) / intr.fx, (v - intr.cy) / intr.fy, np.ones_like(u, np.float64)], -1).reshape(-1, 3)
    d = np.zeros((len(cam), 4), np.float32)
    d[:, :3] = (cam @ pose[:3, :3].T).astype(np.float32)                # unit depth along the optical axis: t is the depth
    o = np.zeros_like(d)
    o[:, :3] = eye
    origins, directions = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    inf = float("inf")
    timings = {"camera rays, nearest hit": timed_rays(L, st, vertices, triangles, origins, directions, inf, False),
               "camera rays, any hit": timed_rays(L, st, vertices, triangles, origins, directions, inf, True)}
    eyes = torch.zeros_like(vertices)
    eyes[:, :3] = torch.from_numpy(eye).cuda()
    to_vertices = vertices - eyes
    timings["segments from the eye to the mesh's own vertices, any hit on [0, 1 - 2^-10] (what visible_points runs)"] = \
        timed_rays(L, st, vertices, triangles, eyes, to_vertices, 1.0 - 2.0 ** -10, True)
    ms_visible, all_visible = median_ms(lambda: mesh_ops.visible_points(vertices, triangles, vertices, eye.tolist()))
    visible = mesh_ops.visible_points(vertices, triangles, vertices, eye.tolist())
    tri, hit = mesh_ops.ray_hits(vertices, triangles, origins, directions)
    depth = hit[:, 3][tri != -1]
    res = {"config": cfg.name, "device": torch.cuda.get_device_name(0), "frames": frames, "vertices": int(vertices.shape[0]),
           "triangles": int(triangles.shape[0]), "camera": {"cols": cfg.cols, "rows": cfg.rows, "rays": int(origins.shape[0]), "eye": eye.tolist()},
           "timings": timings,
           "visible_points": {"points": int(vertices.shape[0]), "visible": int(visible.sum()), "mirror_ms": ms_visible, "samples_ms": all_visible,
                              "what": "mesh_ops.visible_points of the mesh's own vertices from the camera: the call above plus the mirror's five torch "
                                      "launches and allocations"},
           "camera_hits": {"pixels_with_a_hit": int((tri != -1).sum()), "depth_min": float(depth.min()) if depth.numel() else None,
                           "depth_max": float(depth.max()) if depth.numel() else None},
           "for_orientation": {"render_mesh_ms (profiles/render_probe.json: the rasteriser on the warped mesh, one camera)": recorded("render_probe.json", "render_mesh_ms"),
                               "closest_points query_ms (profiles/mesh_closest_probe.json)":
                                   {k: x.get("query_ms") for k, x in (recorded("mesh_closest_probe.json", "timings") or {}).items()},
                               "closest_points build_ms (same file)":
                                   {k: x.get("build_ms") for k, x in (recorded("mesh_closest_probe.json", "timings") or {}).items()}},
           "how": "medians of 5 after 2 warm-up calls, HIP events around one dfusion_mesh_ray_hits call each (no bary), one process, nothing else of "
                  "this project on the device; build = the same call with ONE ray (bounds, codes, sort, tree, boxes and a one-lane walk), walk = the "
                  "full call less that; rays run in the caller's order (row-major pixels; vertices in extraction order), the traversal stack lives in "
                  "scratch memory -- neither alternative was measured, and no time here is a pass condition"}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
