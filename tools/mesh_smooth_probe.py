#!/usr/bin/env python3
"""Times dfusion_mesh_adjacency and one lambda | mu iteration of dfusion_mesh_smooth on the mesh of the headline volume (512^3 after a few
warped frames, the one tools/mesh_probe.py extracts) and on that mesh simplified at one voxel, beside the extraction itself and
dfusion_mesh_simplify in the same process: medians of 5 after two warm-ups, HIP events.  Also the eight counts of both meshes and the share
of triangles whose smallest angle is under 10 degrees before and after 10 iterations.
usage: mesh_smooth_probe.py [config=512] [frames=5] [out.json=profiles/mesh_smooth_probe.json]"""
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from dynamicfusion_amd import Intr, TsdfVolume, WarpField, capi, compute_dists, mesh_ops, synth, upload_u16  # noqa: E402
from mesh_probe import median_ms  # noqa: E402


def share_under_10_degrees(vertices, triangles):
    """The share of the triangles whose smallest angle is under 10 degrees (f64, on the device; a figure of merit, not part of any
    rule; a triangle with a side of length 0 is not counted as one)."""
    p = vertices[:, :3].double()
    t = triangles.long()
    a, b, c = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]

    def cos(o, x, y):
        u, w = x - o, y - o
        return (u * w).sum(1) / (u.norm(dim=1) * w.norm(dim=1)).clamp_min(1e-300)
    largest_cos = torch.maximum(torch.maximum(cos(a, b, c), cos(b, c, a)), cos(c, a, b))
    return float((largest_cos > 0.984807753012208).double().mean())      # cos 10 degrees


def probe(L, st, name, vertices, triangles, ms_fetch):
    nv, nt = int(vertices.shape[0]), int(triangles.shape[0])
    rows = torch.empty(nv + 1, dtype=torch.int32, device="cuda")
    nbr = torch.empty(6 * nt, dtype=torch.int32, device="cuda")
    cls = torch.empty(nv, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(8, dtype=torch.int64, device="cuda")
    out = torch.empty_like(vertices)
    adjacency = lambda: capi.check(L.dfusion_mesh_adjacency(triangles.data_ptr(), nt, nv, rows.data_ptr(), nbr.data_ptr(), 6 * nt, cls.data_ptr(),
                                                            counts.data_ptr(), st))
    count_only = lambda: capi.check(L.dfusion_mesh_adjacency(triangles.data_ptr(), nt, nv, None, None, 0, None, counts.data_ptr(), st))
    ms_adj, all_adj = median_ms(adjacency)
    ms_cnt, all_cnt = median_ms(count_only)
    c = [int(x) for x in counts.tolist()]
    smooth = lambda it: (lambda: capi.check(L.dfusion_mesh_smooth(vertices.data_ptr(), nv, rows.data_ptr(), nbr.data_ptr(), c[0], cls.data_ptr(), it, 0.5,
                                                                  -0.53, mesh_ops.FIX_BOUNDARY, out.data_ptr(), st)))
    ms_one, all_one = median_ms(smooth(1))
    ms_ten, all_ten = median_ms(smooth(10))
    before = share_under_10_degrees(vertices, triangles)
    after = share_under_10_degrees(out, triangles)                       # `out` holds 10 iterations
    degree = (rows[1:] - rows[:-1]).long()
    step_bytes = 16 * c[0] + 4 * c[0] + 8 * nv + 32 * nv                 # gathered positions, indices, row bounds, own position in and out
    return {"mesh": name, "vertices": nv, "triangles": nt, "counts": dict(zip(mesh_ops.TOPOLOGY_NAMES, c)),
            "euler": c[4] - c[1] + nt - c[5], "max_degree": int(degree.max()), "mean_degree": float(degree.double().mean()),
            "adjacency_ms": ms_adj, "adjacency_counts_only_ms": ms_cnt, "adjacency_over_fetch_mesh": ms_adj / ms_fetch,
            "one_iteration_ms": ms_one, "ten_iterations_ms": ms_ten, "step_ms_from_ten": ms_ten / 20,
            "step_GBps_touched_from_ten": step_bytes / (ms_ten / 20 * 1e-3) / 1e9,
            "share_smallest_angle_under_10_deg": {"before": before, "after_10_iterations": after},
            "samples_ms": {"adjacency": all_adj, "counts_only": all_cnt, "one_iteration": all_one, "ten_iterations": all_ten}}


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "512"
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(REPO, "profiles", "mesh_smooth_probe.json")
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
    vertices, triangles = vol.fetchMesh()
    nv, nt = int(vertices.shape[0]), int(triangles.shape[0])
    mcounts = torch.zeros(2, dtype=torch.int64, device="cuda")
    fetch = lambda: capi.check(L.dfusion_extract_mesh(vol.c_volume(), None, aff, vertices.data_ptr(), nv, triangles.data_ptr(), nt, mcounts.data_ptr(), st))
    ms_fetch, all_fetch = median_ms(fetch)
    voxel = float(cfg.size) / float(cfg.dims[0])
    sv, stri, ssrc, smap, scounts = mesh_ops.simplify_mesh(vertices, triangles, voxel, return_counts=True)
    kv, kt = int(sv.shape[0]), int(stri.shape[0])
    simplify = lambda: capi.check(L.dfusion_mesh_simplify(vertices.data_ptr(), nv, triangles.data_ptr(), nt, voxel, 0, sv.data_ptr(), kv, stri.data_ptr(), kt,
                                                          ssrc.data_ptr(), smap.data_ptr(), scounts.data_ptr(), st))
    ms_simplify, all_simplify = median_ms(simplify)
    meshes = [probe(L, st, "full", vertices, triangles, ms_fetch), probe(L, st, "simplified at one voxel", sv, stri, ms_fetch)]
    res = {"config": cfg.name, "device": torch.cuda.get_device_name(0), "frames": frames, "voxel": voxel,
           "fetch_mesh_ms": ms_fetch, "mesh_simplify_ms": ms_simplify, "meshes": meshes,
           "samples_ms": {"fetch_mesh": all_fetch, "mesh_simplify": all_simplify},
           "how": "medians of 5 after 2 warm-up calls, HIP events around one call each, one process; fetch_mesh = the full-size "
                  "dfusion_extract_mesh call (mesh_probe.py's mesh_full_ms); mesh_simplify = one full dfusion_mesh_simplify call at one voxel; "
                  "adjacency = one dfusion_mesh_adjacency call with every output and a capacity of 6 T; one_iteration = dfusion_mesh_smooth "
                  "with iterations = 1 (two steps), out of place, boundary fixed; step_ms_from_ten = the ten-iteration call over its 20 steps; "
                  "step_GBps_touched = the bytes a step asks for (not what reaches HBM) over that time"}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
