#!/usr/bin/env python3
"""Times dfusion_mesh_simplify at cells of 1, 2 and 4 voxel sizes on the mesh of the headline volume (512^3 after a few warped frames,
the one tools/mesh_probe.py extracts), the count-only call and the full call with exact capacities, beside the extraction itself and
dfusion_mesh_components in the same process: medians of 5 after two warm-ups, HIP events.
usage: mesh_simplify_probe.py [config=512] [frames=5] [out.json=profiles/mesh_simplify_probe.json]"""
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from dynamicfusion_amd import Intr, TsdfVolume, WarpField, capi, compute_dists, synth, upload_u16  # noqa: E402
from mesh_probe import median_ms  # noqa: E402

COUNT_NAMES = ("vertices", "triangles", "invalid", "collapsed", "fin", "duplicate", "clusters", "unclusterable")


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "512"
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(REPO, "profiles", "mesh_simplify_probe.json")
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
    label = torch.empty(nv, dtype=torch.int32, device="cuda")
    count = torch.empty(nv, dtype=torch.int32, device="cuda")
    ccounts = torch.zeros(4, dtype=torch.int64, device="cuda")
    components = lambda: capi.check(L.dfusion_mesh_components(triangles.data_ptr(), nt, nv, label.data_ptr(), count.data_ptr(), ccounts.data_ptr(), st))
    ms_fetch, all_fetch = median_ms(fetch)
    ms_comp, all_comp = median_ms(components)
    voxel = float(cfg.size) / float(cfg.dims[0])
    counts = torch.zeros(8, dtype=torch.int64, device="cuda")
    cells = []
    for factor in (1, 2, 4):
        cell = factor * voxel
        count_only = lambda: capi.check(L.dfusion_mesh_simplify(vertices.data_ptr(), nv, triangles.data_ptr(), nt, cell, 0, None, 0, None, 0, None, None,
                                                                counts.data_ptr(), st))
        count_only()
        c = [int(x) for x in counts.tolist()]
        out_v = torch.empty((max(c[0], 1), 4), dtype=torch.float32, device="cuda")
        out_t = torch.empty((max(c[1], 1), 3), dtype=torch.int32, device="cuda")
        src = torch.empty(max(c[0], 1), dtype=torch.int32, device="cuda")
        vmap = torch.empty(nv, dtype=torch.int32, device="cuda")
        full = lambda: capi.check(L.dfusion_mesh_simplify(vertices.data_ptr(), nv, triangles.data_ptr(), nt, cell, 0, out_v.data_ptr(), c[0],
                                                          out_t.data_ptr(), c[1], src.data_ptr(), vmap.data_ptr(), counts.data_ptr(), st))
        ms_count, all_count = median_ms(count_only)
        ms_full, all_full = median_ms(full)
        cells.append({"cell_voxels": factor, "cell": cell, "counts": dict(zip(COUNT_NAMES, c)), "triangles_kept_share": c[1] / max(nt, 1),
                      "count_only_ms": ms_count, "full_ms": ms_full, "full_over_fetch_mesh": ms_full / ms_fetch,
                      "samples_ms": {"count_only": all_count, "full": all_full}})
    res = {"config": cfg.name, "device": torch.cuda.get_device_name(0), "frames": frames, "vertices": nv, "triangles": nt, "voxel": voxel,
           "fetch_mesh_ms": ms_fetch, "mesh_components_ms": ms_comp, "cells": cells,
           "samples_ms": {"fetch_mesh": all_fetch, "components": all_comp},
           "how": "medians of 5 after 2 warm-up calls, HIP events around one call each, one process; fetch_mesh = the full-size "
                  "dfusion_extract_mesh call (mesh_probe.py's mesh_full_ms); full = one dfusion_mesh_simplify call with exact capacities, "
                  "vertex_src and vertex_map"}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
