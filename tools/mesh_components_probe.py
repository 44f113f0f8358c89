#!/usr/bin/env python3
"""Times dfusion_mesh_components and dfusion_mesh_filter (min_triangles 100) on the mesh of the headline volume (512^3 after a few
warped frames, the one tools/mesh_probe.py extracts) beside the extraction itself in the same process: medians of 5 after two warm-ups,
HIP events.  usage: mesh_components_probe.py [config=512] [frames=5] [out.json=profiles/mesh_components_probe.json]"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from dynamicfusion_amd import Intr, TsdfVolume, WarpField, capi, compute_dists, synth, upload_u16  # noqa: E402
from mesh_probe import median_ms  # noqa: E402

MIN_TRIANGLES = 100


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "512"
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(REPO, "profiles", "mesh_components_probe.json")
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
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    components = lambda: capi.check(L.dfusion_mesh_components(triangles.data_ptr(), nt, nv, label.data_ptr(), count.data_ptr(), counts.data_ptr(), st))
    labels_only = lambda: capi.check(L.dfusion_mesh_components(triangles.data_ptr(), nt, nv, label.data_ptr(), None, None, st))
    fcounts = torch.zeros(2, dtype=torch.int64, device="cuda")
    filter_count = lambda: capi.check(L.dfusion_mesh_filter(triangles.data_ptr(), nt, nv, label.data_ptr(), count.data_ptr(), MIN_TRIANGLES, 0,
                                                            None, 0, None, 0, None, fcounts.data_ptr(), st))
    ms_fetch, all_fetch = median_ms(fetch)
    ms_labels, all_labels = median_ms(labels_only)
    ms_comp, all_comp = median_ms(components)
    filter_count()
    kv, kt = (int(c) for c in fcounts.tolist())
    tri_out = torch.empty((max(kt, 1), 3), dtype=torch.int32, device="cuda")
    src = torch.empty(max(kv, 1), dtype=torch.int32, device="cuda")
    filter_full = lambda: capi.check(L.dfusion_mesh_filter(triangles.data_ptr(), nt, nv, label.data_ptr(), count.data_ptr(), MIN_TRIANGLES, 0,
                                                           tri_out.data_ptr(), kt, src.data_ptr(), kv, None, fcounts.data_ptr(), st))
    vout = torch.empty((max(kv, 1), 4), dtype=torch.float32, device="cuda")
    gather = lambda: capi.check(L.dfusion_gather_rows(vertices.data_ptr(), 16, src.data_ptr(), kv, vout.data_ptr(), st))
    ms_fc, all_fc = median_ms(filter_count)
    ms_ff, all_ff = median_ms(filter_full)
    ms_g, all_g = median_ms(gather)
    c = [int(x) for x in counts.tolist()]
    sizes = count.to(torch.int64)
    res = {"config": cfg.name, "device": torch.cuda.get_device_name(0), "frames": frames, "vertices": nv, "triangles": nt,
           "components": c[0], "unused_vertices": c[1], "invalid_triangles": c[2], "largest_component_triangles": c[3],
           "largest_share_of_triangles": c[3] / max(nt, 1), "components_under_100_triangles": int(((sizes > 0) & (sizes < MIN_TRIANGLES)).sum().item()),
           "min_triangles": MIN_TRIANGLES, "kept_vertices": kv, "kept_triangles": kt,
           "fetch_mesh_ms": ms_fetch, "mesh_components_ms": ms_comp, "mesh_components_labels_only_ms": ms_labels,
           "mesh_filter_count_only_ms": ms_fc, "mesh_filter_ms": ms_ff, "gather_vertices_ms": ms_g,
           "components_plus_filter_ms": ms_comp + ms_ff, "components_plus_filter_over_fetch_mesh": (ms_comp + ms_ff) / ms_fetch,
           "samples_ms": {"fetch_mesh": all_fetch, "components": all_comp, "labels_only": all_labels, "filter_count_only": all_fc, "filter": all_ff,
                          "gather_vertices": all_g},
           "how": "medians of 5 after 2 warm-up calls, HIP events around one call each, one process; fetch_mesh = the full-size "
                  "dfusion_extract_mesh call (mesh_probe.py's mesh_full_ms), filter = one call with exact capacities"}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
