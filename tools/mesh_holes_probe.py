#!/usr/bin/env python3
"""Times dfusion_mesh_boundary_loops, and dfusion_mesh_fill_holes at max_edges 16, 64 and 1024, on the mesh of the headline volume (512^3
after a few warped frames, the one tools/mesh_probe.py extracts) and on that mesh simplified at one voxel, beside dfusion_mesh_adjacency
and the extraction itself in the same process: medians of 5 after two warm-ups, HIP events.  Also the loop counts of both meshes, the
histogram of the loop lengths, how many loops each setting fills and the Euler characteristic before and after.
usage: mesh_holes_probe.py [config=512] [frames=5] [out.json=profiles/mesh_holes_probe.json]"""
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from dynamicfusion_amd import Intr, TsdfVolume, WarpField, capi, compute_dists, mesh_ops, synth, upload_u16  # noqa: E402
from mesh_probe import median_ms  # noqa: E402

SETTINGS = (16, 64, 1024)
HISTOGRAM_EDGES = (3, 4, 5, 8, 16, 32, 64, 128, 256, 1024, 4096, 1 << 32)      # [lo, hi) bins of the loop lengths


def probe(L, st, name, vertices, triangles, ms_fetch):
    nv, nt = int(vertices.shape[0]), int(triangles.shape[0])
    nxt, loop, rank, members = (torch.empty(nv, dtype=torch.int32, device="cuda") for _ in range(4))
    start = torch.empty(nv + 1, dtype=torch.int32, device="cuda")
    counts = torch.zeros(8, dtype=torch.int64, device="cuda")
    acounts = torch.zeros(8, dtype=torch.int64, device="cuda")
    rows = torch.empty(nv + 1, dtype=torch.int32, device="cuda")
    nbr = torch.empty(6 * nt, dtype=torch.int32, device="cuda")
    cls = torch.empty(nv, dtype=torch.uint8, device="cuda")
    adjacency = lambda: capi.check(L.dfusion_mesh_adjacency(triangles.data_ptr(), nt, nv, rows.data_ptr(), nbr.data_ptr(), 6 * nt, cls.data_ptr(),
                                                            acounts.data_ptr(), st))
    loops = lambda: capi.check(L.dfusion_mesh_boundary_loops(triangles.data_ptr(), nt, nv, nxt.data_ptr(), loop.data_ptr(), rank.data_ptr(), start.data_ptr(),
                                                             nv, members.data_ptr(), nv, counts.data_ptr(), st))
    per_vertex = lambda: capi.check(L.dfusion_mesh_boundary_loops(triangles.data_ptr(), nt, nv, None, loop.data_ptr(), None, None, 0, None, 0,
                                                                  counts.data_ptr(), st))
    ms_adj, all_adj = median_ms(adjacency)
    ms_loops, all_loops = median_ms(loops)
    ms_pv, all_pv = median_ms(per_vertex)
    c = [int(x) for x in counts.tolist()]
    a = [int(x) for x in acounts.tolist()]
    lengths = (start[1:c[0] + 1] - start[:c[0]]).long()
    histogram = {"%d..%d" % (lo, hi - 1): int(((lengths >= lo) & (lengths < hi)).sum()) for lo, hi in zip(HISTOGRAM_EDGES[:-1], HISTOGRAM_EDGES[1:])}
    euler = a[4] - a[1] + nt - a[5]
    fills, samples = {}, {"adjacency": all_adj, "boundary_loops": all_loops, "boundary_loops_per_vertex_only": all_pv}
    for max_edges in SETTINGS:
        fcounts = torch.zeros(8, dtype=torch.int64, device="cuda")
        capi.check(L.dfusion_mesh_fill_holes(vertices.data_ptr(), nv, triangles.data_ptr(), nt, max_edges, 0, None, 0, None, 0, None, fcounts.data_ptr(), st))
        kv, kt = (int(x) for x in fcounts[:2].tolist())
        out_v = torch.empty((kv, 4), dtype=torch.float32, device="cuda")
        out_t = torch.empty((kt, 3), dtype=torch.int32, device="cuda")
        src = torch.empty(kv, dtype=torch.int32, device="cuda")
        fill = lambda: capi.check(L.dfusion_mesh_fill_holes(vertices.data_ptr(), nv, triangles.data_ptr(), nt, max_edges, 0, out_v.data_ptr(), kv,
                                                            out_t.data_ptr(), kt, src.data_ptr(), fcounts.data_ptr(), st))
        ms_fill, all_fill = median_ms(fill)
        f = [int(x) for x in fcounts.tolist()]
        topo = mesh_ops.mesh_topology(out_t, kv)
        fills[str(max_edges)] = {"ms": ms_fill, "over_adjacency": ms_fill / ms_adj, "over_fetch_mesh": ms_fill / ms_fetch,
                                 "counts": dict(zip(mesh_ops.FILL_COUNT_NAMES, f)), "euler_after": topo["euler"],
                                 "boundary_edges_after": topo["boundary_edges"], "irregular_edges_after": topo["irregular_edges"]}
        samples["fill_holes_%d" % max_edges] = all_fill
    return {"mesh": name, "vertices": nv, "triangles": nt, "counts": dict(zip(mesh_ops.LOOP_COUNT_NAMES, c)),
            "adjacency_counts": dict(zip(mesh_ops.TOPOLOGY_NAMES, a)), "euler": euler, "loop_length_histogram": histogram,
            "adjacency_ms": ms_adj, "boundary_loops_ms": ms_loops, "boundary_loops_per_vertex_only_ms": ms_pv,
            "boundary_loops_over_adjacency": ms_loops / ms_adj, "boundary_loops_over_fetch_mesh": ms_loops / ms_fetch,
            "fill_holes": fills, "samples_ms": samples}


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "512"
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(REPO, "profiles", "mesh_holes_probe.json")
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
    sv, stri, ssrc, smap = mesh_ops.simplify_mesh(vertices, triangles, voxel)
    meshes = [probe(L, st, "full", vertices, triangles, ms_fetch), probe(L, st, "simplified at one voxel", sv, stri, ms_fetch)]
    res = {"config": cfg.name, "device": torch.cuda.get_device_name(0), "frames": frames, "voxel": voxel,
           "fetch_mesh_ms": ms_fetch, "meshes": meshes, "samples_ms": {"fetch_mesh": all_fetch},
           "how": "medians of 5 after 2 warm-up calls, HIP events around one call each, one process; fetch_mesh = the full-size "
                  "dfusion_extract_mesh call (mesh_probe.py's mesh_full_ms); adjacency = one dfusion_mesh_adjacency call with every output and a "
                  "capacity of 6 T; boundary_loops = one dfusion_mesh_boundary_loops call with every output and capacities of V; "
                  "per_vertex_only = the same with both capacities 0 and only vertex_loop; fill_holes = one dfusion_mesh_fill_holes call of "
                  "exactly the output's size (the loop stage runs inside it); euler = used vertices - edges + valid triangles from "
                  "dfusion_mesh_adjacency's counts"}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
