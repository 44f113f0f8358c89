#!/usr/bin/env python3
"""Times dfusion_mesh_closest_points on the mesh of the headline volume (512^3 after a few warped frames, the one tools/mesh_probe.py
extracts) and measures what the mesh operators do to that surface: the one-sided and symmetric Hausdorff, mean and RMS distances between
the extracted mesh and the mesh after simplify_mesh at 1, 2 and 4 voxels, after 10 smoothing iterations and after fill_holes(64).  fetchMesh
leaves vertices that no triangle uses; they are far from every surface and would be all there is to see in a maximum, so every mesh
is compacted first (remove_small_components with no threshold) and the figures are over used vertices; the raw Hausdorff distance
over all vertices is recorded beside them.  A sample of queries is also answered by brute force over all triangles in f64 torch.
Times are medians of 5 after two warm-ups, HIP events, in one process; the build alone is the call with ONE query.
usage: mesh_closest_probe.py [config=512] [frames=5] [out.json=profiles/mesh_closest_probe.json]"""
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from dynamicfusion_amd import Intr, TsdfVolume, WarpField, capi, compute_dists, mesh_ops, synth, upload_u16  # noqa: E402
from mesh_probe import median_ms  # noqa: E402


def timed_query(L, st, vertices, triangles, points):
    """One dfusion_mesh_closest_points call of `points` against the mesh, timed; beside it the same call with one query (the build)."""
    nv, nt, nq = int(vertices.shape[0]), int(triangles.shape[0]), int(points.shape[0])
    tri = torch.empty(nq, dtype=torch.int32, device="cuda")
    point = torch.empty((nq, 4), dtype=torch.float32, device="cuda")
    counts = torch.zeros(8, dtype=torch.int64, device="cuda")
    call = lambda n: capi.check(L.dfusion_mesh_closest_points(vertices.data_ptr(), nv, triangles.data_ptr(), nt, points.data_ptr(), n, float("inf"),
                                                              tri.data_ptr(), point.data_ptr(), None, counts.data_ptr(), st))
    ms_build, all_build = median_ms(lambda: call(1))
    ms_all, all_all = median_ms(lambda: call(nq))
    c = [int(x) for x in counts.tolist()]
    return {"triangles": nt, "queries": nq, "build_ms": ms_build, "build_and_query_ms": ms_all, "query_ms": ms_all - ms_build,
            "counts": dict(zip(mesh_ops.CLOSEST_COUNT_NAMES, c)), "triangle_tests_per_query": c[6] / max(nq, 1),
            "nodes_visited_per_query": c[7] / max(nq, 1), "samples_ms": {"build": all_build, "build_and_query": all_all}}


def brute_force_d2(vertices, triangles, points, chunk=100000):
    """f64 squared distances of `points` to the nearest triangle, every triangle tried (Ericson's regions, in torch)."""
    P = points[:, None, :3].double()
    best = torch.full((points.shape[0],), float("inf"), dtype=torch.float64, device=points.device)
    dot = lambda x, y: (x * y).sum(-1)
    for t0 in range(0, int(triangles.shape[0]), chunk):
        tri = triangles[t0:t0 + chunk].long()
        A, B, C = (vertices[tri[:, k], :3].double()[None] for k in range(3))
        ab, ac, ap, bp, cp = B - A, C - A, P - A, P - B, P - C
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        den = va + vb + vc
        v, w = vb / den, vc / den                                        # face
        zero, one = torch.zeros_like(d1), torch.ones_like(d1)
        wbc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        cases = [((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), 1 - wbc, wbc), ((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, d2 / (d2 - d6)),
                 ((d6 >= 0) & (d5 <= d6), zero, one), ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1 / (d1 - d3), zero),
                 ((d3 >= 0) & (d4 <= d3), one, zero), ((d1 <= 0) & (d2 <= 0), zero, zero)]
        for cond, cv, cw in cases:                                       # the first test of the routine's order is applied last
            v, w = torch.where(cond, cv, v), torch.where(cond, cw, w)
        e = P - (A + ab * v[..., None] + ac * w[..., None])
        dd = dot(e, e)
        best = torch.minimum(best, torch.where(torch.isnan(dd), torch.full_like(dd, float("inf")), dd).min(1).values)
    return best


def compact(vertices, triangles):
    v, t, _, _ = mesh_ops.remove_small_components(vertices, triangles)
    return v, t


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "512"
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(REPO, "profiles", "mesh_closest_probe.json")
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
    vertices, triangles = compact(raw_vertices, raw_triangles)
    voxel = float(cfg.size) / float(cfg.dims[0])
    variants = {}
    for cells in (1, 2, 4):
        sv, stri, ssrc, smap = mesh_ops.simplify_mesh(vertices, triangles, cells * voxel)
        variants["simplify_mesh at %d voxel%s" % (cells, "" if cells == 1 else "s")] = compact(sv, stri)
    variants["smooth_mesh, 10 iterations"] = (mesh_ops.smooth_mesh(vertices, triangles, iterations=10), triangles)
    fv, ft, fsrc = mesh_ops.fill_holes(vertices, triangles, 64)
    variants["fill_holes(64)"] = compact(fv, ft)
    distances = {}
    for label, (v, t) in variants.items():
        d = mesh_ops.mesh_distance(vertices, triangles, v, t)
        d["vertices"], d["triangles"] = int(v.shape[0]), int(t.shape[0])
        for k in ("hausdorff",):
            d[k + "_voxels"] = d[k] / voxel
        for side in ("a_to_b", "b_to_a"):
            for k in ("max", "mean", "rms"):
                d[side][k + "_voxels"] = d[side][k] / voxel
        distances[label] = d
    raw_smooth = mesh_ops.smooth_mesh(raw_vertices, raw_triangles, iterations=10)
    raw = {"vertices": int(raw_vertices.shape[0]), "unused_vertices": int(raw_vertices.shape[0]) - int(vertices.shape[0]),
           "hausdorff_voxels_over_all_vertices, smooth_mesh": mesh_ops.mesh_distance(raw_vertices, raw_triangles, raw_smooth, raw_triangles)["hausdorff"] / voxel,
           "self_distance_max_voxels_over_used_vertices": mesh_ops.mesh_distance(vertices, triangles, vertices, triangles)["hausdorff"] / voxel}
    cv, ct = variants["simplify_mesh at 4 voxels"]
    sample = cv[torch.linspace(0, int(cv.shape[0]) - 1, 384, device="cuda").long()].contiguous()
    tri, point = mesh_ops.closest_points(vertices, triangles, sample)
    want = brute_force_d2(vertices, triangles, sample)
    got = point[:, 3].double()
    brute = {"queries": 384, "triangles": int(triangles.shape[0]), "max_difference_of_distance_voxels": float((got.sqrt() - want.sqrt()).abs().max()) / voxel,
             "max_relative_difference_of_d2_beyond_a_hundredth_voxel": float(torch.where(want.sqrt() > 0.01 * voxel, (got - want).abs() / want, torch.zeros_like(want)).max()),
             "queries_beyond_a_hundredth_voxel": int((want.sqrt() > 0.01 * voxel).sum()),
             "max_distance_voxels": float(want.max().sqrt()) / voxel,
             "what": "384 vertices of the mesh simplified at 4 voxels against the extracted mesh: the call's d2 (f32) beside the minimum over ALL "
                     "triangles of an f64 evaluation in torch"}
    sv, stri = variants["simplify_mesh at 1 voxel"]
    timings = {"simplified-at-one-voxel vertices against the extracted mesh": timed_query(L, st, vertices, triangles, sv),
               "extracted vertices against the mesh simplified at one voxel": timed_query(L, st, sv, stri, vertices),
               "extracted vertices against the extracted mesh": timed_query(L, st, vertices, triangles, vertices)}
    res = {"config": cfg.name, "device": torch.cuda.get_device_name(0), "frames": frames, "voxel": voxel,
           "vertices": int(vertices.shape[0]), "triangles": int(triangles.shape[0]), "fetch_mesh": raw, "brute_force_check": brute,
           "timings": timings, "distances": distances,
           "how": "medians of 5 after 2 warm-up calls, HIP events around one dfusion_mesh_closest_points call each (no bary), one process, nothing "
                  "else of this project on the device; build = the same call with ONE query (bounds, codes, sort, tree, boxes and a "
                  "one-lane query), query = the full call less that; distances: a = the extracted mesh without its unused vertices, b = the operator's output, "
                  "a_to_b samples a's vertices against mesh b; max, mean and rms are distances (not squared), *_voxels the same in "
                  "voxels; queries run in the caller's order, the traversal stack lives in scratch memory -- neither alternative was measured"}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
