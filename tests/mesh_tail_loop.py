"""The mesh tail on the closed non-rigid loop's own state: the colour loop (tests/color_loop.py, FAST) runs on both backends, and on the
frames of TAIL_FRAMES the on_frame hook of nonrigid_loop.run takes the loop's volume, colour volume and warp field -- as they stand
after that frame -- through everything that follows the fusion:

    1 fetchMesh with normals              mesh_ref.extract_mesh + the oracle's extract_normals
    2 mesh_components                     mesh_components_ref.components
    3 remove_small_components (25)        mesh_components_ref.remove_small, the normals gathered by vertex_src; also keep_largest
    4 simplify_mesh (1.5 voxels)          mesh_simplify_ref.simplify, plain and keep_first, on the filtered mesh
    5 mesh_adjacency, mesh_topology       mesh_smooth_ref.adjacency, on the simplified mesh
    6 smooth_mesh (3 iterations)          mesh_smooth_ref.smooth, boundary fixed and free
    7 fetchMesh, all three options        the composition of 1 - 6, the normals taken at the SMOOTHED vertices
    8 warp + renderMesh of 7's mesh       the oracle's warp_points + render_ref.render at the frame's pose;
      renderLiveModelFiltered             the composition of 1, 3, color_ref.fetch, the warp and the render, and with keep_largest

oracle_tail(ob, pose) and gpu_tail(be, pose) return the same flat dict {item: numpy array} (floats as their bits), in the order of the
steps; first_difference names the first item that differs.  figures(tail) are the numbers the non-vacuity conditions are about, taken
from a tail's items; the oracle's are pinned in tests/test_gpu_nonrigid_loop_mesh_tail.py.  The fused surface is what the synthetic
meshes of the features' own suites are not: several components either side of the threshold, vertices no triangle uses, boundary edges,
and after clustering fins and duplicates, all in one mesh."""
import numpy as np

import color_loop as CL
import color_ref as CR
import mesh_components_ref as MC
import mesh_ref as MR
import mesh_simplify_ref as MS
import mesh_smooth_ref as SM
import nonrigid_loop as NL
import oracle_lib as O
import render_ref as RR
from dynamicfusion_amd import synth

F32 = np.float32
TAIL_FRAMES = (3, 6)
MIN_TRIANGLES = 25
CELL_VOXELS = 1.5
ITERATIONS = 3


def cell_of(case):
    vs, _ = NL._geometry(case.cfg)
    return float(F32(CELL_VOXELS) * vs[0])


class _KeepPose:
    """The pose of the frame's last ray-cast: the frame's camera pose."""

    def raycast(self, cam_pose):
        self.last_pose = cam_pose
        return super().raycast(cam_pose)


class TailOracleBackend(_KeepPose, CL.ColorOracleBackend):
    pass


class TailGpuBackend(_KeepPose, CL.ColorGpuBackend):
    pass


def _u(a):
    """The bits of an array: float32 as uint32, every index as uint32, the rest as it is."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a.view(np.uint32).copy()
    if a.dtype in (np.int32, np.uint32):
        return a.view(np.uint32).copy()
    if a.dtype in (np.int64, np.uint64):
        return a.astype(np.int64)
    return a.copy()


def _world2cam(pose):
    return np.linalg.inv(np.asarray(pose, np.float64).reshape(4, 4)).astype(F32)


def _put_render(out, name, r):
    for key in ("points", "normals", "attr", "colors", "tri", "counts"):
        if r.get(key) is not None:
            out["%s.%s" % (name, key)] = _u(r[key])


# ------------------------------------------------------------------------------------------------------------------ oracle
def oracle_tail(ob, pose):
    cfg = ob.cfg
    case = ob.case
    aff = synth.aff12(ob.pose)
    rinv = np.linalg.inv(ob.pose[:3, :3].astype(np.float64)).astype(F32)
    world2vol = synth.aff12(np.linalg.inv(ob.pose.astype(np.float64)).astype(F32))
    w2c = synth.aff12(_world2cam(pose))
    cell = cell_of(case)
    out = {}

    def normals_at(v):
        return O.extract_normals(ob._ovol(), aff, rinv, v, cfg.gradient_delta_factor)

    def live_render(v, t, n, colors=None):
        wp, wn = O.warp_points(ob.pos, ob.dq, ob.sig, np.ascontiguousarray(v[:, :3]), np.ascontiguousarray(n[:, :3]), ob.k)
        warped = np.zeros_like(v); warped[:, :3] = wp
        wnormals = np.zeros_like(v); wnormals[:, :3] = wn
        return RR.render(warped, t, cfg.cols, cfg.rows, cfg.intr, world2cam=w2c, normals=wnormals, attr=v, colors=colors)

    # 1
    m = MR.extract_mesh(ob.vol, cfg.dims, ob.vs, aff)
    v, t = m.vertices, m.triangles
    n = normals_at(v)
    out.update({"1.vertices": _u(v), "1.triangles": _u(t), "1.normals": _u(n)})
    # 2
    label, count, counts = MC.components(t, len(v))
    out.update({"2.label": _u(label), "2.triangle_count": _u(count), "2.counts": _u(counts)})
    # 3
    kept = {}
    for name, largest in (("3", False), ("3L", True)):
        fv, ft, src = MC.remove_small(v, t, MIN_TRIANGLES, largest)
        kept[name] = (fv, ft, n[src])
        out.update({name + ".vertices": _u(fv), name + ".triangles": _u(ft), name + ".vertex_src": _u(src), name + ".normals": _u(n[src])})
    fv, ft, fn = kept["3"]
    # 4
    for name, flags in (("4", 0), ("4F", MS.KEEP_FIRST)):
        s = MS.simplify(fv, ft, cell, flags)
        out.update({name + ".vertices": _u(s.vertices), name + ".triangles": _u(s.triangles), name + ".vertex_src": _u(s.vertex_src),
                    name + ".vertex_map": _u(s.vertex_map), name + ".counts": _u(s.counts)})
        if not flags:
            sv, st = s.vertices, s.triangles
    # 5
    adj = SM.adjacency(st, len(sv))
    out.update({"5.row_start": _u(adj.row_start), "5.neighbours": _u(adj.neighbours), "5.vertex_class": _u(adj.vertex_class),
                "5.counts": _u(adj.counts), "5.topology": _u(np.array(list(adj.counts) + [SM.euler(adj, len(st))], np.int64))})
    # 6
    fixed = SM.smooth(sv, adj, ITERATIONS)
    out.update({"6.fixed": _u(fixed), "6.free": _u(SM.smooth(sv, adj, ITERATIONS, flags=0))})
    # 7
    cn = normals_at(fixed)
    out.update({"7.vertices": _u(fixed), "7.triangles": _u(st), "7.normals": _u(cn), "7.plain.vertices": _u(fixed), "7.plain.triangles": _u(st),
                "7.counts": _u(np.array([len(v), len(t)], np.int64))})
    out["7.normals_before_smoothing"] = _u(normals_at(sv))                   # (a figure's input; the GPU side has no such item)
    # 8
    _put_render(out, "8.composed", live_render(fixed, st, cn))
    for name in ("3", "3L"):
        kv, kt, kn = kept[name]
        colors = CR.fetch(ob.color, cfg.dims, ob.vs, world2vol, kv)
        _put_render(out, "8.filtered" + name[1:], live_render(kv, kt, kn, colors))
    _put_render(out, "8.unfiltered", live_render(v, t, n, CR.fetch(ob.color, cfg.dims, ob.vs, world2vol, v)))   # (for the figures)
    return out


ORACLE_ONLY = ("7.normals_before_smoothing", "8.unfiltered.")


# --------------------------------------------------------------------------------------------------------------------- GPU
def gpu_tail(be, pose):
    import torch
    from dynamicfusion_amd import frontend, mesh_ops
    cfg = be.cfg
    cell = cell_of(be.case)
    w2c = _world2cam(pose)
    out = {}

    def h(x):
        return _u(x.cpu().numpy())

    # 1
    v, t, n = be.v.fetchMesh(with_normals=True)
    out.update({"1.vertices": h(v), "1.triangles": h(t), "1.normals": h(n)})
    # 2
    label, count, counts = mesh_ops.mesh_components(t, int(v.shape[0]), return_counts=True)
    out.update({"2.label": h(label), "2.triangle_count": h(count), "2.counts": h(counts)})
    # 3
    for name, largest in (("3", False), ("3L", True)):
        kv, kt, (kn,), src = mesh_ops.remove_small_components(v, t, min_triangles=MIN_TRIANGLES, keep_largest=largest, attributes=(n,))
        out.update({name + ".vertices": h(kv), name + ".triangles": h(kt), name + ".vertex_src": h(src), name + ".normals": h(kn)})
        if not largest:
            fv, ft = kv, kt
    # 4
    for name, first in (("4", False), ("4F", True)):
        gv, gt, src, vmap, counts = mesh_ops.simplify_mesh(fv, ft, cell, keep_first=first, return_counts=True)
        out.update({name + ".vertices": h(gv), name + ".triangles": h(gt), name + ".vertex_src": h(src), name + ".vertex_map": h(vmap),
                    name + ".counts": h(counts)})
        if not first:
            sv, st = gv, gt
    # 5
    row_start, neighbours, vclass, counts = mesh_ops.mesh_adjacency(st, int(sv.shape[0]), return_counts=True)
    topo = mesh_ops.mesh_topology(st, int(sv.shape[0]))
    out.update({"5.row_start": h(row_start), "5.neighbours": h(neighbours), "5.vertex_class": h(vclass), "5.counts": h(counts),
                "5.topology": np.array([topo[k] for k in mesh_ops.TOPOLOGY_NAMES] + [topo["euler"]], np.int64)})
    # 6
    out.update({"6.fixed": h(mesh_ops.smooth_mesh(sv, st, ITERATIONS)), "6.free": h(mesh_ops.smooth_mesh(sv, st, ITERATIONS, fix_boundary=False))})
    # 7
    cv, ct, cn = be.v.fetchMesh(with_normals=True, min_component_triangles=MIN_TRIANGLES, simplify_cell=cell, smooth_iterations=ITERATIONS)
    mesh_counts = be.v.last_mesh_counts_
    pv, pt = be.v.fetchMesh(min_component_triangles=MIN_TRIANGLES, simplify_cell=cell, smooth_iterations=ITERATIONS)
    out.update({"7.vertices": h(cv), "7.triangles": h(ct), "7.normals": h(cn), "7.plain.vertices": h(pv), "7.plain.triangles": h(pt),
                "7.counts": np.array(mesh_counts, np.int64)})
    # 8
    p3, n3 = cv[:, :3].contiguous(), cn[:, :3].contiguous()
    be.wf.warp(p3, n3)
    warped = torch.zeros_like(cv); warped[:, :3] = p3
    wnormals = torch.zeros_like(cv); wnormals[:, :3] = n3
    r = frontend.renderMesh(be.intr, warped, ct, cfg.cols, cfg.rows, world2cam=w2c, normals=wnormals, attr=cv, return_tri=True, return_counts=True)
    _put_render(out, "8.composed", {k: x.cpu().numpy() for k, x in zip(("points", "normals", "attr", "colors", "tri", "counts"), r) if x is not None})
    for name, largest in (("8.filtered", False), ("8.filteredL", True)):
        r = frontend.renderLiveModelFiltered(be.v, be.wf, pose, be.intr, cfg.cols, cfg.rows, color_volume=be.cv, min_component_triangles=MIN_TRIANGLES,
                                             keep_largest=largest)
        _put_render(out, name, {k: x.cpu().numpy() for k, x in zip(("points", "normals", "attr", "colors"), r)})
    return out


# --------------------------------------------------------------------------------------------------------------------- the runs
def run(be, case, tail):
    """The colour loop on `be` with `tail` (oracle_tail or gpu_tail) on the frames of TAIL_FRAMES: (stage record, {frame: tail})."""
    tails = {}

    def on_frame(f, b):
        if f in TAIL_FRAMES:
            tails[f] = tail(b, b.last_pose)
    return NL.run(be, case, on_frame=on_frame), tails


def first_difference(got, want):
    """None, or a message naming the first item of the oracle's tail that the GPU's lacks or has with other bits.  The renders' tri and
    counts exist only where the GPU side asked for them."""
    for key, w in want.items():
        if key.startswith(ORACLE_ONLY):
            continue
        if key not in got:
            if key.startswith("8.filtered") and key.endswith((".tri", ".counts")):
                continue
            return "%s: missing" % key
        g = got[key]
        if g.shape != w.shape or g.dtype != w.dtype:
            return "%s: %s %s against %s %s" % (key, g.dtype, g.shape, w.dtype, w.shape)
        if not np.array_equal(g, w):
            return "%s: %d of %d elements differ" % (key, int((g != w).sum()), w.size)
    extra = sorted(set(got) - set(want))
    return "items %s have no restatement" % extra if extra else None


def figures(tail):
    """The numbers of one frame's tail that the non-vacuity conditions are about."""
    count = tail["2.triangle_count"].astype(np.int64)
    sizes = count[count > 0]
    simp = dict(zip(MS.COUNT_NAMES, (int(c) for c in tail["4.counts"])))
    topo = dict(zip(SM.COUNT_NAMES, (int(c) for c in tail["5.counts"])))
    cls = tail["5.vertex_class"]
    fig = dict(vertices=int(tail["1.vertices"].shape[0]), triangles=int(tail["1.triangles"].shape[0]), components=len(sizes),
               small=int((sizes < MIN_TRIANGLES).sum()), large=int((sizes >= MIN_TRIANGLES).sum()), unused_vertices=int(tail["2.counts"][1]),
               filtered_triangles=int(tail["3.triangles"].shape[0]), largest_triangles=int(tail["3L.triangles"].shape[0]),
               simplified_vertices=simp["vertices"], simplified_triangles=simp["triangles"], collapsed=simp["collapsed"], fin=simp["fin"],
               duplicate=simp["duplicate"], boundary_edges=topo["boundary_edges"], irregular_edges=topo["irregular_edges"],
               class1=int((cls == 1).sum()), class2=int((cls == 2).sum()), class3=int((cls == 3).sum()),
               moved_fixed=int((tail["6.fixed"] != tail["4.vertices"]).any(1).sum()), moved_free=int((tail["6.free"] != tail["4.vertices"]).any(1).sum()),
               pixels_composed=int(tail["8.composed.counts"][5]), pixels_filtered=int((tail["8.filtered.points"][..., 2] != RR.QNAN_BITS).sum()))
    if "7.normals_before_smoothing" in tail:
        fig["normals_changed_by_smoothing"] = int((tail["7.normals"] != tail["7.normals_before_smoothing"]).any(1).sum())
    if "8.unfiltered.points" in tail:
        fig["pixels_changed_by_filter"] = int((tail["8.filtered.points"] != tail["8.unfiltered.points"]).any(-1).sum())
        fig["pixels_changed_by_largest"] = int((tail["8.filteredL.points"] != tail["8.unfiltered.points"]).any(-1).sum())
    return fig


def nonvacuity(fig):
    """The conditions on one frame's figures (the oracle's); returns the list of those missed."""
    miss = []

    def need(ok, what):
        if not ok:
            miss.append(what)
    need(fig["small"] >= 3 and fig["large"] >= 2, "%d components under %d triangles, %d at or above" % (fig["small"], MIN_TRIANGLES, fig["large"]))
    need(fig["unused_vertices"] > 0, "no vertex without a triangle")
    need(fig["boundary_edges"] > 0, "no boundary edge")
    need(fig["fin"] > 0 and fig["duplicate"] > 0, "%d fin and %d duplicate triangles" % (fig["fin"], fig["duplicate"]))
    need(fig["class1"] >= 1 and fig["class2"] >= 1, "%d vertices of class 1, %d of class 2" % (fig["class1"], fig["class2"]))
    need(fig["moved_fixed"] > 0 and fig["moved_free"] > fig["moved_fixed"], "smoothing moved %d / %d vertices" % (fig["moved_fixed"], fig["moved_free"]))
    need(fig["normals_changed_by_smoothing"] > 0, "the normals at the smoothed vertices are those at the unsmoothed ones")
    need(fig["pixels_changed_by_filter"] > 0 or fig["filtered_triangles"] < fig["triangles"], "the filter changed neither a pixel nor the triangle count")
    need(fig["largest_triangles"] < fig["filtered_triangles"], "keep_largest kept what the threshold kept")
    need(fig["pixels_composed"] > 5000 and fig["pixels_filtered"] > 5000, "%d / %d pixels hit" % (fig["pixels_composed"], fig["pixels_filtered"]))
    return miss
