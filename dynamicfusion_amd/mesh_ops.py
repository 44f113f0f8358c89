"""Operations on an indexed triangle mesh (fetchMesh's, or any) over the C-ABI: its connected components and the mesh without its small
pieces (include/dfusion.h dfusion_mesh_components / dfusion_mesh_filter / dfusion_gather_rows, where the rule is stated), and the mesh
simplified by vertex clustering (dfusion_mesh_simplify), its vertex adjacency with the edge statistics (dfusion_mesh_adjacency) and Taubin
smoothing over it (dfusion_mesh_smooth), its closed boundary loops (dfusion_mesh_boundary_loops) and the mesh with the small ones
filled (dfusion_mesh_fill_holes), and the closest point of the mesh to every query point with the distances between two meshes
(dfusion_mesh_closest_points), and what every ray hits first on the mesh with the visibility of points from an eye
(dfusion_mesh_ray_hits).  Device tensors in, device tensors out; all compute is in libdfusion_hip.so."""
import math
import struct

import torch

from . import capi
from .tsdf_volume import _flat, _stream


def _triangles(triangles):
    if triangles.dtype != torch.int32 or triangles.dim() != 2 or triangles.shape[1] != 3:
        raise ValueError("triangles %s %s, expected int32 [T, 3]" % (triangles.dtype, tuple(triangles.shape)))
    if not triangles.is_cuda:
        raise ValueError("triangles are not on a CUDA device")
    nt = int(triangles.shape[0])
    return (_flat(triangles) if nt else None), nt


def _points4(x, what, letter="N"):
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != 4 or not x.is_contiguous():
        raise ValueError("%s %s %s, expected contiguous float32 [%s, 4]" % (what, x.dtype, tuple(x.shape), letter))
    return int(x.shape[0])


def _mesh_vertices(vertices, triangles):
    """The checks of an operation that takes the vertices with the triangles -> V."""
    nv = _points4(vertices, "vertices", "V")
    if vertices.device != triangles.device:
        raise ValueError("vertices on %s, triangles on %s" % (vertices.device, triangles.device))
    return nv


def _count_then_exact(run, counts):
    """One count-only call, the read-back of counts[0] = output vertices and counts[1] = output triangles, then -- unless both are 0 --
    one call of exactly that size.  run(n_vertices, n_triangles) allocates outputs of these capacities, makes the call and returns
    them.  -> the outputs of the last call."""
    outs = run(0, 0)
    kv, kt = (int(c) for c in counts[:2].tolist())
    return run(kv, kt) if kv or kt else outs


def mesh_components(triangles, n_vertices, return_counts=False):
    """triangles int32 [T, 3] (uint32 bits) over n_vertices vertices -> (vertex_label int32 [V]: the smallest vertex index of every
    vertex's component, triangle_count int32 [V]: the valid triangles of the component labelled r, 0 where r is no label), both uint32
    bits; with return_counts also counts int64 [4]: components with a triangle, unused vertices, invalid triangles, the largest
    component's triangles.  Device tensors; nothing synchronises."""
    tp, nt = _triangles(triangles)
    nv = int(n_vertices)
    dev = triangles.device
    label = torch.empty(nv, dtype=torch.int32, device=dev)
    count = torch.empty(nv, dtype=torch.int32, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev) if return_counts else None
    capi.check(capi.lib().dfusion_mesh_components(tp, nt, nv, _flat(label) if nv else None, _flat(count) if nv else None,
                                                  _flat(counts) if return_counts else None, _stream()), "dfusion_mesh_components")
    return (label, count, counts) if return_counts else (label, count)


def gather_rows(src, index, n=None):
    """src[index[:n]] for a contiguous tensor whose rows are 4, 12 or 16 bytes (index: int32, uint32 bits) -> a new tensor [n, ...]."""
    n = int(index.shape[0]) if n is None else int(n)
    if not src.is_contiguous():
        raise ValueError("per-vertex array must be contiguous (shape %s, strides %s)" % (tuple(src.shape), src.stride()))
    row = src.element_size()
    for d in src.shape[1:]:
        row *= int(d)
    if src.dim() < 1 or row not in (4, 12, 16):
        raise ValueError("per-vertex rows of %d bytes (%s %s), expected 4, 12 or 16" % (row, src.dtype, tuple(src.shape)))
    out = torch.empty((n,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    if n:
        capi.check(capi.lib().dfusion_gather_rows(_flat(src), row, _flat(index), n, _flat(out), _stream()), "dfusion_gather_rows")
    return out


def remove_small_components(vertices, triangles, min_triangles=0, keep_largest=False, attributes=()):
    """The mesh without the components of fewer than min_triangles triangles and -- with keep_largest -- without all but the one with
    the most (a tie: the smaller label); invalid triangles and the vertices no kept triangle uses go too, everything else keeps its
    order.  vertices [V, ...] and every tensor of `attributes` (per-vertex rows of 4, 12 or 16 bytes) are gathered with vertex_src.
    -> (vertices, triangles, attributes (a tuple), vertex_src int32 [n]: the old index of every new vertex).  One count-only filter
    call, then one of exactly that size (the counts are read back, as fetchMesh reads its own)."""
    tp, nt = _triangles(triangles)
    nv = int(vertices.shape[0])
    for a in attributes:
        if int(a.shape[0]) != nv:
            raise ValueError("attribute of %d rows for %d vertices" % (int(a.shape[0]), nv))
    dev = triangles.device
    label, count = mesh_components(triangles, nv)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    L = capi.lib()

    def run(kv, kt):
        tri_out = torch.empty((kt, 3), dtype=torch.int32, device=dev)
        src = torch.empty(kv, dtype=torch.int32, device=dev)
        capi.check(L.dfusion_mesh_filter(tp, nt, nv, _flat(label) if nv else None, _flat(count) if nv else None, int(min_triangles),
                                         1 if keep_largest else 0, _flat(tri_out) if kt else None, kt,
                                         _flat(src) if kv else None, kv, None, _flat(counts), _stream()), "dfusion_mesh_filter")
        return tri_out, src

    tri_out, src = _count_then_exact(run, counts)
    return gather_rows(vertices, src), tri_out, tuple(gather_rows(a, src) for a in attributes), src


KEEP_FIRST, KEEP_DUPLICATES = 1, 2                       # DF_SIMPLIFY_*


def simplify_mesh(vertices, triangles, cell, keep_first=False, keep_duplicates=False, return_counts=False):
    """The mesh simplified by vertex clustering on a grid of cubic cells of size `cell` (include/dfusion.h dfusion_mesh_simplify has the
    rule): the vertices of one cell that a valid triangle uses become one vertex -- their integer-averaged mean, with keep_first the
    lowest-index one of them as it is --, triangles with two corners in one cell collapse, and of the triangles over the same three
    cells one survives, or none where both orientations come equally often (a fin); keep_duplicates keeps every non-collapsed one.
    vertices float32 [V, 4], triangles int32 [T, 3] (uint32 bits) -> (vertices float32 [n, 4], triangles int32 [m, 3], vertex_src int32
    [n]: the lowest old index of every new vertex's cluster, vertex_map int32 [V]: the new index of every old vertex or 0xffffffff);
    with return_counts also counts int64 [8]: output vertices, output triangles, invalid, collapsed, fin and duplicate triangles,
    clusters, unclusterable vertices.  One count-only call, then one of exactly that size (the counts are read back)."""
    tp, nt = _triangles(triangles)
    nv = _mesh_vertices(vertices, triangles)
    dev = triangles.device
    flags = (KEEP_FIRST if keep_first else 0) | (KEEP_DUPLICATES if keep_duplicates else 0)
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    vmap = torch.full((nv,), -1, dtype=torch.int32, device=dev)             # nothing kept: every entry stays 0xffffffff
    L = capi.lib()

    def run(kv, kt):
        out_v = torch.empty((kv, 4), dtype=torch.float32, device=dev)
        out_t = torch.empty((kt, 3), dtype=torch.int32, device=dev)
        src = torch.empty(kv, dtype=torch.int32, device=dev)
        capi.check(L.dfusion_mesh_simplify(_flat(vertices) if nv else None, nv, tp, nt, float(cell), flags, _flat(out_v) if kv else None, kv,
                                           _flat(out_t) if kt else None, kt, _flat(src) if kv else None, _flat(vmap) if (kv or kt) and nv else None,
                                           _flat(counts), _stream()), "dfusion_mesh_simplify")
        return out_v, out_t, src

    out_v, out_t, src = _count_then_exact(run, counts)
    return (out_v, out_t, src, vmap, counts) if return_counts else (out_v, out_t, src, vmap)


FIX_BOUNDARY = 1                                         # DF_SMOOTH_FIX_BOUNDARY
TOPOLOGY_NAMES = ("csr_entries", "edges", "boundary_edges", "irregular_edges", "used_vertices", "invalid_triangles", "degenerate_triangles",
                  "open_vertices")


def mesh_adjacency(triangles, n_vertices, return_counts=False):
    """The vertex adjacency of an indexed mesh (include/dfusion.h dfusion_mesh_adjacency has the rule): triangles int32 [T, 3] (uint32
    bits) over n_vertices vertices -> (row_start int32 [V + 1], neighbours int32 [row_start[V]]: every vertex's neighbours, each once,
    ascending (uint32 bits both), vertex_class uint8 [V]: 0 no neighbour, 1 interior, 2 on a boundary edge, 3 on an irregular edge); with
    return_counts also counts int64 [8]: CSR entries, edges, boundary and irregular edges, vertices with a neighbour, invalid and
    degenerate triangles, vertices of class 2 or 3.  One call with a capacity of 6 T, trimmed from one read-back of the counts."""
    tp, nt = _triangles(triangles)
    nv = int(n_vertices)
    dev = triangles.device
    row_start = torch.empty(nv + 1, dtype=torch.int32, device=dev)
    neighbours = torch.empty(6 * nt, dtype=torch.int32, device=dev)
    vertex_class = torch.empty(nv, dtype=torch.uint8, device=dev)
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    capi.check(capi.lib().dfusion_mesh_adjacency(tp, nt, nv, _flat(row_start), _flat(neighbours) if nt else None, 6 * nt,
                                                 _flat(vertex_class) if nv else None, _flat(counts), _stream()), "dfusion_mesh_adjacency")
    neighbours = neighbours[:int(counts[0])]
    return (row_start, neighbours, vertex_class, counts) if return_counts else (row_start, neighbours, vertex_class)


def mesh_topology(triangles, n_vertices):
    """-> dict of dfusion_mesh_adjacency's eight counts (TOPOLOGY_NAMES) plus `euler`, the Euler characteristic used_vertices - edges +
    valid triangles (of a mesh without degenerate triangles).  A count-only call; the counts are read back."""
    tp, nt = _triangles(triangles)
    counts = torch.empty(8, dtype=torch.int64, device=triangles.device)
    capi.check(capi.lib().dfusion_mesh_adjacency(tp, nt, int(n_vertices), None, None, 0, None, _flat(counts), _stream()), "dfusion_mesh_adjacency")
    out = dict(zip(TOPOLOGY_NAMES, (int(c) for c in counts.tolist())))
    out["euler"] = out["used_vertices"] - out["edges"] + (nt - out["invalid_triangles"])
    return out


LOOP_COUNT_NAMES = ("loops", "loop_vertices", "boundary_half_edges", "other_boundary_vertices", "chain_vertices", "longest_loop",
                    "invalid_triangles", "degenerate_triangles")
FILL_COUNT_NAMES = ("vertices", "triangles", "loops_filled", "loops_open", "triangles_added", "longest_filled", "longest_open", "chain_vertices")


def boundary_loops(triangles, n_vertices, return_counts=False):
    """The closed loops of boundary half-edges of an indexed mesh (include/dfusion.h dfusion_mesh_boundary_loops has the rule): triangles
    int32 [T, 3] (uint32 bits) over n_vertices vertices -> (vertex_next int32 [V]: the head of a simple vertex's one outgoing boundary
    half-edge, vertex_loop int32 [V]: the smallest vertex index of the vertex's loop, vertex_rank int32 [V]: its steps from there --
    0xffffffff each where there is none --, loop_start int32 [loops + 1], loop_vertices int32 [loop_start[-1]]: the loops in ascending
    label, each from its label vertex along next; uint32 bits all); with return_counts also counts int64 [8] (LOOP_COUNT_NAMES).  One
    call with capacities of V, trimmed from one read-back of the counts."""
    tp, nt = _triangles(triangles)
    nv = int(n_vertices)
    dev = triangles.device
    nxt = torch.empty(nv, dtype=torch.int32, device=dev)
    loop = torch.empty(nv, dtype=torch.int32, device=dev)
    rank = torch.empty(nv, dtype=torch.int32, device=dev)
    start = torch.zeros(nv + 1, dtype=torch.int32, device=dev)
    members = torch.empty(nv, dtype=torch.int32, device=dev)
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    capi.check(capi.lib().dfusion_mesh_boundary_loops(tp, nt, nv, _flat(nxt) if nv else None, _flat(loop) if nv else None, _flat(rank) if nv else None,
                                                      _flat(start), nv, _flat(members) if nv else None, nv, _flat(counts), _stream()),
               "dfusion_mesh_boundary_loops")
    n_loops, n_members = (int(c) for c in counts[:2].tolist())
    start, members = start[:n_loops + 1], members[:n_members]
    return (nxt, loop, rank, start, members, counts) if return_counts else (nxt, loop, rank, start, members)


def fill_holes(vertices, triangles, max_edges, return_counts=False):
    """The mesh with every boundary loop of at most max_edges edges closed by a fan around its centroid (include/dfusion.h
    dfusion_mesh_fill_holes has the rule).  vertices float32 [V, 4], triangles int32 [T, 3] (uint32 bits) -> (vertices float32 [V + F, 4]:
    the old ones as they are, then one per filled loop, triangles int32 [T + A, 3]: the old ones, then the fans, vertex_src int32
    [V + F]: i for an old vertex, 0xffffffff for a new one, which has no source row); with return_counts also counts int64 [8]
    (FILL_COUNT_NAMES).  One count-only call, then one of exactly that size (the counts are read back)."""
    tp, nt = _triangles(triangles)
    nv = _mesh_vertices(vertices, triangles)
    if not 0 <= int(max_edges) <= 0xffffffff:
        raise ValueError("max_edges %r, expected 0 .. 2^32 - 1" % (max_edges,))
    dev = triangles.device
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    L = capi.lib()

    def run(kv, kt):
        out_v = torch.empty((kv, 4), dtype=torch.float32, device=dev)
        out_t = torch.empty((kt, 3), dtype=torch.int32, device=dev)
        src = torch.empty(kv, dtype=torch.int32, device=dev)
        capi.check(L.dfusion_mesh_fill_holes(_flat(vertices) if nv else None, nv, tp, nt, int(max_edges), 0, _flat(out_v) if kv else None, kv,
                                             _flat(out_t) if kt else None, kt, _flat(src) if kv else None, _flat(counts), _stream()),
                   "dfusion_mesh_fill_holes")
        return out_v, out_t, src

    out_v, out_t, src = _count_then_exact(run, counts)
    return (out_v, out_t, src, counts) if return_counts else (out_v, out_t, src)


def smooth_mesh(vertices, triangles, iterations=10, lam=0.5, mu=-0.53, fix_boundary=True, adjacency=None):
    """Taubin's lambda | mu smoothing (include/dfusion.h dfusion_mesh_smooth has the rule): every iteration moves each vertex by lam
    towards the mean of its neighbours and then, unless mu == 0, by mu (negative: away again, which undoes the shrinkage) on the
    result; with fix_boundary only the vertices of class 1 move.  vertices float32 [V, 4], triangles int32 [T, 3] (uint32 bits) -> new
    vertices float32 [V, 4]; the triangles stay as they are.  adjacency: mesh_adjacency's (row_start, neighbours, vertex_class) of
    this mesh, built here when None.  Nothing synchronises when an adjacency is given."""
    nv = _mesh_vertices(vertices, triangles)
    row_start, neighbours, vertex_class = mesh_adjacency(triangles, nv) if adjacency is None else adjacency[:3]
    if int(row_start.shape[0]) != nv + 1 or (vertex_class is not None and int(vertex_class.shape[0]) != nv):
        raise ValueError("adjacency of %d vertices for %d vertices" % (int(row_start.shape[0]) - 1, nv))
    nn = int(neighbours.shape[0])
    out = torch.empty_like(vertices)
    capi.check(capi.lib().dfusion_mesh_smooth(_flat(vertices) if nv else None, nv, _flat(row_start), _flat(neighbours) if nn else None, nn,
                                              _flat(vertex_class) if vertex_class is not None and nv else None, int(iterations), float(lam), float(mu),
                                              FIX_BOUNDARY if fix_boundary else 0, _flat(out) if nv else None, _stream()), "dfusion_mesh_smooth")
    return out


CLOSEST_COUNT_NAMES = ("answered", "unanswered", "eligible_triangles", "skipped_triangles", "max_d2_bits", "max_query", "triangle_tests",
                       "nodes_visited")


def closest_points(vertices, triangles, points, max_distance=None, return_barycentric=False, return_counts=False):
    """For every query point the nearest eligible triangle of the mesh and the closest point on it (include/dfusion.h
    dfusion_mesh_closest_points has the rule; a linear BVH is built inside the call).  vertices float32 [V, 4], triangles int32 [T, 3]
    (uint32 bits), points float32 [Q, 4] (w ignored), max_distance None (no limit) or a distance whose f32 square is max_dist2 ->
    (triangle int32 [Q] (uint32 bits; 0xffffffff without a winner), point float32 [Q, 4]: x, y, z and the squared distance); with
    return_barycentric also bary float32 [Q, 4] (u, v, w, 0); with return_counts also counts int64 [8] (CLOSEST_COUNT_NAMES).
    Nothing synchronises."""
    tp, nt = _triangles(triangles)
    nv, nq = _points4(vertices, "vertices"), _points4(points, "points")
    if vertices.device != triangles.device or points.device != triangles.device:
        raise ValueError("vertices on %s, triangles on %s, points on %s" % (vertices.device, triangles.device, points.device))
    if max_distance is None:
        max_d2 = float("inf")
    else:
        d = torch.tensor(float(max_distance), dtype=torch.float32)
        max_d2 = float(d * d)                                            # the f32 product
    dev = triangles.device
    tri = torch.empty(nq, dtype=torch.int32, device=dev)
    point = torch.empty((nq, 4), dtype=torch.float32, device=dev)
    bary = torch.empty((nq, 4), dtype=torch.float32, device=dev) if return_barycentric else None
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    capi.check(capi.lib().dfusion_mesh_closest_points(_flat(vertices) if nv else None, nv, tp, nt, _flat(points) if nq else None, nq, max_d2,
                                                      _flat(tri) if nq else None, _flat(point) if nq else None,
                                                      _flat(bary) if return_barycentric and nq else None, _flat(counts), _stream()),
               "dfusion_mesh_closest_points")
    return (tri, point) + ((bary,) if return_barycentric else ()) + ((counts,) if return_counts else ())


def _one_sided(vertices_a, vertices_b, triangles_b):
    tri, point, counts = closest_points(vertices_b, triangles_b, vertices_a, return_counts=True)
    d2 = torch.where(tri != -1, point[:, 3].double(), torch.zeros((), dtype=torch.float64, device=point.device))      # f64 sums on the device
    sums = torch.stack([d2.sqrt().sum(), d2.sum()])
    c = [int(x) for x in counts.tolist()]                                # the one read-back
    s_d, s_d2 = (float(x) for x in sums.tolist())
    n = c[0]
    max_d = math.sqrt(struct.unpack("<f", struct.pack("<I", c[4]))[0]) if n else 0.0      # the f64 root of the largest f32 d2
    return {"answered": n, "unanswered": c[1], "max": max_d, "max_vertex": c[5] if n else None,
            "mean": s_d / n if n else 0.0, "rms": math.sqrt(s_d2 / n) if n else 0.0}


def mesh_distance(vertices_a, triangles_a, vertices_b, triangles_b):
    """The distances between two meshes, sampled at the given vertices: -> dict with "a_to_b" (every vertex of A against mesh B) and
    "b_to_a", each a dict of answered / unanswered (the vertices with and without a closest point), max (the largest distance, from
    the call's counts) with max_vertex (the smallest index that attains it), mean and rms over the answered vertices (f64 reductions of
    the returned squared distances on the device), and "hausdorff", the larger of the two maxima.  Every vertex of the arrays is a
    sample, used by a triangle or not.  Two closest_points calls; their counts are read back."""
    ab = _one_sided(vertices_a, vertices_b, triangles_b)
    ba = _one_sided(vertices_b, vertices_a, triangles_a)
    return {"a_to_b": ab, "b_to_a": ba, "hausdorff": max(ab["max"], ba["max"])}


RAYS_ANY_HIT = 1                                         # DF_RAYS_ANY_HIT
RAY_COUNT_NAMES = ("hits", "misses", "eligible_triangles", "skipped_triangles", "invalid_rays", "reserved", "triangle_tests", "nodes_visited")


def ray_hits(vertices, triangles, origins, directions, t_min=0.0, t_max=None, any_hit=False, return_barycentric=False, return_counts=False):
    """For every ray o + t d, t in [t_min, t_max], the first eligible triangle of the mesh that it hits (include/dfusion.h
    dfusion_mesh_ray_hits has the rule; a linear BVH is built inside the call).  vertices float32 [V, 4], triangles int32 [T, 3] (uint32
    bits), origins and directions float32 [R, 4] (w ignored; d is used as given, t is in units of d), t_max None: no limit ->
    (triangle int32 [R] (uint32 bits; 0xffffffff without a hit), hit float32 [R, 4]: x, y, z and t); with return_barycentric also bary
    float32 [R, 4] (1 - u - v, u, v, side: +1 where the ray meets the face whose corners it sees run counter-clockwise, else -1); with
    return_counts also counts int64 [8] (RAY_COUNT_NAMES).  any_hit: only (triangle,) -- 0 where the ray hits anything, else 0xffffffff
    -- and the counts on request; the walk stops at the first hit.  Nothing synchronises."""
    tp, nt = _triangles(triangles)
    nv, nr = _points4(vertices, "vertices"), _points4(origins, "origins")
    if _points4(directions, "directions") != nr:
        raise ValueError("%d origins, %d directions" % (nr, int(directions.shape[0])))
    if vertices.device != triangles.device or origins.device != triangles.device or directions.device != triangles.device:
        raise ValueError("vertices on %s, triangles on %s, origins on %s, directions on %s" % (vertices.device, triangles.device, origins.device,
                                                                                             directions.device))
    if any_hit and return_barycentric:
        raise ValueError("any_hit gives no barycentrics")
    dev = triangles.device
    tri = torch.empty(nr, dtype=torch.int32, device=dev)
    hit = None if any_hit else torch.empty((nr, 4), dtype=torch.float32, device=dev)
    bary = torch.empty((nr, 4), dtype=torch.float32, device=dev) if return_barycentric else None
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    capi.check(capi.lib().dfusion_mesh_ray_hits(_flat(vertices) if nv else None, nv, tp, nt, _flat(origins) if nr else None,
                                                _flat(directions) if nr else None, nr, float(t_min), float("inf") if t_max is None else float(t_max),
                                                RAYS_ANY_HIT if any_hit else 0, _flat(tri) if nr else None, _flat(hit) if hit is not None and nr else None,
                                                _flat(bary) if return_barycentric and nr else None, _flat(counts), _stream()), "dfusion_mesh_ray_hits")
    return (tri,) + (() if any_hit else (hit,)) + ((bary,) if return_barycentric else ()) + ((counts,) if return_counts else ())


def visible_points(vertices, triangles, points, eye, margin=2.0 ** -10):
    """bool [N]: which of `points` (float32 [N, 4], w ignored) the eye sees: the segment from the eye to the point p, as the ray o = eye,
    d = p - eye (one f32 subtraction) on [0, 1 - margin] (the f32 difference), hits no triangle of the mesh (an any-hit ray_hits).
    `margin` is the share of the segment in front of p that is not looked at -- a point of the surface itself is not hidden by its
    own triangles --, a parameter of the query and no tolerance.  A point with a non-finite coordinate is not visible.  eye: three
    numbers, or a tensor of three.  Nothing synchronises."""
    n = _points4(points, "points")
    e = torch.as_tensor(eye, dtype=torch.float32).reshape(-1)[:3].to(points.device)
    o = torch.zeros_like(points)
    o[:, :3] = e
    d = points - o
    t_max = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(float(margin), dtype=torch.float32))      # on the host
    tri, = ray_hits(vertices, triangles, o, d, 0.0, t_max, any_hit=True)
    return (tri == -1) & torch.isfinite(points[:, :3]).all(1) if n else torch.zeros(0, dtype=torch.bool, device=points.device)
