// kfusion/cuda/mesh_ops.hpp -- kfusion::cuda::meshComponents / removeSmallComponents: the connected components of an indexed triangle
// mesh and the mesh without its small pieces (no reference counterpart).  Forward to dfusion_mesh_components / dfusion_mesh_filter /
// dfusion_gather_rows of include/dfusion.h, where the rule is stated; no kernels of their own.  simplifyMesh: the mesh simplified by
// vertex clustering (dfusion_mesh_simplify).  meshAdjacency / smoothMesh: the vertex adjacency with the edge statistics and Taubin
// smoothing over it (dfusion_mesh_adjacency / dfusion_mesh_smooth).  boundaryLoops / fillHoles: the closed loops of boundary half-edges
// and the mesh with the small ones filled (dfusion_mesh_boundary_loops / dfusion_mesh_fill_holes).  closestPoints / meshDistance: the
// closest point of a mesh to every query point and the distances between two meshes (dfusion_mesh_closest_points).  rayHits /
// visiblePoints: what every ray hits first on a mesh and which points an eye sees (dfusion_mesh_ray_hits).  Same calls as the Python mirror
// (dynamicfusion_amd.mesh_ops).
#pragma once
#include <vector>
#include <kfusion/types.hpp>

namespace kfusion { namespace cuda {

/// triangles: 3 vertex indices each (TsdfVolume::fetchMesh's) over n_vertices vertices.  vertex_label[v] = the smallest vertex index of
/// v's component, triangle_count[r] = the valid triangles of the component labelled r (0 where r is no label); counts (optional, 4
/// values): components with a triangle, unused vertices, invalid triangles, the largest component's triangles.  Enqueued only: nothing
/// synchronises.
void meshComponents(const DeviceArray<int>& triangles, size_t n_vertices, DeviceArray<int>& vertex_label, DeviceArray<int>& triangle_count,
                    DeviceArray<unsigned long long>* counts = nullptr);

/// The mesh without the components of fewer than min_triangles triangles and -- with keep_largest -- without all but the one with the
/// most; invalid triangles and the vertices no kept triangle uses go too, everything else keeps its order.  vertex_src[i] = the old
/// index of new vertex i.  Every array is sized exactly (a count-only filter call whose counts are read back, then one of that size).
void removeSmallComponents(const DeviceArray<Point>& vertices, const DeviceArray<int>& triangles, unsigned long long min_triangles,
                           bool keep_largest, DeviceArray<Point>& vertices_out, DeviceArray<int>& triangles_out, DeviceArray<int>& vertex_src);

/// out[i] = src[index[i]] for per-vertex rows of 16 bytes (normals, points) or 4 bytes (colours): the attributes of a filtered mesh.
void gatherRows(const DeviceArray<Point>& src, const DeviceArray<int>& index, DeviceArray<Point>& out);
void gatherRows(const DeviceArray<RGB>& src, const DeviceArray<int>& index, DeviceArray<RGB>& out);

/// The mesh simplified by vertex clustering on a grid of cubic cells of size `cell` (> 0, finite): the vertices of one cell become one
/// -- their integer-averaged mean, with DF_SIMPLIFY_KEEP_FIRST the lowest-index one as it is --, triangles with two corners in a cell
/// collapse, and of the triangles over the same three cells one survives, or none where both orientations come equally often
/// (DF_SIMPLIFY_KEEP_DUPLICATES keeps them all).  vertex_src[j] = the lowest old index of new vertex j's cluster; counts (optional): the
/// call's 8 counts.  Every array is sized exactly (a count-only call whose counts are read back, then one of that size).
void simplifyMesh(const DeviceArray<Point>& vertices, const DeviceArray<int>& triangles, float cell, unsigned int flags,
                  DeviceArray<Point>& out_vertices, DeviceArray<int>& out_triangles, DeviceArray<int>& vertex_src,
                  DeviceArray<unsigned long long>* counts = nullptr);

/// The vertex adjacency of a mesh over n_vertices vertices: row v of `neighbours`, [row_start[v], row_start[v + 1]), holds v's
/// neighbours, each once, ascending; vertex_class[v] = 0 no neighbour, 1 interior, 2 on a boundary edge, 3 on an irregular edge (used
/// three or more times, or twice in the same direction); counts (optional): the call's 8 counts -- CSR entries, edges, boundary and
/// irregular edges, vertices with a neighbour, invalid and degenerate triangles, vertices of class 2 or 3.  One call with a capacity of
/// 6 T, trimmed from one read-back of the counts.
void meshAdjacency(const DeviceArray<int>& triangles, size_t n_vertices, DeviceArray<int>& row_start, DeviceArray<int>& neighbours,
                   DeviceArray<unsigned char>& vertex_class, DeviceArray<unsigned long long>* counts = nullptr);

/// `iterations` of Taubin's lambda | mu smoothing (a step with lambda towards the mean of the neighbours, then unless mu == 0 a step with
/// mu on its result) over a meshAdjacency; with DF_SMOOTH_FIX_BOUNDARY only the vertices of class 1 move.  out_vertices may be
/// `vertices` itself.  Nothing synchronises.
void smoothMesh(const DeviceArray<Point>& vertices, const DeviceArray<int>& row_start, const DeviceArray<int>& neighbours,
                const DeviceArray<unsigned char>& vertex_class, int iterations, float lambda, float mu, unsigned int flags,
                DeviceArray<Point>& out_vertices);
/// The same, building the adjacency of `triangles` first.
void smoothMesh(const DeviceArray<Point>& vertices, const DeviceArray<int>& triangles, int iterations, float lambda, float mu, unsigned int flags,
                DeviceArray<Point>& out_vertices);

/// The closed loops of boundary half-edges of a mesh over n_vertices vertices: vertex_next[v] = the head of a simple vertex's one
/// outgoing boundary half-edge, vertex_loop[v] = the smallest vertex index of v's loop, vertex_rank[v] = its steps from there
/// (0xffffffff each where there is none); loop i holds loop_vertices[loop_start[i] .. loop_start[i + 1]), from its label vertex along
/// next, the loops in ascending label; counts (optional): the call's 8 counts -- loops, vertices on loops, boundary half-edges, other
/// boundary vertices, simple vertices on open chains, the longest loop, invalid and degenerate triangles.  One call with capacities of
/// V, trimmed from one read-back of the counts.
void boundaryLoops(const DeviceArray<int>& triangles, size_t n_vertices, DeviceArray<int>& vertex_next, DeviceArray<int>& vertex_loop,
                   DeviceArray<int>& vertex_rank, DeviceArray<int>& loop_start, DeviceArray<int>& loop_vertices,
                   DeviceArray<unsigned long long>* counts = nullptr);

/// The mesh with every boundary loop of at most max_edges edges closed by a fan around a new vertex at its centroid: the old vertices
/// and triangles as they are, then one vertex per filled loop and its L triangles, in ascending label.  vertex_src[i] = i for an old
/// vertex, 0xffffffff for a new one (it has no source row); counts (optional): the call's 8 counts.  Every array is sized exactly (a
/// count-only call whose counts are read back, then one of that size).
void fillHoles(const DeviceArray<Point>& vertices, const DeviceArray<int>& triangles, unsigned int max_edges, DeviceArray<Point>& out_vertices,
               DeviceArray<int>& out_triangles, DeviceArray<int>& vertex_src, DeviceArray<unsigned long long>* counts = nullptr);

/// For every query point (w ignored) the nearest eligible triangle of the mesh and the closest point on it, through a BVH built inside
/// the call: triangle[q] = its index (0xffffffff without a winner: no eligible triangle, a non-finite query, nothing within max_dist2),
/// point[q] = (x, y, z, squared distance); bary (optional) = (u, v, w, 0); counts (optional): the call's 8 counts.  max_dist2: the
/// largest admissible squared distance, +infinity for no limit.  Enqueued only when `counts` is given; without it the call's own counts
/// array is freed on return, so the stream is waited for.
void closestPoints(const DeviceArray<Point>& vertices, const DeviceArray<int>& triangles, const DeviceArray<Point>& points, float max_dist2,
                   DeviceArray<int>& triangle, DeviceArray<Point>& point, DeviceArray<Point>* bary = nullptr,
                   DeviceArray<unsigned long long>* counts = nullptr);

/// One direction of meshDistance: the samples with and without a closest point, the largest distance with the smallest sample index that
/// attains it (from the call's counts; -1 if none), and the mean and RMS distance over the answered samples.
struct MeshDistanceSide { unsigned long long answered, unanswered; double max; long long max_vertex; double mean, rms; };
struct MeshDistance { MeshDistanceSide a_to_b, b_to_a; double hausdorff; };

/// The distances between two meshes sampled at their vertices (every vertex of the arrays, used or not): A's against mesh B, B's against
/// mesh A, and the larger of the two maxima.  Two closestPoints calls; their counts and squared distances are read back, and mean and
/// RMS are double sums over them on the host, in index order.
MeshDistance meshDistance(const DeviceArray<Point>& vertices_a, const DeviceArray<int>& triangles_a, const DeviceArray<Point>& vertices_b,
                          const DeviceArray<int>& triangles_b);

/// For every ray origins[r] + t directions[r] (w ignored; the direction is used as given, t is in its units), t in [t_min, t_max], the
/// first eligible triangle of the mesh that it hits, through a BVH built inside the call: triangle[r] = its index (0xffffffff without a
/// hit), hit[r] = (x, y, z, t); bary (optional) = (1 - u - v, u, v, side); counts (optional): the call's 8 counts.  With
/// DF_RAYS_ANY_HIT in `flags` triangle[r] is 0 where the ray hits anything, `hit` is left alone and `bary` must be null.  Enqueued only
/// when `counts` is given; without it the call's own counts array is freed on return, so the stream is waited for.
void rayHits(const DeviceArray<Point>& vertices, const DeviceArray<int>& triangles, const DeviceArray<Point>& origins,
             const DeviceArray<Point>& directions, float t_min, float t_max, unsigned int flags, DeviceArray<int>& triangle, DeviceArray<Point>& hit,
             DeviceArray<Point>* bary = nullptr, DeviceArray<unsigned long long>* counts = nullptr);

/// visible[i] = 1 iff the eye sees points[i]: the ray o = eye, d = p - eye (one f32 subtraction, on the host) on [0, 1 - margin] hits
/// nothing of the mesh (one any-hit rayHits) and p is finite.  `margin`: the share of the segment in front of p that is not looked at.
/// The points are read back and the rays uploaded: the mirror has no kernels of its own.
void visiblePoints(const DeviceArray<Point>& vertices, const DeviceArray<int>& triangles, const DeviceArray<Point>& points, const float eye[3],
                   float margin, std::vector<unsigned char>& visible);

} }
