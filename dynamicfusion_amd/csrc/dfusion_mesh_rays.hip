// dfusion_mesh_rays.hip -- dfusion_mesh_ray_hits: for every ray the first eligible triangle of an indexed mesh that it hits (or, with
// DF_RAYS_ANY_HIT, whether it hits any), the hit point, its parameter and barycentrics.  The rule is stated in include/dfusion.h and
// DESIGN.md section 29 and restated in numpy by tests/mesh_rays_ref.py (brute force over all triangles), against which every output is
// compared for equality.
//
// The tree is the one of dfusion_mesh_closest_points: df_mbv_build (dfusion_mesh_bvh.hip) runs the bounds, codes, sort, tree and boxes
// stages into this call's workspace; only the walk is new.
//
//   walk      one lane per ray: an iterative walk from the root.  At an internal node the slabs of both children are computed; the child
//             with the smaller entry parameter tn is taken first, a leaf child is tested at once, the farther internal child is pushed
//             (at most one entry per internal node of the current path: DF_MBV_STACK).  A subtree is pruned iff its box fails the slab
//             test or its tn is > the best t_hit so far (strictly, so an equal t_hit with a smaller index is still reached).
//
// Why no slack argument is needed.  The slab test of the triangle's OWN vertex box is part of the rule: a candidate is accepted only if
// that box passes, and its parameter is clamped into the box's [tn, tf].  Every operation of the slab test is monotone in the box (f32
// subtraction, addition and multiplication by a fixed factor round monotonically; the parallel axis is an interval test), so an
// ancestor's [tn, tf], as computed, contains the leaf's, as computed: t_hit >= tn_leaf >= tn_node.  The tree therefore only skips
// triangles that the brute force rejects or that cannot beat the best.
#include "dfusion_mesh_bvh.h"
#include <math.h>

#pragma clang fp contract(off)                       // the rule is single f32 operations in a written order; nothing here may fuse

struct DfMryArgs {
    DfMbvArgs m;                                             // the mesh, the tree, counts, out_t / out_p (hit) / out_b; m.Q = R rays
    const float4 *o, *d;
    float t_min, t_max;
    uint32_t any;
};

// The rule's minimum and maximum: fminf / fmaxf (a NaN operand is dropped) with the one case IEEE leaves open pinned -- of two equal
// operands, zeros of either sign included, the SECOND is returned.
__device__ __forceinline__ float mry_max(float a, float b) { return (b != b || a > b) ? a : b; }
__device__ __forceinline__ float mry_min(float a, float b) { return (b != b || a < b) ? a : b; }

struct MryRay { float ox, oy, oz, dx, dy, dz, ix, iy, iz, slack, t_min, t_max; bool px, py, pz; };

// One axis of the slab test on the grown interval [lo - slack, hi + slack]; false: the box fails.
__device__ __forceinline__ bool mry_axis(uint32_t klo, uint32_t khi, float o, float inv, bool parallel, float slack, float& tn, float& tf)
{
    const float lo = mbv_unkey(klo) - slack, hi = mbv_unkey(khi) + slack;
    if (parallel) return lo <= o && o <= hi;                  // no constraint on t
    const float a = (lo - o) * inv, b = (hi - o) * inv;
    tn = mry_max(tn, mry_min(a, b));
    tf = mry_min(tf, mry_max(a, b));
    return true;
}

// The slab test of a box (six keys) -> passes; [tn, tf] the ray's parameter interval inside the grown box and [t_min, t_max].
__device__ __forceinline__ bool mry_slab(const uint32_t* box, const MryRay& r, float& tn, float& tf)
{
    tn = __uint_as_float(0xff800000u); tf = __uint_as_float(0x7f800000u);
    if (!mry_axis(box[0], box[3], r.ox, r.ix, r.px, r.slack, tn, tf)) return false;
    if (!mry_axis(box[1], box[4], r.oy, r.iy, r.py, r.slack, tn, tf)) return false;
    if (!mry_axis(box[2], box[5], r.oz, r.iz, r.pz, r.slack, tn, tf)) return false;
    tn = mry_max(tn, r.t_min);
    tf = mry_min(tf, r.t_max);
    return tn <= tf;
}

__device__ __forceinline__ float mry_dot(float ax, float ay, float az, float bx, float by, float bz) { return ax * bx + ay * by + az * bz; }

struct MryBest { float t; uint32_t tri; float u, v, side; };

// Moeller-Trumbore, two-sided, on sorted leaf `leaf` whose box passed with [tn, tf]; -> the candidate was accepted and beat `best`.
__device__ __forceinline__ bool mry_test(const DfMbvArgs& a, size_t leaf, const MryRay& r, float tn, float tf, MryBest& best)
{
    const uint32_t t = (uint32_t)a.keys[leaf];
    const float4 A = a.P[a.tris[3 * (size_t)t]], B = a.P[a.tris[3 * (size_t)t + 1]], C = a.P[a.tris[3 * (size_t)t + 2]];
    const float e1x = B.x - A.x, e1y = B.y - A.y, e1z = B.z - A.z, e2x = C.x - A.x, e2y = C.y - A.y, e2z = C.z - A.z;
    const float px = r.dy * e2z - r.dz * e2y, py = r.dz * e2x - r.dx * e2z, pz = r.dx * e2y - r.dy * e2x;
    const float det = mry_dot(e1x, e1y, e1z, px, py, pz);
    const float inv = 1.0f / det;
    const float sx = r.ox - A.x, sy = r.oy - A.y, sz = r.oz - A.z;
    const float u = mry_dot(sx, sy, sz, px, py, pz) * inv;
    const float qx = sy * e1z - sz * e1y, qy = sz * e1x - sx * e1z, qz = sx * e1y - sy * e1x;
    const float v = mry_dot(r.dx, r.dy, r.dz, qx, qy, qz) * inv;
    const float tt = mry_dot(e2x, e2y, e2z, qx, qy, qz) * inv;
    if (!(det != 0.0f && u >= 0.0f && v >= 0.0f && u + v <= 1.0f && tt >= r.t_min && tt <= r.t_max)) return false;     // a NaN fails
    const float t_hit = mry_min(mry_max(tt, tn), tf);
    if (!(t_hit < best.t || (t_hit == best.t && t < best.tri))) return false;
    best.t = t_hit; best.tri = t; best.u = u; best.v = v; best.side = det > 0.0f ? 1.0f : -1.0f;
    return true;
}

__global__ __launch_bounds__(256) void df_mry_walk_kernel(const DfMryArgs g)
{
    const DfMbvArgs& a = g.m;
    const size_t E = (size_t)a.counts[2];
    unsigned long long n_hit = 0ull, n_miss = 0ull, n_invalid = 0ull, n_tests = 0ull, n_nodes = 0ull;
    float root_m = 0.0f;                                                 // the largest |coordinate| of any eligible triangle
    if (E) {
        const uint32_t* const rb = E == 1 ? a.box_l : a.box_i;
        for (int j = 0; j < 6; ++j) root_m = fmaxf(root_m, fabsf(mbv_unkey(rb[j])));
    }
    const float pinf = __uint_as_float(0x7f800000u), ninf = __uint_as_float(0xff800000u);
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < a.Q; q += (size_t)gridDim.x * 256) {
        const float4 o = g.o[q], d = g.d[q];
        MryBest best;
        best.t = g.t_max; best.tri = DF_MBV_NONE; best.u = best.v = best.side = 0.0f;
        bool found = false;                                              // any-hit: an accepted candidate ends the walk
        const bool valid = mbv_finite(o.x) && mbv_finite(o.y) && mbv_finite(o.z) && mbv_finite(d.x) && mbv_finite(d.y) && mbv_finite(d.z) &&
                           !(d.x == 0.0f && d.y == 0.0f && d.z == 0.0f);
        if (!valid) ++n_invalid;
        if (E && valid) {
            MryRay r;
            r.ox = o.x; r.oy = o.y; r.oz = o.z; r.dx = d.x; r.dy = d.y; r.dz = d.z;
            r.ix = 1.0f / d.x; r.iy = 1.0f / d.y; r.iz = 1.0f / d.z;
            r.px = r.ix == pinf || r.ix == ninf; r.py = r.iy == pinf || r.iy == ninf; r.pz = r.iz == pinf || r.iz == ninf;
            const float m = fmaxf(fmaxf(root_m, fabsf(o.x)), fmaxf(fabsf(o.y), fabsf(o.z)));
            r.slack = m * 0x1p-18f + 0x1p-126f;
            r.t_min = g.t_min; r.t_max = g.t_max;
            float tn, tf;
            if (E == 1) {
                if (mry_slab(a.box_l, r, tn, tf)) { ++n_tests; found = mry_test(a, 0, r, tn, tf, best); }
            } else {
                uint32_t stack[DF_MBV_STACK];
                int sp = 0;
                uint32_t node = 0u;
                for (;;) {                                               // `node` is an internal node that is not pruned
                    ++n_nodes;
                    const uint32_t s = a.split[node], f = a.flags[node];
                    uint32_t c0 = s, c1 = s + 1u;
                    bool leaf0 = (f & DF_MBV_LEFT_LEAF) != 0u, leaf1 = (f & DF_MBV_RIGHT_LEAF) != 0u;
                    float tn0, tf0, tn1, tf1;
                    bool ok0 = mry_slab((leaf0 ? a.box_l : a.box_i) + 6 * (size_t)c0, r, tn0, tf0);
                    bool ok1 = mry_slab((leaf1 ? a.box_l : a.box_i) + 6 * (size_t)c1, r, tn1, tf1);
                    if (ok1 && (!ok0 || tn1 < tn0)) {                    // nearer child first
                        const uint32_t c = c0; c0 = c1; c1 = c;
                        const bool l = leaf0; leaf0 = leaf1; leaf1 = l;
                        const bool k = ok0; ok0 = ok1; ok1 = k;
                        float x = tn0; tn0 = tn1; tn1 = x;
                        x = tf0; tf0 = tf1; tf1 = x;
                    }
                    bool descend = false;
                    uint32_t next = 0u;
                    if (ok0 && !(tn0 > best.t)) {
                        if (leaf0) { ++n_tests; found = mry_test(a, c0, r, tn0, tf0, best) && g.any; }
                        else { next = c0; descend = true; }
                    }
                    if (found) break;
                    if (ok1 && !(tn1 > best.t)) {                        // against the best the nearer leaf may just have set
                        if (leaf1) { ++n_tests; found = mry_test(a, c1, r, tn1, tf1, best) && g.any; }
                        else if (descend) { if (sp < DF_MBV_STACK) stack[sp++] = c1; }
                        else { next = c1; descend = true; }
                    }
                    if (found) break;
                    while (!descend && sp > 0) {                         // pop; the slab again, against the best of now
                        next = stack[--sp];
                        descend = mry_slab(a.box_i + 6 * (size_t)next, r, tn, tf) && !(tn > best.t);
                    }
                    if (!descend) break;
                    node = next;
                }
            }
        }
        const bool won = best.tri != DF_MBV_NONE;
        if (won) ++n_hit; else ++n_miss;
        a.out_t[q] = won && g.any ? 0u : best.tri;
        if (a.out_p) {
            const float nanf_ = __uint_as_float(0x7fc00000u);
            a.out_p[q] = won ? make_float4(o.x + d.x * best.t, o.y + d.y * best.t, o.z + d.z * best.t, best.t) : make_float4(nanf_, nanf_, nanf_, pinf);
        }
        if (a.out_b) a.out_b[q] = won ? make_float4((1.0f - best.u) - best.v, best.u, best.v, best.side) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    const int slot[5] = {0, 1, 4, 6, 7};
    const unsigned long long n[5] = {n_hit, n_miss, n_invalid, n_tests, n_nodes};
    df_mesh_block_add(a.counts, slot, n);
}

extern "C" int dfusion_mesh_ray_hits(const float* vertices_dev, unsigned long long n_vertices, const unsigned int* triangles_dev,
                                     unsigned long long n_triangles, const float* origins_dev, const float* directions_dev, unsigned long long n_rays,
                                     float t_min, float t_max, unsigned int flags, unsigned int* triangle_dev, float* hit_dev, float* bary_dev,
                                     unsigned long long* counts_dev, dfStream stream)
{
    if (n_vertices > 0xffffffffull || n_triangles > 0xffffffffull || n_rays > 0xffffffffull || !counts_dev) return DF_E_INVALID;
    if (flags & ~DF_RAYS_ANY_HIT) return DF_E_INVALID;
    const bool any = (flags & DF_RAYS_ANY_HIT) != 0u;
    if ((n_vertices && !vertices_dev) || (n_triangles && !triangles_dev)) return DF_E_INVALID;
    if (n_rays && (!origins_dev || !directions_dev || !triangle_dev || (!any && !hit_dev))) return DF_E_INVALID;
    if (any && (hit_dev || bary_dev)) return DF_E_INVALID;
    const size_t V = (size_t)n_vertices, T = (size_t)n_triangles, R = (size_t)n_rays;
    const struct { const void* p; size_t n; } outs[4] = {{triangle_dev, R * 4}, {hit_dev, R * 16}, {bary_dev, R * 16}, {counts_dev, 64}};
    for (const auto& o : outs)
        if (df_mesh_overlap(vertices_dev, V * 16, o.p, o.n) || df_mesh_overlap(triangles_dev, T * 12, o.p, o.n) || df_mesh_overlap(origins_dev, R * 16, o.p, o.n) ||
            df_mesh_overlap(directions_dev, R * 16, o.p, o.n))
            return DF_E_INVALID;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return DF_E_NO_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    DF_HIP(hipMemsetAsync(counts_dev, 0, 64, st));
    DfMryArgs g;
    memset(&g, 0, sizeof(g));
    g.m.V = V; g.m.T = T; g.m.Q = R;
    g.m.P = (const float4*)vertices_dev; g.m.tris = triangles_dev;
    g.m.counts = counts_dev; g.m.out_t = triangle_dev; g.m.out_p = (float4*)hit_dev; g.m.out_b = (float4*)bary_dev;
    g.o = (const float4*)origins_dev; g.d = (const float4*)directions_dev; g.t_min = t_min; g.t_max = t_max; g.any = any ? 1u : 0u;
    const dim3 wg(256), gr(df_mesh_blocks(R));
    if (!T) {                                                            // counts [2] stays 0: the walk indexes nothing of the tree
        if (R) { hipLaunchKernelGGL(df_mry_walk_kernel, gr, wg, 0, st, g); DF_LAUNCH_CHECK(); }
        return DF_OK;
    }
    DfMbvLayout l;
    DF_TRY(df_mbv_plan(T, st, &l));
    DfScratchHold hold(st, l.total);                                      // held until the last launch is enqueued
    if (!hold.entry) return (int)hipErrorOutOfMemory;
    DF_TRY(df_mbv_build(g.m, l, hold.mem, R != 0, st));
    if (R) { hipLaunchKernelGGL(df_mry_walk_kernel, gr, wg, 0, st, g); DF_LAUNCH_CHECK(); }
    return DF_OK;
}
