// dfusion_mesh_bvh.hip -- dfusion_mesh_closest_points: for every query point the nearest eligible triangle of an indexed mesh, the
// closest point on it, its squared distance and barycentrics.  The rule is stated in include/dfusion.h and DESIGN.md section 28 and
// restated in numpy by tests/mesh_closest_ref.py (brute force over all triangles), against which every output is compared for equality:
// the winner under a fixed f32 distance routine with ties to the smaller index does not depend on the tree, so the tree may only prune.
//
//   bounds    one lane per triangle: ELIGIBLE or skipped, counted; the box of the eligible centroids by integer atomicMin / atomicMax on
//             an order-preserving key of the float (one atomic per wave and word)
//   codes     one lane per triangle: the 30-bit Morton code of its centroid in that box; key = code << 32 | t, so keys are unique; a
//             skipped triangle gets the all-ones key and falls off the end of the sort
//   sort      one hipcub::DeviceRadixSort::SortKeys over the 64 bits
//   tree      Karras' construction over the E unique keys: one lane per internal node (E - 1 of them; node 0 is the root) finds its
//             range and its split; children g and g + 1 with a leaf flag each, and the parent of either child.  E == 0: nothing.
//             E == 1: no internal node, the one leaf has no parent
//   boxes     one lane per sorted leaf: its triangle's vertex box, then up the parents raising each ancestor's box by integer atomicMin /
//             atomicMax on the keys.  No lane waits for another and no box is read in this launch except through the value an atomic
//             returns: a lane stops early at an ancestor none of whose six words it changed (DESIGN section 28 proves that every
//             ancestor still ends with the union of its leaves).  The boxes are read by plain loads only in the NEXT launch
//   query     one lane per query: an iterative walk from the root, nearer child first, a subtree pruned iff its lower bound is > best
//             (strictly, so an equal distance with a smaller index is still reached); the bound carries the slack of DESIGN section 28
//   finish    one lane: counts [4] and [5] from the packed maximum
// Every grid is capped at DF_MESH_MAX_BLOCKS workgroups (524 288 lanes) and strides over its range with 64-bit indices.
// The stages bounds .. boxes are also what dfusion_mesh_ray_hits (dfusion_mesh_rays.hip) builds its tree with: df_mbv_plan and df_mbv_build
// below run them for both; what the two files share is declared in dfusion_mesh_bvh.h.
//
// The stack.  A key has 62 significant bits (30 of code, 32 of index; bits 63 and 62 are zero in every eligible key).  An internal node's
// keys share a prefix of d bits, 2 <= d <= 63 (two different keys differ somewhere), and a child's prefix is strictly longer than its
// parent's.  So a root-to-leaf path holds at most 62 internal nodes.  The walk pushes at most one entry (the farther child) per
// internal node on the current path and only internal nodes are ever pushed, so at most 62 entries are live: DF_MBV_STACK = 64.
#include <hipcub/hipcub.hpp>                          // the sort of the codes
#include "dfusion_mesh_bvh.h"
#include <math.h>

#pragma clang fp contract(off)                       // the routine is single f32 operations in a written order; nothing here may fuse

// ELIGIBLE: three indices < V (df_mesh_load tests them before anything is indexed), pairwise different, nine finite coordinates.
__device__ __forceinline__ bool mbv_eligible(const DfMbvArgs& a, size_t t, float4& A, float4& B, float4& C)
{
    uint32_t i[3];
    if (!df_mesh_load(a.tris, t, a.T, (uint32_t)a.V, i)) return false;   // (V < 2^32)
    if (i[0] == i[1] || i[1] == i[2] || i[0] == i[2]) return false;
    A = a.P[i[0]]; B = a.P[i[1]]; C = a.P[i[2]];
    return mbv_finite(A.x) && mbv_finite(A.y) && mbv_finite(A.z) && mbv_finite(B.x) && mbv_finite(B.y) && mbv_finite(B.z) &&
           mbv_finite(C.x) && mbv_finite(C.y) && mbv_finite(C.z);
}

__device__ __forceinline__ float mbv_centroid(float a, float b, float c) { return ((a + b) + c) / 3.0f; }

__global__ __launch_bounds__(256) void df_mbv_bounds_kernel(const DfMbvArgs a)
{
    unsigned long long n_el = 0ull, n_skip = 0ull;
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < a.T; t += (size_t)gridDim.x * 256) {
        float4 A, B, C;
        if (mbv_eligible(a, t, A, B, C)) {
            ++n_el;
            const uint32_t k[3] = {mbv_key(mbv_centroid(A.x, B.x, C.x)), mbv_key(mbv_centroid(A.y, B.y, C.y)), mbv_key(mbv_centroid(A.z, B.z, C.z))};
            for (int j = 0; j < 3; ++j) { lo[j] = k[j] < lo[j] ? k[j] : lo[j]; hi[j] = k[j] > hi[j] ? k[j] : hi[j]; }
        } else ++n_skip;
    }
    for (int j = 0; j < 3; ++j) {                                        // the wave's box by shuffles, one atomic per wave and word
        lo[j] = ~df_mesh_wave_max(~lo[j]);                               // (a minimum is the complement of the complements' maximum)
        hi[j] = df_mesh_wave_max(hi[j]);
        if ((threadIdx.x & 63) == 0 && lo[j] <= hi[j]) { atomicMin(&a.bounds[j], lo[j]); atomicMax(&a.bounds[4 + j], hi[j]); }
    }
    const int slot[2] = {2, 3};
    const unsigned long long n[2] = {n_el, n_skip};
    df_mesh_block_add(a.counts, slot, n);
}

// 10 bits -> every third bit of 30.
__device__ __forceinline__ uint32_t mbv_spread(uint32_t v)
{
    v = (v | (v << 16)) & 0x030000ffu; v = (v | (v << 8)) & 0x0300f00fu; v = (v | (v << 4)) & 0x030c30c3u; v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// The cell 0 .. 1023 of c in [lo, hi]; hi == lo (0 / 0), an infinite extent and every other NaN give cell 0.
__device__ __forceinline__ uint32_t mbv_cell(float c, float lo, float hi)
{
    const float s = ((c - lo) / (hi - lo)) * 1024.0f;
    return (uint32_t)fminf(fmaxf(s, 0.0f), 1023.0f);
}

__global__ __launch_bounds__(256) void df_mbv_codes_kernel(const DfMbvArgs a)
{
    const float lx = mbv_unkey(a.bounds[0]), ly = mbv_unkey(a.bounds[1]), lz = mbv_unkey(a.bounds[2]);
    const float hx = mbv_unkey(a.bounds[4]), hy = mbv_unkey(a.bounds[5]), hz = mbv_unkey(a.bounds[6]);
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < a.T; t += (size_t)gridDim.x * 256) {
        float4 A, B, C;
        unsigned long long key = ~0ull;
        if (mbv_eligible(a, t, A, B, C)) {
            const uint32_t code = mbv_spread(mbv_cell(mbv_centroid(A.x, B.x, C.x), lx, hx)) << 2 | mbv_spread(mbv_cell(mbv_centroid(A.y, B.y, C.y), ly, hy)) << 1 |
                                  mbv_spread(mbv_cell(mbv_centroid(A.z, B.z, C.z), lz, hz));
            key = (unsigned long long)code << 32 | (unsigned long long)t;
        }
        a.keys_in[t] = key;
    }
}

// The length of the common prefix of keys i and j, -1 where j is out of range.  Keys are unique, so the xor is never 0.
__device__ __forceinline__ int mbv_delta(const unsigned long long* k, long long i, long long j, long long E)
{
    if (j < 0 || j >= E) return -1;
    return __clzll((long long)(k[i] ^ k[j]));
}

__global__ __launch_bounds__(256) void df_mbv_tree_kernel(const DfMbvArgs a)
{
    const long long E = (long long)a.counts[2];
    if (E == 1 && blockIdx.x == 0 && threadIdx.x == 0) a.par_l[0] = DF_MBV_NONE;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < E - 1; i += (long long)gridDim.x * 256) {
        const unsigned long long* k = a.keys;
        const long long d = mbv_delta(k, i, i + 1, E) > mbv_delta(k, i, i - 1, E) ? 1 : -1;
        const int dmin = mbv_delta(k, i, i - d, E);
        long long lmax = 2;                                              // (at most 33 doublings: out of range gives -1 <= dmin)
        while (mbv_delta(k, i, i + lmax * d, E) > dmin) lmax *= 2;
        long long l = 0;
        for (long long s = lmax / 2; s >= 1; s /= 2)
            if (mbv_delta(k, i, i + (l + s) * d, E) > dmin) l += s;
        const long long j = i + l * d;
        const int dnode = mbv_delta(k, i, j, E);
        long long s = 0, step = l;
        do {
            step = (step + 1) >> 1;
            if (mbv_delta(k, i, i + (s + step) * d, E) > dnode) s += step;
        } while (step > 1);
        const long long g = i + s * d + (d < 0 ? -1 : 0), first = i < j ? i : j, last = i < j ? j : i;
        const bool left_leaf = first == g, right_leaf = last == g + 1;
        a.split[i] = (uint32_t)g;
        a.flags[i] = (uint8_t)((left_leaf ? DF_MBV_LEFT_LEAF : 0u) | (right_leaf ? DF_MBV_RIGHT_LEAF : 0u));
        (left_leaf ? a.par_l : a.par_i)[g] = (uint32_t)i;               // every node is the child of exactly one: no two lanes write a word
        (right_leaf ? a.par_l : a.par_i)[g + 1] = (uint32_t)i;
        if (i == 0) a.par_i[0] = DF_MBV_NONE;                            // the root is nobody's child
        uint32_t* const b = a.box_i + 6 * (size_t)i;                     // the empty box, raised in the next launch
        b[0] = b[1] = b[2] = 0xffffffffu; b[3] = b[4] = b[5] = 0u;
    }
}

__global__ __launch_bounds__(256) void df_mbv_boxes_kernel(const DfMbvArgs a)
{
    const size_t E = (size_t)a.counts[2];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < E; i += (size_t)gridDim.x * 256) {
        const size_t t = (size_t)(uint32_t)a.keys[i];
        const float4 A = a.P[a.tris[3 * t]], B = a.P[a.tris[3 * t + 1]], C = a.P[a.tris[3 * t + 2]];   // eligible, or it would not be among the first E
        const uint32_t lo[3] = {mbv_key(fminf(fminf(A.x, B.x), C.x)), mbv_key(fminf(fminf(A.y, B.y), C.y)), mbv_key(fminf(fminf(A.z, B.z), C.z))};
        const uint32_t hi[3] = {mbv_key(fmaxf(fmaxf(A.x, B.x), C.x)), mbv_key(fmaxf(fmaxf(A.y, B.y), C.y)), mbv_key(fmaxf(fmaxf(A.z, B.z), C.z))};
        uint32_t* const bl = a.box_l + 6 * i;
        for (int j = 0; j < 3; ++j) { bl[j] = lo[j]; bl[3 + j] = hi[j]; }
        uint32_t n = a.par_l[i];
        for (int up = 0; up < DF_MBV_STACK && n != DF_MBV_NONE; ++up) {  // at most 62 ancestors (the stack bound above)
            uint32_t* const b = a.box_i + 6 * (size_t)n;
            bool changed = false;
            for (int j = 0; j < 3; ++j) {
                changed |= lo[j] < atomicMin(&b[j], lo[j]);
                changed |= hi[j] > atomicMax(&b[3 + j], hi[j]);
            }
            if (!changed) break;                                         // those who wrote these six words go on upwards themselves
            n = a.par_i[n];
        }
    }
}

struct MbvHit { float v, w, x, y, z, d2; };

__device__ __forceinline__ float mbv_dot(float ax, float ay, float az, float bx, float by, float bz) { return ax * bx + ay * by + az * bz; }

// Ericson, Real-Time Collision Detection 5.1.5, in its order of tests; every line one f32 operation per result.
__device__ __forceinline__ MbvHit mbv_closest(float px, float py, float pz, const float4& A, const float4& B, const float4& C)
{
    const float abx = B.x - A.x, aby = B.y - A.y, abz = B.z - A.z, acx = C.x - A.x, acy = C.y - A.y, acz = C.z - A.z;
    const float apx = px - A.x, apy = py - A.y, apz = pz - A.z;
    const float d1 = mbv_dot(abx, aby, abz, apx, apy, apz), d2 = mbv_dot(acx, acy, acz, apx, apy, apz);
    const float bpx = px - B.x, bpy = py - B.y, bpz = pz - B.z;
    const float d3 = mbv_dot(abx, aby, abz, bpx, bpy, bpz), d4 = mbv_dot(acx, acy, acz, bpx, bpy, bpz);
    const float cpx = px - C.x, cpy = py - C.y, cpz = pz - C.z;
    const float d5 = mbv_dot(abx, aby, abz, cpx, cpy, cpz), d6 = mbv_dot(acx, acy, acz, cpx, cpy, cpz);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float e43 = d4 - d3, e56 = d5 - d6;
    float v, w;
    if (d1 <= 0.0f && d2 <= 0.0f) { v = 0.0f; w = 0.0f; }                                     // vertex A
    else if (d3 >= 0.0f && d4 <= d3) { v = 1.0f; w = 0.0f; }                                  // vertex B
    else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { v = d1 / (d1 - d3); w = 0.0f; }        // edge AB
    else if (d6 >= 0.0f && d5 <= d6) { v = 0.0f; w = 1.0f; }                                  // vertex C
    else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { v = 0.0f; w = d2 / (d2 - d6); }        // edge AC
    else if (va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f) { w = e43 / (e43 + e56); v = 1.0f - w; }   // edge BC
    else { const float denom = 1.0f / ((va + vb) + vc); v = vb * denom; w = vc * denom; }     // face (and every NaN)
    MbvHit h;
    h.v = v; h.w = w;
    h.x = (A.x + abx * v) + acx * w; h.y = (A.y + aby * v) + acy * w; h.z = (A.z + abz * v) + acz * w;
    const float dx = px - h.x, dy = py - h.y, dz = pz - h.z;
    h.d2 = mbv_dot(dx, dy, dz, dx, dy, dz);
    return h;
}

// A lower bound, as computed, of the d2 that mbv_closest computes for any triangle whose vertices lie in the box: the squared distance to
// the box grown by `slack` on every side, shrunk by 2^-19 of itself and 2^-120 for the roundings of both sums.
// fmaxf drops a NaN in favour of the other operand, so a NaN anywhere lowers the bound towards 0 and never prunes.
__device__ __forceinline__ float mbv_lower(const uint32_t* box, float px, float py, float pz, float slack)
{
    const float ex = fmaxf(fmaxf(mbv_unkey(box[0]) - px, px - mbv_unkey(box[3])) - slack, 0.0f);
    const float ey = fmaxf(fmaxf(mbv_unkey(box[1]) - py, py - mbv_unkey(box[4])) - slack, 0.0f);
    const float ez = fmaxf(fmaxf(mbv_unkey(box[2]) - pz, pz - mbv_unkey(box[5])) - slack, 0.0f);
    return fmaxf(mbv_dot(ex, ey, ez, ex, ey, ez) * (1.0f - 0x1p-19f) - 0x1p-120f, 0.0f);
}

struct MbvBest { float d2; uint32_t t; MbvHit h; };

__device__ __forceinline__ void mbv_test(const DfMbvArgs& a, size_t leaf, float px, float py, float pz, MbvBest& best)
{
    const uint32_t t = (uint32_t)a.keys[leaf];
    const float4 A = a.P[a.tris[3 * (size_t)t]], B = a.P[a.tris[3 * (size_t)t + 1]], C = a.P[a.tris[3 * (size_t)t + 2]];
    const MbvHit h = mbv_closest(px, py, pz, A, B, C);
    if (h.d2 < best.d2 || (h.d2 == best.d2 && t < best.t)) { best.d2 = h.d2; best.t = t; best.h = h; }      // a NaN d2 fails both
}

__global__ __launch_bounds__(256) void df_mbv_query_kernel(const DfMbvArgs a)
{
    __shared__ unsigned long long wg_top;
    if (threadIdx.x == 0) wg_top = 0ull;
    const size_t E = (size_t)a.counts[2];
    unsigned long long n_hit = 0ull, n_miss = 0ull, n_tests = 0ull, n_nodes = 0ull, top = 0ull;
    float root_m = 0.0f;                                                 // the largest |coordinate| of any eligible triangle
    if (E) {
        const uint32_t* const rb = E == 1 ? a.box_l : a.box_i;
        for (int j = 0; j < 6; ++j) root_m = fmaxf(root_m, fabsf(mbv_unkey(rb[j])));
    }
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < a.Q; q += (size_t)gridDim.x * 256) {
        const float4 p = a.q[q];
        MbvBest best;
        best.d2 = a.max_d2; best.t = DF_MBV_NONE;                        // admissible iff d2 <= max_d2: equal wins by the index, NaN never
        if (E && mbv_finite(p.x) && mbv_finite(p.y) && mbv_finite(p.z)) {
            const float m = fmaxf(fmaxf(root_m, fabsf(p.x)), fmaxf(fabsf(p.y), fabsf(p.z)));
            const float slack = m * 0x1p-18f + 0x1p-126f;
            if (E == 1) {
                ++n_tests;
                mbv_test(a, 0, p.x, p.y, p.z, best);
            } else {
                uint32_t stack[DF_MBV_STACK];
                int sp = 0;
                uint32_t node = 0u;
                for (;;) {                                               // `node` is an internal node that is not pruned
                    ++n_nodes;
                    const uint32_t g = a.split[node], f = a.flags[node];
                    uint32_t c0 = g, c1 = g + 1u;
                    bool leaf0 = (f & DF_MBV_LEFT_LEAF) != 0u, leaf1 = (f & DF_MBV_RIGHT_LEAF) != 0u;
                    float lb0 = mbv_lower((leaf0 ? a.box_l : a.box_i) + 6 * (size_t)c0, p.x, p.y, p.z, slack);
                    float lb1 = mbv_lower((leaf1 ? a.box_l : a.box_i) + 6 * (size_t)c1, p.x, p.y, p.z, slack);
                    if (lb1 < lb0) {                                     // nearer child first
                        const uint32_t c = c0; c0 = c1; c1 = c;
                        const bool l = leaf0; leaf0 = leaf1; leaf1 = l;
                        const float b = lb0; lb0 = lb1; lb1 = b;
                    }
                    bool descend = false;
                    uint32_t next = 0u;
                    if (!(lb0 > best.d2)) {
                        if (leaf0) { ++n_tests; mbv_test(a, c0, p.x, p.y, p.z, best); }
                        else { next = c0; descend = true; }
                    }
                    if (!(lb1 > best.d2)) {                              // against the best the nearer leaf may just have set
                        if (leaf1) { ++n_tests; mbv_test(a, c1, p.x, p.y, p.z, best); }
                        else if (descend) { if (sp < DF_MBV_STACK) stack[sp++] = c1; }
                        else { next = c1; descend = true; }
                    }
                    while (!descend && sp > 0) {                         // pop; the bound again, against the best of now
                        next = stack[--sp];
                        descend = !(mbv_lower(a.box_i + 6 * (size_t)next, p.x, p.y, p.z, slack) > best.d2);
                    }
                    if (!descend) break;
                    node = next;
                }
            }
        }
        const bool won = best.t != DF_MBV_NONE;
        if (won) {
            ++n_hit;
            const unsigned long long packed = (unsigned long long)__float_as_uint(best.d2) << 32 | (unsigned long long)(uint32_t)~(uint32_t)q;
            top = packed > top ? packed : top;
        } else ++n_miss;
        const float nanf_ = __uint_as_float(0x7fc00000u);
        a.out_t[q] = best.t;
        a.out_p[q] = won ? make_float4(best.h.x, best.h.y, best.h.z, best.d2) : make_float4(nanf_, nanf_, nanf_, __uint_as_float(0x7f800000u));
        if (a.out_b) a.out_b[q] = won ? make_float4((1.0f - best.h.v) - best.h.w, best.h.v, best.h.w, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    __syncthreads();
    if (top) atomicMax(&wg_top, top);
    const int slot[4] = {0, 1, 6, 7};
    const unsigned long long n[4] = {n_hit, n_miss, n_tests, n_nodes};
    df_mesh_block_add(a.counts, slot, n);                                // (synchronises: wg_top is complete behind it)
    if (threadIdx.x == 0 && wg_top) atomicMax(a.top, wg_top);
}

__global__ void df_mbv_finish_kernel(const unsigned long long* top, unsigned long long* counts)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const unsigned long long t = top ? *top : 0ull;                  // 0: no winner (a winner's ~q is never 0, q <= 2^32 - 2)
        counts[4] = t >> 32;
        counts[5] = t ? (unsigned long long)(uint32_t)~(uint32_t)t : 0xffffffffull;
    }
}

// No eligible triangle is known without a launch (T == 0): every query goes without a winner.
__global__ __launch_bounds__(256) void df_mbv_none_kernel(const DfMbvArgs a)
{
    const float nanf_ = __uint_as_float(0x7fc00000u);
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < a.Q; q += (size_t)gridDim.x * 256) {
        a.out_t[q] = DF_MBV_NONE;
        a.out_p[q] = make_float4(nanf_, nanf_, nanf_, __uint_as_float(0x7f800000u));
        if (a.out_b) a.out_b[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) a.counts[1] = (unsigned long long)a.Q;
}

int df_mbv_plan(size_t T, hipStream_t st, DfMbvLayout* l)
{
    l->cub_bytes = 0;
    DF_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, l->cub_bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, T, 0, 64, st));
    DfMeshCarve c; c.take(T * 8);                                         // (the keys as emitted, at the front)
    l->o_keys = c.take(T * 8); l->o_split = c.take(T * 4); l->o_flags = c.take(T); l->o_par_i = c.take(T * 4); l->o_par_l = c.take(T * 4);
    l->o_box_i = c.take(T * 24); l->o_box_l = c.take(T * 24); l->o_bounds = c.take(32); l->o_top = c.take(16);
    l->o_cub = c.take(l->cub_bytes, 256);
    l->total = c.total();
    return DF_OK;
}

int df_mbv_build(DfMbvArgs& a, const DfMbvLayout& l, char* ws, bool tree, hipStream_t st)
{
    a.keys_in = (unsigned long long*)ws; a.keys = (unsigned long long*)(ws + l.o_keys);
    a.split = (uint32_t*)(ws + l.o_split); a.flags = (uint8_t*)(ws + l.o_flags);
    a.par_i = (uint32_t*)(ws + l.o_par_i); a.par_l = (uint32_t*)(ws + l.o_par_l);
    a.box_i = (uint32_t*)(ws + l.o_box_i); a.box_l = (uint32_t*)(ws + l.o_box_l);
    a.bounds = (uint32_t*)(ws + l.o_bounds); a.top = (unsigned long long*)(ws + l.o_top);
    const dim3 wg(256), gt(df_mesh_blocks(a.T));
    DF_HIP(hipMemsetAsync(a.bounds, 0xff, 16, st));
    DF_HIP(hipMemsetAsync(a.bounds + 4, 0, 16 + 16, st));                 // the maxima and, behind them, top
    hipLaunchKernelGGL(df_mbv_bounds_kernel, gt, wg, 0, st, a);
    DF_LAUNCH_CHECK();
    if (!tree) return DF_OK;
    hipLaunchKernelGGL(df_mbv_codes_kernel, gt, wg, 0, st, a);
    DF_LAUNCH_CHECK();
    size_t cub_bytes = l.cub_bytes;
    DF_HIP(hipcub::DeviceRadixSort::SortKeys(ws + l.o_cub, cub_bytes, (const unsigned long long*)a.keys_in, a.keys, a.T, 0, 64, st));
    hipLaunchKernelGGL(df_mbv_tree_kernel, gt, wg, 0, st, a);
    DF_LAUNCH_CHECK();
    hipLaunchKernelGGL(df_mbv_boxes_kernel, gt, wg, 0, st, a);
    DF_LAUNCH_CHECK();
    return DF_OK;
}

extern "C" int dfusion_mesh_closest_points(const float* vertices_dev, unsigned long long n_vertices, const unsigned int* triangles_dev,
                                           unsigned long long n_triangles, const float* queries_dev, unsigned long long n_queries, float max_dist2,
                                           unsigned int* triangle_dev, float* point_dev, float* bary_dev, unsigned long long* counts_dev,
                                           dfStream stream)
{
    if (n_vertices > 0xffffffffull || n_triangles > 0xffffffffull || n_queries > 0xffffffffull || !counts_dev) return DF_E_INVALID;
    if ((n_vertices && !vertices_dev) || (n_triangles && !triangles_dev)) return DF_E_INVALID;
    if (n_queries && (!queries_dev || !triangle_dev || !point_dev)) return DF_E_INVALID;
    const size_t V = (size_t)n_vertices, T = (size_t)n_triangles, Q = (size_t)n_queries;
    const struct { const void* p; size_t n; } outs[4] = {{triangle_dev, Q * 4}, {point_dev, Q * 16}, {bary_dev, Q * 16}, {counts_dev, 64}};
    for (const auto& o : outs)
        if (df_mesh_overlap(vertices_dev, V * 16, o.p, o.n) || df_mesh_overlap(triangles_dev, T * 12, o.p, o.n) || df_mesh_overlap(queries_dev, Q * 16, o.p, o.n))
            return DF_E_INVALID;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return DF_E_NO_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    DF_HIP(hipMemsetAsync(counts_dev, 0, 64, st));
    DfMbvArgs a;
    memset(&a, 0, sizeof(a));
    a.V = V; a.T = T; a.Q = Q;
    a.P = (const float4*)vertices_dev; a.tris = triangles_dev; a.q = (const float4*)queries_dev; a.max_d2 = max_dist2;
    a.counts = counts_dev; a.out_t = triangle_dev; a.out_p = (float4*)point_dev; a.out_b = (float4*)bary_dev;
    const dim3 wg(256), gq(df_mesh_blocks(Q));
    if (!T) {
        if (Q) { hipLaunchKernelGGL(df_mbv_none_kernel, gq, wg, 0, st, a); DF_LAUNCH_CHECK(); }
        hipLaunchKernelGGL(df_mbv_finish_kernel, dim3(1), dim3(64), 0, st, (const unsigned long long*)nullptr, counts_dev);
        DF_LAUNCH_CHECK();
        return DF_OK;
    }
    DfMbvLayout l;
    DF_TRY(df_mbv_plan(T, st, &l));
    DfScratchHold hold(st, l.total);                                      // held until the last launch is enqueued
    if (!hold.entry) return (int)hipErrorOutOfMemory;
    DF_TRY(df_mbv_build(a, l, hold.mem, Q != 0, st));
    if (Q) {
        hipLaunchKernelGGL(df_mbv_query_kernel, gq, wg, 0, st, a);
        DF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(df_mbv_finish_kernel, dim3(1), dim3(64), 0, st, (const unsigned long long*)a.top, counts_dev);
    DF_LAUNCH_CHECK();
    return DF_OK;
}
