// dfusion_mesh_simplify.hip -- dfusion_mesh_simplify: an indexed triangle mesh (dfusion_extract_mesh's, or any) simplified by vertex
// clustering on a grid of cubic cells.  The rule -- which vertices cluster, the integer-averaged representative, which triangles are
// kept, collapsed, cancelled as fins or dropped as duplicates, and the order of everything -- is stated in include/dfusion.h and
// DESIGN.md section 23 and restated in numpy by tests/mesh_simplify_ref.py, against which every output is compared for equality.
// Integer atomics only; the one floating-point result, a position, is a function of integer sums.
//
//   mark      one lane per triangle: a flag of 1 on the three vertices of a valid triangle (members), of 2 on the unclusterable
//             vertices of a triangle whose indices are all < V; the invalid triangles counted
//   claim     one lane per member: its cell's slot in an open-addressing table.  A slot belongs to the first vertex index that takes it
//             by atomicCAS, its cell is that vertex's, recomputed from the read-only input (df_ext_claim_kernel's technique), so no key
//             is published beside the claim; per slot an integer atomicMin of the member index -- the cluster's src
//   sums      after the kernel boundary the minima are final: cluster[v] = src, and on the arrays indexed by src one 32-bit add of n
//             and three 64-bit adds of the 24-bit fractions; clusters and unclusterable vertices counted
//   classify  one lane per triangle: invalid, collapsed (counted), or -- its three clusters differ -- kept at once with
//             DF_SIMPLIFY_KEEP_DUPLICATES, else entered in a second table of the same kind, keyed by the first triangle index that took
//             the slot and compared by recomputing that triangle's ascending cluster triple: per slot |P| - |N| and the lowest
//             triangle index of either parity
//   decide    fin (|P| == |N|), the lowest index of the larger side (kept) or duplicate; a kept triangle flags itself and, at their
//             src, its three clusters
//   scan      df_mesh_scan_pair: two hipcub exclusive sums, in place, one spare element each for the total (the tail dfusion_mesh_filter has)
//   compact   triangles through cluster and the scanned offsets; one lane per vertex index: a used src writes vertex_src and its
//             position, every vertex its vertex_map -- the flags sit at the src indices, so the scan puts the clusters in src order
// Every grid is capped at DF_MESH_MAX_BLOCKS workgroups (524 288 lanes) and strides over its range with 64-bit indices.  The grid, the
// triangle load, the counting, the overlap test, the workspace carve and the scan tail are the mesh kit's (dfusion_mesh_kit.h).
#include "dfusion_mesh_kit.h"
#include <math.h>

#define DF_MSP_NONE 0xffffffffu
#define DF_MSP_CELL_LIM 1073741824.f                 // 2^30
#define DF_MSP_FLAGS (DF_SIMPLIFY_KEEP_FIRST | DF_SIMPLIFY_KEEP_DUPLICATES)

struct DfMspArgs {
    const float* vtx; uint32_t V;
    const uint32_t* tris; size_t T;
    float cell; unsigned flags;
    uint8_t* mark;                      // [V] 0, 1 member, 2 unclusterable and used by a triangle with its indices < V
    uint32_t* cluster;                  // [V] the slot, then the src of v's cluster; NONE for a non-member
    uint32_t* n;                        // [V] at src: the members
    unsigned long long* sum;            // [3 V] at src: S_a
    uint32_t *tscan, *vscan;            // [T + 1], [V + 1]: the slot / flags, then their exclusive sums
    uint32_t *vowner, *vmin; uint32_t vslots;      // the cell table
    uint32_t *towner, *tmin; int* tbal; uint32_t tslots;   // the group table (tmin: [2 tslots], even then odd)
    float* vtx_out; unsigned long long vcap;
    uint32_t* tris_out; unsigned long long tcap;
    uint32_t *vsrc, *vmap;
    unsigned long long* counts;
};

// t_a = p_a / cell (IEEE f32 division, -fno-fast-math), the cell floorf(t_a) and the fraction's 24 bits; false if v takes no part
__device__ __forceinline__ bool msp_cell(const float* __restrict__ vtx, uint32_t v, float cell, int (&c)[3], uint32_t (&q)[3])
{
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float t = vtx[4 * (size_t)v + a] / cell;
        ok = ok && fabsf(t) < DF_MSP_CELL_LIM;                           // (NaN and inf fail this too)
        const float fl = floorf(t);
        c[a] = ok ? (int)fl : 0;
        q[a] = ok ? (uint32_t)((t - fl) * 16777216.f) : 0u;              // t - fl in [0, 1]; the scaling is exact
    }
    return ok;
}

__device__ __forceinline__ bool msp_clusterable(const float* __restrict__ vtx, uint32_t v, float cell)
{
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) ok = ok && fabsf(vtx[4 * (size_t)v + a] / cell) < DF_MSP_CELL_LIM;
    return ok;
}

__device__ __forceinline__ uint32_t msp_hash(uint32_t a, uint32_t b, uint32_t c, uint32_t slots)
{
    uint32_t h = a * 73856093u ^ b * 19349663u ^ c * 83492791u;
    h = (h ^ (h >> 15)) * 0x2c1b3c6du;
    h = (h ^ (h >> 12)) * 0x297a2d39u;
    return (h ^ (h >> 15)) % slots;
}

__global__ __launch_bounds__(256) void df_msp_mark_kernel(const DfMspArgs a)
{
    unsigned long long n_invalid = 0ull;                                 // wave-uniform
    for (size_t t0 = (size_t)blockIdx.x * 256; t0 < a.T; t0 += (size_t)gridDim.x * 256) {      // (workgroup-uniform trip count)
        const size_t t = t0 + threadIdx.x;
        uint32_t i[3];
        const bool inb = df_mesh_load(a.tris, t, a.T, a.V, i);
        bool ok[3] = {false, false, false};
        if (inb) {
#pragma unroll
            for (int k = 0; k < 3; ++k) ok[k] = msp_clusterable(a.vtx, i[k], a.cell);
        }
        const bool valid = inb && ok[0] && ok[1] && ok[2];
        if (inb) {
            // a vertex is clusterable or it is not: every lane that writes mark[v] writes the same value
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (valid) a.mark[i[k]] = 1;
                else if (!ok[k]) a.mark[i[k]] = 2;
            }
        }
        n_invalid += (unsigned long long)__popcll(__ballot(t < a.T && !valid));
    }
    df_mesh_wave_add(a.counts, 2, n_invalid);
}

__global__ __launch_bounds__(256) void df_msp_claim_kernel(const DfMspArgs a)
{
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < (size_t)a.V; v += (size_t)gridDim.x * 256) {
        if (a.mark[v] != 1) continue;
        int c[3]; uint32_t q[3];
        (void)msp_cell(a.vtx, (uint32_t)v, a.cell, c, q);
        uint32_t h = msp_hash((uint32_t)c[0], (uint32_t)c[1], (uint32_t)c[2], a.vslots);
        for (;;) {                                                       // more slots than members: a free or an own one is always found
            const uint32_t prev = atomicCAS(&a.vowner[h], 0u, (uint32_t)v + 1u);
            bool same = prev == 0u;
            if (!same) {
                int o[3]; uint32_t oq[3];
                (void)msp_cell(a.vtx, prev - 1u, a.cell, o, oq);
                same = o[0] == c[0] && o[1] == c[1] && o[2] == c[2];
            }
            if (same) break;
            h = h + 1u == a.vslots ? 0u : h + 1u;
        }
        atomicMin(&a.vmin[h], (uint32_t)v);
        a.cluster[v] = h;
    }
}

__global__ __launch_bounds__(256) void df_msp_sums_kernel(const DfMspArgs a)
{
    unsigned long long n_clusters = 0ull, n_bad = 0ull;                  // wave-uniform
    for (size_t v0 = (size_t)blockIdx.x * 256; v0 < (size_t)a.V; v0 += (size_t)gridDim.x * 256) {
        const size_t v = v0 + threadIdx.x;
        const uint8_t m = v < (size_t)a.V ? a.mark[v] : (uint8_t)0;
        uint32_t s = DF_MSP_NONE;
        if (m == 1) {
            s = a.vmin[a.cluster[v]];
            int c[3]; uint32_t q[3];
            (void)msp_cell(a.vtx, (uint32_t)v, a.cell, c, q);
            atomicAdd(&a.n[s], 1u);
#pragma unroll
            for (int k = 0; k < 3; ++k) atomicAdd(&a.sum[3 * (size_t)s + k], (unsigned long long)q[k]);
        }
        if (v < (size_t)a.V) a.cluster[v] = s;
        n_clusters += (unsigned long long)__popcll(__ballot(m == 1 && s == (uint32_t)v));
        n_bad += (unsigned long long)__popcll(__ballot(m == 2));
    }
    df_mesh_wave_add(a.counts, 6, n_clusters);
    df_mesh_wave_add(a.counts, 7, n_bad);
}

// the clusters of a triangle; false unless it is valid and the three differ (collapsed: valid, and two are the same)
__device__ __forceinline__ bool msp_triple(const DfMspArgs& a, size_t t, uint32_t (&c)[3], bool& collapsed)
{
    uint32_t i[3];
    collapsed = false;
    if (!df_mesh_load(a.tris, t, a.T, a.V, i)) return false;
    c[0] = a.cluster[i[0]]; c[1] = a.cluster[i[1]]; c[2] = a.cluster[i[2]];
    if (c[0] == DF_MSP_NONE || c[1] == DF_MSP_NONE || c[2] == DF_MSP_NONE) return false;      // a valid triangle's vertices are members, and
    collapsed = c[0] == c[1] || c[1] == c[2] || c[0] == c[2];                                   // three members make a valid triangle
    return !collapsed;
}

// ascending; -> the permutation was even
__device__ __forceinline__ bool msp_sort(uint32_t (&c)[3])
{
    const int inversions = (int)(c[0] > c[1]) + (int)(c[1] > c[2]) + (int)(c[0] > c[2]);
    const uint32_t lo = min(c[0], min(c[1], c[2])), hi = max(c[0], max(c[1], c[2]));
    const uint32_t mid = c[0] ^ c[1] ^ c[2] ^ lo ^ hi;
    c[0] = lo; c[1] = mid; c[2] = hi;
    return (inversions & 1) == 0;
}

__global__ __launch_bounds__(256) void df_msp_classify_kernel(const DfMspArgs a)
{
    const bool grouping = !(a.flags & DF_SIMPLIFY_KEEP_DUPLICATES);
    unsigned long long n_collapsed = 0ull;                               // wave-uniform
    for (size_t t0 = (size_t)blockIdx.x * 256; t0 < a.T; t0 += (size_t)gridDim.x * 256) {
        const size_t t = t0 + threadIdx.x;
        uint32_t c[3];
        bool collapsed = false;
        const bool live = t < a.T && msp_triple(a, t, c, collapsed);
        n_collapsed += (unsigned long long)__popcll(__ballot(collapsed));
        if (t >= a.T) continue;
        if (!grouping) {
            a.tscan[t] = live ? 1u : 0u;
            if (live) { a.vscan[c[0]] = 1u; a.vscan[c[1]] = 1u; a.vscan[c[2]] = 1u; }
            continue;
        }
        uint32_t h = DF_MSP_NONE;
        if (live) {
            const bool even = msp_sort(c);
            h = msp_hash(c[0], c[1], c[2], a.tslots);
            for (;;) {                                                   // more slots than triangles
                const uint32_t prev = atomicCAS(&a.towner[h], 0u, (uint32_t)t + 1u);
                bool same = prev == 0u;
                if (!same) {
                    uint32_t o[3]; bool unused;
                    (void)msp_triple(a, (size_t)(prev - 1u), o, unused);  // (only live triangles claim)
                    (void)msp_sort(o);
                    same = o[0] == c[0] && o[1] == c[1] && o[2] == c[2];
                }
                if (same) break;
                h = h + 1u == a.tslots ? 0u : h + 1u;
            }
            atomicAdd(&a.tbal[h], even ? 1 : -1);
            atomicMin(&a.tmin[2 * (size_t)h + (even ? 0 : 1)], (uint32_t)t);
        }
        a.tscan[t] = h;
    }
    df_mesh_wave_add(a.counts, 3, n_collapsed);
}

__global__ __launch_bounds__(256) void df_msp_decide_kernel(const DfMspArgs a)
{
    unsigned long long n_fin = 0ull, n_dup = 0ull;                       // wave-uniform
    for (size_t t0 = (size_t)blockIdx.x * 256; t0 < a.T; t0 += (size_t)gridDim.x * 256) {
        const size_t t = t0 + threadIdx.x;
        const uint32_t h = t < a.T ? a.tscan[t] : DF_MSP_NONE;
        bool fin = false, dup = false, keep = false;
        uint32_t c[3];
        if (h != DF_MSP_NONE) {
            bool unused;
            (void)msp_triple(a, t, c, unused);
            uint32_t s[3] = {c[0], c[1], c[2]};
            const bool even = msp_sort(s);
            const int bal = a.tbal[h];
            fin = bal == 0;
            keep = !fin && (bal > 0) == even && a.tmin[2 * (size_t)h + (even ? 0 : 1)] == (uint32_t)t;
            dup = !fin && !keep;
        }
        if (t < a.T) a.tscan[t] = keep ? 1u : 0u;
        if (keep) { a.vscan[c[0]] = 1u; a.vscan[c[1]] = 1u; a.vscan[c[2]] = 1u; }
        n_fin += (unsigned long long)__popcll(__ballot(fin));
        n_dup += (unsigned long long)__popcll(__ballot(dup));
    }
    df_mesh_wave_add(a.counts, 4, n_fin);
    df_mesh_wave_add(a.counts, 5, n_dup);
}

__global__ __launch_bounds__(256) void df_msp_compact_triangles_kernel(const DfMspArgs a)
{
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < a.T; t += (size_t)gridDim.x * 256) {
        const uint32_t o = a.tscan[t];
        if (a.tscan[t + 1] == o || (unsigned long long)o >= a.tcap) continue;            // (a kept triangle is valid: its vertices are members)
#pragma unroll
        for (int k = 0; k < 3; ++k) a.tris_out[3 * (size_t)o + k] = a.vscan[a.cluster[a.tris[3 * t + k]]];
    }
}

__global__ __launch_bounds__(256) void df_msp_compact_vertices_kernel(const DfMspArgs a)
{
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < (size_t)a.V; v += (size_t)gridDim.x * 256) {
        const uint32_t j = a.vscan[v];
        if (a.vscan[v + 1] != j && (unsigned long long)j < a.vcap) {     // v is the src of a cluster a kept triangle uses
            if (a.vsrc) a.vsrc[j] = (uint32_t)v;
            float r[4] = {0.f, 0.f, 0.f, 0.f};
            if (a.flags & DF_SIMPLIFY_KEEP_FIRST) {
#pragma unroll
                for (int k = 0; k < 4; ++k) r[k] = a.vtx[4 * v + k];     // (the 16 bytes as they are: loads and stores move bits)
            } else {
                int c[3]; uint32_t q[3];
                (void)msp_cell(a.vtx, (uint32_t)v, a.cell, c, q);        // the cluster's cell is its src's
                const double n = (double)a.n[v];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double m = (double)a.sum[3 * v + k] / n;       // f64, no contraction (-ffp-contract=off)
                    r[k] = (float)(((double)c[k] + m * 0x1p-24) * (double)a.cell);
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) a.vtx_out[4 * (size_t)j + k] = r[k];
        }
        if (a.vmap) {
            const uint32_t s = a.cluster[v];
            a.vmap[v] = s != DF_MSP_NONE && a.vscan[(size_t)s + 1] != a.vscan[s] ? a.vscan[s] : DF_MSP_NONE;
        }
    }
}

extern "C" int dfusion_mesh_simplify(const float* vertices_dev, unsigned long long n_vertices, const unsigned int* triangles_dev,
                                     unsigned long long n_triangles, float cell, unsigned int flags, float* vertices_out_dev,
                                     unsigned long long vertex_capacity, unsigned int* triangles_out_dev, unsigned long long triangle_capacity,
                                     unsigned int* vertex_src_dev, unsigned int* vertex_map_dev, unsigned long long* counts_dev, dfStream stream)
{
    if (n_vertices > 0xffffffffull || n_triangles > 0xffffffffull || !counts_dev) return DF_E_INVALID;
    if ((n_triangles && !triangles_dev) || (n_vertices && !vertices_dev)) return DF_E_INVALID;
    if ((triangle_capacity && !triangles_out_dev) || (vertex_capacity && !vertices_out_dev)) return DF_E_INVALID;
    if (!(cell > 0.f) || !isfinite(cell) || (flags & ~DF_MSP_FLAGS)) return DF_E_INVALID;
    const size_t V = (size_t)n_vertices, T = (size_t)n_triangles;
    const struct { const void* p; size_t n; } ins[2] = {{vertices_dev, V * 16}, {triangles_dev, T * 12}},
        outs[5] = {{vertices_out_dev, (size_t)vertex_capacity * 16}, {triangles_out_dev, (size_t)triangle_capacity * 12},
                   {vertex_src_dev, (size_t)vertex_capacity * 4}, {vertex_map_dev, V * 4}, {counts_dev, 64}};
    for (const auto& i : ins)
        for (const auto& o : outs)
            if (df_mesh_overlap(i.p, i.n, o.p, o.n)) return DF_E_INVALID;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return DF_E_NO_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    const bool emit = triangle_capacity != 0 || vertex_capacity != 0;
    DF_HIP(hipMemsetAsync(counts_dev, 0, 64, st));
    if (!V || !T) {                                                       // no vertex: every triangle is invalid; no triangle: no member
        if (!V && T) DF_TRY(df_mesh_set_counts(counts_dev, 2, n_triangles, 2, n_triangles, st));
        return DF_OK;                                                     // (nothing is kept: the exact capacities are 0 and 0, counts only)
    }
    DfMspArgs a;
    memset(&a, 0, sizeof(a));
    a.vtx = vertices_dev; a.V = (uint32_t)V; a.tris = triangles_dev; a.T = T; a.cell = cell; a.flags = flags;
    a.vtx_out = vertices_out_dev; a.vcap = vertex_capacity; a.tris_out = triangles_out_dev; a.tcap = triangle_capacity;
    a.vsrc = vertex_src_dev; a.vmap = vertex_map_dev; a.counts = counts_dev;
    const bool grouping = !(flags & DF_SIMPLIFY_KEEP_DUPLICATES);
    // the tables: 2 n + 1 slots, more than twice what can enter; slots are 32-bit, so past 2^31 - 1 entries the table only stays larger
    // than its entries
    a.vslots = (uint32_t)(2 * V + 1 < 0xffffffffull ? 2 * V + 1 : 0xffffffffull);
    a.tslots = grouping ? (uint32_t)(2 * T + 1 < 0xffffffffull ? 2 * T + 1 : 0xffffffffull) : 0u;
    size_t scan_bytes = 0;
    DF_TRY(df_mesh_scan_bytes((T > V ? T : V) + 1, st, &scan_bytes));
    // workspace: [zeroed: sums 24 V | n 4 V | vertex flags 4 (V + 1) | triangle flags 4 (T + 1) | cell owners | group owners | balances
    //             | marks V] [set to 0xff: cell minima | group minima, 2 a slot] [cluster 4 V] [hipcub's storage]; one memset a bracket
    DfMeshCarve c;
    const size_t o_sum = c.take(V * 24), o_n = c.take(V * 4), o_vscan = c.take((V + 1) * 4), o_tscan = c.take((T + 1) * 4),
                 o_vowner = c.take((size_t)a.vslots * 4), o_towner = c.take((size_t)a.tslots * 4), o_tbal = c.take((size_t)a.tslots * 4),
                 o_mark = c.take(V), o_vmin = c.take((size_t)a.vslots * 4), o_tmin = c.take((size_t)a.tslots * 8), o_cluster = c.take(V * 4),
                 o_scan = c.take(scan_bytes, 256), zero_end = o_vmin, ff_end = o_cluster;
    DfScratchHold hold(st, c.total());                                    // held until the last launch is enqueued
    if (!hold.entry) return (int)hipErrorOutOfMemory;
    char* const ws = hold.mem;
    a.sum = (unsigned long long*)(ws + o_sum); a.n = (uint32_t*)(ws + o_n); a.vscan = (uint32_t*)(ws + o_vscan); a.tscan = (uint32_t*)(ws + o_tscan);
    a.vowner = (uint32_t*)(ws + o_vowner); a.towner = (uint32_t*)(ws + o_towner); a.tbal = (int*)(ws + o_tbal); a.mark = (uint8_t*)(ws + o_mark);
    a.vmin = (uint32_t*)(ws + o_vmin); a.tmin = (uint32_t*)(ws + o_tmin); a.cluster = (uint32_t*)(ws + o_cluster);
    DF_HIP(hipMemsetAsync(ws, 0, zero_end, st));
    DF_HIP(hipMemsetAsync(ws + zero_end, 0xff, ff_end - zero_end, st));
    const dim3 gt(df_mesh_blocks(T)), gv(df_mesh_blocks(V)), wg(256);
    hipLaunchKernelGGL(df_msp_mark_kernel, gt, wg, 0, st, a);
    DF_LAUNCH_CHECK();
    hipLaunchKernelGGL(df_msp_claim_kernel, gv, wg, 0, st, a);
    DF_LAUNCH_CHECK();
    hipLaunchKernelGGL(df_msp_sums_kernel, gv, wg, 0, st, a);
    DF_LAUNCH_CHECK();
    hipLaunchKernelGGL(df_msp_classify_kernel, gt, wg, 0, st, a);
    DF_LAUNCH_CHECK();
    if (grouping) {
        hipLaunchKernelGGL(df_msp_decide_kernel, gt, wg, 0, st, a);
        DF_LAUNCH_CHECK();
    }
    DF_TRY(df_mesh_scan_pair(ws + o_scan, scan_bytes, a.tscan, T + 1, a.vscan, V + 1, counts_dev, st));
    if (!emit) return DF_OK;
    if (a.tcap) {
        hipLaunchKernelGGL(df_msp_compact_triangles_kernel, gt, wg, 0, st, a);
        DF_LAUNCH_CHECK();
    }
    if (a.vcap || a.vmap) {
        hipLaunchKernelGGL(df_msp_compact_vertices_kernel, gv, wg, 0, st, a);
        DF_LAUNCH_CHECK();
    }
    return DF_OK;
}
