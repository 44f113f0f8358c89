// dfusion_mesh_smooth.hip -- dfusion_mesh_adjacency: the vertex adjacency of an indexed triangle mesh as a CSR of sorted unique
// neighbours, with the classes of its edges and vertices; dfusion_mesh_smooth: lambda | mu umbrella steps (Taubin) over that adjacency.
// Both rules are stated in include/dfusion.h and DESIGN.md section 24 and restated in numpy by tests/mesh_smooth_ref.py, against which
// every output is compared for equality.  The adjacency is decided by integers alone (a sort, a scan for the positions, integer
// atomicMax and counts); a smoothing step is a function of its input buffer alone, its f32 operations in one stated order.
//
//   emit, sort, heads   dfusion_mesh_uses.h: the directed uses of every edge as sorted 2k-bit keys (src << k | dst) with a direction
//             byte, and the position of every run of equal keys -- the position of every CSR entry
//   edges     one lane per sorted key: a run head writes its dst at its position; the head of a run with src < dst judges its run
//             (msm_run of dfusion_mesh_uses.h), classifies the edge and raises the classes of its two ends by integer atomicMax
//   rows      one lane per v in 0 .. V: a binary search for the first key with src >= v; row_start[v] is that key's position
//   classes   one lane per vertex: its class byte from its degree and the raised word; the vertices with a neighbour and those on a
//             boundary or irregular edge counted
//   step      one lane per vertex: dfusion_mesh_smooth's hot path, run 2 x iterations times (below)
// Every grid is capped at DF_MESH_MAX_BLOCKS workgroups (524 288 lanes) and strides over its range with 64-bit indices (dfusion_mesh_kit.h).
#include "dfusion_mesh_uses.h"                        // emit, sort, heads and the scan: shared with dfusion_mesh_boundary_loops
#include <math.h>

#pragma clang fp contract(off)                       // p + s * delta is a multiply, then an add (the library's -ffp-contract=off, kept for this file)

#define DF_MSM_GATHER 8                              // neighbour positions in flight per lane

struct DfMsmAdjArgs : DfMsmArgs {                            // the sorted uses, and what only the adjacency has
    uint32_t* cls;                                           // [V] 0, raised to 2 (boundary) or 3 (irregular)
    uint32_t* row_start;                                     // [V + 1] the caller's, or workspace
    uint32_t* nbr; unsigned long long cap; uint8_t* vclass;
};

__global__ __launch_bounds__(256) void df_msm_edges_kernel(const DfMsmAdjArgs a)
{
    const unsigned long long lo_mask = a.k == 32 ? 0xffffffffull : (1ull << a.k) - 1ull;
    unsigned long long n_edges = 0ull, n_boundary = 0ull, n_irregular = 0ull;                  // wave-uniform
    for (size_t i0 = (size_t)blockIdx.x * 256; i0 < a.N; i0 += (size_t)gridDim.x * 256) {
        const size_t i = i0 + threadIdx.x;
        bool edge = false, boundary = false, irregular = false;
        if (i < a.N) {
            const uint32_t p = a.pos[i];
            if (a.pos[i + 1] != p) {                                    // a run head
                const unsigned long long key = a.keys[i];
                const uint32_t src = (uint32_t)(key >> a.k), dst = (uint32_t)(key & lo_mask);
                if ((unsigned long long)p < a.cap) a.nbr[p] = dst;
                if (src < dst) {                                        // the edge {src < dst} is judged once, here
                    const DfMsmRun run = msm_run(a.keys, a.dir, a.N, i);
                    edge = true;
                    boundary = run.boundary();
                    irregular = run.irregular();
                    if (boundary || irregular) {
                        const uint32_t c = irregular ? 3u : 2u;
                        atomicMax(&a.cls[src], c);
                        atomicMax(&a.cls[dst], c);
                    }
                }
            }
        }
        n_edges += (unsigned long long)__popcll(__ballot(edge));
        n_boundary += (unsigned long long)__popcll(__ballot(boundary));
        n_irregular += (unsigned long long)__popcll(__ballot(irregular));
    }
    df_mesh_wave_add(a.counts, 1, n_edges);
    df_mesh_wave_add(a.counts, 2, n_boundary);
    df_mesh_wave_add(a.counts, 3, n_irregular);
}

__global__ __launch_bounds__(256) void df_msm_rows_kernel(const DfMsmAdjArgs a)
{
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v <= a.V; v += (size_t)gridDim.x * 256) {
        size_t lo = 0, hi = a.N;                                        // the first key whose src is >= v (the all-ones key's is 2^k - 1 >= V)
        while (lo < hi) {
            const size_t mid = lo + (hi - lo) / 2;
            if ((a.keys[mid] >> a.k) < (unsigned long long)v) lo = mid + 1; else hi = mid;
        }
        a.row_start[v] = a.pos[lo];
        if (v == a.V) a.counts[0] = a.pos[a.N];                         // (= pos[lo]: no real key has a src >= V)
    }
}

__global__ __launch_bounds__(256) void df_msm_classes_kernel(const DfMsmAdjArgs a)
{
    unsigned long long n_used = 0ull, n_open = 0ull;                    // wave-uniform
    for (size_t v0 = (size_t)blockIdx.x * 256; v0 < a.V; v0 += (size_t)gridDim.x * 256) {
        const size_t v = v0 + threadIdx.x;
        uint32_t c = 0u;
        if (v < a.V) {
            const uint32_t raised = a.cls[v];
            c = a.row_start[v + 1] != a.row_start[v] ? (raised > 1u ? raised : 1u) : 0u;
            if (a.vclass) a.vclass[v] = (uint8_t)c;
        }
        n_used += (unsigned long long)__popcll(__ballot(c != 0u));
        n_open += (unsigned long long)__popcll(__ballot(c >= 2u));
    }
    df_mesh_wave_add(a.counts, 4, n_used);
    df_mesh_wave_add(a.counts, 7, n_open);
}

extern "C" int dfusion_mesh_adjacency(const unsigned int* triangles_dev, unsigned long long n_triangles, unsigned long long n_vertices,
                                      unsigned int* row_start_dev, unsigned int* neighbours_dev, unsigned long long neighbour_capacity,
                                      unsigned char* vertex_class_dev, unsigned long long* counts_dev, dfStream stream)
{
    if (n_vertices > 0xffffffffull || n_triangles > 0xffffffffull / 6ull || !counts_dev) return DF_E_INVALID;
    if ((n_triangles && !triangles_dev) || (neighbour_capacity && !neighbours_dev)) return DF_E_INVALID;
    const size_t V = (size_t)n_vertices, T = (size_t)n_triangles, N = 6 * T;
    const struct { const void* p; size_t n; } outs[4] = {{row_start_dev, (V + 1) * 4}, {neighbours_dev, (size_t)neighbour_capacity * 4},
                                                         {vertex_class_dev, V}, {counts_dev, 64}};
    for (const auto& o : outs)
        if (df_mesh_overlap(triangles_dev, T * 12, o.p, o.n)) return DF_E_INVALID;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return DF_E_NO_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    DF_HIP(hipMemsetAsync(counts_dev, 0, 64, st));
    if (!V || !T) {                                                       // no vertex: every triangle is invalid; no triangle: no neighbour
        if (row_start_dev) DF_HIP(hipMemsetAsync(row_start_dev, 0, (V + 1) * 4, st));
        if (vertex_class_dev && V) DF_HIP(hipMemsetAsync(vertex_class_dev, 0, V, st));
        if (!V && T) DF_TRY(df_mesh_set_counts(counts_dev, 5, n_triangles, 5, n_triangles, st));
        return DF_OK;
    }
    DfMsmAdjArgs a;
    memset(&a, 0, sizeof(a));
    a.tris = triangles_dev; a.T = T; a.V = V; a.N = N;
    a.k = df_msm_key_bits(V);                                             // 2^k > V
    a.nbr = neighbours_dev; a.cap = neighbour_capacity; a.vclass = vertex_class_dev; a.counts = counts_dev;
    a.slot_invalid = 5; a.slot_degenerate = 6;
    size_t cub_bytes = 0;
    DF_TRY(df_msm_uses_cub_bytes(N, a.k, N + 1, st, &cub_bytes));
    // workspace: [the sorted uses' 108 T (dfusion_mesh_uses.h)] [raised classes 4 V, zeroed] [row_start 4 (V + 1), unless the caller
    //            gives one] [hipcub's storage]
    DfMeshCarve c; c.take(df_msm_uses_bytes(N));
    const size_t o_cls = c.take(V * 4), o_rows = row_start_dev ? 0 : c.take((V + 1) * 4), o_cub = c.take(cub_bytes, 256);
    DfScratchHold hold(st, c.total());                                    // held until the last launch is enqueued
    if (!hold.entry) return (int)hipErrorOutOfMemory;
    char* const ws = hold.mem;
    a.cls = (uint32_t*)(ws + o_cls);
    a.row_start = row_start_dev ? row_start_dev : (uint32_t*)(ws + o_rows);
    DF_HIP(hipMemsetAsync(a.cls, 0, V * 4, st));
    DF_TRY(df_msm_sorted_uses(a, ws, ws + o_cub, cub_bytes, st));
    const dim3 gn(df_mesh_blocks(N + 1)), gv(df_mesh_blocks(V + 1)), wg(256);
    hipLaunchKernelGGL(df_msm_edges_kernel, gn, wg, 0, st, a);
    DF_LAUNCH_CHECK();
    hipLaunchKernelGGL(df_msm_rows_kernel, gv, wg, 0, st, a);
    DF_LAUNCH_CHECK();
    hipLaunchKernelGGL(df_msm_classes_kernel, gv, wg, 0, st, a);
    DF_LAUNCH_CHECK();
    return DF_OK;
}

// ---------------------------------------------------------------------------------------------------------------- dfusion_mesh_smooth
// One step: Q[v] = P[v] + s * (mean of P over v's row - P[v]) for a movable v, P[v] as it is otherwise.  One lane per vertex.  The row
// bounds are one 8-byte load where v is even (row_start is 8-byte aligned then), every position one load of a float4 (of a neighbour
// the compiler fetches the 12 bytes that are used), the result one 16-byte store.  A row is taken DF_MSM_GATHER neighbours at a time: their indices are read first, then all their positions are
// requested, and only then added in the row's order -- up to DF_MSM_GATHER gathers in flight per lane, whatever the degree.
__global__ __launch_bounds__(256) void df_msm_step_kernel(const float4* __restrict__ P, float4* __restrict__ Q, const uint32_t* __restrict__ row_start,
                                                          const uint32_t* __restrict__ nbr, const uint8_t* __restrict__ vclass, size_t V, float s,
                                                          int fix_boundary)
{
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (size_t)gridDim.x * 256) {
        uint32_t r0, r1;
        if ((v & 1) == 0 && ((uintptr_t)row_start & 7) == 0) {
            const uint2 r = *reinterpret_cast<const uint2*>(row_start + v);
            r0 = r.x; r1 = r.y;
        } else {
            r0 = row_start[v]; r1 = row_start[v + 1];
        }
        const float4 p = P[v];
        const uint32_t d = r1 - r0;
        const bool movable = d != 0u && (!fix_boundary || !vclass || vclass[v] == 1);
        float4 q = p;
        if (movable) {
            float ax = 0.f, ay = 0.f, az = 0.f;
            for (size_t j = r0; j < r1; j += DF_MSM_GATHER) {
                const size_t left = r1 - j;                              // >= 1
                uint32_t u[DF_MSM_GATHER];
                float4 g[DF_MSM_GATHER];
#pragma unroll
                for (int c = 0; c < DF_MSM_GATHER; ++c) u[c] = (size_t)c < left ? nbr[j + c] : (uint32_t)v;     // past the row: v itself, not added
#pragma unroll
                for (int c = 0; c < DF_MSM_GATHER; ++c) g[c] = P[u[c]];
#pragma unroll
                for (int c = 0; c < DF_MSM_GATHER; ++c)
                    if ((size_t)c < left) { ax = ax + g[c].x; ay = ay + g[c].y; az = az + g[c].z; }
            }
            const float n = (float)d;
            const float mx = ax / n, my = ay / n, mz = az / n;               // IEEE f32 division
            const float dx = mx - p.x, dy = my - p.y, dz = mz - p.z;
            q.x = p.x + s * dx; q.y = p.y + s * dy; q.z = p.z + s * dz;       // a multiply, then an add
        }
        Q[v] = q;
    }
}

extern "C" int dfusion_mesh_smooth(const float* vertices_dev, unsigned long long n_vertices, const unsigned int* row_start_dev,
                                   const unsigned int* neighbours_dev, unsigned long long n_neighbours, const unsigned char* vertex_class_dev,
                                   int iterations, float lambda, float mu, unsigned int flags, float* vertices_out_dev, dfStream stream)
{
    if (n_vertices > 0xffffffffull || n_neighbours > 0xffffffffull || iterations < 0 || !isfinite(lambda) || !isfinite(mu)) return DF_E_INVALID;
    if (flags & ~DF_SMOOTH_FIX_BOUNDARY) return DF_E_INVALID;
    if (n_vertices && (!vertices_dev || !vertices_out_dev || !row_start_dev)) return DF_E_INVALID;
    if (n_neighbours && !neighbours_dev) return DF_E_INVALID;
    const size_t V = (size_t)n_vertices;
    const bool in_place = vertices_out_dev == vertices_dev;
    const struct { const void* p; size_t n; } ins[4] = {{in_place ? nullptr : vertices_dev, V * 16}, {row_start_dev, (V + 1) * 4},
                                                        {neighbours_dev, (size_t)n_neighbours * 4}, {vertex_class_dev, V}};
    for (const auto& i : ins)
        if (df_mesh_overlap(i.p, i.n, vertices_out_dev, V * 16)) return DF_E_INVALID;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return DF_E_NO_DEVICE;
    if (!V) return DF_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t per_iteration = mu == 0.f ? 1 : 2, steps = (size_t)iterations * per_iteration;
    if (!steps) {
        if (!in_place) DF_HIP(hipMemcpyAsync(vertices_out_dev, vertices_dev, V * 16, hipMemcpyDeviceToDevice, st));
        return DF_OK;
    }
    // Ping-pong between the output and one scratch buffer [16 V].  Out of place the step that has an even number of steps after it
    // writes the output, so the last one does.  In place no step may write the buffer it reads: step 0 writes the scratch, and when
    // that leaves the last step in the scratch too (an odd count) one copy brings the result home.
    DfScratchHold hold(st, steps > 1 || in_place ? V * 16 : 16);
    if (!hold.entry) return (int)hipErrorOutOfMemory;
    float4* const scratch = (float4*)hold.mem;
    float4* const out = (float4*)vertices_out_dev;
    const dim3 grid(df_mesh_blocks(V)), wg(256);
    const float4* src = (const float4*)vertices_dev;
    float4* dst = nullptr;
    for (size_t k = 0; k < steps; ++k) {
        const bool to_out = in_place ? (k & 1) != 0 : ((steps - 1 - k) & 1) == 0;
        dst = to_out ? out : scratch;
        const float s = per_iteration == 2 && (k & 1) ? mu : lambda;
        hipLaunchKernelGGL(df_msm_step_kernel, grid, wg, 0, st, src, dst, (const uint32_t*)row_start_dev, (const uint32_t*)neighbours_dev,
                           (const uint8_t*)vertex_class_dev, V, s, (int)((flags & DF_SMOOTH_FIX_BOUNDARY) != 0));
        DF_LAUNCH_CHECK();
        src = dst;
    }
    if (dst != out) DF_HIP(hipMemcpyAsync(out, scratch, V * 16, hipMemcpyDeviceToDevice, st));
    return DF_OK;
}
