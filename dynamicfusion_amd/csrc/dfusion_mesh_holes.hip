// dfusion_mesh_holes.hip -- dfusion_mesh_boundary_loops: the closed loops of boundary half-edges of an indexed triangle mesh, every
// vertex's loop label and rank and a CSR of the loops; dfusion_mesh_fill_holes: the mesh with every loop of at most max_edges edges
// closed by a fan around its centroid.  Both rules are stated in include/dfusion.h and DESIGN.md section 27 and restated in numpy by
// tests/mesh_holes_ref.py, against which every output is compared for equality.  The loops are decided by integers alone (the sorted
// edge uses of dfusion_mesh_uses.h, integer atomics, pointer doubling between two buffers, two scans); a centroid is one lane's f32
// sum in rank order and one division.
//
//   uses      dfusion_mesh_uses.h: emit, sort, heads and their scan -- shared with dfusion_mesh_adjacency
//   runs      one lane per sorted key: the head of a run judges its run (msm_run: f zeros, b ones).  f == 1, b == 0: a boundary half-edge
//             src -> dst: out[src] and in[dst] are incremented, cand[src] = dst.  Neither that nor f == 1, b == 1 nor f == 0, b == 1:
//             an irregular edge, a flag raised on both ends by integer atomicMax
//   classify  one lane per vertex: SIMPLE iff out == 1, in == 1 and no flag; next[v]; the first record of the doubling pass
//             {smallest index in the window, forward offset of its first occurrence, jump}: {v, 0, next(v) if that is simple, else DEAD}
//   round     ceil(log2 V) Jacobi rounds from one buffer into the other: a live record takes the record behind its jump -- index
//             and offset only where that index is STRICTLY smaller (so an offset counts to the first occurrence and stays below L), the
//             jump always (DEAD spreads back from the end of an open chain)
//   label     one lane per vertex: on a loop iff the jump is alive; label = the window's smallest index, D = its offset,
//             L = D(next(label)) + 1, rank = (L - D) % L; a flag and L at every label vertex
//   scans     df_mesh_scan_pair: two hipcub exclusive sums, the loops' numbers and their starts
//   scatter   one lane per vertex: loop_vertices[start + rank] = v; the label vertex writes loop_start
//   select, fill   dfusion_mesh_fill_holes (below)
// Every grid is capped at DF_MESH_MAX_BLOCKS workgroups (524 288 lanes) and strides over its range with 64-bit indices.  Counts are summed
// per wave from ballots, then per workgroup through LDS (df_mesh_block_add, lane 0 speaking for its wave): one atomic per workgroup and slot.
#include "dfusion_mesh_uses.h"
#include <math.h>

#pragma clang fp contract(off)                       // the centroid is adds and one division; nothing here may fuse

#define DF_MHL_NONE 0xffffffffu                      // no vertex: V <= 2^32 - 1, so every index is smaller

struct DfMhlArgs {
    size_t V, N, T; int k;
    const unsigned long long* keys; const uint8_t* dir; const uint32_t* pos;         // the sorted uses
    uint32_t *out, *in, *irr;                                // [V] each, zeroed: boundary half-edges leaving / entering, irregular flag
    uint32_t *cand;                                          // [V] the head of a boundary half-edge that leaves v (the one, where out == 1)
    uint32_t *next, *lab, *rnk;                              // [V] the caller's arrays, or workspace
    uint32_t *vnext;                                         // [V] the caller's copy of next, or NULL
    uint4 *rec_a, *rec_b;                                    // [V] {index, offset, jump, -}
    uint32_t *flag, *len;                                    // [V + 1] 1 / L at a label vertex; after the scans the loop's number / start
    uint32_t *loop_start, *loop_vertices; unsigned long long loop_cap, vertex_cap;
    unsigned long long* counts;                              // the loop stage's eight
    // dfusion_mesh_fill_holes
    uint32_t max_edges;
    uint32_t *sel, *toff;                                    // [V + 1] 1 / L at the label vertex of a filled loop; after the scans number / first triangle
    const float4* P; const uint32_t* tris;
    float4* out_v; uint32_t* out_t; uint32_t* vsrc; unsigned long long out_vcap, out_tcap;
    unsigned long long* fill_counts;
};

// (a wave-uniform count as df_mesh_block_add takes it: from lane 0 of the wave, 0 from the others)
__device__ __forceinline__ unsigned long long mhl_once(unsigned long long wave_uniform) { return (threadIdx.x & 63) == 0 ? wave_uniform : 0ull; }

__global__ __launch_bounds__(256) void df_mhl_runs_kernel(const DfMhlArgs a)
{
    const unsigned long long lo_mask = a.k == 32 ? 0xffffffffull : (1ull << a.k) - 1ull;
    unsigned long long n_boundary = 0ull;                                // wave-uniform
    for (size_t i0 = (size_t)blockIdx.x * 256; i0 < a.N; i0 += (size_t)gridDim.x * 256) {      // (workgroup-uniform trip count)
        const size_t i = i0 + threadIdx.x;
        bool boundary = false;
        if (i < a.N && a.pos[i + 1] != a.pos[i]) {                       // a run head (src, dst); src != dst, both < V
            const unsigned long long key = a.keys[i];
            const uint32_t src = (uint32_t)(key >> a.k), dst = (uint32_t)(key & lo_mask);
            const DfMsmRun run = msm_run(a.keys, a.dir, a.N, i);
            if (run.boundary()) {
                if (run.f) {                                             // the edge's one use runs src -> dst
                    boundary = true;
                    atomicAdd(&a.out[src], 1u);
                    atomicAdd(&a.in[dst], 1u);
                    a.cand[src] = dst;                                   // several writers only where out > 1: never read then
                }
            } else if (run.irregular()) {
                atomicMax(&a.irr[src], 1u);
                atomicMax(&a.irr[dst], 1u);
            }
        }
        n_boundary += (unsigned long long)__popcll(__ballot(boundary));
    }
    const int slot[1] = {2};
    const unsigned long long n[1] = {mhl_once(n_boundary)};
    df_mesh_block_add(a.counts, slot, n);
}

__device__ __forceinline__ bool mhl_simple(const DfMhlArgs& a, size_t v) { return a.out[v] == 1u && a.in[v] == 1u && a.irr[v] == 0u; }

__global__ __launch_bounds__(256) void df_mhl_classify_kernel(const DfMhlArgs a)
{
    unsigned long long n_other = 0ull;
    for (size_t v0 = (size_t)blockIdx.x * 256; v0 < a.V; v0 += (size_t)gridDim.x * 256) {
        const size_t v = v0 + threadIdx.x;
        bool other = false;
        if (v < a.V) {
            const bool simple = mhl_simple(a, v);
            other = !simple && a.out[v] + a.in[v] != 0u;                 // (neither sum nor counter can wrap: 6 T < 2^32)
            uint32_t nx = DF_MHL_NONE;
            uint4 rec = make_uint4(DF_MHL_NONE, 0u, DF_MHL_NONE, 0u);
            if (simple) {
                nx = a.cand[v];
                rec = make_uint4((uint32_t)v, 0u, mhl_simple(a, nx) ? nx : DF_MHL_NONE, 0u);
            }
            a.next[v] = nx;
            if (a.vnext) a.vnext[v] = nx;
            a.rec_a[v] = rec;
        }
        n_other += (unsigned long long)__popcll(__ballot(other));
    }
    const int slot[1] = {3};
    const unsigned long long n[1] = {mhl_once(n_other)};
    df_mesh_block_add(a.counts, slot, n);
}

// Round r: the window of 2^r vertices from v takes in the window of 2^r behind it.  Reads `from` only, writes `to` only.
__global__ __launch_bounds__(256) void df_mhl_round_kernel(const uint4* __restrict__ from, uint4* __restrict__ to, size_t V, int r)
{
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (size_t)gridDim.x * 256) {
        uint4 rec = from[v];
        if (rec.z != DF_MHL_NONE) {
            const uint4 far = from[rec.z];
            if (far.x < rec.x) { rec.x = far.x; rec.y = (r < 32 ? 1u << r : 0u) + far.y; }     // strictly smaller only; then 2^r < L <= V
            rec.z = far.z;
        }
        to[v] = rec;
    }
}

__global__ __launch_bounds__(256) void df_mhl_label_kernel(const DfMhlArgs a, const uint4* __restrict__ rec)
{
    unsigned long long n_loops = 0ull, n_on = 0ull, n_chain = 0ull;
    uint32_t longest = 0u;
    for (size_t v0 = (size_t)blockIdx.x * 256; v0 <= a.V; v0 += (size_t)gridDim.x * 256) {
        const size_t v = v0 + threadIdx.x;
        bool is_label = false, on = false, chain = false;
        if (v < a.V) {
            const uint4 r = rec[v];
            on = r.z != DF_MHL_NONE;                                     // simple, and the walk never ends
            chain = !on && r.x != DF_MHL_NONE;                           // simple, and it does
            uint32_t label = DF_MHL_NONE, rank = DF_MHL_NONE, L = 0u;
            if (on) {
                label = r.x;
                L = rec[a.next[label]].y + 1u;                           // the label's successor is L - 1 steps before it
                rank = (L - r.y) % L;
                is_label = label == (uint32_t)v;
                if (is_label && L > longest) longest = L;
            }
            a.lab[v] = label;
            a.rnk[v] = rank;
            a.flag[v] = is_label ? 1u : 0u;
            a.len[v] = is_label ? L : 0u;
        } else if (v == a.V) {
            a.flag[v] = 0u; a.len[v] = 0u;                               // the spare element: the totals after the scans
        }
        n_loops += (unsigned long long)__popcll(__ballot(is_label));
        n_on += (unsigned long long)__popcll(__ballot(on));
        n_chain += (unsigned long long)__popcll(__ballot(chain));
    }
    const int slot[3] = {0, 1, 4};
    const unsigned long long n[3] = {mhl_once(n_loops), mhl_once(n_on), mhl_once(n_chain)};
    df_mesh_block_add(a.counts, slot, n);
    const int mslot[1] = {5};
    const uint32_t m[1] = {longest};
    df_mesh_block_max(a.counts, mslot, m);
}

// After the scans: flag[l] is the number of the loop labelled l, len[l] its start; flag[V] and len[V] are the totals.
__global__ __launch_bounds__(256) void df_mhl_scatter_kernel(const DfMhlArgs a)
{
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v <= a.V; v += (size_t)gridDim.x * 256) {
        if (v == a.V) {
            if ((unsigned long long)a.flag[v] <= a.loop_cap) a.loop_start[a.flag[v]] = a.len[v];
            continue;
        }
        const uint32_t l = a.lab[v];
        if (l == DF_MHL_NONE) continue;
        const uint32_t number = a.flag[l], start = a.len[l];
        if ((uint32_t)v == l && (unsigned long long)number < a.loop_cap) a.loop_start[number] = start;
        const unsigned long long at = (unsigned long long)start + a.rnk[v];
        if (at < a.vertex_cap) a.loop_vertices[at] = (uint32_t)v;
    }
}

// What the loop stage needs of the scratch behind the sorted uses, front to back (all 16-byte aligned):
// [out, in, irr 12 V, zeroed] [cand 4 V] [next, lab, rnk 4 V each] [flag, len, sel, toff 4 (V + 1) each] [two record buffers 16 V each]
// [eight counts] [hipcub's storage, 256-byte aligned]
struct DfMhlLayout { size_t o_cnt3, o_cand, o_next, o_lab, o_rnk, o_flag, o_len, o_sel, o_toff, o_rec_a, o_rec_b, o_counts, o_cub, cub_bytes, total; };

static int mhl_plan(size_t V, size_t N, int k, hipStream_t st, DfMhlLayout* l)
{
    DF_TRY(df_msm_uses_cub_bytes(N, k, (N > V ? N : V) + 1, st, &l->cub_bytes));
    DfMeshCarve c; c.take(df_msm_uses_bytes(N));
    l->o_cnt3 = c.take(V * 12); l->o_cand = c.take(V * 4); l->o_next = c.take(V * 4); l->o_lab = c.take(V * 4); l->o_rnk = c.take(V * 4);
    l->o_flag = c.take((V + 1) * 4); l->o_len = c.take((V + 1) * 4); l->o_sel = c.take((V + 1) * 4); l->o_toff = c.take((V + 1) * 4);
    l->o_rec_a = c.take(V * 16); l->o_rec_b = c.take(V * 16); l->o_counts = c.take(64);
    l->o_cub = c.take(l->cub_bytes, 256);
    l->total = c.total();
    return DF_OK;
}

// The loop stage up to the label kernel, for T > 0 and V > 0: a.next / a.lab / a.rnk (NULL: workspace), a.vnext and a.counts (zeroed by
// the caller) are the caller's.  Leaves flag / len unscanned.
static int mhl_loops(DfMhlArgs& a, const uint32_t* tris, char* ws, const DfMhlLayout& l, hipStream_t st)
{
    const size_t V = a.V;
    DfMsmArgs u;
    memset(&u, 0, sizeof(u));
    u.tris = tris; u.T = a.T; u.V = V; u.N = a.N; u.k = a.k; u.counts = a.counts; u.slot_invalid = 6; u.slot_degenerate = 7;
    DF_TRY(df_msm_sorted_uses(u, ws, ws + l.o_cub, l.cub_bytes, st));
    a.keys = u.keys; a.dir = u.dir; a.pos = u.pos;
    a.out = (uint32_t*)(ws + l.o_cnt3); a.in = a.out + V; a.irr = a.in + V;
    a.cand = (uint32_t*)(ws + l.o_cand);
    if (!a.next) a.next = (uint32_t*)(ws + l.o_next);
    if (!a.lab) a.lab = (uint32_t*)(ws + l.o_lab);
    if (!a.rnk) a.rnk = (uint32_t*)(ws + l.o_rnk);
    a.flag = (uint32_t*)(ws + l.o_flag); a.len = (uint32_t*)(ws + l.o_len); a.sel = (uint32_t*)(ws + l.o_sel); a.toff = (uint32_t*)(ws + l.o_toff);
    a.rec_a = (uint4*)(ws + l.o_rec_a); a.rec_b = (uint4*)(ws + l.o_rec_b);
    DF_HIP(hipMemsetAsync(a.out, 0, V * 12, st));
    const dim3 gn(df_mesh_blocks(a.N)), gv(df_mesh_blocks(V + 1)), wg(256);
    hipLaunchKernelGGL(df_mhl_runs_kernel, gn, wg, 0, st, a);
    DF_LAUNCH_CHECK();
    hipLaunchKernelGGL(df_mhl_classify_kernel, gv, wg, 0, st, a);
    DF_LAUNCH_CHECK();
    // ceil(log2 V) rounds: windows of 2^rounds >= V vertices.  A loop has L <= V vertices, so every window holds its label; a simple v
    // on an open chain is d <= V - 1 steps from the vertex that ends its walk, and its jump is alive after r rounds iff 2^r <= d - 1.
    int rounds = 0;
    while (rounds < 32 && (1ull << rounds) < (unsigned long long)V) ++rounds;
    uint4 *from = a.rec_a, *to = a.rec_b;
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(df_mhl_round_kernel, gv, wg, 0, st, (const uint4*)from, to, V, r);
        DF_LAUNCH_CHECK();
        uint4* const t = from; from = to; to = t;
    }
    hipLaunchKernelGGL(df_mhl_label_kernel, gv, wg, 0, st, a, (const uint4*)from);
    DF_LAUNCH_CHECK();
    return DF_OK;
}

extern "C" int dfusion_mesh_boundary_loops(const unsigned int* triangles_dev, unsigned long long n_triangles, unsigned long long n_vertices,
                                           unsigned int* vertex_next_dev, unsigned int* vertex_loop_dev, unsigned int* vertex_rank_dev,
                                           unsigned int* loop_start_dev, unsigned long long loop_capacity, unsigned int* loop_vertices_dev,
                                           unsigned long long vertex_capacity, unsigned long long* counts_dev, dfStream stream)
{
    if (n_vertices > 0xffffffffull || n_triangles > 0xffffffffull / 6ull || !counts_dev) return DF_E_INVALID;
    if (loop_capacity > 0xffffffffull || vertex_capacity > 0xffffffffull) return DF_E_INVALID;
    if ((n_triangles && !triangles_dev) || (n_vertices && !vertex_loop_dev)) return DF_E_INVALID;
    const bool csr = loop_capacity || vertex_capacity;
    if ((csr && !loop_start_dev) || (vertex_capacity && !loop_vertices_dev)) return DF_E_INVALID;
    const size_t V = (size_t)n_vertices, T = (size_t)n_triangles, N = 6 * T;
    const struct { const void* p; size_t n; } outs[6] = {{vertex_next_dev, V * 4}, {vertex_loop_dev, V * 4}, {vertex_rank_dev, V * 4},
                                                         {csr ? loop_start_dev : nullptr, ((size_t)loop_capacity + 1) * 4},
                                                         {loop_vertices_dev, (size_t)vertex_capacity * 4}, {counts_dev, 64}};
    for (const auto& o : outs)
        if (df_mesh_overlap(triangles_dev, T * 12, o.p, o.n)) return DF_E_INVALID;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return DF_E_NO_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    DF_HIP(hipMemsetAsync(counts_dev, 0, 64, st));
    if (!V || !T) {                                                       // no vertex: every triangle is invalid; no triangle: no boundary
        if (V) {
            if (vertex_next_dev) DF_HIP(hipMemsetAsync(vertex_next_dev, 0xff, V * 4, st));
            DF_HIP(hipMemsetAsync(vertex_loop_dev, 0xff, V * 4, st));
            if (vertex_rank_dev) DF_HIP(hipMemsetAsync(vertex_rank_dev, 0xff, V * 4, st));
        }
        if (csr) DF_HIP(hipMemsetAsync(loop_start_dev, 0, 4, st));
        if (!V && T) DF_TRY(df_mesh_set_counts(counts_dev, 6, n_triangles, 7, 0ull, st));
        return DF_OK;
    }
    DfMhlArgs a;
    memset(&a, 0, sizeof(a));
    a.V = V; a.N = N; a.T = T; a.k = df_msm_key_bits(V);
    a.lab = vertex_loop_dev; a.rnk = vertex_rank_dev; a.vnext = vertex_next_dev; a.counts = counts_dev;
    a.loop_start = loop_start_dev; a.loop_vertices = loop_vertices_dev; a.loop_cap = loop_capacity; a.vertex_cap = vertex_capacity;
    DfMhlLayout l;
    DF_TRY(mhl_plan(V, N, a.k, st, &l));
    DfScratchHold hold(st, l.total);                                      // held until the last launch is enqueued
    if (!hold.entry) return (int)hipErrorOutOfMemory;
    DF_TRY(mhl_loops(a, triangles_dev, hold.mem, l, st));
    if (!csr) return DF_OK;
    DF_TRY(df_mesh_scan_pair(hold.mem + l.o_cub, l.cub_bytes, a.flag, V + 1, a.len, V + 1, nullptr, st));
    hipLaunchKernelGGL(df_mhl_scatter_kernel, dim3(df_mesh_blocks(V + 1)), dim3(256), 0, st, a);
    DF_LAUNCH_CHECK();
    return DF_OK;
}

// ------------------------------------------------------------------------------------------------------------ dfusion_mesh_fill_holes
// select    one lane per v in 0 .. V: sel / toff = 1 / L at the label vertex of a loop with L <= max_edges, 0 elsewhere; the loops left
//           open and the longest loop of either kind counted.  Two exclusive sums: the filled loops' numbers and first triangles.
// fill      one lane per v in 0 .. V.  A vertex of rank j on a filled loop writes triangle j of its loop, (next(v), v, m); the label
//           vertex also walks its loop once in rank order for the centroid -- L <= max_edges steps of dependent loads in ONE lane,
//           so the launch grows with max_edges -- and writes vertex m.  Lane V writes the counts that the scans' totals give.
__global__ __launch_bounds__(256) void df_mhl_select_kernel(const DfMhlArgs a)
{
    unsigned long long n_open = 0ull;
    uint32_t top_filled = 0u, top_open = 0u;
    for (size_t v0 = (size_t)blockIdx.x * 256; v0 <= a.V; v0 += (size_t)gridDim.x * 256) {
        const size_t v = v0 + threadIdx.x;
        bool open = false;
        if (v <= a.V) {
            const uint32_t L = a.len[v];                                 // 0 unless v is a label vertex (and at v == V)
            const bool filled = a.flag[v] != 0u && L <= a.max_edges;
            open = a.flag[v] != 0u && !filled;
            a.sel[v] = filled ? 1u : 0u;
            a.toff[v] = filled ? L : 0u;
            if (filled && L > top_filled) top_filled = L;
            if (open && L > top_open) top_open = L;
        }
        n_open += (unsigned long long)__popcll(__ballot(open));
    }
    const int slot[1] = {3};
    const unsigned long long n[1] = {mhl_once(n_open)};
    df_mesh_block_add(a.fill_counts, slot, n);
    const int mslot[2] = {5, 6};
    const uint32_t m[2] = {top_filled, top_open};
    df_mesh_block_max(a.fill_counts, mslot, m);
}

__global__ __launch_bounds__(256) void df_mhl_fill_kernel(const DfMhlArgs a)
{
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v <= a.V; v += (size_t)gridDim.x * 256) {
        if (v == a.V) {
            const unsigned long long filled = a.sel[v], added = a.toff[v];
            a.fill_counts[0] = (unsigned long long)a.V + filled;
            a.fill_counts[1] = (unsigned long long)a.T + added;
            a.fill_counts[2] = filled;
            a.fill_counts[4] = added;
            a.fill_counts[7] = a.counts[4];
            continue;
        }
        if (a.vsrc && (unsigned long long)v < a.out_vcap) a.vsrc[v] = (uint32_t)v;
        const uint32_t l = a.lab[v];
        if (l == DF_MHL_NONE) continue;
        const uint32_t L = a.len[l];
        if (L > a.max_edges) continue;
        const unsigned long long m = (unsigned long long)a.V + a.sel[l];
        const unsigned long long t = (unsigned long long)a.T + a.toff[l] + a.rnk[v];
        if (t < a.out_tcap) {
            a.out_t[3 * t] = a.next[v]; a.out_t[3 * t + 1] = (uint32_t)v; a.out_t[3 * t + 2] = (uint32_t)m;
        }
        if ((uint32_t)v == l && m < a.out_vcap) {
            float ax = 0.f, ay = 0.f, az = 0.f;
            uint32_t u = l;
            for (uint32_t j = 0; j < L; ++j) {                           // rank order: the label vertex first
                const float4 p = a.P[u];
                ax = ax + p.x; ay = ay + p.y; az = az + p.z;
                u = a.next[u];
            }
            const float n = (float)L;
            a.out_v[m] = make_float4(ax / n, ay / n, az / n, 0.f);       // IEEE f32 division
            if (a.vsrc) a.vsrc[m] = DF_MHL_NONE;
        }
    }
}

extern "C" int dfusion_mesh_fill_holes(const float* vertices_dev, unsigned long long n_vertices, const unsigned int* triangles_dev,
                                       unsigned long long n_triangles, unsigned int max_edges, unsigned int flags, float* vertices_out_dev,
                                       unsigned long long vertex_capacity, unsigned int* triangles_out_dev, unsigned long long triangle_capacity,
                                       unsigned int* vertex_src_dev, unsigned long long* counts_dev, dfStream stream)
{
    if (flags || n_vertices > 0xffffffffull || n_triangles > 0xffffffffull / 6ull || !counts_dev) return DF_E_INVALID;
    if (vertex_capacity > 0xffffffffull || triangle_capacity > 0xffffffffull) return DF_E_INVALID;
    if ((n_vertices && !vertices_dev) || (n_triangles && !triangles_dev)) return DF_E_INVALID;
    if ((vertex_capacity && !vertices_out_dev) || (triangle_capacity && !triangles_out_dev)) return DF_E_INVALID;
    const size_t V = (size_t)n_vertices, T = (size_t)n_triangles, N = 6 * T;
    const struct { const void* p; size_t n; } outs[4] = {{vertices_out_dev, (size_t)vertex_capacity * 16}, {triangles_out_dev, (size_t)triangle_capacity * 12},
                                                         {vertex_src_dev, (size_t)vertex_capacity * 4}, {counts_dev, 64}};
    for (const auto& o : outs)
        if (df_mesh_overlap(vertices_dev, V * 16, o.p, o.n) || df_mesh_overlap(triangles_dev, T * 12, o.p, o.n)) return DF_E_INVALID;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return DF_E_NO_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    const bool write = vertex_capacity || triangle_capacity;             // both 0: counts only
    DF_HIP(hipMemsetAsync(counts_dev, 0, 64, st));
    if (write) {                                                          // the old arrays go across as they are
        const size_t nv = V < vertex_capacity ? V : (size_t)vertex_capacity, nt = T < triangle_capacity ? T : (size_t)triangle_capacity;
        if (nv) DF_HIP(hipMemcpyAsync(vertices_out_dev, vertices_dev, nv * 16, hipMemcpyDeviceToDevice, st));
        if (nt) DF_HIP(hipMemcpyAsync(triangles_out_dev, triangles_dev, nt * 12, hipMemcpyDeviceToDevice, st));
    }
    DfMhlArgs a;
    memset(&a, 0, sizeof(a));
    a.V = V; a.N = N; a.T = T; a.k = df_msm_key_bits(V);
    a.max_edges = max_edges;
    a.P = (const float4*)vertices_dev; a.tris = triangles_dev;
    a.out_v = (float4*)vertices_out_dev; a.out_t = triangles_out_dev; a.vsrc = write ? vertex_src_dev : nullptr;
    a.out_vcap = vertex_capacity; a.out_tcap = triangle_capacity;
    a.fill_counts = counts_dev;
    if (!V || !T) {                                                       // nothing to fill: the mesh is copied
        DF_TRY(df_mesh_set_counts(counts_dev, 0, n_vertices, 1, n_triangles, st));
        if (a.vsrc && V) {                                                // vertex_src = 0 .. V - 1: the fill kernel over no loop
            DfMeshCarve c;                                                // [lab: no loop] [sel, toff, the loop stage's counts: zeroed]
            const size_t o_lab = c.take(V * 4), o_sel = c.take((V + 1) * 4), o_toff = c.take((V + 1) * 4), o_counts = c.take(64);
            DfScratchHold hold(st, c.total());
            if (!hold.entry) return (int)hipErrorOutOfMemory;
            a.lab = (uint32_t*)(hold.mem + o_lab); a.sel = (uint32_t*)(hold.mem + o_sel); a.toff = (uint32_t*)(hold.mem + o_toff);
            a.counts = (unsigned long long*)(hold.mem + o_counts);
            DF_HIP(hipMemsetAsync(a.lab, 0xff, V * 4, st));
            DF_HIP(hipMemsetAsync(a.sel, 0, c.total() - o_sel, st));
            hipLaunchKernelGGL(df_mhl_fill_kernel, dim3(df_mesh_blocks(V + 1)), dim3(256), 0, st, a);
            DF_LAUNCH_CHECK();
        }
        return DF_OK;
    }
    DfMhlLayout l;
    DF_TRY(mhl_plan(V, N, a.k, st, &l));
    DfScratchHold hold(st, l.total);                                      // held until the last launch is enqueued
    if (!hold.entry) return (int)hipErrorOutOfMemory;
    a.counts = (unsigned long long*)(hold.mem + l.o_counts);
    DF_HIP(hipMemsetAsync(a.counts, 0, 64, st));
    DF_TRY(mhl_loops(a, triangles_dev, hold.mem, l, st));
    const dim3 gv(df_mesh_blocks(V + 1)), wg(256);
    hipLaunchKernelGGL(df_mhl_select_kernel, gv, wg, 0, st, a);
    DF_LAUNCH_CHECK();
    DF_TRY(df_mesh_scan_pair(hold.mem + l.o_cub, l.cub_bytes, a.sel, V + 1, a.toff, V + 1, nullptr, st));
    hipLaunchKernelGGL(df_mhl_fill_kernel, gv, wg, 0, st, a);
    DF_LAUNCH_CHECK();
    return DF_OK;
}
