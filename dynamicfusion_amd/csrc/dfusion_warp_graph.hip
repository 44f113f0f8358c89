// dfusion_warp_graph.hip -- the hierarchical node graph of the regularised warp solve (DynamicFusion, Newcombe et al. CVPR 2015,
// section 3.3 eq. 8 and section 3.4: the regularisation graph is a hierarchy of deformation nodes, each level a coarser subsampling of
// the one below, edges from a node to its nearest nodes one level up).  The rule is exact and deterministic (include/dfusion.h
// dfusion_warp_set_graph_hierarchy, DESIGN.md section 20, restated in tests/solver_hier_ref.py):
//   * S_0 = every node; S_l = one node per cell of the grid floor(p / c_l) among S_{l-1}, the lowest node index of a cell, c_1 = radius,
//     c_{l+1} = f32(c_l * beta) -- the decimation of dfusion_warp_extend; a node that is not finite, or |p / c_l| >= 2^30 on an axis, is
//     never a member; a c_l that overflows to infinity leaves level l and all above it empty;
//   * L' = the largest l <= levels with |S_l| >= kg + 1; top(i) = the highest l <= L' with i in S_l;
//   * node i's kg targets = the nearest members of S_t \ {i}, t = min(top(i) + 1, L'), by (d2, node index) ascending, d2 =
//     (dx dx + dy dy) + dz dz in f32, query minus candidate, a NaN d2 after every finite one.
// L' = 0 leaves the flat graph to its caller (dfusion_solver.hip df_sv_graph), which also makes the CSR transpose of either graph.
//
// Device work, all on the caller's stream: per level a claim pass (cell, per-cell winner by integer atomicMin into an open-addressing
// table keyed by the first node that claimed the slot), count / scan / compact passes (members and non-members, both in index order;
// the level sizes stay on the device, every pass is launched for M); then, the sizes read back once, per target level a brute-force
// k-NN of that level's queries (one per lane) over its member list staged through LDS, and one thread per node for the edges.
// The cascade follows the scheme of dfusion_warp_extend.hip; its passes are written out here because they run over the members of a
// level, read their count from the device and leave two lists, where extend's run over points behind a support test.
#include "dfusion_internal.h"
#include <math.h>

#define DF_HG_WG 256
#define DF_HG_CELL_LIM 1073741824.f        // 2^30: nodes with |p / c| >= this on an axis take no part
#define DF_HG_NAN_KEY 0x7fc00000u          // sort key of a NaN d2: above +inf (0x7f800000), below an empty entry
#define DF_HG_EMPTY_KEY 0xffffffffu

__global__ __launch_bounds__(DF_HG_WG) void df_hg_init_kernel(int M, int* __restrict__ top, int* __restrict__ sizes)
{
    const int i = blockIdx.x * DF_HG_WG + threadIdx.x;
    if (i < M) top[i] = 0;
    if (i <= DF_GRAPH_MAX_LEVELS) sizes[i] = i == 0 ? M : 0;
}

// cell of p, false if p takes no part (not finite, or beyond 2^30 cells from the origin on an axis)
__device__ __forceinline__ bool df_hg_cell(const float4 p, float c, int (&cell)[3])
{
    const float v[3] = {p.x, p.y, p.z};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float f = v[a] / c;                                        // IEEE f32 division (-fno-fast-math)
        if (!(fabsf(f) < DF_HG_CELL_LIM)) return false;                  // (NaN and inf fail this too)
        cell[a] = (int)floorf(f);
    }
    return true;
}

__device__ __forceinline__ int df_hg_member(const int* __restrict__ members, int m) { return members ? members[m] : m; }

// One thread per member m of the level below (members == nullptr: level 0, every node): slot_of[m] = the table slot of its cell, or -1;
// min_idx[slot] = the lowest node index of the cell.  A slot belongs to the first node that claims it (owner = index + 1); its cell is
// that node's cell, recomputed from the node positions, so no key has to be published beside the claim.
__global__ __launch_bounds__(DF_HG_WG) void df_hg_claim_kernel(const float4* __restrict__ pos_sigma, const int* __restrict__ members,
                                                               const int* __restrict__ n_dev, float c, unsigned* __restrict__ owner,
                                                               int* __restrict__ min_idx, unsigned tmask, int* __restrict__ slot_of)
{
    const int m = blockIdx.x * DF_HG_WG + threadIdx.x;
    if (m >= *n_dev) return;
    const int i = df_hg_member(members, m);
    int slot = -1, cell[3];
    if (df_hg_cell(pos_sigma[i], c, cell)) {
        unsigned h = (unsigned)cell[0] * 73856093u ^ (unsigned)cell[1] * 19349663u ^ (unsigned)cell[2] * 83492791u;
        h = (h ^ (h >> 15)) * 0x2c1b3c6du;
        h = (h ^ (h >> 12)) & tmask;
        for (;;) {                                                       // the table has >= 2M slots: a free one is always found
            const unsigned prev = atomicCAS(&owner[h], 0u, (unsigned)i + 1u);
            bool same = prev == 0u;
            if (!same) {
                int o[3];
                (void)df_hg_cell(pos_sigma[(int)prev - 1], c, o);
                same = o[0] == cell[0] && o[1] == cell[1] && o[2] == cell[2];
            }
            if (same) { atomicMin(&min_idx[h], i); slot = (int)h; break; }
            h = (h + 1u) & tmask;
        }
    }
    slot_of[m] = slot;
}

__device__ __forceinline__ bool df_hg_winner(const int* __restrict__ members, const int* __restrict__ slot_of, const int* __restrict__ min_idx,
                                             int m, int n)
{
    if (m >= n) return false;
    const int s = slot_of[m];
    return s >= 0 && min_idx[s] == df_hg_member(members, m);
}

__global__ __launch_bounds__(DF_HG_WG) void df_hg_count_kernel(const int* __restrict__ members, const int* __restrict__ slot_of,
                                                               const int* __restrict__ min_idx, const int* __restrict__ n_dev,
                                                               unsigned* __restrict__ blk_cnt)
{
    const int m = blockIdx.x * DF_HG_WG + threadIdx.x;
    const int n = __syncthreads_count(df_hg_winner(members, slot_of, min_idx, m, *n_dev));
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = (unsigned)n;
}

// exclusive scan of nb block counts in one workgroup (each thread a contiguous run); *total_out = the level's size
__global__ __launch_bounds__(DF_HG_WG) void df_hg_scan_kernel(const unsigned* __restrict__ cnt, unsigned* __restrict__ off, int nb,
                                                              int* __restrict__ total_out)
{
    __shared__ unsigned s[DF_HG_WG];
    const int per = (nb + DF_HG_WG - 1) / DF_HG_WG, b0 = min((int)threadIdx.x * per, nb), b1 = min(b0 + per, nb);
    unsigned sum = 0;
    for (int b = b0; b < b1; ++b) sum += cnt[b];
    s[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 1; o < DF_HG_WG; o <<= 1) {                             // Hillis-Steele, inclusive
        const unsigned v = threadIdx.x >= (unsigned)o ? s[threadIdx.x - o] : 0u;
        __syncthreads();
        s[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned run = s[threadIdx.x] - sum;
    for (int b = b0; b < b1; ++b) { off[b] = run; run += cnt[b]; }
    if (threadIdx.x == DF_HG_WG - 1) *total_out = (int)s[DF_HG_WG - 1];
}

// members of the new level in index order (rank = the block's offset + winners before it in the block), top = the level for them; the
// others of the level below, in index order too, are the queries whose target level this is
__global__ __launch_bounds__(DF_HG_WG) void df_hg_compact_kernel(const int* __restrict__ members, const int* __restrict__ slot_of,
                                                                 const int* __restrict__ min_idx, const int* __restrict__ n_dev,
                                                                 const unsigned* __restrict__ blk_off, int level, int* __restrict__ win,
                                                                 int* __restrict__ rest, int* __restrict__ top)
{
    __shared__ unsigned s_wave[DF_HG_WG / 64];
    const int m = blockIdx.x * DF_HG_WG + threadIdx.x, n = *n_dev;
    const bool w = df_hg_winner(members, slot_of, min_idx, m, n);
    const unsigned long long bal = __ballot(w);
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) s_wave[wave] = (unsigned)__popcll(bal);
    __syncthreads();
    unsigned r = blk_off[blockIdx.x] + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
    for (unsigned v = 0; v < wave; ++v) r += s_wave[v];
    if (m >= n) return;
    const int i = df_hg_member(members, m);
    if (w) { win[r] = i; top[i] = level; }
    else rest[(unsigned)m - r] = i;
}

__global__ __launch_bounds__(DF_HG_WG) void df_hg_clamp_top_kernel(int* __restrict__ top, int M, int eff)
{
    const int i = blockIdx.x * DF_HG_WG + threadIdx.x;
    if (i < M) top[i] = min(top[i], eff);
}

// One query per lane: the KG nearest of the nc candidates without the query itself, by (d2, node index).  A tile of 256 candidate
// positions (with the node index in .w) goes through LDS and every lane reads the same entry at a time (a broadcast); each lane keeps
// its sorted top-KG in registers and a candidate enters only where it is strictly less, so candidates in ascending index order leave
// ties in index order.
template <int KG>
__global__ __launch_bounds__(DF_HG_WG) void df_hg_knn_kernel(const float4* __restrict__ pos_sigma, const int* __restrict__ queries, int nq,
                                                             const int* __restrict__ cands, int nc, int* __restrict__ tgt)
{
    __shared__ float4 s_c[DF_HG_WG];
    const int q = blockIdx.x * DF_HG_WG + threadIdx.x;
    const bool live = q < nq;
    const int i = live ? df_hg_member(queries, q) : -1;
    const float4 pq = live ? pos_sigma[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    unsigned bk[KG]; int bi[KG];
#pragma unroll
    for (int s = 0; s < KG; ++s) { bk[s] = DF_HG_EMPTY_KEY; bi[s] = 0; }
    for (int t0 = 0; t0 < nc; t0 += DF_HG_WG) {
        __syncthreads();                                                 // (the tile before is read out)
        const int c = t0 + (int)threadIdx.x;
        if (c < nc) {
            const int j = cands[c];
            const float4 p = pos_sigma[j];
            s_c[threadIdx.x] = make_float4(p.x, p.y, p.z, __int_as_float(j));
        }
        __syncthreads();
        const int nt = min(DF_HG_WG, nc - t0);
        if (live) for (int u = 0; u < nt; ++u) {
            const float4 cp = s_c[u];
            const int j = __float_as_int(cp.w);
            const float dx = pq.x - cp.x, dy = pq.y - cp.y, dz = pq.z - cp.z;
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            const unsigned key = d2 != d2 ? DF_HG_NAN_KEY : __float_as_uint(d2);    // (d2 >= +0: its bits order as it does)
            if (j != i && key < bk[KG - 1]) {
                bk[KG - 1] = key; bi[KG - 1] = j;
#pragma unroll
                for (int s = KG - 1; s > 0; --s) {
                    if (bk[s] < bk[s - 1]) {
                        const unsigned tk = bk[s]; bk[s] = bk[s - 1]; bk[s - 1] = tk;
                        const int ti = bi[s]; bi[s] = bi[s - 1]; bi[s - 1] = ti;
                    }
                }
            }
        }
    }
    if (live) {
#pragma unroll
        for (int s = 0; s < KG; ++s) tgt[(size_t)i * KG + s] = bi[s];
    }
}

// the edges in the layout of df_sv_graph_kernel (dfusion_solver.hip): e = i * kg + s, the sort's keys (head node) and values (edge id)
__global__ __launch_bounds__(DF_HG_WG) void df_hg_edges_kernel(const int* __restrict__ tgt, const float4* __restrict__ pos_sigma, int M, int kg,
                                                               int* __restrict__ nbr, float* __restrict__ alpha, unsigned int* __restrict__ keys,
                                                               unsigned int* __restrict__ vals)
{
    const int i = blockIdx.x * DF_HG_WG + threadIdx.x;
    if (i >= M) return;
    const float si = pos_sigma[i].w;
    for (int s = 0; s < kg; ++s) {
        const int e = i * kg + s;
        const int j = min(max(tgt[e], 0), M - 1);
        nbr[e] = j;
        alpha[e] = fmaxf(si, pos_sigma[j].w);
        keys[e] = (unsigned int)j; vals[e] = (unsigned int)e;
    }
}

static inline size_t df_hg_align(size_t x) { return (x + 255) & ~(size_t)255; }

// The level cascade and, where L' > 0, the edges: wf->graph_top, graph_sizes and graph_eff are set; with graph_eff > 0 also
// graph_nbr / graph_alpha and the sort's keys / vals [M * kg].  graph_eff == 0: the caller builds the flat graph.  Blocks once, to read
// the level sizes.
int df_hg_build(DfWarpField* wf, int kg, unsigned int* keys, unsigned int* vals, hipStream_t st)
{
    const int M = wf->M, L = wf->hier_levels;
    const int nb = (M + DF_HG_WG - 1) / DF_HG_WG;
    unsigned T = 1024;
    while (T < 2u * (unsigned)M) T <<= 1;                                  // (M <= 65535)
    // scratch: table owner [T] + min index [T], slot_of [M], block counts [nb], offsets [nb], level sizes [9], k-NN targets [M kg],
    // then per level 1..L its members [M] and the non-members of the level below [M]
    const size_t o_own = 0, o_min = o_own + df_hg_align((size_t)T * 4), o_slot = o_min + df_hg_align((size_t)T * 4),
                 o_cnt = o_slot + df_hg_align((size_t)M * 4), o_off = o_cnt + df_hg_align((size_t)nb * 4),
                 o_size = o_off + df_hg_align((size_t)nb * 4), o_tgt = o_size + df_hg_align((DF_GRAPH_MAX_LEVELS + 1) * 4),
                 o_list = o_tgt + df_hg_align((size_t)M * kg * 4), list_bytes = df_hg_align((size_t)M * 4),
                 total_bytes = o_list + 2 * (size_t)L * list_bytes;
    int rc;
    if ((rc = wf->graph_hws.reserve(total_bytes)) || (rc = wf->graph_top.reserve((size_t)M))) return rc;
    char* base = wf->graph_hws;
    unsigned* owner = (unsigned*)(base + o_own); int* min_idx = (int*)(base + o_min); int* slot_of = (int*)(base + o_slot);
    unsigned* blk_cnt = (unsigned*)(base + o_cnt); unsigned* blk_off = (unsigned*)(base + o_off); int* sizes = (int*)(base + o_size);
    int* tgt = (int*)(base + o_tgt);
    auto members = [&](int l) { return l == 0 ? (int*)nullptr : (int*)(base + o_list + (size_t)(2 * (l - 1)) * list_bytes); };
    auto rest = [&](int l) { return (int*)(base + o_list + (size_t)(2 * (l - 1) + 1) * list_bytes); };   // S_{l-1} \ S_l
    int* top = wf->graph_top;
    const dim3 gM(nb), wg(DF_HG_WG);
    hipLaunchKernelGGL(df_hg_init_kernel, dim3((unsigned)((M > DF_GRAPH_MAX_LEVELS ? M : DF_GRAPH_MAX_LEVELS + 1) + DF_HG_WG - 1) / DF_HG_WG), wg, 0, st,
                       M, top, sizes);
    float c = wf->hier_radius;
    for (int l = 1; l <= L && isfinite(c); ++l, c = c * wf->hier_beta) {
        DF_HIP(hipMemsetAsync(owner, 0, (size_t)T * 4, st));
        DF_HIP(hipMemsetAsync(min_idx, 0x7f, (size_t)T * 4, st));         // 0x7f7f7f7f > every node index
        hipLaunchKernelGGL(df_hg_claim_kernel, gM, wg, 0, st, wf->pos_sigma.p, members(l - 1), sizes + l - 1, c, owner, min_idx, T - 1u, slot_of);
        hipLaunchKernelGGL(df_hg_count_kernel, gM, wg, 0, st, members(l - 1), slot_of, min_idx, sizes + l - 1, blk_cnt);
        hipLaunchKernelGGL(df_hg_scan_kernel, dim3(1), wg, 0, st, blk_cnt, blk_off, nb, sizes + l);
        hipLaunchKernelGGL(df_hg_compact_kernel, gM, wg, 0, st, members(l - 1), slot_of, min_idx, sizes + l - 1, blk_off, l, members(l), rest(l), top);
    }
    DF_LAUNCH_CHECK();
    DF_HIP(hipMemcpyAsync(wf->graph_sizes, sizes, sizeof(wf->graph_sizes), hipMemcpyDeviceToHost, st));
    DF_HIP(hipStreamSynchronize(st));
    int eff = 0;
    for (int l = 1; l <= L; ++l) if (wf->graph_sizes[l] >= kg + 1) eff = l;
    wf->graph_eff = eff;
    hipLaunchKernelGGL(df_hg_clamp_top_kernel, gM, wg, 0, st, top, M, eff);
    DF_LAUNCH_CHECK();
    if (eff == 0) return DF_OK;
    // target level t: the queries are S_{t-1} \ S_t, and for t = L' all of S_{L'-1} (a member of S_L' looks among the other members)
    for (int t = 1; t <= eff; ++t) {
        const bool last = t == eff;
        const int nq = last ? wf->graph_sizes[t - 1] : wf->graph_sizes[t - 1] - wf->graph_sizes[t], nc = wf->graph_sizes[t];
        if (nq == 0) continue;
        const int* queries = last ? members(t - 1) : rest(t);              // (nullptr with L' = 1: every node, in index order)
        const dim3 gq((nq + DF_HG_WG - 1) / DF_HG_WG);
        switch (kg) {
            case 1: hipLaunchKernelGGL(df_hg_knn_kernel<1>, gq, wg, 0, st, wf->pos_sigma.p, queries, nq, members(t), nc, tgt); break;
            case 2: hipLaunchKernelGGL(df_hg_knn_kernel<2>, gq, wg, 0, st, wf->pos_sigma.p, queries, nq, members(t), nc, tgt); break;
            case 3: hipLaunchKernelGGL(df_hg_knn_kernel<3>, gq, wg, 0, st, wf->pos_sigma.p, queries, nq, members(t), nc, tgt); break;
            case 4: hipLaunchKernelGGL(df_hg_knn_kernel<4>, gq, wg, 0, st, wf->pos_sigma.p, queries, nq, members(t), nc, tgt); break;
            case 5: hipLaunchKernelGGL(df_hg_knn_kernel<5>, gq, wg, 0, st, wf->pos_sigma.p, queries, nq, members(t), nc, tgt); break;
            case 6: hipLaunchKernelGGL(df_hg_knn_kernel<6>, gq, wg, 0, st, wf->pos_sigma.p, queries, nq, members(t), nc, tgt); break;
            case 7: hipLaunchKernelGGL(df_hg_knn_kernel<7>, gq, wg, 0, st, wf->pos_sigma.p, queries, nq, members(t), nc, tgt); break;
            default: return DF_E_INVALID;
        }
    }
    hipLaunchKernelGGL(df_hg_edges_kernel, gM, wg, 0, st, tgt, wf->pos_sigma.p, M, kg, wf->graph_nbr.p, wf->graph_alpha.p, keys, vals);
    DF_LAUNCH_CHECK();
    return DF_OK;
}

extern "C" int dfusion_warp_set_graph_hierarchy(DfWarpField* wf, int levels, float radius, float beta)
{
    if (!wf || levels < 0 || levels > DF_GRAPH_MAX_LEVELS) return DF_E_INVALID;
    if (levels > 0 && (!(radius > 0.f) || !isfinite(radius) || !(beta >= 1.f) || !isfinite(beta))) return DF_E_INVALID;
    wf->hier_levels = levels; wf->hier_radius = radius; wf->hier_beta = beta;
    wf->graph_kg = 0;
    return DF_OK;
}
