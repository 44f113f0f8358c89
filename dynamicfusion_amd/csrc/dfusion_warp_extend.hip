// dfusion_warp_extend.hip -- growing the warp field: new deformation nodes where fused surface has no node near it
// (DynamicFusion, Newcombe et al. CVPR 2015, section 3.4 "extending the warp field").  The reference seeds its nodes once
// (warp_field.cpp:41-88) and never adds any; this is the paper's insertion, with a rule that is exact and deterministic
// (include/dfusion.h dfusion_warp_extend, DESIGN.md "Growing the warp field"):
//   * a finite point p is UNSUPPORTED when d2_i >= sigma_i^2 (f32) for each of its k nearest nodes (dfusion_knn, nanoflann's order);
//   * unsupported points are decimated to one per cell of the grid floor(p / radius): the lowest point index of a cell wins;
//   * winners become nodes in increasing index order, at most min(max_new, 65535 - M) of them: vertex = p, dg_w = sigma_new,
//     transform = WarpField::DQB(p) over the OLD node set (warp_field.cpp:203-217), or, when all k weights are 0, the transform of p's
//     nearest node.
// The handle then takes the grown set (df_warp_grow, dfusion_warp_index.hip): node arrays re-packed with headroom, tie tree re-made, brick lists
// re-made, and only the table blocks whose brick list changed or whose build met an exact distance tie marked unbuilt -- every result
// is what dfusion_warp_set_nodes + dfusion_warp_build_index make of the grown set on a fresh handle.
//
// Device work, all on the caller's stream: a pass that sanitises the queries (non-finite -> origin, their k-NN is never looked at),
// dfusion_knn, a claim pass (support test, cell, per-cell winner by integer atomicMin into an open-addressing table keyed by the first
// point that claimed the slot), count / scan / compact passes (winners in index order), and one thread per new node for the blend.
#include "dfusion_internal.h"
#include <math.h>

#define DF_EXT_WG 256
#define DF_EXT_CELL_LIM 1073741824.f       // 2^30: points with |p / radius| >= this on an axis take no part

__global__ __launch_bounds__(DF_EXT_WG) void df_ext_sanitize_kernel(const float* __restrict__ points, int N, float* __restrict__ q)
{
    const int i = blockIdx.x * DF_EXT_WG + threadIdx.x;
    if (i >= N) return;
    const float x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
    const bool fin = isfinite(x) && isfinite(y) && isfinite(z);
    q[3 * (size_t)i] = fin ? x : 0.f; q[3 * (size_t)i + 1] = fin ? y : 0.f; q[3 * (size_t)i + 2] = fin ? z : 0.f;
}

// cell of p, false if p takes no part (not finite, or beyond 2^30 cells from the origin on an axis)
__device__ __forceinline__ bool df_ext_cell(const float* __restrict__ points, int i, float radius, int (&c)[3])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float f = points[3 * (size_t)i + a] / radius;           // IEEE f32 division (-fno-fast-math)
        if (!(fabsf(f) < DF_EXT_CELL_LIM)) return false;                 // (NaN and inf fail this too)
        c[a] = (int)floorf(f);
    }
    return true;
}

// One thread per point: slot_of[i] = the table slot of p's cell if p is an unsupported candidate, else -1; min_idx[slot] = the
// lowest candidate index of the cell.  A slot belongs to the first point that claims it (owner = index + 1); its cell is that point's
// cell, recomputed from the (read-only) input, so no key has to be published beside the claim.
__global__ __launch_bounds__(DF_EXT_WG) void df_ext_claim_kernel(const float* __restrict__ points, int N, float radius, int k,
                                                                 const int* __restrict__ idx, const float* __restrict__ d2,
                                                                 const float4* __restrict__ pos_sigma, unsigned* __restrict__ owner,
                                                                 int* __restrict__ min_idx, unsigned tmask, int* __restrict__ slot_of)
{
    const int i = blockIdx.x * DF_EXT_WG + threadIdx.x;
    if (i >= N) return;
    int slot = -1, c[3];
    const float x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
    bool cand = (x == x) && (y == y) && (z == z) && df_ext_cell(points, i, radius, c);
    for (int j = 0; cand && j < k; ++j) {
        const float s = pos_sigma[idx[(size_t)i * k + j]].w;
        cand = d2[(size_t)i * k + j] >= s * s;                          // a node within its own dg_w supports p
    }
    if (cand) {
        unsigned h = (unsigned)c[0] * 73856093u ^ (unsigned)c[1] * 19349663u ^ (unsigned)c[2] * 83492791u;
        h = (h ^ (h >> 15)) * 0x2c1b3c6du;
        h = (h ^ (h >> 12)) & tmask;
        for (;;) {                                                      // the table has > 2N slots: a free one is always found
            const unsigned prev = atomicCAS(&owner[h], 0u, (unsigned)i + 1u);
            bool same = prev == 0u;
            if (!same) {
                int o[3];
                (void)df_ext_cell(points, (int)prev - 1, radius, o);
                same = o[0] == c[0] && o[1] == c[1] && o[2] == c[2];
            }
            if (same) { atomicMin(&min_idx[h], i); slot = (int)h; break; }
            h = (h + 1u) & tmask;
        }
    }
    slot_of[i] = slot;
}

__device__ __forceinline__ bool df_ext_winner(const int* __restrict__ slot_of, const int* __restrict__ min_idx, int i, int N)
{
    if (i >= N) return false;
    const int s = slot_of[i];
    return s >= 0 && min_idx[s] == i;
}

__global__ __launch_bounds__(DF_EXT_WG) void df_ext_count_kernel(const int* __restrict__ slot_of, const int* __restrict__ min_idx, int N,
                                                                 unsigned* __restrict__ blk_cnt)
{
    const int i = blockIdx.x * DF_EXT_WG + threadIdx.x;
    const int n = __syncthreads_count(df_ext_winner(slot_of, min_idx, i, N));
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = (unsigned)n;
}

// exclusive scan of nb block counts in one workgroup (each thread a contiguous run); off[nb] = the total
__global__ __launch_bounds__(1024) void df_ext_scan_kernel(const unsigned* __restrict__ cnt, unsigned* __restrict__ off, int nb)
{
    __shared__ unsigned s[1024];
    const int per = (nb + 1023) / 1024, b0 = threadIdx.x * per, b1 = min(b0 + per, nb);
    unsigned sum = 0;
    for (int b = b0; b < b1; ++b) sum += cnt[b];
    s[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                                // Hillis-Steele, inclusive
        const unsigned v = threadIdx.x >= (unsigned)o ? s[threadIdx.x - o] : 0u;
        __syncthreads();
        s[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned run = s[threadIdx.x] - sum;
    for (int b = b0; b < b1; ++b) { off[b] = run; run += cnt[b]; }
    if (threadIdx.x == 1023) off[nb] = s[1023];
}

// winners in index order: rank = the block's offset + winners before it in the block; the first `take` ranks are kept
__global__ __launch_bounds__(DF_EXT_WG) void df_ext_compact_kernel(const int* __restrict__ slot_of, const int* __restrict__ min_idx, int N,
                                                                   const unsigned* __restrict__ blk_off, unsigned take, int* __restrict__ win)
{
    __shared__ unsigned s_wave[DF_EXT_WG / 64];
    const int i = blockIdx.x * DF_EXT_WG + threadIdx.x;
    const bool w = df_ext_winner(slot_of, min_idx, i, N);
    const unsigned long long bal = __ballot(w);
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) s_wave[wave] = (unsigned)__popcll(bal);
    __syncthreads();
    unsigned r = blk_off[blockIdx.x] + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
    for (unsigned v = 0; v < wave; ++v) r += s_wave[v];
    if (w && r < take) win[r] = i;
}

// The grown node arrays in the layout dfusion_warp_set_nodes takes: the M old nodes as the handle holds them now ...
__global__ __launch_bounds__(DF_EXT_WG) void df_ext_copy_old_kernel(DfWarpView W, float* __restrict__ pos, float* __restrict__ dq,
                                                                    float* __restrict__ sigma)
{
    const int j = blockIdx.x * DF_EXT_WG + threadIdx.x;
    if (j >= W.M) return;
    const float4 ps = W.pos_sigma[j], r = W.rot[j], d = W.dual[j];
    pos[3 * (size_t)j] = ps.x; pos[3 * (size_t)j + 1] = ps.y; pos[3 * (size_t)j + 2] = ps.z; sigma[j] = ps.w;
    float* o = dq + 8 * (size_t)j;
    o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w; o[4] = d.x; o[5] = d.y; o[6] = d.z; o[7] = d.w;
}

// ... then one thread per new node: WarpField::DQB(p) over the old nodes with the helpers dfusion_warp_points blends with (dqb_weights,
// dqb_blend_w).  All k weights 0 (p beyond ~14 sigma of its neighbours: the rotation sum is 0 and the blend NaN) -> the transform of the
// nearest node.
template <int K>
__global__ __launch_bounds__(DF_EXT_WG) void df_ext_new_nodes_kernel(DfWarpView W, const float* __restrict__ points, const int* __restrict__ idx,
                                                                     const float* __restrict__ d2, const int* __restrict__ win, int n, float sigma_new,
                                                                     float* __restrict__ pos, float* __restrict__ dq, float* __restrict__ sigma)
{
    const int r = blockIdx.x * DF_EXT_WG + threadIdx.x;
    if (r >= n) return;
    const int i = win[r];
    const size_t o = (size_t)W.M + r;
    pos[3 * o] = points[3 * (size_t)i]; pos[3 * o + 1] = points[3 * (size_t)i + 1]; pos[3 * o + 2] = points[3 * (size_t)i + 2];
    sigma[o] = sigma_new;
    float bd[K], wt[K]; int bi[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { bi[j] = idx[(size_t)i * K + j]; bd[j] = d2[(size_t)i * K + j]; }
    dqb_weights<K>(W, bd, bi, wt);                                      // warp_field.cpp:238-241
    bool any = false;
#pragma unroll
    for (int j = 0; j < K; ++j) any = any || wt[j] != 0.f;
    float* out = dq + 8 * o;
    if (!any) {
        const float4 a = W.rot[bi[0]], b = W.dual[bi[0]];
        out[0] = a.x; out[1] = a.y; out[2] = a.z; out[3] = a.w; out[4] = b.x; out[5] = b.y; out[6] = b.z; out[7] = b.w;
        return;
    }
    quat rot, dual;
    dqb_blend_w<K>(W, wt, bi, &rot, &dual);                             // warp_field.cpp:203-217
    out[0] = rot.w; out[1] = rot.x; out[2] = rot.y; out[3] = rot.z;
    out[4] = dual.w; out[5] = dual.x; out[6] = dual.y; out[7] = dual.z;
}

static inline size_t df_ext_align(size_t x) { return (x + 255) & ~(size_t)255; }

#define DF_EXT_MAX_POINTS (1 << 28)         // points per call at most (the claim table has 2N..4N slots, counted in 32 bits)

// the handle's extend scratch, grown when too small (kept between calls)
static int df_ext_scratch(DfWarpField* wf, size_t bytes, char** out)
{
    int rc = wf->ext_ws.reserve(bytes);
    *out = wf->ext_ws;
    return rc;
}

extern "C" int dfusion_warp_extend(DfWarpField* wf, int k, const float* points, int N, float radius, float sigma_new, int max_new,
                                   float* new_pos, float* new_dq, float* new_sigma, int* n_added, int* n_winners, dfStream stream)
{
    if (!wf || !n_added || !n_winners) return DF_E_INVALID;
    *n_added = 0; *n_winners = 0;
    if (k < 1 || k > 8 || wf->M < k || N < 0 || N > DF_EXT_MAX_POINTS || (N > 0 && !points) || max_new < 0) return DF_E_INVALID;
    if (!(radius > 0.f) || !isfinite(radius) || !isfinite(sigma_new)) return DF_E_INVALID;
    if (N == 0) return DF_OK;
    hipStream_t st = (hipStream_t)stream;
    const int M = wf->M;
    const int cap = max_new < 65535 - M ? max_new : 65535 - M;             // nodes this call may add at most
    const int nb = (N + DF_EXT_WG - 1) / DF_EXT_WG;
    unsigned T = 1024;
    while (T < 2u * (unsigned)N) T <<= 1;                                   // (N <= 2^28: no wrap)
    const int Mmax = 65535;
    // scratch: queries [3N], k-NN [N k] ids + [N k] d2, slot_of [N], table owner [T] + min index [T], block counts [nb], offsets [nb + 1],
    // winners [min(cap, N)], then the grown node arrays pos [3 Mn], dq [8 Mn], sigma [Mn] (sized for the largest node set)
    const size_t o_q = 0, o_idx = o_q + df_ext_align((size_t)N * 12), o_d2 = o_idx + df_ext_align((size_t)N * k * 4),
                 o_slot = o_d2 + df_ext_align((size_t)N * k * 4), o_own = o_slot + df_ext_align((size_t)N * 4),
                 o_min = o_own + df_ext_align((size_t)T * 4), o_cnt = o_min + df_ext_align((size_t)T * 4),
                 o_off = o_cnt + df_ext_align((size_t)nb * 4), o_win = o_off + df_ext_align(((size_t)nb + 1) * 4),
                 o_pos = o_win + df_ext_align((size_t)(cap < N ? cap : N) * 4 + 4), o_dq = o_pos + df_ext_align((size_t)Mmax * 12),
                 o_sig = o_dq + df_ext_align((size_t)Mmax * 32), total_bytes = o_sig + df_ext_align((size_t)Mmax * 4);
    char* base = nullptr;
    { int rc = df_ext_scratch(wf, total_bytes, &base); if (rc) return rc; }
    float* q = (float*)(base + o_q); int* idx = (int*)(base + o_idx); float* d2 = (float*)(base + o_d2);
    int* slot_of = (int*)(base + o_slot); unsigned* owner = (unsigned*)(base + o_own); int* min_idx = (int*)(base + o_min);
    unsigned* blk_cnt = (unsigned*)(base + o_cnt); unsigned* blk_off = (unsigned*)(base + o_off); int* win = (int*)(base + o_win);
    float* gpos = (float*)(base + o_pos); float* gdq = (float*)(base + o_dq); float* gsig = (float*)(base + o_sig);
    DF_HIP(hipMemsetAsync(owner, 0, (size_t)T * 4, st));
    DF_HIP(hipMemsetAsync(min_idx, 0x7f, (size_t)T * 4, st));             // 0x7f7f7f7f > every point index
    hipLaunchKernelGGL(df_ext_sanitize_kernel, dim3(nb), dim3(DF_EXT_WG), 0, st, points, N, q);
    DF_LAUNCH_CHECK();
    { int rc = dfusion_knn(wf, k, q, N, idx, d2, stream); if (rc) return rc; }
    hipLaunchKernelGGL(df_ext_claim_kernel, dim3(nb), dim3(DF_EXT_WG), 0, st, points, N, radius, k, idx, d2, wf->pos_sigma, owner, min_idx,
                       T - 1u, slot_of);
    hipLaunchKernelGGL(df_ext_count_kernel, dim3(nb), dim3(DF_EXT_WG), 0, st, slot_of, min_idx, N, blk_cnt);
    hipLaunchKernelGGL(df_ext_scan_kernel, dim3(1), dim3(1024), 0, st, blk_cnt, blk_off, nb);
    hipLaunchKernelGGL(df_ext_compact_kernel, dim3(nb), dim3(DF_EXT_WG), 0, st, slot_of, min_idx, N, blk_off, (unsigned)cap, win);
    DF_LAUNCH_CHECK();
    unsigned total = 0;
    DF_HIP(hipMemcpyAsync(&total, blk_off + nb, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    DF_HIP(hipStreamSynchronize(st));
    const int n = (int)total < cap ? (int)total : cap;
    *n_winners = (int)total;
    if (n == 0) return DF_OK;                                               // nothing added: the handle is untouched

    const int Mn = M + n;
    DfWarpView W;
    memset(&W, 0, sizeof(W));
    W.pos_sigma = wf->pos_sigma; W.rot = wf->rot; W.dual = wf->dual; W.node_t = wf->node_t; W.M = M;
    hipLaunchKernelGGL(df_ext_copy_old_kernel, dim3((M + DF_EXT_WG - 1) / DF_EXT_WG), dim3(DF_EXT_WG), 0, st, W, gpos, gdq, gsig);
    const dim3 g((n + DF_EXT_WG - 1) / DF_EXT_WG);
    switch (k) {
        case 1: df_ext_new_nodes_kernel<1><<<g, DF_EXT_WG, 0, st>>>(W, points, idx, d2, win, n, sigma_new, gpos, gdq, gsig); break;
        case 2: df_ext_new_nodes_kernel<2><<<g, DF_EXT_WG, 0, st>>>(W, points, idx, d2, win, n, sigma_new, gpos, gdq, gsig); break;
        case 3: df_ext_new_nodes_kernel<3><<<g, DF_EXT_WG, 0, st>>>(W, points, idx, d2, win, n, sigma_new, gpos, gdq, gsig); break;
        case 4: df_ext_new_nodes_kernel<4><<<g, DF_EXT_WG, 0, st>>>(W, points, idx, d2, win, n, sigma_new, gpos, gdq, gsig); break;
        case 5: df_ext_new_nodes_kernel<5><<<g, DF_EXT_WG, 0, st>>>(W, points, idx, d2, win, n, sigma_new, gpos, gdq, gsig); break;
        case 6: df_ext_new_nodes_kernel<6><<<g, DF_EXT_WG, 0, st>>>(W, points, idx, d2, win, n, sigma_new, gpos, gdq, gsig); break;
        case 7: df_ext_new_nodes_kernel<7><<<g, DF_EXT_WG, 0, st>>>(W, points, idx, d2, win, n, sigma_new, gpos, gdq, gsig); break;
        default: df_ext_new_nodes_kernel<8><<<g, DF_EXT_WG, 0, st>>>(W, points, idx, d2, win, n, sigma_new, gpos, gdq, gsig); break;
    }
    DF_LAUNCH_CHECK();
    if (new_pos) DF_HIP(hipMemcpyAsync(new_pos, gpos + 3 * (size_t)M, (size_t)n * 12, hipMemcpyDeviceToDevice, st));
    if (new_dq) DF_HIP(hipMemcpyAsync(new_dq, gdq + 8 * (size_t)M, (size_t)n * 32, hipMemcpyDeviceToDevice, st));
    if (new_sigma) DF_HIP(hipMemcpyAsync(new_sigma, gsig + M, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    // the handle takes the grown set; its index, if any, is updated in place (dfusion_warp_index.hip df_warp_grow).  Once the nodes are in,
    // *n_added reports them even if the index update then fails (the handle then has no index: DF_E_NO_INDEX until build_index)
    const int rc = df_warp_grow(wf, gpos, gdq, gsig, Mn, st);
    if (wf->M == Mn) *n_added = n;
    return rc;
}
