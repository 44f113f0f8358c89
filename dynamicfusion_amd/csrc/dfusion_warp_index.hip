// dfusion_warp_index.hip -- the exact k-NN brick index (dfusion_warp_build_index) and its update when the node set grows.
//
// MI355X design notes
//   * k-NN: a kd-tree walk is pointer-chasing and divergent.  Instead, for every 8^3 voxel brick
//     the index stores the EXACT candidate set {n : |n - c_B| <= D_k(c_B) + 2 r_B} (c_B brick
//     centre, r_B half diagonal, D_k distance to the k-th nearest node).  Any node among the k
//     nearest of any voxel of the brick is in that set, so a brute-force top-k over the list is
//     the exact nanoflann answer.  Lists depend only on canonical node positions: they are
//     rebuilt when nodes are inserted, not per frame.  Built on the GPU, one wave per brick,
//     with wave-level k-th-smallest selection and ballot/popcount-prefix compaction.
#include "dfusion_internal.h"
#include "dfusion_warp_sweep.h"     // DfWarpedArgs (df_table_args) and, through it, dfusion_warp_topk.h: no kernel of it is launched here.
                                    // DF_TRACE_WG adds a member to DfWarpedArgs, so a variant build gives this file the define too (tools/build_variant.py)
#include <math.h>

// ====================================================================================== brick index build
struct DfIndexGeom {
    int X, Y, Z; int bx, by, bz;
    float vsx, vsy, vsz;
    DfAff vol2world;
    float r2x;            // 2 * half-diagonal of a brick's cell (metres), inflated
};

// Brick lists.  For brick b with centre c_b (of its voxel-centre lattice): D_k(c_b) = distance of the k-th nearest node; every node
// that can be among the k nearest of ANY voxel of the brick satisfies |n - c_b| <= D_k(c_b) + 2 r_B (g.r2x).  Two launches: counts
// (FILL = false: cnt[b], brick_thr[b] = that radius, brick_d1[b] = the nearest node's distance), then, after a scan, the lists in
// node-index order (FILL = true).  Made hierarchically: one workgroup per SUPER-BRICK of 4 x 4 x 4 bricks first gathers (in
// node-index order, into LDS) every node that can be on the list of ANY of its bricks, then each wave makes 16 bricks' lists from
// those few hundred nodes instead of all M (one wave per brick over all M nodes took 0.70 + 0.34 ms at 512^3 / 2000 nodes; 0.40 + 0.20).  With c_S the centre of the super-brick's brick centres and d = max_b |c_b - c_S|:
//     D_k(c_b) <= D_k(c_S) + d     (the k nodes within D_k(c_S) of c_S are within that of c_b)
//     a node on b's list has |n - c_b| <= D_k(c_b) + r2x, hence |n - c_S| <= D_k(c_S) + 2 d + r2x  -- the gather radius,
// and the k nearest nodes of every c_b are inside it too, so D_k(c_b) and with it every list come out exactly as from the full scan
// (same members, same order, same brick_thr).  A super-brick whose gather exceeds the LDS list scans all M nodes per brick.
#define DF_SUPER 4
#define DF_SUPER_CAP 1024
template <int K>
__device__ __forceinline__ float df_wave_kth_pop(float (&bd)[K], float* first)   // K-th (and the) smallest over the wave's per-lane sorted lists (destroys them)
{
    const int lane = threadIdx.x & 63;
    float dk2 = 0.f;
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const float m = wave_min_f32(bd[0]);
        dk2 = m;
        if (r == 0) *first = m;
        const unsigned long long who = __ballot(bd[0] == m);
        const int first = __ffsll((long long)who) - 1;
        if (lane == first) {
#pragma unroll
            for (int i = 0; i < K - 1; ++i) bd[i] = bd[i + 1];
            bd[K - 1] = __uint_as_float(0x7f800000u);
        }
    }
    return dk2;
}
template <int K, bool FILL>
__global__ __launch_bounds__(256) void df_brick_index_super_kernel(const float4* __restrict__ pos_sigma, int M, DfIndexGeom g, float super_d,
                                                                   uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off,
                                                                   uint16_t* __restrict__ list, float* __restrict__ brick_thr, float* __restrict__ brick_d1)
{
    __shared__ float4 s_pos[DF_SUPER_CAP];
    __shared__ uint16_t s_id[DF_SUPER_CAP];
    __shared__ float s_k[4][K];
    __shared__ uint32_t s_wcnt[4], s_total;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int sbx = (g.bx + DF_SUPER - 1) / DF_SUPER, sby = (g.by + DF_SUPER - 1) / DF_SUPER;
    const int sx = blockIdx.x % sbx, sy = (blockIdx.x / sbx) % sby, sz = blockIdx.x / (sbx * sby);
    // centre of the super-brick's brick-centre lattice (brick b's centre is voxel 8 b + 3.5)
    const f3 cS = aff_mul(g.vol2world, mk3(((float)(sx * DF_SUPER * DF_BRICK) + 15.5f) * g.vsx, ((float)(sy * DF_SUPER * DF_BRICK) + 15.5f) * g.vsy,
                                           ((float)(sz * DF_SUPER * DF_BRICK) + 15.5f) * g.vsz));
    // ---- D_k(c_S): per-thread top-K over a strided share, the K smallest of each wave, then the K-th of the 4 K values
    {
        float bd[K]; int bi[K];
        topk_init<K>(bd, bi);
        for (int j = t; j < M; j += 256) { const float4 p = pos_sigma[j]; topk_insert<K>(bd, bi, knn_dist2(cS, p.x, p.y, p.z), j); }
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const float m = wave_min_f32(bd[0]);
            if (lane == 0) s_k[wave][r] = m;
            const unsigned long long who = __ballot(bd[0] == m);
            const int first = __ffsll((long long)who) - 1;
            if (lane == first) {
#pragma unroll
                for (int i = 0; i < K - 1; ++i) bd[i] = bd[i + 1];
                bd[K - 1] = __uint_as_float(0x7f800000u);
            }
        }
    }
    __syncthreads();
    float dkS2;
    {   // rank of each of the 4 K values (ties by position): the one of rank K - 1 is the K-th smallest
        const float v = lane < 4 * K ? s_k[lane / K][lane % K] : __uint_as_float(0x7f800000u);
        int rank = 0;
#pragma unroll
        for (int i = 0; i < 4 * K; ++i) { const float o = s_k[i / K][i % K]; rank += (o < v || (o == v && i < lane)) ? 1 : 0; }
        const unsigned long long hit = __ballot(lane < 4 * K && rank == K - 1);
        dkS2 = __shfl(v, __ffsll((long long)hit) - 1, 64);
    }
    const float thrS = (sqrtf(dkS2) + 2.f * super_d + g.r2x) * 1.001f + 1e-5f;
    const float thrS2 = thrS * thrS;
    // ---- the gather, in node-index order
    if (t == 0) s_total = 0;
    __syncthreads();
    bool overflow = false;
    for (int base = 0; base < M; base += 256) {
        const int j = base + t;
        bool in = false; float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < M) { p = pos_sigma[j]; in = knn_dist2(cS, p.x, p.y, p.z) <= thrS2; }
        const unsigned long long m = __ballot(in);
        if (lane == 0) s_wcnt[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t o = s_total;
        for (int w = 0; w < wave; ++w) o += s_wcnt[w];
        o += (uint32_t)__popcll(m & lane_mask_lt());
        if (in && o < DF_SUPER_CAP) { s_pos[o] = p; s_id[o] = (uint16_t)j; }
        __syncthreads();
        if (t == 0) s_total += s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
        __syncthreads();
    }
    const int nS = (int)s_total;
    overflow = nS > DF_SUPER_CAP;
    // ---- 16 bricks per wave
    for (int q = wave; q < DF_SUPER * DF_SUPER * DF_SUPER; q += 4) {
        const int bxx = sx * DF_SUPER + (q & 3), byy = sy * DF_SUPER + ((q >> 2) & 3), bzz = sz * DF_SUPER + (q >> 4);
        if (bxx >= g.bx || byy >= g.by || bzz >= g.bz) continue;            // wave-uniform
        const int b = (bzz * g.by + byy) * g.bx + bxx;
        const f3 c = aff_mul(g.vol2world, mk3(((float)(bxx * DF_BRICK) + 3.5f) * g.vsx, ((float)(byy * DF_BRICK) + 3.5f) * g.vsy,
                                              ((float)(bzz * DF_BRICK) + 3.5f) * g.vsz));
        const int n = overflow ? M : nS;
        float thr, d1sq = 0.f;
        if (!FILL) {
            float bd[K]; int bi[K];
            topk_init<K>(bd, bi);
            for (int i = lane; i < n; i += 64) {
                const float4 p = overflow ? pos_sigma[i] : s_pos[i];
                topk_insert<K>(bd, bi, knn_dist2(c, p.x, p.y, p.z), i);
            }
            thr = (sqrtf(df_wave_kth_pop<K>(bd, &d1sq)) + g.r2x) * 1.0001f + 1e-6f;
        } else thr = brick_thr[b];
        const float thr2 = thr * thr;
        uint32_t total = 0;
        const uint32_t o = FILL ? off[b] : 0u;
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            bool in = false; int j = 0;
            if (i < n) { const float4 p = overflow ? pos_sigma[i] : s_pos[i]; j = overflow ? i : (int)s_id[i]; in = knn_dist2(c, p.x, p.y, p.z) <= thr2; }
            const unsigned long long m = __ballot(in);
            if (FILL && in) list[o + total + (uint32_t)__popcll(m & lane_mask_lt())] = (uint16_t)j;
            total += (uint32_t)__popcll(m);
        }
        if (!FILL && lane == 0) { cnt[b] = total; brick_thr[b] = thr; brick_d1[b] = sqrtf(d1sq) * 0.9999f; }   // (rounded down: a lower bound)
    }
}

// Exclusive scan of n counts into off[0..n] with ONE 1024-thread block (n <= a few million).
__global__ __launch_bounds__(1024) void df_scan_kernel(const uint32_t* __restrict__ cnt, uint32_t* __restrict__ off, int n)
{
    __shared__ uint32_t part[1024];
    const int t = threadIdx.x;
    const int per = (n + 1023) / 1024;
    const int b = t * per, e = min(b + per, n);
    uint32_t s = 0;
    for (int i = b; i < e; ++i) s += cnt[i];
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {                    // Hillis-Steele inclusive scan
        uint32_t v = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = t ? part[t - 1] : 0u;
    for (int i = b; i < e; ++i) { off[i] = run; run += cnt[i]; }
    if (t == 1023) off[n] = part[1023];
}

// The same over tiles of DF_SCAN_TILE counts: sums[b] = sum of tile b; then (after df_scan_kernel over the sums) off[i] = tile offset +
// exclusive scan inside the tile, off[n] = the total.
#define DF_SCAN_TILE 2048
__global__ __launch_bounds__(256) void df_scan_sums_kernel(const uint32_t* __restrict__ cnt, uint32_t* __restrict__ sums, int n)
{
    __shared__ uint32_t part[4];
    const int base = blockIdx.x * DF_SCAN_TILE;
    uint32_t s = 0;
#pragma unroll
    for (int i = 0; i < DF_SCAN_TILE / 256; ++i) { const int j = base + i * 256 + (int)threadIdx.x; s += j < n ? cnt[j] : 0u; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}
__global__ __launch_bounds__(256) void df_scan_apply_kernel(const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ sums_off,
                                                            uint32_t* __restrict__ off, int n, int ntile)
{
    __shared__ uint32_t wsum[4];
    constexpr int PER = DF_SCAN_TILE / 256;
    const int first = blockIdx.x * DF_SCAN_TILE + (int)threadIdx.x * PER;       // a thread owns PER consecutive counts
    uint32_t v[PER], s = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) { v[i] = first + i < n ? cnt[first + i] : 0u; s += v[i]; }
    uint32_t incl = s;                                                          // inclusive scan of the thread sums: wave, then workgroup
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o, 64); if ((int)(threadIdx.x & 63) >= o) incl += t; }
    if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t run = sums_off[blockIdx.x] + incl - s;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) run += wsum[w];
#pragma unroll
    for (int i = 0; i < PER; ++i) { if (first + i < n) off[first + i] = run; run += v[i]; }
    if (blockIdx.x == 0 && threadIdx.x == 0) off[n] = sums_off[ntile];
}

// The brick lists (and the geometry they were made for) of dfusion_warp_build_index, for the node set the handle holds; blocks until built.
int df_index_bricks(DfWarpField* wf, const DfVolume& v, const float vol2world[12], int k, hipStream_t st)
{
    DfIndexGeom g;
    g.X = v.dims[0]; g.Y = v.dims[1]; g.Z = v.dims[2];
    g.bx = (g.X + DF_BRICK - 1) / DF_BRICK; g.by = (g.Y + DF_BRICK - 1) / DF_BRICK; g.bz = (g.Z + DF_BRICK - 1) / DF_BRICK;
    g.vsx = v.voxel_size[0]; g.vsy = v.voxel_size[1]; g.vsz = v.voxel_size[2];
    g.vol2world = df_aff(vol2world);
    {   // half diagonal of a brick's CELL (8 voxels wide: every point that rounds to one of its voxels, not only the 8x8x8 voxel
        // centres, so that dfusion_knn / dfusion_warp_points can use the lists for arbitrary points) under vol2world
        double r = 0.0;
        for (int sx = -1; sx <= 1; sx += 2) for (int sy = -1; sy <= 1; sy += 2) for (int sz = -1; sz <= 1; sz += 2) {
            double ex = sx * 4.0 * g.vsx, ey = sy * 4.0 * g.vsy, ez = sz * 4.0 * g.vsz;
            double wx = vol2world[0] * ex + vol2world[1] * ey + vol2world[2] * ez;
            double wy = vol2world[3] * ex + vol2world[4] * ey + vol2world[5] * ez;
            double wz = vol2world[6] * ex + vol2world[7] * ey + vol2world[8] * ez;
            double d = sqrt(wx * wx + wy * wy + wz * wz);
            if (d > r) r = d;
        }
        g.r2x = (float)(2.0 * r * 1.0001 + 1e-6);
    }
    const size_t nb = (size_t)g.bx * g.by * g.bz;
    if (nb + 1 > wf->off_cap) {
        wf->off_cap = 0;
        { int rc = wf->brick_off.reserve(nb + 1); if (rc) return rc; }
        { int rc = wf->brick_cnt.reserve(nb + 1); if (rc) return rc; }
        { int rc = wf->brick_thr.reserve(2 * (nb + 1)); if (rc) return rc; }     // [nb + 1] list radii, then [nb + 1] nearest-node distances
        wf->off_cap = nb + 1;
    }
    // (one workgroup per 4 x 4 x 4 bricks; df_brick_index_kernel, one wave per brick over all M nodes, makes the same lists)
    const dim3 grid((unsigned)(((g.bx + DF_SUPER - 1) / DF_SUPER) * ((g.by + DF_SUPER - 1) / DF_SUPER) * ((g.bz + DF_SUPER - 1) / DF_SUPER)));
    float super_d;
    {   // largest distance of a brick centre from its super-brick's centre: the corner of the 3 x 3 x 3-brick lattice, under vol2world
        double r = 0.0;
        for (int sx = -1; sx <= 1; sx += 2) for (int sy = -1; sy <= 1; sy += 2) for (int sz = -1; sz <= 1; sz += 2) {
            const double ex = sx * 12.0 * g.vsx, ey = sy * 12.0 * g.vsy, ez = sz * 12.0 * g.vsz;
            const double wx = vol2world[0] * ex + vol2world[1] * ey + vol2world[2] * ez;
            const double wy = vol2world[3] * ex + vol2world[4] * ey + vol2world[5] * ez;
            const double wz = vol2world[6] * ex + vol2world[7] * ey + vol2world[8] * ez;
            const double d = sqrt(wx * wx + wy * wy + wz * wz);
            if (d > r) r = d;
        }
        super_d = (float)(r * 1.0001 + 1e-6);
    }
    DF_DISPATCH_K(k, df_brick_index_super_kernel<K, false><<<grid, dim3(256), 0, st>>>(wf->pos_sigma, wf->M, g, super_d, wf->brick_cnt,
                                                                                       (const uint32_t*)nullptr, (uint16_t*)nullptr, wf->brick_thr,
                                                                                       wf->brick_thr + wf->off_cap));
    DF_LAUNCH_CHECK();
    {   // exclusive scan of the counts: tile sums, a one-workgroup scan of those, then the tiles (388 us -> 3 short launches at 512^3)
        const int ntile = (int)((nb + DF_SCAN_TILE - 1) / DF_SCAN_TILE);
        if ((size_t)ntile + 1 > wf->scan_cap) {
            wf->scan_cap = 0;
            { int rc = wf->scan_tmp.reserve(2 * ((size_t)ntile + 1)); if (rc) return rc; }
            wf->scan_cap = (size_t)ntile + 1;
        }
        uint32_t* sums = wf->scan_tmp; uint32_t* sums_off = wf->scan_tmp + wf->scan_cap;
        hipLaunchKernelGGL(df_scan_sums_kernel, dim3((unsigned)ntile), dim3(256), 0, st, wf->brick_cnt, sums, (int)nb);
        hipLaunchKernelGGL(df_scan_kernel, dim3(1), dim3(1024), 0, st, sums, sums_off, ntile);
        hipLaunchKernelGGL(df_scan_apply_kernel, dim3((unsigned)ntile), dim3(256), 0, st, wf->brick_cnt, sums_off, wf->brick_off, (int)nb, ntile);
        DF_LAUNCH_CHECK();
    }
    uint32_t total = 0;
    DF_HIP(hipMemcpyAsync(&total, wf->brick_off + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    DF_HIP(hipStreamSynchronize(st));
    if ((size_t)total > wf->brick_list.cap) { int rc = wf->brick_list.reserve((size_t)total + (size_t)total / 8 + 1024); if (rc) return rc; }
    DF_DISPATCH_K(k, df_brick_index_super_kernel<K, true><<<grid, dim3(256), 0, st>>>(wf->pos_sigma, wf->M, g, super_d, (uint32_t*)nullptr,
                                                                                      (const uint32_t*)wf->brick_off, wf->brick_list, wf->brick_thr,
                                                                                      (float*)nullptr));
    DF_LAUNCH_CHECK();
    DF_HIP(hipStreamSynchronize(st));
    wf->bx = g.bx; wf->by = g.by; wf->bz = g.bz; wf->k_built = k;
    memcpy(wf->geom_dims, v.dims, sizeof(wf->geom_dims));
    memcpy(wf->geom_vs, v.voxel_size, sizeof(wf->geom_vs));
    memcpy(wf->geom_aff, vol2world, sizeof(wf->geom_aff));
    {   // world -> volume, for locating the brick of a query point (double adjugate; only used to pick a cell, never in results)
        const float* m = vol2world; double d[9];
        d[0] = (double)m[4] * m[8] - (double)m[5] * m[7]; d[1] = (double)m[2] * m[7] - (double)m[1] * m[8]; d[2] = (double)m[1] * m[5] - (double)m[2] * m[4];
        d[3] = (double)m[5] * m[6] - (double)m[3] * m[8]; d[4] = (double)m[0] * m[8] - (double)m[2] * m[6]; d[5] = (double)m[2] * m[3] - (double)m[0] * m[5];
        d[6] = (double)m[3] * m[7] - (double)m[4] * m[6]; d[7] = (double)m[1] * m[6] - (double)m[0] * m[7]; d[8] = (double)m[0] * m[4] - (double)m[1] * m[3];
        const double det = m[0] * d[0] + m[1] * d[3] + m[2] * d[6];
        wf->geom_inv_ok = fabs(det) > 1e-30;
        for (int i = 0; i < 9; ++i) wf->geom_inv[i] = (float)(d[i] / det);
        for (int i = 0; i < 3; ++i)
            wf->geom_inv[9 + i] = (float)-((d[3 * i] * m[9] + d[3 * i + 1] * m[10] + d[3 * i + 2] * m[11]) / det);
    }
    return DF_OK;
}

extern "C" int dfusion_warp_build_index(DfWarpField* wf, DfVolume v, const DfSlab* slab, const float vol2world[12], int k,
                                        unsigned flags, dfStream stream)
{
    if (!wf || !vol2world || wf->M <= 0 || k < 1 || k > 8 || wf->M < k) return DF_E_INVALID;
    if (v.dims[0] <= 0 || v.dims[1] <= 0 || v.dims[2] <= 0) return DF_E_INVALID;
    DfSlab sl = df_slab_or_full(v, slab);
    if (sl.z_own_n < 0 || sl.z_own0 < 0 || sl.z_own0 + sl.z_own_n > v.dims[2]) return DF_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    df_side_drain(wf);                                         // (look-ahead builds of the tables about to be re-made)
    wf->prep_valid = false;                                    // (a prepared plan points into the index and tables re-made here: ADVICE r5)
    { int rc = df_index_bricks(wf, v, vol2world, k, st); if (rc) return rc; }
    wf->index_flags = flags; wf->index_slab = sl;
    wf->index_valid = true;
    wf->tab_valid = false;
    wf->w_tab_valid = false;
    if (flags & (DF_INDEX_VOXEL_TABLE | DF_INDEX_WEIGHT_TABLE))
        return df_build_voxel_table(wf, v, sl, vol2world, k, (flags & DF_INDEX_WEIGHT_TABLE) != 0,
                                    (flags & DF_INDEX_TABLES_ON_DEMAND) != 0 && (flags & DF_INDEX_WEIGHT_TABLE) != 0, st);
    return DF_OK;
}

extern "C" int dfusion_warp_index_info(const DfWarpField* wf, unsigned long long* total_entries, unsigned int* n_bricks, int* k_built)
{
    if (!wf || !wf->index_valid) return DF_E_NO_INDEX;
    const size_t nb = (size_t)wf->bx * wf->by * wf->bz;
    uint32_t total = 0;
    DF_HIP(hipMemcpy(&total, wf->brick_off + nb, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (total_entries) *total_entries = total;
    if (n_bricks) *n_bricks = (unsigned int)nb;
    if (k_built) *k_built = wf->k_built;
    return DF_OK;
}

// ====================================================================================== growth (dfusion_warp_extend)
// A table block is stale after growth when its brick's list changed (then a new node may be among its voxels' k nearest, and the lists
// are what the table build ranks), or when its build met an exact distance tie (the rebuilt tie tree may order the equidistant old nodes
// differently).  Otherwise its voxels rank the same candidates at the same distances without consulting the tree: the same tables,
// weights, blend model and codes.  Stale blocks go back to "not built", as after dfusion_warp_build_index with on-demand tables.
__global__ __launch_bounds__(256) void df_grow_dirty_kernel(const uint32_t* __restrict__ old_off, const uint16_t* __restrict__ old_list,
                                                            const uint32_t* __restrict__ off, const uint16_t* __restrict__ list,
                                                            int bx, int by, int bz, int nbx, int nby, int nbz, int bz0,
                                                            uint8_t* __restrict__ blk_state, float* __restrict__ blk_wmax, uint8_t* __restrict__ blk_tie)
{
    const size_t blk = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (blk >= (size_t)nbx * nby * nbz) return;
    const int x = (int)(blk % (size_t)nbx), y = (int)((blk / (size_t)nbx) % (size_t)nby), z = (int)(blk / ((size_t)nbx * nby));
    if (x >= bx || y >= by || z + bz0 >= bz) return;                       // (blocks of the table's padding hold no voxels)
    const size_t b = ((size_t)(z + bz0) * by + y) * bx + x;
    const uint32_t o0 = old_off[b], n0 = old_off[b + 1] - o0, o1 = off[b], n1 = off[b + 1] - o1;
    bool dirty = blk_tie[blk] != 0 || n0 != n1;
    for (uint32_t i = 0; !dirty && i < n1; ++i) dirty = old_list[o0 + i] != list[o1 + i];
    if (dirty) {
        blk_state[blk] = 0; blk_tie[blk] = 0;
        if (blk_wmax) blk_wmax[blk] = 0.f;
    }
}

int df_warp_grow(DfWarpField* wf, const float* pos, const float* dq, const float* sigma, int Mn, hipStream_t st)
{
    if (!wf || !pos || !dq || !sigma || Mn < wf->M || Mn > 65535) return DF_E_INVALID;
    df_side_drain(wf);                                         // (look-ahead builds read the node arrays and write the tables)
    wf->prep_valid = false;                                    // (a prepared plan was made for the old node set)
    if (Mn > wf->cap) {                                        // headroom: a run of small extends does not reallocate every time
        int cap = wf->cap + wf->cap / 2 + 256;
        cap = cap < Mn ? Mn : cap > 65535 ? 65535 : cap;
        int rc = df_warp_reserve(wf, cap);                     // (waits for every split sweep; the arrays are re-packed whole below)
        if (rc) return rc;
    }
    { int rc = df_wait_split_sweep(wf, st); if (rc) return rc; }
    const int M_old = wf->M;
    wf->M = Mn;
    if (Mn > M_old) wf->graph_kg = 0;                          // (the solver's node graph: rebuilt by the next regularised solve)
    { int rc = df_warp_pack_current(wf, pos, dq, sigma, st); if (rc) return rc; }   // (bounds, the sigma bound [4] included)
    { int rc = df_warp_build_tie_tree(wf, st); if (rc) return rc; }
    if (!wf->index_valid) return DF_OK;
    const size_t nb = (size_t)wf->bx * wf->by * wf->bz;
    const bool tabs = wf->tab_valid && wf->blk.state && wf->blk.tie;
    uint32_t* old_off = nullptr; uint16_t* old_list = nullptr;
    if (tabs) {                                                // the lists before the update, to find the bricks whose list changes
        const size_t off_bytes = ((nb + 1) * sizeof(uint32_t) + 255) & ~(size_t)255, need = off_bytes + wf->brick_list.cap * sizeof(uint16_t);
        { int rc = wf->grow_ws.reserve(need); if (rc) return rc; }
        old_off = (uint32_t*)wf->grow_ws.p; old_list = (uint16_t*)(wf->grow_ws + off_bytes);
        DF_HIP(hipMemcpyAsync(old_off, wf->brick_off, (nb + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        DF_HIP(hipMemcpyAsync(old_list, wf->brick_list, wf->brick_list.cap * sizeof(uint16_t), hipMemcpyDeviceToDevice, st));
    }
    wf->index_valid = false;                                   // (until the lists are re-made)
    DfVolume v; memset(&v, 0, sizeof(v));
    memcpy(v.dims, wf->geom_dims, sizeof(v.dims)); memcpy(v.voxel_size, wf->geom_vs, sizeof(v.voxel_size));
    float aff[12]; memcpy(aff, wf->geom_aff, sizeof(aff));
    { int rc = df_index_bricks(wf, v, aff, wf->k_built, st); if (rc) return rc; }
    wf->index_valid = true;
    if (!tabs) return DF_OK;
    const DfWarpedArgs a = df_table_args(wf);
    const int nbz = wf->tab_zn / 8;
    const size_t nblk = (size_t)a.bm_nbx * a.bm_nby * nbz;
    hipLaunchKernelGGL(df_grow_dirty_kernel, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, st, old_off, old_list, wf->brick_off, wf->brick_list,
                       wf->bx, wf->by, wf->bz, a.bm_nbx, a.bm_nby, nbz, wf->tab_z0 / DF_BRICK, wf->blk.state, a.blk_wmax, wf->blk.tie);
    DF_LAUNCH_CHECK();
    wf->alive_valid = false; wf->tab_complete = false;
    if (!((wf->index_flags & DF_INDEX_TABLES_ON_DEMAND) && wf->w_tab_valid)) {   // eager tables: the stale blocks are re-made here
        int rc = df_tables_complete(wf, st);
        if (rc) return rc;
    }
    DF_HIP(hipStreamSynchronize(st));
    return DF_OK;
}
