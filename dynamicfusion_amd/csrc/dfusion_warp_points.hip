// dfusion_warp_points.hip -- k-NN and warp of arbitrary points (dfusion_knn, dfusion_warp_points): a brute-force scan of the nodes, or,
// where the handle holds a brick index for >= k neighbours, its candidate lists (dfusion_warp_index.hip) with the scan as the fallback.
#include "dfusion_internal.h"
#include "dfusion_warp_topk.h"

// ====================================================================================== brute-force k-NN / warp of points
// One lane per query point; all M node positions stream through LDS in chunks (broadcast reads).
#define DF_PT_CHUNK 1024

// what a point kernel does with the k nearest nodes of point i: MODE 0 writes them out (WarpField::KNN), MODE 1 warps the point
// (and its normal) in place (WarpField::warp, warp_field.cpp:185-192; the index drift on NaN is fixed)
template <int K, int MODE>
__device__ __forceinline__ void df_point_finish(const DfWarpView& W, int i, f3 q, const float (&bd)[K], const int (&bi)[K],
                                                int* __restrict__ idx_out, float* __restrict__ d2_out, float* __restrict__ points,
                                                float* __restrict__ normals, const DfAff& to_live)
{
    if (MODE == 0) {
#pragma unroll
        for (int j = 0; j < K; ++j) { idx_out[(size_t)i * K + j] = bi[j]; d2_out[(size_t)i * K + j] = bd[j]; }
    } else {
        bool skip = q.x != q.x;
        f3 nq = mk3(0.f, 0.f, 0.f);
        if (normals) { nq = mk3(normals[3 * (size_t)i], normals[3 * (size_t)i + 1], normals[3 * (size_t)i + 2]); skip = skip || (nq.x != nq.x); }
        if (skip) return;
        quat rot, dual;
        dqb_blend<K>(W, bd, bi, &rot, &dual);
        f3 p = dq_transform(rot, dual, q);
        // cv::Affine3f * Vec3f : left-associated, no fma (opencv affine.hpp)
        const float* A = to_live.R; const float* T = to_live.t;
        points[3 * (size_t)i]     = A[0] * p.x + A[1] * p.y + A[2] * p.z + T[0];
        points[3 * (size_t)i + 1] = A[3] * p.x + A[4] * p.y + A[5] * p.z + T[1];
        points[3 * (size_t)i + 2] = A[6] * p.x + A[7] * p.y + A[8] * p.z + T[2];
        if (normals) {
            f3 nn = dq_transform(rot, dual, nq);      // reference translates normals too (warp_field.cpp:191)
            normals[3 * (size_t)i]     = A[0] * nn.x + A[1] * nn.y + A[2] * nn.z + T[0];
            normals[3 * (size_t)i + 1] = A[3] * nn.x + A[4] * nn.y + A[5] * nn.z + T[1];
            normals[3 * (size_t)i + 2] = A[6] * nn.x + A[7] * nn.y + A[8] * nn.z + T[2];
        }
    }
}

template <int K, int MODE /* 0 = knn out, 1 = warp points */>
__global__ __launch_bounds__(256) void df_points_kernel(DfWarpView W, const float* __restrict__ queries, int N,
                                                        int* __restrict__ idx_out, float* __restrict__ d2_out,
                                                        float* __restrict__ points, float* __restrict__ normals,
                                                        DfAff to_live)
{
    __shared__ float4 s_pos[DF_PT_CHUNK];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool active = i < N;
    f3 q = mk3(0.f, 0.f, 0.f);
    const float* src = MODE == 0 ? queries : points;
    if (active) q = mk3(src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2]);
    float bd[K]; int bi[K];
    topk_init<K>(bd, bi);
    for (int base = 0; base < W.M; base += DF_PT_CHUNK) {
        const int n = min(DF_PT_CHUNK, W.M - base);
        __syncthreads();
        for (int t = threadIdx.x; t < n; t += 256) s_pos[t] = W.pos_sigma[base + t];
        __syncthreads();
        for (int c = 0; c < n; ++c) {
            const float4 p = s_pos[c];
            topk_insert<K>(bd, bi, knn_dist2(q, p.x, p.y, p.z), base + c, W.nf, q);
        }
    }
    if (!active) return;
    df_point_finish<K, MODE>(W, i, q, bd, bi, idx_out, d2_out, points, normals, to_live);
}

// Exact k-NN of arbitrary points through the brick candidate lists: a point that rounds to a voxel of brick B lies inside B's
// cell, whose half-diagonal the lists were built for, so top-k over B's list (node-index order, like the brute-force scan) is the
// brute-force answer; points outside the grid search the nearest boundary brick.  Every result is verified by a distance bound
// (see the end of the kernel) and the rare points that fail it are handled by the scan kernel in a second launch; NaN points
// find nothing, as in the scan.
// ~50-150 candidates per point instead of all M.
struct DfPointIndex { DfAff world2vol, vol2world; int X, Y, Z; float ivx, ivy, ivz, vsx, vsy, vsz; };
template <int K, int MODE>
__global__ __launch_bounds__(64) void df_points_index_kernel(DfWarpView W, DfPointIndex G, const float* __restrict__ queries, int N,
                                                             int* __restrict__ idx_out, float* __restrict__ d2_out,
                                                             float* __restrict__ points, float* __restrict__ normals, DfAff to_live,
                                                             int* __restrict__ out_ids, int* __restrict__ out_count, int image_cols)
{
    // One wave64 per workgroup (so __syncthreads is a wave-level barrier and every loop below is wave-uniform).  Neighbouring
    // query points (pixels) mostly share a brick: the wave visits its DISTINCT bricks one after the other, stages each brick's
    // candidate positions through LDS with coalesced loads (a per-lane walk of the list is a chain of dependent global loads --
    // measured no faster than scanning all nodes), and the lanes of that brick rank them from LDS.
    constexpr int CAP = 384, NBMAX = 8;                    // LDS stage (7.5 KiB: 20 one-wave workgroups per CU), bricks per pass
    __shared__ float4 s_pos[CAP];
    __shared__ int s_id[CAP];
    const int lane = threadIdx.x;
    // image_cols > 0 (dfusion_warp_set_point_tiling): the points are the pixels of an image that wide and a wave takes an 8 x 8 pixel
    // tile instead of 64 consecutive pixels of a row -- 3 distinct bricks per wave instead of 8 on a 640 x 480 ray-cast cloud, and every
    // brick visit is a chain of dependent loads plus a ranking pass in which only that brick's lanes work.  Same results per point.
    int i = blockIdx.x * 64 + lane;
    if (image_cols > 0) {
        const int tiles = image_cols >> 3, ty = blockIdx.x / tiles, tx = blockIdx.x - ty * tiles;
        i = (ty * 8 + (lane >> 3)) * image_cols + tx * 8 + (lane & 7);
    }
    const bool active = i < N;
    f3 q = mk3(0.f, 0.f, 0.f);
    const float* src = MODE == 0 ? queries : points;
    if (active) q = mk3(src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2]);
    float bd[K]; int bi[K];
    topk_init<K>(bd, bi);
    const bool is_nan = (q.x != q.x) || (q.y != q.y) || (q.z != q.z);
    int brick = -1;                                        // -1: nothing to search (inactive / NaN)
    float dq = 0.f;                                        // distance to the centre of the brick that is searched
    if (active && !is_nan) {
        const f3 v = aff_mul(G.world2vol, q);
        // nearest brick (clamped to the grid: a point outside is tested against the closest boundary brick)
        const float fx = fminf(fmaxf(floorf(v.x * G.ivx + 0.5f), 0.f), (float)(G.X - 1));
        const float fy = fminf(fmaxf(floorf(v.y * G.ivy + 0.5f), 0.f), (float)(G.Y - 1));
        const float fz = fminf(fmaxf(floorf(v.z * G.ivz + 0.5f), 0.f), (float)(G.Z - 1));
        const int bxx = (int)fx / DF_BRICK, byy = (int)fy / DF_BRICK, bzz = (int)fz / DF_BRICK;
        if (fx == fx && fy == fy && fz == fz) {
            brick = (bzz * W.by + byy) * W.bx + bxx;
            const f3 c = aff_mul(G.vol2world, mk3(((float)(bxx * DF_BRICK) + 3.5f) * G.vsx, ((float)(byy * DF_BRICK) + 3.5f) * G.vsy,
                                                  ((float)(bzz * DF_BRICK) + 3.5f) * G.vsz));          // as df_brick_index_kernel
            const f3 dc = sub3(q, c);
            dq = sqrtf(dot3(dc, dc));
        }
    }
    // A pass stages the candidate lists of up to NBMAX of the wave's distinct bricks in LDS TOGETHER (their entries dealt out over the
    // lanes: two dependent load rounds -- ids, then positions -- for all of them, not two per brick and 64 candidates) and every lane
    // then ranks ITS brick's candidates from there, all bricks at once: the pass costs the longest list, not the sum of the lists.
    // Each lane still sees its brick's candidates in list order, so the results (ties included) are those of the one-brick-at-a-time walk.
    unsigned long long todo = __ballot(brick != -1);
    while (todo) {
        int nb = 0, myslot = -1, slot_brick = 0;
        for (unsigned long long rem = todo; rem && nb < NBMAX; ++nb) {
            const int leader = __ffsll((long long)rem) - 1;
            const int b = __shfl(brick, leader, 64);
            const bool mine = brick == b;
            if (mine) myslot = nb;
            if (lane == nb) slot_brick = b;
            rem &= ~__ballot(mine);
        }
        uint32_t lo = 0, len = 0;                          // lane s < nb: list range of brick s of this pass
        if (lane < nb) { lo = W.brick_off[slot_brick]; len = W.brick_off[slot_brick + 1] - lo; }
        uint32_t end = len;                                // running total over the slots
#pragma unroll
        for (int o = 1; o < NBMAX; o <<= 1) { const uint32_t t = __shfl_up(end, o, 64); if (lane >= o) end += t; }
        const uint32_t base = end - len;
        // the slots whose lists fit the stage together (a prefix of them); none = the first list alone is longer: walked in pieces
        const int nfit = __popcll(__ballot(lane < nb && end <= (uint32_t)CAP));
        const int ntake = max(nfit, 1);
        const int ms = min(max(myslot, 0), ntake - 1);
        const bool mine = myslot >= 0 && myslot < ntake;
        const uint32_t my_base = __shfl(base, ms, 64), my_len = __shfl(len, ms, 64);
        const uint32_t total = nfit ? (uint32_t)__shfl(end, nfit - 1, 64) : (uint32_t)__shfl(len, 0, 64);
        for (uint32_t c0 = 0; c0 < total; c0 += CAP) {     // (one round unless a single list exceeds the stage)
            const uint32_t n = min((uint32_t)CAP, total - c0);
            __syncthreads();
            for (uint32_t e = lane; e < n; e += 64) {
                // list position of staged entry c0 + e: it belongs to the last slot that starts at or before it (the per-slot values
                // are read with readlane -- scalar, whatever lanes this loop has left active)
                uint32_t adj = (uint32_t)__builtin_amdgcn_readlane((int)lo, 0) - (uint32_t)__builtin_amdgcn_readlane((int)base, 0);
#pragma unroll
                for (int i = 1; i < NBMAX; ++i)
                    if (i < ntake && c0 + e >= (uint32_t)__builtin_amdgcn_readlane((int)base, i))
                        adj = (uint32_t)__builtin_amdgcn_readlane((int)lo, i) - (uint32_t)__builtin_amdgcn_readlane((int)base, i);
                const uint32_t src = c0 + e + adj;
                const int j = (int)W.brick_list[src];
                s_id[e] = j;
                s_pos[e] = W.pos_sigma[j];
            }
            __syncthreads();
            if (mine) {
                const uint32_t b0 = max(my_base, c0), b1 = min(my_base + my_len, c0 + n);
                for (uint32_t c = b0; c < b1; ++c) {
                    const float4 p = s_pos[c - c0];
                    topk_insert<K>(bd, bi, knn_dist2(q, p.x, p.y, p.z), s_id[c - c0], W.nf, q);
                }
            }
        }
        todo &= ~__ballot(mine);
    }
    // Exactness check: a node outside the brick's list is farther than thr from the brick centre, hence farther than thr - dq from
    // the query; if the k-th distance found is within that, nothing outside the list can belong to the k nearest.  (Always true for
    // a point inside the brick's cell; for a point outside the grid it decides whether the boundary brick's list suffices.)  The rare
    // failures -- and inf coordinates -- are listed for the scan kernel (second launch).
    bool outside = false;
    if (active && !is_nan) {
        const float slack = brick >= 0 ? (W.brick_thr[brick] - dq) * 0.9999f - 1e-6f : -1.f;
        outside = !(slack > 0.f && bd[K - 1] <= slack * slack);
        if (outside) out_ids[atomicAdd(out_count, 1)] = i;
    }
    if (!active || outside) return;
    df_point_finish<K, MODE>(W, i, q, bd, bi, idx_out, d2_out, points, normals, to_live);
}

// Second pass of the indexed query: ONE WAVE per listed point.  The lanes split the nodes (lane, lane + 64, ...), each keeps its own
// top-K, and the wave merges them with K pops of the lexicographic minimum (distance, node index) -- the order of a serial scan in
// node-index order with strict '<' insertion, equal distances in the reference's tree order.  A serial scan by one lane takes ~0.5 ms whatever the number
// of points (it is the depth of df_points_kernel); this takes M / 64 steps.
template <int K, int MODE>
__global__ __launch_bounds__(256) void df_points_wave_kernel(DfWarpView W, const float* __restrict__ queries, int* __restrict__ idx_out,
                                                             float* __restrict__ d2_out, float* __restrict__ points,
                                                             float* __restrict__ normals, DfAff to_live, const int* __restrict__ ids,
                                                             const int* __restrict__ id_count)
{
    const int lane = threadIdx.x & 63;
    const int n_ids = *id_count;
    for (int slot = blockIdx.x * 4 + (threadIdx.x >> 6); slot < n_ids; slot += gridDim.x * 4) {      // wave-uniform
        const int i = ids[slot];
        const float* src = MODE == 0 ? queries : points;
        const f3 q = mk3(src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2]);
        float bd[K]; int bi[K];
        topk_init<K>(bd, bi);
        for (int j = lane; j < W.M; j += 64) {
            const float4 p = W.pos_sigma[j];
            topk_insert<K>(bd, bi, knn_dist2(q, p.x, p.y, p.z), j, W.nf, q);
        }
        float rd[K]; int ri[K];
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const float m = wave_min_f32(bd[0]);
            // the lanes whose head is at the minimum distance: the one whose node the reference's walk meets first wins
            // (wave-uniform loop over the set bits; one bit unless distances tie)
            unsigned long long who = __ballot(bd[0] == m);
            int cand = __shfl(bi[0], __ffsll((long long)who) - 1, 64);
            who &= who - 1;
            while (who) {
                const int other = __shfl(bi[0], __ffsll((long long)who) - 1, 64);
                who &= who - 1;
                if (W.nf.nodes ? df_nf_visited_before(W.nf, q.x, q.y, q.z, other, cand) : other < cand) cand = other;
            }
            rd[r] = m; ri[r] = cand;
            if (bd[0] == m && bi[0] == cand) {              // the owner pops its head
#pragma unroll
                for (int t = 0; t < K - 1; ++t) { bd[t] = bd[t + 1]; bi[t] = bi[t + 1]; }
                bd[K - 1] = __uint_as_float(0x7f800000u); bi[K - 1] = -1;
            }
        }
        if (lane == 0) df_point_finish<K, MODE>(W, i, q, rd, ri, idx_out, d2_out, points, normals, to_live);
    }
}

// the brick lists serve point queries when an index for >= k neighbours exists (a list built for k_built >= k contains the k nearest)
// [0] = count, [1..] = ids of the points the indexed pass left to the scan; zeroed per call
static int df_point_fallback_reserve(DfWarpField* wf, int N, hipStream_t st)
{
    { int rc = wf->pt_ids.reserve((size_t)N + 1); if (rc) return rc; }
    DF_HIP(hipMemsetAsync(wf->pt_ids, 0, sizeof(int), st));
    return DF_OK;
}

static bool df_point_index(const DfWarpField* wf, int k, DfPointIndex* G)
{
    if (!wf->index_valid || wf->k_built < k || !wf->geom_inv_ok) return false;
    G->world2vol = df_aff(wf->geom_inv);
    G->X = wf->geom_dims[0]; G->Y = wf->geom_dims[1]; G->Z = wf->geom_dims[2];
    G->ivx = 1.f / wf->geom_vs[0]; G->ivy = 1.f / wf->geom_vs[1]; G->ivz = 1.f / wf->geom_vs[2];
    G->vol2world = df_aff(wf->geom_aff); G->vsx = wf->geom_vs[0]; G->vsy = wf->geom_vs[1]; G->vsz = wf->geom_vs[2];
    return wf->brick_thr != nullptr;
}

// the image width to tile point queries by, if the hint applies to this query (whole 8 x 8 tiles), else 0 = linear order
static int df_point_tiling(const DfWarpField* wf, int N)
{
    const int c = wf->pt_image_cols;
    return (c >= 8 && (c & 7) == 0 && N % (8 * c) == 0) ? c : 0;
}

extern "C" int dfusion_warp_set_point_tiling(DfWarpField* wf, int image_cols)
{
    if (!wf || image_cols < 0) return DF_E_INVALID;
    wf->pt_image_cols = image_cols;
    return DF_OK;
}

extern "C" int dfusion_knn(DfWarpField* wf, int k, const float* queries, int N, int* idx, float* d2, dfStream stream)
{
    if (!wf || !queries || !idx || !d2 || N < 0 || wf->M < k || k < 1) return DF_E_INVALID;
    if (N == 0) return DF_OK;
    DfWarpView W = df_view(wf);
    DfAff ident; memset(&ident, 0, sizeof(ident));
    DfPointIndex G;
    if (df_point_index(wf, k, &G)) {
        int rc = df_point_fallback_reserve(wf, N, (hipStream_t)stream);
        if (rc) return rc;
        DF_DISPATCH_K(k, df_points_index_kernel<K, 0><<<dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream>>>(
                             W, G, queries, N, idx, d2, (float*)nullptr, (float*)nullptr, ident, wf->pt_ids + 1, wf->pt_ids, df_point_tiling(wf, N)));
        DF_DISPATCH_K(k, df_points_wave_kernel<K, 0><<<dim3(2048), dim3(256), 0, (hipStream_t)stream>>>(
                             W, queries, idx, d2, (float*)nullptr, (float*)nullptr, ident, wf->pt_ids + 1, wf->pt_ids));
    } else
    DF_DISPATCH_K(k, df_points_kernel<K, 0><<<dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream>>>(
                         W, queries, N, idx, d2, (float*)nullptr, (float*)nullptr, ident));
    DF_LAUNCH_CHECK();
    return DF_OK;
}

extern "C" int dfusion_warp_points(DfWarpField* wf, int k, float* points, float* normals, int N, const float warp_to_live[12],
                                   dfStream stream)
{
    if (!wf || !points || !warp_to_live || N < 0 || wf->M < k || k < 1) return DF_E_INVALID;
    if (N == 0) return DF_OK;
    DfWarpView W = df_view(wf);
    DfAff live = df_aff(warp_to_live);
    DfPointIndex G;
    if (df_point_index(wf, k, &G)) {
        int rc = df_point_fallback_reserve(wf, N, (hipStream_t)stream);
        if (rc) return rc;
        DF_DISPATCH_K(k, df_points_index_kernel<K, 1><<<dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream>>>(
                             W, G, (const float*)nullptr, N, (int*)nullptr, (float*)nullptr, points, normals, live, wf->pt_ids + 1, wf->pt_ids, df_point_tiling(wf, N)));
        DF_DISPATCH_K(k, df_points_wave_kernel<K, 1><<<dim3(2048), dim3(256), 0, (hipStream_t)stream>>>(
                             W, (const float*)nullptr, (int*)nullptr, (float*)nullptr, points, normals, live, wf->pt_ids + 1, wf->pt_ids));
    } else
    DF_DISPATCH_K(k, df_points_kernel<K, 1><<<dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream>>>(
                         W, (const float*)nullptr, N, (int*)nullptr, (float*)nullptr, points, normals, live));
    DF_LAUNCH_CHECK();
    return DF_OK;
}
