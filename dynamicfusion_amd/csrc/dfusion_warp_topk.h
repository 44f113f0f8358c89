// dfusion_warp_topk.h -- device code shared by the k-NN kernels (point queries, brick index, table build) and the sweeps: the sorted
// top-k insert in registers and the dual-quaternion blend out of LDS.
#pragma once
#include "dfusion_internal.h"

// ====================================================================================== top-k in registers
// What nanoflann returns (KNNResultSet::addPoint nanoflann.hpp:110-131 fed in searchLevel's order :1200-1254): the first k nodes by
// (distance, order in which THIS query's tree walk meets them).  Candidates arrive here in some other order (node index, brick
// list), so the sorted insert ranks by distance with strict '<' and, only when two distances are EQUAL, asks
// df_nf_visited_before (dfusion_nanoflann.h) which node the reference's walk meets first.  The common case costs K compares more
// than a plain insert; the equal-distance branch (nodes mirrored about a voxel / pixel plane, duplicated nodes) is a short
// stackless walk down the tree replica.  Without a tree (T.nodes == null) equal distances keep arrival order.
template <int K>
__device__ __forceinline__ void topk_insert(float (&bd)[K], int (&bi)[K], float d, int j, const DfNfView& T, f3 q)
{
    if (d <= bd[K - 1]) {
        bool eq = false;
#pragma unroll
        for (int i = 0; i < K; ++i) eq = eq || (bd[i] == d);
        if (!eq) {                                           // (then d < bd[K - 1])
            bd[K - 1] = d; bi[K - 1] = j;
#pragma unroll
            for (int i = K - 1; i > 0; --i) {
                if (bd[i] < bd[i - 1]) {
                    float td = bd[i]; bd[i] = bd[i - 1]; bd[i - 1] = td;
                    int ti = bi[i]; bi[i] = bi[i - 1]; bi[i - 1] = ti;
                }
            }
        } else {
            // position = entries strictly closer + equidistant entries the reference meets before j
            int pos = 0;
#pragma unroll 1
            for (int i = 0; i < K; ++i) {
                float di = bd[0]; int ji = bi[0];
#pragma unroll
                for (int t = 1; t < K; ++t) { di = (i == t) ? bd[t] : di; ji = (i == t) ? bi[t] : ji; }   // register select, no scratch
                if (di < d) ++pos;
                else if (di == d && (!T.nodes || df_nf_visited_before(T, q.x, q.y, q.z, ji, j))) ++pos;
            }
#pragma unroll
            for (int i = K - 1; i > 0; --i)
                if (i > pos) { bd[i] = bd[i - 1]; bi[i] = bi[i - 1]; }
#pragma unroll
            for (int i = 0; i < K; ++i)
                if (i == pos) { bd[i] = d; bi[i] = j; }
        }
    }
}
// distance-only variant (callers that need the k-th distance, not the list)
template <int K>
__device__ __forceinline__ void topk_insert(float (&bd)[K], int (&bi)[K], float d, int j)
{
    if (d < bd[K - 1]) {
        bd[K - 1] = d; bi[K - 1] = j;
#pragma unroll
        for (int i = K - 1; i > 0; --i) {
            if (bd[i] < bd[i - 1]) {
                float td = bd[i]; bd[i] = bd[i - 1]; bd[i - 1] = td;
                int ti = bi[i]; bi[i] = bi[i - 1]; bi[i - 1] = ti;
            }
        }
    }
}
// true when topk_insert(bd, .., d, ..) takes its equal-distance branch (the result then depends on the tie tree)
template <int K>
__device__ __forceinline__ bool df_topk_tie(const float (&bd)[K], float d)
{
    bool eq = false;
#pragma unroll
    for (int i = 0; i < K; ++i) eq = eq || (bd[i] == d);
    return eq && d <= bd[K - 1];
}
template <int K>
__device__ __forceinline__ void topk_init(float (&bd)[K], int (&bi)[K])
{
#pragma unroll
    for (int i = 0; i < K; ++i) { bd[i] = __uint_as_float(0x7f800000u); bi[i] = 0; }   // +inf
}

// dqb_blend_w (WarpField::DQB from the k weights + node indices): dfusion_internal.h
// Same blend with the node transforms staged in LDS: s_node[2j] = rot_j, s_node[2j+1] = node_t_j (GLOBAL node id j), so
// the two ds_read_b128 of a node share one address (the second uses the instruction's immediate offset).  The sums are
// kept as two float2 halves in MEMORY order ((w,x),(y,z)): the backend maps them 1:1 onto v_pk_mul_f32 / v_pk_add_f32
// without register shuffles (left to itself it paired (w,z),(x,y) and spent ~65 v_mov per voxel re-pairing the LDS
// words).  Element-wise IEEE mul then add, exactly the scalar sequence of :211-212.
struct DfBlendSums { df_v2f t01, t23, r01, r23; };      // sum w_i * node_t_i and sum w_i * rot_i as (w,x),(y,z) halves
template <int K>
__device__ __forceinline__ DfBlendSums dqb_sums_lds(const float4* s_node, const float (&wt)[K], const int (&bi)[K])
{
    DfBlendSums S;
    S.t01 = S.t23 = S.r01 = S.r23 = df_v2f{0.f, 0.f};
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const float4* nd = s_node + 2 * bi[i];
        const float4 r4 = nd[0], t4 = nd[1];
        const df_v2f ww = {wt[i], wt[i]};
        const df_v2f ta = {t4.x, t4.y}, tb = {t4.z, t4.w}, ra = {r4.x, r4.y}, rb = {r4.z, r4.w};
        S.t01 = S.t01 + ww * ta; S.t23 = S.t23 + ww * tb;     // :211
        S.r01 = S.r01 + ww * ra; S.r23 = S.r23 + ww * rb;     // :212
    }
    return S;
}
template <int K>
__device__ __forceinline__ void dqb_blend_lds(const float4* s_node, const float (&wt)[K], const int (&bi)[K], quat* rot_out,
                                              quat* dual_out)
{
    const DfBlendSums S = dqb_sums_lds<K>(s_node, wt, bi);
    quat tsum, rsum;
    tsum.w = S.t01.x; tsum.x = S.t01.y; tsum.y = S.t23.x; tsum.z = S.t23.y;
    rsum.w = S.r01.x; rsum.x = S.r01.y; rsum.y = S.r23.x; rsum.z = S.r23.y;
    rsum = q_normalize(rsum);                         // :214
    quat half;
    half.w = 0.5f * tsum.w; half.x = 0.5f * tsum.x; half.y = 0.5f * tsum.y; half.z = 0.5f * tsum.z;
    *rot_out = rsum;
    *dual_out = q_mul(half, rsum);                    // dual_quaternion.hpp:59-63
}

// weights from squared distances (WarpField::weighting per neighbour): dqb_weights, dfusion_internal.h
template <int K>
__device__ __forceinline__ void dqb_blend(const DfWarpView& W, const float (&bd)[K], const int (&bi)[K], quat* rot_out,
                                          quat* dual_out)
{
    float wt[K];
    dqb_weights<K>(W, bd, bi, wt);
    dqb_blend_w<K>(W, wt, bi, rot_out, dual_out);
}
