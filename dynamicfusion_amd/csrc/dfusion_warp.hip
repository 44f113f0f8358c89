// dfusion_warp.hip -- warp-field nodes on device, exact k-NN brick index, per-point warp, and the
// north-star kernel: per-voxel dual-quaternion blend fused into the projective TSDF update.
//
// Replaces (on device) /root/reference/kfusion/src/warp_field.cpp:180-251 (KNN / weighting / DQB /
// warp), the nanoflann kd-tree it queries (warp_field.cpp:275-282), and composes them with
// kfusion/src/cuda/tsdf_volume.cu:77-104.
//
// MI355X design notes
//   * k-NN: a kd-tree walk is pointer-chasing and divergent.  Instead, for every 8^3 voxel brick
//     the index stores the EXACT candidate set {n : |n - c_B| <= D_k(c_B) + 2 r_B} (c_B brick
//     centre, r_B half diagonal, D_k distance to the k-th nearest node).  Any node among the k
//     nearest of any voxel of the brick is in that set, so a brute-force top-k over the list is
//     the exact nanoflann answer.  Lists depend only on canonical node positions: they are
//     rebuilt when nodes are inserted, not per frame.  Built on the GPU, one wave per brick,
//     with wave-level k-th-smallest selection and ballot/popcount-prefix compaction.
//   * integrate_warped: one 256-thread workgroup per brick; candidate positions (+sigma) are
//     staged in LDS once per brick and read back with broadcast ds_read_b128; each lane keeps the
//     running top-k of its voxel in registers.
#include "dfusion_internal.h"
#include "dfusion_pyramid.h"
#include <atomic>
#include <mutex>
#include <utility>
#include <vector>
#include <stdlib.h>
#include <stdio.h>
#include <math.h>

// ====================================================================================== nodes
__global__ __launch_bounds__(256) void df_pack_nodes_kernel(const float* __restrict__ pos, const float* __restrict__ dq,
                                                            const float* __restrict__ sigma, int M,
                                                            float4* __restrict__ pos_sigma, float4* __restrict__ rot,
                                                            float4* __restrict__ dual, float4* __restrict__ node_t, float4* __restrict__ rt)
{
    int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    if (pos) pos_sigma[j] = make_float4(pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], sigma[j]);
    quat r, d;
    r.w = dq[8 * j]; r.x = dq[8 * j + 1]; r.y = dq[8 * j + 2]; r.z = dq[8 * j + 3];
    d.w = dq[8 * j + 4]; d.x = dq[8 * j + 5]; d.y = dq[8 * j + 6]; d.z = dq[8 * j + 7];
    quat t = dq_get_translation(r, d);                 // DualQuaternion::getTranslation, dual_quaternion.hpp:120-125
    rot[j] = make_float4(r.w, r.x, r.y, r.z);
    dual[j] = make_float4(d.w, d.x, d.y, d.z);
    node_t[j] = make_float4(t.w, t.x, t.y, t.z);
    rt[2 * j] = rot[j]; rt[2 * j + 1] = node_t[j];
}

// Conservative per-node displacement ingredients for brick culling: max |t_i| and max sin(theta_i/2)
// over nodes.  bounds[0] = max |t|, bounds[3] = max |rotation quaternion| (for the zero-weight tile test), bounds[1] = max
// sin(half angle), bounds[1] = 2 (=> no culling) if
// any rotation has w < 0 or is not finite (the hemisphere argument of the bound needs w >= 0).
__global__ __launch_bounds__(256) void df_node_bounds_kernel(const float4* __restrict__ rot, const float4* __restrict__ node_t,
                                                             int M, float* __restrict__ bounds)
{
    int j = blockIdx.x * 256 + threadIdx.x;
    float tn = 0.f, sh = 0.f, rn = 0.f;
    if (j < M) {
        float4 t = node_t[j], r = rot[j];
        tn = sqrtf(t.y * t.y + t.z * t.z + t.w * t.w);          // (x,y,z) of the quaternion are .y .z .w of the float4
        float n = sqrtf(r.x * r.x + r.y * r.y + r.z * r.z + r.w * r.w);
        rn = (n == n) ? n : 3.0e38f;                            // >= every |component| of the rotation quaternion
        float vn = sqrtf(r.y * r.y + r.z * r.z + r.w * r.w);
        sh = vn / n;
        if (!(r.x >= 0.f) || !(n > 0.f) || !(sh == sh) || !(tn == tn)) { sh = 2.f; }
        if (!(tn == tn)) tn = 3.0e38f;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        tn = fmaxf(tn, __shfl_xor(tn, o, 64)); sh = fmaxf(sh, __shfl_xor(sh, o, 64)); rn = fmaxf(rn, __shfl_xor(rn, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMax((unsigned int*)&bounds[0], __float_as_uint(tn));   // non-negative floats order as uints
        atomicMax((unsigned int*)&bounds[1], __float_as_uint(sh));
        atomicMax((unsigned int*)&bounds[3], __float_as_uint(rn));
    }
}

extern "C" int dfusion_warp_create(DfWarpField** out)
{
    if (!out) return DF_E_INVALID;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return DF_E_NO_DEVICE;
    DfWarpField* wf = new (std::nothrow) DfWarpField();
    if (!wf) return DF_E_INVALID;
    wf->device = dev;
    *out = wf;
    return DF_OK;
}

// The handle's side stream (look-ahead table / model builds): made on first use; df_side_join makes `st` wait for whatever is still
// running there (a device-side wait, nothing blocks the host), df_side_drain blocks until it is idle (before tables are re-made).
static int df_side_init(DfWarpField* wf)
{
    if (wf->side) return DF_OK;
    // every resource first, the handle last: a failure part-way leaves nothing behind that passes the test above
    hipStream_t side = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr; void* h = wf->host_report ? (void*)wf->host_report : nullptr;
    hipError_t e = hipStreamCreateWithFlags(&side, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ev_join, hipEventDisableTiming);
    if (e == hipSuccess && !h) e = hipHostMalloc(&h, 4 * sizeof(uint32_t), hipHostMallocDefault);
    if (e != hipSuccess) {
        if (ev_join) (void)hipEventDestroy(ev_join);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (side) (void)hipStreamDestroy(side);
        if (h && !wf->host_report) (void)hipHostFree(h);
        (void)hipGetLastError();
        return (int)e;
    }
    if (!wf->host_report) {
        wf->host_report = (volatile uint32_t*)h;
        wf->host_report[0] = wf->host_report[1] = wf->host_report[2] = 1u;       // nothing reported yet: assume work
        wf->host_report[3] = 0u;
    }
    wf->ev_fork = ev_fork; wf->ev_join = ev_join; wf->side = side;
    return DF_OK;
}
static int df_side_join(DfWarpField* wf, hipStream_t st)
{
    if (!wf->side_pending) return DF_OK;
    DF_HIP(hipStreamWaitEvent(st, wf->ev_join, 0));
    wf->side_pending = false;
    return DF_OK;
}
static void df_side_drain(DfWarpField* wf)
{
    if (wf->side) (void)hipStreamSynchronize(wf->side);
    wf->side_pending = false;
}

// A sweep issued through dfusion_integrate_warped_sweep may still be reading the node arrays, the launch plan and the verdict bytes on ITS
// stream when the next frame's set_transforms / prepare arrive on another one: they wait for it on the device.
static int df_wait_split_sweep(DfWarpField* wf, hipStream_t st)            // every sweep recorded so far
{
    if (wf->recorded_seq) DF_HIP(hipStreamWaitEvent(st, wf->ev_sweep_done[wf->recorded_seq & 1], 0));
    return DF_OK;
}
// ... or only the sweep (number `reader`) that last read a buffer about to be rewritten.  The ring holds the last two sweeps' events; all
// sweeps are on one stream, so an older one is done when the second-to-last is.  A reader that was never recorded (a prepared plan that was
// dropped) holds nothing.
static int df_wait_reader(DfWarpField* wf, unsigned long long reader, hipStream_t st)
{
    if (reader == 0 || wf->recorded_seq == 0 || reader > wf->recorded_seq) return DF_OK;
    // the earliest recorded sweep that is not older than `reader` (sweeps complete in order: its completion implies the reader's)
    int pick = -1;
    for (int i = 0; i < 2; ++i)
        if (wf->ring_seq[i] >= reader && (pick < 0 || wf->ring_seq[i] < wf->ring_seq[pick])) pick = i;
    if (pick < 0) return DF_OK;
    DF_HIP(hipStreamWaitEvent(st, wf->ev_sweep_done[pick], 0));
    return DF_OK;
}
extern "C" int dfusion_warp_destroy(DfWarpField* wf)
{
    if (!wf) return DF_OK;
    df_side_drain(wf);
    if (wf->side) { (void)hipEventDestroy(wf->ev_fork); (void)hipEventDestroy(wf->ev_join); (void)hipStreamDestroy(wf->side); }
    if (wf->split_events) { (void)hipEventDestroy(wf->ev_prep_done); (void)hipEventDestroy(wf->ev_sweep_done[0]); (void)hipEventDestroy(wf->ev_sweep_done[1]); }
    if (wf->host_report) (void)hipHostFree((void*)wf->host_report);
    delete wf;
    return DF_OK;
}

static int df_wait_all_sweeps_host(DfWarpField* wf)
{
    if (wf->recorded_seq) DF_HIP(hipEventSynchronize(wf->ev_sweep_done[wf->recorded_seq & 1]));
    return DF_OK;
}
static int df_warp_reserve(DfWarpField* wf, int M)
{
    if (M <= wf->cap) return DF_OK;
    { int rc = df_wait_all_sweeps_host(wf); if (rc) return rc; }        // (a split sweep may still read what is freed here)
    wf->cap = 0;
    wf->prep_valid = false;                                               // (a prepared plan points into the arrays freed here)
    { int rc = wf->pos_sigma.reserve((size_t)M); if (rc) return rc; }
    { int rc = wf->rot.reserve((size_t)M); if (rc) return rc; }
    { int rc = wf->dual.reserve((size_t)M); if (rc) return rc; }
    { int rc = wf->node_t.reserve((size_t)M); if (rc) return rc; }
    { int rc = wf->rot_alt.reserve((size_t)M); if (rc) return rc; }       // (the alternate set the next set_transforms writes)
    { int rc = wf->dual_alt.reserve((size_t)M); if (rc) return rc; }
    { int rc = wf->node_t_alt.reserve((size_t)M); if (rc) return rc; }
    { int rc = wf->rt.reserve(2 * (size_t)M); if (rc) return rc; }
    { int rc = wf->rt_alt.reserve(2 * (size_t)M); if (rc) return rc; }
    wf->node_reader[0] = wf->node_reader[1] = 0;
    if (!wf->bounds_dev) { int rc = wf->bounds_dev.reserve(8); if (rc) return rc; DF_HIP(hipMemset(wf->bounds_dev, 0, 8 * sizeof(float))); }   // ([6]: the capped pyramid's image-wide maximum, 0 between frames)
    wf->cap = M;
    return DF_OK;
}

// Pack + bounds in ONE launch for node sets of ordinary size (one workgroup: no atomics, no memset of the bounds; the per-frame
// set_transforms was three launches of ~4.5 us each).
__global__ __launch_bounds__(1024) void df_pack_bounds_kernel(const float* __restrict__ pos, const float* __restrict__ dq, const float* __restrict__ sigma,
                                                              int M, float4* __restrict__ pos_sigma, float4* __restrict__ rot,
                                                              float4* __restrict__ dual, float4* __restrict__ node_t, float4* __restrict__ rt,
                                                              float* __restrict__ bounds)
{
    __shared__ float s_red[4][16];
    float tn = 0.f, sh = 0.f, rn = 0.f, sg = 0.f;
    for (int j = threadIdx.x; j < M; j += 1024) {
        if (pos) {
            pos_sigma[j] = make_float4(pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], sigma[j]);
            const float a = fabsf(sigma[j]); sg = fmaxf(sg, a == a ? a : 3.0e38f);
        }
        quat r, d;
        r.w = dq[8 * j]; r.x = dq[8 * j + 1]; r.y = dq[8 * j + 2]; r.z = dq[8 * j + 3];
        d.w = dq[8 * j + 4]; d.x = dq[8 * j + 5]; d.y = dq[8 * j + 6]; d.z = dq[8 * j + 7];
        const quat t = dq_get_translation(r, d);              // DualQuaternion::getTranslation, dual_quaternion.hpp:120-125
        rot[j] = make_float4(r.w, r.x, r.y, r.z);
        dual[j] = make_float4(d.w, d.x, d.y, d.z);
        node_t[j] = make_float4(t.w, t.x, t.y, t.z);
        rt[2 * j] = make_float4(r.w, r.x, r.y, r.z); rt[2 * j + 1] = make_float4(t.w, t.x, t.y, t.z);
        // (the bounds exactly as df_node_bounds_kernel takes them from the packed arrays)
        float tj = sqrtf(t.x * t.x + t.y * t.y + t.z * t.z);
        const float n = sqrtf(r.w * r.w + r.x * r.x + r.y * r.y + r.z * r.z);
        const float rj = (n == n) ? n : 3.0e38f;
        const float vn = sqrtf(r.x * r.x + r.y * r.y + r.z * r.z);
        float sj = vn / n;
        if (!(r.w >= 0.f) || !(n > 0.f) || !(sj == sj) || !(tj == tj)) sj = 2.f;
        if (!(tj == tj)) tj = 3.0e38f;
        tn = fmaxf(tn, tj); sh = fmaxf(sh, sj); rn = fmaxf(rn, rj);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        tn = fmaxf(tn, __shfl_xor(tn, o, 64)); sh = fmaxf(sh, __shfl_xor(sh, o, 64)); rn = fmaxf(rn, __shfl_xor(rn, o, 64));
        sg = fmaxf(sg, __shfl_xor(sg, o, 64));
    }
    if ((threadIdx.x & 63) == 0) { s_red[0][threadIdx.x >> 6] = tn; s_red[1][threadIdx.x >> 6] = sh; s_red[2][threadIdx.x >> 6] = rn; s_red[3][threadIdx.x >> 6] = sg; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) { tn = fmaxf(tn, s_red[0][w]); sh = fmaxf(sh, s_red[1][w]); rn = fmaxf(rn, s_red[2][w]); sg = fmaxf(sg, s_red[3][w]); }
        bounds[0] = tn; bounds[1] = sh; bounds[2] = 0.f; bounds[3] = rn;
        if (pos) bounds[4] = sg;                              // max |dg_w| of the node set (the verdict pass's bound on unbuilt blocks' weights)
    }
}

static int df_warp_pack_current(DfWarpField* wf, const float* pos, const float* dq, const float* sigma, hipStream_t st);
// The transforms go into the ALTERNATE node arrays, which then become the current ones: a sweep issued through the split API on another
// stream may still be reading the set that was current when its plan was made.  What is waited for is the last sweep that read the
// alternate set -- two set_transforms ago -- not the one running now.  (Positions -- set_nodes -- are not double-buffered: every
// recorded sweep is waited for.)
static int df_warp_pack(DfWarpField* wf, const float* pos, const float* dq, const float* sigma, hipStream_t st)
{
    if (pos) { int rc = df_wait_split_sweep(wf, st); if (rc) return rc; }
    else {
        // The alternate set is about to be rewritten.  Its last reader may be a plan that was PREPARED and not yet swept (host order
        // prepare(t), set_transforms, set_transforms, sweep(t)): nothing on the device orders this write after a sweep that has not been
        // issued, and the sweep would blend with the wrong transforms without an error.  Such a plan is void from here on -- its sweep
        // call returns DF_E_INVALID.
        if (wf->prep_valid && wf->node_reader[wf->nphase ^ 1] == wf->seq && wf->seq > wf->recorded_seq) wf->prep_valid = false;
        int rc = df_wait_reader(wf, wf->node_reader[wf->nphase ^ 1], st); if (rc) return rc;
    }
    std::swap(wf->rot, wf->rot_alt); std::swap(wf->dual, wf->dual_alt); std::swap(wf->node_t, wf->node_t_alt); std::swap(wf->rt, wf->rt_alt);
    wf->nphase ^= 1;
    wf->node_reader[wf->nphase] = 0;                                       // (rewritten: nobody reads the old contents any more)
    return df_warp_pack_current(wf, pos, dq, sigma, st);
}
static int df_warp_pack_current(DfWarpField* wf, const float* pos, const float* dq, const float* sigma, hipStream_t st)
{
    if (wf->M <= 8192) {
        hipLaunchKernelGGL(df_pack_bounds_kernel, dim3(1), dim3(1024), 0, st, pos, dq, sigma, wf->M, wf->pos_sigma, wf->rot, wf->dual, wf->node_t,
                           wf->rt, wf->bounds_dev);
        DF_LAUNCH_CHECK();
        return DF_OK;
    }
    hipLaunchKernelGGL(df_pack_nodes_kernel, dim3((wf->M + 255) / 256), dim3(256), 0, st, pos, dq, sigma, wf->M,
                       wf->pos_sigma, wf->rot, wf->dual, wf->node_t, wf->rt);
    DF_LAUNCH_CHECK();
    DF_HIP(hipMemsetAsync(wf->bounds_dev, 0, 4 * sizeof(float), st));     // [2] (max dists) is rewritten by every integrate
    if (pos) { const float unknown = 3.0e38f; DF_HIP(hipMemcpyAsync(wf->bounds_dev + 4, &unknown, sizeof(float), hipMemcpyHostToDevice, st)); }   // (no sigma bound on this path)
    hipLaunchKernelGGL(df_node_bounds_kernel, dim3((wf->M + 255) / 256), dim3(256), 0, st, wf->rot, wf->node_t, wf->M,
                       wf->bounds_dev);
    DF_LAUNCH_CHECK();
    return DF_OK;
}

// buildKDTree (warp_field.cpp:275-282): nanoflann's tree over the node positions, replayed on the host (the build is sequential in
// nanoflann too -- the partition order depends on every swap) from the positions just packed on the device; M <= 65535 nodes, a
// few hundred microseconds.  The tree only orders exactly equidistant nodes (dfusion_nanoflann.h).
static int df_warp_build_tie_tree(DfWarpField* wf, hipStream_t st)
{
    const int M = wf->M;
    wf->nf_ok = false;
    std::vector<float> host((size_t)M * 4);
    DF_HIP(hipMemcpyAsync(host.data(), wf->pos_sigma, (size_t)M * sizeof(float4), hipMemcpyDeviceToHost, st));
    DF_HIP(hipStreamSynchronize(st));
    for (size_t i = 0; i < (size_t)M * 4; ++i) if ((i & 3) != 3 && !(host[i] == host[i])) return DF_OK;     // NaN position: no tree
    DfNfBuild B;
    B.build(host.data(), M);
    { int rc = wf->nf_nodes.reserve(B.nodes.size()); if (rc) return rc; }
    { int rc = wf->nf_vpos.reserve((size_t)M); if (rc) return rc; }
    std::vector<uint16_t> vpos((size_t)M);
    for (int i = 0; i < M; ++i) vpos[B.vind[i]] = (uint16_t)i;
    DF_HIP(hipMemcpyAsync(wf->nf_nodes, B.nodes.data(), B.nodes.size() * sizeof(DfNfNode), hipMemcpyHostToDevice, st));
    DF_HIP(hipMemcpyAsync(wf->nf_vpos, vpos.data(), (size_t)M * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    DF_HIP(hipStreamSynchronize(st));                        // the host vectors go out of scope
    wf->nf_depth = B.depth;
    wf->nf_ok = true;
    return DF_OK;
}

extern "C" int dfusion_warp_set_nodes(DfWarpField* wf, const float* pos, const float* dq, const float* sigma, int M,
                                      dfStream stream)
{
    if (!wf || !pos || !dq || !sigma || M <= 0 || M > 65535) return DF_E_INVALID;
    df_side_drain(wf);                                         // (look-ahead builds read the node arrays)
    wf->prep_valid = false;                                    // (a prepared plan was made for the old node set: ADVICE r5)
    int rc = df_warp_reserve(wf, M);
    if (rc) return rc;
    wf->M = M;
    wf->index_valid = false;
    wf->tab_valid = false; wf->w_tab_valid = false;
    rc = df_warp_pack(wf, pos, dq, sigma, (hipStream_t)stream);
    if (rc) return rc;
    return df_warp_build_tie_tree(wf, (hipStream_t)stream);
}

extern "C" int dfusion_warp_set_transforms(DfWarpField* wf, const float* dq, dfStream stream)
{
    if (!wf || !dq || wf->M <= 0) return DF_E_INVALID;
    return df_warp_pack(wf, nullptr, dq, nullptr, (hipStream_t)stream);
}

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

static DfWarpView df_view(const DfWarpField* wf)
{
    DfWarpView W;
    W.pos_sigma = wf->pos_sigma; W.rot = wf->rot; W.dual = wf->dual; W.node_t = wf->node_t; W.rt = wf->rt; W.M = wf->M;
    W.brick_off = wf->brick_off; W.brick_list = wf->brick_list; W.brick_thr = wf->brick_thr; W.bx = wf->bx; W.by = wf->by; W.bz = wf->bz;
    W.nf.nodes = wf->nf_ok ? wf->nf_nodes : nullptr; W.nf.vpos = wf->nf_vpos;
    return W;
}

#define DF_DISPATCH_K(k, ...)                             \
    switch (k) {                                          \
        case 1: { constexpr int K = 1; __VA_ARGS__; } break; \
        case 2: { constexpr int K = 2; __VA_ARGS__; } break; \
        case 3: { constexpr int K = 3; __VA_ARGS__; } break; \
        case 4: { constexpr int K = 4; __VA_ARGS__; } break; \
        case 5: { constexpr int K = 5; __VA_ARGS__; } break; \
        case 6: { constexpr int K = 6; __VA_ARGS__; } break; \
        case 7: { constexpr int K = 7; __VA_ARGS__; } break; \
        case 8: { constexpr int K = 8; __VA_ARGS__; } break; \
        default: return DF_E_INVALID;                     \
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

static int df_build_voxel_table(DfWarpField* wf, const DfVolume& v, const DfSlab& s, const float vol2world[12], int k, bool weights,
                                bool on_demand, hipStream_t st);

// The brick lists (and the geometry they were made for) of dfusion_warp_build_index, for the node set the handle holds; blocks until built.
static int df_index_bricks(DfWarpField* wf, const DfVolume& v, const float vol2world[12], int k, hipStream_t st)
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

// ====================================================================================== integrate (warped)
struct DfWarpedArgs {
    uint32_t* vol; int X, Y, Z;
    int z_store0, z_own0, z_own_n;
    int bz0;                       // first brick / tile layer of this launch
    float vsx, vsy, vsz;
    DfAff vol2world, world2cam;
    DfIntegrateParams P;
    unsigned long long* n_upd;
    unsigned long long* n_swept;   // nullable (dfusion_warp_debug_counters): += voxels of the plan's alive (patch, layer) cells
    // conservative cull (disabled when cull == null).  cull[0] = max |t_i|, cull[1] = max sin(theta_i/2)
    // (> 1 => bound unavailable), cull[2] = max dists value of this frame; all produced on the stream, so the
    // frame needs no host round trip.
    const float* cull;
    float kf;                      // (float)k
    float tile_r;                  // half diagonal of a work tile's voxel-centre lattice (world metres), inflated
    float cam_scale;               // >= operator norm of world2cam.R (1 for a rigid pose), inflated
    float origin_cam;              // |world2cam.t| = distance of the WORLD ORIGIN from the camera centre when world2cam is rigid, else < 0
    DfDistsPyramid py;             // max-pyramid of this frame's dists (py.top == 0: only the image-wide maximum cull[2] is available)
    // per-voxel tables over planes [tab_z0, tab_z0 + tab_zn), TILE-MAJOR (private layout, see df_tab_index): the
    // 32x16x8 voxels a sweep workgroup owns are contiguous, so it streams 8 KiB (k-NN) + 2 x 8 KiB (weights) runs per plane:
    //   knn_tab  K uint16 node indices per voxel, ascending distance (16 B/voxel at K = 8: one dwordx4 per lane)
    //   w_tab    K float weights per voxel, stored as K/4 float4 PLANES of tab_nvox entries each, so that a wave of
    //            x-adjacent lanes reads 1 KiB contiguous per instruction
    uint16_t* knn_tab; float* w_tab; int tab_z0; size_t tab_nvox; int tab_ntx, tab_nty;
    int zt;                        // pipelined sweep: tile layers per workgroup (1..16)
    int v2w_identity;              // vol2world.R is exactly the identity (set by the launcher)
    int sat_ok;                    // trunc inside the domain of the saturated-sample shortcut (df_sat_trunc_ok; set by the launcher)
    // pipelined sweep: the launch plan.  A STRIP item is half a 32 x 16 tile column (4 patches of 8 x 8 columns side by side: the
    // waves that share the 128-byte lines of the voxel rows) over one block of zt tile layers; item = ((zb * tiles_y + ty) * tiles_x
    // + tx) * 2 + half.  plan_mask[item] holds its 4 x 16 verdict bits (bit 16 p + l: patch p, layer l alive); the items with w > 0
    // bits set are listed in bin w (plan_bins[w * plan_items ...], plan_cnt[w] of them) -- all made on the stream by
    // df_sweep_plan_kernel, so the sweep's workgroups are full of work from the first to the last, whatever the frustum cuts out.
    const unsigned long long* plan_mask; const unsigned int* plan_bins; const unsigned int* plan_cnt; unsigned int plan_items; int plan_tiles_y;
    // the verdict pass's list lengths (device, this frame's counter set) and where the plan kernel reports them to the host (pinned; both nullable)
    const uint32_t* blk_cnt; uint32_t* host_report; uint32_t sweep_no;
#ifdef DF_TRACE_WG
    unsigned long long* trace;     // [waves][4]: start, end (s_memrealtime), hw id, alive layers
#endif
    // max over the voxels of each table tile of sum_i w_i (written by the table build, frame-invariant); null = no zero-weight test
    float* tile_wmax;
    // this frame's verdicts of the block blend models (dfusion_warp_blocks.h), one byte per 8 x 8 x 8 block of the table's planes,
    // x fastest; null = none.  bm_nbx / bm_nby: blocks per row / column (whole table tiles)
    const uint8_t* blk_alive; int bm_nbx, bm_nby;
    // 4-bit neighbour codes (null = none): see df_code_index / df_block_model_kernel
    uint32_t* code_tab; uint32_t* bm_ids; uint8_t* bm_coded;
    const unsigned long long* plan_code;       // pipelined sweep: per strip item, bit 16 p + l: the cell's block has codes
    // table build (df_warp_brick_kernel<K, true>): per-block bound on sum_i w_i (same block grid), and -- when the build is driven by a
    // work list instead of the launch grid -- the list of packed brick coordinates (x | y << 10 | z << 20) and its length
    float* blk_wmax; const uint32_t* work; const uint32_t* work_cnt; uint32_t* work_cursor;
    // verdict pass: look-ahead margin (metres; 0 = none).  Blocks that are not alive this frame but would be with every radius
    // widened by this much are "near": their tables / blend models are made off the critical path (dfusion_warp_blocks.h)
    float pf_margin;
    unsigned pf_cap;               // look-ahead builds per frame at most (the list's counter may run past it)
    unsigned work_cap;             // list-driven build: entries of the list at most (0 = all)
    uint8_t* blk_tie;              // table build: per block (blk_wmax's grid), set to 1 when a voxel's top-k met an exact distance tie (nullable)
};
// A tile is ZERO-WEIGHT for a frame when tile_wmax * max_j |rot_j| < 2^-76: every component of every voxel's blend sum
// sum_i w_i rot_i is then below 2^-75 in magnitude (the 2x margin covers the rounding of the sums), its square below 2^-150
// rounds to 0 in f32, the norm is 0, the reference's 1.0 / norm is inf, inf * c is inf or NaN, the second normalize makes every
// component NaN and the NaN position fails vc.z > 0 (tsdf_volume.cu:86): no voxel of the tile can update.  Far from every
// node (> 10 sigma) that is the normal case, and such tiles are skipped without reading their tables.
#define DF_ZERO_WEIGHT 1.3234890e-23f      // 2^-76

// table entry of voxel (x, y, z): tiles of 32(x) x 16(y) x 8(z) voxels, tile-major; inside a tile z, then y, then x --
// a wave of the sweep (32 x-lanes x 2 y rows) reads 64 consecutive entries, a workgroup plane 512.
#define DF_TAB_TX 32
#define DF_TAB_TY 16
#define DF_TAB_TZ 8
// Inside a tile plane (32 x 16 voxels): rows of 32.  (Round 5 measured the alternative -- the eight 8 x 8 column patches one after the
// other, a wave's 64 records as ONE 1 KiB run -- same box, interleaved: 0.691 against 0.686 ms at 512^3, profiles/r05_ab_warp_variants.txt:
// the four waves of a strip fetch the pieces of a row's lines together anyway.)
__device__ __forceinline__ unsigned df_tab_in_plane(int x, int y)
{
    const unsigned xt = (unsigned)x % DF_TAB_TX, yt = (unsigned)y % DF_TAB_TY;
    return yt * DF_TAB_TX + xt;
}
__device__ __forceinline__ size_t df_tab_index(const DfWarpedArgs& a, int x, int y, int z)
{
    const int zl = z - a.tab_z0;
    const size_t tile = ((size_t)(zl / DF_TAB_TZ) * a.tab_nty + (y / DF_TAB_TY)) * a.tab_ntx + (x / DF_TAB_TX);
    return tile * (DF_TAB_TX * DF_TAB_TY * DF_TAB_TZ) + (size_t)(zl % DF_TAB_TZ) * (DF_TAB_TX * DF_TAB_TY) + df_tab_in_plane(x, y);
}

// entry of voxel (x, y, z) in the CODE table: the tables' tiles, but patch-major inside a tile plane (the eight 8 x 8 column patches one
// after the other) -- the 64 codes a wave of the pipelined sweep loads for its 8 x 8 patch are ONE 256-byte run, two L2 requests.  (The
// sweep is bound by the L2's request rate, TCC 86 % busy: measured, the same 4 bytes per voxel laid out in rows of 32 -- eight 32-byte
// pieces per wave -- cost as much as the 16-byte index records they replace.)
__device__ __forceinline__ unsigned df_code_in_plane(int x, int y)
{
    const unsigned xt = (unsigned)x % DF_TAB_TX, yt = (unsigned)y % DF_TAB_TY;
    return (((yt >> 3) * (DF_TAB_TX / 8) + (xt >> 3)) << 6) + ((yt & 7u) << 3) + (xt & 7u);
}
__device__ __forceinline__ size_t df_code_index(const DfWarpedArgs& a, int x, int y, int z)
{
    const int zl = z - a.tab_z0;
    const size_t tile = ((size_t)(zl / DF_TAB_TZ) * a.tab_nty + (y / DF_TAB_TY)) * a.tab_ntx + (x / DF_TAB_TX);
    return tile * (DF_TAB_TX * DF_TAB_TY * DF_TAB_TZ) + (size_t)(zl % DF_TAB_TZ) * (DF_TAB_TX * DF_TAB_TY) + df_code_in_plane(x, y);
}

#define DF_CAND_CHUNK 256

template <int K>
__device__ __forceinline__ void knn_tab_store(uint16_t* tab, size_t voxel, const int (&bi)[K])
{
    if constexpr (K == 8) {
        uint4 v;
        v.x = (uint32_t)bi[0] | ((uint32_t)bi[1] << 16); v.y = (uint32_t)bi[2] | ((uint32_t)bi[3] << 16);
        v.z = (uint32_t)bi[4] | ((uint32_t)bi[5] << 16); v.w = (uint32_t)bi[6] | ((uint32_t)bi[7] << 16);
        reinterpret_cast<uint4*>(tab)[voxel] = v;
    } else if constexpr (K == 4) {
        uint2 v;
        v.x = (uint32_t)bi[0] | ((uint32_t)bi[1] << 16); v.y = (uint32_t)bi[2] | ((uint32_t)bi[3] << 16);
        reinterpret_cast<uint2*>(tab)[voxel] = v;
    } else {
#pragma unroll
        for (int i = 0; i < K; ++i) tab[voxel * K + i] = (uint16_t)bi[i];
    }
}
template <int K>
__device__ __forceinline__ void knn_tab_load(const uint16_t* tab, size_t voxel, int (&bi)[K])
{
    if constexpr (K == 8) {
        const uint4 v = reinterpret_cast<const uint4*>(tab)[voxel];
        bi[0] = v.x & 0xffff; bi[1] = v.x >> 16; bi[2] = v.y & 0xffff; bi[3] = v.y >> 16;
        bi[4] = v.z & 0xffff; bi[5] = v.z >> 16; bi[6] = v.w & 0xffff; bi[7] = v.w >> 16;
    } else if constexpr (K == 4) {
        const uint2 v = reinterpret_cast<const uint2*>(tab)[voxel];
        bi[0] = v.x & 0xffff; bi[1] = v.x >> 16; bi[2] = v.y & 0xffff; bi[3] = v.y >> 16;
    } else {
#pragma unroll
        for (int i = 0; i < K; ++i) bi[i] = tab[voxel * K + i];
    }
}
template <int K>
__device__ __forceinline__ void w_tab_store(float* tab, size_t nvox, size_t voxel, const float (&wt)[K])
{
    if constexpr (K % 4 == 0) {
#pragma unroll
        for (int i = 0; i < K / 4; ++i)
            reinterpret_cast<float4*>(tab)[(size_t)i * nvox + voxel] = make_float4(wt[4 * i], wt[4 * i + 1], wt[4 * i + 2], wt[4 * i + 3]);
    } else {
#pragma unroll
        for (int i = 0; i < K; ++i) tab[(size_t)i * nvox + voxel] = wt[i];
    }
}
template <int K>
__device__ __forceinline__ void w_tab_load(const float* tab, size_t nvox, size_t voxel, float (&wt)[K])
{
    if constexpr (K % 4 == 0) {
#pragma unroll
        for (int i = 0; i < K / 4; ++i) {
            const float4 v = reinterpret_cast<const float4*>(tab)[(size_t)i * nvox + voxel];
            wt[4 * i] = v.x; wt[4 * i + 1] = v.y; wt[4 * i + 2] = v.z; wt[4 * i + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < K; ++i) wt[i] = tab[(size_t)i * nvox + voxel];
    }
}

// Conservative, result-identical rejection of a whole work tile (brick or row tile).  Every voxel of the tile has
// canonical position within tile_r of the tile centre c; its warped position is within
//   delta = 2 sin(theta_max/2) * (|c| + tile_r) + k * max|t_i|
// of its canonical one: the blend of unit quaternions with w >= 0 and weights >= 0 rotates (about the origin) by at
// most theta_max, and |T| = |sum w_i t_i| <= k max|t_i| because w_i = exp(-..) <= 1.  So its camera-frame position
// lies within rho = cam_scale*(tile_r + delta) of cc = world2cam * c.  No voxel of the tile can update if that ball
// is entirely behind the camera, entirely outside one image-frustum side plane, or entirely farther from the camera centre than
// (the largest dists value it can meet) + trunc.
// The DISTANCE from the camera centre moves much less than the position: the blend rotates about the world origin, which is
// origin_cam from the camera centre, so |R x - o| = |x - R^T o| differs from |x - o| by at most 2 sin(theta_max/2) |o| -- not
// (|c| + tile_r) -- and the distance of every warped voxel is at least |cc| - rho_r,
//   rho_r = tile_r + 2 sin(theta_max/2) * origin_cam + k * max|t_i|        (rigid world2cam; rho otherwise).
// "The largest dists value it can meet" is the maximum over the pixel rectangle the ball projects into (max-pyramid of the frame's
// dists, dfusion_pyramid.h), or over the whole image where there is no pyramid or the ball reaches the camera plane.
// wk >= sum_i w_i of every voxel of the tile: (float)k always (w_i <= 1), the table build's per-tile bound where there is one
// `extra` (metres, >= 0) widens every radius: the verdict pass's look-ahead test ("could be alive within the next few frames").
__device__ __forceinline__ bool df_tile_culled(const DfWarpedArgs& a, f3 c, float wk, float extra = 0.f)
{
    const float max_t = a.cull[0], sin_half = a.cull[1];
    if (!(sin_half <= 1.0f && max_t < 1.0e30f)) return false;
    float max_dist;                                                              // image-wide: the pyramid's top texel, or df_dists_max_kernel's result
    if (a.py.top != 0) { const uint32_t tb = df_pyramid_image_max(a.py); max_dist = tb < 0x7c00u ? h2f_bits((uint16_t)tb) : 3.0e38f; }
    else max_dist = a.cull[2];
    const float cn = sqrtf(dot3(c, c));
    const float delta = 2.f * sin_half * (cn + a.tile_r) + wk * max_t;
    const float rho = a.cam_scale * (a.tile_r + delta + extra) * 1.002f + 1e-3f;
    const float rho_r = a.origin_cam >= 0.f ? fminf(rho, (a.tile_r + 2.f * sin_half * a.origin_cam + wk * max_t + extra) * 1.002f + 1e-3f) : rho;   // (both bounds hold)
    const f3 cc = aff_mul(a.world2cam, c);
    const float rmin = sqrtf(dot3(cc, cc)) - rho_r;                              // no warped voxel of the tile is nearer to the camera centre
    bool out = false;
    if (cc.z + rho <= 0.f) out = true;                                           // behind the camera
    if (rmin > max_dist * 1.002f + a.P.trunc) out = true;                        // sdf < -trunc everywhere
    // side planes through the camera centre: u >= 0 <=> fx*x + cx*z >= 0 ; u < cols <=> -fx*x + (cols-cx)*z > 0
    const float nl = sqrtf(a.P.fx * a.P.fx + a.P.cx * a.P.cx);
    if ((a.P.fx * cc.x + a.P.cx * cc.z) / nl < -rho) out = true;
    const float cr = (float)a.P.cols - a.P.cx;
    const float nr = sqrtf(a.P.fx * a.P.fx + cr * cr);
    if ((-a.P.fx * cc.x + cr * cc.z) / nr < -rho) out = true;
    const float nt = sqrtf(a.P.fy * a.P.fy + a.P.cy * a.P.cy);
    if ((a.P.fy * cc.y + a.P.cy * cc.z) / nt < -rho) out = true;
    const float cb = (float)a.P.rows - a.P.cy;
    const float nbt = sqrtf(a.P.fy * a.P.fy + cb * cb);
    if ((-a.P.fy * cc.y + cb * cc.z) / nbt < -rho) out = true;
    // the pixels the ball can project to: the box [cc - rho, cc + rho] over the depths [zl, zh], two pixels of margin for the
    // rounding of the projection and of the pixel pick (device.hpp:35-37)
    const float zl = cc.z - rho, zh = cc.z + rho;
    if (!out && a.py.top != 0 && zl > 0.05f) {
        const float il = 1.f / zl, ih = 1.f / zh;
        const float xl = cc.x - rho, xh = cc.x + rho, yl = cc.y - rho, yh = cc.y + rho;
        const float ulo = a.P.fx * fminf(xl * il, xl * ih) + a.P.cx - 2.f, uhi = a.P.fx * fmaxf(xh * il, xh * ih) + a.P.cx + 2.f;
        const float vlo = a.P.fy * fminf(yl * il, yl * ih) + a.P.cy - 2.f, vhi = a.P.fy * fmaxf(yh * il, yh * ih) + a.P.cy + 2.f;
        if (ulo == ulo && uhi == uhi && vlo == vlo && vhi == vhi) {
            if (uhi < 0.f || vhi < 0.f || ulo > (float)(a.P.cols - 1) || vlo > (float)(a.P.rows - 1)) out = true;   // projects outside the image
            else {
                const int iu0 = (int)fmaxf(ulo, 0.f), iv0 = (int)fmaxf(vlo, 0.f);
                const int iu1 = (int)fminf(uhi, (float)(a.P.cols - 1)), iv1 = (int)fminf(vhi, (float)(a.P.rows - 1));
                const uint32_t dbits = df_pyramid_max_fine(a.py, iu0, iv0, iu1, iv1, 2);        // <= 5 x 5 texels
                if (dbits == 0u) out = true;                                     // no valid depth anywhere it can project to (Dp == 0, :86)
                else if (dbits < 0x7c00u && rmin > h2f_bits((uint16_t)dbits) * 1.002f + a.P.trunc) out = true;   // finite non-negative lengths only
            }
        }
    }
    return out;
}

#include "dfusion_warp_blocks.h"

// blend -> transform -> project -> fuse for one voxel; returns 1 if the update branch was taken
template <int K>
__device__ __forceinline__ unsigned int df_warp_update(const DfWarpedArgs& a, const DfWarpView& W, f3 q, const float (&wt)[K],
                                                       const int (&bi)[K], uint32_t* vox)
{
    quat rot, dual;
    dqb_blend_w<K>(W, wt, bi, &rot, &dual);
    const f3 vc = aff_mul(a.world2cam, dq_transform(rot, dual, q));
    float ts;
    if (!tsdf_sample(a.P, vc, &ts)) return 0u;
    *vox = tsdf_fuse(*vox, ts, a.P.max_weight);
    return 1u;
}

__device__ __forceinline__ void df_count_updates(const DfWarpedArgs& a, unsigned int my_upd)
{
    if (a.n_upd) {
        unsigned int s = my_upd;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(a.n_upd, (unsigned long long)s);
    }
}

// ---- brick kernel: exact k-NN from the brick candidate lists (through LDS), one 256-thread workgroup per 8^3 brick.
// BUILD = false: fused with the TSDF update -- no per-voxel memory ("lean" path, re-ranks ~150 candidates per voxel per frame).
// BUILD = true : writes the per-voxel k-NN (and weight) tables instead; run when node POSITIONS change, not per frame.
template <int K, bool BUILD>
__device__ __forceinline__ void df_warp_brick_body(const DfWarpedArgs& a, const DfWarpView& W, const int bxx, const int byy, const int bzz,
                                                   float4* s_pos, uint16_t* s_idx, float* s_key)
{
    const int b = (bzz * W.by + byy) * W.bx + bxx;

    const int t = threadIdx.x;
    const int lx = t & 7, ly = (t >> 3) & 7, lz = t >> 6;           // lz in 0..3 ; each thread does z = lz and lz+4
    const int x = bxx * DF_BRICK + lx, y = byy * DF_BRICK + ly;
    const int z0 = bzz * DF_BRICK + lz, z1 = z0 + 4;

    if (!BUILD && a.cull) {
        const f3 c = aff_mul(a.vol2world, mk3(((float)(bxx * DF_BRICK) + 3.5f) * a.vsx, ((float)(byy * DF_BRICK) + 3.5f) * a.vsy,
                                              ((float)(bzz * DF_BRICK) + 3.5f) * a.vsz));
        if (df_tile_culled(a, c, a.kf)) return;                           // block-uniform
    }

    const bool in_xy = x < a.X && y < a.Y;
    const bool act0 = in_xy && z0 >= a.z_own0 && z0 < a.z_own0 + a.z_own_n && z0 < a.Z;
    const bool act1 = in_xy && z1 >= a.z_own0 && z1 < a.z_own0 + a.z_own_n && z1 < a.Z;

    // canonical positions
    const float fxv = (float)x * a.vsx, fyv = (float)y * a.vsy;
    const f3 q0 = aff_mul(a.vol2world, mk3(fxv, fyv, (float)z0 * a.vsz));
    const f3 q1 = aff_mul(a.vol2world, mk3(fxv, fyv, (float)z1 * a.vsz));

    float bd0[K], bd1[K]; int bi0[K], bi1[K];
    topk_init<K>(bd0, bi0);
    topk_init<K>(bd1, bi1);
    const uint32_t off = W.brick_off[b];
    const uint32_t cnt = W.brick_off[b + 1] - off;
    [[maybe_unused]] bool tie = false;               // (BUILD) topk_insert took its equal-distance branch: the tie tree decided
    // The candidates are visited NEAREST (to the brick's centre) FIRST: the result does not depend on the order (topk_insert places
    // equal distances by the reference's rule whatever the arrival order), but the cost does -- an insert runs for the whole wave when
    // any lane needs it, and with the near nodes seen first the lists are final after a third of the candidates and the rest fail the
    // first compare in every lane.  A chunk is sorted in LDS by a bitonic network over the next power of two (<= 36 steps).
    const f3 cb = aff_mul(a.vol2world, mk3(((float)(bxx * DF_BRICK) + 3.5f) * a.vsx, ((float)(byy * DF_BRICK) + 3.5f) * a.vsy,
                                           ((float)(bzz * DF_BRICK) + 3.5f) * a.vsz));
    for (uint32_t base = 0; base < cnt; base += DF_CAND_CHUNK) {
        const int n = (int)min((uint32_t)DF_CAND_CHUNK, cnt - base);
        unsigned np2 = 2;
        while ((int)np2 < n) np2 <<= 1;
        __syncthreads();
        {
            uint16_t j = 0; float key = __uint_as_float(0x7f800000u);
            if (t < n) { j = W.brick_list[off + base + t]; const float4 p = W.pos_sigma[j]; key = knn_dist2(cb, p.x, p.y, p.z); key = key == key ? key : 3.0e38f; }
            s_key[t] = key; s_idx[t] = j;
        }
        __syncthreads();
        for (unsigned k2 = 2; k2 <= np2; k2 <<= 1)
            for (unsigned j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
                const unsigned p = (unsigned)t ^ j2;
                if ((unsigned)t < np2 && p > (unsigned)t) {
                    const float ka = s_key[t], kb = s_key[p];
                    if ((ka > kb) == (((unsigned)t & k2) == 0u)) {
                        s_key[t] = kb; s_key[p] = ka;
                        const uint16_t ia = s_idx[t]; s_idx[t] = s_idx[p]; s_idx[p] = ia;
                    }
                }
                __syncthreads();
            }
        if (t < n) s_pos[t] = W.pos_sigma[s_idx[t]];
        __syncthreads();
        for (int c = 0; c < n; ++c) {
            const float4 p = s_pos[c];                 // broadcast ds_read_b128
            const int j = s_idx[c];
            const float d0 = knn_dist2(q0, p.x, p.y, p.z), d1 = knn_dist2(q1, p.x, p.y, p.z);
            if constexpr (BUILD) tie = tie || df_topk_tie<K>(bd0, d0) || df_topk_tie<K>(bd1, d1);
            topk_insert<K>(bd0, bi0, d0, j, W.nf, q0);
            topk_insert<K>(bd1, bi1, d1, j, W.nf, q1);
        }
    }

    const size_t plane = (size_t)a.X * a.Y;
    float wt0[K], wt1[K];
    if constexpr (BUILD) {
        const size_t tv0 = df_tab_index(a, x, y, z0), tv1 = df_tab_index(a, x, y, z1);
        if (tie && a.blk_tie)                               // plain byte store; every lane that saw a tie writes the same 1
            a.blk_tie[((size_t)((bzz * DF_BRICK - a.tab_z0) / 8) * a.bm_nby + byy) * a.bm_nbx + bxx] = 1;
        float wsum = 0.f;
        if (act0) { knn_tab_store<K>(a.knn_tab, tv0, bi0); if (a.w_tab) { dqb_weights<K>(W, bd0, bi0, wt0); w_tab_store<K>(a.w_tab, a.tab_nvox, tv0, wt0); } }
        if (act1) { knn_tab_store<K>(a.knn_tab, tv1, bi1); if (a.w_tab) { dqb_weights<K>(W, bd1, bi1, wt1); w_tab_store<K>(a.w_tab, a.tab_nvox, tv1, wt1); } }
        if (a.w_tab && a.tile_wmax) {                       // a brick lies inside one table tile (8 | 32, 16, 8; table planes are brick-aligned)
            if (act0) {
                float s0 = 0.f;
#pragma unroll
                for (int i = 0; i < K; ++i) s0 += wt0[i];
                wsum = !(s0 == s0) ? 3.0e38f : s0;
            }
            if (act1) {
                float s1 = 0.f;
#pragma unroll
                for (int i = 0; i < K; ++i) s1 += wt1[i];
                wsum = fmaxf(wsum, !(s1 == s1) ? 3.0e38f : s1);
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) wsum = fmaxf(wsum, __shfl_xor(wsum, o, 64));
            if ((threadIdx.x & 63) == 0) {
                const int zl = bzz * DF_BRICK - a.tab_z0;
                const size_t tile = ((size_t)(zl / DF_TAB_TZ) * a.tab_nty + (byy * DF_BRICK) / DF_TAB_TY) * a.tab_ntx + (bxx * DF_BRICK) / DF_TAB_TX;
                atomicMax((unsigned int*)&a.tile_wmax[tile], __float_as_uint(wsum));      // non-negative floats order as uints
                if (a.blk_wmax)
                    atomicMax((unsigned int*)&a.blk_wmax[((size_t)(zl / 8) * a.bm_nby + byy) * a.bm_nbx + bxx], __float_as_uint(wsum));
            }
        }
    } else {
        unsigned int my_upd = 0;
        if (act0) {
            dqb_weights<K>(W, bd0, bi0, wt0);
            my_upd += df_warp_update<K>(a, W, q0, wt0, bi0, a.vol + (size_t)(z0 - a.z_store0) * plane + (size_t)y * a.X + x);
        }
        if (act1) {
            dqb_weights<K>(W, bd1, bi1, wt1);
            my_upd += df_warp_update<K>(a, W, q1, wt1, bi1, a.vol + (size_t)(z1 - a.z_store0) * plane + (size_t)y * a.X + x);
        }
        df_count_updates(a, my_upd);
    }
}

template <int K, bool BUILD>
__global__ __launch_bounds__(256) void df_warp_brick_kernel(const DfWarpedArgs a, const DfWarpView W)
{
    __shared__ float4 s_pos[DF_CAND_CHUNK];
    __shared__ uint16_t s_idx[DF_CAND_CHUNK];
    __shared__ float s_key[DF_CAND_CHUNK];
    if (BUILD && a.work) {                                                 // on-demand build: the bricks of a work list, over a resident grid
        __shared__ uint32_t s_item;                                        // (drawn one at a time: a brick costs 20-80 us, unevenly)
        const uint32_t n = a.work_cap ? min(*a.work_cnt, a.work_cap) : *a.work_cnt;
        for (uint32_t round = 0;; ++round) {
            uint32_t i = blockIdx.x;                                       // the first brick without an atomic (an empty list costs nothing)
            if (round) {
                if (threadIdx.x == 0) s_item = atomicAdd(a.work_cursor, 1u) + gridDim.x;
                __syncthreads();
                i = s_item;
            }
            if (i >= n) break;
            const uint32_t code = a.work[i];
            df_warp_brick_body<K, BUILD>(a, W, (int)(code & 1023u), (int)((code >> 10) & 1023u), (int)(code >> 20), s_pos, s_idx, s_key);
            __syncthreads();
        }
        return;
    }
    df_warp_brick_body<K, BUILD>(a, W, (int)(blockIdx.x % (unsigned)W.bx), (int)(blockIdx.x / (unsigned)W.bx), a.bz0 + (int)blockIdx.y, s_pos, s_idx, s_key);
}

// ---- row-tile kernel: the per-frame sweep when the per-voxel tables are cached in HBM.
// The exact k-NN of a voxel (and its k blend weights) depend only on canonical node positions, so with 288 GB of HBM
// they are computed once per node set and streamed back every frame: 16 B (+32 B) per voxel at k = 8 instead of
// re-ranking ~150 candidates (and 8 f32 divisions + 8 f64 exp) per voxel.  A workgroup owns a 32(x) x 8(y) x 8(z) tile:
// a wave covers two 32-voxel rows, so every access is a run of >= 128 contiguous bytes (volume 4 B, k-NN 16 B, weights
// 16 B per lane and plane); each lane walks the 8 planes of the tile.
// ---- geometry of the pipelined sweep.  (Rounds 4-5 measured, and dropped, a series of compile-time variants of it -- 32 x 2 patches, an
// f32-division normalisation, a short fuse division, split LDS node arrays, patch-major tables, both-loads code records: profiles/NOTES.md
// and profiles/r05_ab_warp_variants.txt hold the numbers; the source keeps only what runs.)
#define DF_PIPE_WGT 256           // threads of a k = 8 sweep workgroup: 4 waves dealing out ONE strip item; <= 80 VGPRs: 6 workgroups per CU = 6 waves / SIMD.
                                  // (Rounds 4-5 ran 768: the 64 KiB LDS node table left room for two workgroups per CU, so each had to bring 12 waves.
                                  // Without the table the size is free, and a CU refills 4 wave slots as soon as a SMALL workgroup ends instead of
                                  // waiting for the last of 12 waves: a per-wave timeline showed ~4100 of 6144 slots filled at 768 threads.  Same
                                  // box, interleaved: 256 threads 0.577 ms, 512 0.580, 768 0.594, 128 0.622 (profiles/r06_ab_wgsize.txt).)
#define DF_ROW_TX 32
#define DF_ROW_TY 8
#define DF_ROW_TZ 8

template <int K, bool HAS_W, int UNROLL>
__global__ __launch_bounds__(256, UNROLL) void df_warp_rows_kernel(const DfWarpedArgs a, const DfWarpView W, int tiles_x)
{
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int zt = a.bz0 + blockIdx.y;                                 // tile layer (DF_ROW_TZ planes)
    if (a.cull) {
        const f3 c = aff_mul(a.vol2world, mk3(((float)(tx * DF_ROW_TX) + 0.5f * (DF_ROW_TX - 1)) * a.vsx,
                                              ((float)(ty * DF_ROW_TY) + 0.5f * (DF_ROW_TY - 1)) * a.vsy,
                                              ((float)(zt * DF_ROW_TZ) + 0.5f * (DF_ROW_TZ - 1)) * a.vsz));
        if (df_tile_culled(a, c, a.kf)) return;                               // block-uniform
    }
    const int x = tx * DF_ROW_TX + (threadIdx.x & (DF_ROW_TX - 1));
    const int y = ty * DF_ROW_TY + (threadIdx.x >> 5);
    const bool in_xy = x < a.X && y < a.Y;
    const size_t plane = (size_t)a.X * a.Y;
    const float fxv = (float)x * a.vsx, fyv = (float)y * a.vsy;
    const int zb = max(zt * DF_ROW_TZ, a.z_own0), ze = min(min((zt + 1) * DF_ROW_TZ, a.z_own0 + a.z_own_n), a.Z);
    unsigned int my_upd = 0;
    if (in_xy) {
        for (int z = zb; z < ze; ++z) {
            const size_t tv = df_tab_index(a, x, y, z);
            const f3 q = aff_mul(a.vol2world, mk3(fxv, fyv, (float)z * a.vsz));     // canonical position
            int bi[K]; float wt[K];
            knn_tab_load<K>(a.knn_tab, tv, bi);
            if constexpr (HAS_W) {
                w_tab_load<K>(a.w_tab, a.tab_nvox, tv, wt);
            } else {
                // distances recomputed with the expression the build used (knn_point_cloud.hpp:25-31): bit-identical
#pragma unroll
                for (int i = 0; i < K; ++i) { const float4 p = W.pos_sigma[bi[i]]; wt[i] = dqb_weight(knn_dist2(q, p.x, p.y, p.z), p.w); }
            }
            my_upd += df_warp_update<K>(a, W, q, wt, bi, a.vol + (size_t)(z - a.z_store0) * plane + (size_t)y * a.X + x);
        }
    }
    df_count_updates(a, my_upd);
}

// ---- row-tile kernel, node transforms in LDS.  PMC on the kernel above: ~116 vector-memory instructions per wave, 16 of
// every 19 being 16-byte node gathers through the texture-address path (64 lanes x 16 B = 16 TA cycles each) -- on par
// with the HBM time of the table stream.  When the whole node table fits (M * 32 B <= 128 KiB, i.e. M <= 4096), a
// 512-thread workgroup stages rot + node_t of ALL nodes in LDS once and walks DF_LDS_ZT tile layers; gathers become
// ds_read_b128 (256 B/clk/CU, identical addresses broadcast).  Two such workgroups fill a CU (160 KiB LDS, 16 waves).
#define DF_LDS_TY 16
#define DF_LDS_ZT 8          // tile layers (of DF_ROW_TZ planes) walked per workgroup (batched kernel; the pipelined one takes a.zt)

template <int K, bool HAS_W, int NB>
__global__ __launch_bounds__(512) void df_warp_rows_lds_kernel(const DfWarpedArgs a, const DfWarpView W, int tiles_x)
{
    extern __shared__ __attribute__((aligned(16))) float4 s_nodes[];     // [2M]: rot_j, node_t_j interleaved
    for (int j = threadIdx.x; j < W.M; j += 512) { s_nodes[2 * j] = W.rot[j]; s_nodes[2 * j + 1] = W.node_t[j]; }
    __syncthreads();

    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int x = tx * DF_ROW_TX + (threadIdx.x & (DF_ROW_TX - 1));
    const int y = ty * DF_LDS_TY + (threadIdx.x >> 5);
    const bool in_xy = x < a.X && y < a.Y;
    const size_t plane = (size_t)a.X * a.Y;
    const float fxv = (float)x * a.vsx, fyv = (float)y * a.vsy;
    unsigned int my_upd = 0;
    // the verdicts of the workgroup's layers first (lane l judges layer l, a ballot collects them): what the test needs is then
    // dead before the sweep starts
    unsigned alive;
    {
        const int l = threadIdx.x & 7;
        const int zt = a.bz0 + blockIdx.y * DF_LDS_ZT + l;
        bool keep = max(zt * DF_ROW_TZ, a.z_own0) < min(min((zt + 1) * DF_ROW_TZ, a.z_own0 + a.z_own_n), a.Z);
        if (keep && a.cull) {
            const f3 c = aff_mul(a.vol2world, mk3(((float)(tx * DF_ROW_TX) + 0.5f * (DF_ROW_TX - 1)) * a.vsx,
                                                  ((float)(ty * DF_LDS_TY) + 0.5f * (DF_LDS_TY - 1)) * a.vsy,
                                                  ((float)(zt * DF_ROW_TZ) + 0.5f * (DF_ROW_TZ - 1)) * a.vsz));
            keep = !df_tile_culled(a, c, a.kf);
        }
        alive = (unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned)__builtin_amdgcn_ballot_w64(keep) & 0xffu));   // block-uniform
    }
    for (int l = 0; l < DF_LDS_ZT; ++l) {
        if (!((alive >> l) & 1u)) continue;
        const int zt = a.bz0 + blockIdx.y * DF_LDS_ZT + l;                // tile layer (DF_ROW_TZ planes)
        const int zb = max(zt * DF_ROW_TZ, a.z_own0), ze = min(min((zt + 1) * DF_ROW_TZ, a.z_own0 + a.z_own_n), a.Z);
        if (!in_xy) continue;
        // NB planes per batch: all table loads of the batch are issued back to back (NB * 3 KiB in flight per wave),
        // then the NB voxels are blended one after the other -- memory-level parallelism without more waves.
        for (int z0 = zb; z0 < ze; z0 += NB) {
            int bi[NB][K]; float wt[NB][K];
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const int z = min(z0 + u, ze - 1);                        // clamp: tail lanes re-read a valid entry
                const size_t tv = df_tab_index(a, x, y, z);
                knn_tab_load<K>(a.knn_tab, tv, bi[u]);
                if constexpr (HAS_W) w_tab_load<K>(a.w_tab, a.tab_nvox, tv, wt[u]);
            }
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const int z = z0 + u;
                if (z < ze) {
                    const f3 q = aff_mul(a.vol2world, mk3(fxv, fyv, (float)z * a.vsz));     // canonical position
                    if constexpr (!HAS_W) {
#pragma unroll
                        for (int i = 0; i < K; ++i) { const float4 p = W.pos_sigma[bi[u][i]]; wt[u][i] = dqb_weight(knn_dist2(q, p.x, p.y, p.z), p.w); }
                    }
                    quat rot, dual;
                    dqb_blend_lds<K>(s_nodes, wt[u], bi[u], &rot, &dual);
                    const f3 vc = aff_mul(a.world2cam, dq_transform(rot, dual, q));
                    float ts;
                    if (tsdf_sample(a.P, vc, &ts)) {
                        uint32_t* vox = a.vol + (size_t)(z - a.z_store0) * plane + (size_t)y * a.X + x;
                        *vox = tsdf_fuse(*vox, ts, a.P.max_weight);
                        ++my_upd;
                    }
                }
            }
        }
    }
    df_count_updates(a, my_upd);
}

// ---- software-pipelined form of the kernel above (the default).  PMC on the batched kernel: waves spend ~45 % of their
// cycles parked on the table loads and raising occupancy is not possible (~100 VGPRs),
// so the loads of batch b+1 are issued in the middle of batch b.  Vector-memory results return IN ORDER (vmcnt), hence the
// order inside a batch matters:  volume words + dists gathers of batch b (needed now)  ->  table loads of batch b+1 (needed
// next iteration)  ->  wait only for the former (vmcnt leaves the 6 prefetches in flight)  ->  sqrt / fuse / store, then the
// whole blend of batch b+1 runs while nothing is waited for.  The sample is the branch-free form (clamped, always-valid
// dists address; same verdict as tsdf_sample for every voxel) so the gathers can be issued before the verdict is known; the
// voxel word is read unconditionally (it is the read half of the RMW for 1 voxel in 4, +4 B for the others).
// raw (still packed) table record of one voxel: kept packed while in flight, so that nothing consumes a prefetched
// register before the next iteration (an unpack right after the load would make the compiler wait for it at once)
template <int K> struct DfTabRaw;
template <> struct DfTabRaw<8> { uint4 idx; float4 w0, w1; unsigned code; };
template <> struct DfTabRaw<4> { uint2 idx; float4 w0; };
__device__ __forceinline__ void tab_raw_load(const DfWarpedArgs& a, size_t tv, DfTabRaw<8>& r)
{
    r.idx = reinterpret_cast<const uint4*>(a.knn_tab)[tv];
    r.w0 = reinterpret_cast<const float4*>(a.w_tab)[tv];
    r.w1 = reinterpret_cast<const float4*>(a.w_tab)[a.tab_nvox + tv];
}
__device__ __forceinline__ void tab_raw_load(const DfWarpedArgs& a, size_t tv, DfTabRaw<4>& r)
{
    r.idx = reinterpret_cast<const uint2*>(a.knn_tab)[tv];
    r.w0 = reinterpret_cast<const float4*>(a.w_tab)[tv];
}
// A pointer the whole wave agrees on, moved to scalar registers: address = SGPR base + 32-bit lane offset is then one
// instruction operand (global_load ... v_off, s[base]) instead of a 64-bit add per lane and a VGPR pair per address.  The
// result is typed as a GLOBAL (address space 1) pointer: rebuilt from integers it would otherwise be a generic one, its accesses
// FLAT instructions, and a pending FLAT load makes the compiler wait with vmcnt(0) -- which drains the table prefetch.
typedef float df_v4f __attribute__((ext_vector_type(4)));
typedef unsigned int df_v4u __attribute__((ext_vector_type(4)));
typedef unsigned int df_v2u __attribute__((ext_vector_type(2)));
template <typename T> using df_global_ptr = __attribute__((address_space(1))) T*;
template <typename T>
__device__ __forceinline__ df_global_ptr<T> df_wave_uniform(T* p)
{
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return (df_global_ptr<T>)(((unsigned long long)hi << 32) | lo);
}
// the per-voxel tables are read once per frame and never again before 5 GB of other data have gone by: non-temporal loads (`nt`)
#define DF_TAB_LD(p) __builtin_nontemporal_load(p)
// the record index split into a wave-uniform base and a 32-bit lane offset.  k = 8: a cell whose block has 4-bit neighbour codes loads
// the 4-byte code (record rec_c + lane_c of the patch-major code plane) INSTEAD of the 16-byte index record, behind a wave-uniform
// branch whose arms issue exactly one load each (the prefetch queue's vmcnt stays exact)
__device__ __forceinline__ void tab_raw_load_at(const DfWarpedArgs& a, size_t rec, size_t rec_c, bool coded, unsigned lane, unsigned lane_c, DfTabRaw<8>& r)
{
    r.idx = make_uint4(0u, 0u, 0u, 0u); r.code = 0u;
    if (coded) {
        r.code = DF_TAB_LD(df_wave_uniform(a.code_tab + rec_c) + lane_c);
    } else {
        const df_v4u i4 = DF_TAB_LD(df_wave_uniform(reinterpret_cast<const df_v4u*>(a.knn_tab) + rec) + lane);
        r.idx = make_uint4(i4.x, i4.y, i4.z, i4.w);
    }
    const df_v4f a4 = DF_TAB_LD(df_wave_uniform(reinterpret_cast<const df_v4f*>(a.w_tab) + rec) + lane);
    const df_v4f b4 = DF_TAB_LD(df_wave_uniform(reinterpret_cast<const df_v4f*>(a.w_tab) + a.tab_nvox + rec) + lane);
    r.w0 = make_float4(a4.x, a4.y, a4.z, a4.w); r.w1 = make_float4(b4.x, b4.y, b4.z, b4.w);
}
__device__ __forceinline__ void tab_raw_load_at(const DfWarpedArgs& a, size_t rec, size_t, bool, unsigned lane, unsigned, DfTabRaw<4>& r)
{
    const df_v2u i2 = DF_TAB_LD(df_wave_uniform(reinterpret_cast<const df_v2u*>(a.knn_tab) + rec) + lane);
    const df_v4f a4 = DF_TAB_LD(df_wave_uniform(reinterpret_cast<const df_v4f*>(a.w_tab) + rec) + lane);
    r.idx = make_uint2(i2.x, i2.y); r.w0 = make_float4(a4.x, a4.y, a4.z, a4.w);
}
__device__ __forceinline__ void tab_raw_unpack(const DfTabRaw<8>& r, int (&bi)[8], float (&wt)[8])
{
    bi[0] = r.idx.x & 0xffff; bi[1] = r.idx.x >> 16; bi[2] = r.idx.y & 0xffff; bi[3] = r.idx.y >> 16;
    bi[4] = r.idx.z & 0xffff; bi[5] = r.idx.z >> 16; bi[6] = r.idx.w & 0xffff; bi[7] = r.idx.w >> 16;
    wt[0] = r.w0.x; wt[1] = r.w0.y; wt[2] = r.w0.z; wt[3] = r.w0.w; wt[4] = r.w1.x; wt[5] = r.w1.y; wt[6] = r.w1.z; wt[7] = r.w1.w;
}
__device__ __forceinline__ void tab_raw_unpack(const DfTabRaw<4>& r, int (&bi)[4], float (&wt)[4])
{
    bi[0] = r.idx.x & 0xffff; bi[1] = r.idx.x >> 16; bi[2] = r.idx.y & 0xffff; bi[3] = r.idx.y >> 16;
    wt[0] = r.w0.x; wt[1] = r.w0.y; wt[2] = r.w0.z; wt[3] = r.w0.w;
}
// Byte offset of node `word` (0 = low, 1 = high 16 bits of v) in an interleaved {rot, node_t} node table: index * 32 in ONE instruction
// (SDWA selects the 16-bit word as the shift's operand; and + shift / bfe + shift otherwise, two per index, 16 per voxel).
__device__ __forceinline__ unsigned df_node_off_lo(unsigned v)
{
    unsigned r;
    asm("v_lshlrev_b32_sdwa %0, 5, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0" : "=v"(r) : "v"(v));
    return r;
}
__device__ __forceinline__ unsigned df_node_off_hi(unsigned v)
{
    unsigned r;
    asm("v_lshlrev_b32_sdwa %0, 5, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1" : "=v"(r) : "v"(v));
    return r;
}
// The LDS forms of the blend address the nodes by byte offsets into the workgroup's LDS.  The dynamic array is the kernel's only LDS
// object, so it starts at LDS address 0 and the offset IS the address -- df_warp_rows_pipe_kernel checks that.
typedef const __attribute__((address_space(3))) df_v4f df_lds_cf4;
// w.lo * q and w.hi * q on both halves of q: the weight is picked out of its register PAIR by op_sel (the table record delivers the
// weights two to a pair), instead of being copied into a {w, w} pair first -- 12 v_mov per voxel at k = 8.
__device__ __forceinline__ df_v2f df_pk_mul_lo(df_v2f w, df_v2f q)
{
    df_v2f r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(r) : "v"(w), "v"(q));
    return r;
}
__device__ __forceinline__ df_v2f df_pk_mul_hi(df_v2f w, df_v2f q)
{
    df_v2f r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(r) : "v"(w), "v"(q));
    return r;
}
// One pair of neighbours added to the blend sums (element-wise IEEE mul then add, the scalar sequence of warp_field.cpp:211-212), given
// their {rot, node_t} records
__device__ __forceinline__ void df_blend_acc(DfBlendSums& S, df_v2f wp, df_v4f r_lo, df_v4f t_lo, df_v4f r_hi, df_v4f t_hi)
{
    {
        const df_v2f ta = {t_lo.x, t_lo.y}, tb = {t_lo.z, t_lo.w}, ra = {r_lo.x, r_lo.y}, rb = {r_lo.z, r_lo.w};
        S.t01 = S.t01 + df_pk_mul_lo(wp, ta); S.t23 = S.t23 + df_pk_mul_lo(wp, tb);     // :211
        S.r01 = S.r01 + df_pk_mul_lo(wp, ra); S.r23 = S.r23 + df_pk_mul_lo(wp, rb);     // :212
    }
    {
        const df_v2f ta = {t_hi.x, t_hi.y}, tb = {t_hi.z, t_hi.w}, ra = {r_hi.x, r_hi.y}, rb = {r_hi.z, r_hi.w};
        S.t01 = S.t01 + df_pk_mul_hi(wp, ta); S.t23 = S.t23 + df_pk_mul_hi(wp, tb);
        S.r01 = S.r01 + df_pk_mul_hi(wp, ra); S.r23 = S.r23 + df_pk_mul_hi(wp, rb);
    }
}
// ... the two records read from LDS byte addresses
__device__ __forceinline__ void df_blend_pair_at(DfBlendSums& S, unsigned off_lo, unsigned off_hi, df_v2f wp)
{
    df_lds_cf4* nl = (df_lds_cf4*)(size_t)off_lo; df_lds_cf4* nh = (df_lds_cf4*)(size_t)off_hi;
    df_blend_acc(S, wp, nl[0], nl[1], nh[0], nh[1]);
}
// the blend sums straight from a packed table record: node offsets and weights are taken out of the loaded registers where they are used.
// (i) node table in LDS at address 0 (k = 4)
__device__ __forceinline__ DfBlendSums dqb_sums_lds_rec(const DfTabRaw<4>& r)
{
    DfBlendSums S;
    S.t01 = S.t23 = S.r01 = S.r23 = df_v2f{0.f, 0.f};
    df_blend_pair_at(S, df_node_off_lo(r.idx.x), df_node_off_hi(r.idx.x), df_v2f{r.w0.x, r.w0.y});
    df_blend_pair_at(S, df_node_off_lo(r.idx.y), df_node_off_hi(r.idx.y), df_v2f{r.w0.z, r.w0.w});
    return S;
}
// (ii) node table in global memory (the L2): W.rt, 32 bytes a node -- the cells without codes of the k = 8 sweep, and k = 4 node sets too
// large for the LDS
__device__ __forceinline__ void df_blend_pair_global(DfBlendSums& S, df_global_ptr<const char> rt, unsigned idx2, df_v2f wp)
{
    const df_global_ptr<const df_v4f> nl = (df_global_ptr<const df_v4f>)(rt + df_node_off_lo(idx2));
    const df_global_ptr<const df_v4f> nh = (df_global_ptr<const df_v4f>)(rt + df_node_off_hi(idx2));
    df_blend_acc(S, wp, nl[0], nl[1], nh[0], nh[1]);
}
__device__ __forceinline__ DfBlendSums dqb_sums_global_rec(const DfTabRaw<8>& r, df_global_ptr<const char> rt)
{
    DfBlendSums S;
    S.t01 = S.t23 = S.r01 = S.r23 = df_v2f{0.f, 0.f};
    df_blend_pair_global(S, rt, r.idx.x, df_v2f{r.w0.x, r.w0.y}); df_blend_pair_global(S, rt, r.idx.y, df_v2f{r.w0.z, r.w0.w});
    df_blend_pair_global(S, rt, r.idx.z, df_v2f{r.w1.x, r.w1.y}); df_blend_pair_global(S, rt, r.idx.w, df_v2f{r.w1.z, r.w1.w});
    return S;
}
__device__ __forceinline__ DfBlendSums dqb_sums_global_rec(const DfTabRaw<4>& r, df_global_ptr<const char> rt)
{
    DfBlendSums S;
    S.t01 = S.t23 = S.r01 = S.r23 = df_v2f{0.f, 0.f};
    df_blend_pair_global(S, rt, r.idx.x, df_v2f{r.w0.x, r.w0.y}); df_blend_pair_global(S, rt, r.idx.y, df_v2f{r.w0.z, r.w0.w});
    return S;
}
// (iii) from 4-bit codes: neighbour i = entry ((code >> 4 i) & 15) of the wave's LOCAL copy of the voxel's sub-block union (16 x 32 bytes at
// LDS address lbase, a multiple of 512, per lane: the four column quadrants of a wave's patch have a union each): a shift and an and-or per
// neighbour; the same nodes in the same order as the index record names, so the same sums.
__device__ __forceinline__ DfBlendSums dqb_sums_codes(const DfTabRaw<8>& r, unsigned lbase)
{
    DfBlendSums S;
    S.t01 = S.t23 = S.r01 = S.r23 = df_v2f{0.f, 0.f};
    const unsigned c = r.code;
#define DF_CODE_OFF(i) ((((i) == 0 ? (c << 5) : (i) == 1 ? (c << 1) : (c >> (4 * (i) - 5))) & 0x1e0u) | lbase)
    df_blend_pair_at(S, DF_CODE_OFF(0), DF_CODE_OFF(1), df_v2f{r.w0.x, r.w0.y}); df_blend_pair_at(S, DF_CODE_OFF(2), DF_CODE_OFF(3), df_v2f{r.w0.z, r.w0.w});
    df_blend_pair_at(S, DF_CODE_OFF(4), DF_CODE_OFF(5), df_v2f{r.w1.x, r.w1.y}); df_blend_pair_at(S, DF_CODE_OFF(6), DF_CODE_OFF(7), df_v2f{r.w1.z, r.w1.w});
#undef DF_CODE_OFF
    return S;
}

// the lane's number in its wave, made where it is used (two mbcnt instructions) instead of living in a register
__device__ __forceinline__ unsigned df_lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
// ... and in a form the optimiser cannot hoist out of a loop and keep (or spill) for the loop's whole life: two instructions per use
__device__ __forceinline__ unsigned df_lane_id_here()
{
    unsigned r;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(r));
    return r;
}
// buffer descriptor of one volume plane (raw: stride 0, num_records in bytes; out-of-range lanes read 0 / store nothing)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t df_plane_rsrc(uint32_t* plane_ptr, unsigned bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc((void*)df_wave_uniform(plane_ptr), (short)0, (int)bytes, 0x00020000);
}

// The launch plan of the pipelined sweep.  One wave per strip item: lane = (patch p = lane / 16, layer l = lane % 16) judges the
// 8 x 8 x 8 voxels of its patch and layer (the verdict costs ~200 instructions; in the sweep itself it held a workgroup's LDS while
// it ran); the ballot is the item's mask, its population count w the item's work.  Alive items go into bin w (bins[w * n_items ...],
// cnt[w] entries; the order inside a bin is whatever the atomics make it -- items are independent, the result does not depend on
// it): the sweep takes the bins from w = 64 down, i.e. the items most work first, without a sorting pass.  `cnt_next` is the counter
// set of the NEXT launch (the two sets alternate), zeroed here: nothing reads it any more once this kernel runs.
#define DF_PLAN_BINS 65
#define DF_PLAN_WG 1024          // 16 items per workgroup: neighbours in the volume, mostly of equal work, so their bin slots are taken with one atomic
__global__ __launch_bounds__(DF_PLAN_WG) void df_sweep_plan_kernel(const DfWarpedArgs a, int tiles_x, int tiles_y, unsigned n_items,
                                                                   unsigned long long* __restrict__ mask_out, unsigned int* __restrict__ cnt,
                                                                   unsigned int* __restrict__ bins, unsigned int* __restrict__ cnt_next,
                                                                   unsigned long long* __restrict__ code_out)
{
    __shared__ unsigned int s_cnt[DF_PLAN_BINS], s_base[DF_PLAN_BINS];
    if (threadIdx.x < DF_PLAN_BINS) { s_cnt[threadIdx.x] = 0u; if (blockIdx.x == 0) cnt_next[threadIdx.x] = 0u; }
    if (blockIdx.x == 0 && threadIdx.x < 2 && a.py.capped && a.cull) ((uint32_t*)a.cull)[6 + threadIdx.x] = 0u;   // (both image-maximum words: this frame's -- its readers, the verdict pass, are done -- and the other one, see the launcher)
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.host_report && a.blk_cnt) {      // (the verdict pass is complete: this kernel follows it in the stream)
        a.host_report[0] = a.blk_cnt[0]; a.host_report[1] = a.blk_cnt[1]; a.host_report[2] = a.blk_cnt[3]; a.host_report[3] = a.sweep_no;
    }
    __syncthreads();
    const unsigned item = blockIdx.x * (DF_PLAN_WG / 64) + (threadIdx.x >> 6);
    const int ln = threadIdx.x & 63, p = ln >> 4, l = ln & 15;
    unsigned long long m = 0;
    if (item < n_items) {                                                  // wave-uniform
        const unsigned half = item & 1u, tcol = item >> 1;
        const int tx = (int)(tcol % (unsigned)tiles_x), ty = (int)((tcol / (unsigned)tiles_x) % (unsigned)tiles_y);
        const int zb = (int)(tcol / ((unsigned)tiles_x * (unsigned)tiles_y));
        const int lt0 = a.bz0 + zb * a.zt;
        const int own1 = min(a.z_own0 + a.z_own_n, a.Z);
        const int x0 = tx * DF_ROW_TX + p * 8, y0 = ty * DF_LDS_TY + (int)half * 8;                  // first column of the patch
        bool keep = l < a.zt && max((lt0 + l) * DF_ROW_TZ, a.z_own0) < min((lt0 + l + 1) * DF_ROW_TZ, own1) && x0 < a.X && y0 < a.Y;
        // the verdict pass has judged the patch's 8 x 8 x 8 voxels of the layer (df_block_verdict_kernel: zero-weight, ball, blend-model box)
        unsigned verdict = 1u;
        if (keep && a.blk_alive) {
            verdict = a.blk_alive[((size_t)(lt0 + l - a.tab_z0 / DF_ROW_TZ) * a.bm_nby + (unsigned)(y0 >> 3)) * a.bm_nbx + (unsigned)(x0 >> 3)];
            keep = verdict != 0u;
        }
        m = __builtin_amdgcn_ballot_w64(keep);
        if (code_out) {                                                    // (wave-uniform) which alive cells' blocks have 4-bit neighbour codes
            const bool coded = keep && a.blk_alive && (verdict & 2u) != 0u;                          // (bit 1 of the verdict byte: see df_block_verdict_kernel)
            const unsigned long long cm = __builtin_amdgcn_ballot_w64(coded);
            if (ln == 0 && m) code_out[item] = cm;
        }
        if (a.n_swept) {                                                   // (measurement hook: what the sweep will put through the warp)
            unsigned v = keep ? (unsigned)(64 * (min((lt0 + l + 1) * DF_ROW_TZ, own1) - max((lt0 + l) * DF_ROW_TZ, a.z_own0))) : 0u;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
            if (ln == 0 && v) atomicAdd(a.n_swept, (unsigned long long)v);
        }
    }
    const unsigned w = (unsigned)__popcll(m);
    unsigned slot = 0;
    if (ln == 0 && m) slot = atomicAdd(&s_cnt[w], 1u);
    __syncthreads();
    if (threadIdx.x < DF_PLAN_BINS && s_cnt[threadIdx.x]) s_base[threadIdx.x] = atomicAdd(&cnt[threadIdx.x], s_cnt[threadIdx.x]);
    __syncthreads();
    if (ln == 0 && m) {
        mask_out[item] = m;
        bins[(size_t)w * n_items + s_base[w] + slot] = item;
    }
}

// The sweep.  One workgroup = WGT / 256 strip items of the plan; its waves are independent of each other once the plan is read.
//   LDSN = false (k = 8, every node count; k = 4 where the node table is too large for the LDS): NO node table in LDS.  A cell whose block
//     has 4-bit neighbour codes (the model pass has been over it: all but the blocks new this frame) blends out of the wave's own copies
//     of its sub-block unions -- 8 sub-blocks x 16 x {rot, node_t} = 4 KiB per wave, refilled once per (patch, layer) cell from W.rt in the
//     L2 through the union lists (bm_ids: one dword per lane, prefetched a layer ahead); the others gather their neighbours from W.rt.
//     48 KiB of LDS per 768-thread workgroup whatever M is: the occupancy (two workgroups per CU, 6 waves / SIMD at <= 80 VGPRs) and the
//     codes no longer depend on the node count.  (Rounds 1-5 kept rot / node_t of ALL nodes in LDS: 32 bytes a node, one workgroup per CU
//     from 2560 nodes on, no room for the union copies -- so no codes -- from 4864, no pipelined sweep at all from 5120.)
//   LDSN = true (k = 4, M <= 5120): rot / node_t of all nodes in LDS, gathers by ds_read_b128 (k = 4 has no codes: measured +2 %, NOTES r5).
template <int K, int U, int WGT, bool V2W_IDENTITY, bool LDSN>
// (waves per SIMD asked of the compiler: 6 for k = 8 -- 78 VGPRs, no scratch; 7 waves at 72 VGPRs spill 48 bytes a lane and lose 5 %,
// and holding a CU to 5 workgroups changes nothing: profiles/r06_ab_wgsize.txt, r06_ab_occupancy.txt -- waves buy nothing from 5 on; neither do fewer instructions or a third table
// set in flight: the launch sits 8-15 % above two floors a few per cent apart, its arithmetic alone and its memory accesses alone -- DESIGN 4.1)
__global__ __launch_bounds__(WGT, LDSN ? (WGT == 512 ? 4 : 1) : (K == 8 ? 6 : 5)) void df_warp_rows_pipe_kernel(const DfWarpedArgs a, const DfWarpView W, int tiles_x)
{
    extern __shared__ __attribute__((aligned(16))) float4 s_lds[];      // LDSN: [2M] rot_j, node_t_j interleaved; else [waves][8][16][2] union copies
    constexpr bool CODES = !LDSN && K == 8;
    static_assert(!CODES || U == 1, "a coded batch lies in one half layer");
    constexpr unsigned SPW = WGT >= 256 ? WGT / 256 : 1;                   // strip items per group of NW waves
    constexpr unsigned NW = WGT / 64;
    // ---- what a wave works on: plan entries (strip items, fullest bins first) are taken SPW at a time -- a GROUP, one per workgroup -- and a
    // group's alive cells are dealt out over the workgroup's NW waves in equal SHARES (see below).
    // (Round 6 measured the alternative -- a RESIDENT grid whose waves each take (group, share) units from an atomic cursor, no workgroup
    // launches after the first fill: 0.623 against 0.582 ms, same box, profiles/r06_ab_resident.txt.  A wave's time for a unit is set by how
    // many waves share its SIMD; workgroups put one equal share on each of a CU's four SIMDs, free-running waves do not, and the launch
    // ended on a 200 us tail of overloaded SIMDs.  What the timeline's unfilled slots were -- ~14 % -- is not the dispatcher but every
    // unit's start: five dependent trips to memory, plan to bins to masks to union lists to node records, before the first blend.)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // in an SGPR: what follows from it stays scalar
    const unsigned group = blockIdx.x, share = (unsigned)wave;
    if ((unsigned)(size_t)(df_lds_cf4*)s_lds != 0u) __builtin_trap();    // the blend addresses the LDS from address 0
    if constexpr (LDSN) {
        for (int j = threadIdx.x; j < W.M; j += WGT) { s_lds[2 * j] = W.rot[j]; s_lds[2 * j + 1] = W.node_t[j]; }
        __syncthreads();
    }
    const df_global_ptr<const char> rt_g = (df_global_ptr<const char>)df_wave_uniform(reinterpret_cast<const char*>(W.rt));
    const size_t plane = (size_t)a.X * a.Y;
    const int own1 = min(a.z_own0 + a.z_own_n, a.Z);
    const unsigned pitch24 = (unsigned)a.P.pitch;                          // rows, pitch < 2^24 (checked by the launcher): 24-bit multiply
    unsigned int wave_upd = 0;                                             // (a wave-level count: ballots, no lane register)
    // entry e of the plan = the e-th item counting the bins from the fullest down: lane j holds the count of bin 64 - j and the
    // running total up to and including it
    const unsigned bin_cnt = a.plan_cnt[DF_PLAN_BINS - 1 - df_lane_id_here()];
    unsigned bin_end = bin_cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(bin_end, o, 64); if ((int)df_lane_id() >= o) bin_end += t; }
    const unsigned n_alive = (unsigned)__builtin_amdgcn_readlane((int)bin_end, 63);
    if (group * SPW >= n_alive) return;                                    // past the end of the plan (the grid is sized for every strip; no barrier follows)
#ifdef DF_TRACE_WG
    const unsigned long long t_start = wall_clock64();
    unsigned n_layers = 0;
#endif
    // ---- the workgroup's work, dealt out evenly (round 4).  A workgroup takes SPW strip items = 4 SPW patches x <= 16 layers of alive
    // (patch, layer) cells.  With one patch per wave the workgroup lasted as long as its fullest patch while the other waves' slots sat
    // idle: a per-wave timeline showed the waves busy for 83 % of the time their workgroups held the slots.  Now the alive cells of all
    // the workgroup's patches form ONE sequence (item, patch, layer, half-layer of 4 planes) and wave w takes the w-th of WGT / 64
    // equal shares of it: a run of layers of one patch, or the tail of one patch and the head of the next -- SEGMENTS, each walked by
    // the pipelined loop below as before.  Which voxel is updated by which wave changes; what is computed for it does not.
    unsigned items_s[SPW]; unsigned long long masks_s[SPW];
    unsigned long long cmask_s[SPW];
    unsigned total2 = 0;
#pragma unroll
    for (unsigned s_ = 0; s_ < SPW; ++s_) {
        const unsigned sidx = group * SPW + s_;
        items_s[s_] = 0u; masks_s[s_] = 0ull;
        cmask_s[s_] = 0ull;
        if (sidx < n_alive) {
            const int j = __ffsll((unsigned long long)__builtin_amdgcn_ballot_w64(sidx < bin_end)) - 1;      // its bin: the first running total above sidx
            const unsigned r = sidx - ((unsigned)__builtin_amdgcn_readlane((int)bin_end, j) - (unsigned)__builtin_amdgcn_readlane((int)bin_cnt, j));
            items_s[s_] = (unsigned)__builtin_amdgcn_readfirstlane((int)a.plan_bins[(size_t)(DF_PLAN_BINS - 1 - j) * a.plan_items + r]);
            const unsigned long long m = a.plan_mask[items_s[s_]];
            masks_s[s_] = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(m >> 32)) << 32) |
                          (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)m);
            total2 += 2u * (unsigned)__popcll(masks_s[s_]);
            if (CODES && a.plan_code) {
                const unsigned long long cm = a.plan_code[items_s[s_]];
                cmask_s[s_] = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(cm >> 32)) << 32) |
                              (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)cm);
            }
        }
    }
    const unsigned c0 = total2 * share / NW, c1 = total2 * (share + 1u) / NW;      // this unit's half-layer cells [c0, c1)
    unsigned pre = 0;
#pragma unroll 1
    for (unsigned q = 0; q < SPW * 4u; ++q) {
    unsigned item = items_s[0]; unsigned long long m_item = masks_s[0];
#pragma unroll
    for (unsigned s_ = 1; s_ < SPW; ++s_) if ((q >> 2) == s_) { item = items_s[s_]; m_item = masks_s[s_]; }
    const unsigned a16 = (unsigned)(m_item >> (16u * (q & 3u))) & 0xffffu;
    unsigned long long c_item = cmask_s[0];
#pragma unroll
    for (unsigned s_ = 1; s_ < SPW; ++s_) if ((q >> 2) == s_) c_item = cmask_s[s_];
    const unsigned cbits = CODES ? (unsigned)(c_item >> (16u * (q & 3u))) & 0xffffu : 0u;      // layers of this patch whose block has 4-bit codes
    const unsigned n2 = 2u * (unsigned)__popc(a16);
    const unsigned seg_lo = max(c0, pre), seg_hi = min(c1, pre + n2);
    const unsigned pre0 = pre;
    pre += n2;
    if (seg_lo >= seg_hi) continue;                                        // none of this patch's cells are this wave's
    const unsigned lo = seg_lo - pre0, hi = seg_hi - pre0;                 // half-layer cells [lo, hi) of the patch's 2 popc(a16)
    unsigned alive = a16;
    for (unsigned i = 0; i < (lo >> 1); ++i) alive &= alive - 1u;          // drop the layers before the segment ...
    {
        unsigned keep = ((hi - 1u) >> 1) - (lo >> 1) + 1u, rest = alive, seg = 0u;
        for (unsigned i = 0; i < keep; ++i) { const unsigned low = rest & (0u - rest); seg |= low; rest ^= low; }
        alive = seg;                                                       // ... and those after it
    }
    int first_l = __ffs(alive) - 1, last_l = 31 - __clz(alive);
    int z_first_off = (int)(lo & 1u) * (DF_ROW_TZ / 2), z_last_off = ((int)((hi - 1u) & 1u) + 1) * (DF_ROW_TZ / 2);
    const int wave_patch = (int)(q & 3u);
    // item -> tile column, half, layer block; the wave's 8 x 8 patch is number wv of the 32 x 16 footprint (4 across, 2 down): a compact
    // footprint, so that the voxels of a wave fall on the same side of the frustum and of the observed surface more often
    const unsigned tcol = item >> 1;
    const int tx = (int)(tcol % (unsigned)tiles_x), ty = (int)((tcol / (unsigned)tiles_x) % (unsigned)a.plan_tiles_y);
    const int wv = (int)(item & 1u) * 4 + wave_patch;
    const int lnq = (int)df_lane_id_here();                               // (per segment: nothing of the lane's number is kept across segments)
    const int x = tx * DF_ROW_TX + (wv & 3) * 8 + (lnq & 7);
    const int y = ty * DF_LDS_TY + (wv >> 2) * 8 + (lnq >> 3);
    const bool in_xy = x < a.X && y < a.Y;
    const int xc = min(x, a.X - 1), yc = min(y, a.Y - 1);                 // clamped: out-of-volume lanes read valid entries, write nothing
    const float fxv = (float)x * a.vsx, fyv = (float)y * a.vsy;
    const int lt0 = a.bz0 + (int)(tcol / ((unsigned)tiles_x * (unsigned)a.plan_tiles_y)) * a.zt;     // first tile layer of the item
    // the segment's first / last layer start / end at a half-layer boundary; a layer the slab's own range cuts down to nothing is dropped
    auto layer_zb = [&](int l) { const int z = max((lt0 + l) * DF_ROW_TZ, a.z_own0); return l == first_l ? max(z, (lt0 + l) * DF_ROW_TZ + z_first_off) : z; };
    auto layer_ze = [&](int l) { const int z = min((lt0 + l + 1) * DF_ROW_TZ, own1); return l == last_l ? min(z, (lt0 + l) * DF_ROW_TZ + z_last_off) : z; };
    if (alive && layer_zb(first_l) >= layer_ze(first_l)) { alive &= alive - 1u; first_l = alive ? __ffs(alive) - 1 : 0; z_first_off = 0; }   // (the next layer, if any, is taken whole)
    if (alive && layer_zb(last_l) >= layer_ze(last_l)) { alive &= ~(1u << last_l); last_l = alive ? 31 - __clz(alive) : 0; z_last_off = DF_ROW_TZ; }
    if (alive) {
        // batch sequence: U planes per batch inside a layer, then the first batch of the next alive layer; l < 0 = none
        auto advance = [&](int l, int z0, int* nl, int* nz0) {
            *nl = l; *nz0 = z0 + U;
            if (*nz0 >= layer_ze(l)) {
                const unsigned rem = alive >> (l + 1);
                *nl = rem ? l + 1 + (__ffs(rem) - 1) : -1;
                *nz0 = *nl >= 0 ? layer_zb(*nl) : 0;
            }
        };
        // prefetch distance is TWO batches (two packed register sets, used alternately): the tables of batch b+2 are
        // requested in the middle of batch b and consumed at the start of batch b+2, a whole blend later.
        // table address = (workgroup-uniform record index: tile column + tile layer + plane in tile) + (loop-invariant 32-bit lane
        // offset inside the tile plane): the uniform part stays in SGPRs and the loads take the saddr + voffset form instead of
        // a 64-bit VALU address per load
        // (the lane's BYTE offset in a volume plane, 32 bits.  The voxel word is read and written through a BUFFER descriptor of its plane
        // -- four scalar registers made from the plane's address -- with this offset in one VGPR: the global_load / _store forms of the same
        // access took a 64-bit VALU address per access and a register pair for the zero-extended offset, because the extension is hoisted
        // out of the loop and instruction selection then no longer sees scalar base + 32-bit offset.)
        const unsigned lane_vox4 = (unsigned)(yc * a.X + xc) * 4u;
        const unsigned plane_bytes = (unsigned)plane * 4u;                // (< 2^32: dims[0] * dims[1] < 2^30, checked by the launcher)
        const unsigned lane_tab = df_tab_in_plane(xc, yc);
        const size_t tile_col = (size_t)(yc / DF_TAB_TY) * a.tab_ntx + (size_t)(xc / DF_TAB_TX);      // == (ty, tx) of the workgroup: uniform
        const size_t tile_col_u = (size_t)__builtin_amdgcn_readfirstlane((int)tile_col);
        // (round 5) the record index of plane z of tile layer lt0 + l is rec0 + l * rec_layer + (z mod 8) * 512: a tile layer of the sweep IS
        // a tile layer of the tables (DF_ROW_TZ = DF_TAB_TZ, tab_z0 a multiple of 8), so the division, the remainder and the 64-bit
        // products of the general form (39 scalar instructions per load, a fifth of the kernel's SALU work) are made once per segment
        static_assert(DF_ROW_TZ == DF_TAB_TZ, "the sweep's layers are the tables' tile layers");
        const size_t rec_layer = (size_t)a.tab_nty * (size_t)a.tab_ntx * (DF_TAB_TX * DF_TAB_TY * DF_TAB_TZ);
        const size_t rec0 = ((size_t)(lt0 - a.tab_z0 / DF_TAB_TZ) * a.tab_nty * a.tab_ntx + tile_col_u) * (DF_TAB_TX * DF_TAB_TY * DF_TAB_TZ);
        // (the code plane is patch-major: the wave's 64 codes are entries [64 * patch, + 64) of the tile plane, lane ln's at + ln -- formed
        // from the lane id where it is used instead of living in a register across the loop; a lane past the volume's edge reads the
        // padding's code, some 4-bit positions in the copies the wave holds, and stores nothing)
        const unsigned code_patch = ((unsigned)wv << 6);
        // ---- the wave's copies of the sub-block unions of the cell it is in (CODES): LDS bytes [wave * 4096, + 4096) = [h][q][16] x {rot,
        // node_t}; a lane's voxel of plane z reads the copy of (h = z >> 2 & 1, q = its column quadrant).  The union lists of the segment's
        // coded layers are fetched one layer ahead (ids_nxt: the dword of lane = q * 16 + e holds entry e of quadrant q, low half word
        // h = 0, high half word h = 1), the 2 x 64 records they name gathered from W.rt at the cell's first batch.
        const unsigned lds_wave = (unsigned)wave * 4096u;
        const unsigned lq_base = lds_wave + ((((unsigned)xc >> 2) & 1u) | ((((unsigned)yc >> 2) & 1u) << 1)) * 512u;
        int loc_layer = -1;                                            // the layer whose unions the copies hold
        unsigned ids_nxt = 0u;
        const unsigned coded_alive = CODES ? (alive & cbits) : 0u;
        // (the block of the wave's patch in layer l, from scalars: tile column, patch number)
        const unsigned blk_x = (unsigned)tx * (DF_ROW_TX / 8) + ((unsigned)wv & 3u), blk_y = (unsigned)ty * (DF_LDS_TY / 8) + ((unsigned)wv >> 2);
        auto lane_id = [&]() -> unsigned { return df_lane_id(); };       // (recomputed where used: no register held across the loop)
        auto ids_load = [&](int l) -> unsigned {
            const size_t blk = ((size_t)(unsigned)(lt0 + l - a.tab_z0 / DF_ROW_TZ) * (unsigned)a.bm_nby + blk_y) * (unsigned)a.bm_nbx + blk_x;
            return *((df_global_ptr<const uint32_t>)(a.bm_ids + blk * 64) + lane_id());
        };
        auto refill = [&](int l) {
            const unsigned ids = ids_nxt;                                  // (of layer l: refills come in the order of the coded layers)
            const df_global_ptr<const df_v4f> n0 = (df_global_ptr<const df_v4f>)(rt_g + df_node_off_lo(ids));
            const df_global_ptr<const df_v4f> n1 = (df_global_ptr<const df_v4f>)(rt_g + df_node_off_hi(ids));
            const df_v4f r0 = n0[0], t0 = n0[1], r1 = n1[0], t1 = n1[1];
            __builtin_amdgcn_sched_barrier(0);
            const unsigned rem = coded_alive >> (l + 1);                   // the next coded layer's list: in flight until its refill
            ids_nxt = ids_load(rem ? l + 1 + (__ffs(rem) - 1) : l);
            __builtin_amdgcn_sched_barrier(0);
            df_v4f* loc = (df_v4f*)((char*)s_lds + lds_wave + lane_id() * 32u);
            loc[0] = r0; loc[1] = t0; loc[128] = r1; loc[129] = t1;        // (h = 1: 2048 bytes on)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // (the wave's own LDS writes, before its blends read them)
        };
        if (coded_alive) ids_nxt = ids_load(__ffs(coded_alive) - 1);
        auto load_batch = [&](DfTabRaw<K> (&S)[U], int l, int z0) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int zi = min(z0 + u, layer_ze(l) - 1) - (lt0 + l) * DF_ROW_TZ;         // plane inside the layer
                const size_t rec = rec0 + (size_t)(unsigned)l * rec_layer + (size_t)(unsigned)(zi * (DF_TAB_TX * DF_TAB_TY));
                const bool coded_l = CODES && ((cbits >> l) & 1u) != 0u;
                tab_raw_load_at(a, rec, rec + code_patch, coded_l, lane_tab, lane_id(), S[u]);
            }
        };
        int l = __ffs(alive) - 1, z0 = layer_zb(l);
        int l1, z1; advance(l, z0, &l1, &z1);
        DfTabRaw<K> S0[U], S1[U];
        load_batch(S0, l, z0);
        load_batch(S1, l1 >= 0 ? l1 : l, l1 >= 0 ? z1 : z0);               // dummy re-read when there is no second batch

        // The end of a batch's sample (:85-93: compare with the dists value, fuse, store) is carried into the NEXT batch: the dists
        // gather is the last thing a voxel's chain issues, so finishing the batch at once waits for it with nothing left to do in the
        // wave; a batch later it has long arrived.  `pend` is what the finish needs (6 VGPRs); an empty one (ok = false) stores nothing.
        // (round 6) The finish is the rigid sweep's two-stage sample (dfusion_device.h, tsdf_sample_pre / _finish -- proven and selftested
        // there): with s = v_sqrt_f32(|vc|^2), one ulp, and sdf_a = Dp - s, a voxel with sdf_a >= T = df_sat_threshold(trunc) has tsdf = 1.f
        // EXACTLY, one with sdf_a <= -T does not update, whatever the last bits of |vc| are (|vc| < 64 m, 2^-10 <= trunc <= 2^10).  Most
        // batches lie in observed free space or behind the surface: when every voxel the wave is about to decide is decided that way, the
        // exact square root (9 instructions) is never made, and where the stored values are 1.0 or still cleared the fuse is a weight
        // increment (tsdf_fuse_one: (w + 1) / (w + 1) = 1 without the division).  A wave with a voxel within T of the surface takes :89-93
        // as written.  `pend` is what either form needs.
        // (a voxel that does not project into the image waits with dists bits 0: `no measurement`, :86 -- one flag less to carry)
        struct { float d2[U]; uint16_t dpb[U]; uint32_t vox[U]; int z[U]; } pend;
#pragma unroll
        for (int u = 0; u < U; ++u) { pend.d2[u] = 1.f; pend.dpb[u] = 0; pend.vox[u] = 0u; pend.z[u] = a.z_store0; }
        const float sat_t = df_sat_threshold(a.P.trunc);
        auto finish_pending = [&]() {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float Dp = h2f_bits(pend.dpb[u]);
                const float d2 = pend.d2[u];
                const float sdf_a = Dp - __builtin_amdgcn_sqrtf(d2);
                // Wave-wide decisions as algebra on the compares' lane masks (a ballot of a compound bool costs two more VALU instructions)
                const unsigned long long live_m = __builtin_amdgcn_ballot_w64(Dp != 0.f);                  // :82, :86
                // decided: far enough from the surface on either side, inside the domain of the error bound (|vc| <= 32 m; a NaN fails)
                const unsigned long long decided_m = __builtin_amdgcn_ballot_w64(fabsf(sdf_a) >= sat_t) & __builtin_amdgcn_ballot_w64(d2 <= 1024.f);
                bool upd; uint32_t out;
                if (a.sat_ok && (live_m & ~decided_m) == 0ull) {
                    const unsigned long long upd_m = live_m & __builtin_amdgcn_ballot_w64(sdf_a >= sat_t);
                    upd = (Dp != 0.f) & (sdf_a >= sat_t);
                    const unsigned long long one_m = __builtin_amdgcn_ballot_w64(pend.vox[u] == 0u) | __builtin_amdgcn_ballot_w64((pend.vox[u] & 0xffffu) == 0x3c00u);   // tsdf_fuse_one_ok
                    if ((upd_m & ~one_m) == 0ull) out = tsdf_fuse_one(pend.vox[u], a.P.max_weight);
                    else out = tsdf_fuse(pend.vox[u], 1.f, a.P.max_weight);                   // :93 with tsdf = fminf(1.f, .) = 1.f
                    wave_upd += (unsigned)__popcll(upd_m);
                } else {
                    float vn;
                    if (__builtin_expect(df_wave_all(df_sqrt_short_ok(d2)), 1)) vn = df_sqrt_short(d2);
                    else vn = sqrtf(d2);                                                      // (NaN positions of zero-weight voxels come here)
                    const float sdf = Dp - vn;                                                // :89
                    upd = (Dp != 0.f) & (sdf >= -a.P.trunc);                                  // :91
                    out = tsdf_fuse(pend.vox[u], fminf(1.f, sdf * a.P.trunc_inv), a.P.max_weight);   // :93
                    wave_upd += (unsigned)__popcll(live_m & __builtin_amdgcn_ballot_w64(sdf >= -a.P.trunc));
                }
                if (upd) __builtin_amdgcn_raw_buffer_store_b32(out, df_plane_rsrc(a.vol + (size_t)(pend.z[u] - a.z_store0) * plane, plane_bytes), lane_vox4, 0, 0);
            }
        };
        // one batch: consumes S (tables of batch (l, z0)), then refills S with the tables of batch (l2, z2)
        auto step = [&](DfTabRaw<K> (&S)[U], int l, int z0, int l2, int z2) {
            const int ze = layer_ze(l);
            // (1) planes of this batch (clamped for the tail)
            bool inz[U]; int zv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                inz[u] = in_xy && z0 + u < ze;
                zv[u] = min(z0 + u, ze - 1);
            }
            // (2) blend -> transform -> project, then the dists gathers (clamped address, always valid).  The normalisations and the
            // square root take their short forms (dfusion_device.h: same bits on a restricted domain) when the whole wave is inside
            // the domain.
            f3 vc[U]; bool ok[U]; uint16_t dpb[U];
            const bool coded = CODES && ((cbits >> l) & 1u) != 0u;        // wave-uniform
            if (CODES && coded && l != loc_layer) { refill(l); loc_layer = l; }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                // canonical position.  With an axis-aligned volume (R = I exactly -- the reference's default pose is a pure
                // translation) the nested FMAs of R * p return p itself: fma(1, x, fma(0, y, 0 * z)) = x for the finite, non-negative grid
                // coordinates, so only the translation is left to add.
                const f3 pv3 = mk3(fxv, fyv, (float)(z0 + u) * a.vsz);
                f3 q;
                if constexpr (V2W_IDENTITY) q = add3(pv3, mk3(a.vol2world.t[0], a.vol2world.t[1], a.vol2world.t[2]));
                else q = aff_mul(a.vol2world, pv3);
                DfBlendSums B;
                if constexpr (LDSN) B = dqb_sums_lds_rec(S[u]);
                else if constexpr (CODES) {
                    if (coded) B = dqb_sums_codes(S[u], lq_base | (((unsigned)(z0 + u) & 4u) << 9));        // (h = plane 4-7 of the layer: + 2048)
                    else B = dqb_sums_global_rec(S[u], rt_g);
                } else B = dqb_sums_global_rec(S[u], rt_g);
                quat rsum, rn; quat2 half;
                rsum.w = B.r01.x; rsum.x = B.r01.y; rsum.y = B.r23.x; rsum.z = B.r23.y;
                half.wx = B.t01 * 0.5f; half.yz = B.t23 * 0.5f;
                const float s1 = q_sumsq(rsum);
                float n1;
                if (__builtin_expect(df_wave_all(df_sqrt_short_ok(s1)), 1)) n1 = df_sqrt_short(s1);
                else n1 = sqrtf(s1);                             // far from the nodes: tiny, denormal or zero sums
                const quat rot = q_scale_f64(df_rcp_short((double)n1), rsum);                 // :214 (see q_normalize_rcp_short)
                const quat2 dual = q_mul_pk(half, q_pairs(rot));                              // dual_quaternion.hpp:59-63
                const float s2 = q_sumsq(rot);
                if (__builtin_expect(df_wave_all(q_near_unit_ok(s2)), 1)) rn = q_normalize_near_unit(rot, s2);
                else rn = q_normalize(rot);                      // blend sums so small that their squares were denormal: rot is not unit
                vc[u] = aff_mul(a.world2cam, dq_transform_rn_pk(rn, dual, q));
                const float pu = fmaf(a.P.fx, vc[u].x / vc[u].z, a.P.cx);                     // device.hpp:35
                const float pv = fmaf(a.P.fy, vc[u].y / vc[u].z, a.P.cy);                     // device.hpp:36
                ok[u] = inz[u] & (vc[u].z > 0.f) & (pu >= 0.f) & (pv >= 0.f) & (pu < (float)a.P.cols) & (pv < (float)a.P.rows);   // :82,:86
                // clamped pixel (one v_med3_f32 each; a NaN coordinate gives some in-range pixel, and such a voxel is not `ok` anyway)
                const int ui = (int)__builtin_amdgcn_fmed3f(pu, 0.f, (float)(a.P.cols - 1));
                const int vi = (int)__builtin_amdgcn_fmed3f(pv, 0.f, (float)(a.P.rows - 1));
                dpb[u] = *(const uint16_t*)((const char*)a.P.dists + (__umul24((unsigned)vi, pitch24) + 2u * (unsigned)ui));   // :85
            }
            // (2b) the previous batch's compare / fuse / store: its gathers were issued a whole batch ago
            finish_pending();
            __builtin_amdgcn_sched_barrier(0);
            // (3) tables of batch b+2 into the set just consumed.  Unconditional (a dummy re-read at the end): a branch here
            // would make the compiler assume the loads may not have been issued and wait for most of the prefetch.
            load_batch(S, l2 >= 0 ? l2 : l, l2 >= 0 ? z2 : z0);
            __builtin_amdgcn_sched_barrier(0);
            // (4) |vc|^2 of this batch (:89); the rest of the sample waits in `pend`
#pragma unroll
            for (int u = 0; u < U; ++u) {
                // the voxel word is only needed if the voxel projects into the image (the finish is a batch away: time enough), and
                // whole 32-byte runs of lanes that do not are not fetched at all
                uint32_t vw = 0u;
                if (ok[u]) vw = __builtin_amdgcn_raw_buffer_load_b32(df_plane_rsrc(a.vol + (size_t)(zv[u] - a.z_store0) * plane, plane_bytes), lane_vox4, 0, 0);
                pend.d2[u] = dot3(vc[u], vc[u]); pend.dpb[u] = ok[u] ? dpb[u] : (uint16_t)0; pend.vox[u] = vw; pend.z[u] = zv[u];
            }
        };
        for (;;) {
            int l2, z2;
            if (l1 >= 0) advance(l1, z1, &l2, &z2); else { l2 = -1; z2 = 0; }
            step(S0, l, z0, l2, z2);
            if (l1 < 0) break;
            int l3, z3;
            if (l2 >= 0) advance(l2, z2, &l3, &z3); else { l3 = -1; z3 = 0; }
            step(S1, l1, z1, l3, z3);
            if (l2 < 0) break;
            l = l2; z0 = z2; l1 = l3; z1 = z3;
        }
        finish_pending();                                                   // the last batch
    }
#ifdef DF_TRACE_WG
    n_layers += __popc(alive);
#endif
    }                                                                       // (the next segment of this unit)
#ifdef DF_TRACE_WG
    {
        unsigned hw; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        unsigned xcc; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        if (df_lane_id_here() == 0u) {
            unsigned long long* t = a.trace + ((size_t)group * NW + share) * 4;
            t[0] = t_start; t[1] = wall_clock64(); t[2] = ((unsigned long long)xcc << 32) | hw; t[3] = (unsigned long long)n_layers;
        }
    }
#endif
    if (a.n_upd && df_lane_id_here() == 0u && wave_upd) atomicAdd(a.n_upd, (unsigned long long)wave_upd);
}

// max dists value over the image (for the cull's depth test); `out` zeroed on the stream first.
__global__ __launch_bounds__(256) void df_dists_max_kernel(const uint16_t* __restrict__ dists, size_t pitch, int cols, int rows,
                                                           float* __restrict__ out)
{
    float m = 0.f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < cols * rows; i += gridDim.x * 256) {
        const int y = i / cols, x = i - y * cols;
        const float d = h2f_bits(*(const uint16_t*)((const char*)dists + (size_t)y * pitch + 2 * (size_t)x));
        if (!(d <= 3.0e38f)) m = 3.0e38f;              // inf / NaN distances: make the depth test vacuous
        else m = fmaxf(m, d);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) atomicMax((unsigned int*)out, __float_as_uint(m));
}

// half diagonal (world metres) of the voxel-centre lattice of an nx x ny x nz tile under vol2world
static double df_tile_radius(const float vol2world[12], double nx, double ny, double nz, const DfVolume& v)
{
    double r = 0.0;
    for (int sx = -1; sx <= 1; sx += 2) for (int sy = -1; sy <= 1; sy += 2) for (int sz = -1; sz <= 1; sz += 2) {
        double ex = sx * 0.5 * (nx - 1) * v.voxel_size[0], ey = sy * 0.5 * (ny - 1) * v.voxel_size[1], ez = sz * 0.5 * (nz - 1) * v.voxel_size[2];
        double wx = vol2world[0] * ex + vol2world[1] * ey + vol2world[2] * ez;
        double wy = vol2world[3] * ex + vol2world[4] * ey + vol2world[5] * ez;
        double wz = vol2world[6] * ex + vol2world[7] * ey + vol2world[8] * ez;
        double d = sqrt(wx * wx + wy * wy + wz * wz);
        if (d > r) r = d;
    }
    return r;
}

// measurement hook of the warped sweep, per handle (the handle is single-stream: no race with its own launches)
extern "C" int dfusion_warp_debug_counters(DfWarpField* wf, unsigned long long* swept_dev)
{
    if (!wf) return DF_E_INVALID;
    wf->dbg_swept = swept_dev;
    return DF_OK;
}

// alive 8 x 8 x 8 blocks per 8-plane layer, from the verdict bytes of the last sweep: one workgroup per layer of the table
__global__ __launch_bounds__(256) void df_alive_per_layer_kernel(const uint8_t* __restrict__ alive, unsigned mask, unsigned per_layer, int layer0, int l_lo,
                                                                 int l_hi, unsigned long long* __restrict__ out)
{
    __shared__ unsigned s[4];
    const int layer = layer0 + (int)blockIdx.x;
    if (layer < l_lo || layer >= l_hi) return;
    const uint8_t* a = alive + (size_t)blockIdx.x * per_layer;
    unsigned n = 0;
    for (unsigned i = threadIdx.x; i < per_layer; i += 256) n += (a[i] & mask) ? 1u : 0u;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&out[layer], (unsigned long long)(s[0] + s[1] + s[2] + s[3]));
}
static int df_count_verdicts(DfWarpField* wf, unsigned mask, int z0, int zn, unsigned long long* per_layer_dev, int n_layers, dfStream stream)
{
    if (!wf || !per_layer_dev || n_layers <= 0 || z0 < 0 || zn < 0) return DF_E_INVALID;
    if (!wf->tab_valid || !wf->alive_valid || !wf->blk_alive) return DF_E_NO_INDEX;
    const int ntx = (wf->geom_dims[0] + DF_TAB_TX - 1) / DF_TAB_TX, nty = (wf->geom_dims[1] + DF_TAB_TY - 1) / DF_TAB_TY;
    const unsigned per_layer = (unsigned)(ntx * (DF_TAB_TX / 8)) * (unsigned)(nty * (DF_TAB_TY / 8));
    const int nbz = wf->tab_zn / 8, layer0 = wf->tab_z0 / 8;
    const int l_lo = (z0 + 7) / 8, l_hi = min((z0 + zn) / 8, n_layers);                 // layers entirely inside [z0, z0 + zn)
    if (nbz <= 0 || l_hi <= l_lo) return DF_OK;
    hipLaunchKernelGGL(df_alive_per_layer_kernel, dim3((unsigned)nbz), dim3(256), 0, (hipStream_t)stream, wf->blk_alive, mask, per_layer, layer0, l_lo,
                       l_hi, per_layer_dev);
    DF_LAUNCH_CHECK();
    return DF_OK;
}
extern "C" int dfusion_warp_alive_blocks(DfWarpField* wf, int z0, int zn, unsigned long long* per_layer_dev, int n_layers, dfStream stream)
{
    return df_count_verdicts(wf, 0xffu, z0, zn, per_layer_dev, n_layers, stream);
}
// The kept blocks among them that the sweep served from 4-bit neighbour codes (verdict bit 1, dfusion_warp_blocks.h).
extern "C" int dfusion_warp_coded_blocks(DfWarpField* wf, int z0, int zn, unsigned long long* per_layer_dev, int n_layers, dfStream stream)
{
    return df_count_verdicts(wf, 2u, z0, zn, per_layer_dev, n_layers, stream);
}

// The arguments of a table build over the current tables (geometry as dfusion_warp_build_index recorded it).
static DfWarpedArgs df_table_args(const DfWarpField* wf)
{
    DfWarpedArgs a;
    memset(&a, 0, sizeof(a));
    const int ntx = (wf->geom_dims[0] + DF_TAB_TX - 1) / DF_TAB_TX, nty = (wf->geom_dims[1] + DF_TAB_TY - 1) / DF_TAB_TY;
    a.w_tab = wf->w_tab_valid ? wf->w_tab : nullptr;
    a.tile_wmax = wf->w_tab_valid ? wf->tile_wmax : nullptr;
    a.blk_wmax = wf->w_tab_valid ? wf->blk_wmax : nullptr;
    a.X = wf->geom_dims[0]; a.Y = wf->geom_dims[1]; a.Z = wf->geom_dims[2];
    a.z_store0 = wf->tab_z0; a.z_own0 = wf->tab_z0; a.z_own_n = wf->tab_zn;        // every voxel of the covered bricks gets an entry
    a.vsx = wf->geom_vs[0]; a.vsy = wf->geom_vs[1]; a.vsz = wf->geom_vs[2];
    a.vol2world = df_aff(wf->geom_aff);
    a.knn_tab = wf->knn_tab; a.tab_z0 = wf->tab_z0; a.tab_ntx = ntx; a.tab_nty = nty;
    a.tab_nvox = (size_t)ntx * DF_TAB_TX * nty * DF_TAB_TY * wf->tab_zn;
    a.bz0 = wf->tab_z0 / DF_BRICK;
    a.bm_nbx = ntx * (DF_TAB_TX / 8); a.bm_nby = nty * (DF_TAB_TY / 8);
    a.code_tab = wf->code_tab; a.bm_ids = wf->bm_ids; a.bm_coded = wf->bm_coded;
    a.blk_tie = wf->blk_tie;
    return a;
}
// LDS a workgroup may ask for on this device (160 KiB on gfx950), what the node-table kernels' "fits" is decided against (the
// dynamic-LDS attribute used to be a fixed 160 KiB, which fails on a part with less whatever the launch needs)
static size_t df_lds_limit()
{
    static std::atomic<size_t> cached{0};
    size_t v = cached.load();
    if (v) return v;
    int dev = 0, bytes = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&bytes, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || bytes < 64 * 1024) {
        (void)hipGetLastError();
        bytes = 64 * 1024;
    }
    v = (size_t)bytes < (size_t)160 * 1024 ? (size_t)bytes : (size_t)160 * 1024;
    cached.store(v);
    return v;
}

// Workgroups of a list-driven pass: as many as are resident at once (workgroup i takes entries i, i + grid, ...: a second round of
// workgroups would start when the first has finished its whole share).  An empty list costs their launch.
static unsigned df_work_grid(const void* kernel)
{
    int per_cu = 0, dev = 0; hipDeviceProp_t prop;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0) != hipSuccess || per_cu < 1) per_cu = 2;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess || prop.multiProcessorCount < 1) return 512u;
    return (unsigned)per_cu * (unsigned)prop.multiProcessorCount;
}

// the build of the bricks on a work list: list 0 (urgent; length cnt[0], cursor cnt[2]) or list 1 (look-ahead; cnt[3], cnt[4])
static int df_build_listed(DfWarpField* wf, const uint32_t* cnt, hipStream_t st, int list = 0)
{
    DfWarpedArgs b = df_table_args(wf);
    b.work = wf->blk_work + (size_t)list * wf->blk_cap; b.work_cnt = cnt + (list ? 3 : 0); b.work_cursor = const_cast<uint32_t*>(cnt) + (list ? 4 : 2);
    b.work_cap = list ? DF_WARP_PREFETCH_CAP : 0u;
    const DfWarpView W = df_view(wf);
    static unsigned grid[9] = {0};
    DF_DISPATCH_K(wf->tab_k, {
        if (!grid[K]) grid[K] = df_work_grid((const void*)df_warp_brick_kernel<K, true>);
        df_warp_brick_kernel<K, true><<<dim3(grid[K]), dim3(256), 0, st>>>(b, W);
    });
    DF_LAUNCH_CHECK();
    return DF_OK;
}

// On-demand tables (DF_INDEX_TABLES_ON_DEMAND) hold only the blocks some sweep's verdict pass has asked for.  A sweep that takes
// no verdicts (cull switched off, or a kernel other than the pipelined one) needs them all: build what is missing.
static int df_tables_complete(DfWarpField* wf, hipStream_t st)
{
    if (wf->tab_complete) return DF_OK;
    const DfWarpedArgs b = df_table_args(wf);
    const int nbz = wf->tab_zn / 8;
    const size_t nblk = (size_t)b.bm_nbx * b.bm_nby * nbz;
    uint32_t* cnt = wf->blk_cnt + 8 * wf->blk_phase;
    uint32_t* cnt_next = wf->blk_cnt + 8 * (wf->blk_phase ^ 1);
    hipLaunchKernelGGL(df_blocks_unbuilt_kernel, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, st, b.bm_nbx, b.bm_nby, nbz, wf->bx, wf->by,
                       wf->tab_z0 / 8, wf->blk_state, wf->blk_work, cnt, cnt_next);
    DF_LAUNCH_CHECK();
    wf->blk_phase ^= 1;
    int rc = df_build_listed(wf, cnt, st);
    if (rc) return rc;
    wf->tab_complete = true;
    return DF_OK;
}

// The verdict pass of the pipelined sweep (dfusion_warp_blocks.h) and the on-demand work it finds: table builds for alive blocks that
// have none yet, blend models for alive blocks that have tables but no model (from the second sweep over the tables on, so that a node
// set that changes every frame never pays for models; `now` = from the first).
static int df_block_verdicts(DfWarpField* wf, DfWarpedArgs& a, int k, unsigned flags, hipStream_t st)
{
    const int nbx = a.tab_ntx * (DF_TAB_TX / 8), nby = a.tab_nty * (DF_TAB_TY / 8), nbz = wf->tab_zn / 8;
    const size_t nblk = (size_t)nbx * nby * nbz;
    if (nblk == 0 || nblk > wf->blk_cap) return DF_E_INVALID;
    const bool use_models = !(flags & DF_WARP_NO_BLOCK_MODEL) && (k == 8 || k == 4);
    const int want_models = !use_models ? 0 : (flags & DF_WARP_BLOCK_MODEL_NOW) ? 2 : wf->tab_sweeps >= 1 ? 1 : 0;
    if (want_models && nblk > wf->bm_cap) {
        wf->bm_cap = 0;
        { int rc = wf->bm_idx.reserve(nblk * DF_BM_NU); if (rc) return rc; }
        { int rc = wf->bm_lam.reserve(nblk * DF_BM_NU); if (rc) return rc; }
        { int rc = wf->bm_w.reserve(nblk * DF_BM_NU); if (rc) return rc; }
        { int rc = wf->bm_cnt.reserve(nblk); if (rc) return rc; }
        wf->bm_cap = nblk;
    }
    // 4-bit neighbour codes + the sub-blocks' union lists (the sweep reads them at k = 8 only: no 4 bytes a voxel for the others)
    if (want_models && k == 8 && (nblk * 512 > wf->code_cap || !wf->bm_ids || !wf->code_tab || !wf->bm_coded)) {
        wf->code_cap = 0;
        { int rc = wf->bm_ids.reserve(nblk * 64); if (rc) return rc; }
        { int rc = wf->code_tab.reserve(nblk * 512); if (rc) return rc; }
        { int rc = wf->bm_coded.reserve(nblk); if (rc) return rc; }
        DF_HIP(hipMemsetAsync(wf->bm_coded, 0, nblk, st));
        wf->code_cap = nblk * 512;
    }
    // look-ahead: with on-demand tables or models still to make, blocks NEAR the alive set get theirs on the side
    // stream while the sweep runs -- unless the caller wants models made at once (then everything stays on the launch stream, in order)
    bool ahead = !(flags & (DF_WARP_NO_PREFETCH | DF_WARP_BLOCK_MODEL_NOW));
    if (ahead) { int rc = df_side_init(wf); if (rc) return rc; }
    // The side stream costs a fork and a join (~13 us of barrier packets per frame): worth it while blocks are being built or modelled,
    // not on a scene at rest.  Whether anything was listed lately comes from the plan kernel's host report -- read without a
    // synchronisation, so it may be frames old; it only decides WHERE optional work runs.  On from the first sweeps over new tables,
    // while the last report listed anything, and every 8th sweep as a probe (a camera that starts to move is picked up by the urgent
    // list at once, by the look-ahead within the report's age).
    // (The unsynchronised read makes WHICH frame switches the side stream off depend on host / GPU timing -- never a result, but the
    // swept-voxel counter and frame times of a run.  DF_WARP_STEADY_PREFETCH keeps the look-ahead on in every frame: what tests and
    // measurements that compare such counters between runs pass -- ADVICE r4.)
    if (ahead && !(flags & DF_WARP_STEADY_PREFETCH) && wf->tab_sweeps >= 8 && (wf->tab_sweeps & 7) != 0 && wf->host_report &&
        wf->host_report[0] == 0u && wf->host_report[1] == 0u && wf->host_report[2] == 0u) ahead = false;
    const bool quiet = !ahead && !(flags & (DF_WARP_NO_PREFETCH | DF_WARP_BLOCK_MODEL_NOW));      // a frame at rest: optional work waits for the next probe
    const int want_models_policy = want_models;
    const int want_models_now = quiet ? 0 : want_models_policy;
    // (not on the very first sweep over new tables: the urgent build of the whole alive set is the frame then, and a node set that
    // changes every frame never pays for look-ahead work)
    a.pf_margin = ahead && !wf->tab_complete && wf->tab_sweeps >= 1 ? DF_WARP_PREFETCH_MARGIN_M : 0.f;
    a.pf_cap = DF_WARP_PREFETCH_CAP;
    uint32_t* cnt = wf->blk_cnt + 8 * wf->blk_phase;
    uint32_t* cnt_next = wf->blk_cnt + 8 * (wf->blk_phase ^ 1);
    uint32_t* list_urgent = wf->blk_work, *list_ahead = wf->blk_work + wf->blk_cap, *list_model = wf->blk_work + 2 * wf->blk_cap;
    hipLaunchKernelGGL(df_block_verdict_kernel, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, st, a, wf->rot, wf->node_t, nbx, nby, nbz,
                       wf->blk_state, wf->blk_wmax, wf->brick_thr + wf->off_cap, wf->bx, wf->by, a.tile_wmax != nullptr ? 1 : 0,
                       (use_models && wf->bm_cap >= nblk ? 1 : 0) | (k == 8 && wf->bm_cnt && wf->code_tab && wf->bm_ids && wf->bm_coded && wf->code_cap >= nblk * 512 ? 2 : 0),     // (bit 1: the blocks' codes exist)
                       want_models_now,
                       wf->tab_complete ? 0 : 1, wf->bm_idx, wf->bm_lam, wf->bm_w, wf->bm_cnt, wf->bm_coded, wf->blk_alive, list_urgent, list_ahead, list_model,
                       cnt, cnt_next);
    a.blk_cnt = cnt; a.host_report = (uint32_t*)wf->host_report; a.sweep_no = (uint32_t)wf->tab_sweeps;
    DF_LAUNCH_CHECK();
#ifdef DF_TRACE_VERDICT
    if (getenv("DF_TRACE_VERDICT_FILE")) {
        DF_HIP(hipStreamSynchronize(st));
        static unsigned long long h[8192 * 4];
        DF_HIP(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_df_vtrace), sizeof(h)));
        FILE* f = fopen(getenv("DF_TRACE_VERDICT_FILE"), "wb");
        if (f) { fwrite(h, 8, 8192 * 4, f); fclose(f); }
    }
#endif
    wf->blk_phase ^= 1;
    // (every frame: running this pass only every 4th frame saved its 4.6 us launch and cost 3 % more swept voxels, 18 us, on a moving camera)
    auto launch_models = [&](hipStream_t s2) -> int {
        const DfWarpedArgs b = df_table_args(wf);
        static unsigned g8 = 0, g4 = 0;
        if (!g8) {
            g8 = df_work_grid((const void*)df_block_model_kernel<8>); g4 = df_work_grid((const void*)df_block_model_kernel<4>);
        }
        if (k == 8) hipLaunchKernelGGL(df_block_model_kernel<8>, dim3(g8), dim3(256), 0, s2, b, nbx, nby, nbz, list_model, cnt + 1,
                                       wf->bm_idx, wf->bm_lam, wf->bm_w, wf->bm_cnt, wf->blk_state);
        else hipLaunchKernelGGL(df_block_model_kernel<4>, dim3(g4), dim3(256), 0, s2, b, nbx, nby, nbz, list_model, cnt + 1,
                                wf->bm_idx, wf->bm_lam, wf->bm_w, wf->bm_cnt, wf->blk_state);
        DF_LAUNCH_CHECK();
        return DF_OK;
    };
    const bool side_work = ahead && (!wf->tab_complete || want_models_now);
    if (side_work) {
        // fork: the side stream starts once the verdict pass has written the lists; its kernels touch only blocks this frame's sweep
        // does not read (near, not alive) or structures the sweep never reads (model records, state bytes)
        DF_HIP(hipEventRecord(wf->ev_fork, st));
        DF_HIP(hipStreamWaitEvent(wf->side, wf->ev_fork, 0));
        // from here on the side stream may hold kernels that write tables, state bytes and model records: whatever fails below, the next
        // call must not touch them before those kernels are done (an early return used to leave the fork unjoined)
        int rc_side = DF_OK;
        if (!wf->tab_complete) rc_side = df_build_listed(wf, cnt, wf->side, 1);
        if (rc_side == DF_OK && want_models_now) rc_side = launch_models(wf->side);
        if (hipEventRecord(wf->ev_join, wf->side) == hipSuccess) wf->side_pending = true;      // joined by the next call that touches the tables
        else { (void)hipGetLastError(); df_side_drain(wf); if (rc_side == DF_OK) rc_side = (int)hipErrorUnknown; }
        if (rc_side != DF_OK) return rc_side;
    }
    if (!wf->tab_complete) { int rc = df_build_listed(wf, cnt, st, 0); if (rc) return rc; }      // urgent: before this frame's sweep
    if (want_models_now && !ahead) { int rc = launch_models(st); if (rc) return rc; }
    a.blk_alive = wf->blk_alive; a.bm_nbx = nbx; a.bm_nby = nby;
    wf->alive_valid = true;
    return DF_OK;
}

// The launch state dfusion_integrate_warped_prepare leaves for dfusion_integrate_warped_sweep
typedef void (*df_lds_kernel_t)(const DfWarpedArgs, const DfWarpView, int);
struct DfPrepared { DfWarpedArgs a; DfWarpView W; df_lds_kernel_t kern; dim3 grid; unsigned threads; size_t lds; int tiles_x; DfVolume v; DfSlab s; unsigned long long seq; };
DfWarpField::DfWarpField() = default;
DfWarpField::~DfWarpField() = default;
enum { DF_MODE_WHOLE = 0, DF_MODE_PREPARE = 1 };

static int df_integrate_warped_impl(const uint16_t* dists, size_t pitch, int cols, int rows, DfVolume v, const DfSlab* slab,
                                    const float vol2world[12], const float world2cam[12], const float proj[4],
                                    DfWarpField* wf, int k, unsigned flags, unsigned long long* n_updated, dfStream stream, int mode);

extern "C" int dfusion_integrate_warped(const uint16_t* dists, size_t pitch, int cols, int rows, DfVolume v, const DfSlab* slab,
                                        const float vol2world[12], const float world2cam[12], const float proj[4],
                                        DfWarpField* wf, int k, unsigned flags, unsigned long long* n_updated, dfStream stream)
{
    return df_integrate_warped_impl(dists, pitch, cols, rows, v, slab, vol2world, world2cam, proj, wf, k, flags, n_updated, stream, DF_MODE_WHOLE);
}

// ---- the frame's warped integrate in two calls (include/dfusion.h): everything that does not touch the volume -- dists pyramid, verdict pass,
// table builds, launch plan -- and the sweep.  The halves may be issued on different streams; the handle's events order them.
extern "C" int dfusion_integrate_warped_prepare(const uint16_t* dists, size_t pitch, int cols, int rows, DfVolume geometry, const DfSlab* slab,
                                                const float vol2world[12], const float world2cam[12], const float proj[4],
                                                DfWarpField* wf, int k, unsigned flags, dfStream stream)
{
    if (!wf) return DF_E_INVALID;
    if (!wf->split_events) {
        hipEvent_t e[3] = {nullptr, nullptr, nullptr};
        for (int i = 0; i < 3; ++i)
            if (hipEventCreateWithFlags(&e[i], hipEventDisableTiming) != hipSuccess) {
                for (int j = 0; j < i; ++j) (void)hipEventDestroy(e[j]);
                return (int)hipGetLastError();
            }
        wf->ev_prep_done = e[0]; wf->ev_sweep_done[0] = e[1]; wf->ev_sweep_done[1] = e[2]; wf->split_events = true;
    }
    wf->prep_valid = false;
    if (!geometry.data) geometry.data = (void*)(size_t)16;          // (never dereferenced by the prepare half; df_volume_valid wants a pointer)
    const int rc = df_integrate_warped_impl(dists, pitch, cols, rows, geometry, slab, vol2world, world2cam, proj, wf, k, flags, nullptr, stream, DF_MODE_PREPARE);
    if (rc != DF_OK) return rc;
    DF_HIP(hipEventRecord(wf->ev_prep_done, (hipStream_t)stream));
    return DF_OK;
}

extern "C" int dfusion_integrate_warped_sweep(DfVolume v, const DfSlab* slab, DfWarpField* wf, unsigned long long* n_updated, dfStream stream)
{
    if (!wf || !df_volume_valid(v)) return DF_E_INVALID;
    const DfSlab s = df_slab_or_full(v, slab);
    if (!df_slab_valid(v, s)) return DF_E_INVALID;
    if (s.z_own_n == 0) return DF_OK;                                // (as dfusion_integrate_warped: nothing to sweep, nothing was prepared)
    DfPrepared* P = wf->prep.get();
    if (!P || !wf->prep_valid) return DF_E_INVALID;                  // no prepare call pending on this handle
    if (memcmp(P->v.dims, v.dims, sizeof(v.dims)) || memcmp(P->v.voxel_size, v.voxel_size, sizeof(v.voxel_size)) || P->v.trunc_dist != v.trunc_dist ||
        P->v.max_weight != v.max_weight || memcmp(&P->s, &s, sizeof(s))) return DF_E_INVALID;       // not the volume the plan was made for
    hipStream_t st = (hipStream_t)stream;
    wf->prep_valid = false;
    DF_HIP(hipStreamWaitEvent(st, wf->ev_prep_done, 0));
    P->a.vol = (uint32_t*)v.data; P->a.n_upd = n_updated;
    P->kern<<<P->grid, dim3(P->threads), P->lds, st>>>(P->a, P->W, P->tiles_x);
    DF_LAUNCH_CHECK();
    DF_HIP(hipEventRecord(wf->ev_sweep_done[P->seq & 1], st));
    wf->recorded_seq = P->seq; wf->ring_seq[P->seq & 1] = P->seq;
    return DF_OK;
}

static int df_integrate_warped_impl(const uint16_t* dists, size_t pitch, int cols, int rows, DfVolume v, const DfSlab* slab,
                                    const float vol2world[12], const float world2cam[12], const float proj[4],
                                    DfWarpField* wf, int k, unsigned flags, unsigned long long* n_updated, dfStream stream, int mode)
{
    if (!dists || !vol2world || !world2cam || !proj || !wf || cols <= 0 || rows <= 0 || !df_pitch_ok(pitch, cols, 2) || !df_volume_valid(v)) return DF_E_INVALID;
    if (k < 1 || k > 8 || wf->M < k) return DF_E_INVALID;
    DfSlab s = df_slab_or_full(v, slab);
    if (!df_slab_valid(v, s)) return DF_E_INVALID;
    if (!wf->index_valid || wf->k_built < k || memcmp(wf->geom_dims, v.dims, sizeof(wf->geom_dims)) ||
        memcmp(wf->geom_vs, v.voxel_size, sizeof(wf->geom_vs)) || memcmp(wf->geom_aff, vol2world, sizeof(wf->geom_aff)))
        return DF_E_NO_INDEX;
    if (s.z_own_n == 0) return DF_OK;
    hipStream_t st = (hipStream_t)stream;
    // (sweeps issued through the split API on another stream: the single call waits for all of them; a prepare only for the sweeps that
    // still read what it rewrites -- see the plan sets below and df_warp_pack)
    if (mode == DF_MODE_WHOLE) { int rc = df_wait_split_sweep(wf, st); if (rc) return rc; }
    { int rc = df_side_join(wf, st); if (rc) return rc; }     // the previous call's look-ahead builds (tables, models, state bytes)
    wf->prep_valid = false;                                   // (a prepared plan that was never swept is void once the handle's scratch is rewritten)

    DfWarpedArgs a;
    memset(&a, 0, sizeof(a));
    a.vol = (uint32_t*)v.data; a.X = v.dims[0]; a.Y = v.dims[1]; a.Z = v.dims[2];
    a.z_store0 = s.z_store0; a.z_own0 = s.z_own0; a.z_own_n = s.z_own_n;
    a.vsx = v.voxel_size[0]; a.vsy = v.voxel_size[1]; a.vsz = v.voxel_size[2];
    a.vol2world = df_aff(vol2world); a.world2cam = df_aff(world2cam);
    {
        static const float I9[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
        a.v2w_identity = memcmp(vol2world, I9, sizeof(I9)) == 0;     // bitwise: -0 entries do not qualify
    }
    a.P.dists = dists; a.P.pitch = pitch; a.P.cols = cols; a.P.rows = rows;
    a.P.fx = proj[0]; a.P.fy = proj[1]; a.P.cx = proj[2]; a.P.cy = proj[3];
    a.P.trunc = v.trunc_dist; a.P.trunc_inv = 1.f / v.trunc_dist; a.P.max_weight = v.max_weight;
    a.sat_ok = df_sat_trunc_ok(v.trunc_dist) ? 1 : 0;
    a.n_upd = n_updated;
    a.n_swept = wf->dbg_swept;
    a.kf = (float)k; a.cam_scale = 1.f; a.origin_cam = -1.f;
    const bool use_tab = wf->tab_valid && wf->tab_k == k && !(flags & DF_WARP_NO_TABLE) && s.z_own0 >= wf->tab_z0 &&
                         s.z_own0 + s.z_own_n <= wf->tab_z0 + wf->tab_zn;
    const bool use_w = use_tab && wf->w_tab_valid && !(flags & DF_WARP_NO_WEIGHT_TABLE);
    if (use_tab) {
        a.knn_tab = wf->knn_tab; a.tab_z0 = wf->tab_z0;
        a.tab_ntx = (a.X + DF_TAB_TX - 1) / DF_TAB_TX; a.tab_nty = (a.Y + DF_TAB_TY - 1) / DF_TAB_TY;
        a.tab_nvox = (size_t)a.tab_ntx * DF_TAB_TX * a.tab_nty * DF_TAB_TY * wf->tab_zn;
    }
    if (use_w) a.w_tab = wf->w_tab;
    // the pipelined sweep's preconditions, decided ONCE: which pyramid is built below and which kernel is launched further down both
    // follow from them (they used to be two hand-copied predicates).  The pipelined kernel forms row * pitch with a 24-bit
    // multiply and a 32-bit dists offset.  It needs no LDS node table (round 6): k = 8 blends out of per-wave union copies or gathers from
    // the L2, for ANY node count; k = 4 keeps the table (32 B per node) where it fits the CU's LDS.  DF_WARP_NO_LDS asks for the plain
    // gather kernel (df_warp_rows_kernel: no plan, no verdicts).
    const size_t lds_limit = df_lds_limit();
    const bool no_lds = (flags & DF_WARP_NO_LDS) != 0;
    const bool lds_fits = (size_t)wf->M * 32 <= lds_limit;
    const bool pipe_form_ok = use_w && !(flags & DF_WARP_NO_PIPELINE) && pitch < (1u << 24) && rows < (1 << 24) &&
                              (unsigned long long)rows * pitch < (1ull << 32) && (unsigned long long)v.dims[0] * v.dims[1] < (1ull << 30);
    const bool pipe_sweep = use_tab && !no_lds && pipe_form_ok && (k == 8 || k == 4);

    if (!(flags & DF_WARP_NO_CULL) && proj[0] > 0.f && proj[1] > 0.f) {
        if (!(flags & DF_WARP_NO_DEPTH_PYRAMID)) {
            const size_t elems = df_pyramid_elems(cols, rows);
            { int rc = wf->pyr_mem.reserve(elems); if (rc) return rc; }
            // the pipelined sweep (the product path) reads the pyramid in its verdict pass only, and its plan kernel re-arms the
            // image-maximum word: levels 1..5 in ONE launch.  The other kernels take the full pyramid (two launches).
            const bool pipe_path = pipe_sweep;
            // The image-maximum word: TWO of them ([6], [7]), used alternately; every plan kernel zeroes both once its readers are done.
            // A call that returns early between its pyramid build and its plan kernel leaves ITS word dirty -- the next call uses the other
            // one (zeroed by the plan kernel before), and that call's plan kernel cleans both (no memset node per frame).
            wf->max_phase ^= 1;
            unsigned int* max_word = (unsigned int*)(wf->bounds_dev + 6 + wf->max_phase);
            int rc = df_build_dists_pyramid(dists, pitch, cols, rows, wf->pyr_mem, wf->pyr_mem.cap, &a.py, st, pipe_path, nullptr,
                                            pipe_path ? max_word : nullptr);
            if (rc) return rc;
        }
        if (a.py.top == 0) {                                      // no pyramid (switched off, or an image under 32 px): the image-wide maximum alone
            DF_HIP(hipMemsetAsync(wf->bounds_dev + 2, 0, sizeof(float), st));
            hipLaunchKernelGGL(df_dists_max_kernel, dim3(64), dim3(256), 0, st, dists, pitch, cols, rows, wf->bounds_dev + 2);
            DF_LAUNCH_CHECK();
        }
        {   // world2cam rigid (R^T R = I to 1e-5)?  Then the distance bound of df_tile_culled holds with |world2cam.t|.
            bool rigid = true;
            for (int i = 0; i < 3 && rigid; ++i)
                for (int j = 0; j < 3; ++j) {
                    double d = 0.0;
                    for (int r = 0; r < 3; ++r) d += (double)world2cam[3 * r + i] * world2cam[3 * r + j];
                    if (!(fabs(d - (i == j ? 1.0 : 0.0)) < 1e-5)) { rigid = false; break; }
                }
            a.origin_cam = rigid ? (float)(sqrt((double)world2cam[9] * world2cam[9] + (double)world2cam[10] * world2cam[10] +
                                                (double)world2cam[11] * world2cam[11]) * 1.0001 + 1e-6) : -1.f;
        }
        const double r = use_tab ? df_tile_radius(vol2world, DF_ROW_TX, DF_ROW_TY, DF_ROW_TZ, v)
                                 : df_tile_radius(vol2world, DF_BRICK, DF_BRICK, DF_BRICK, v);
        double fro = 0.0;    // Frobenius norm of world2cam.R bounds its operator norm; == sqrt(3) for a rotation
        for (int i = 0; i < 9; ++i) fro += (double)world2cam[i] * world2cam[i];
        fro = sqrt(fro);
        a.cam_scale = (float)((fabs(fro - 1.7320508075688772) < 1e-3) ? 1.001 : fro * 1.001);
        a.tile_r = (float)(r * 1.001 + 1e-6);
        a.cull = wf->bounds_dev;
        if (use_w && !(flags & DF_WARP_NO_ZERO_SKIP)) a.tile_wmax = wf->tile_wmax;
    }

    DfWarpView W = df_view(wf);
    if (use_tab && !no_lds && (pipe_sweep || lds_fits)) {
        const int tiles_x = (a.X + DF_ROW_TX - 1) / DF_ROW_TX, tiles_y = (a.Y + DF_LDS_TY - 1) / DF_LDS_TY;
        const int zt_lo = s.z_own0 / DF_ROW_TZ, zt_hi = (s.z_own0 + s.z_own_n - 1) / DF_ROW_TZ;
        a.bz0 = zt_lo;
        const bool pipe_ok = pipe_sweep;
        if (a.cull) a.tile_r = (float)(df_tile_radius(vol2world, pipe_ok ? 8 : DF_ROW_TX, pipe_ok ? 8 : DF_LDS_TY, DF_ROW_TZ, v) * 1.001 + 1e-6);
        // LDS of a launch: the node table (32 B a node) for the kernels that keep one -- k = 4's pipelined sweep where it fits, the batched
        // kernel of the other k --, 4 KiB of union copies per wave for k = 8's, nothing for k = 4 without a table
        const bool k4_table = pipe_ok && k == 4 && lds_fits;
        const size_t lds = !pipe_ok || k4_table ? (size_t)wf->M * 32 : k == 8 ? (size_t)(DF_PIPE_WGT / 64) * 4096 : 0;
        typedef void (*lds_kernel_t)(const DfWarpedArgs, const DfWarpView, int);
        lds_kernel_t kern = nullptr;
        // tile layers per workgroup: long walks amortise the LDS fill and the pipeline ramp, short ones even out the last round of
        // workgroups on the 256 CUs (measured: 4 layers best at 256^3 = 1024 workgroups, 8 at 512^3, 16 at 1024^3 = 16384)
        const long long cols_layers = (long long)tiles_x * tiles_y * (zt_hi - zt_lo + 1);
        const bool pipe = pipe_sweep;                           // df_warp_rows_lds_kernel always walks DF_LDS_ZT layers per workgroup
        a.zt = !pipe ? DF_LDS_ZT : cols_layers <= 8192 ? 4 : cols_layers <= 65536 ? 8 : 16;
        dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)((zt_hi - zt_lo + 1 + a.zt - 1) / a.zt));
        const bool wide = k4_table && lds > 80 * 1024;          // one workgroup per CU either way: make it 1024 threads
        const bool vi = a.v2w_identity != 0;
        // workgroup geometry: k = 8 runs 768 threads, one plane per batch (<= 80 VGPRs: two workgroups per CU, 6 waves / SIMD; round 5: -2 to
        // -4 % against 512 threads, two planes, 4 waves); k = 4 keeps two planes per batch (+4 % that way at 256^3)
        unsigned wg_threads = 512u;
        if (pipe_ok && k == 8) {
            kern = vi ? df_warp_rows_pipe_kernel<8, 1, DF_PIPE_WGT, true, false> : df_warp_rows_pipe_kernel<8, 1, DF_PIPE_WGT, false, false>;
            wg_threads = (unsigned)DF_PIPE_WGT;
        } else if (pipe_ok && k4_table) {
            kern = wide ? (vi ? df_warp_rows_pipe_kernel<4, 2, 1024, true, true> : df_warp_rows_pipe_kernel<4, 2, 1024, false, true>)
                        : (vi ? df_warp_rows_pipe_kernel<4, 2, 512, true, true> : df_warp_rows_pipe_kernel<4, 2, 512, false, true>);
            wg_threads = wide ? 1024u : 512u;
        } else if (pipe_ok) {
            kern = vi ? df_warp_rows_pipe_kernel<4, 2, 512, true, false> : df_warp_rows_pipe_kernel<4, 2, 512, false, false>;
        }
        else if (use_w) { DF_DISPATCH_K(k, kern = (df_warp_rows_lds_kernel<K, true, 2>)); }
        else { DF_DISPATCH_K(k, kern = (df_warp_rows_lds_kernel<K, false, 1>)); }
        // (the CU's whole LDS, whatever THIS launch asks for: the attribute belongs to the kernel, not to the launch, and two host threads
        // sweeping warp fields of different sizes would otherwise lower it under each other's launches)
        if (lds > lds_limit) return DF_E_INVALID;
        DF_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_limit));
        if (!pipe) { int rc = df_tables_complete(wf, st); if (rc) return rc; }
        if (pipe) {
            // the launch plan: verdict masks of all strip items (one wave each), the alive ones sorted by work; then one workgroup per
            // 2 (4) plan entries.  The grid is sized for every strip -- nothing is read back -- and the workgroups past the plan's end
            // return at once.
            const unsigned n_zb = grid.y, n_items = (unsigned)tiles_x * (unsigned)tiles_y * 2u * n_zb;
            // The plan lives in TWO sets of (masks, bins), used alternately, and its bin counters in FOUR, each plan kernel zeroing the set of
            // the plan after next: a sweep issued through the split API may still be reading its plan while the next frame's is made.
            if (n_items > wf->plan_cap) {
                { int rc = df_wait_all_sweeps_host(wf); if (rc) return rc; }
                wf->plan_cap = 0;
                for (int i = 0; i < 2; ++i) {
                    { int rc = wf->plan_mask2[i].reserve(n_items); if (rc) return rc; }
                    { int rc = wf->plan_list2[i].reserve((size_t)n_items * DF_PLAN_BINS); if (rc) return rc; }      // the bins
                    { int rc = wf->plan_code2[i].reserve(n_items); if (rc) return rc; }
                }
                wf->plan_cap = n_items; wf->plan_reader[0] = wf->plan_reader[1] = 0;
            }
            if (!wf->plan_hist) {
                { int rc = wf->plan_hist.reserve(4 * 128); if (rc) return rc; }
                DF_HIP(hipMemsetAsync(wf->plan_hist, 0, 4 * 128 * sizeof(unsigned int), st));
                wf->hphase = 0;
            }
            wf->pphase ^= 1;
            { int rc = df_wait_reader(wf, wf->plan_reader[wf->pphase], st); if (rc) return rc; }     // (the sweep two plans ago)
            if (a.cull) { int rc = df_block_verdicts(wf, a, k, flags, st); if (rc) return rc; }
            else { int rc = df_tables_complete(wf, st); if (rc) return rc; }
            ++wf->tab_sweeps;
            unsigned int* cnt = wf->plan_hist + 128 * (wf->hphase & 3u);
            unsigned int* cnt_next = wf->plan_hist + 128 * ((wf->hphase + 2u) & 3u);       // (last read by the sweep two plans ago: waited for above)
            unsigned long long* pmask = wf->plan_mask2[wf->pphase]; unsigned int* plist = wf->plan_list2[wf->pphase];
            // 4-bit neighbour codes (k = 8): for the cells whose block the model pass has been over, unless the models are switched off
            unsigned long long* pcode = nullptr;
            if (k == 8 && a.cull && a.blk_alive && wf->code_tab && wf->bm_ids && wf->bm_coded && wf->bm_cap >= (size_t)a.bm_nbx * a.bm_nby * (wf->tab_zn / 8) &&
                !(flags & (DF_WARP_NO_BLOCK_MODEL | DF_WARP_NO_CODES))) {
                pcode = wf->plan_code2[wf->pphase];
                a.code_tab = wf->code_tab; a.bm_ids = wf->bm_ids; a.bm_coded = wf->bm_coded;
            }
            hipLaunchKernelGGL(df_sweep_plan_kernel, dim3((n_items + DF_PLAN_WG / 64 - 1) / (DF_PLAN_WG / 64)), dim3(DF_PLAN_WG), 0, st, a, tiles_x, tiles_y, n_items, pmask, cnt,
                               plist, cnt_next, pcode);
            DF_LAUNCH_CHECK();
            a.plan_code = pcode;
            ++wf->hphase;                                                  // (only once the kernel that zeroes the set after next is in the stream)
            a.plan_mask = pmask; a.plan_bins = plist; a.plan_cnt = cnt; a.plan_items = n_items; a.plan_tiles_y = tiles_y;
            // this plan's sweep: its number, and what it will read
            wf->plan_reader[wf->pphase] = wf->node_reader[wf->nphase] = ++wf->seq;
            const unsigned spw = wg_threads >= 256u ? wg_threads / 256u : 1u;
            const unsigned groups = (n_items + spw - 1) / spw;
            grid = dim3(groups, 1);
#ifdef DF_TRACE_WG
            static unsigned long long* trace_dev = nullptr; static size_t trace_cap = 0;
            const size_t trace_n = (size_t)groups * (wg_threads / 64u) * 4;
            if (trace_n > trace_cap) { (void)hipFree(trace_dev); DF_HIP(hipMalloc((void**)&trace_dev, trace_n * 8)); trace_cap = trace_n; }
            DF_HIP(hipMemsetAsync(trace_dev, 0, trace_n * 8, st));
            a.trace = trace_dev;
            kern<<<grid, dim3(wg_threads), lds, st>>>(a, W, tiles_x);
            if (getenv("DF_TRACE_FILE")) {
                DF_HIP(hipStreamSynchronize(st));
                unsigned long long* h = (unsigned long long*)malloc(trace_n * 8);
                DF_HIP(hipMemcpy(h, trace_dev, trace_n * 8, hipMemcpyDeviceToHost));
                FILE* f = fopen(getenv("DF_TRACE_FILE"), "wb");
                if (f) { unsigned long long hdr[4] = {groups, 1, (unsigned long long)(wg_threads / 64u), 0}; fwrite(hdr, 8, 4, f); fwrite(h, 8, trace_n, f); fclose(f); }
                free(h);
            }
            DF_LAUNCH_CHECK();
            return DF_OK;
#endif
        }
        if (mode == DF_MODE_PREPARE) {
            if (!pipe) return DF_E_INVALID;                                // (the split exists for the cached, pipelined sweep only)
            if (!wf->prep) wf->prep.reset(new DfPrepared());
            DfPrepared* P = wf->prep.get();
            P->a = a; P->W = W; P->kern = kern; P->grid = grid; P->threads = wg_threads; P->lds = lds; P->tiles_x = tiles_x; P->v = v; P->s = s;
            P->seq = wf->seq;
            wf->prep_valid = true;
            return DF_OK;
        }
        kern<<<grid, dim3(wg_threads), lds, st>>>(a, W, tiles_x);
        if (pipe && wf->split_events) {                                   // (a handle that is also driven through the split API: this sweep counts)
            DF_LAUNCH_CHECK();
            DF_HIP(hipEventRecord(wf->ev_sweep_done[wf->seq & 1], st));
            wf->recorded_seq = wf->seq; wf->ring_seq[wf->seq & 1] = wf->seq;
        }
    } else if (use_tab) {
        if (mode == DF_MODE_PREPARE) return DF_E_INVALID;
        { int rc = df_tables_complete(wf, st); if (rc) return rc; }
        const int tiles_x = (a.X + DF_ROW_TX - 1) / DF_ROW_TX, tiles_y = (a.Y + DF_ROW_TY - 1) / DF_ROW_TY;
        const int zt_lo = s.z_own0 / DF_ROW_TZ, zt_hi = (s.z_own0 + s.z_own_n - 1) / DF_ROW_TZ;
        a.bz0 = zt_lo;
        dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)(zt_hi - zt_lo + 1));
        if (use_w) { DF_DISPATCH_K(k, df_warp_rows_kernel<K, true, 4><<<grid, dim3(256), 0, st>>>(a, W, tiles_x)); }
        else { DF_DISPATCH_K(k, df_warp_rows_kernel<K, false, 4><<<grid, dim3(256), 0, st>>>(a, W, tiles_x)); }
    } else {
        if (mode == DF_MODE_PREPARE) return DF_E_INVALID;
        const int bz_lo = s.z_own0 / DF_BRICK, bz_hi = (s.z_own0 + s.z_own_n - 1) / DF_BRICK;
        a.bz0 = bz_lo;
        dim3 grid((unsigned)(W.bx * W.by), (unsigned)(bz_hi - bz_lo + 1));
        DF_DISPATCH_K(k, df_warp_brick_kernel<K, false><<<grid, dim3(256), 0, st>>>(a, W));
    }
    DF_LAUNCH_CHECK();
    return DF_OK;
}

// Per-voxel k-NN (and weight) tables for planes [z_own0, z_own0 + z_own_n) (this rank's slab): allocated here; built here (every brick)
// or, with `on_demand`, block by block as the sweeps' verdict passes ask for them.
static int df_build_voxel_table(DfWarpField* wf, const DfVolume& v, const DfSlab& s, const float vol2world[12], int k, bool weights,
                                bool on_demand, hipStream_t st)
{
    (void)vol2world;
    if (s.z_own_n == 0) return DF_OK;
    // table planes are brick-aligned so that both voxels of a build thread (z, z+4) index inside it
    const int bz_lo = s.z_own0 / DF_BRICK, bz_hi = (s.z_own0 + s.z_own_n - 1) / DF_BRICK;
    const int tz0 = bz_lo * DF_BRICK, tzn = (bz_hi - bz_lo + 1) * DF_BRICK;
    const int ntx = (v.dims[0] + DF_TAB_TX - 1) / DF_TAB_TX, nty = (v.dims[1] + DF_TAB_TY - 1) / DF_TAB_TY;
    if (ntx * (DF_TAB_TX / 8) > 1023 || nty * (DF_TAB_TY / 8) > 1023 || bz_hi > 4095) return DF_E_INVALID;    // packed brick coordinates of the work lists
    const size_t nvox = (size_t)ntx * DF_TAB_TX * nty * DF_TAB_TY * tzn;          // padded to whole tiles
    const size_t need = nvox * k;
    { int rc = wf->knn_tab.reserve(need); if (rc) return rc; }
    if (weights) { int rc = wf->w_tab.reserve(need); if (rc) return rc; }
    const size_t ntile = (size_t)ntx * nty * (tzn / DF_TAB_TZ);
    if (weights) {
        { int rc = wf->tile_wmax.reserve(ntile); if (rc) return rc; }
        DF_HIP(hipMemsetAsync(wf->tile_wmax, 0, ntile * sizeof(float), st));
    }
    const size_t nblk = (size_t)ntx * (DF_TAB_TX / 8) * nty * (DF_TAB_TY / 8) * (tzn / 8);
    if (nblk > wf->blk_cap) {
        wf->blk_cap = 0;
        { int rc = wf->blk_state.reserve(nblk); if (rc) return rc; }
        { int rc = wf->blk_tie.reserve(nblk); if (rc) return rc; }
        { int rc = wf->blk_wmax.reserve(nblk); if (rc) return rc; }
        { int rc = wf->blk_alive.reserve(nblk); if (rc) return rc; }
        { int rc = wf->blk_work.reserve(3 * nblk); if (rc) return rc; }
        wf->blk_cap = nblk;
    }
    { int rc = wf->blk_cnt.reserve(16); if (rc) return rc; }
    DF_HIP(hipMemsetAsync(wf->blk_cnt, 0, 16 * sizeof(uint32_t), st));
    DF_HIP(hipMemsetAsync(wf->blk_state, on_demand ? 0 : 1, nblk, st));
    DF_HIP(hipMemsetAsync(wf->blk_tie, 0, nblk, st));
    DF_HIP(hipMemsetAsync(wf->blk_wmax, 0, nblk * sizeof(float), st));
    wf->blk_phase = 0;
    wf->tab_z0 = tz0; wf->tab_zn = tzn; wf->tab_k = k; wf->tab_valid = true; wf->w_tab_valid = weights;
    wf->tab_complete = !on_demand; wf->tab_sweeps = 0; wf->alive_valid = false;
    if (on_demand) return DF_OK;
    const DfWarpedArgs a = df_table_args(wf);                  // (reads the fields just set)
    DfWarpView W = df_view(wf);
    dim3 grid((unsigned)(W.bx * W.by), (unsigned)(bz_hi - bz_lo + 1));
    DF_DISPATCH_K(k, df_warp_brick_kernel<K, true><<<grid, dim3(256), 0, st>>>(a, W));
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {                                     // the tables were not built: the handle must not claim them
        wf->tab_valid = false; wf->w_tab_valid = false; wf->tab_complete = false;
        return (int)e;
    }
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
    wf->M = Mn;
    { int rc = df_warp_pack_current(wf, pos, dq, sigma, st); if (rc) return rc; }   // (bounds, the sigma bound [4] included)
    { int rc = df_warp_build_tie_tree(wf, st); if (rc) return rc; }
    if (!wf->index_valid) return DF_OK;
    const size_t nb = (size_t)wf->bx * wf->by * wf->bz;
    const bool tabs = wf->tab_valid && wf->blk_state && wf->blk_tie;
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
                       wf->bx, wf->by, wf->bz, a.bm_nbx, a.bm_nby, nbz, wf->tab_z0 / DF_BRICK, wf->blk_state, a.blk_wmax, wf->blk_tie);
    DF_LAUNCH_CHECK();
    wf->alive_valid = false; wf->tab_complete = false;
    if (!((wf->index_flags & DF_INDEX_TABLES_ON_DEMAND) && wf->w_tab_valid)) {   // eager tables: the stale blocks are re-made here
        int rc = df_tables_complete(wf, st);
        if (rc) return rc;
    }
    DF_HIP(hipStreamSynchronize(st));
    return DF_OK;
}
