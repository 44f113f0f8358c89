// dfusion_warp_nodes.hip -- the warp-field handle: its node arrays on the device (packed positions / transforms, the cull bounds, the
// tie tree), the side stream for look-ahead work and the waits that order a split sweep against the next frame's updates.
#include "dfusion_internal.h"
#include <utility>
#include <vector>

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
int df_side_init(DfWarpField* wf)
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
        wf->host_report[0] = wf->host_report[1] = wf->host_report[2] = DF_REPORT_NONE;
        wf->host_report[3] = 0u;
    }
    wf->ev_fork = ev_fork; wf->ev_join = ev_join; wf->side = side;
    return DF_OK;
}
int df_side_join(DfWarpField* wf, hipStream_t st)
{
    if (!wf->side_pending) return DF_OK;
    DF_HIP(hipStreamWaitEvent(st, wf->ev_join, 0));
    wf->side_pending = false;
    return DF_OK;
}
void df_side_drain(DfWarpField* wf)
{
    if (wf->side) (void)hipStreamSynchronize(wf->side);
    wf->side_pending = false;
}

// A sweep issued through dfusion_integrate_warped_sweep may still be reading the node arrays, the launch plan and the verdict bytes on ITS
// stream when the next frame's set_transforms / prepare arrive on another one: they wait for it on the device.
int df_wait_split_sweep(DfWarpField* wf, hipStream_t st)            // every sweep recorded so far
{
    if (wf->recorded_seq) DF_HIP(hipStreamWaitEvent(st, wf->ev_sweep_done[wf->recorded_seq & 1], 0));
    return DF_OK;
}
// ... or only the sweep (number `reader`) that last read a buffer about to be rewritten.  The ring holds the last two sweeps' events; all
// sweeps are on one stream, so an older one is done when the second-to-last is.  A reader that was never recorded (a prepared plan that was
// dropped) holds nothing.
int df_wait_reader(DfWarpField* wf, unsigned long long reader, hipStream_t st)
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

int df_wait_all_sweeps_host(DfWarpField* wf)
{
    if (wf->recorded_seq) DF_HIP(hipEventSynchronize(wf->ev_sweep_done[wf->recorded_seq & 1]));
    return DF_OK;
}
int df_warp_reserve(DfWarpField* wf, int M)
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
int df_warp_pack_current(DfWarpField* wf, const float* pos, const float* dq, const float* sigma, hipStream_t st)
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
int df_warp_build_tie_tree(DfWarpField* wf, hipStream_t st)
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
    wf->graph_kg = 0;                                          // (the solver's node graph belongs to the old node set)
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

DfWarpView df_view(const DfWarpField* wf)
{
    DfWarpView W;
    W.pos_sigma = wf->pos_sigma; W.rot = wf->rot; W.dual = wf->dual; W.node_t = wf->node_t; W.rt = wf->rt; W.M = wf->M;
    W.brick_off = wf->brick_off; W.brick_list = wf->brick_list; W.brick_thr = wf->brick_thr; W.bx = wf->bx; W.by = wf->by; W.bz = wf->bz;
    W.nf.nodes = wf->nf_ok ? wf->nf_nodes : nullptr; W.nf.vpos = wf->nf_vpos;
    return W;
}
