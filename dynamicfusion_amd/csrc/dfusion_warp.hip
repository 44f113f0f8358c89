// dfusion_warp.hip -- the north-star kernel's translation unit: per-voxel dual-quaternion blend fused into the projective TSDF update
// (dfusion_integrate_warped and its prepare / sweep halves), with the per-voxel table build, the verdict pass and the launch plan.
// The handle and its node arrays are dfusion_warp_nodes.hip, point queries dfusion_warp_points.hip, the brick index and the growth path
// dfusion_warp_index.hip; the kernels launched here are dfusion_warp_sweep.h, dfusion_warp_blocks.h and dfusion_warp_pipe.h.
//
// Replaces (on device) /root/reference/kfusion/src/warp_field.cpp:180-251 (KNN / weighting / DQB /
// warp), the nanoflann kd-tree it queries (warp_field.cpp:275-282), and composes them with
// kfusion/src/cuda/tsdf_volume.cu:77-104.
//
// MI355X design notes
//   * integrate_warped: one 256-thread workgroup per brick; candidate positions (+sigma) are
//     staged in LDS once per brick and read back with broadcast ds_read_b128; each lane keeps the
//     running top-k of its voxel in registers.
#include "dfusion_internal.h"
#include "dfusion_pyramid.h"
#include "dfusion_warp_sweep.h"
#include "dfusion_warp_blocks.h"
#include "dfusion_warp_pipe.h"
#include <algorithm>
#include <atomic>
#include <stdlib.h>
#include <stdio.h>
#include <math.h>

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
DfWarpedArgs df_table_args(const DfWarpField* wf)
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
    if (wf->bm_sub_lam && wf->bm_sub_w && wf->bm_sub_cnt && wf->bm_sub_ok) {
        a.bm_sub_lam = wf->bm_sub_lam; a.bm_sub_w = wf->bm_sub_w; a.bm_sub_cnt = wf->bm_sub_cnt; a.bm_sub_ok = wf->bm_sub_ok;
    }
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
int df_tables_complete(DfWarpField* wf, hipStream_t st)
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
    // ... and the sub-blocks' own blend models, 2 x 4 bytes per union entry: what the sub-verdicts judge half layers by
    if (want_models && k == 8 && (nblk * 512 > wf->code_cap || !wf->bm_ids || !wf->code_tab || !wf->bm_coded || !wf->bm_sub_lam || !wf->bm_sub_w ||
                                  !wf->bm_sub_cnt || !wf->bm_sub_ok || !wf->blk_sub || !wf->sub_list)) {
        wf->code_cap = 0;
        { int rc = wf->bm_ids.reserve(nblk * 64); if (rc) return rc; }
        { int rc = wf->code_tab.reserve(nblk * 512); if (rc) return rc; }
        { int rc = wf->bm_coded.reserve(nblk); if (rc) return rc; }
        DF_HIP(hipMemsetAsync(wf->bm_coded, 0, nblk, st));
        { int rc = wf->bm_sub_lam.reserve(nblk * 8 * DF_BM_NU); if (rc) return rc; }
        { int rc = wf->bm_sub_w.reserve(nblk * 8 * DF_BM_NU); if (rc) return rc; }
        { int rc = wf->bm_sub_cnt.reserve(nblk * 8); if (rc) return rc; }
        { int rc = wf->bm_sub_ok.reserve(nblk); if (rc) return rc; }
        { int rc = wf->blk_sub.reserve(nblk); if (rc) return rc; }
        { int rc = wf->sub_list.reserve(nblk); if (rc) return rc; }
        DF_HIP(hipMemsetAsync(wf->bm_sub_ok, 0, nblk, st));
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
    // sub-verdicts (k = 8): the kept blocks that have sub-block models and touch the dead set are listed and judged per 4 x 4 x 4 sub-block
    // right after the pass.  The verdict bytes alternate between two arrays: the pass reads its neighbours' verdicts of the frame before.
    std::swap(wf->blk_alive, wf->blk_alive_prev);
    const bool codes_exist = k == 8 && wf->bm_cnt && wf->code_tab && wf->bm_ids && wf->bm_coded && wf->code_cap >= nblk * 512;
    const bool sub_verdicts = use_models && wf->bm_cap >= nblk && codes_exist && !(flags & DF_WARP_NO_SUB_VERDICT) && wf->bm_sub_lam && wf->bm_sub_w &&
                              wf->bm_sub_cnt && wf->bm_sub_ok && wf->blk_sub && wf->sub_list && wf->blk_alive_prev;
    if (sub_verdicts) { a.bm_ids = wf->bm_ids; a.bm_sub_lam = wf->bm_sub_lam; a.bm_sub_w = wf->bm_sub_w; a.bm_sub_cnt = wf->bm_sub_cnt; a.bm_sub_ok = wf->bm_sub_ok; }
    hipLaunchKernelGGL(df_block_verdict_kernel, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, st, a, wf->rot, wf->node_t, nbx, nby, nbz,
                       wf->blk_state, wf->blk_wmax, wf->brick_thr + wf->off_cap, wf->bx, wf->by, a.tile_wmax != nullptr ? 1 : 0,
                       (use_models && wf->bm_cap >= nblk ? 1 : 0) | (codes_exist ? 2 : 0) | (sub_verdicts ? 4 : 0),     // (bit 1: the blocks' codes exist; bit 2: sub-verdicts follow)
                       want_models_now,
                       wf->tab_complete ? 0 : 1, wf->bm_idx, wf->bm_lam, wf->bm_w, wf->bm_cnt, wf->bm_coded, wf->blk_alive, list_urgent, list_ahead, list_model,
                       cnt, cnt_next, sub_verdicts ? (uint8_t*)wf->blk_sub : nullptr, wf->sub_list, wf->blk_alive_prev);
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
    if (sub_verdicts) {
        // (it reads models of blocks whose state was 2 when the verdict pass ran -- none that this frame's side-stream model builds write.
        // The list's length stays on the device: at most 1024 workgroups stride over it, those past its end return at once.)
        const unsigned sub_grid = (unsigned)std::min<size_t>((nblk * 8 + 255) / 256, 1024);
        hipLaunchKernelGGL(df_sub_verdict_kernel, dim3(sub_grid), dim3(256), 0, st, a, wf->rot, wf->node_t, nbx, nby, nbz, wf->sub_list, cnt + 5, wf->blk_sub);
        DF_LAUNCH_CHECK();
        a.blk_sub = wf->blk_sub;
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
        // workgroup geometry: k = 8 runs DF_PIPE_WGT = 256 threads (4 waves, 4 KiB of union copies each), one plane per batch (<= 80 VGPRs: six
        // workgroups per CU, 6 waves / SIMD; round 5, at 768 threads: -2 to -4 % against 512 threads, two planes, 4 waves); k = 4 keeps two planes per batch (+4 % that way at 256^3)
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
                    { int rc = wf->plan_mask2[i].reserve((size_t)n_items * 2); if (rc) return rc; }
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
int df_build_voxel_table(DfWarpField* wf, const DfVolume& v, const DfSlab& s, const float vol2world[12], int k, bool weights,
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
        { int rc = wf->blk_alive_prev.reserve(nblk); if (rc) return rc; }
        { int rc = wf->blk_work.reserve(3 * nblk); if (rc) return rc; }
        wf->blk_cap = nblk;
    }
    { int rc = wf->blk_cnt.reserve(16); if (rc) return rc; }
    DF_HIP(hipMemsetAsync(wf->blk_cnt, 0, 16 * sizeof(uint32_t), st));
    DF_HIP(hipMemsetAsync(wf->blk_state, on_demand ? 0 : 1, nblk, st));
    DF_HIP(hipMemsetAsync(wf->blk_tie, 0, nblk, st));
    DF_HIP(hipMemsetAsync(wf->blk_wmax, 0, nblk * sizeof(float), st));
    DF_HIP(hipMemsetAsync(wf->blk_alive, 1, nblk, st));                   // (no verdicts yet: "every neighbour kept" for the first pass's sub-verdict list)
    DF_HIP(hipMemsetAsync(wf->blk_alive_prev, 1, nblk, st));
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
