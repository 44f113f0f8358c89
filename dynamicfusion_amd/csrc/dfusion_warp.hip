// dfusion_warp.hip -- the north-star kernel's translation unit: per-voxel dual-quaternion blend fused into the projective TSDF update
// (dfusion_integrate_warped and its prepare / sweep halves), with the per-voxel table build, the verdict pass and the launch plan.
// The handle and its node arrays are dfusion_warp_nodes.hip, point queries dfusion_warp_points.hip, the brick index and the growth path
// dfusion_warp_index.hip; the kernels launched here are dfusion_warp_sweep.h, dfusion_warp_blocks.h and dfusion_warp_pipe.h, the two
// host decisions (which sweep, where the verdict pass's optional work runs) dfusion_warp_decide.h.
//
// Replaces (on device) /root/reference/kfusion/src/warp_field.cpp:180-251 (KNN / weighting / DQB /
// warp), the nanoflann kd-tree it queries (warp_field.cpp:275-282), and composes them with
// kfusion/src/cuda/tsdf_volume.cu:77-104.
#include "dfusion_internal.h"
#include "dfusion_pyramid.h"
#include "dfusion_warp_sweep.h"
#include "dfusion_warp_blocks.h"
#include "dfusion_warp_pipe.h"
#include "dfusion_warp_decide.h"
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
    if (!wf->tab_valid || !wf->alive_valid || !wf->blk.alive) return DF_E_NO_INDEX;
    const int ntx = (wf->geom_dims[0] + DF_TAB_TX - 1) / DF_TAB_TX, nty = (wf->geom_dims[1] + DF_TAB_TY - 1) / DF_TAB_TY;
    const unsigned per_layer = (unsigned)(ntx * (DF_TAB_TX / 8)) * (unsigned)(nty * (DF_TAB_TY / 8));
    const int nbz = wf->tab_zn / 8, layer0 = wf->tab_z0 / 8;
    const int l_lo = (z0 + 7) / 8, l_hi = min((z0 + zn) / 8, n_layers);                 // layers entirely inside [z0, z0 + zn)
    if (nbz <= 0 || l_hi <= l_lo) return DF_OK;
    hipLaunchKernelGGL(df_alive_per_layer_kernel, dim3((unsigned)nbz), dim3(256), 0, (hipStream_t)stream, wf->blk.alive, mask, per_layer, layer0, l_lo,
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
    a.blk_wmax = wf->w_tab_valid ? wf->blk.wmax : nullptr;
    a.X = wf->geom_dims[0]; a.Y = wf->geom_dims[1]; a.Z = wf->geom_dims[2];
    a.z_store0 = wf->tab_z0; a.z_own0 = wf->tab_z0; a.z_own_n = wf->tab_zn;        // every voxel of the covered bricks gets an entry
    a.vsx = wf->geom_vs[0]; a.vsy = wf->geom_vs[1]; a.vsz = wf->geom_vs[2];
    a.vol2world = df_aff(wf->geom_aff);
    a.knn_tab = wf->knn_tab; a.tab_z0 = wf->tab_z0; a.tab_ntx = ntx; a.tab_nty = nty;
    a.tab_nvox = (size_t)ntx * DF_TAB_TX * nty * DF_TAB_TY * wf->tab_zn;
    a.bz0 = wf->tab_z0 / DF_BRICK;
    a.bm_nbx = ntx * (DF_TAB_TX / 8); a.bm_nby = nty * (DF_TAB_TY / 8);
    const DfBlockCodes& c = wf->codes;
    a.code_tab = c.tab; a.bm_ids = c.ids; a.bm_coded = c.coded;
    if (c.sub_lam && c.sub_w && c.sub_cnt && c.sub_ok) { a.bm_sub_lam = c.sub_lam; a.bm_sub_w = c.sub_w; a.bm_sub_cnt = c.sub_cnt; a.bm_sub_ok = c.sub_ok; }
    a.blk_tie = wf->blk.tie;
    return a;
}
// LDS a workgroup may ask for on this device (160 KiB on gfx950): what the node-table kernels' "fits" is decided against, and the
// dynamic-LDS attribute of their launches (a fixed 160 KiB fails on a part with less, whatever the launch needs)
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
    b.work = wf->blk.work + (size_t)list * wf->blk.cap; b.work_cnt = cnt + (list ? 3 : 0); b.work_cursor = const_cast<uint32_t*>(cnt) + (list ? 4 : 2);
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
    uint32_t* cnt = wf->blk_cnt + 8 * wf->blk_phase, *cnt_next = wf->blk_cnt + 8 * (wf->blk_phase ^ 1);
    hipLaunchKernelGGL(df_blocks_unbuilt_kernel, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, st, b.bm_nbx, b.bm_nby, nbz, wf->bx, wf->by,
                       wf->tab_z0 / 8, wf->blk.state, wf->blk.work, cnt, cnt_next);
    DF_LAUNCH_CHECK();
    wf->blk_phase ^= 1;
    DF_TRY(df_build_listed(wf, cnt, st));
    wf->tab_complete = true;
    return DF_OK;
}

// blend models for the blocks on the verdict pass's model list (length cnt[1])
static int df_model_listed(DfWarpField* wf, int k, int nbx, int nby, int nbz, uint32_t* cnt, hipStream_t st)
{
    const DfWarpedArgs b = df_table_args(wf);
    uint32_t* list_model = wf->blk.work + 2 * wf->blk.cap;
    static unsigned g8 = 0, g4 = 0;
    if (!g8) { g8 = df_work_grid((const void*)df_block_model_kernel<8>); g4 = df_work_grid((const void*)df_block_model_kernel<4>); }
    if (k == 8) hipLaunchKernelGGL(df_block_model_kernel<8>, dim3(g8), dim3(256), 0, st, b, nbx, nby, nbz, list_model, cnt + 1,
                                   wf->bm.idx, wf->bm.lam, wf->bm.w, wf->bm.cnt, wf->blk.state);
    else hipLaunchKernelGGL(df_block_model_kernel<4>, dim3(g4), dim3(256), 0, st, b, nbx, nby, nbz, list_model, cnt + 1,
                            wf->bm.idx, wf->bm.lam, wf->bm.w, wf->bm.cnt, wf->blk.state);
    DF_LAUNCH_CHECK();
    return DF_OK;
}

// The verdict pass of the pipelined sweep (dfusion_warp_blocks.h) and the on-demand work it finds: table builds for alive blocks that
// have none yet, blend models for alive blocks that have tables but no model; what is made, and on which stream, is df_verdict_policy's.
static int df_block_verdicts(DfWarpField* wf, DfWarpedArgs& a, int k, unsigned flags, hipStream_t st)
{
    const int nbx = a.tab_ntx * (DF_TAB_TX / 8), nby = a.tab_nty * (DF_TAB_TY / 8), nbz = wf->tab_zn / 8;
    const size_t nblk = (size_t)nbx * nby * nbz;
    if (nblk == 0 || !wf->blk.ready(nblk)) return DF_E_INVALID;
    // The plan kernel's host report is read without a synchronisation, so it may be frames old; it only decides WHERE optional work runs:
    // never a result, but the swept-voxel counter and frame times of a run (comparisons between runs pass DF_WARP_STEADY_PREFETCH).
    uint32_t report[3] = {DF_REPORT_NONE, DF_REPORT_NONE, DF_REPORT_NONE};    // (what df_side_init, below, would leave in a new one)
    if (wf->host_report) for (int i = 0; i < 3; ++i) report[i] = wf->host_report[i];
    const DfVerdictPolicy p = df_verdict_policy(flags, k, wf->tab_sweeps, wf->tab_complete, report);
    if (p.want_models) DF_TRY(wf->bm.reserve(nblk));
    if (p.want_models && k == 8) DF_TRY(wf->codes.reserve(nblk, st));
    if (p.ahead || p.quiet) DF_TRY(df_side_init(wf));                   // (a quiet frame keeps the side stream for the next probe)
    a.pf_margin = p.pf_margin; a.pf_cap = DF_WARP_PREFETCH_CAP;
    uint32_t* cnt = wf->blk_cnt + 8 * wf->blk_phase, *cnt_next = wf->blk_cnt + 8 * (wf->blk_phase ^ 1);
    uint32_t* list_urgent = wf->blk.work, *list_ahead = wf->blk.work + wf->blk.cap, *list_model = wf->blk.work + 2 * wf->blk.cap;
    // sub-verdicts (k = 8): the kept blocks that have sub-block models and touch the dead set are listed and judged per 4 x 4 x 4 sub-block
    // right after the pass.  The verdict bytes alternate between two arrays: the pass reads its neighbours' verdicts of the frame before.
    std::swap(wf->blk.alive, wf->blk.alive_prev);
    const DfBlockCodes& c = wf->codes;
    const bool models = p.use_models && wf->bm.ready(nblk);
    const bool codes_exist = k == 8 && wf->bm.cnt && c.ready(nblk);
    const bool sub_verdicts = models && codes_exist && !(flags & DF_WARP_NO_SUB_VERDICT);
    if (sub_verdicts) { a.bm_ids = c.ids; a.bm_sub_lam = c.sub_lam; a.bm_sub_w = c.sub_w; a.bm_sub_cnt = c.sub_cnt; a.bm_sub_ok = c.sub_ok; }
    hipLaunchKernelGGL(df_block_verdict_kernel, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, st, a, wf->rot, wf->node_t, nbx, nby, nbz,
                       wf->blk.state, wf->blk.wmax, wf->brick_thr + wf->off_cap, wf->bx, wf->by, a.tile_wmax != nullptr ? 1 : 0,
                       (models ? 1 : 0) | (codes_exist ? 2 : 0) | (sub_verdicts ? 4 : 0),     // (bit 1: the blocks' codes exist; bit 2: sub-verdicts follow)
                       p.want_models_now,
                       wf->tab_complete ? 0 : 1, wf->bm.idx, wf->bm.lam, wf->bm.w, wf->bm.cnt, c.coded, wf->blk.alive, list_urgent, list_ahead, list_model,
                       cnt, cnt_next, sub_verdicts ? (uint8_t*)c.blk_sub : nullptr, c.sub_list, wf->blk.alive_prev);
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
    if (p.side_work) {
        // fork: the side stream starts once the verdict pass has written the lists; its kernels touch only blocks this frame's sweep
        // does not read (near, not alive) or structures the sweep never reads (model records, state bytes)
        DF_HIP(hipEventRecord(wf->ev_fork, st));
        DF_HIP(hipStreamWaitEvent(wf->side, wf->ev_fork, 0));
        // from here on the side stream may hold kernels that write tables, state bytes and model records: whatever fails below, the next
        // call must not touch them before those kernels are done
        int rc_side = DF_OK;
        if (!wf->tab_complete) rc_side = df_build_listed(wf, cnt, wf->side, 1);
        if (rc_side == DF_OK && p.want_models_now) rc_side = df_model_listed(wf, k, nbx, nby, nbz, cnt, wf->side);
        if (hipEventRecord(wf->ev_join, wf->side) == hipSuccess) wf->side_pending = true;      // joined by the next call that touches the tables
        else { (void)hipGetLastError(); df_side_drain(wf); if (rc_side == DF_OK) rc_side = (int)hipErrorUnknown; }
        if (rc_side != DF_OK) return rc_side;
    }
    if (sub_verdicts) {
        // (it reads models of blocks whose state was 2 when the verdict pass ran -- none that this frame's side-stream model builds write.
        // The list's length stays on the device: at most 1024 workgroups stride over it, those past its end return at once.)
        const unsigned sub_grid = (unsigned)std::min<size_t>((nblk * 8 + 255) / 256, 1024);
        hipLaunchKernelGGL(df_sub_verdict_kernel, dim3(sub_grid), dim3(256), 0, st, a, wf->rot, wf->node_t, nbx, nby, nbz, c.sub_list, cnt + 5, c.blk_sub);
        DF_LAUNCH_CHECK();
        a.blk_sub = c.blk_sub;
    }
    if (!wf->tab_complete) DF_TRY(df_build_listed(wf, cnt, st, 0));                            // urgent: before this frame's sweep
    if (p.want_models_now && !p.ahead) DF_TRY(df_model_listed(wf, k, nbx, nby, nbz, cnt, st));
    a.blk_alive = wf->blk.alive; a.bm_nbx = nbx; a.bm_nby = nby; wf->alive_valid = true;
    return DF_OK;
}

// A planned launch of the batched or the pipelined sweep (a.plan_mask set: pipelined) and the geometry it was planned for: what
// df_integrate_warped_impl hands to df_launch_prepared, on the whole call's stack or, from a prepare call to its sweep call, in the handle.
typedef void (*df_lds_kernel_t)(const DfWarpedArgs, const DfWarpView, int);
struct DfPrepared { DfWarpedArgs a; DfWarpView W; df_lds_kernel_t kern; dim3 grid; unsigned threads; size_t lds; int tiles_x; DfVolume v; DfSlab s; unsigned long long seq; };
DfWarpField::DfWarpField() = default;
DfWarpField::~DfWarpField() = default;
static_assert(DF_DECIDE_PIPE_WGT == DF_PIPE_WGT && DF_DECIDE_LDS_ZT == DF_LDS_ZT && DF_ROW_TZ == DF_BRICK, "constants repeated in dfusion_warp_decide.h / assumed below");

// The pipelined sweep's launch plan: verdict masks of all strip items (one wave each), the alive ones sorted by work; then one workgroup per
// 2 (4) plan entries: P.grid, sized for every strip (nothing is read back; the workgroups past the plan's end return at once).
static int df_pipe_plan(DfWarpField* wf, DfPrepared& P, int tiles_y, int k, unsigned flags, hipStream_t st)
{
    DfWarpedArgs& a = P.a;
    const unsigned n_items = (unsigned)P.tiles_x * (unsigned)tiles_y * 2u * P.grid.y;
    // The plan lives in TWO sets of (masks, bins), used alternately, and its bin counters in FOUR, each plan kernel zeroing the set of
    // the plan after next: a sweep issued through the split API may still be reading its plan while the next frame's is made.
    if (n_items > wf->plan_cap) {
        DF_TRY(df_wait_all_sweeps_host(wf));
        wf->plan_cap = 0;
        for (int i = 0; i < 2; ++i) {
            DF_TRY(wf->plan_mask2[i].reserve((size_t)n_items * 2));
            DF_TRY(wf->plan_list2[i].reserve((size_t)n_items * DF_PLAN_BINS));      // the bins
            DF_TRY(wf->plan_code2[i].reserve(n_items));
        }
        wf->plan_cap = n_items; wf->plan_reader[0] = wf->plan_reader[1] = 0;
    }
    if (!wf->plan_hist) {
        DF_TRY(wf->plan_hist.reserve(4 * 128));
        DF_HIP(hipMemsetAsync(wf->plan_hist, 0, 4 * 128 * sizeof(unsigned int), st));
        wf->hphase = 0;
    }
    wf->pphase ^= 1;
    DF_TRY(df_wait_reader(wf, wf->plan_reader[wf->pphase], st));      // (the sweep two plans ago)
    if (a.cull) DF_TRY(df_block_verdicts(wf, a, k, flags, st));
    else DF_TRY(df_tables_complete(wf, st));                          // (no verdicts: every block's tables)
    ++wf->tab_sweeps;
    unsigned int* cnt = wf->plan_hist + 128 * (wf->hphase & 3u);
    unsigned int* cnt_next = wf->plan_hist + 128 * ((wf->hphase + 2u) & 3u);       // (last read by the sweep two plans ago: waited for above)
    unsigned long long* pmask = wf->plan_mask2[wf->pphase]; unsigned int* plist = wf->plan_list2[wf->pphase];
    // 4-bit neighbour codes (k = 8): for the cells whose block the model pass has been over, unless the models are switched off
    unsigned long long* pcode = nullptr;
    const DfBlockCodes& c = wf->codes;
    if (k == 8 && a.cull && a.blk_alive && c.tab && c.ids && c.coded && wf->bm.cap >= (size_t)a.bm_nbx * a.bm_nby * (wf->tab_zn / 8) &&
        !(flags & (DF_WARP_NO_BLOCK_MODEL | DF_WARP_NO_CODES))) {
        pcode = wf->plan_code2[wf->pphase];
        a.code_tab = c.tab; a.bm_ids = c.ids; a.bm_coded = c.coded;
    }
    hipLaunchKernelGGL(df_sweep_plan_kernel, dim3((n_items + DF_PLAN_WG / 64 - 1) / (DF_PLAN_WG / 64)), dim3(DF_PLAN_WG), 0, st, a, P.tiles_x, tiles_y, n_items, pmask, cnt,
                       plist, cnt_next, pcode);
    DF_LAUNCH_CHECK();
    ++wf->hphase;                                                  // (only once the kernel that zeroes the set after next is in the stream)
    a.plan_code = pcode; a.plan_mask = pmask; a.plan_bins = plist; a.plan_cnt = cnt; a.plan_items = n_items; a.plan_tiles_y = tiles_y;
    // this plan's sweep: its number, and what it will read
    wf->plan_reader[wf->pphase] = wf->node_reader[wf->nphase] = ++wf->seq;
    const unsigned spw = P.threads >= 256u ? P.threads / 256u : 1u;
    P.grid = dim3((n_items + spw - 1) / spw, 1);
    return DF_OK;
}

// The argument checks of dfusion_integrate_warped and of its prepare half (include/dfusion.h); *s = the slab to sweep, z_own_n == 0: none.
static int df_warped_check(const uint16_t* dists, size_t pitch, int cols, int rows, const DfVolume& v, const DfSlab* slab, const float vol2world[12],
                           const float world2cam[12], const float proj[4], const DfWarpField* wf, int k, DfSlab* s)
{
    if (!dists || !vol2world || !world2cam || !proj || !wf || cols <= 0 || rows <= 0 || !df_pitch_ok(pitch, cols, 2) || !df_volume_valid(v)) return DF_E_INVALID;
    if (k < 1 || k > 8 || wf->M < k) return DF_E_INVALID;
    *s = df_slab_or_full(v, slab);
    if (!df_slab_valid(v, *s)) return DF_E_INVALID;
    if (!wf->index_valid || wf->k_built < k || memcmp(wf->geom_dims, v.dims, sizeof(wf->geom_dims)) ||
        memcmp(wf->geom_vs, v.voxel_size, sizeof(wf->geom_vs)) || memcmp(wf->geom_aff, vol2world, sizeof(wf->geom_aff)))
        return DF_E_NO_INDEX;
    return DF_OK;
}

// Everything of a warped integrate that does not touch the volume, on `st`.  Which sweep runs is decided ONCE (df_warp_variant), before the
// pyramid build; then the pyramid, the verdict pass with its builds and the launch plan are enqueued and P is filled.  P.kern stays null for
// the brick and table-rows variants, which only the whole call launches.  `pipelined_only` (the prepare half: the split exists for the
// cached, pipelined sweep only) refuses every other variant at the decision.
static int df_integrate_warped_impl(const uint16_t* dists, size_t pitch, int cols, int rows, const DfVolume& v, const DfSlab& s,
                                    const float vol2world[12], const float world2cam[12], const float proj[4],
                                    DfWarpField* wf, int k, unsigned flags, hipStream_t st, bool pipelined_only, DfPrepared& P)
{
    DF_TRY(df_side_join(wf, st));                             // the previous call's look-ahead builds (tables, models, state bytes)
    wf->prep_valid = false;                                   // (a prepared plan that was never swept is void once the handle's scratch is rewritten)
    const int tiles_x = (v.dims[0] + DF_ROW_TX - 1) / DF_ROW_TX, tiles_y = (v.dims[1] + DF_LDS_TY - 1) / DF_LDS_TY;       // (batched and pipelined kernels)
    const int zt_lo = s.z_own0 / DF_ROW_TZ, layers = (s.z_own0 + s.z_own_n - 1) / DF_ROW_TZ - zt_lo + 1;
    const bool tables_cover = wf->tab_valid && wf->tab_k == k && s.z_own0 >= wf->tab_z0 && s.z_own0 + s.z_own_n <= wf->tab_z0 + wf->tab_zn;
    const size_t lds_limit = df_lds_limit();
    const DfWarpVariant d = df_warp_variant(k, wf->M, flags, tables_cover, wf->w_tab_valid, pitch, rows, (unsigned long long)v.dims[0] * v.dims[1],
                                            lds_limit, (long long)tiles_x * tiles_y * layers);
    const bool use_tab = d.kind != DF_SWEEP_BRICKS, lds_rows = d.kind == DF_SWEEP_LDS_ROWS, pipelined = d.kind == DF_SWEEP_PIPELINED;
    if (pipelined_only && !pipelined) return DF_E_INVALID;

    DfWarpedArgs& a = P.a;
    memset(&a, 0, sizeof(a));
    a.X = v.dims[0]; a.Y = v.dims[1]; a.Z = v.dims[2];
    a.z_store0 = s.z_store0; a.z_own0 = s.z_own0; a.z_own_n = s.z_own_n;
    a.vsx = v.voxel_size[0]; a.vsy = v.voxel_size[1]; a.vsz = v.voxel_size[2];
    a.vol2world = df_aff(vol2world); a.world2cam = df_aff(world2cam);
    static const float I9[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    a.v2w_identity = memcmp(vol2world, I9, sizeof(I9)) == 0;         // bitwise: -0 entries do not qualify
    a.P.dists = dists; a.P.pitch = pitch; a.P.cols = cols; a.P.rows = rows;
    a.P.fx = proj[0]; a.P.fy = proj[1]; a.P.cx = proj[2]; a.P.cy = proj[3];
    a.P.trunc = v.trunc_dist; a.P.trunc_inv = 1.f / v.trunc_dist; a.P.max_weight = v.max_weight;
    a.sat_ok = df_sat_trunc_ok(v.trunc_dist) ? 1 : 0; a.n_swept = wf->dbg_swept;
    a.kf = (float)k; a.cam_scale = 1.f; a.origin_cam = -1.f;
    if (use_tab) {
        a.knn_tab = wf->knn_tab; a.tab_z0 = wf->tab_z0;
        a.tab_ntx = (a.X + DF_TAB_TX - 1) / DF_TAB_TX; a.tab_nty = (a.Y + DF_TAB_TY - 1) / DF_TAB_TY;
        a.tab_nvox = (size_t)a.tab_ntx * DF_TAB_TX * a.tab_nty * DF_TAB_TY * wf->tab_zn;
    }
    if (d.weights) a.w_tab = wf->w_tab;
    if (!(flags & DF_WARP_NO_CULL) && proj[0] > 0.f && proj[1] > 0.f) {
        if (!(flags & DF_WARP_NO_DEPTH_PYRAMID)) {
            DF_TRY(wf->pyr_mem.reserve(df_pyramid_elems(cols, rows)));
            // the pipelined sweep reads the pyramid in its verdict pass only, and its plan kernel re-arms the image-maximum word: levels
            // 1..5 in ONE launch; the other kernels take the full pyramid (two launches).  TWO such words ([6], [7]), used alternately: a
            // call that returns early between its pyramid build and its plan kernel leaves ITS word dirty -- the next call uses the other
            // one (zeroed by the plan kernel before), and that call's plan kernel cleans both (no memset node per frame).
            wf->max_phase ^= 1;
            unsigned int* max_word = (unsigned int*)(wf->bounds_dev + 6 + wf->max_phase);
            DF_TRY(df_build_dists_pyramid(dists, pitch, cols, rows, wf->pyr_mem, wf->pyr_mem.cap, &a.py, st, pipelined, nullptr, pipelined ? max_word : nullptr));
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
                    double dot = 0.0;
                    for (int r = 0; r < 3; ++r) dot += (double)world2cam[3 * r + i] * world2cam[3 * r + j];
                    if (!(fabs(dot - (i == j ? 1.0 : 0.0)) < 1e-5)) { rigid = false; break; }
                }
            a.origin_cam = rigid ? (float)(sqrt((double)world2cam[9] * world2cam[9] + (double)world2cam[10] * world2cam[10] +
                                                (double)world2cam[11] * world2cam[11]) * 1.0001 + 1e-6) : -1.f;
        }
        const double r = pipelined ? df_tile_radius(vol2world, 8, 8, DF_ROW_TZ, v)                   // (the tile of the chosen kernel)
                         : use_tab ? df_tile_radius(vol2world, DF_ROW_TX, lds_rows ? DF_LDS_TY : DF_ROW_TY, DF_ROW_TZ, v)
                                   : df_tile_radius(vol2world, DF_BRICK, DF_BRICK, DF_BRICK, v);
        double fro = 0.0;    // Frobenius norm of world2cam.R bounds its operator norm; == sqrt(3) for a rotation
        for (int i = 0; i < 9; ++i) fro += (double)world2cam[i] * world2cam[i];
        fro = sqrt(fro);
        a.cam_scale = (float)((fabs(fro - 1.7320508075688772) < 1e-3) ? 1.001 : fro * 1.001);
        a.tile_r = (float)(r * 1.001 + 1e-6);
        a.cull = wf->bounds_dev;
        if (d.weights && !(flags & DF_WARP_NO_ZERO_SKIP)) a.tile_wmax = wf->tile_wmax;
    }
    P.W = df_view(wf); P.kern = nullptr; P.tiles_x = tiles_x; P.v = v; P.s = s;
    if (!lds_rows && !pipelined) return DF_OK;

    // The kernel, from the variant: k = 8 runs DF_PIPE_WGT = 256 threads (4 waves, 4 KiB of union copies each), one plane per batch (<= 80 VGPRs:
    // six workgroups per CU, 6 waves / SIMD); k = 4 keeps two planes per batch (+4 % that way at 256^3).
    const bool vi = a.v2w_identity != 0;
    if (lds_rows && d.weights) { DF_DISPATCH_K(k, P.kern = (df_warp_rows_lds_kernel<K, true, 2>)); }
    else if (lds_rows) { DF_DISPATCH_K(k, P.kern = (df_warp_rows_lds_kernel<K, false, 1>)); }
    else if (k == 8) P.kern = vi ? df_warp_rows_pipe_kernel<8, 1, DF_PIPE_WGT, true, false> : df_warp_rows_pipe_kernel<8, 1, DF_PIPE_WGT, false, false>;
    else if (d.wide) P.kern = vi ? df_warp_rows_pipe_kernel<4, 2, 1024, true, true> : df_warp_rows_pipe_kernel<4, 2, 1024, false, true>;
    else if (d.k4_table) P.kern = vi ? df_warp_rows_pipe_kernel<4, 2, 512, true, true> : df_warp_rows_pipe_kernel<4, 2, 512, false, true>;
    else P.kern = vi ? df_warp_rows_pipe_kernel<4, 2, 512, true, false> : df_warp_rows_pipe_kernel<4, 2, 512, false, false>;
    a.bz0 = zt_lo; a.zt = d.zt; P.threads = d.threads; P.lds = d.lds;
    P.grid = dim3((unsigned)(tiles_x * tiles_y), (unsigned)((layers + d.zt - 1) / d.zt));
    // (the CU's whole LDS, whatever THIS launch asks for: the attribute belongs to the kernel, not to the launch, and two host threads
    // sweeping warp fields of different sizes would otherwise lower it under each other's launches)
    DF_HIP(hipFuncSetAttribute((const void*)P.kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_limit));
    if (lds_rows) DF_TRY(df_tables_complete(wf, st));
    else DF_TRY(df_pipe_plan(wf, P, tiles_y, k, flags, st));
    P.seq = wf->seq;
    return DF_OK;
}

// The one launch of a planned batched or pipelined sweep into `vol`.  A pipelined sweep on a handle that is also driven through the split
// API is recorded: the next frame's set_transforms / prepare on another stream wait for the sweeps that still read what they rewrite.
static int df_launch_prepared(DfWarpField* wf, DfPrepared& P, void* vol, unsigned long long* n_updated, hipStream_t st)
{
    P.a.vol = (uint32_t*)vol; P.a.n_upd = n_updated;
#ifdef DF_TRACE_WG
    static unsigned long long* trace_dev = nullptr; static size_t trace_cap = 0;
    const size_t trace_n = (size_t)P.grid.x * (P.threads / 64u) * 4;
    if (P.a.plan_mask && trace_n > trace_cap) { (void)hipFree(trace_dev); DF_HIP(hipMalloc((void**)&trace_dev, trace_n * 8)); trace_cap = trace_n; }
    if (P.a.plan_mask) { DF_HIP(hipMemsetAsync(trace_dev, 0, trace_n * 8, st)); P.a.trace = trace_dev; }
#endif
    P.kern<<<P.grid, dim3(P.threads), P.lds, st>>>(P.a, P.W, P.tiles_x);
    DF_LAUNCH_CHECK();
#ifdef DF_TRACE_WG
    if (P.a.plan_mask && getenv("DF_TRACE_FILE")) {
        DF_HIP(hipStreamSynchronize(st));
        unsigned long long* h = (unsigned long long*)malloc(trace_n * 8);
        DF_HIP(hipMemcpy(h, trace_dev, trace_n * 8, hipMemcpyDeviceToHost));
        FILE* f = fopen(getenv("DF_TRACE_FILE"), "wb");
        if (f) { unsigned long long hdr[4] = {P.grid.x, 1, (unsigned long long)(P.threads / 64u), 0}; fwrite(hdr, 8, 4, f); fwrite(h, 8, trace_n, f); fclose(f); }
        free(h);
    }
#endif
    if (P.a.plan_mask && wf->split_events) {
        DF_HIP(hipEventRecord(wf->ev_sweep_done[P.seq & 1], st));
        wf->recorded_seq = P.seq; wf->ring_seq[P.seq & 1] = P.seq;
    }
    return DF_OK;
}

extern "C" int dfusion_integrate_warped(const uint16_t* dists, size_t pitch, int cols, int rows, DfVolume v, const DfSlab* slab,
                                        const float vol2world[12], const float world2cam[12], const float proj[4],
                                        DfWarpField* wf, int k, unsigned flags, unsigned long long* n_updated, dfStream stream)
{
    DfSlab s;
    DF_TRY(df_warped_check(dists, pitch, cols, rows, v, slab, vol2world, world2cam, proj, wf, k, &s));
    if (s.z_own_n == 0) return DF_OK;
    hipStream_t st = (hipStream_t)stream;
    DF_TRY(df_wait_split_sweep(wf, st));                      // (sweeps issued through the split API on another stream: all of them)
    DfPrepared P;
    DF_TRY(df_integrate_warped_impl(dists, pitch, cols, rows, v, s, vol2world, world2cam, proj, wf, k, flags, st, false, P));
    if (P.kern) return df_launch_prepared(wf, P, v.data, n_updated, st);
    DfWarpedArgs& a = P.a;                                    // the two variants without a launch plan: table rows, bricks
    const int zt_lo = s.z_own0 / DF_ROW_TZ, zt_hi = (s.z_own0 + s.z_own_n - 1) / DF_ROW_TZ;      // (DF_ROW_TZ == DF_BRICK)
    a.vol = (uint32_t*)v.data; a.n_upd = n_updated; a.bz0 = zt_lo;
    if (a.knn_tab) {
        DF_TRY(df_tables_complete(wf, st));
        dim3 grid((unsigned)(P.tiles_x * ((a.Y + DF_ROW_TY - 1) / DF_ROW_TY)), (unsigned)(zt_hi - zt_lo + 1));
        if (a.w_tab) { DF_DISPATCH_K(k, df_warp_rows_kernel<K, true, 4><<<grid, dim3(256), 0, st>>>(a, P.W, P.tiles_x)); }
        else { DF_DISPATCH_K(k, df_warp_rows_kernel<K, false, 4><<<grid, dim3(256), 0, st>>>(a, P.W, P.tiles_x)); }
    } else {
        dim3 grid((unsigned)(P.W.bx * P.W.by), (unsigned)(zt_hi - zt_lo + 1));
        DF_DISPATCH_K(k, df_warp_brick_kernel<K, false><<<grid, dim3(256), 0, st>>>(a, P.W));
    }
    DF_LAUNCH_CHECK();
    return DF_OK;
}

// ---- the frame's warped integrate in two calls (include/dfusion.h), which may be issued on different streams: the handle's events order
// them.  (A prepare waits only for the sweeps that still read what it rewrites: the plan sets of df_pipe_plan, the node arrays of df_warp_pack.)
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
    DfSlab s;
    DF_TRY(df_warped_check(dists, pitch, cols, rows, geometry, slab, vol2world, world2cam, proj, wf, k, &s));
    if (s.z_own_n != 0) {
        if (!wf->prep) wf->prep.reset(new DfPrepared());
        DF_TRY(df_integrate_warped_impl(dists, pitch, cols, rows, geometry, s, vol2world, world2cam, proj, wf, k, flags, (hipStream_t)stream, true, *wf->prep));
        wf->prep_valid = true;
    }
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
    return df_launch_prepared(wf, *P, v.data, n_updated, st);
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
    DF_TRY(wf->blk.reserve(nblk));
    DF_TRY(wf->blk_cnt.reserve(16));
    DF_HIP(hipMemsetAsync(wf->blk_cnt, 0, 16 * sizeof(uint32_t), st));
    DF_HIP(hipMemsetAsync(wf->blk.state, on_demand ? 0 : 1, nblk, st));
    DF_HIP(hipMemsetAsync(wf->blk.tie, 0, nblk, st));
    DF_HIP(hipMemsetAsync(wf->blk.wmax, 0, nblk * sizeof(float), st));
    DF_HIP(hipMemsetAsync(wf->blk.alive, 1, nblk, st));                   // (no verdicts yet: "every neighbour kept" for the first pass's sub-verdict list)
    DF_HIP(hipMemsetAsync(wf->blk.alive_prev, 1, nblk, st));
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
