// dfusion_internal.h -- host-side internals shared by the .hip translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <memory>
#include <utility>
#include "dfusion.h"
#include "dfusion_device.h"
#include "dfusion_nanoflann.h"

#define DF_BRICK 8                    // k-NN index brick edge (voxels)
#define DF_WARP_PREFETCH_CAP 1024u    // look-ahead table builds per frame at most: about one round of the resident build grid (50-80 us beside the sweep)
#define DF_REPORT_NONE 1u             // the host report words before any plan kernel has reported: assume work (df_side_init, df_block_verdicts)

#define DF_HIP(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) return (int)e__; } while (0)
#define DF_LAUNCH_CHECK() do { hipError_t e__ = hipGetLastError(); if (e__ != hipSuccess) return (int)e__; } while (0)
#define DF_TRY(expr) do { int rc__ = (expr); if (rc__) return rc__; } while (0)      // a DF_* / HIP code from one of the library's own functions

static inline DfSlab df_slab_or_full(const DfVolume& v, const DfSlab* s)
{
    if (s) return *s;
    DfSlab f; f.z_store0 = 0; f.z_store_n = v.dims[2]; f.z_own0 = 0; f.z_own_n = v.dims[2]; return f;
}
static inline bool df_slab_valid(const DfVolume& v, const DfSlab& s)
{
    return s.z_store_n > 0 && s.z_own_n >= 0 && s.z_store0 >= 0 && s.z_store0 + s.z_store_n <= v.dims[2] &&
           s.z_own0 >= s.z_store0 && s.z_own0 + s.z_own_n <= s.z_store0 + s.z_store_n;
}
static inline bool df_volume_valid(const DfVolume& v)
{
    return v.data && v.dims[0] > 0 && v.dims[1] > 0 && v.dims[2] > 0 && (v.dims[0] % 4) == 0 &&
           v.voxel_size[0] > 0 && v.voxel_size[1] > 0 && v.voxel_size[2] > 0 && v.trunc_dist > 0;
}
static inline DfAff df_aff(const float a[12]) { DfAff r; memcpy(r.R, a, 36); memcpy(r.t, a + 9, 12); return r; }
// an image row of `cols` pixels of `bpp` bytes fits its byte pitch (include/dfusion.h Conventions); cols <= 0 never fits
static inline bool df_pitch_ok(size_t pitch, int cols, size_t bpp) { return cols > 0 && pitch >= (size_t)cols * bpp; }

// Device-side view of the warp field + brick index (passed to kernels by value).
struct DfWarpView {
    const float4* pos_sigma;   // [M] xyz = vertex, w = dg_w
    const float4* rot;         // [M] rotation_ (w,x,y,z)
    const float4* dual;        // [M] translation_ (w,x,y,z)
    const float4* node_t;      // [M] getTranslation() of the node (w,x,y,z), dual_quaternion.hpp:120-125
    const float4* rt;          // [2M] rot_j, node_t_j interleaved (32 bytes a node: what the sweep's union refills and uncoded cells gather)
    int M;
    // brick index
    const uint32_t* brick_off; // [nb+1]
    const uint16_t* brick_list;
    const float* brick_thr;    // [nb] list radius: nodes outside brick b's list are farther than this from its centre
    int bx, by, bz;            // brick grid over the GLOBAL volume
    DfNfView nf;               // nanoflann's tree over the nodes: orders exactly equidistant nodes (dfusion_nanoflann.h)
};

// A device allocation the handle owns: pointer and capacity (in elements) change together, and the memory is freed exactly once.
// reserve() frees FIRST (the old and the new buffer never exist together) and then allocates exactly n elements: no headroom, no copy of
// the old contents, no zeroing and no synchronisation -- a caller that needs one of those does it itself.  Reads as a T*.
template <typename T>
struct DfDevBuf {
    T* p = nullptr; size_t cap = 0;
    DfDevBuf() = default;
    DfDevBuf(DfDevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DfDevBuf& operator=(DfDevBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~DfDevBuf() { (void)hipFree(p); }
    operator T*() const { return p; }
    void release() { (void)hipFree(p); p = nullptr; cap = 0; }
    int reserve(size_t n)                      // DF_OK or the HIP error; null / 0 after a failure
    {
        if (n <= cap) return DF_OK;
        release();
        DF_HIP(hipMalloc((void**)&p, n * sizeof(T)));
        cap = n;
        return DF_OK;
    }
};

// The per-block buffers of the warped sweep's verdict pass, in the three groups they are reserved in.  reserve(nblk) zeroes the group's
// capacity first and sets it last, so cap > 0 says that EVERY buffer of the group holds cap blocks; a failure part-way leaves cap == 0
// and the next reserve makes all of them again.  Nothing else frees or shrinks them: ready(n) stands for "n <= cap and
// no pointer of the group is null".
struct DfBlockState {          // with the tables (df_build_voxel_table)
    DfDevBuf<uint8_t> state;   // 0 = tables not built (DF_INDEX_TABLES_ON_DEMAND), 1 = built, 2 = built and a blend-model record written
    DfDevBuf<uint8_t> tie;     // 1 = the block's table build met two exactly equidistant candidates (topk_insert's tie branch): its table
                               // depends on the tie tree, and a rebuilt tree (dfusion_warp_extend) may reorder them anywhere
    DfDevBuf<float> wmax;      // max over the block's voxels of the weight sum (0 until built)
    DfDevBuf<uint8_t> alive, alive_prev;   // this frame's verdicts and those of the pass before (every pass swaps the two)
    DfDevBuf<uint32_t> work;   // [3][cap] the frame's urgent-build / look-ahead-build / model work lists
    size_t cap = 0;
    bool ready(size_t n) const { return n <= cap; }
    int reserve(size_t n)
    {
        if (ready(n)) return DF_OK;
        cap = 0;
        DF_TRY(state.reserve(n)); DF_TRY(tie.reserve(n)); DF_TRY(wmax.reserve(n)); DF_TRY(alive.reserve(n)); DF_TRY(alive_prev.reserve(n));
        DF_TRY(work.reserve(3 * n));
        cap = n; return DF_OK;
    }
};
#define DF_BM_NU 16                   // entries per block model (dfusion_warp_blocks.h defines the same)
struct DfBlockModels {         // block blend models, with the first model: entry-major [DF_BM_NU][cap] node ids, {mid, half width} half
    DfDevBuf<uint16_t> idx; DfDevBuf<uint32_t> lam, w; DfDevBuf<uint8_t> cnt;   // pairs of the normalised and of the raw weights, entry counts
    size_t cap = 0;
    bool ready(size_t n) const { return n <= cap; }
    int reserve(size_t n)
    {
        if (ready(n)) return DF_OK;
        cap = 0;
        DF_TRY(idx.reserve(n * DF_BM_NU)); DF_TRY(lam.reserve(n * DF_BM_NU)); DF_TRY(w.reserve(n * DF_BM_NU)); DF_TRY(cnt.reserve(n));
        cap = n; return DF_OK;
    }
};
// 4-bit neighbour codes (k = 8), per 4 x 4 x 4 SUB-block so that they exist at any node density: per voxel of a block the model pass has
// visited, its k neighbours as positions in the union list of its sub-block (ascending node ids, <= 16).  With them, because the same pass
// writes them, the sub-blocks' own blend models and this frame's sub-verdicts.
struct DfBlockCodes {
    DfDevBuf<uint32_t> ids;    // [block][64] entry q * 16 + e = union entry e of column quadrant q (x >> 2 & 1 | (y >> 2 & 1) << 1), low half word for
                               // planes 0-3 of the block, high half word for planes 4-7 -- the dword a sweep lane loads to refill its wave's copies
    DfDevBuf<uint32_t> tab;    // one u32 per voxel, tile-major like the tables but PATCH-major inside a tile plane
    DfDevBuf<uint8_t> coded;   // [block] 1 = every sub-block's union fits 16 entries and the codes are written
    DfDevBuf<uint32_t> sub_lam, sub_w;   // [block][DF_BM_NU][sub] the intervals of a sub-block's union entries over its 64 voxels (sub = 4 h + q)
    DfDevBuf<uint16_t> sub_cnt;          // [block * 8 + sub] entries | reference entry << 8
    DfDevBuf<uint8_t> sub_ok;            // [block] 1 = the block has sub-block models
    DfDevBuf<uint8_t> blk_sub;           // [block] bit 4 h + q = the sub-block may update this frame (0xff where not judged)
    DfDevBuf<uint32_t> sub_list;         // the blocks to judge
    size_t cap = 0;
    bool ready(size_t n) const { return n <= cap; }
    int reserve(size_t n, hipStream_t st)      // coded and sub_ok zeroed on `st`
    {
        if (ready(n)) return DF_OK;
        cap = 0;
        DF_TRY(ids.reserve(n * 64)); DF_TRY(tab.reserve(n * 512)); DF_TRY(coded.reserve(n));
        DF_HIP(hipMemsetAsync(coded, 0, n, st));
        DF_TRY(sub_lam.reserve(n * 8 * DF_BM_NU)); DF_TRY(sub_w.reserve(n * 8 * DF_BM_NU)); DF_TRY(sub_cnt.reserve(n * 8)); DF_TRY(sub_ok.reserve(n));
        DF_TRY(blk_sub.reserve(n)); DF_TRY(sub_list.reserve(n));
        DF_HIP(hipMemsetAsync(sub_ok, 0, n, st));
        cap = n; return DF_OK;
    }
};

struct DfPrepared;                             // (dfusion_warp.hip)
#define DF_GRAPH_MAX_LEVELS 8                  // levels of the hierarchical node graph at most (dfusion_warp_graph.hip)

struct __attribute__((visibility("hidden"))) DfWarpField {     // (opaque in dfusion.h: the library exports none of its members)
    DfWarpField(); ~DfWarpField();             // (dfusion_warp.hip, where DfPrepared is complete)
    int device = 0;
    int M = 0, cap = 0;
    DfDevBuf<float4> pos_sigma, rot, dual, node_t;
    // index
    DfDevBuf<uint32_t> brick_off, brick_cnt; DfDevBuf<uint16_t> brick_list; DfDevBuf<float> brick_thr;
    size_t off_cap = 0;
    DfDevBuf<uint32_t> scan_tmp; size_t scan_cap = 0;       // tile sums / tile offsets of the brick-count scan
    int bx = 0, by = 0, bz = 0, k_built = 0;
    int geom_dims[3] = {}; float geom_vs[3] = {}; float geom_aff[12] = {};
    float geom_inv[12] = {}; bool geom_inv_ok = false;      // world -> volume (locates the brick of a query point)
    bool index_valid = false;
    unsigned index_flags = 0; DfSlab index_slab = {};   // what the last dfusion_warp_build_index was given (dfusion_warp_extend rebuilds with them)
    // per-voxel k-NN table (optional, DF_INDEX_VOXEL_TABLE)
    DfDevBuf<uint16_t> knn_tab;
    int tab_z0 = 0, tab_zn = 0, tab_k = 0; bool tab_valid = false;
    DfDevBuf<float> w_tab; bool w_tab_valid = false;   // per-voxel blend weights (optional, DF_INDEX_WEIGHT_TABLE)
    DfDevBuf<float> tile_wmax;                          // per table tile: max over its voxels of the weight sum (with w_tab)
    // device scalars for the conservative brick cull: [0] max |t_i|, [1] max sin(theta_i/2), [2] max dists
    DfDevBuf<float> bounds_dev;
    int max_phase = 0;                // which of bounds_dev[6], [7] this frame's capped pyramid leaves the image-wide maximum in
    // dfusion_integrate_warped_prepare / _sweep: the planned launch a prepare call leaves for the sweep call (opaque here: the argument
    // structs live in dfusion_warp_sweep.h), and the events that order the halves when they are issued on different streams
    std::unique_ptr<DfPrepared> prep; bool prep_valid = false;
    hipEvent_t ev_prep_done = nullptr, ev_sweep_done[2] = {}; bool split_events = false;
    // What a sweep issued through the split API may still be READING when the next frame's set_transforms / prepare arrive on another
    // stream is double-buffered, so that they can run BESIDE that sweep instead of after it: the node transform arrays (rot / dual / node_t
    // and their alternates), the launch plan (two sets of mask + bins; FOUR counter sets, zeroed two frames ahead).  Sweeps are numbered;
    // a buffer remembers the last sweep that reads it, the ring of two events holds the last two sweeps (all sweeps on one stream).
    DfDevBuf<float4> rot_alt, dual_alt, node_t_alt;
    DfDevBuf<float4> rt, rt_alt;                     // {rot, node_t} interleaved, and its alternate (see DfWarpView)
    unsigned long long seq = 0, recorded_seq = 0;    // sweeps prepared / recorded so far
    unsigned long long ring_seq[2] = {};             // the sweep whose completion ev_sweep_done[i] stands for (0: none)
    unsigned long long node_reader[2] = {}; int nphase = 0;  // [nphase] = the current node set's last reader, [nphase ^ 1] = the alternate's
    unsigned long long plan_reader[2] = {};
    DfDevBuf<unsigned long long> plan_mask2[2]; DfDevBuf<unsigned int> plan_list2[2]; int pphase = 0; unsigned hphase = 0;   // (masks: two words per item, a bit per half layer)
    DfDevBuf<unsigned long long> plan_code2[2];      // per strip item: which of its (patch, layer) cells read 4-bit codes
    DfDevBuf<uint16_t> pyr_mem;             // max-pyramid of the frame's dists image (warped sweep's depth cull), entries
    // scratch of the warp solver (dfusion_solver.hip: one carve-up for its three entry points; grown on demand)
    DfDevBuf<char> solver_ws;
    // node graph of the regularised solve (dfusion_solver.hip): node i's graph_kg nearest other nodes nbr[M * kg], the edge weights
    // alpha[M * kg], the incoming edges of every node (CSR: in_off[M + 1] into in_edge, ascending edge ids) and the build's scratch.
    // graph_kg = 0: none -- dfusion_warp_set_nodes and an extend that adds nodes drop it, the next regularised solve rebuilds it
    DfDevBuf<int> graph_nbr; DfDevBuf<float> graph_alpha; DfDevBuf<unsigned int> graph_in_off, graph_in_edge; DfDevBuf<char> graph_ws;
    int graph_kg = 0;
    // the hierarchical form of that graph (dfusion_warp_graph.hip; dfusion_warp_set_graph_hierarchy): the setting -- hier_levels = 0: the
    // flat graph -- which outlives the graph, and with the graph the highest level of every node top[M], the level sizes |S_0..S_8| and
    // the effective depth L' (0: the graph held is the flat one)
    int hier_levels = 0; float hier_radius = 0.f, hier_beta = 0.f;
    DfDevBuf<int> graph_top; DfDevBuf<char> graph_hws;
    int graph_sizes[DF_GRAPH_MAX_LEVELS + 1] = {}; int graph_eff = 0;
    // dfusion_warp_set_preconditioner: 0 = none, 1 = 6x6 node blocks; read by dfusion_warp_solve_rigid alone (dfusion_solver.hip)
    int precond = 0;
    // points an indexed k-NN / warp pass left to the scan kernel: [0] count, [1..] ids
    DfDevBuf<int> pt_ids;
    int pt_image_cols = 0;                             // dfusion_warp_set_point_tiling: 0 = point queries in linear order
    // replica of the reference's nanoflann tree over the node positions (rebuilt by dfusion_warp_set_nodes)
    DfDevBuf<DfNfNode> nf_nodes; DfDevBuf<uint16_t> nf_vpos; bool nf_ok = false; int nf_depth = 0;
    // pipelined warped sweep: the launch plan (verdict masks of the strip items, the alive ones sorted by work), dfusion_warp.hip
    DfDevBuf<unsigned int> plan_hist; size_t plan_cap = 0;
    // per 8x8x8 block of the table planes (dfusion_warp_blocks.h; block grid over whole table tiles x tab_zn / 8), in three groups that
    // are reserved -- and, when a reservation fails, voided -- together (above)
    DfBlockState blk; DfBlockModels bm; DfBlockCodes codes;
    DfDevBuf<uint32_t> blk_cnt; int blk_phase = 0;   // [2 sets][8] the work lists' lengths and the build passes' cursors (the sets alternate between passes: each pass zeroes the other one)
    bool tab_complete = false;   // every block's tables are built
    int tab_sweeps = 0;          // sweeps over the current tables so far (the models are made from the second one on)
    unsigned long long* dbg_swept = nullptr;   // dfusion_warp_debug_counters: nullable device counter (the caller's) the sweeps through this handle add to
    bool alive_valid = false;    // blk.alive holds the verdicts of a sweep over the current tables (dfusion_warp_alive_blocks)
    // look-ahead work (tables / models of blocks a sweep does not need yet) runs on a side stream the handle owns, beside the sweep on
    // the caller's stream: ev_fork (caller's stream, after the verdict pass) releases it, ev_join (side stream, after its last kernel)
    // is waited for by the next call that touches the tables
    hipStream_t side = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr; bool side_pending = false;
    // the verdict pass's list lengths, reported to pinned host memory by the plan kernel ([0] urgent builds, [1] models, [2] look-ahead
    // builds, [3] sweep number): read WITHOUT synchronisation by a later call -- a hint whether on-demand work is going on (then the side
    // stream is worth its fork / join, ~13 us per frame), never a condition of correctness
    volatile uint32_t* host_report = nullptr;
    DfDevBuf<char> ext_ws;             // scratch of dfusion_warp_extend (grown on demand)
    DfDevBuf<char> grow_ws;            // df_warp_grow: the brick lists before the update (grown on demand)
};

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

// Host helpers of the warp field that one dfusion_warp*.hip translation unit defines and another calls (the library exports none of them).
struct DfWarpedArgs;                           // (dfusion_warp_sweep.h)
#define DF_LOCAL __attribute__((visibility("hidden")))
// dfusion_warp_nodes.hip
DF_LOCAL DfWarpView df_view(const DfWarpField* wf);
DF_LOCAL int df_side_init(DfWarpField* wf);
DF_LOCAL int df_side_join(DfWarpField* wf, hipStream_t st);
DF_LOCAL void df_side_drain(DfWarpField* wf);
DF_LOCAL int df_wait_split_sweep(DfWarpField* wf, hipStream_t st);
DF_LOCAL int df_wait_reader(DfWarpField* wf, unsigned long long reader, hipStream_t st);
DF_LOCAL int df_wait_all_sweeps_host(DfWarpField* wf);
DF_LOCAL int df_warp_reserve(DfWarpField* wf, int M);
DF_LOCAL int df_warp_pack_current(DfWarpField* wf, const float* pos, const float* dq, const float* sigma, hipStream_t st);
DF_LOCAL int df_warp_build_tie_tree(DfWarpField* wf, hipStream_t st);
// dfusion_warp_index.hip
DF_LOCAL int df_index_bricks(DfWarpField* wf, const DfVolume& v, const float vol2world[12], int k, hipStream_t st);
// dfusion_warp_graph.hip
DF_LOCAL int df_hg_build(DfWarpField* wf, int kg, unsigned int* keys, unsigned int* vals, hipStream_t st);
// dfusion_warp.hip
DF_LOCAL DfWarpedArgs df_table_args(const DfWarpField* wf);
DF_LOCAL int df_tables_complete(DfWarpField* wf, hipStream_t st);
DF_LOCAL int df_build_voxel_table(DfWarpField* wf, const DfVolume& v, const DfSlab& s, const float vol2world[12], int k, bool weights,
                                  bool on_demand, hipStream_t st);

// The scratch buffer the library keeps per (device, stream) until dfusion_release_scratch() (dfusion_volume.hip; the rigid integrate's
// plan and the mesh extraction's workspace: calls on one stream are ordered, so they can share it).  df_scratch_acquire returns the
// entry of (current device, st), LOCKED, and at least `bytes` of device memory in *mem_out, or nullptr when that cannot be allocated;
// df_scratch_release unlocks it, once the call's last launch that uses the memory is enqueued.  DfScratchHold does both.
struct DfScratchEntry;
DF_LOCAL DfScratchEntry* df_scratch_acquire(hipStream_t st, size_t bytes, char** mem_out);
DF_LOCAL void df_scratch_release(DfScratchEntry* entry);
struct DfScratchHold {
    char* mem = nullptr; DfScratchEntry* entry;                 // entry == nullptr: out of memory
    DfScratchHold(hipStream_t st, size_t bytes) : entry(df_scratch_acquire(st, bytes, &mem)) {}
    ~DfScratchHold() { if (entry) df_scratch_release(entry); }
    DfScratchHold(const DfScratchHold&) = delete; DfScratchHold& operator=(const DfScratchHold&) = delete;
};

// Appends to the node set without dropping what still holds (dfusion_warp_index.hip; used by dfusion_warp_extend): the handle takes the grown
// set pos/dq/sigma[Mn] (layout of dfusion_warp_set_nodes; the first M entries are the current nodes), and an index is brought up to date
// for it in place -- the brick lists are re-made, and only the table blocks whose brick list changed or whose build met an exact
// distance tie are marked unbuilt.  Blocks until done.
int df_warp_grow(DfWarpField* wf, const float* pos, const float* dq, const float* sigma, int Mn, hipStream_t st);

// WarpField::weighting (warp_field.cpp:238-241) per neighbour, and WarpField::DQB (:203-217) from the k weights + node indices, then
// the DualQuaternion ctor (dual_quaternion.hpp:59-63): what dfusion_warp_points and dfusion_warp_extend blend with
template <int K>
__device__ __forceinline__ void dqb_weights(const DfWarpView& W, const float (&bd)[K], const int (&bi)[K], float (&wt)[K])
{
#pragma unroll
    for (int i = 0; i < K; ++i) wt[i] = dqb_weight(bd[i], W.pos_sigma[bi[i]].w);
}
template <int K>
__device__ __forceinline__ void dqb_blend_w(const DfWarpView& W, const float (&wt)[K], const int (&bi)[K], quat* rot_out,
                                            quat* dual_out)
{
    quat tsum, rsum;
    tsum.w = tsum.x = tsum.y = tsum.z = 0.f;
    rsum.w = rsum.x = rsum.y = rsum.z = 0.f;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const int j = bi[i];
        const float w = wt[i];
        const float4 t4 = W.node_t[j], r4 = W.rot[j];
        quat t, r;
        t.w = t4.x; t.x = t4.y; t.y = t4.z; t.z = t4.w;
        r.w = r4.x; r.x = r4.y; r.y = r4.z; r.z = r4.w;
        tsum = q_add(tsum, q_scale(w, t));            // :211
        rsum = q_add(rsum, q_scale(w, r));            // :212
    }
    rsum = q_normalize(rsum);                         // :214
    quat half;
    half.w = 0.5f * tsum.w; half.x = 0.5f * tsum.x; half.y = 0.5f * tsum.y; half.z = 0.5f * tsum.z;
    *rot_out = rsum;
    *dual_out = q_mul(half, rsum);                    // dual_quaternion.hpp:59-63
}
