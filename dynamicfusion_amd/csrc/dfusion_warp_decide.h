// dfusion_warp_decide.h -- the two host decisions of the warped integrate (dfusion_warp.hip) as pure functions of plain values: which sweep
// a call takes and with what launch shape (df_warp_variant), and where the verdict pass's optional work runs (df_verdict_policy).
// No HIP types: compiled for the host by tests/cxx/warp_decide_test.cpp, which pins both against written-out tables.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "dfusion.h"

// Look-ahead margin of the verdict pass (metres): blocks that would be alive with every cull radius widened by this much get their tables /
// blend models made on the handle's side stream before a sweep needs them.  A camera turning 0.25 degrees per frame moves a voxel 2 m from
// its axis by 9 mm, the benchmark's warp amplitude moves the cull radii by up to 2 cm per frame: 5 cm is two to five frames of lead.
#define DF_WARP_PREFETCH_MARGIN_M 0.05f
#define DF_DECIDE_PIPE_WGT 256        // == DF_PIPE_WGT, DF_LDS_ZT of dfusion_warp_sweep.h (dfusion_warp.hip asserts it)
#define DF_DECIDE_LDS_ZT 8

enum DfSweepKind {
    DF_SWEEP_BRICKS,                  // df_warp_brick_kernel: ranks the brick's candidates per voxel, no tables
    DF_SWEEP_TABLE_ROWS,              // df_warp_rows_kernel: tables, node transforms gathered from global memory
    DF_SWEEP_LDS_ROWS,                // df_warp_rows_lds_kernel: tables, the node table (32 B a node) in LDS, batched loads
    DF_SWEEP_PIPELINED                // df_warp_rows_pipe_kernel: the product path (k = 8, 4), with verdicts and a launch plan
};
struct DfWarpVariant {
    DfSweepKind kind;
    bool weights;                     // the weight tables are read (kinds with tables)
    unsigned threads; size_t lds;     // the last two kinds (0 for the others): workgroup size, dynamic LDS bytes,
    bool k4_table, wide;              // pipelined k = 4 keeps the LDS node table / runs it with 1024 threads,
    int zt;                           // tile layers walked per workgroup
};
// `tables_cover`: the handle's tables were built for this k and cover the slab's own planes.  `dims01` = dims[0] * dims[1];
// `cols_layers` = the tile columns of a layer times the slab's tile layers.  lds <= lds_limit in every result (lds_limit >= 16 KiB).
static inline DfWarpVariant df_warp_variant(int k, int M, unsigned flags, bool tables_cover, bool weight_tables, unsigned long long pitch, long long rows,
                                            unsigned long long dims01, size_t lds_limit, long long cols_layers)
{
    DfWarpVariant d = {DF_SWEEP_BRICKS, false, 0u, 0, false, false, 0};
    if (!tables_cover || (flags & DF_WARP_NO_TABLE)) return d;
    d.weights = weight_tables && !(flags & DF_WARP_NO_WEIGHT_TABLE);
    d.kind = DF_SWEEP_TABLE_ROWS;
    if (flags & DF_WARP_NO_LDS) return d;
    const size_t table = (size_t)M * 32;                             // the LDS node table
    // The pipelined kernel forms row * pitch with a 24-bit multiply and a 32-bit dists offset.  It needs no LDS node table: k = 8 blends
    // out of per-wave union copies (4 KiB a wave) or gathers from the L2, for ANY node count; k = 4 keeps the table where it fits.
    if (d.weights && !(flags & DF_WARP_NO_PIPELINE) && (k == 8 || k == 4) && pitch < (1ull << 24) && rows < (1ll << 24) &&
        (unsigned long long)rows * pitch < (1ull << 32) && dims01 < (1ull << 30)) {
        d.kind = DF_SWEEP_PIPELINED;
        d.k4_table = k == 4 && table <= lds_limit;
        d.wide = d.k4_table && table > 80 * 1024;                    // one workgroup per CU either way: make it 1024 threads
        d.threads = k == 8 ? (unsigned)DF_DECIDE_PIPE_WGT : d.wide ? 1024u : 512u;
        d.lds = k == 8 ? (size_t)(DF_DECIDE_PIPE_WGT / 64) * 4096 : d.k4_table ? table : 0;
        // long walks amortise the LDS fill and the pipeline ramp, short ones even out the last round of workgroups on the 256 CUs
        // (measured: 4 layers best at 256^3 = 1024 workgroups, 8 at 512^3, 16 at 1024^3 = 16384)
        d.zt = cols_layers <= 8192 ? 4 : cols_layers <= 65536 ? 8 : 16;
    } else if (table <= lds_limit) {
        d.kind = DF_SWEEP_LDS_ROWS;
        d.threads = 512u; d.lds = table; d.zt = DF_DECIDE_LDS_ZT;
    }
    return d;
}

// Where the verdict pass's optional work -- look-ahead table builds, blend models -- runs this frame.
struct DfVerdictPolicy {
    bool use_models;                  // the sweep reads block models (k = 8, 4, not switched off)
    int want_models, want_models_now; // models are made: 0 no, 1 from the second sweep over the tables on, 2 from the first; _now: 0 on a quiet frame
    bool ahead, quiet;                // look-ahead work goes to the side stream / a frame at rest: optional work waits for the next probe
    float pf_margin;                  // the verdict pass's look-ahead margin (0: lists nothing ahead)
    bool side_work;                   // the side stream gets work: fork and join
};
// `report` = the last plan kernel's list lengths as the host sees them (urgent builds, models, look-ahead builds).
// The side stream costs a fork and a join (~13 us of barrier packets per frame): worth it while blocks are being built or modelled, not
// on a scene at rest.  On from the first sweeps over new tables, while the last report listed anything, and every 8th sweep as a probe
// (a camera that starts to move is picked up by the urgent list at once, by the look-ahead within the report's age).
// DF_WARP_STEADY_PREFETCH keeps it on in every frame; DF_WARP_BLOCK_MODEL_NOW keeps everything on the launch stream, in order.
static inline DfVerdictPolicy df_verdict_policy(unsigned flags, int k, int tab_sweeps, bool tab_complete, const uint32_t report[3])
{
    DfVerdictPolicy p;
    p.use_models = !(flags & DF_WARP_NO_BLOCK_MODEL) && (k == 8 || k == 4);
    p.want_models = !p.use_models ? 0 : (flags & DF_WARP_BLOCK_MODEL_NOW) ? 2 : tab_sweeps >= 1 ? 1 : 0;
    const bool may_ahead = !(flags & (DF_WARP_NO_PREFETCH | DF_WARP_BLOCK_MODEL_NOW));
    const bool at_rest = !(flags & DF_WARP_STEADY_PREFETCH) && tab_sweeps >= 8 && (tab_sweeps & 7) != 0 && report[0] == 0u && report[1] == 0u &&
                         report[2] == 0u;
    p.ahead = may_ahead && !at_rest;
    p.quiet = may_ahead && at_rest;
    p.want_models_now = p.quiet ? 0 : p.want_models;
    // (no margin on the very first sweep over new tables: the urgent build of the whole alive set is the frame then, and a node set that
    // changes every frame never pays for look-ahead work)
    p.pf_margin = p.ahead && !tab_complete && tab_sweeps >= 1 ? DF_WARP_PREFETCH_MARGIN_M : 0.f;
    p.side_work = p.ahead && (!tab_complete || p.want_models_now != 0);
    return p;
}
