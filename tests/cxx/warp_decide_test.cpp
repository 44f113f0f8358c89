// Stand-alone check of dynamicfusion_amd/csrc/dfusion_warp_decide.h, the two host decisions of the warped integrate.  Each is pinned twice:
// against rows written out by hand, and -- over every combination of the inputs' edge values -- against an independent specification,
// variant_rules and policy_rules below: the same rules stated as separate predicates (use_tab, use_w, lds_fits, pipe_sweep ...) and as a
// statement sequence, not derived from the header.  Built and run by tests/test_warp_decide.py.
#include <stdio.h>
#include <stdint.h>
#include "dfusion_warp_decide.h"

#define KiB 1024ull
#define CHECK(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)

struct Want { int kind; bool weights; unsigned threads; size_t lds; bool k4_table, wide; int zt; };

// ---- the variant: the specification
static Want variant_rules(int k, int M, unsigned flags, bool tables, bool wtables, unsigned long long pitch, long long rows, unsigned long long dims01,
                          size_t lds_limit, long long cols_layers)
{
    const bool use_tab = tables && !(flags & DF_WARP_NO_TABLE);
    const bool use_w = use_tab && wtables && !(flags & DF_WARP_NO_WEIGHT_TABLE);
    const bool no_lds = (flags & DF_WARP_NO_LDS) != 0;
    const bool lds_fits = (size_t)M * 32 <= lds_limit;
    const bool pipe_form_ok = use_w && !(flags & DF_WARP_NO_PIPELINE) && pitch < (1u << 24) && rows < (1 << 24) &&
                              (unsigned long long)rows * pitch < (1ull << 32) && dims01 < (1ull << 30);
    const bool pipe_sweep = use_tab && !no_lds && pipe_form_ok && (k == 8 || k == 4);
    Want w = {DF_SWEEP_BRICKS, use_w, 0u, 0, false, false, 0};
    if (use_tab && !no_lds && (pipe_sweep || lds_fits)) {
        const bool k4_table = pipe_sweep && k == 4 && lds_fits;
        const size_t lds = !pipe_sweep || k4_table ? (size_t)M * 32 : k == 8 ? (size_t)(256 / 64) * 4096 : 0;
        w.zt = !pipe_sweep ? 8 : cols_layers <= 8192 ? 4 : cols_layers <= 65536 ? 8 : 16;
        const bool wide = k4_table && lds > 80 * 1024;
        unsigned wg_threads = 512u;
        if (pipe_sweep && k == 8) wg_threads = 256u;
        else if (pipe_sweep && k4_table) wg_threads = wide ? 1024u : 512u;
        w.kind = pipe_sweep ? DF_SWEEP_PIPELINED : DF_SWEEP_LDS_ROWS;
        w.threads = wg_threads; w.lds = lds; w.k4_table = k4_table; w.wide = wide;
    } else if (use_tab) {
        w.kind = DF_SWEEP_TABLE_ROWS;
    }
    return w;
}

static int same(const DfWarpVariant& d, const Want& w)
{
    return (int)d.kind == w.kind && d.weights == w.weights && d.threads == w.threads && d.lds == w.lds && d.k4_table == w.k4_table && d.wide == w.wide &&
           d.zt == w.zt;
}

static int check_variant(long* n_out)
{
    const unsigned NT = DF_WARP_NO_TABLE, NW = DF_WARP_NO_WEIGHT_TABLE, NL = DF_WARP_NO_LDS, NP = DF_WARP_NO_PIPELINE;
    const size_t L = 160 * KiB;
    // hand-written rows: {k, M, flags, tables, weight tables, pitch, rows, dims01, lds limit, cols_layers} -> {kind, weights, threads, lds, k4_table, wide, zt}
    struct Row { int k, M; unsigned flags; bool tables, wtables; unsigned long long pitch; long long rows; unsigned long long dims01; size_t limit; long long cl; Want want; };
    const Row rows[] = {
        // k = 8 pipelined: 256 threads and 16 KiB at any M
        {8, 200, 0, true, true, 320, 120, 64 * 64, L, 8, {DF_SWEEP_PIPELINED, true, 256u, 16 * KiB, false, false, 4}},
        {8, 60000, 0, true, true, 320, 120, 64 * 64, L, 8193, {DF_SWEEP_PIPELINED, true, 256u, 16 * KiB, false, false, 8}},
        {8, 60000, 0, true, true, 320, 120, 64 * 64, 64 * KiB, 65537, {DF_SWEEP_PIPELINED, true, 256u, 16 * KiB, false, false, 16}},
        // k = 4 keeps the node table while it fits, 1024 threads past 80 KiB, no table past the limit
        {4, 200, 0, true, true, 320, 120, 64 * 64, L, 8192, {DF_SWEEP_PIPELINED, true, 512u, 6400, true, false, 4}},
        {4, 2560, 0, true, true, 320, 120, 64 * 64, L, 65536, {DF_SWEEP_PIPELINED, true, 512u, 80 * KiB, true, false, 8}},
        {4, 2561, 0, true, true, 320, 120, 64 * 64, L, 8, {DF_SWEEP_PIPELINED, true, 1024u, 80 * KiB + 32, true, true, 4}},
        {4, 5120, 0, true, true, 320, 120, 64 * 64, L, 8, {DF_SWEEP_PIPELINED, true, 1024u, 160 * KiB, true, true, 4}},
        {4, 5121, 0, true, true, 320, 120, 64 * 64, L, 8, {DF_SWEEP_PIPELINED, true, 512u, 0, false, false, 4}},
        // the other k: the batched LDS kernel while 32 M fits, table rows otherwise
        {3, 200, 0, true, true, 320, 120, 64 * 64, L, 8, {DF_SWEEP_LDS_ROWS, true, 512u, 6400, false, false, 8}},
        {3, 5120, 0, true, false, 320, 120, 64 * 64, L, 65537, {DF_SWEEP_LDS_ROWS, false, 512u, 160 * KiB, false, false, 8}},
        {3, 5121, 0, true, true, 320, 120, 64 * 64, L, 8, {DF_SWEEP_TABLE_ROWS, true, 0u, 0, false, false, 0}},
        // the switches, one at a time, at k = 8
        {8, 200, NP, true, true, 320, 120, 64 * 64, L, 8, {DF_SWEEP_LDS_ROWS, true, 512u, 6400, false, false, 8}},
        {8, 200, NW, true, true, 320, 120, 64 * 64, L, 8, {DF_SWEEP_LDS_ROWS, false, 512u, 6400, false, false, 8}},
        {8, 200, NL, true, true, 320, 120, 64 * 64, L, 8, {DF_SWEEP_TABLE_ROWS, true, 0u, 0, false, false, 0}},
        {8, 200, NT, true, true, 320, 120, 64 * 64, L, 8, {DF_SWEEP_BRICKS, false, 0u, 0, false, false, 0}},
        {8, 200, 0, false, true, 320, 120, 64 * 64, L, 8, {DF_SWEEP_BRICKS, false, 0u, 0, false, false, 0}},
        {8, 200, 0, true, false, 320, 120, 64 * 64, L, 8, {DF_SWEEP_LDS_ROWS, false, 512u, 6400, false, false, 8}},
        // the pipelined kernel's 24-bit multiply, 32-bit dists offset and 30-bit plane
        {8, 200, 0, true, true, (1ull << 24) - 1, 1, 64 * 64, L, 8, {DF_SWEEP_PIPELINED, true, 256u, 16 * KiB, false, false, 4}},
        {8, 200, 0, true, true, 1ull << 24, 1, 64 * 64, L, 8, {DF_SWEEP_LDS_ROWS, true, 512u, 6400, false, false, 8}},
        {8, 200, 0, true, true, 2, (1ll << 24) - 1, 64 * 64, L, 8, {DF_SWEEP_PIPELINED, true, 256u, 16 * KiB, false, false, 4}},
        {8, 200, 0, true, true, 2, 1ll << 24, 64 * 64, L, 8, {DF_SWEEP_LDS_ROWS, true, 512u, 6400, false, false, 8}},
        {8, 200, 0, true, true, 65537, 65535, 64 * 64, L, 8, {DF_SWEEP_PIPELINED, true, 256u, 16 * KiB, false, false, 4}},
        {8, 200, 0, true, true, 65536, 65536, 64 * 64, L, 8, {DF_SWEEP_LDS_ROWS, true, 512u, 6400, false, false, 8}},
        {8, 200, 0, true, true, 320, 120, (1ull << 30) - 1, L, 8, {DF_SWEEP_PIPELINED, true, 256u, 16 * KiB, false, false, 4}},
        {8, 200, 0, true, true, 320, 120, 1ull << 30, L, 8, {DF_SWEEP_LDS_ROWS, true, 512u, 6400, false, false, 8}},
    };
    for (const Row& r : rows) {
        const DfWarpVariant d = df_warp_variant(r.k, r.M, r.flags, r.tables, r.wtables, r.pitch, r.rows, r.dims01, r.limit, r.cl);
        if (!same(d, r.want)) { printf("variant row %d: kind %d threads %u lds %zu zt %d\n", (int)(&r - rows), (int)d.kind, d.threads, d.lds, d.zt); return 1; }
    }
    // every combination of the edge values
    const int Ms[] = {8, 200, 2047, 2048, 2049, 2559, 2560, 2561, 5119, 5120, 5121, 60000};
    const size_t limits[] = {64 * KiB, 160 * KiB};
    const struct { unsigned long long pitch; long long rows; } images[] = {{320, 120}, {(1ull << 24) - 1, 1}, {1ull << 24, 1}, {2, (1ll << 24) - 1}, {2, 1ll << 24},
                                                                          {65537, 65535}, {65536, 65536}};
    const unsigned long long planes[] = {64 * 64, (1ull << 30) - 1, 1ull << 30};
    const long long cls[] = {1, 8192, 8193, 65536, 65537};
    long n = 0;
    for (int k = 1; k <= 8; ++k) for (int M : Ms) for (unsigned fb = 0; fb < 16; ++fb) for (int tw = 0; tw < 4; ++tw)
        for (size_t limit : limits) for (const auto& im : images) for (unsigned long long dims01 : planes) for (long long cl : cls) {
            const unsigned flags = (fb & 1 ? NT : 0) | (fb & 2 ? NW : 0) | (fb & 4 ? NL : 0) | (fb & 8 ? NP : 0);
            const bool tables = tw & 1, wtables = tw & 2;
            const DfWarpVariant d = df_warp_variant(k, M, flags, tables, wtables, im.pitch, im.rows, dims01, limit, cl);
            const Want w = variant_rules(k, M, flags, tables, wtables, im.pitch, im.rows, dims01, limit, cl);
            if (!same(d, w) || d.lds > limit) {
                printf("variant k %d M %d flags %u tables %d %d pitch %llu rows %lld plane %llu limit %zu cl %lld: kind %d/%d threads %u/%u lds %zu/%zu zt %d/%d\n", k, M,
                       flags, tables, wtables, im.pitch, im.rows, dims01, limit, cl, (int)d.kind, w.kind, d.threads, w.threads, d.lds, w.lds, d.zt, w.zt);
                return 1;
            }
            ++n;
        }
    *n_out = n;
    return 0;
}

// ---- the look-ahead policy: the specification
struct WantPolicy { bool use_models; int want_models; bool ahead, quiet; int want_models_now; float pf_margin; bool side_work; };
static WantPolicy policy_rules(unsigned flags, int k, int tab_sweeps, bool tab_complete, const uint32_t host_report[3])
{
    WantPolicy w;
    const bool use_models = !(flags & DF_WARP_NO_BLOCK_MODEL) && (k == 8 || k == 4);
    const int want_models = !use_models ? 0 : (flags & DF_WARP_BLOCK_MODEL_NOW) ? 2 : tab_sweeps >= 1 ? 1 : 0;
    bool ahead = !(flags & (DF_WARP_NO_PREFETCH | DF_WARP_BLOCK_MODEL_NOW));
    if (ahead && !(flags & DF_WARP_STEADY_PREFETCH) && tab_sweeps >= 8 && (tab_sweeps & 7) != 0 && host_report[0] == 0u && host_report[1] == 0u &&
        host_report[2] == 0u) ahead = false;
    const bool quiet = !ahead && !(flags & (DF_WARP_NO_PREFETCH | DF_WARP_BLOCK_MODEL_NOW));
    const int want_models_now = quiet ? 0 : want_models;
    w.use_models = use_models; w.want_models = want_models; w.ahead = ahead; w.quiet = quiet; w.want_models_now = want_models_now;
    w.pf_margin = ahead && !tab_complete && tab_sweeps >= 1 ? 0.05f : 0.f;
    w.side_work = ahead && (!tab_complete || want_models_now);
    return w;
}
static int same(const DfVerdictPolicy& p, const WantPolicy& w)
{
    return p.use_models == w.use_models && p.want_models == w.want_models && p.ahead == w.ahead && p.quiet == w.quiet && p.want_models_now == w.want_models_now &&
           p.pf_margin == w.pf_margin && p.side_work == w.side_work;
}

static int check_policy(long* n_out)
{
    const unsigned NPF = DF_WARP_NO_PREFETCH, SP = DF_WARP_STEADY_PREFETCH, NOW = DF_WARP_BLOCK_MODEL_NOW, NBM = DF_WARP_NO_BLOCK_MODEL;
    const uint32_t idle[3] = {0u, 0u, 0u}, busy[3] = {0u, 0u, 5u};
    // hand-written rows: {flags, k, tab_sweeps, tab_complete, report} -> {use_models, want_models, ahead, quiet, want_models_now, pf_margin, side_work}
    struct Row { unsigned flags; int k, sweeps; bool complete; const uint32_t* report; WantPolicy want; };
    const Row rows[] = {
        {0, 8, 0, false, busy, {true, 0, true, false, 0, 0.f, true}},             // first sweep over on-demand tables: no models, no margin yet
        {0, 8, 0, true, busy, {true, 0, true, false, 0, 0.f, false}},             // ... over complete tables: nothing for the side stream
        {0, 8, 1, false, busy, {true, 1, true, false, 1, 0.05f, true}},           // second sweep: models and look-ahead builds
        {0, 8, 7, true, idle, {true, 1, true, false, 1, 0.f, true}},              // the report is not asked before sweep 8
        {0, 8, 8, true, idle, {true, 1, true, false, 1, 0.f, true}},              // every 8th sweep probes
        {0, 8, 9, true, idle, {true, 1, false, true, 0, 0.f, false}},             // at rest: a quiet frame
        {0, 8, 9, true, busy, {true, 1, true, false, 1, 0.f, true}},              // something was listed lately
        {0, 8, 16, true, idle, {true, 1, true, false, 1, 0.f, true}},
        {SP, 8, 9, true, idle, {true, 1, true, false, 1, 0.f, true}},             // steady: on in every frame
        {NPF, 8, 9, false, idle, {true, 1, false, false, 1, 0.f, false}},         // everything on the caller's stream: not quiet, models made there
        {NOW, 8, 0, false, idle, {true, 2, false, false, 2, 0.f, false}},         // models from the first sweep on, in order
        {NBM, 8, 9, false, busy, {false, 0, true, false, 0, 0.05f, true}},        // no models; the look-ahead builds stay
        {0, 3, 9, true, busy, {false, 0, true, false, 0, 0.f, false}},            // k without models, complete tables: no side work
        {0, 4, 1, true, busy, {true, 1, true, false, 1, 0.f, true}},
    };
    for (const Row& r : rows) {
        const DfVerdictPolicy p = df_verdict_policy(r.flags, r.k, r.sweeps, r.complete, r.report);
        if (!same(p, r.want)) { printf("policy row %d\n", (int)(&r - rows)); return 1; }
    }
    const int sweeps[] = {0, 1, 7, 8, 9, 16};
    const uint32_t reports[][3] = {{0u, 0u, 0u}, {1u, 0u, 0u}, {0u, 1u, 0u}, {0u, 0u, 1u}, {7u, 7u, 7u}};
    long n = 0;
    for (unsigned fb = 0; fb < 16; ++fb) for (int k = 1; k <= 8; ++k) for (int ts : sweeps) for (int complete = 0; complete < 2; ++complete) for (const auto& rep : reports) {
        const unsigned flags = (fb & 1 ? NPF : 0) | (fb & 2 ? SP : 0) | (fb & 4 ? NOW : 0) | (fb & 8 ? NBM : 0);
        const DfVerdictPolicy p = df_verdict_policy(flags, k, ts, complete != 0, rep);
        if (!same(p, policy_rules(flags, k, ts, complete != 0, rep))) {
            printf("policy flags %u k %d sweeps %d complete %d report %u %u %u\n", flags, k, ts, complete, rep[0], rep[1], rep[2]);
            return 1;
        }
        ++n;
    }
    *n_out = n;
    return 0;
}

int main()
{
    long nv = 0, np = 0;
    if (check_variant(&nv) || check_policy(&np)) return 1;
    CHECK(DF_WARP_PREFETCH_MARGIN_M == 0.05f);
    printf("warp decide ok: %ld variants, %ld policies\n", nv, np);
    return 0;
}
