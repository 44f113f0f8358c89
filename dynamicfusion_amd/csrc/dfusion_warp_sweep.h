// dfusion_warp_sweep.h -- device code of the warped integrate: the kernel arguments, the per-voxel table layout, the conservative tile
// cull, the candidate ranking of the table build and the brick / row-tile / LDS row-tile sweeps.  Launched from dfusion_warp.hip only.
#pragma once
#include "dfusion_internal.h"
#include "dfusion_pyramid.h"
#include "dfusion_warp_topk.h"

// ====================================================================================== integrate (warped)
struct DfWarpedArgs {
    uint32_t* vol; int X, Y, Z;
    int z_store0, z_own0, z_own_n;
    int bz0;                       // first brick / tile layer of this launch
    float vsx, vsy, vsz;
    DfAff vol2world, world2cam;
    DfIntegrateParams P;
    unsigned long long* n_upd;
    unsigned long long* n_swept;   // nullable (dfusion_warp_debug_counters): += voxels of the plan's alive (patch, half layer) cells
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
    // + tx) * 2 + half.  plan_mask[2 item], [2 item + 1] hold its 4 x 16 x 2 verdict bits, one per HALF layer (8 x 8 x 4 voxels): word
    // p >> 1, bit 32 (p & 1) + 2 l + h = planes 4 h .. 4 h + 3 of layer l of patch p are swept (dfusion_plan_halves.h); the items with
    // any bit set are listed in bin w = half the set bits, rounded up (plan_bins[w * plan_items ...], plan_cnt[w] of them) -- all made on the stream by
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
    // sub-block models (k = 8, written by the model pass beside the union lists; null = none): per union entry of every 4 x 4 x 4 sub-block
    // the {mid, half width} half pairs of lambda and of w over its 64 voxels, [block][entry][sub] (sub = 4 h + q); bm_sub_cnt
    // [block * 8 + sub] = entries | reference entry << 8; bm_sub_ok [block] 1 = the block has them (every sub-union fits, weights normalise)
    uint32_t* bm_sub_lam; uint32_t* bm_sub_w; uint16_t* bm_sub_cnt; uint8_t* bm_sub_ok;
    // this frame's sub-verdicts (df_sub_verdict_kernel), one byte per block, bit 4 h + q; null = every half layer of an alive block is swept
    const uint8_t* blk_sub;
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
