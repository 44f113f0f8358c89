// dfusion_warp_pipe.h -- device code of the pipelined warped sweep (the default): its launch plan and the sweep kernel.  Launched from
// dfusion_warp.hip only.
#pragma once
#include "dfusion_warp_sweep.h"
#include "dfusion_plan_halves.h"

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
// it ran), per HALF layer of 4 planes: a half is swept when the block is alive, the sub-verdicts (a.blk_sub, where there are any) keep one
// of the half's four sub-blocks, and the slab owns one of its planes.  The ballots of the two halves, interleaved per patch
// (dfusion_plan_halves.h), are the item's mask; its work w is half the number of set bits, rounded up.  Alive items go into bin w (bins[w * n_items ...],
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
    unsigned long long m = 0, hw01 = 0, hw23 = 0;
    unsigned n_half = 0;
    if (item < n_items) {                                                  // wave-uniform
        const unsigned half = item & 1u, tcol = item >> 1;
        const int tx = (int)(tcol % (unsigned)tiles_x), ty = (int)((tcol / (unsigned)tiles_x) % (unsigned)tiles_y);
        const int zb = (int)(tcol / ((unsigned)tiles_x * (unsigned)tiles_y));
        const int lt0 = a.bz0 + zb * a.zt;
        const int own1 = min(a.z_own0 + a.z_own_n, a.Z);
        const int x0 = tx * DF_ROW_TX + p * 8, y0 = ty * DF_LDS_TY + (int)half * 8;                  // first column of the patch
        bool keep = l < a.zt && max((lt0 + l) * DF_ROW_TZ, a.z_own0) < min((lt0 + l + 1) * DF_ROW_TZ, own1) && x0 < a.X && y0 < a.Y;
        // the verdict pass has judged the patch's 8 x 8 x 8 voxels of the layer (df_block_verdict_kernel: zero-weight, ball, blend-model box)
        unsigned verdict = 1u, sub = 0xffu;
        if (keep && a.blk_alive) {
            const size_t blk = ((size_t)(lt0 + l - a.tab_z0 / DF_ROW_TZ) * a.bm_nby + (unsigned)(y0 >> 3)) * a.bm_nbx + (unsigned)(x0 >> 3);
            verdict = a.blk_alive[blk];
            keep = verdict != 0u;
            if (keep && a.blk_sub) {
                sub = a.blk_sub[blk];                                      // (bit 4 h + q: df_sub_verdict_kernel)
                // (no sub-block kept: the block leaves the frame's verdicts too)
                if (sub == 0u) const_cast<uint8_t*>(a.blk_alive)[blk] = 0;
            }
        }
        // the planes of either half that this launch sweeps (never one the slab does not own)
        const int np0 = keep && (sub & 0x0fu) ? df_half_planes((lt0 + l) * DF_ROW_TZ, 0, a.z_own0, own1) : 0;
        const int np1 = keep && (sub & 0xf0u) ? df_half_planes((lt0 + l) * DF_ROW_TZ, 1, a.z_own0, own1) : 0;
        keep = (np0 | np1) != 0;
        m = __builtin_amdgcn_ballot_w64(keep);
        const unsigned long long m0 = __builtin_amdgcn_ballot_w64(np0 != 0), m1 = __builtin_amdgcn_ballot_w64(np1 != 0);
        n_half = (unsigned)__popcll(m0) + (unsigned)__popcll(m1);
        hw01 = (unsigned long long)df_halves_word((unsigned)m0 & 0xffffu, (unsigned)m1 & 0xffffu) |
               ((unsigned long long)df_halves_word((unsigned)(m0 >> 16) & 0xffffu, (unsigned)(m1 >> 16) & 0xffffu) << 32);
        hw23 = (unsigned long long)df_halves_word((unsigned)(m0 >> 32) & 0xffffu, (unsigned)(m1 >> 32) & 0xffffu) |
               ((unsigned long long)df_halves_word((unsigned)(m0 >> 48) & 0xffffu, (unsigned)(m1 >> 48) & 0xffffu) << 32);
        if (code_out) {                                                    // (wave-uniform) which alive cells' blocks have 4-bit neighbour codes
            const bool coded = keep && a.blk_alive && (verdict & 2u) != 0u;                          // (bit 1 of the verdict byte: see df_block_verdict_kernel)
            const unsigned long long cm = __builtin_amdgcn_ballot_w64(coded);
            if (ln == 0 && m) code_out[item] = cm;
        }
        if (a.n_swept) {                                                   // (measurement hook: what the sweep will put through the warp)
            unsigned v = (unsigned)(64 * (np0 + np1));
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
            if (ln == 0 && v) atomicAdd(a.n_swept, (unsigned long long)v);
        }
    }
    const unsigned w = (n_half + 1u) >> 1;                                 // 1 .. 64 for 1 .. 128 half layers: the 65 bins
    unsigned slot = 0;
    if (ln == 0 && m) slot = atomicAdd(&s_cnt[w], 1u);
    __syncthreads();
    if (threadIdx.x < DF_PLAN_BINS && s_cnt[threadIdx.x]) s_base[threadIdx.x] = atomicAdd(&cnt[threadIdx.x], s_cnt[threadIdx.x]);
    __syncthreads();
    if (ln == 0 && m) {
        mask_out[2 * (size_t)item] = hw01; mask_out[2 * (size_t)item + 1] = hw23;
        bins[(size_t)w * n_items + s_base[w] + slot] = item;
    }
}

// The sweep.  One workgroup = WGT / 256 strip items of the plan; its waves are independent of each other once the plan is read.
//   LDSN = false (k = 8, every node count; k = 4 where the node table is too large for the LDS): NO node table in LDS.  A cell whose block
//     has 4-bit neighbour codes (the model pass has been over it: all but the blocks new this frame) blends out of the wave's own copies
//     of its sub-block unions -- 8 sub-blocks x 16 x {rot, node_t} = 4 KiB per wave, refilled once per (patch, layer) cell from W.rt in the
//     L2 through the union lists (bm_ids: one dword per lane, prefetched a layer ahead); the others gather their neighbours from W.rt.
//     16 KiB of LDS per 256-thread workgroup (DF_PIPE_WGT: 4 waves) whatever M is: the occupancy (six workgroups per CU, 6 waves / SIMD at <= 80 VGPRs) and the
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
    // (round 7: the cells are the plan's HALF layers -- where the sub-verdicts found a half's four sub-blocks dead, the sequence skips it)
    unsigned items_s[SPW]; unsigned long long masks_s[2 * SPW];             // (per item: patches 0-1, patches 2-3; dfusion_plan_halves.h)
    unsigned long long cmask_s[SPW];
    unsigned total2 = 0;
#pragma unroll
    for (unsigned s_ = 0; s_ < SPW; ++s_) {
        const unsigned sidx = group * SPW + s_;
        items_s[s_] = 0u; masks_s[2 * s_] = masks_s[2 * s_ + 1] = 0ull;
        cmask_s[s_] = 0ull;
        if (sidx < n_alive) {
            const int j = __ffsll((unsigned long long)__builtin_amdgcn_ballot_w64(sidx < bin_end)) - 1;      // its bin: the first running total above sidx
            const unsigned r = sidx - ((unsigned)__builtin_amdgcn_readlane((int)bin_end, j) - (unsigned)__builtin_amdgcn_readlane((int)bin_cnt, j));
            items_s[s_] = (unsigned)__builtin_amdgcn_readfirstlane((int)a.plan_bins[(size_t)(DF_PLAN_BINS - 1 - j) * a.plan_items + r]);
#pragma unroll
            for (unsigned w_ = 0; w_ < 2u; ++w_) {
                const unsigned long long m = a.plan_mask[2 * (size_t)items_s[s_] + w_];
                masks_s[2 * s_ + w_] = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(m >> 32)) << 32) |
                                       (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)m);
                total2 += (unsigned)__popcll(masks_s[2 * s_ + w_]);
            }
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
    for (unsigned s_ = 1; s_ < SPW; ++s_) if ((q >> 2) == s_) item = items_s[s_];
#pragma unroll
    for (unsigned w_ = 1; w_ < 2 * SPW; ++w_) if ((q >> 1) == w_) m_item = masks_s[w_];
    const unsigned h32 = (unsigned)(m_item >> (32u * (q & 1u)));           // the patch's half layers, bit 2 l + h
    unsigned long long c_item = cmask_s[0];
#pragma unroll
    for (unsigned s_ = 1; s_ < SPW; ++s_) if ((q >> 2) == s_) c_item = cmask_s[s_];
    const unsigned cbits = CODES ? (unsigned)(c_item >> (16u * (q & 3u))) & 0xffffu : 0u;      // layers of this patch whose block has 4-bit codes
    const unsigned n2 = (unsigned)__popc(h32);
    const unsigned seg_lo = max(c0, pre), seg_hi = min(c1, pre + n2);
    const unsigned pre0 = pre;
    pre += n2;
    if (seg_lo >= seg_hi) continue;                                        // none of this patch's cells are this wave's
    const unsigned lo = seg_lo - pre0, hi = seg_hi - pre0;                 // half-layer cells [lo, hi) of the patch's popc(h32)
    const unsigned seg = df_halves_segment(h32, lo, hi);                   // ... as bits: what this segment sweeps
    const unsigned alive = df_halves_layers(seg);                          // its layers
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
    // a layer's first and last plane follow from its half bits: a layer whose upper half alone is swept starts at + 4, one whose lower
    // half alone is swept ends at + 4 -- at the segment's ends (the neighbouring wave has the other half) as inside it (the sub-verdicts
    // found the other half dead).  Every set half has a plane the slab owns (the plan kernel saw to it), so no layer is cut down to nothing.
    auto layer_zb = [&](int l) { return max((lt0 + l) * DF_ROW_TZ + df_halves_z0(seg, l), a.z_own0); };
    auto layer_ze = [&](int l) { return min((lt0 + l) * DF_ROW_TZ + df_halves_z1(seg, l), own1); };
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
