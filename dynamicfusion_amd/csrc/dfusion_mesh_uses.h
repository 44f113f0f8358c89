// dfusion_mesh_uses.h -- the directed uses of every edge of an indexed triangle mesh, sorted: the emit / sort / heads / scan stages that
// dfusion_mesh_adjacency (dfusion_mesh_smooth.hip) and dfusion_mesh_boundary_loops (dfusion_mesh_holes.hip) both start with, once.
// The kernels are static: each of the two files gets its own copy of the same text under the same name.
//
//   emit      one lane per triangle: six 2k-bit keys (src << k | dst), k the bits of V -- each half-edge a -> b with a != b as (a, b)
//             with the value 0 and as (b, a) with the value 1; every other place of the six holds the all-ones key, whose src no vertex
//             has.  Invalid and degenerate triangles counted
//   sort      one hipcub::DeviceRadixSort::SortPairs over the 2k bits
//   heads     a flag of 1 on the first key of every run of equal keys but the all-ones one; one hipcub exclusive sum, in place, with a
//             spare element for the total: the position of every run among the runs
// Every grid is capped at DF_MSM_MAX_BLOCKS workgroups (524 288 lanes) and strides over its range with 64-bit indices.
#pragma once
#include <hipcub/hipcub.hpp>
#include "dfusion_internal.h"

#define DF_MSM_MAX_BLOCKS 2048u

static inline unsigned df_msm_blocks(size_t n) { const size_t b = (n + 255) / 256; return (unsigned)(b < DF_MSM_MAX_BLOCKS ? b : DF_MSM_MAX_BLOCKS); }

struct DfMsmArgs {
    const uint32_t* tris; size_t T; size_t V; size_t N;      // N = 6 T keys
    int k;                                                   // bits of V: every index < V fits, and 2^k - 1 is no vertex
    unsigned long long *keys_in, *keys;                      // [N] as emitted, sorted
    uint8_t *dir_in, *dir;                                   // [N] 0: the half-edge src -> dst exists, 1: its reverse does
    uint32_t* pos;                                           // [N + 1] head flags, then their exclusive sum (over keys_in, dead after the sort)
    uint32_t* cls;                                           // [V] 0, raised to 2 (boundary) or 3 (irregular)
    uint32_t* row_start;                                     // [V + 1] the caller's, or workspace
    uint32_t* nbr; unsigned long long cap;
    uint8_t* vclass;
    unsigned long long* counts;
    int slot_invalid, slot_degenerate;                       // where in counts the emit stage adds its two numbers
};

__device__ __forceinline__ void msm_count(unsigned long long* counts, int which, unsigned long long wave_uniform)
{
    if ((threadIdx.x & 63) == 0 && wave_uniform) atomicAdd(&counts[which], wave_uniform);
}

static __global__ __launch_bounds__(256) void df_msm_emit_kernel(const DfMsmArgs a)
{
    const unsigned long long none = a.k == 32 ? ~0ull : (1ull << (2 * a.k)) - 1ull;
    unsigned long long n_invalid = 0ull, n_degenerate = 0ull;           // wave-uniform
    for (size_t t0 = (size_t)blockIdx.x * 256; t0 < a.T; t0 += (size_t)gridDim.x * 256) {      // (workgroup-uniform trip count)
        const size_t t = t0 + threadIdx.x;
        bool invalid = false, degenerate = false;
        if (t < a.T) {
            const uint32_t i[3] = {a.tris[3 * t], a.tris[3 * t + 1], a.tris[3 * t + 2]};
            invalid = !((size_t)i[0] < a.V && (size_t)i[1] < a.V && (size_t)i[2] < a.V);       // tested before anything is indexed
            degenerate = !invalid && (i[0] == i[1] || i[1] == i[2] || i[0] == i[2]);
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const unsigned long long s = i[e], d = i[e == 2 ? 0 : e + 1];
                const bool live = !invalid && s != d;
                a.keys_in[6 * t + 2 * e] = live ? (s << a.k | d) : none;
                a.keys_in[6 * t + 2 * e + 1] = live ? (d << a.k | s) : none;
                a.dir_in[6 * t + 2 * e] = 0;
                a.dir_in[6 * t + 2 * e + 1] = 1;
            }
        }
        n_invalid += (unsigned long long)__popcll(__ballot(invalid));
        n_degenerate += (unsigned long long)__popcll(__ballot(degenerate));
    }
    msm_count(a.counts, a.slot_invalid, n_invalid);
    msm_count(a.counts, a.slot_degenerate, n_degenerate);
}

static __global__ __launch_bounds__(256) void df_msm_heads_kernel(const DfMsmArgs a)
{
    const unsigned long long none = a.k == 32 ? ~0ull : (1ull << (2 * a.k)) - 1ull;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i <= a.N; i += (size_t)gridDim.x * 256) {
        uint32_t head = 0u;
        if (i < a.N) {
            const unsigned long long key = a.keys[i];
            head = key != none && (i == 0 || a.keys[i - 1] != key) ? 1u : 0u;
        }
        a.pos[i] = head;
    }
}

static inline bool msm_overlap(const void* p, size_t pn, const void* q, size_t qn)
{
    if (!p || !q || !pn || !qn) return false;
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qn && b < a + pn;
}

static inline size_t df_msm_up16(size_t b) { return (b + 15) / 16 * 16; }

// The bits of V (2^k > V, k >= 1).
static inline int df_msm_key_bits(size_t V)
{
    int k = 1;
    while (k < 32 && (V >> k)) ++k;
    return k;
}

// The workspace of the stages above, front to back: [keys as emitted 48 T, then the positions 24 T + 4 over them] [sorted keys 48 T]
// [values 6 T] [sorted values 6 T].  -> its size, a multiple of 16.
static inline size_t df_msm_uses_bytes(size_t N) { return 2 * df_msm_up16(N * 8) + 2 * df_msm_up16(N); }

// hipcub's storage for the sort of N keys of 2k bits and for an exclusive sum over `scan_items` uint32 (the larger of the two).
static inline int df_msm_uses_cub_bytes(size_t N, int k, size_t scan_items, hipStream_t st, size_t* bytes)
{
    size_t sort_bytes = 0, scan_bytes = 0;
    DF_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                              (const uint8_t*)nullptr, (uint8_t*)nullptr, N, 0, 2 * k, st));
    DF_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, scan_items, st));
    *bytes = sort_bytes > scan_bytes ? sort_bytes : scan_bytes;
    return DF_OK;
}

// Runs the stages: a.tris, T, V, N, k, counts and the two slots are the caller's; keys_in, keys, dir_in, dir and pos are set here from
// `ws` (df_msm_uses_bytes(N) bytes).  Afterwards a.keys / a.dir hold the sorted uses and a.pos [N + 1] the run positions.
static inline int df_msm_sorted_uses(DfMsmArgs& a, char* ws, char* cub, size_t cub_bytes, hipStream_t st)
{
    const size_t N = a.N, o_keys = df_msm_up16(N * 8), o_dir_in = o_keys + df_msm_up16(N * 8), o_dir = o_dir_in + df_msm_up16(N);
    a.keys_in = (unsigned long long*)ws; a.keys = (unsigned long long*)(ws + o_keys);
    a.dir_in = (uint8_t*)(ws + o_dir_in); a.dir = (uint8_t*)(ws + o_dir);
    a.pos = (uint32_t*)ws;                                               // 4 (N + 1) <= 8 N
    const dim3 gt(df_msm_blocks(a.T)), gn(df_msm_blocks(N + 1)), wg(256);
    hipLaunchKernelGGL(df_msm_emit_kernel, gt, wg, 0, st, a);
    DF_LAUNCH_CHECK();
    DF_HIP(hipcub::DeviceRadixSort::SortPairs(cub, cub_bytes, (const unsigned long long*)a.keys_in, a.keys, (const uint8_t*)a.dir_in, a.dir,
                                              N, 0, 2 * a.k, st));
    hipLaunchKernelGGL(df_msm_heads_kernel, gn, wg, 0, st, a);
    DF_LAUNCH_CHECK();
    DF_HIP(hipcub::DeviceScan::ExclusiveSum(cub, cub_bytes, a.pos, a.pos, N + 1, st));
    return DF_OK;
}
