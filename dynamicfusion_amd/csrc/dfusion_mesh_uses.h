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
// and msm_run, the judge of one run of equal keys.  Every grid is capped at DF_MESH_MAX_BLOCKS workgroups (524 288 lanes) and strides over
// its range with 64-bit indices; grids, rounding, the triangle load and the counting are the mesh kit's (dfusion_mesh_kit.h).
#pragma once
#include <hipcub/hipcub.hpp>
#include "dfusion_mesh_kit.h"

struct DfMsmArgs {
    const uint32_t* tris; size_t T; size_t V; size_t N;      // N = 6 T keys
    int k;                                                   // bits of V: every index < V fits, and 2^k - 1 is no vertex
    unsigned long long *keys_in, *keys;                      // [N] as emitted, sorted
    uint8_t *dir_in, *dir;                                   // [N] 0: the half-edge src -> dst exists, 1: its reverse does
    uint32_t* pos;                                           // [N + 1] head flags, then their exclusive sum (over keys_in, dead after the sort)
    unsigned long long* counts;
    int slot_invalid, slot_degenerate;                       // where in counts the emit stage adds its two numbers
};

// The uses of one edge: f half-edges src -> dst (the value 0), b half-edges dst -> src (the value 1).
struct DfMsmRun {
    unsigned long long f, b;
    __device__ __forceinline__ bool boundary() const { return f + b == 1ull; }                              // used once
    __device__ __forceinline__ bool irregular() const { return !boundary() && !(f == 1ull && b == 1ull); }  // not once each way either
};
// Counts the run of equal keys whose head is sorted key i.
__device__ __forceinline__ DfMsmRun msm_run(const unsigned long long* keys, const uint8_t* dir, size_t N, size_t i)
{
    DfMsmRun r = {0ull, 0ull};
    for (size_t j = i; j < N && keys[j] == keys[i]; ++j) { if (dir[j]) ++r.b; else ++r.f; }
    return r;
}

static __global__ __launch_bounds__(256) void df_msm_emit_kernel(const DfMsmArgs a)
{
    const unsigned long long none = a.k == 32 ? ~0ull : (1ull << (2 * a.k)) - 1ull;
    unsigned long long n_invalid = 0ull, n_degenerate = 0ull;           // wave-uniform
    for (size_t t0 = (size_t)blockIdx.x * 256; t0 < a.T; t0 += (size_t)gridDim.x * 256) {      // (workgroup-uniform trip count)
        const size_t t = t0 + threadIdx.x;
        uint32_t i[3];
        const bool valid = df_mesh_load(a.tris, t, a.T, (uint32_t)a.V, i);                     // (V < 2^32)
        const bool invalid = t < a.T && !valid, degenerate = valid && (i[0] == i[1] || i[1] == i[2] || i[0] == i[2]);
        if (t < a.T) {
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const unsigned long long s = i[e], d = i[e == 2 ? 0 : e + 1];
                const bool live = valid && s != d;
                a.keys_in[6 * t + 2 * e] = live ? (s << a.k | d) : none;
                a.keys_in[6 * t + 2 * e + 1] = live ? (d << a.k | s) : none;
                a.dir_in[6 * t + 2 * e] = 0;
                a.dir_in[6 * t + 2 * e + 1] = 1;
            }
        }
        n_invalid += (unsigned long long)__popcll(__ballot(invalid));
        n_degenerate += (unsigned long long)__popcll(__ballot(degenerate));
    }
    df_mesh_wave_add(a.counts, a.slot_invalid, n_invalid);
    df_mesh_wave_add(a.counts, a.slot_degenerate, n_degenerate);
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

// The bits of V (2^k > V, k >= 1).
static inline int df_msm_key_bits(size_t V)
{
    int k = 1;
    while (k < 32 && (V >> k)) ++k;
    return k;
}

// The workspace of the stages above, front to back: [keys as emitted 48 T, then the positions 24 T + 4 over them] [sorted keys 48 T]
// [values 6 T] [sorted values 6 T].  -> its size, a multiple of 16.
static inline size_t df_msm_uses_bytes(size_t N) { return 2 * df_mesh_up16(N * 8) + 2 * df_mesh_up16(N); }

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
    const size_t N = a.N, o_keys = df_mesh_up16(N * 8), o_dir_in = o_keys + df_mesh_up16(N * 8), o_dir = o_dir_in + df_mesh_up16(N);
    a.keys_in = (unsigned long long*)ws; a.keys = (unsigned long long*)(ws + o_keys);
    a.dir_in = (uint8_t*)(ws + o_dir_in); a.dir = (uint8_t*)(ws + o_dir);
    a.pos = (uint32_t*)ws;                                               // 4 (N + 1) <= 8 N
    const dim3 gt(df_mesh_blocks(a.T)), gn(df_mesh_blocks(N + 1)), wg(256);
    hipLaunchKernelGGL(df_msm_emit_kernel, gt, wg, 0, st, a);
    DF_LAUNCH_CHECK();
    DF_HIP(hipcub::DeviceRadixSort::SortPairs(cub, cub_bytes, (const unsigned long long*)a.keys_in, a.keys, (const uint8_t*)a.dir_in, a.dir,
                                              N, 0, 2 * a.k, st));
    hipLaunchKernelGGL(df_msm_heads_kernel, gn, wg, 0, st, a);
    DF_LAUNCH_CHECK();
    DF_HIP(hipcub::DeviceScan::ExclusiveSum(cub, cub_bytes, a.pos, a.pos, N + 1, st));
    return DF_OK;
}
