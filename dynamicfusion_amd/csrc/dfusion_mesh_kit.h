// dfusion_mesh_kit.h -- the small machinery every operation on an indexed triangle mesh (the dfusion_mesh_*.hip files) is built from,
// once: the capped grid, the rounding and the overlap test of the argument checks, the carving of a workspace, the guarded load of a
// triangle's indices, the integer sums and maxima of a wave and of a workgroup, and the host launchers of a store of counts and of a pair
// of scans.  A new mesh operation starts from here.  The part above __HIPCC__ is plain C++, checked on the host
// by tests/cxx/mesh_kit_test.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define DF_MESH_MAX_BLOCKS 2048u                     // workgroups of 256 lanes: 524 288 lanes, which then stride over the range
// The grid for n items, one per lane of 256-lane workgroups, capped.  n == 0 gives 0: no caller launches over an empty range.
static inline unsigned df_mesh_blocks(size_t n, unsigned cap = DF_MESH_MAX_BLOCKS) { const size_t b = (n + 255) / 256; return (unsigned)(b < cap ? b : cap); }
static inline size_t df_mesh_up16(size_t b) { return (b + 15) / 16 * 16; }

// Whether the byte ranges [p, p + pn) and [q, q + qn) share a byte; a null pointer or an empty range overlaps nothing.
static inline bool df_mesh_overlap(const void* p, size_t pn, const void* q, size_t qn)
{
    if (!p || !q || !pn || !qn) return false;
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qn && b < a + pn;
}

// Carves a workspace front to back: take() -> the offset of the next array, rounded up to `align`; total() -> the end of the last one.
// Arrays taken one after the other are contiguous up to that rounding, which the callers' memsets rely on.
struct DfMeshCarve {
    size_t at = 0;
    size_t take(size_t bytes, size_t align = 16) { const size_t o = (at + align - 1) / align * align; at = o + bytes; return o; }
    size_t total() const { return at; }
};

#ifdef __HIPCC__
#include "dfusion_internal.h"

// The three indices of triangle t -> all three are < V, tested before anything is indexed.  t >= T: zeros, false.
__device__ __forceinline__ bool df_mesh_load(const uint32_t* __restrict__ tris, size_t t, size_t T, uint32_t V, uint32_t (&i)[3])
{
    if (t >= T) { i[0] = i[1] = i[2] = 0u; return false; }
    i[0] = tris[3 * t]; i[1] = tris[3 * t + 1]; i[2] = tris[3 * t + 2];
    return i[0] < V && i[1] < V && i[2] < V;
}

// The maximum of v over the wave's 64 lanes, in every lane (uint32_t or unsigned long long).  A minimum is ~max(~v).
template <typename U>
__device__ __forceinline__ U df_mesh_wave_max(U v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const U o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
    return v;
}

// counts[which] += a number every lane of the wave holds alike (a sum of ballots): one atomic per wave.
__device__ __forceinline__ void df_mesh_wave_add(unsigned long long* counts, int which, unsigned long long wave_uniform)
{
    if ((threadIdx.x & 63) == 0 && wave_uniform) atomicAdd(&counts[which], wave_uniform);
}

// counts[slot[j]] += the workgroup's sum of every lane's value[j], through LDS: one global atomic per workgroup and slot.  Wave-uniform
// numbers come from lane 0 of each wave, 0 from the others.  It synchronises: EVERY lane of the workgroup must call it, once per kernel.
template <int K>
__device__ __forceinline__ void df_mesh_block_add(unsigned long long* counts, const int (&slot)[K], const unsigned long long (&value)[K])
{
    __shared__ unsigned long long acc[K];
    if (threadIdx.x < K) acc[threadIdx.x] = 0ull;
    __syncthreads();
    for (int j = 0; j < K; ++j)
        if (value[j]) atomicAdd(&acc[j], value[j]);
    __syncthreads();
    if (threadIdx.x < K && acc[threadIdx.x]) atomicAdd(&counts[slot[threadIdx.x]], acc[threadIdx.x]);
}

// counts[slot[j]] = max(itself, every lane's value[j]): the wave's maximum by shuffles, the workgroup's (256 lanes at most) through LDS.
// It synchronises: EVERY lane of the workgroup must call it, once per kernel.
template <int K>
__device__ __forceinline__ void df_mesh_block_max(unsigned long long* counts, const int (&slot)[K], const uint32_t (&value)[K])
{
    __shared__ uint32_t top[K][4];
    for (int j = 0; j < K; ++j) {
        const uint32_t m = df_mesh_wave_max(value[j]);
        if ((threadIdx.x & 63) == 0) top[j][threadIdx.x >> 6] = m;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        uint32_t m = top[threadIdx.x][0];
        for (int w = 1; w < 4; ++w) m = top[threadIdx.x][w] > m ? top[threadIdx.x][w] : m;
        if (m) atomicMax(&counts[slot[threadIdx.x]], (unsigned long long)m);
    }
}

// Host launchers, defined once in dfusion_mesh_components.hip.  set_counts: one lane stores counts[i0] = v0 and counts[i1] = v1 (one
// number is named twice).  scan_bytes: hipcub's storage for an exclusive sum over up to items_max uint32.  scan_pair: the exclusive sums
// of a [na] and b [nb] in place (flags and a spare element for the total) and, with `counts`, counts[0] = b[nb - 1], counts[1] = a[na - 1].
DF_LOCAL int df_mesh_set_counts(unsigned long long* counts, int i0, unsigned long long v0, int i1, unsigned long long v1, hipStream_t st);
DF_LOCAL int df_mesh_scan_bytes(size_t items_max, hipStream_t st, size_t* bytes);
DF_LOCAL int df_mesh_scan_pair(char* cub, size_t cub_bytes, uint32_t* a, size_t na, uint32_t* b, size_t nb, unsigned long long* counts,
                               hipStream_t st);
#endif
