// dfusion_mesh_components.hip -- dfusion_mesh_components / dfusion_mesh_filter / dfusion_gather_rows: the connected components of an
// indexed triangle mesh (dfusion_extract_mesh's, or any), and the mesh without its small pieces.  The rule -- what connects, what a
// label is, what is kept and in which order -- is stated in include/dfusion.h and DESIGN.md section 22 and restated in numpy by
// tests/mesh_components_ref.py, against which every output is compared for equality.  Integers only: no output depends on scheduling.
//
//   components   init      parent[v] = v (IN vertex_label_dev: the labels' array is the forest), counts and flags cleared
//                union     one lane per triangle: a lock-free union-find, a root only ever linked under a smaller index
//                          (dfusion_mesh_cc.h, with the termination argument), read with relaxed agent-scope atomic loads
//                flatten   after the kernel boundary the forest is final: vertex_label[v] = root of v = smallest index of its component
//                count     per valid triangle one integer add on triangle_count[label] -- lanes of a wave with the same label add once
//                          -- and a plain store of 1 into the used flag of its three vertices
//                totals    the four counts by integer adds and an integer maximum
//   filter       best      with keep_largest: max over r of (triangle_count[r] << 32 | ~r): most triangles, then the smaller label
//                keep      a flag per kept triangle, a flag per vertex a kept triangle uses (plain stores of 1)
//                scan      df_mesh_scan_pair: two hipcub exclusive sums, in place, one spare element each for the total
//                compact   triangles rewritten through the scanned vertex offsets; vertex_src / vertex_map
// Every grid is capped and strides over its range with 64-bit indices, so a launch covers any T and V the ABI admits.
// Grids, loads, sums and the scan tail are the mesh kit's (dfusion_mesh_kit.h); its host launchers are defined at the end of this file.
#include <hipcub/hipcub.hpp>
#include "dfusion_mesh_kit.h"
#include "dfusion_mesh_cc.h"

// Deliberately not the kit's 2048: nobody has measured this file's kernels with fewer workgroups.  (The two reductions cap theirs at 1024.)
#define DF_MCC_MAX_BLOCKS (256u * 32u)
#define DF_MCC_NONE 0xffffffffu

// parent[] in device memory.  A plain load may be served from a CU's L1 and see a stale root; these go to the L2, where the
// compare-and-swap is decided.
struct DfCcDeviceMem {
    uint32_t* p;
    __device__ __forceinline__ uint32_t load(uint32_t i) const { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ void store(uint32_t i, uint32_t v) const { __hip_atomic_store(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ uint32_t cas(uint32_t i, uint32_t expect, uint32_t v) const { return atomicCAS(p + i, expect, v); }
};

__global__ __launch_bounds__(256) void df_mcc_init_kernel(uint32_t* parent, size_t V, uint32_t* tcount, uint8_t* used)
{
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (size_t)gridDim.x * 256) {
        parent[v] = (uint32_t)v;
        if (tcount) tcount[v] = 0u;
        if (used) used[v] = 0;
    }
}

__global__ __launch_bounds__(256) void df_mcc_union_kernel(const uint32_t* tris, size_t T, uint32_t V, uint32_t* parent)
{
    DfCcDeviceMem m{parent};
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < T; t += (size_t)gridDim.x * 256) {
        uint32_t i[3];
        if (!df_mesh_load(tris, t, T, V, i)) continue;
        if (i[0] != i[1]) df_cc_union(m, i[0], i[1]);                       // (edges (i0, i1) and (i1, i2) connect all three)
        if (i[1] != i[2]) df_cc_union(m, i[1], i[2]);
    }
}

__global__ __launch_bounds__(256) void df_mcc_flatten_kernel(uint32_t* parent, size_t V)
{
    DfCcDeviceMem m{parent};
    // No union runs beside this: every tree is final, and a lane overwrites only its own entry, with its root -- whoever walks through
    // that entry meanwhile meets the old parent or the root, both ancestors.
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (size_t)gridDim.x * 256)
        m.store((uint32_t)v, df_cc_root(m, (uint32_t)v));
}

__global__ __launch_bounds__(256) void df_mcc_count_kernel(const uint32_t* tris, size_t T, uint32_t V, const uint32_t* label, uint32_t* tcount,
                                                           uint8_t* used, unsigned long long* counts)
{
    const int lane = threadIdx.x & 63;
    unsigned long long n_invalid = 0ull;                                    // wave-uniform
    for (size_t t0 = (size_t)blockIdx.x * 256; t0 < T; t0 += (size_t)gridDim.x * 256) {   // (workgroup-uniform trip count)
        const size_t t = t0 + threadIdx.x;
        uint32_t i[3];
        const bool valid = df_mesh_load(tris, t, T, V, i);
        n_invalid += (unsigned long long)__popcll(__ballot(t < T && !valid));
        uint32_t r = 0u;
        if (valid) { r = label[i[0]]; used[i[0]] = 1; used[i[1]] = 1; used[i[2]] = 1; }
        // the lanes of a wave that hold the same label add once: a mesh in extraction order has one or two labels per wave
        unsigned long long todo = __ballot(valid);
        while (todo) {                                                      // wave-uniform; every trip retires its leader at least
            const int leader = __ffsll((unsigned long long)todo) - 1;
            const uint32_t rl = __shfl(r, leader, 64);
            const unsigned long long same = __ballot(valid && r == rl) & todo;
            if (lane == leader) atomicAdd(&tcount[rl], (unsigned int)__popcll(same));
            todo &= ~same;
        }
    }
    if (counts) df_mesh_wave_add(counts, 2, n_invalid);
}

__global__ __launch_bounds__(256) void df_mcc_totals_kernel(const uint32_t* tcount, const uint8_t* used, size_t V, unsigned long long* counts)
{
    unsigned long long n_comp = 0ull, n_unused = 0ull, largest = 0ull;      // the first two wave-uniform
    for (size_t v0 = (size_t)blockIdx.x * 256; v0 < V; v0 += (size_t)gridDim.x * 256) {
        const size_t v = v0 + threadIdx.x;
        const uint32_t c = v < V ? tcount[v] : 0u;
        n_comp += (unsigned long long)__popcll(__ballot(c != 0u));
        n_unused += (unsigned long long)__popcll(__ballot(v < V && used[v] == 0));
        largest = c > largest ? c : largest;
    }
    largest = df_mesh_wave_max(largest);
    df_mesh_wave_add(counts, 0, n_comp);
    df_mesh_wave_add(counts, 1, n_unused);
    if ((threadIdx.x & 63) == 0 && largest) atomicMax(&counts[3], largest);
}

extern "C" int dfusion_mesh_components(const unsigned int* triangles_dev, unsigned long long n_triangles, unsigned long long n_vertices,
                                       unsigned int* vertex_label_dev, unsigned int* triangle_count_dev, unsigned long long* counts_dev,
                                       dfStream stream)
{
    if (n_vertices > 0xffffffffull || n_triangles > 0xffffffffull) return DF_E_INVALID;
    if ((n_triangles && !triangles_dev) || (n_vertices && !vertex_label_dev)) return DF_E_INVALID;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return DF_E_NO_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    const size_t T = (size_t)n_triangles, V = (size_t)n_vertices;
    if (counts_dev) DF_HIP(hipMemsetAsync(counts_dev, 0, 32, st));
    if (!V) {                                                                                   // every triangle is invalid
        if (counts_dev && T) DF_TRY(df_mesh_set_counts(counts_dev, 2, n_triangles, 2, n_triangles, st));
        return DF_OK;
    }
    const bool counting = triangle_count_dev || counts_dev;
    // workspace: [used flags: V bytes | triangle counts: 4 V bytes, when the caller keeps none]
    const size_t o_cnt = df_mesh_up16(V);
    DfScratchHold hold(st, counting ? o_cnt + (triangle_count_dev ? 0 : V * 4) : 16);           // held until the last launch is enqueued
    if (!hold.entry) return (int)hipErrorOutOfMemory;
    uint8_t* used = counting ? (uint8_t*)hold.mem : nullptr;
    uint32_t* tcount = triangle_count_dev ? triangle_count_dev : counting ? (uint32_t*)(hold.mem + o_cnt) : nullptr;
    hipLaunchKernelGGL(df_mcc_init_kernel, dim3(df_mesh_blocks(V, DF_MCC_MAX_BLOCKS)), dim3(256), 0, st, vertex_label_dev, V, tcount, used);
    DF_LAUNCH_CHECK();
    if (T) {
        hipLaunchKernelGGL(df_mcc_union_kernel, dim3(df_mesh_blocks(T, DF_MCC_MAX_BLOCKS)), dim3(256), 0, st, triangles_dev, T, (uint32_t)V, vertex_label_dev);
        DF_LAUNCH_CHECK();
        hipLaunchKernelGGL(df_mcc_flatten_kernel, dim3(df_mesh_blocks(V, DF_MCC_MAX_BLOCKS)), dim3(256), 0, st, vertex_label_dev, V);
        DF_LAUNCH_CHECK();
    }
    if (!counting) return DF_OK;
    if (T) {
        hipLaunchKernelGGL(df_mcc_count_kernel, dim3(df_mesh_blocks(T, DF_MCC_MAX_BLOCKS)), dim3(256), 0, st, triangles_dev, T, (uint32_t)V,
                           (const uint32_t*)vertex_label_dev, tcount, used, counts_dev);
        DF_LAUNCH_CHECK();
    }
    if (counts_dev) {
        hipLaunchKernelGGL(df_mcc_totals_kernel, dim3(df_mesh_blocks(V, 1024u)), dim3(256), 0, st,
                           (const uint32_t*)tcount, (const uint8_t*)used, V, counts_dev);
        DF_LAUNCH_CHECK();
    }
    return DF_OK;
}

// ---- filter
struct DfMccFilterArgs {
    const uint32_t* tris; size_t T; uint32_t V;
    const uint32_t *label, *tcount;
    unsigned long long min_triangles; int keep_largest;
    unsigned long long* best;          // max of (triangle_count[r] << 32 | ~r)
    uint32_t *tscan, *vscan;           // [T + 1], [V + 1]: flags, then their exclusive sums
    uint32_t* tris_out; unsigned long long tcap;
    uint32_t* vsrc; unsigned long long vcap;
    uint32_t* vmap;
};

__global__ __launch_bounds__(256) void df_mcc_best_kernel(const uint32_t* tcount, size_t V, unsigned long long* best)
{
    unsigned long long key = 0ull;
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (size_t)gridDim.x * 256) {
        const unsigned long long k = ((unsigned long long)tcount[v] << 32) | (unsigned long long)(DF_MCC_NONE - (uint32_t)v);
        key = k > key ? k : key;
    }
    key = df_mesh_wave_max(key);
    if ((threadIdx.x & 63) == 0 && key) atomicMax(best, key);
}

__global__ __launch_bounds__(256) void df_mcc_keep_kernel(const DfMccFilterArgs a)
{
    const uint32_t only = a.keep_largest ? DF_MCC_NONE - (uint32_t)(*a.best & 0xffffffffull) : 0u;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < a.T; t += (size_t)gridDim.x * 256) {
        uint32_t i[3];
        if (!df_mesh_load(a.tris, t, a.T, a.V, i)) continue;
        const uint32_t r = a.label[i[0]];
        if (r >= a.V || (unsigned long long)a.tcount[r] < a.min_triangles || (a.keep_largest && r != only)) continue;
        a.tscan[t] = 1u;
        a.vscan[i[0]] = 1u; a.vscan[i[1]] = 1u; a.vscan[i[2]] = 1u;
    }
}

__global__ __launch_bounds__(256) void df_mcc_compact_triangles_kernel(const DfMccFilterArgs a)
{
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < a.T; t += (size_t)gridDim.x * 256) {
        const uint32_t o = a.tscan[t];
        if (a.tscan[t + 1] == o || (unsigned long long)o >= a.tcap) continue;            // (a kept triangle is valid: its indices are < V)
        a.tris_out[3 * (size_t)o] = a.vscan[a.tris[3 * t]];
        a.tris_out[3 * (size_t)o + 1] = a.vscan[a.tris[3 * t + 1]];
        a.tris_out[3 * (size_t)o + 2] = a.vscan[a.tris[3 * t + 2]];
    }
}

__global__ __launch_bounds__(256) void df_mcc_compact_vertices_kernel(const DfMccFilterArgs a)
{
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < (size_t)a.V; v += (size_t)gridDim.x * 256) {
        const uint32_t n = a.vscan[v];
        const bool kept = a.vscan[v + 1] != n;
        if (kept && (unsigned long long)n < a.vcap) a.vsrc[n] = (uint32_t)v;
        if (a.vmap) a.vmap[v] = kept ? n : DF_MCC_NONE;
    }
}

extern "C" int dfusion_mesh_filter(const unsigned int* triangles_dev, unsigned long long n_triangles, unsigned long long n_vertices,
                                   const unsigned int* vertex_label_dev, const unsigned int* triangle_count_dev, unsigned long long min_triangles,
                                   int keep_largest, unsigned int* triangles_out_dev, unsigned long long triangle_capacity,
                                   unsigned int* vertex_src_dev, unsigned long long vertex_capacity, unsigned int* vertex_map_dev,
                                   unsigned long long* counts_dev, dfStream stream)
{
    if (n_vertices > 0xffffffffull || n_triangles > 0xffffffffull || !counts_dev) return DF_E_INVALID;
    if ((n_triangles && !triangles_dev) || (n_vertices && (!vertex_label_dev || !triangle_count_dev))) return DF_E_INVALID;
    if ((triangle_capacity && !triangles_out_dev) || (vertex_capacity && !vertex_src_dev)) return DF_E_INVALID;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return DF_E_NO_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    const bool emit = triangle_capacity != 0 || vertex_capacity != 0;
    DfMccFilterArgs a;
    memset(&a, 0, sizeof(a));
    a.tris = triangles_dev; a.T = (size_t)n_triangles; a.V = (uint32_t)n_vertices;
    a.label = vertex_label_dev; a.tcount = triangle_count_dev; a.min_triangles = min_triangles; a.keep_largest = keep_largest != 0;
    a.tris_out = triangles_out_dev; a.tcap = triangle_capacity; a.vsrc = vertex_src_dev; a.vcap = vertex_capacity; a.vmap = vertex_map_dev;
    if (!a.T || !a.V) {                                                                  // nothing is valid, nothing is kept
        DF_HIP(hipMemsetAsync(counts_dev, 0, 16, st));
        if (emit && a.vmap && a.V) DF_HIP(hipMemsetAsync(a.vmap, 0xff, (size_t)a.V * 4, st));
        return DF_OK;
    }
    // workspace (zeroed): [best | triangle flags / offsets [T + 1] | vertex flags / offsets [V + 1]], then hipcub's temporary storage
    const size_t V = (size_t)a.V;
    size_t scan_bytes = 0;
    DF_TRY(df_mesh_scan_bytes((a.T > V ? a.T : V) + 1, st, &scan_bytes));
    DfMeshCarve c; c.take(16);                                                           // (best, at the front)
    const size_t o_t = c.take((a.T + 1) * 4, 4), o_v = c.take((V + 1) * 4, 4), zero_bytes = c.total(), o_scan = c.take(scan_bytes, 256);
    DfScratchHold hold(st, c.total());                                                   // held until the last launch is enqueued
    if (!hold.entry) return (int)hipErrorOutOfMemory;
    char* const ws = hold.mem;
    a.best = (unsigned long long*)ws; a.tscan = (uint32_t*)(ws + o_t); a.vscan = (uint32_t*)(ws + o_v);
    DF_HIP(hipMemsetAsync(ws, 0, zero_bytes, st));
    if (a.keep_largest) {
        hipLaunchKernelGGL(df_mcc_best_kernel, dim3(df_mesh_blocks(V, 1024u)), dim3(256), 0, st, a.tcount, V, a.best);
        DF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(df_mcc_keep_kernel, dim3(df_mesh_blocks(a.T, DF_MCC_MAX_BLOCKS)), dim3(256), 0, st, a);
    DF_LAUNCH_CHECK();
    DF_TRY(df_mesh_scan_pair(ws + o_scan, scan_bytes, a.tscan, a.T + 1, a.vscan, V + 1, counts_dev, st));
    if (!emit) return DF_OK;
    if (a.tcap) {
        hipLaunchKernelGGL(df_mcc_compact_triangles_kernel, dim3(df_mesh_blocks(a.T, DF_MCC_MAX_BLOCKS)), dim3(256), 0, st, a);
        DF_LAUNCH_CHECK();
    }
    if (a.vcap || a.vmap) {
        hipLaunchKernelGGL(df_mcc_compact_vertices_kernel, dim3(df_mesh_blocks(V, DF_MCC_MAX_BLOCKS)), dim3(256), 0, st, a);
        DF_LAUNCH_CHECK();
    }
    return DF_OK;
}

// ---- gather: dst row i = src row index[i], rows of W 32-bit words; one lane per word, so a wave's stores are contiguous
template <int W>
__global__ __launch_bounds__(256) void df_mcc_gather_kernel(const uint32_t* src, const uint32_t* index, size_t n_words, uint32_t* dst)
{
    for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < n_words; j += (size_t)gridDim.x * 256) {
        const size_t i = j / W;
        dst[j] = src[(size_t)index[i] * W + (j - i * W)];
    }
}

extern "C" int dfusion_gather_rows(const void* src_dev, unsigned int row_bytes, const unsigned int* index_dev, unsigned long long n, void* dst_dev,
                                   dfStream stream)
{
    if (row_bytes != 4u && row_bytes != 12u && row_bytes != 16u) return DF_E_INVALID;
    if (n && (!src_dev || !index_dev || !dst_dev)) return DF_E_INVALID;
    if (n > (~0ull) / 16ull) return DF_E_INVALID;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return DF_E_NO_DEVICE;
    if (!n) return DF_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t words = (size_t)n * (row_bytes / 4u);
    const dim3 grid(df_mesh_blocks(words, DF_MCC_MAX_BLOCKS));
    if (row_bytes == 4u) hipLaunchKernelGGL(df_mcc_gather_kernel<1>, grid, dim3(256), 0, st, (const uint32_t*)src_dev, index_dev, words, (uint32_t*)dst_dev);
    else if (row_bytes == 12u) hipLaunchKernelGGL(df_mcc_gather_kernel<3>, grid, dim3(256), 0, st, (const uint32_t*)src_dev, index_dev, words, (uint32_t*)dst_dev);
    else hipLaunchKernelGGL(df_mcc_gather_kernel<4>, grid, dim3(256), 0, st, (const uint32_t*)src_dev, index_dev, words, (uint32_t*)dst_dev);
    DF_LAUNCH_CHECK();
    return DF_OK;
}

// ---- the mesh kit's host launchers (dfusion_mesh_kit.h), for every mesh file
__global__ void df_mcc_set_counts_kernel(unsigned long long* counts, int i0, unsigned long long v0, int i1, unsigned long long v1)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) { counts[i0] = v0; counts[i1] = v1; }
}

__global__ void df_mcc_scan_totals_kernel(const uint32_t* a, size_t na, const uint32_t* b, size_t nb, unsigned long long* counts)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) { counts[0] = b[nb - 1]; counts[1] = a[na - 1]; }
}

int df_mesh_set_counts(unsigned long long* counts, int i0, unsigned long long v0, int i1, unsigned long long v1, hipStream_t st)
{
    hipLaunchKernelGGL(df_mcc_set_counts_kernel, dim3(1), dim3(64), 0, st, counts, i0, v0, i1, v1);
    DF_LAUNCH_CHECK();
    return DF_OK;
}

int df_mesh_scan_bytes(size_t items_max, hipStream_t st, size_t* bytes)
{
    DF_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, items_max, st));
    return DF_OK;
}

int df_mesh_scan_pair(char* cub, size_t cub_bytes, uint32_t* a, size_t na, uint32_t* b, size_t nb, unsigned long long* counts, hipStream_t st)
{
    DF_HIP(hipcub::DeviceScan::ExclusiveSum(cub, cub_bytes, a, a, na, st));
    DF_HIP(hipcub::DeviceScan::ExclusiveSum(cub, cub_bytes, b, b, nb, st));
    if (!counts) return DF_OK;
    hipLaunchKernelGGL(df_mcc_scan_totals_kernel, dim3(1), dim3(64), 0, st, (const uint32_t*)a, na, (const uint32_t*)b, nb, counts);
    DF_LAUNCH_CHECK();
    return DF_OK;
}
