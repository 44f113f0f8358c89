// dfusion_color.hip -- the colour volume (no reference counterpart: the reference accepts a colour image and drops it).
// dfusion_color_clear / dfusion_color_integrate / dfusion_color_fetch; the rule -- which voxels take a colour, where they look it up,
// how it is averaged and how a point reads it back -- is stated in include/dfusion.h and DESIGN.md and restated in numpy by
// tests/color_ref.py, against which the bytes are compared.
//
// Colour is wanted in the band around the surface only, so a frame lists that band and works on the list:
//   count   streams the owner planes of the TSDF once (df_mesh_count_kernel's shape: contiguous 16 KiB runs per workgroup, non-temporal
//           16-byte loads, no LDS, no barrier) and leaves the number of selected voxels of every wave-item of 256 x-adjacent voxels.
//   scan    hipcub exclusive sum over the per-item counts (one spare element at the end receives the total).
//   list    every item with selected voxels re-reads its 1 KiB and writes, at its scanned base + ballot / popcount prefix, each selected
//           voxel's stored linear index and its canonical position x_c = vol2world * (x vsx, y vsy, z vsz): ascending linear index,
//           truncated at the capacity.  Nothing a caller sees is ordered by an atomic.
//   warp    dfusion_warp_points over the WHOLE capacity with an identity warp_to_live (1 * x + 0 * y + 0 * z + 0 keeps every finite
//           value): the exact k-NN + DQB of the point path.  The positions were filled with NaN first and the point path skips NaN
//           points, so the tail past the device-side count costs a load and a compare per lane and no host ever reads the count.
//   fuse    one lane per listed voxel: world2cam, the projector and gates of the depth integrate, the occlusion test, the integer
//           running average.  A voxel is in the list once, so it is written by one thread.
#include <hipcub/hipcub.hpp>
#include "dfusion_internal.h"

struct DfColorArgs {
    const uint32_t* vol;               // plane z_own0 of the TSDF
    uint32_t* color;                   // plane z_store0 of the colour volume: {c0, c1, c2, w} bytes, c0 in the low byte
    int X, Y, nz, z_own0, z_off;       // owner planes [z_own0, z_own0 + nz); z_off = z_own0 - z_store0
    float vsx, vsy, vsz, band;
    DfAff vol2world, world2cam;
    size_t n4, n_items;                // lane-items (4 voxels), wave-items (256 voxels)
    unsigned long long* base;          // [n_items + 1] counts, then exclusive sums
    uint32_t* list; float* pos;        // [cap] stored linear index, [3 cap] position of every listed voxel
    unsigned long long cap;
    const unsigned char* rgb; size_t rgb_pitch;
    DfIntegrateParams P;               // dists image + projector (trunc = band * trunc_dist here: the occlusion threshold)
    int max_weight;
    unsigned long long *n_selected, *n_fused;
};

// selected: stored weight > 0 and |tsdf| < band (strict: saturated free space, tsdf = 1 with band = 1, is out; a NaN tsdf is out)
__device__ __forceinline__ bool cl_selected(uint32_t v, float band) { return (v >> 16) != 0u && fabsf(h2f_bits(v)) < band; }
__device__ __forceinline__ unsigned cl_mask4(uint4 c, float band)
{
    return (cl_selected(c.x, band) ? 1u : 0u) | (cl_selected(c.y, band) ? 2u : 0u) | (cl_selected(c.z, band) ? 4u : 0u) | (cl_selected(c.w, band) ? 8u : 0u);
}
// (dfusion_mesh.hip's wave sums, kept local: a shared header of the warped sweep would have to change to hold them)
__device__ __forceinline__ unsigned cl_wave_sum(unsigned v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ unsigned cl_wave_excl(unsigned v, int lane)
{
    unsigned s = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const unsigned t = __shfl_up(s, d, 64); if (lane >= d) s += t; }
    return s - v;
}

// ---- count
template <int U>      // 16-byte loads in flight per lane
__global__ __launch_bounds__(256) void df_color_count_kernel(const DfColorArgs a)
{
    typedef unsigned int df_cl_u4 __attribute__((ext_vector_type(4)));
    const df_cl_u4* base4 = reinterpret_cast<const df_cl_u4*>(a.vol);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t chunk = (size_t)256 * U;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.base[a.n_items] = 0ull;      // the spare element: the scan leaves the total here
    for (size_t c0 = (size_t)blockIdx.x * chunk; c0 < a.n4; c0 += (size_t)gridDim.x * chunk) {
        df_cl_u4 own[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t i = c0 + (size_t)u * 256 + threadIdx.x;
            own[u] = i < a.n4 ? __builtin_nontemporal_load(base4 + i) : df_cl_u4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned n = cl_wave_sum((unsigned)__popc(cl_mask4(make_uint4(own[u].x, own[u].y, own[u].z, own[u].w), a.band)));
            const size_t item = (c0 + (size_t)u * 256 + (size_t)wave * 64) >> 6;
            if (lane == 0 && item < a.n_items) a.base[item] = n;
        }
    }
}

__global__ void df_color_totals_kernel(const unsigned long long* base, size_t n_items, unsigned long long* n_selected, unsigned long long* n_fused)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        if (n_selected) *n_selected = base[n_items];
        if (n_fused) *n_fused = 0ull;
    }
}

// ---- list: a wave looks at 64 consecutive items and works through those that have selected voxels (their scanned bases differ)
__global__ __launch_bounds__(256) void df_color_list_kernel(const DfColorArgs a)
{
    const int lane = threadIdx.x & 63;
    const size_t item0 = ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    if (item0 >= a.n_items) return;
    const size_t i = item0 + (size_t)lane;
    const unsigned long long b0 = i < a.n_items ? a.base[i] : 0ull, b1 = i < a.n_items ? a.base[i + 1] : 0ull;
    unsigned long long todo = __ballot(b1 > b0);
    const size_t plane = (size_t)a.X * a.Y;
    while (todo) {                                                          // wave-uniform
        const int s = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1ull;
        const unsigned long long base = __shfl(b0, s, 64);
        if (base >= a.cap) break;                                           // bases ascend: everything from here on is past the capacity
        const size_t li = (item0 + (size_t)s) * 64 + (size_t)lane;
        const bool act = li < a.n4;
        const uint4 c = act ? *reinterpret_cast<const uint4*>(a.vol + 4 * li) : make_uint4(0u, 0u, 0u, 0u);
        const unsigned m = cl_mask4(c, a.band);
        unsigned long long o = base + cl_wave_excl((unsigned)__popc(m), lane);
        if (m) {
            const size_t v0 = 4 * li;
            const int zr = (int)(v0 / plane);
            const int rem = (int)(v0 - (size_t)zr * plane);
            const int y = rem / a.X, x0 = rem - y * a.X;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!((m >> k) & 1u)) continue;
                if (o < a.cap) {
                    a.list[o] = (uint32_t)((size_t)a.z_off * plane + v0 + (size_t)k);
                    const f3 xc = aff_mul(a.vol2world, mk3((float)(x0 + k) * a.vsx, (float)y * a.vsy, (float)(a.z_own0 + zr) * a.vsz));
                    a.pos[3 * o] = xc.x; a.pos[3 * o + 1] = xc.y; a.pos[3 * o + 2] = xc.z;
                }
                ++o;
            }
        }
    }
}

// ---- fuse
__global__ __launch_bounds__(256) void df_color_fuse_kernel(const DfColorArgs a)
{
    const unsigned long long total = a.base[a.n_items];
    const unsigned long long n = total < a.cap ? total : a.cap;
    const unsigned long long o = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if ((unsigned long long)blockIdx.x * 256ull >= n) return;               // block-uniform
    bool fused = false;
    if (o < n) {
        const f3 xw = mk3(a.pos[3 * o], a.pos[3 * o + 1], a.pos[3 * o + 2]);
        const f3 vc = aff_mul(a.world2cam, xw);
        const DfIntegrateParams& P = a.P;
        const float u = fmaf(P.fx, vc.x / vc.z, P.cx);                      // device.hpp:35
        const float v = fmaf(P.fy, vc.y / vc.z, P.cy);                      // device.hpp:36
        if (u >= 0.f && v >= 0.f && u < (float)P.cols && v < (float)P.rows) {           // tsdf_volume.cu:82 (NaN skips)
            const int ui = (int)u, vi = (int)v;
            const float Dp = h2f_bits(*(const uint16_t*)((const char*)P.dists + (size_t)vi * P.pitch + 2 * (size_t)ui));
            if (!(Dp == 0.f || vc.z <= 0.f)) {                              // :86
                const float sdf = Dp - sqrtf(dot3(vc, vc));                 // :89
                if (fabsf(sdf) < P.trunc) {                                 // observed: not behind what the camera sees, not far in front of it
                    const uint32_t px = *(const uint32_t*)(a.rgb + (size_t)vi * a.rgb_pitch + 4 * (size_t)ui);
                    const uint32_t idx = a.list[o];
                    const uint32_t old = a.color[idx];
                    const uint32_t w = old >> 24, d = w + 1u, r = d >> 1;
                    const uint32_t c0 = ((old & 0xffu) * w + (px & 0xffu) + r) / d;
                    const uint32_t c1 = (((old >> 8) & 0xffu) * w + ((px >> 8) & 0xffu) + r) / d;
                    const uint32_t c2 = (((old >> 16) & 0xffu) * w + ((px >> 16) & 0xffu) + r) / d;
                    const uint32_t wn = min(d, (uint32_t)a.max_weight);
                    a.color[idx] = c0 | (c1 << 8) | (c2 << 16) | (wn << 24);
                    fused = true;
                }
            }
        }
    }
    if (a.n_fused) {
        const unsigned long long who = __ballot(fused);
        if ((threadIdx.x & 63) == 0 && who) atomicAdd(a.n_fused, (unsigned long long)__popcll(who));   // an integer count: any order, one sum
    }
}

// ---- fetch: one lane per point
struct DfColorFetchArgs {
    const uint32_t* color;             // plane z_store0
    int X, Y, z_store0, z_store_n;
    float vsx, vsy, vsz;
    DfAff world2vol;
    const float4* points; unsigned long long n;
    uint32_t* out;
};
__global__ __launch_bounds__(256) void df_color_fetch_kernel(const DfColorFetchArgs a)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (i >= a.n) return;
    const float4 q = a.points[i];
    uint32_t out = 0u;
    const float inf = __uint_as_float(0x7f800000u);
    if (fabsf(q.x) < inf && fabsf(q.y) < inf && fabsf(q.z) < inf) {          // finite (NaN compares false)
        const f3 p = aff_mul(a.world2vol, mk3(q.x, q.y, q.z));
        const float cfx = p.x / a.vsx, cfy = p.y / a.vsy, cfz = p.z / a.vsz;
        const float gx = floorf(cfx), gy = floorf(cfy), gz = floorf(cfz);
        const float fa = cfx - gx, fb = cfy - gy, fc = cfz - gz;
        const size_t plane = (size_t)a.X * a.Y;
        float sw = 0.f, sc0 = 0.f, sc1 = 0.f, sc2 = 0.f;
#pragma unroll
        for (int t = 0; t < 8; ++t) {                                        // the oracle's interpolate order: z fastest, then y, then x
            const int dx = t >> 2, dy = (t >> 1) & 1, dz = t & 1;
            const float tx = gx + (float)dx, ty = gy + (float)dy, tz = gz + (float)dz;
            const bool in = tx >= 0.f && tx < (float)a.X && ty >= 0.f && ty < (float)a.Y &&
                            tz >= (float)a.z_store0 && tz < (float)(a.z_store0 + a.z_store_n);
            if (!in) continue;
            const uint32_t c = a.color[(size_t)((int)tz - a.z_store0) * plane + (size_t)(int)ty * a.X + (size_t)(int)tx];
            if (!(c >> 24)) continue;
            const float wt = ((dx ? fa : 1.f - fa) * (dy ? fb : 1.f - fb)) * (dz ? fc : 1.f - fc);
            sw += wt;
            sc0 += (float)(c & 0xffu) * wt; sc1 += (float)((c >> 8) & 0xffu) * wt; sc2 += (float)((c >> 16) & 0xffu) * wt;
        }
        if (sw > 0.f) {
            const uint32_t r0 = (uint32_t)min(255, (int)floorf(sc0 / sw + 0.5f));
            const uint32_t r1 = (uint32_t)min(255, (int)floorf(sc1 / sw + 0.5f));
            const uint32_t r2 = (uint32_t)min(255, (int)floorf(sc2 / sw + 0.5f));
            out = r0 | (r1 << 8) | (r2 << 16) | 0xff000000u;
        }
    }
    a.out[i] = out;
}

// ---- host
extern "C" int dfusion_color_clear(void* color, DfVolume g, const DfSlab* slab, dfStream stream)
{
    g.data = color;                                                         // (the geometry's own blob is not looked at)
    if (!color || !df_volume_valid(g)) return DF_E_INVALID;
    const DfSlab s = df_slab_or_full(g, slab);
    if (!df_slab_valid(g, s)) return DF_E_INVALID;
    DF_HIP(hipMemsetAsync(color, 0, (size_t)g.dims[0] * g.dims[1] * (size_t)s.z_store_n * 4, (hipStream_t)stream));
    return DF_OK;
}

extern "C" int dfusion_color_integrate(const unsigned char* rgb, size_t rgb_pitch, const uint16_t* dists, size_t dists_pitch, int cols, int rows,
                                       DfVolume v, const DfSlab* slab, void* color, const float vol2world[12], const float world2cam[12],
                                       const float proj[4], DfWarpField* wf, int k, float band, int max_weight, long long capacity,
                                       unsigned long long* n_selected, unsigned long long* n_fused, dfStream stream)
{
    if (!rgb || !dists || !color || !vol2world || !world2cam || !proj || !df_volume_valid(v)) return DF_E_INVALID;
    if (!df_pitch_ok(rgb_pitch, cols, 4) || !df_pitch_ok(dists_pitch, cols, 2) || rows <= 0) return DF_E_INVALID;
    if (((uintptr_t)rgb | rgb_pitch) & 3u) return DF_E_INVALID;                                 // (a pixel is read as one 32-bit word)
    if (!(band > 0.f && band <= 1.f) || max_weight < 1 || max_weight > 255 || capacity <= 0) return DF_E_INVALID;
    if (wf && (k < 1 || k > 8 || wf->M < k)) return DF_E_INVALID;
    if (capacity > 0x7fffffffll) capacity = 0x7fffffffll;                   // (the point path counts in int)
    const DfSlab s = df_slab_or_full(v, slab);
    if (!df_slab_valid(v, s)) return DF_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    DfColorArgs a;
    memset(&a, 0, sizeof(a));
    a.X = v.dims[0]; a.Y = v.dims[1]; a.nz = s.z_own_n; a.z_own0 = s.z_own0; a.z_off = s.z_own0 - s.z_store0;
    const size_t plane = (size_t)a.X * a.Y;
    if (plane * (size_t)s.z_store_n > 0xffffffffull) return DF_E_INVALID;   // (listed indices are 32-bit)
    a.n_selected = n_selected; a.n_fused = n_fused;
    if (a.nz == 0) {
        if (n_selected) DF_HIP(hipMemsetAsync(n_selected, 0, 8, st));
        if (n_fused) DF_HIP(hipMemsetAsync(n_fused, 0, 8, st));
        return DF_OK;
    }
    a.vol = (const uint32_t*)v.data + (size_t)a.z_off * plane;
    a.color = (uint32_t*)color;
    a.vsx = v.voxel_size[0]; a.vsy = v.voxel_size[1]; a.vsz = v.voxel_size[2]; a.band = band;
    a.vol2world = df_aff(vol2world); a.world2cam = df_aff(world2cam);
    a.n4 = plane * (size_t)a.nz / 4;
    a.n_items = (a.n4 + 63) / 64;
    if (a.n_items + 1 > 0x7fffffffull) return DF_E_INVALID;
    a.cap = (unsigned long long)capacity;
    if (a.cap > 4ull * a.n4) a.cap = 4ull * a.n4;                           // (no more voxels than there are)
    a.rgb = rgb; a.rgb_pitch = rgb_pitch;
    a.P.dists = dists; a.P.pitch = dists_pitch; a.P.cols = cols; a.P.rows = rows;
    a.P.fx = proj[0]; a.P.fy = proj[1]; a.P.cx = proj[2]; a.P.cy = proj[3];
    a.P.trunc = band * v.trunc_dist; a.P.trunc_inv = 0.f; a.P.max_weight = max_weight;
    a.max_weight = max_weight;
    // workspace: [per-item counts / bases | list | positions], hipcub's temporary storage
    size_t scan_bytes = 0;
    DF_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (int)(a.n_items + 1), st));
    const size_t o_list = ((a.n_items + 1) * 8 + 255) / 256 * 256, o_pos = (o_list + (size_t)a.cap * 4 + 255) / 256 * 256;
    const size_t o_scan = (o_pos + (size_t)a.cap * 12 + 255) / 256 * 256;
    DfScratchHold hold(st, o_scan + scan_bytes);                            // held until the last launch is enqueued
    if (!hold.entry) return (int)hipErrorOutOfMemory;
    char* const ws = hold.mem;
    a.base = (unsigned long long*)ws; a.list = (uint32_t*)(ws + o_list); a.pos = (float*)(ws + o_pos);
    const int U = 4;
    size_t blocks = (a.n4 + 256 * U - 1) / (256 * U);
    if (blocks > 256 * 32) blocks = 256 * 32;
    hipLaunchKernelGGL(df_color_count_kernel<U>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    DF_LAUNCH_CHECK();
    DF_HIP(hipcub::DeviceScan::ExclusiveSum(ws + o_scan, scan_bytes, a.base, a.base, (int)(a.n_items + 1), st));
    hipLaunchKernelGGL(df_color_totals_kernel, dim3(1), dim3(64), 0, st, a.base, a.n_items, n_selected, n_fused);
    DF_LAUNCH_CHECK();
    if (wf) DF_HIP(hipMemsetAsync(a.pos, 0xff, (size_t)a.cap * 12, st));    // NaN: what the point path skips past the listed voxels
    hipLaunchKernelGGL(df_color_list_kernel, dim3((unsigned)((a.n_items + 255) / 256)), dim3(256), 0, st, a);
    DF_LAUNCH_CHECK();
    if (wf) {
        const float ident[12] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
        const int rc = dfusion_warp_points(wf, k, a.pos, nullptr, (int)a.cap, ident, stream);
        if (rc != DF_OK) return rc;
    }
    hipLaunchKernelGGL(df_color_fuse_kernel, dim3((unsigned)((a.cap + 255) / 256)), dim3(256), 0, st, a);
    DF_LAUNCH_CHECK();
    return DF_OK;
}

extern "C" int dfusion_color_fetch(const void* color, DfVolume g, const DfSlab* slab, const float world2vol[12], const float* points,
                                   unsigned long long n, unsigned char* rgba_out, dfStream stream)
{
    g.data = const_cast<void*>(color);
    if (!color || !world2vol || !df_volume_valid(g) || (n && (!points || !rgba_out))) return DF_E_INVALID;
    const DfSlab s = df_slab_or_full(g, slab);
    if (!df_slab_valid(g, s)) return DF_E_INVALID;
    if (n == 0) return DF_OK;
    if ((n + 255) / 256 > 0x7fffffffull) return DF_E_INVALID;
    DfColorFetchArgs a;
    a.color = (const uint32_t*)color; a.X = g.dims[0]; a.Y = g.dims[1]; a.z_store0 = s.z_store0; a.z_store_n = s.z_store_n;
    a.vsx = g.voxel_size[0]; a.vsy = g.voxel_size[1]; a.vsz = g.voxel_size[2];
    a.world2vol = df_aff(world2vol);
    a.points = (const float4*)points; a.n = n; a.out = (uint32_t*)rgba_out;
    hipLaunchKernelGGL(df_color_fetch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    DF_LAUNCH_CHECK();
    return DF_OK;
}
