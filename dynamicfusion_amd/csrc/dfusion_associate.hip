// dfusion_associate.hip -- dfusion_associate_projective: projective data association for the warp solve (no reference counterpart: the
// reference's loop pairs ray-cast point i with live point i).  Every predicted (warped) point is paired with the live sample at the
// pixel it projects to, visible surface only; the rule -- seven tests in a fixed order, the first failing one names the status -- is
// stated in include/dfusion.h and DESIGN.md section 15 and restated in numpy by tests/associate_ref.py, against which live_out, status
// and counts are compared bit for bit.  The projection and its bounds are fe_find_coresp's (dfusion_frontend.hip).
//
//   fill     the cols x rows depth buffer (u32, in the per-(device, stream) scratch) <- 0xffffffff
//   splat    one lane per point: a point that passes tests 1-3 does an integer atomicMin of the bits of p.z at its pixel (positive
//            floats order as their bits; no value comes back, so the compiler emits the no-return form)
//   resolve  one lane per point: projects again (the same operations give the same pixel, no pixel index is stored), runs tests 4-7,
//            gathers the live sample, writes live_out / status and counts the statuses (ballot + popcount per wave, summed per
//            workgroup, one integer atomic add per workgroup and status)
// A negative occlusion margin runs resolve alone.  No float atomics, and a minimum does not depend on the order of its operands: the
// output does not depend on scheduling.
#include "dfusion_internal.h"

struct DfAssocArgs {
    const float* pts; const float* nrm; int N;          // packed float3; nrm nullable
    const char* lp; size_t lp_pitch;                    // live points, float4 image
    const char* ln; size_t ln_pitch;                    // live normals (with nrm)
    int cols, rows;
    float fx, fy, cx, cy;
    float dist2, min_cosine, margin;
    uint32_t* zbuf;                                     // [rows * cols] bits of the smallest p.z per pixel (margin >= 0)
    float* out; unsigned char* status; unsigned long long* counts;
};

__device__ __forceinline__ bool as_finite3(f3 a)
{
    const uint32_t e = 0x7f800000u;
    return ((__float_as_uint(a.x) & e) != e) & ((__float_as_uint(a.y) & e) != e) & ((__float_as_uint(a.z) & e) != e);
}

// tests 1-3: 0 = the point falls on pixel (ui, vi), else the status.  p (and n, with normals) are loaded either way.
__device__ __forceinline__ int as_project(const DfAssocArgs& A, int i, f3* p, f3* n, int* ui, int* vi)
{
    const float* pp = A.pts + (size_t)i * 3;
    *p = mk3(pp[0], pp[1], pp[2]);
    bool fin = as_finite3(*p);
    if (A.nrm) {
        const float* np = A.nrm + (size_t)i * 3;
        *n = mk3(np[0], np[1], np[2]);
        fin = fin & as_finite3(*n);
    }
    if (!fin) return 1;
    if (!(p->z > 0.f)) return 2;
    const float u = fmaf(A.fx, p->x / p->z, A.cx);                      // fe_find_coresp's projection and bounds
    const float v = fmaf(A.fy, p->y / p->z, A.cy);
    if (!(u >= 0.f && v >= 0.f && u < (float)A.cols && v < (float)A.rows)) return 3;
    *ui = (int)u; *vi = (int)v;
    return 0;
}

__global__ __launch_bounds__(256) void df_assoc_fill_kernel(uint4* zbuf4, size_t n4)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n4) zbuf4[i] = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
}

__global__ __launch_bounds__(256) void df_assoc_splat_kernel(const DfAssocArgs A)
{
    const size_t gi = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (gi >= (size_t)A.N) return;
    f3 p, n; int ui, vi;
    if (as_project(A, (int)gi, &p, &n, &ui, &vi)) return;
    atomicMin(A.zbuf + ((size_t)vi * A.cols + ui), __float_as_uint(p.z));
}

// Every workgroup walks the points in steps of the grid (DF_ASSOC_RESOLVE_BLOCKS workgroups at most): the statuses are counted per wave
// (ballot + popcount, in wave-uniform registers over the whole walk), summed per workgroup in LDS, and leave as one integer atomic add
// per workgroup and status -- a few thousand adds on one 64-byte line instead of one per wave and status (14 400 at 307 200 points,
// which serialise in the L2: the first trace of this kernel showed 167 us, nearly all of it those adds).
#define DF_ASSOC_RESOLVE_BLOCKS 512u
__global__ __launch_bounds__(256) void df_assoc_resolve_kernel(const DfAssocArgs A)
{
    __shared__ unsigned int s_cnt[8];
    if (threadIdx.x < 8) s_cnt[threadIdx.x] = 0u;
    unsigned int wcnt[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};             // wave-uniform
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t g0 = (size_t)blockIdx.x * 256; g0 < (size_t)A.N; g0 += stride) {     // (workgroup-uniform trip count)
        const size_t gi = g0 + threadIdx.x;
        int st = 8;                                                      // (no point: counted nowhere)
        if (gi < (size_t)A.N) {
            f3 p, n; int ui, vi;
            f3 q = mk3(0.f, 0.f, 0.f);
            st = as_project(A, (int)gi, &p, &n, &ui, &vi);
            if (!st && A.margin >= 0.f) {
                const float zmin = __uint_as_float(A.zbuf[(size_t)vi * A.cols + ui]);
                if (p.z - zmin > A.margin) st = 4;
            }
            if (!st) {
                const float4 q4 = *reinterpret_cast<const float4*>(A.lp + (size_t)vi * A.lp_pitch + (size_t)ui * 16);
                q = mk3(q4.x, q4.y, q4.z);
                const f3 d = sub3(p, q);
                if (isnan(q.x)) st = 5;
                else if (dot3(d, d) > A.dist2) st = 6;
                else if (A.nrm) {
                    const float4 l4 = *reinterpret_cast<const float4*>(A.ln + (size_t)vi * A.ln_pitch + (size_t)ui * 16);
                    if (!(fabsf(dot3(n, mk3(l4.x, l4.y, l4.z))) >= A.min_cosine)) st = 7;
                }
            }
            if (st) q = mk3(qnanf_(), qnanf_(), qnanf_());
            float* o = A.out + gi * 3;
            o[0] = q.x; o[1] = q.y; o[2] = q.z;
            if (A.status) A.status[gi] = (unsigned char)st;
        }
        if (A.counts) {
#pragma unroll
            for (int s = 0; s < 8; ++s) wcnt[s] += (unsigned int)__popcll(__ballot(st == s));
        }
    }
    if (!A.counts) return;                                               // (uniform: a kernel argument)
    __syncthreads();                                                     // s_cnt is zero
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int s = 0; s < 8; ++s) if (wcnt[s]) atomicAdd(&s_cnt[s], wcnt[s]);
    }
    __syncthreads();
    if (threadIdx.x < 8 && s_cnt[threadIdx.x]) atomicAdd(A.counts + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
}

extern "C" int dfusion_associate_projective(const float* points_dev, const float* normals_dev, int N, const float* live_points_dev,
                                            size_t live_points_pitch, const float* live_normals_dev, size_t live_normals_pitch, int cols,
                                            int rows, const float intr[4], float dist_thres, float min_cosine, float occlusion_margin,
                                            float* live_out_dev, unsigned char* status_dev, unsigned long long* counts_dev, dfStream stream)
{
    if (N < 0 || cols <= 0 || rows <= 0 || !intr) return DF_E_INVALID;
    if ((normals_dev == nullptr) != (live_normals_dev == nullptr)) return DF_E_INVALID;
    if (!df_pitch_ok(live_points_pitch, cols, 16) || (live_normals_dev && !df_pitch_ok(live_normals_pitch, cols, 16))) return DF_E_INVALID;
    if (!(dist_thres >= 0.f) || min_cosine != min_cosine) return DF_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {
        if (counts_dev) DF_HIP(hipMemsetAsync(counts_dev, 0, 64, st));
        return DF_OK;
    }
    if (!points_dev || !live_points_dev || !live_out_dev) return DF_E_INVALID;
    DfAssocArgs a;
    memset(&a, 0, sizeof(a));
    a.pts = points_dev; a.nrm = normals_dev; a.N = N;
    a.lp = (const char*)live_points_dev; a.lp_pitch = live_points_pitch;
    a.ln = (const char*)live_normals_dev; a.ln_pitch = live_normals_pitch;
    a.cols = cols; a.rows = rows;
    a.fx = intr[0]; a.fy = intr[1]; a.cx = intr[2]; a.cy = intr[3];
    a.dist2 = dist_thres * dist_thres; a.min_cosine = min_cosine; a.margin = occlusion_margin;
    a.out = live_out_dev; a.status = status_dev; a.counts = counts_dev;
    const unsigned blocks = (unsigned)(((size_t)N + 255) / 256);
    const unsigned rblocks = blocks < DF_ASSOC_RESOLVE_BLOCKS ? blocks : DF_ASSOC_RESOLVE_BLOCKS;
    if (counts_dev) DF_HIP(hipMemsetAsync(counts_dev, 0, 64, st));
    if (!(occlusion_margin >= 0.f)) {                                    // the occlusion test is off (a NaN margin never rejects either)
        a.margin = -1.f;
        hipLaunchKernelGGL(df_assoc_resolve_kernel, dim3(rblocks), dim3(256), 0, st, a);
        DF_LAUNCH_CHECK();
        return DF_OK;
    }
    const size_t n4 = ((size_t)cols * (size_t)rows + 3) / 4;
    DfScratchHold hold(st, n4 * 16);                                     // held until the last launch is enqueued
    if (!hold.entry) return (int)hipErrorOutOfMemory;
    a.zbuf = (uint32_t*)hold.mem;
    hipLaunchKernelGGL(df_assoc_fill_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, (uint4*)hold.mem, n4);
    DF_LAUNCH_CHECK();
    hipLaunchKernelGGL(df_assoc_splat_kernel, dim3(blocks), dim3(256), 0, st, a);
    DF_LAUNCH_CHECK();
    hipLaunchKernelGGL(df_assoc_resolve_kernel, dim3(rblocks), dim3(256), 0, st, a);
    DF_LAUNCH_CHECK();
    return DF_OK;
}
