// dfusion_render.hip -- dfusion_render_mesh: a z-buffered rasteriser of a triangle mesh into a pinhole camera (no reference counterpart:
// the reference shows the ray-cast of the canonical volume only).  It gives the vertex map, normal map, colour image, an interpolated
// per-vertex attribute (the canonical positions) and the winning triangle of every pixel; every output point lies on its pixel's ray.
// The rule -- vertices snapped to 1/16 pixel, integer edge functions, inclusive coverage, 64-bit {z bits, triangle} keys -- is stated in
// include/dfusion.h and DESIGN.md section 19 and restated in numpy by tests/render_ref.py, against which every output is compared bit
// for bit.
//
//   fill     the cols x rows key buffer (u64, in the per-(device, stream) scratch) <- all ones
//   raster   one lane per triangle (workgroups walk the triangles in steps of the grid): the three vertices are gathered and projected
//            PER TRIANGLE (three 16-byte loads; no vertex pass, no V-sized buffer), the statuses are decided -- the stretch test before
//            the loop, so that the loop visits at most (max_extent + 1)^2 samples -- and every covered sample does a 64-bit integer
//            atomicMin of (bits(z) << 32) | t at its pixel (no value comes back: the no-return form).  Counts the statuses.
//   resolve  one lane per pixel: z and t come out of the key, the triangle is projected again (the same operations give the same bits)
//            and the outputs are interpolated.  Counts the covered pixels.
// Counts as in dfusion_associate.hip: ballot + popcount per wave, summed per workgroup, one integer atomic add per workgroup and entry.
// No float atomics, and a minimum does not depend on the order of its operands: the output does not depend on scheduling.
#include "dfusion_internal.h"

struct DfRenderArgs {
    const float4* vtx; const uint32_t* tri; uint32_t V, T;
    DfAff w2c; int has_w2c;
    const float4* nrm; const float4* attr; const uchar4* col;      // per vertex, nullable
    int cols, rows;
    float fx, fy, cx, cy;
    int ext16;                                                      // 16 * max_extent
    unsigned long long* keys;                                       // [rows * cols]
    char* out_p; size_t p_pitch;                                    // float4
    char* out_n; size_t n_pitch;                                    // float4, nullable
    char* out_a; size_t a_pitch;                                    // float4, nullable
    char* out_c; size_t c_pitch;                                    // 4 bytes, nullable
    char* out_t; size_t t_pitch;                                    // i32, nullable
    unsigned long long* counts;                                     // [6], nullable
};

struct RnVert { int X, Y; float iz; };
struct RnTri { uint32_t i[3]; RnVert v[3]; int area2; int x0, x1, y0, y1; };

// the rule's "Vertex": false = invalid
__device__ __forceinline__ bool rn_vertex(const DfRenderArgs& A, uint32_t i, RnVert* o)
{
    const float4 v4 = A.vtx[i];
    f3 pc = mk3(v4.x, v4.y, v4.z);
    if (A.has_w2c) pc = aff_mul(A.w2c, pc);
    const uint32_t e = 0x7f800000u;
    const bool fin = ((__float_as_uint(pc.x) & e) != e) & ((__float_as_uint(pc.y) & e) != e) & ((__float_as_uint(pc.z) & e) != e);
    if (!fin || !(pc.z > 0.f)) return false;
    const float u = fmaf(A.fx, pc.x / pc.z, A.cx);
    const float v = fmaf(A.fy, pc.y / pc.z, A.cy);
    if (!(fabsf(u) < 65536.f && fabsf(v) < 65536.f)) return false;
    o->X = (int)rintf(16.f * u);
    o->Y = (int)rintf(16.f * v);
    o->iz = 1.f / pc.z;
    return true;
}

// the rule's "Triangle": the status, and for status 0 the (oriented) triangle and its clamped box
__device__ __forceinline__ int rn_triangle(const DfRenderArgs& A, uint32_t t, RnTri* o)
{
    const uint32_t* ip = A.tri + (size_t)t * 3;
    o->i[0] = ip[0]; o->i[1] = ip[1]; o->i[2] = ip[2];
    if (o->i[0] >= A.V || o->i[1] >= A.V || o->i[2] >= A.V) return 1;                  // before any vertex is read
    const bool ok0 = rn_vertex(A, o->i[0], &o->v[0]), ok1 = rn_vertex(A, o->i[1], &o->v[1]), ok2 = rn_vertex(A, o->i[2], &o->v[2]);
    if (!(ok0 && ok1 && ok2)) return 1;
    const RnVert a = o->v[0], b = o->v[1], c = o->v[2];
    const long long area2 = (long long)(b.X - a.X) * (long long)(c.Y - a.Y) - (long long)(c.X - a.X) * (long long)(b.Y - a.Y);
    if (area2 == 0) return 2;
    const int minX = min(a.X, min(b.X, c.X)), maxX = max(a.X, max(b.X, c.X));
    const int minY = min(a.Y, min(b.Y, c.Y)), maxY = max(a.Y, max(b.Y, c.Y));
    if (maxX - minX > A.ext16 || maxY - minY > A.ext16) return 3;                       // (from here on |area2| <= 2^21)
    o->x0 = max((minX + 15) >> 4, 0); o->x1 = min(maxX >> 4, A.cols - 1);               // ceil / floor of signed integers
    o->y0 = max((minY + 15) >> 4, 0); o->y1 = min(maxY >> 4, A.rows - 1);
    if (o->x0 > o->x1 || o->y0 > o->y1) return 4;
    o->area2 = (int)area2;
    if (area2 < 0) {
        const uint32_t ti = o->i[1]; o->i[1] = o->i[2]; o->i[2] = ti;
        o->v[1] = c; o->v[2] = b;
        o->area2 = -(int)area2;
    }
    return 0;
}

// the three edge functions at sample (x, y); covered iff all are >= 0
__device__ __forceinline__ void rn_edges(const RnTri& R, int x, int y, int* w0, int* w1, int* w2)
{
    const int px = 16 * x, py = 16 * y;
    const RnVert a = R.v[0], b = R.v[1], c = R.v[2];
    *w0 = (c.X - b.X) * (py - b.Y) - (c.Y - b.Y) * (px - b.X);
    *w1 = (a.X - c.X) * (py - c.Y) - (a.Y - c.Y) * (px - c.X);
    *w2 = (b.X - a.X) * (py - a.Y) - (b.Y - a.Y) * (px - a.X);
}

__global__ __launch_bounds__(256) void df_render_fill_kernel(uint4* keys4, size_t n4)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n4) keys4[i] = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
}

#define DF_RENDER_RASTER_BLOCKS 2048u
#define DF_RENDER_RESOLVE_BLOCKS 512u
__global__ __launch_bounds__(256) void df_render_raster_kernel(const DfRenderArgs A)
{
    __shared__ unsigned int s_cnt[5];
    if (threadIdx.x < 5) s_cnt[threadIdx.x] = 0u;
    unsigned int wcnt[5] = {0u, 0u, 0u, 0u, 0u};                          // wave-uniform
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t g0 = (size_t)blockIdx.x * 256; g0 < (size_t)A.T; g0 += stride) {      // (workgroup-uniform trip count)
        const size_t gi = g0 + threadIdx.x;
        int st = 5;                                                       // (no triangle: counted nowhere)
        if (gi < (size_t)A.T) {
            RnTri R;
            st = rn_triangle(A, (uint32_t)gi, &R);
            if (!st) {
                const float fa = (float)R.area2;
                for (int y = R.y0; y <= R.y1; ++y)
                    for (int x = R.x0; x <= R.x1; ++x) {                  // at most (max_extent + 1)^2 samples
                        int w0, w1, w2;
                        rn_edges(R, x, y, &w0, &w1, &w2);
                        if ((w0 | w1 | w2) < 0) continue;
                        const float b0 = (float)w0 / fa, b1 = (float)w1 / fa, b2 = (float)w2 / fa;
                        const float iz = (b0 * R.v[0].iz + b1 * R.v[1].iz) + b2 * R.v[2].iz;
                        const float z = 1.f / iz;
                        if (!(z > 0.f) || (__float_as_uint(z) & 0x7f800000u) == 0x7f800000u) continue;
                        const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)gi;
                        atomicMin(A.keys + ((size_t)y * A.cols + x), key);
                    }
            }
        }
        if (A.counts) {
#pragma unroll
            for (int s = 0; s < 5; ++s) wcnt[s] += (unsigned int)__popcll(__ballot(st == s));
        }
    }
    if (!A.counts) return;                                                // (uniform: a kernel argument)
    __syncthreads();                                                      // s_cnt is zero
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int s = 0; s < 5; ++s) if (wcnt[s]) atomicAdd(&s_cnt[s], wcnt[s]);
    }
    __syncthreads();
    if (threadIdx.x < 5 && s_cnt[threadIdx.x]) atomicAdd(A.counts + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
}

__device__ __forceinline__ float rn_mix(float c0, float c1, float c2, float a0, float a1, float a2) { return (c0 * a0 + c1 * a1) + c2 * a2; }
__device__ __forceinline__ unsigned char rn_byte(float f) { const int q = (int)floorf(f + 0.5f); return (unsigned char)(q < 255 ? q : 255); }

__global__ __launch_bounds__(256) void df_render_resolve_kernel(const DfRenderArgs A)
{
    __shared__ unsigned int s_cnt;
    if (threadIdx.x == 0) s_cnt = 0u;
    unsigned int wcnt = 0u;                                               // wave-uniform
    const size_t npix = (size_t)A.cols * (size_t)A.rows;
    const size_t stride = (size_t)gridDim.x * 256;
    const float qn = qnanf_();
    for (size_t g0 = (size_t)blockIdx.x * 256; g0 < npix; g0 += stride) { // (workgroup-uniform trip count)
        const size_t gi = g0 + threadIdx.x;
        bool hit = false;
        if (gi < npix) {
            const int y = (int)(gi / (size_t)A.cols), x = (int)(gi - (size_t)y * A.cols);
            const unsigned long long key = A.keys[gi];
            float4 op = make_float4(qn, qn, qn, qn), on = op, oa = op;    // a miss: what dfusion_raycast_points writes
            uchar4 oc = make_uchar4(0, 0, 0, 0);
            int ot = -1;
            RnTri R;
            // (a key is only ever written for a triangle of status 0, so the indices are in range and the status is 0 again)
            if (key != ~0ull && rn_triangle(A, (uint32_t)key, &R) == 0) {
                hit = true;
                ot = (int)(uint32_t)key;
                const float z = __uint_as_float((uint32_t)(key >> 32));
                int w0, w1, w2;
                rn_edges(R, x, y, &w0, &w1, &w2);
                const float fa = (float)R.area2;
                const float c0 = (((float)w0 / fa) * R.v[0].iz) * z, c1 = (((float)w1 / fa) * R.v[1].iz) * z, c2 = (((float)w2 / fa) * R.v[2].iz) * z;
                op = make_float4(((float)x - A.cx) / A.fx * z, ((float)y - A.cy) / A.fy * z, z, 0.f);
                if (A.out_a) {
                    const float4 a0 = A.attr[R.i[0]], a1 = A.attr[R.i[1]], a2 = A.attr[R.i[2]];
                    oa = make_float4(rn_mix(c0, c1, c2, a0.x, a1.x, a2.x), rn_mix(c0, c1, c2, a0.y, a1.y, a2.y), rn_mix(c0, c1, c2, a0.z, a1.z, a2.z), 0.f);
                }
                if (A.out_n) {
                    const float4 n0 = A.nrm[R.i[0]], n1 = A.nrm[R.i[1]], n2 = A.nrm[R.i[2]];
                    const f3 m = mk3(rn_mix(c0, c1, c2, n0.x, n1.x, n2.x), rn_mix(c0, c1, c2, n0.y, n1.y, n2.y), rn_mix(c0, c1, c2, n0.z, n1.z, n2.z));
                    const float l2 = dot3(m, m);
                    if (l2 > 0.f) { const float l = sqrtf(l2); on = make_float4(m.x / l, m.y / l, m.z / l, 0.f); }
                }
                if (A.out_c) {
                    const uchar4 k0 = A.col[R.i[0]], k1 = A.col[R.i[1]], k2 = A.col[R.i[2]];
                    oc = make_uchar4(rn_byte(rn_mix(c0, c1, c2, (float)k0.x, (float)k1.x, (float)k2.x)), rn_byte(rn_mix(c0, c1, c2, (float)k0.y, (float)k1.y, (float)k2.y)),
                                     rn_byte(rn_mix(c0, c1, c2, (float)k0.z, (float)k1.z, (float)k2.z)), 255);
                }
            }
            *reinterpret_cast<float4*>(A.out_p + (size_t)y * A.p_pitch + (size_t)x * 16) = op;
            if (A.out_n) *reinterpret_cast<float4*>(A.out_n + (size_t)y * A.n_pitch + (size_t)x * 16) = on;
            if (A.out_a) *reinterpret_cast<float4*>(A.out_a + (size_t)y * A.a_pitch + (size_t)x * 16) = oa;
            if (A.out_c) *reinterpret_cast<uchar4*>(A.out_c + (size_t)y * A.c_pitch + (size_t)x * 4) = oc;
            if (A.out_t) *reinterpret_cast<int*>(A.out_t + (size_t)y * A.t_pitch + (size_t)x * 4) = ot;
        }
        if (A.counts) wcnt += (unsigned int)__popcll(__ballot(hit));
    }
    if (!A.counts) return;                                                // (uniform: a kernel argument)
    __syncthreads();                                                      // s_cnt is zero
    if ((threadIdx.x & 63) == 0 && wcnt) atomicAdd(&s_cnt, wcnt);
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(A.counts + 5, (unsigned long long)s_cnt);
}

static inline bool rn_image_ok(const void* p, size_t pitch, int cols, size_t bpp)
{
    return df_pitch_ok(pitch, cols, bpp) && (pitch % bpp) == 0 && ((uintptr_t)p % bpp) == 0;
}

extern "C" int dfusion_render_mesh(const float* vertices_dev, unsigned long long V, const unsigned int* triangles_dev, unsigned long long T,
                                   const float world2cam[12], const float* normals_dev, const float* attr_dev, const unsigned char* colors_dev,
                                   int cols, int rows, const float intr[4], int max_extent, float* points_out, size_t points_pitch,
                                   float* normals_out, size_t normals_pitch, float* attr_out, size_t attr_pitch, unsigned char* colors_out,
                                   size_t colors_pitch, int* tri_out, size_t tri_pitch, unsigned long long* counts_dev, dfStream stream)
{
    if (cols <= 0 || rows <= 0 || !intr || !points_out) return DF_E_INVALID;
    if (max_extent < 1 || max_extent > 64) return DF_E_INVALID;
    if (V > 0xffffffffull || T > 0xffffffffull) return DF_E_INVALID;
    if ((V && !vertices_dev) || (T && !triangles_dev)) return DF_E_INVALID;
    const uint32_t e = 0x7f800000u;
    for (int i = 0; i < 4; ++i) {
        uint32_t b; memcpy(&b, intr + i, 4);
        if ((b & e) == e) return DF_E_INVALID;
    }
    if (intr[0] == 0.f || intr[1] == 0.f) return DF_E_INVALID;
    if (!rn_image_ok(points_out, points_pitch, cols, 16)) return DF_E_INVALID;
    if (normals_out && !rn_image_ok(normals_out, normals_pitch, cols, 16)) return DF_E_INVALID;
    if (attr_out && !rn_image_ok(attr_out, attr_pitch, cols, 16)) return DF_E_INVALID;
    if (colors_out && !rn_image_ok(colors_out, colors_pitch, cols, 4)) return DF_E_INVALID;
    if (tri_out && !rn_image_ok(tri_out, tri_pitch, cols, 4)) return DF_E_INVALID;
    const bool draw = V != 0 && T != 0;
    // an output image needs its per-vertex input (nothing to interpolate otherwise)
    if (draw && ((normals_out && !normals_dev) || (attr_out && !attr_dev) || (colors_out && !colors_dev))) return DF_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    DfRenderArgs a;
    memset(&a, 0, sizeof(a));
    a.vtx = (const float4*)vertices_dev; a.tri = triangles_dev; a.V = (uint32_t)V; a.T = draw ? (uint32_t)T : 0u;
    if (world2cam) { a.w2c = df_aff(world2cam); a.has_w2c = 1; }
    a.nrm = (const float4*)normals_dev; a.attr = (const float4*)attr_dev; a.col = (const uchar4*)colors_dev;
    a.cols = cols; a.rows = rows;
    a.fx = intr[0]; a.fy = intr[1]; a.cx = intr[2]; a.cy = intr[3];
    a.ext16 = 16 * max_extent;
    a.out_p = (char*)points_out; a.p_pitch = points_pitch;
    a.out_n = (char*)normals_out; a.n_pitch = normals_pitch;
    a.out_a = (char*)attr_out; a.a_pitch = attr_pitch;
    a.out_c = (char*)colors_out; a.c_pitch = colors_pitch;
    a.out_t = (char*)tri_out; a.t_pitch = tri_pitch;
    a.counts = counts_dev;
    const size_t npix = (size_t)cols * (size_t)rows;
    const size_t n4 = (npix + 1) / 2;
    DfScratchHold hold(st, n4 * 16);                                     // held until the last launch is enqueued
    if (!hold.entry) return (int)hipErrorOutOfMemory;
    a.keys = (unsigned long long*)hold.mem;
    if (counts_dev) DF_HIP(hipMemsetAsync(counts_dev, 0, 48, st));
    hipLaunchKernelGGL(df_render_fill_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, (uint4*)hold.mem, n4);
    DF_LAUNCH_CHECK();
    if (draw) {
        const size_t tb = ((size_t)a.T + 255) / 256;
        hipLaunchKernelGGL(df_render_raster_kernel, dim3((unsigned)(tb < DF_RENDER_RASTER_BLOCKS ? tb : DF_RENDER_RASTER_BLOCKS)), dim3(256), 0, st, a);
        DF_LAUNCH_CHECK();
    }
    const size_t pb = (npix + 255) / 256;
    hipLaunchKernelGGL(df_render_resolve_kernel, dim3((unsigned)(pb < DF_RENDER_RESOLVE_BLOCKS ? pb : DF_RENDER_RESOLVE_BLOCKS)), dim3(256), 0, st, a);
    DF_LAUNCH_CHECK();
    return DF_OK;
}
