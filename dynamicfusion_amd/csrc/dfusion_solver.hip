// dfusion_solver.hip -- the warp-field data term on the GPU (gfx950), SURVEY.md 8(f) "next" #4.
//
// Replaces WarpFieldOptimiser::optimiseWarpData -> CombinedSolver (Opt, kfusion/solvers/dynamicfusion.t:26-52) and
// WarpField::energy_data (Ceres, kfusion/src/warp_field.cpp:117-163 with the functor of
// kfusion/include/kfusion/optimisation.hpp:36-71).  Both hand the SAME energy to a third-party non-linear solver:
//     E(T) = sum_v | (live_v - canonical_v) - sum_{i<k} w_vi * T_{n_vi} |^2
// with n_vi / w_vi the k nearest nodes of canonical_v and their weights exp(-d^2 / 2 sigma^2) (getWeightsAndUpdateKNN); only
// the node TRANSLATIONS T are unknowns (RotationDeform is declared but unused in dynamicfusion.t; the Ceres functor reads only
// the translation slots), and there is no regularisation term in the reference (optimisation.hpp:125-157 is never added).
// E is linear least squares, so Gauss-Newton is one linear solve: here `iters` steps of conjugate gradients on the normal
// equations (W^T W + lambda I) delta = W^T e0, e0 the residual at the current translations, matrix-free:
//   W   (N x M, k non-zeros per row)  : one lane per point, gathers its k node entries in slot order;
//   W^T (M x N)                       : a node-major copy of the entries (stable radix sort by node id, so every node's list
//                                       is in ascending point order), one workgroup per node, thread-strided partial sums then
//                                       a fixed tree -- no float atomics, so the result is reproducible (and bit-comparable
//                                       with the restatement in oracle/dfusion_frontend_oracle.c);
//   dot products / vector updates     : one 1024-thread workgroup (M <= 65535), fixed tree.
// dfusion_warp_solve adds DynamicFusion's regularisation term over a node graph, dfusion_warp_solve_robust a Tukey
// penalty on the data term and a Huber penalty on the edges by re-weighted rounds, dfusion_warp_solve_plane takes the
// data term along the model normals (point-to-plane), and dfusion_warp_solve_rigid makes the node rotations
// unknowns too, against the warp dfusion_warp_points applies, with 6x6 node blocks as preconditioner where the handle asks for them
// (DESIGN.md 21).  The host pipeline is at the end of this file.  Every entry point fills one
// description of its solve (SvSolve), checked by df_sv_check; df_sv_context makes of it what a solve works with (SvContext: flags, grids,
// one workspace, the graph, the CG kernels) and holds every stage the solves share -- the preparation, the penalty weights, the energies,
// the CG skeleton, the outputs -- in which a term that is switched off launches nothing.  What is left in the two round loops is their
// difference: df_sv_rounds (translations: W, W^T, a linear final residual) and df_sv_rigid_rounds (six unknowns a node: warp, J, J^T).
// Nothing returns to the host between iterations: once every component has converged (scal[SV_ACTIVE] == 0) the kernels of the
// remaining steps return at once.
#include <hipcub/hipcub.hpp>
#include "dfusion_internal.h"

#pragma clang fp contract(off)

#define SV_BLOCK 1024

// ---- per point: validity, weights, node ids (sort keys), residual at the current translations
// PLANE: a normal with a NaN or infinite component makes the point invalid too (normals is not read otherwise)
template <bool PLANE>
__global__ __launch_bounds__(256) void df_sv_setup_kernel(const float* __restrict__ canonical, const float* __restrict__ live,
                                                          const float* __restrict__ normals, int N, int k,
                                                          const int* __restrict__ idx, const float* __restrict__ d2,
                                                          const float4* __restrict__ pos_sigma, const float4* __restrict__ node_t, int M,
                                                          float* __restrict__ w, unsigned int* __restrict__ keys,
                                                          unsigned int* __restrict__ vals, float* __restrict__ e0)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= N) return;
    const float cx = canonical[3 * v], cy = canonical[3 * v + 1], cz = canonical[3 * v + 2];
    const float lx = live[3 * v], ly = live[3 * v + 1], lz = live[3 * v + 2];
    bool valid = !(isnan(cx) || isnan(cy) || isnan(cz) || isnan(lx) || isnan(ly) || isnan(lz));         // warp_field.cpp:130-136
    if constexpr (PLANE) valid = valid && isfinite(normals[3 * v]) && isfinite(normals[3 * v + 1]) && isfinite(normals[3 * v + 2]);
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int j = 0; j < k; ++j) {
        const int e = v * k + j;
        const int n = valid ? idx[e] : M;                               // invalid points sort behind every node
        float wj = 0.f;
        if (valid) {
            wj = dqb_weight(d2[e], pos_sigma[n].w);                     // warp_field.cpp:238-241
            const float4 t = node_t[n];                                 // (w, x, y, z): translation in .y .z .w
            sx = sx + wj * t.y; sy = sy + wj * t.z; sz = sz + wj * t.w; // optimisation.hpp:58-60
        }
        w[e] = wj;
        keys[e] = (unsigned int)n;
        vals[e] = (unsigned int)e;
    }
    e0[3 * v] = valid ? (lx - cx) - sx : 0.f;                           // optimisation.hpp:64-66
    e0[3 * v + 1] = valid ? (ly - cy) - sy : 0.f;
    e0[3 * v + 2] = valid ? (lz - cz) - sz : 0.f;
}

// ---- node offsets into the sorted entry list: off[n] = first position whose key >= n (off[M] = number of valid entries)
__global__ __launch_bounds__(256) void df_sv_offsets_kernel(const unsigned int* __restrict__ sorted_keys, int E, int M, unsigned int* __restrict__ off)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > E) return;
    const unsigned int cur = i < E ? min(sorted_keys[i], (unsigned int)M) : (unsigned int)M;
    const unsigned int prev = i > 0 ? min(sorted_keys[i - 1], (unsigned int)M) : 0u;
    const unsigned int lo = i > 0 ? prev + 1 : 0u;
    for (unsigned int n = lo; n <= cur; ++n) off[n] = (unsigned int)i;
}

// ---- u = W p : per point, slot order
// K > 0: compile-time neighbour count, so that the 2K entry loads and 3K gathers of a point are all in flight before the first sum
// (with a run-time k the loop issues and waits entry by entry); K = 0: any k.  Same sums in the same order either way.
// PLANE: u = n (n . W p), the point-to-plane operator's N N^T W p.  The normal is loaded before the entries, so that it
// arrives while the gathers are in flight, and an invalid point (no entry: its normal may hold anything) stores 0.
template <int K, bool PLANE>
__global__ __launch_bounds__(256) void df_sv_w_apply_kernel(const float* __restrict__ w, const unsigned int* __restrict__ keys, int N, int k,
                                                            int M, const float* __restrict__ p, float* __restrict__ u,
                                                            const float* __restrict__ active, const float* __restrict__ normals)
{
    // `active` (nullable): scal + SV_ACTIVE, the number of CG components still iterating.  Once it is 0 every further step is an exact no-op
    // (alpha = beta = 0), so the kernels of the remaining steps return at once -- the host enqueues all steps without looking.
    if (active && *active == 0.f) return;
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= N) return;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if constexpr (PLANE) { nx = normals[3 * v]; ny = normals[3 * v + 1]; nz = normals[3 * v + 2]; }
    float sx = 0.f, sy = 0.f, sz = 0.f;
    if constexpr (K > 0) {
        unsigned int n[K]; float wj[K], px[K], py[K], pz[K];
#pragma unroll
        for (int j = 0; j < K; ++j) { n[j] = keys[v * K + j]; wj[j] = w[v * K + j]; }
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const unsigned int nc = min(n[j], (unsigned int)(M - 1));            // clamped gather; the entry is skipped below if n >= M
            px[j] = p[3 * nc]; py[j] = p[3 * nc + 1]; pz[j] = p[3 * nc + 2];
        }
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (n[j] < (unsigned int)M) { sx = sx + wj[j] * px[j]; sy = sy + wj[j] * py[j]; sz = sz + wj[j] * pz[j]; }
    } else {
        for (int j = 0; j < k; ++j) {
            const int e = v * k + j;
            const unsigned int n = keys[e];
            if (n < (unsigned int)M) {
                const float wj = w[e];
                sx = sx + wj * p[3 * n]; sy = sy + wj * p[3 * n + 1]; sz = sz + wj * p[3 * n + 2];
            }
        }
    }
    if constexpr (PLANE) {
        const float d = (nx * sx + ny * sy) + nz * sz;
        const bool valid = keys[v * k] < (unsigned int)M;               // (a point's k entries are valid together)
        sx = valid ? nx * d : 0.f; sy = valid ? ny * d : 0.f; sz = valid ? nz * d : 0.f;
    }
    u[3 * v] = sx; u[3 * v + 1] = sy; u[3 * v + 2] = sz;
}

// ---- node-major copies of the entries' point ids and weights (once per solve; the W^T kernel then reads them in list order)
__global__ __launch_bounds__(256) void df_sv_sorted_kernel(const unsigned int* __restrict__ sorted_vals, const float* __restrict__ w, int E, int k,
                                                           unsigned int* __restrict__ sorted_pt, float* __restrict__ sorted_w)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= E) return;
    const unsigned int e = sorted_vals[i];
    sorted_pt[i] = e / (unsigned int)k;
    sorted_w[i] = w[e];
}

// ---- the node tree of the two apply^T kernels: S sums a thread, 256 threads; the partials are combined by the tree (t, t + s),
// s = 128 .. 1 (s >= 64 through LDS, s <= 32 with __shfl_down inside wave 0) -- a fixed order, restated in the oracle.  Lane 0 of wave 0
// ends with the totals in s and runs `done`.
template <int S, typename Done>
__device__ __forceinline__ void sv_node_tree(float (&s)[S], float* lds /* [S][128] */, Done done)
{
    const int t = threadIdx.x, wv = t >> 6, l = t & 63;
    if (wv >= 2) { for (int c = 0; c < S; ++c) lds[c * 128 + (t - 128)] = s[c]; }
    __syncthreads();
    if (wv < 2) { for (int c = 0; c < S; ++c) s[c] = s[c] + lds[c * 128 + t]; }
    __syncthreads();
    if (wv == 1) { for (int c = 0; c < S; ++c) lds[c * 128 + l] = s[c]; }
    __syncthreads();
    if (wv == 0) {
#pragma unroll
        for (int c = 0; c < S; ++c) {
            float a = s[c] + lds[c * 128 + l];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) a = a + __shfl_down(a, o, 64);
            s[c] = a;
        }
        if (l == 0) done();
    }
}

// ---- out = W^T u (+ lambda * p) : one 256-thread workgroup per node over its (ascending-point-order) entry list.
// Thread t sums entries t, t + 256, ... ; then sv_node_tree.
__global__ __launch_bounds__(256) void df_sv_wt_apply_kernel(const unsigned int* __restrict__ off, const unsigned int* __restrict__ sorted_pt,
                                                             const float* __restrict__ sorted_w, int M, const float* __restrict__ u,
                                                             float lambda, const float* __restrict__ p, float* __restrict__ out,
                                                             const float* __restrict__ active)
{
    __shared__ float lds[3 * 128];
    if (active && *active == 0.f) return;                               // see df_sv_w_apply_kernel
    const int n = blockIdx.x, t = threadIdx.x;
    const unsigned int b = off[n], e_end = off[n + 1];
    float s[3] = {0.f, 0.f, 0.f};
    // the entry's point id and weight sit in list order (df_sv_sorted_kernel), so a trip is one coalesced read + the u gather
    for (unsigned int i = b + t; i < e_end; i += 256) {
        const unsigned int v = sorted_pt[i];
        const float we = sorted_w[i];
        s[0] = s[0] + we * u[3 * v]; s[1] = s[1] + we * u[3 * v + 1]; s[2] = s[2] + we * u[3 * v + 2];
    }
    sv_node_tree(s, lds, [&]() {
        if (p) { s[0] = s[0] + lambda * p[3 * n]; s[1] = s[1] + lambda * p[3 * n + 1]; s[2] = s[2] + lambda * p[3 * n + 2]; }
        out[3 * n] = s[0]; out[3 * n + 1] = s[1]; out[3 * n + 2] = s[2];
    });
}

// ---- single-workgroup vector algebra: three independent CG recurrences (x, y, z components share the matrix), or ONE over all three
// (COUPLED, below: the point-to-plane matrix mixes the components)
// block-wide sums of three values: thread t owns elements t, t + 1024, ... ; then the tree 512 .. 1 in LDS
__device__ __forceinline__ void sv_block_sum3(float (&s)[3], float* lds /* [3][1024] */)
{
    const int t = threadIdx.x;
#pragma unroll
    for (int c = 0; c < 3; ++c) lds[c * SV_BLOCK + t] = s[c];
    __syncthreads();
    for (int st = SV_BLOCK / 2; st >= 64; st >>= 1) {                   // pairs (t, t + st)
        if (t < st) {
#pragma unroll
            for (int c = 0; c < 3; ++c) lds[c * SV_BLOCK + t] = lds[c * SV_BLOCK + t] + lds[c * SV_BLOCK + t + st];
        }
        __syncthreads();
    }
    if (t < 64) {                                                        // st = 32 .. 1 inside wave 0: the same pairs
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float a = lds[c * SV_BLOCK + t];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) a = a + __shfl_down(a, o, 64);
            if (t == 0) lds[c * SV_BLOCK] = a;
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = lds[c * SV_BLOCK];
    __syncthreads();
}

// scal, the solve's device scalars: the slots, per x / y / z component where there are three (4, 5 and 9 .. 11 are free)
enum {
    SV_RR = 0,          // [3] rr of the current residual (0 = component converged / frozen)
    SV_ACTIVE = 3,      //     number of components still iterating
    SV_RR0 = 6,         // [3] rr of the first residual (the convergence test is relative to it)
    SV_ENERGY = 12,     // [4] E_data before, after, E_reg before, after (a data-only solve writes the first two)
    SV_SCAL_N = 16
};
#define SV_REL_TOL2 1.0e-10f        // stop a component once |r|^2 <= 1e-10 |r0|^2

// COUPLED (the point-to-plane solve, whose matrix differs between x, y and z): ONE recurrence over the 3M vector.  Every dot product is
// the three per-component sums combined; with the same value in all three slots the per-component code below is the scalar recurrence.
template <bool COUPLED>
__device__ __forceinline__ void sv_cg_couple(float (&s)[3])
{
    if constexpr (COUPLED) s[0] = s[1] = s[2] = (s[0] + s[1]) + s[2];
}

template <bool COUPLED>
__global__ __launch_bounds__(SV_BLOCK) void df_sv_init_kernel(const float* __restrict__ r, int M, float* __restrict__ x, float* __restrict__ p,
                                                              float* __restrict__ scal)
{
    __shared__ float lds[3 * SV_BLOCK];
    float s[3] = {0.f, 0.f, 0.f};
    for (int n = threadIdx.x; n < M; n += SV_BLOCK)
        for (int c = 0; c < 3; ++c) { const float rv = r[3 * n + c]; x[3 * n + c] = 0.f; p[3 * n + c] = rv; s[c] = s[c] + rv * rv; }
    sv_block_sum3(s, lds);
    sv_cg_couple<COUPLED>(s);
    if (threadIdx.x == 0) {
        for (int c = 0; c < 3; ++c) { scal[SV_RR + c] = s[c]; scal[SV_RR0 + c] = s[c]; }
        scal[SV_ACTIVE] = COUPLED ? (float)(s[0] > 0.f) : (float)((s[0] > 0.f) + (s[1] > 0.f) + (s[2] > 0.f));
    }
}

// The scalar recurrence of a CG step, per component, for both step kernels below.
__device__ __forceinline__ float sv_cg_alpha(float pq, float rr_old)
{
    return (pq > 0.f && rr_old > 0.f) ? rr_old / pq : 0.f;              // converged / degenerate component: frozen
}

__device__ __forceinline__ float sv_cg_beta(float alpha, float rr, float rr_old)
{
    return (alpha != 0.f && rr_old > 0.f) ? rr / rr_old : 0.f;
}

// one thread, once every thread has read scal's rr: the new rr (0 = frozen from here on) and the number of components left
// (COUPLED: the three slots hold one recurrence, which counts once)
template <bool COUPLED>
__device__ __forceinline__ void sv_cg_freeze(const float (&alpha)[3], const float (&rr)[3], float* scal)
{
    float active = 0.f;
    for (int c = 0; c < 3; ++c) {
        const float keep = (alpha[c] != 0.f && rr[c] > SV_REL_TOL2 * scal[SV_RR0 + c]) ? rr[c] : 0.f;
        scal[SV_RR + c] = keep;
        active += keep > 0.f ? 1.f : 0.f;
    }
    scal[SV_ACTIVE] = COUPLED ? (active > 0.f ? 1.f : 0.f) : active;
}

template <bool COUPLED>
__global__ __launch_bounds__(SV_BLOCK) void df_sv_step_kernel(const float* __restrict__ q, int M, float* __restrict__ x, float* __restrict__ r,
                                                              float* __restrict__ p, float* __restrict__ scal)
{
    __shared__ float lds[3 * SV_BLOCK];
    if (scal[SV_ACTIVE] == 0.f) return;                                 // all components frozen: the step would change nothing
    float pq[3] = {0.f, 0.f, 0.f};
    for (int n = threadIdx.x; n < M; n += SV_BLOCK)
        for (int c = 0; c < 3; ++c) pq[c] = pq[c] + p[3 * n + c] * q[3 * n + c];
    sv_block_sum3(pq, lds);
    sv_cg_couple<COUPLED>(pq);
    float alpha[3], rr_old[3];
    for (int c = 0; c < 3; ++c) { rr_old[c] = scal[SV_RR + c]; alpha[c] = sv_cg_alpha(pq[c], rr_old[c]); }
    float rr[3] = {0.f, 0.f, 0.f};
    for (int n = threadIdx.x; n < M; n += SV_BLOCK)
        for (int c = 0; c < 3; ++c) {
            x[3 * n + c] = x[3 * n + c] + alpha[c] * p[3 * n + c];
            const float rv = r[3 * n + c] - alpha[c] * q[3 * n + c];
            r[3 * n + c] = rv;
            rr[c] = rr[c] + rv * rv;
        }
    sv_block_sum3(rr, lds);
    sv_cg_couple<COUPLED>(rr);
    float beta[3];
    for (int c = 0; c < 3; ++c) beta[c] = sv_cg_beta(alpha[c], rr[c], rr_old[c]);
    for (int n = threadIdx.x; n < M; n += SV_BLOCK)
        for (int c = 0; c < 3; ++c) p[3 * n + c] = r[3 * n + c] + beta[c] * p[3 * n + c];
    __syncthreads();
    if (threadIdx.x == 0) sv_cg_freeze<COUPLED>(alpha, rr, scal);
}

// df_sv_step_kernel for M <= EPT * SV_BLOCK: x, r, p, q are read once and stay in registers between the three passes (the passes of
// the kernel above each wait for their own global loads).  Same element -> thread assignment, same sums, same trees.
template <int EPT, bool COUPLED>
__global__ __launch_bounds__(SV_BLOCK) void df_sv_step_reg_kernel(const float* __restrict__ q, int M, float* __restrict__ x, float* __restrict__ r,
                                                                  float* __restrict__ p, float* __restrict__ scal)
{
    __shared__ float lds[3 * SV_BLOCK];
    if (scal[SV_ACTIVE] == 0.f) return;                                 // all components frozen: the step would change nothing
    float pv[EPT][3], qv[EPT][3], rv[EPT][3], xv[EPT][3];
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int n = threadIdx.x + j * SV_BLOCK;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const bool in = n < M;
            pv[j][c] = in ? p[3 * n + c] : 0.f; qv[j][c] = in ? q[3 * n + c] : 0.f;
            rv[j][c] = in ? r[3 * n + c] : 0.f; xv[j][c] = in ? x[3 * n + c] : 0.f;
        }
    }
    float pq[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < EPT; ++j)
        if (threadIdx.x + j * SV_BLOCK < M)
#pragma unroll
            for (int c = 0; c < 3; ++c) pq[c] = pq[c] + pv[j][c] * qv[j][c];
    sv_block_sum3(pq, lds);
    sv_cg_couple<COUPLED>(pq);
    float alpha[3], rr_old[3];
    for (int c = 0; c < 3; ++c) { rr_old[c] = scal[SV_RR + c]; alpha[c] = sv_cg_alpha(pq[c], rr_old[c]); }
    float rr[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < EPT; ++j)
        if (threadIdx.x + j * SV_BLOCK < M)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                xv[j][c] = xv[j][c] + alpha[c] * pv[j][c];
                rv[j][c] = rv[j][c] - alpha[c] * qv[j][c];
                rr[c] = rr[c] + rv[j][c] * rv[j][c];
            }
    sv_block_sum3(rr, lds);
    sv_cg_couple<COUPLED>(rr);
    float beta[3];
    for (int c = 0; c < 3; ++c) beta[c] = sv_cg_beta(alpha[c], rr[c], rr_old[c]);
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int n = threadIdx.x + j * SV_BLOCK;
        if (n < M)
#pragma unroll
            for (int c = 0; c < 3; ++c) { x[3 * n + c] = xv[j][c]; r[3 * n + c] = rv[j][c]; p[3 * n + c] = rv[j][c] + beta[c] * pv[j][c]; }
    }
    if (threadIdx.x == 0) sv_cg_freeze<COUPLED>(alpha, rr, scal);
}

// ---- energy = sum_v |e_v|^2 (single workgroup, same tree)
__global__ __launch_bounds__(SV_BLOCK) void df_sv_energy_kernel(const float* __restrict__ e, int N, float* __restrict__ out)
{
    __shared__ float lds[3 * SV_BLOCK];
    float s[3] = {0.f, 0.f, 0.f};
    for (int v = threadIdx.x; v < N; v += SV_BLOCK)
        for (int c = 0; c < 3; ++c) s[c] = s[c] + e[3 * v + c] * e[3 * v + c];
    sv_block_sum3(s, lds);
    if (threadIdx.x == 0) *out = (s[0] + s[1]) + s[2];
}

// e1 = e0 - W x  (final residual, for the reported energy)
__global__ __launch_bounds__(256) void df_sv_residual_kernel(const float* __restrict__ e0, const float* wx, int n3, float* e1)   // e1 may alias wx
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n3) e1[i] = e0[i] - wx[i];
}

// ---- a node's rot / dual float4 as a quaternion, and node n's transform applied to a point
__device__ __forceinline__ quat sv_quat(float4 v) { quat q; q.w = v.x; q.x = v.y; q.y = v.z; q.z = v.w; return q; }
__device__ __forceinline__ f3 sv_node_transform(const float4* __restrict__ rot, const float4* __restrict__ dual, int n, float4 p) { return dq_transform(sv_quat(rot[n]), sv_quat(dual[n]), mk3(p.x, p.y, p.z)); }

// ---- write back: T = T0 + x ; translation_ = 0.5 * (0, T) * rotation_ (encodeTranslation, dual_quaternion.hpp:82-85)
__global__ __launch_bounds__(256) void df_sv_writeback_kernel(const float4* __restrict__ rot, const float4* __restrict__ node_t,
                                                              const float* __restrict__ x, int M, float* __restrict__ dq_out)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= M) return;
    const float4 t4 = node_t[n];
    const quat r = sv_quat(rot[n]);
    quat T; T.w = 0.f; T.x = t4.y + x[3 * n]; T.y = t4.z + x[3 * n + 1]; T.z = t4.w + x[3 * n + 2];
    const quat d = q_mul(q_scale(0.5f, T), r);
    float* o = dq_out + 8 * (size_t)n;
    o[0] = r.w; o[1] = r.x; o[2] = r.y; o[3] = r.z; o[4] = d.w; o[5] = d.x; o[6] = d.y; o[7] = d.z;
}

// ---------------------------------------------------------------- regularisation over the node graph
// E_reg = sum_e alpha_e |g_e + delta_i - delta_j|^2 over the directed edges e = (i -> j), j one of node i's kg nearest other nodes:
//   g_e = T_i(v_j) - T_j(v_j) at the transforms the solve starts from, alpha_e = max(dg_w_i, dg_w_j)  (DynamicFusion eq. 8, psi quadratic).
// Edge e = i * kg + s (s = slot in i's list).  A node's sums run over its outgoing edges in slot order, then over its incoming edges in
// ascending edge id (a CSR transpose made with the graph by a stable sort of the edge ids by head node): one thread per node, no atomics.
__global__ __launch_bounds__(256) void df_sv_graph_pos_kernel(const float4* __restrict__ pos_sigma, int M, float* __restrict__ pos3)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= M) return;
    const float4 p = pos_sigma[n];
    pos3[3 * n] = p.x; pos3[3 * n + 1] = p.y; pos3[3 * n + 2] = p.z;
}

// node i's list: its kg + 1 nearest nodes without the entry whose id is i -- or without the last one when none is (duplicate positions)
__global__ __launch_bounds__(256) void df_sv_graph_kernel(const int* __restrict__ idx, const float4* __restrict__ pos_sigma, int M, int kg,
                                                          int* __restrict__ nbr, float* __restrict__ alpha, unsigned int* __restrict__ keys,
                                                          unsigned int* __restrict__ vals)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const float si = pos_sigma[i].w;
    int drop = kg;
    for (int s = kg; s >= 0; --s) if (idx[i * (kg + 1) + s] == i) drop = s;        // the first entry that is i itself
    for (int s = 0; s < kg; ++s) {
        const int j = min(max(idx[i * (kg + 1) + s + (s >= drop ? 1 : 0)], 0), M - 1);   // (clamped: a NaN position must not index outside)
        const int e = i * kg + s;
        nbr[e] = j;
        alpha[e] = fmaxf(si, pos_sigma[j].w);
        keys[e] = (unsigned int)j; vals[e] = (unsigned int)e;
    }
}

__global__ __launch_bounds__(256) void df_sv_reg_edge_kernel(const int* __restrict__ nbr, const float4* __restrict__ pos_sigma,
                                                             const float4* __restrict__ rot, const float4* __restrict__ dual, int E, int kg,
                                                             float* __restrict__ g)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int i = e / kg, j = nbr[e];
    const float4 pj = pos_sigma[j];
    const f3 ti = sv_node_transform(rot, dual, i, pj), tj = sv_node_transform(rot, dual, j, pj);
    g[3 * e] = ti.x - tj.x; g[3 * e + 1] = ti.y - tj.y; g[3 * e + 2] = ti.z - tj.z;
}

// r_n = r_n - lambda_reg * acc_n, acc_n = sum_out alpha_e g_e - sum_in alpha_e g_e  (r holds W^T e0)
__global__ __launch_bounds__(256) void df_sv_reg_rhs_kernel(const float* __restrict__ alpha, const unsigned int* __restrict__ in_off,
                                                            const unsigned int* __restrict__ in_edge, int M, int kg,
                                                            const float* __restrict__ g, float lambda_reg, float* __restrict__ r)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= M) return;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int s = 0; s < kg; ++s) {
        const int e = n * kg + s;
        const float a = alpha[e];
        for (int c = 0; c < 3; ++c) acc[c] = acc[c] + a * g[3 * e + c];
    }
    for (unsigned int i = in_off[n]; i < in_off[n + 1]; ++i) {
        const unsigned int e = in_edge[i];
        const float a = alpha[e];
        for (int c = 0; c < 3; ++c) acc[c] = acc[c] - a * g[3 * e + c];
    }
    for (int c = 0; c < 3; ++c) r[3 * n + c] = r[3 * n + c] - lambda_reg * acc[c];
}

// q_n = q_n + lambda_reg * (L p)_n, the edge differences p_i - p_j formed in the node's thread (q holds (W^T W + lambda I) p)
__global__ __launch_bounds__(256) void df_sv_reg_apply_kernel(const int* __restrict__ nbr, const float* __restrict__ alpha,
                                                              const unsigned int* __restrict__ in_off, const unsigned int* __restrict__ in_edge,
                                                              int M, int kg, const float* __restrict__ p, float lambda_reg,
                                                              float* __restrict__ q, const float* __restrict__ active)
{
    if (active && *active == 0.f) return;                               // see df_sv_w_apply_kernel
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= M) return;
    const float pn[3] = {p[3 * n], p[3 * n + 1], p[3 * n + 2]};
    float acc[3] = {0.f, 0.f, 0.f};
    for (int s = 0; s < kg; ++s) {
        const int e = n * kg + s, j = nbr[e];
        const float a = alpha[e];
        for (int c = 0; c < 3; ++c) acc[c] = acc[c] + a * (pn[c] - p[3 * j + c]);
    }
    for (unsigned int i = in_off[n]; i < in_off[n + 1]; ++i) {
        const unsigned int e = in_edge[i], t = e / (unsigned int)kg;     // the edge t -> n
        const float a = alpha[e];
        for (int c = 0; c < 3; ++c) acc[c] = acc[c] - a * (p[3 * t + c] - pn[c]);
    }
    for (int c = 0; c < 3; ++c) q[3 * n + c] = q[3 * n + c] + lambda_reg * acc[c];
}

// component c of the edge value h_e = (g_e + x_i) - x_j of the edge e = (i -> j), x nullable = 0
__device__ __forceinline__ float sv_edge_h(const float* __restrict__ g, const float* __restrict__ x, int e, int i, int j, int c) { return x ? (g[3 * e + c] + x[3 * i + c]) - x[3 * j + c] : g[3 * e + c]; }

// ---- E_reg = sum_e alpha_e |h_e|^2, reduced like df_sv_energy_kernel over the edges
__global__ __launch_bounds__(SV_BLOCK) void df_sv_reg_energy_kernel(const int* __restrict__ nbr, const float* __restrict__ alpha,
                                                                    const float* __restrict__ g, const float* __restrict__ x, int E, int kg,
                                                                    float* __restrict__ out)
{
    __shared__ float lds[3 * SV_BLOCK];
    float s[3] = {0.f, 0.f, 0.f};
    for (int e = threadIdx.x; e < E; e += SV_BLOCK) {
        const int i = e / kg, j = nbr[e];
        const float a = alpha[e];
        for (int c = 0; c < 3; ++c) {
            const float h = sv_edge_h(g, x, e, i, j, c);
            s[c] = s[c] + a * (h * h);
        }
    }
    sv_block_sum3(s, lds);
    if (threadIdx.x == 0) *out = (s[0] + s[1]) + s[2];
}

// ---------------------------------------------------------------- robust solve: Tukey data term, Huber regularisation, IRLS
// A round is one solve of above with weights: omega_v (Tukey, from the residual the round starts at) multiplied into the node-major copy
// of the entry weights, omega_e (Huber, from the round's g_e) into a copy of alpha; the kernels above are launched unchanged.

// e0 at the transforms the handle holds now, from the stored entries: df_sv_setup_kernel's sums in its order (keys[e] = M: invalid point)
__global__ __launch_bounds__(256) void df_sv_round_e0_kernel(const float* __restrict__ canonical, const float* __restrict__ live, int N, int k,
                                                             const unsigned int* __restrict__ keys, const float* __restrict__ w,
                                                             const float4* __restrict__ node_t, int M, float* __restrict__ e0)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= N) return;
    const bool valid = keys[v * k] < (unsigned int)M;                   // (a point's k entries are valid together)
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int j = 0; j < k; ++j) {
        const int e = v * k + j;
        const unsigned int n = keys[e];
        if (valid && n < (unsigned int)M) {
            const float wj = w[e];
            const float4 t = node_t[n];
            sx = sx + wj * t.y; sy = sy + wj * t.z; sz = sz + wj * t.w;
        }
    }
    e0[3 * v] = valid ? (live[3 * v] - canonical[3 * v]) - sx : 0.f;
    e0[3 * v + 1] = valid ? (live[3 * v + 1] - canonical[3 * v + 1]) - sy : 0.f;
    e0[3 * v + 2] = valid ? (live[3 * v + 2] - canonical[3 * v + 2]) - sz : 0.f;
}

// The Tukey penalty of a point on s, its squared residual: s = |e_v|^2 from the residuals e [3N], or (PLANE) s = rho_v^2
// from the projected residuals e = rho [N].  The weight is (1 - s / c^2)^2 for s < c^2, else 0 (a NaN s compares false: 0); the
// energy rho(s) = c^2/3 (1 - (1 - s/c^2)^3) below c^2 and c^2/3 above (third = c^2 / 3).
template <bool PLANE>
__device__ __forceinline__ float sv_point_s(const float* __restrict__ e, int v)
{
    if constexpr (PLANE) return e[v] * e[v];
    const float ex = e[3 * v], ey = e[3 * v + 1], ez = e[3 * v + 2];
    return (ex * ex + ey * ey) + ez * ez;
}
__device__ __forceinline__ float sv_tukey_weight(float s, float c2) { const float u = 1.f - s / c2; return (s < c2) ? u * u : 0.f; }
__device__ __forceinline__ float sv_tukey_rho(float s, float c2, float third) { const float u = 1.f - s / c2; return (s < c2) ? third * (1.f - (u * u) * u) : third; }

// omega_v = the Tukey weight of point v
template <bool PLANE>
__global__ __launch_bounds__(256) void df_sv_tukey_kernel(const float* __restrict__ e, int N, float c2, float* __restrict__ omega)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= N) return;
    omega[v] = sv_tukey_weight(sv_point_s<PLANE>(e, v), c2);
}

// sorted_w'[i] = omega_pt(i) * sorted_w[i]: list order, so the two entry reads and the write are coalesced; omega is a gather (ascending
// point ids inside a node's list)
__global__ __launch_bounds__(256) void df_sv_scale_list_kernel(const unsigned int* __restrict__ sorted_pt, const float* __restrict__ sorted_w,
                                                               const float* __restrict__ omega, int E, float* __restrict__ scaled_w)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= E) return;
    scaled_w[i] = omega[sorted_pt[i]] * sorted_w[i];
}

// omega_e = 1 for s = |g_e|^2 <= delta^2, else delta / |g_e|; alpha'_e = alpha_e * omega_e
__global__ __launch_bounds__(256) void df_sv_huber_kernel(const float* __restrict__ g, const float* __restrict__ alpha, int E, float delta, float d2,
                                                          float* __restrict__ omega_e, float* __restrict__ alpha_w)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const float gx = g[3 * e], gy = g[3 * e + 1], gz = g[3 * e + 2];
    const float s = (gx * gx + gy * gy) + gz * gz;
    const float om = (s <= d2) ? 1.f : delta / sqrtf(s);
    omega_e[e] = om;
    alpha_w[e] = alpha[e] * om;
}

// ---- E_reg = sum_e alpha_e psi(|h_e|^2), h = (g_e + x_i) - x_j (x nullable = 0), psi(s) = s up to delta^2 and 2 delta sqrt(s) - delta^2 above
__global__ __launch_bounds__(SV_BLOCK) void df_sv_huber_energy_kernel(const int* __restrict__ nbr, const float* __restrict__ alpha,
                                                                      const float* __restrict__ g, const float* __restrict__ x, int E, int kg,
                                                                      float delta, float d2, float* __restrict__ out)
{
    __shared__ float lds[3 * SV_BLOCK];
    float acc[3] = {0.f, 0.f, 0.f};
    const float two_delta = 2.f * delta;
    for (int e = threadIdx.x; e < E; e += SV_BLOCK) {
        const int i = e / kg, j = nbr[e];
        float h[3];
        for (int c = 0; c < 3; ++c) h[c] = sv_edge_h(g, x, e, i, j, c);
        const float s = (h[0] * h[0] + h[1] * h[1]) + h[2] * h[2];
        acc[0] = acc[0] + alpha[e] * ((s <= d2) ? s : two_delta * sqrtf(s) - d2);
    }
    sv_block_sum3(acc, lds);
    if (threadIdx.x == 0) *out = acc[0];
}

// ---------------------------------------------------------------- point-to-plane data term
// E_data = sum_v rho_v^2, rho_v = n_v . e_v with the normals as given (never normalised): the rows of W are projected on n_v, so the
// normal matrix is W^T N N^T W (df_sv_w_apply_kernel<K, true> followed by the unchanged W^T walk), the right-hand side W^T (n rho), and
// the three components are one system (the COUPLED step kernels).  Tukey works on rho^2.

// rho_v = (nx ex + ny ey) + nz ez and, with b, b_v = n_v rho_v; 0 for an invalid point (e = 0 there, but its normal may be NaN or inf)
__global__ __launch_bounds__(256) void df_sv_plane_rho_kernel(const float* __restrict__ e, const float* __restrict__ normals,
                                                              const unsigned int* __restrict__ keys, int N, int k, int M,
                                                              float* __restrict__ rho, float* __restrict__ b)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= N) return;
    const float nx = normals[3 * v], ny = normals[3 * v + 1], nz = normals[3 * v + 2];
    const bool valid = keys[v * k] < (unsigned int)M;
    const float r = valid ? (nx * e[3 * v] + ny * e[3 * v + 1]) + nz * e[3 * v + 2] : 0.f;
    rho[v] = r;
    if (b) { b[3 * v] = valid ? nx * r : 0.f; b[3 * v + 1] = valid ? ny * r : 0.f; b[3 * v + 2] = valid ? nz * r : 0.f; }
}

// ---- E_data as a sum of ONE value per point: s_v = rho_v^2 (PLANE) or, TUKEY, the Tukey rho(s_v) with s_v as in df_sv_tukey_kernel<PLANE>.
// Thread t owns points t, t + 1024, ..., then the 1024-tree.  (The quadratic point-to-point energy is df_sv_energy_kernel's: three sums
// through three trees, another order.)
template <bool PLANE, bool TUKEY>
__global__ __launch_bounds__(SV_BLOCK) void df_sv_point_energy_kernel(const float* __restrict__ e, int N, float c2, float* __restrict__ out)
{
    static_assert(PLANE || TUKEY, "the quadratic point-to-point energy sums per component: df_sv_energy_kernel");
    __shared__ float lds[3 * SV_BLOCK];
    float acc[3] = {0.f, 0.f, 0.f};
    const float third = c2 / 3.f;
    for (int v = threadIdx.x; v < N; v += SV_BLOCK) {
        const float s = sv_point_s<PLANE>(e, v);
        acc[0] = acc[0] + (TUKEY ? sv_tukey_rho(s, c2, third) : s);
    }
    sv_block_sum3(acc, lds);
    if (threadIdx.x == 0) *out = acc[0];
}

// ---------------------------------------------------------------- node rotations as unknowns
// dfusion_warp_solve_rigid: Gauss-Newton rounds against the warp the pipeline applies, y_v = DQB(canonical_v).transform(canonical_v)
// from dfusion_warp_points.  That blend (dqb_blend_w) turns the point by the normalised sum of the weighted node rotations and adds the
// sum of the node translations under the UNNORMALISED weights: y_v = R_v p_v + T_v, T_v = sum_i w_vi t_i.  Six unknowns a node, a rotation
// omega_n about the node's warped position c_n = T_n(pos_n) and a translation tau_n, change t_n by tau_n - omega_n x q_n, q_n = c_n - t_n,
// and R_v by the blend of the omega_i under wn_vi = w_vi / S_v (to first order, for node rotations that are close to each other):
//     dy_v = sum_i w_vi (tau_i - omega_i x q_i) + (sum_i wn_vi omega_i) x a_v,   a_v = y_v - T_v = R_v p_v.
// The unknowns are one 3-component array of 2M entries (omega_n at entry n, tau_n at entry M + n), so that the COUPLED init and step
// kernels above run on it as they are.  Products are rounded before they are added, sums run in slot / list / edge order.

// ---- per point, once per call: validity (the first round's warp included), the blend weights and their normalised copies, node ids
__global__ __launch_bounds__(256) void df_sv_rigid_setup_kernel(const float* __restrict__ canonical, const float* __restrict__ live,
                                                                const float* __restrict__ normals, const float* __restrict__ y,
                                                                const float* __restrict__ nw, int N, int k, const int* __restrict__ idx,
                                                                const float* __restrict__ d2, const float4* __restrict__ pos_sigma, int M,
                                                                float* __restrict__ w, float* __restrict__ wn, unsigned int* __restrict__ keys,
                                                                unsigned int* __restrict__ vals)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= N) return;
    bool valid = true;
    for (int c = 0; c < 3; ++c) {
        valid = valid && !isnan(canonical[3 * v + c]) && !isnan(live[3 * v + c]) && isfinite(y[3 * v + c]);
        if (normals) valid = valid && isfinite(normals[3 * v + c]) && isfinite(nw[3 * v + c]);
    }
    float S = 0.f;
    for (int j = 0; j < k; ++j) {                                       // (a finite y had a finite query: its k ids are node ids)
        const int e = v * k + j;
        const float wj = valid ? dqb_weight(d2[e], pos_sigma[min(max(idx[e], 0), M - 1)].w) : 0.f;
        w[e] = wj;
        S = S + wj;
    }
    valid = valid && !(S == 0.f);
    for (int j = 0; j < k; ++j) {
        const int e = v * k + j;
        const float wj = w[e];
        w[e] = valid ? wj : 0.f;
        wn[e] = valid ? wj / S : 0.f;
        keys[e] = valid ? (unsigned int)min(max(idx[e], 0), M - 1) : (unsigned int)M;
        vals[e] = (unsigned int)e;
    }
}

// ---- per node and round: c_n = T_n(pos_n), the point the round's rotation update turns about, and q_n = c_n - t_n
__global__ __launch_bounds__(256) void df_sv_rigid_centre_kernel(const float4* __restrict__ pos_sigma, const float4* __restrict__ rot,
                                                                 const float4* __restrict__ dual, const float4* __restrict__ node_t, int M,
                                                                 float4* __restrict__ c, float4* __restrict__ qc)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= M) return;
    const float4 nt = node_t[n];
    const f3 t = sv_node_transform(rot, dual, n, pos_sigma[n]);
    c[n] = make_float4(t.x, t.y, t.z, 0.f);
    qc[n] = make_float4(t.x - nt.y, t.y - nt.z, t.z - nt.w, 0.f);
}

// ---- e_v = live_v - y_v and a_v = y_v - T_v, T_v = sum_i w_vi t_i in slot order (df_sv_setup_kernel's sums); 0 for an invalid point
__global__ __launch_bounds__(256) void df_sv_rigid_residual_kernel(const float* __restrict__ live, const float* __restrict__ y,
                                                                   const unsigned int* __restrict__ keys, const float* __restrict__ w,
                                                                   const float4* __restrict__ node_t, int N, int k, int M,
                                                                   float* __restrict__ e, float* __restrict__ arm)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= N) return;
    const bool valid = keys[v * k] < (unsigned int)M;                   // (a point's k entries are valid together)
    float sx = 0.f, sy = 0.f, sz = 0.f;
    if (arm && valid)
        for (int j = 0; j < k; ++j) {
            const float wj = w[v * k + j];
            const float4 t = node_t[keys[v * k + j]];                   // (w, x, y, z): translation in .y .z .w
            sx = sx + wj * t.y; sy = sy + wj * t.z; sz = sz + wj * t.w;
        }
    const float yx = y[3 * v], yy = y[3 * v + 1], yz = y[3 * v + 2];
    e[3 * v] = valid ? live[3 * v] - yx : 0.f; e[3 * v + 1] = valid ? live[3 * v + 1] - yy : 0.f; e[3 * v + 2] = valid ? live[3 * v + 2] - yz : 0.f;
    if (arm) { arm[3 * v] = valid ? yx - sx : 0.f; arm[3 * v + 1] = valid ? yy - sy : 0.f; arm[3 * v + 2] = valid ? yz - sz : 0.f; }
}

// What J^T reads of a point, as one 32-byte record: (u, 0) and (a_v x u, 0).  The cross product depends on the point alone, so it is
// formed once here instead of once per list entry, and a list entry's gather is two 16-byte loads of one aligned record.
__device__ __forceinline__ void sv_rigid_store(float4* __restrict__ rec, int v, float ux, float uy, float uz, float ax, float ay, float az)
{
    rec[2 * (size_t)v] = make_float4(ux, uy, uz, 0.f);
    rec[2 * (size_t)v + 1] = make_float4(ay * uz - az * uy, az * ux - ax * uz, ax * uy - ay * ux, 0.f);
}

// ---- u = J p : per point, slot order:  st = st + w (p_tau_n - (p_om_n x q_n)),  sr = sr + wn p_om_n,  u = st + (sr x a_v).
// K as in df_sv_w_apply_kernel: with K > 0 the normal, a_v, the 3K entry loads and the K x (two p triples + one 16-byte q gather) are
// all in flight before the first sum.  PLANE: u = n' (n' . J p) with n' the warped normal of the round; an invalid point stores 0.
template <int K, bool PLANE>
__global__ __launch_bounds__(256) void df_sv_rigid_j_apply_kernel(const float* __restrict__ w, const float* __restrict__ wn,
                                                                  const unsigned int* __restrict__ keys, int N, int k, int M,
                                                                  const float* __restrict__ p, const float* __restrict__ arm,
                                                                  const float4* __restrict__ qc, float4* __restrict__ rec,
                                                                  const float* __restrict__ active, const float* __restrict__ nw)
{
    if (active && *active == 0.f) return;                               // see df_sv_w_apply_kernel
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= N) return;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if constexpr (PLANE) { nx = nw[3 * v]; ny = nw[3 * v + 1]; nz = nw[3 * v + 2]; }
    const float ax = arm[3 * v], ay = arm[3 * v + 1], az = arm[3 * v + 2];
    const float* const pt = p + 3 * (size_t)M;                          // the tau half
    float tx = 0.f, ty = 0.f, tz = 0.f, rx = 0.f, ry = 0.f, rz = 0.f;
    if constexpr (K > 0) {
        unsigned int n[K]; float wj[K], wnj[K], ox[K], oy[K], oz[K], hx[K], hy[K], hz[K]; float4 qn[K];
#pragma unroll
        for (int j = 0; j < K; ++j) { n[j] = keys[v * K + j]; wj[j] = w[v * K + j]; wnj[j] = wn[v * K + j]; }
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const unsigned int nc = min(n[j], (unsigned int)(M - 1));            // clamped gather; the entry is skipped below if n >= M
            ox[j] = p[3 * nc]; oy[j] = p[3 * nc + 1]; oz[j] = p[3 * nc + 2];
            hx[j] = pt[3 * nc]; hy[j] = pt[3 * nc + 1]; hz[j] = pt[3 * nc + 2];
            qn[j] = qc[nc];
        }
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (n[j] < (unsigned int)M) {
                const float gx = hx[j] - (oy[j] * qn[j].z - oz[j] * qn[j].y), gy = hy[j] - (oz[j] * qn[j].x - ox[j] * qn[j].z),
                            gz = hz[j] - (ox[j] * qn[j].y - oy[j] * qn[j].x);
                tx = tx + wj[j] * gx; ty = ty + wj[j] * gy; tz = tz + wj[j] * gz;
                rx = rx + wnj[j] * ox[j]; ry = ry + wnj[j] * oy[j]; rz = rz + wnj[j] * oz[j];
            }
    } else {
        for (int j = 0; j < k; ++j) {
            const int e = v * k + j;
            const unsigned int n = keys[e];
            if (n < (unsigned int)M) {
                const float wj = w[e], wnj = wn[e];
                const float4 qn = qc[n];
                const float ox = p[3 * n], oy = p[3 * n + 1], oz = p[3 * n + 2];
                const float gx = pt[3 * n] - (oy * qn.z - oz * qn.y), gy = pt[3 * n + 1] - (oz * qn.x - ox * qn.z), gz = pt[3 * n + 2] - (ox * qn.y - oy * qn.x);
                tx = tx + wj * gx; ty = ty + wj * gy; tz = tz + wj * gz;
                rx = rx + wnj * ox; ry = ry + wnj * oy; rz = rz + wnj * oz;
            }
        }
    }
    float sx = tx + (ry * az - rz * ay), sy = ty + (rz * ax - rx * az), sz = tz + (rx * ay - ry * ax);
    if constexpr (PLANE) {
        const float d = (nx * sx + ny * sy) + nz * sz;
        const bool valid = keys[v * k] < (unsigned int)M;               // (a point's k entries are valid together)
        sx = valid ? nx * d : 0.f; sy = valid ? ny * d : 0.f; sz = valid ? nz * d : 0.f;
    }
    sv_rigid_store(rec, v, sx, sy, sz, ax, ay, az);
}

// ---- the record of a right-hand side u that no J p made (a round's b): see sv_rigid_store
__global__ __launch_bounds__(256) void df_sv_rigid_pack_kernel(const float* __restrict__ u, const float* __restrict__ arm, int N,
                                                               float4* __restrict__ rec)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= N) return;
    sv_rigid_store(rec, v, u[3 * v], u[3 * v + 1], u[3 * v + 2], arm[3 * v], arm[3 * v + 1], arm[3 * v + 2]);
}

// ---- out = J^T u (+ lambda_rot * p_om, + lambda * p_tau) : df_sv_wt_apply_kernel's walk, thread stride and tree with six sums a node,
// S1 = sum w u (the tau part) and S2 = sum wn (a_v x u); the omega part is S2 - (q_n x S1).
__global__ __launch_bounds__(256) void df_sv_rigid_jt_apply_kernel(const unsigned int* __restrict__ off, const unsigned int* __restrict__ sorted_pt,
                                                                   const float* __restrict__ sorted_w, const float* __restrict__ sorted_wn, int M,
                                                                   const float4* __restrict__ rec, const float4* __restrict__ qc, float lambda,
                                                                   float lambda_rot,
                                                                   const float* __restrict__ p, float* __restrict__ out,
                                                                   const float* __restrict__ active)
{
    __shared__ float lds[6 * 128];
    if (active && *active == 0.f) return;                               // see df_sv_w_apply_kernel
    const int n = blockIdx.x, t = threadIdx.x;
    const unsigned int b = off[n], e_end = off[n + 1];
    float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (unsigned int i = b + t; i < e_end; i += 256) {
        const unsigned int v = sorted_pt[i];
        const float we = sorted_w[i], wne = sorted_wn[i];
        const float4 uv = rec[2 * (size_t)v], xv = rec[2 * (size_t)v + 1];   // (u, a_v x u): sv_rigid_store
        s[0] = s[0] + we * uv.x; s[1] = s[1] + we * uv.y; s[2] = s[2] + we * uv.z;
        s[3] = s[3] + wne * xv.x; s[4] = s[4] + wne * xv.y; s[5] = s[5] + wne * xv.z;
    }
    sv_node_tree(s, lds, [&]() {
        const float4 qn = qc[n];
        float om[3] = {s[3] - (qn.y * s[2] - qn.z * s[1]), s[4] - (qn.z * s[0] - qn.x * s[2]), s[5] - (qn.x * s[1] - qn.y * s[0])};
        float* const ot = out + 3 * (size_t)M;
        if (p) {
            const float* const pt = p + 3 * (size_t)M;
            for (int q = 0; q < 3; ++q) { om[q] = om[q] + lambda_rot * p[3 * n + q]; s[q] = s[q] + lambda * pt[3 * n + q]; }
        }
        for (int q = 0; q < 3; ++q) { out[3 * n + q] = om[q]; ot[3 * n + q] = s[q]; }
    });
}

// ---- per edge e = (i -> j) and round: g_e = T_i(v_j) - c_j (the regularisation residual) and b_e = T_i(v_j) - c_i (the arm omega_i turns)
__global__ __launch_bounds__(256) void df_sv_rigid_edge_kernel(const int* __restrict__ nbr, const float4* __restrict__ pos_sigma,
                                                               const float4* __restrict__ rot, const float4* __restrict__ dual,
                                                               const float4* __restrict__ c, int E, int kg, float* __restrict__ g,
                                                               float* __restrict__ arm)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int i = e / kg, j = nbr[e];
    const float4 ci = c[i], cj = c[j];
    const f3 ti = sv_node_transform(rot, dual, i, pos_sigma[j]);
    g[3 * e] = ti.x - cj.x; g[3 * e + 1] = ti.y - cj.y; g[3 * e + 2] = ti.z - cj.z;
    arm[3 * e] = ti.x - ci.x; arm[3 * e + 1] = ti.y - ci.y; arm[3 * e + 2] = ti.z - ci.z;
}

// ---- the regularisation on the six unknowns, one thread per node, df_sv_reg_apply_kernel's sum orders.  Per edge d_e = g_e (RHS) or
// (p_tau_i + (p_om_i x b_e)) - p_tau_j, formed in the thread.  tau_n: + alpha_e d_e over the outgoing edges in slot order, then
// - alpha_e d_e over the incoming edges in ascending edge id; om_n: + alpha_e (b_e x d_e) over the outgoing edges.
// RHS: out = out - lambda_reg * acc (out holds J^T Omega b) ; else out = out + lambda_reg * acc (out holds (J^T Omega J + damping) p).
template <bool RHS>
__global__ __launch_bounds__(256) void df_sv_rigid_reg_kernel(const int* __restrict__ nbr, const float* __restrict__ alpha,
                                                              const unsigned int* __restrict__ in_off, const unsigned int* __restrict__ in_edge,
                                                              int M, int kg, const float* __restrict__ g, const float* __restrict__ arm,
                                                              const float* __restrict__ p, float lambda_reg, float* __restrict__ out,
                                                              const float* __restrict__ active)
{
    if (active && *active == 0.f) return;                               // see df_sv_w_apply_kernel
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= M) return;
    const float* const pt = RHS ? nullptr : p + 3 * (size_t)M;
    float on[3] = {0.f, 0.f, 0.f}, tn[3] = {0.f, 0.f, 0.f};
    if constexpr (!RHS) for (int q = 0; q < 3; ++q) { on[q] = p[3 * n + q]; tn[q] = pt[3 * n + q]; }
    float acc_o[3] = {0.f, 0.f, 0.f}, acc_t[3] = {0.f, 0.f, 0.f};
    for (int s = 0; s < kg; ++s) {
        const int e = n * kg + s;
        const float a = alpha[e];
        const float bx = arm[3 * e], by = arm[3 * e + 1], bz = arm[3 * e + 2];
        float d[3];
        if constexpr (RHS) { d[0] = g[3 * e]; d[1] = g[3 * e + 1]; d[2] = g[3 * e + 2]; }
        else {
            const int j = nbr[e];
            d[0] = (tn[0] + (on[1] * bz - on[2] * by)) - pt[3 * j];
            d[1] = (tn[1] + (on[2] * bx - on[0] * bz)) - pt[3 * j + 1];
            d[2] = (tn[2] + (on[0] * by - on[1] * bx)) - pt[3 * j + 2];
        }
        for (int q = 0; q < 3; ++q) acc_t[q] = acc_t[q] + a * d[q];
        acc_o[0] = acc_o[0] + a * (by * d[2] - bz * d[1]);
        acc_o[1] = acc_o[1] + a * (bz * d[0] - bx * d[2]);
        acc_o[2] = acc_o[2] + a * (bx * d[1] - by * d[0]);
    }
    for (unsigned int i = in_off[n]; i < in_off[n + 1]; ++i) {
        const unsigned int e = in_edge[i], t = e / (unsigned int)kg;     // the edge t -> n
        const float a = alpha[e];
        float d[3];
        if constexpr (RHS) { d[0] = g[3 * e]; d[1] = g[3 * e + 1]; d[2] = g[3 * e + 2]; }
        else {
            const float bx = arm[3 * e], by = arm[3 * e + 1], bz = arm[3 * e + 2];
            const float ox = p[3 * t], oy = p[3 * t + 1], oz = p[3 * t + 2];
            d[0] = (pt[3 * t] + (oy * bz - oz * by)) - tn[0];
            d[1] = (pt[3 * t + 1] + (oz * bx - ox * bz)) - tn[1];
            d[2] = (pt[3 * t + 2] + (ox * by - oy * bx)) - tn[2];
        }
        for (int q = 0; q < 3; ++q) acc_t[q] = acc_t[q] - a * d[q];
    }
    float* const ot = out + 3 * (size_t)M;
    for (int q = 0; q < 3; ++q) {
        if constexpr (RHS) { out[3 * n + q] = out[3 * n + q] - lambda_reg * acc_o[q]; ot[3 * n + q] = ot[3 * n + q] - lambda_reg * acc_t[q]; }
        else { out[3 * n + q] = out[3 * n + q] + lambda_reg * acc_o[q]; ot[3 * n + q] = ot[3 * n + q] + lambda_reg * acc_t[q]; }
    }
}

// ---- write back.  A node whose six update components are all exactly 0 keeps its eight floats; otherwise
//   qo = normalize((1, om / 2)),  r' = qo * normalize(rot),  t' = (qo (t - c) + c) + tau,  dual' = 0.5 (0, t') r'
// -- correctly rounded operations only (no sin / cos), so that the restatement is exact.
__global__ __launch_bounds__(256) void df_sv_rigid_writeback_kernel(const float4* __restrict__ rot, const float4* __restrict__ dual,
                                                                    const float4* __restrict__ node_t, const float4* __restrict__ c,
                                                                    const float* __restrict__ x, int M, float* __restrict__ dq_out)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= M) return;
    const float4 r4 = rot[n], d4 = dual[n], t4 = node_t[n], cn = c[n];
    const float* const xt = x + 3 * (size_t)M;
    const float ox = x[3 * n], oy = x[3 * n + 1], oz = x[3 * n + 2], tx = xt[3 * n], ty = xt[3 * n + 1], tz = xt[3 * n + 2];
    float* o = dq_out + 8 * (size_t)n;
    if (ox == 0.f && oy == 0.f && oz == 0.f && tx == 0.f && ty == 0.f && tz == 0.f) {
        o[0] = r4.x; o[1] = r4.y; o[2] = r4.z; o[3] = r4.w; o[4] = d4.x; o[5] = d4.y; o[6] = d4.z; o[7] = d4.w;
        return;
    }
    const quat r = sv_quat(r4);
    quat qo; qo.w = 1.f; qo.x = 0.5f * ox; qo.y = 0.5f * oy; qo.z = 0.5f * oz;
    qo = q_normalize(qo);
    const quat r1 = q_mul(qo, q_normalize(r));
    quat zero; zero.w = 0.f; zero.x = 0.f; zero.y = 0.f; zero.z = 0.f;
    const f3 turned = dq_transform(qo, zero, mk3(t4.y - cn.x, t4.z - cn.y, t4.w - cn.z));
    quat T; T.w = 0.f; T.x = (turned.x + cn.x) + tx; T.y = (turned.y + cn.y) + ty; T.z = (turned.z + cn.z) + tz;
    const quat d = q_mul(q_scale(0.5f, T), r1);
    o[0] = r1.w; o[1] = r1.x; o[2] = r1.y; o[3] = r1.z; o[4] = d.w; o[5] = d.x; o[6] = d.y; o[7] = d.z;
}

// ---------------------------------------------------------------- 6x6 node-block Jacobi preconditioner of the solve with rotations
// dfusion_warp_set_preconditioner(1): per round the diagonal block B_n of every node of J^T Omega J + lambda_reg L + damping over its six
// unknowns (omega_n, tau_n), factored B_n = L L^T in f32, and a conjugate-gradient recurrence preconditioned with them: z = B^-1 r is two
// triangular substitutions in the node's thread, inside the init and step kernels, so a step launches what it launched.  The rule, sum
// for sum, is restated in tests/solver_precond_ref.py.  Entry (i, j), i <= j, of a block sits at SV_UP(i, j) of its 21 upper-triangle
// entries, L_ij (j <= i) at SV_LO(i, j); 0..2 = omega x y z, 3..5 = tau x y z.
#define SV_UP(i, j) ((i) * 6 - (i) * ((i) - 1) / 2 + ((j) - (i)))
#define SV_LO(i, j) ((i) * ((i) + 1) / 2 + (j))
#define SV_PC_PLANES 22             // fac [22][M]: the 21 entries of L, then 1 (factored) or 0 (a pivot failed: the identity)

// OO entries from the six sums xx xy xz yy yz zz of outer products: |m|^2 I - m m^T
__device__ __forceinline__ void sv_pc_rotation_part(const float (&P)[6], float (&out)[6])
{
    out[0] = P[3] + P[5]; out[1] = -P[1]; out[2] = -P[2]; out[3] = P[0] + P[5]; out[4] = -P[4]; out[5] = P[0] + P[3];
}

// ---- the blocks and their factors: df_sv_rigid_jt_apply_kernel's walk, thread stride and tree over the node's list with, per entry,
// m = w q_n - wn a_v and m' = w' q_n - wn' a_v (w', wn': the Tukey-scaled copies, or the lists themselves):
//   point-to-point, 10 sums: P_cd += m'_c m_d (c <= d), K_c += w' m_c, T += w' w ; PLANE, 21 sums: B_ij += h'_i h_j, h = (n' x m, w n'),
//   h' = (n' x m', w' n').
// Lane 0 then adds the graph term (kg > 0: outgoing edges in slot order, incoming in ascending edge id) and the damping, factors the
// block and stores the factor.
template <bool PLANE>
__global__ __launch_bounds__(256) void df_sv_pc_blocks_kernel(const unsigned int* __restrict__ off, const unsigned int* __restrict__ sorted_pt,
                                                              const float* __restrict__ sw, const float* __restrict__ swn,
                                                              const float* __restrict__ sw_use, const float* __restrict__ swn_use, int M,
                                                              const float* __restrict__ a, const float4* __restrict__ qc,
                                                              const float* __restrict__ nw, const float* __restrict__ alpha,
                                                              const unsigned int* __restrict__ in_off, const unsigned int* __restrict__ in_edge,
                                                              int kg, const float* __restrict__ arm, float lambda_reg, float lambda,
                                                              float lambda_rot, float* __restrict__ fac)
{
    constexpr int S = PLANE ? 21 : 10;
    __shared__ float lds[S * 128];
    const int n = blockIdx.x, t = threadIdx.x;
    const unsigned int b0 = off[n], e_end = off[n + 1];
    const float4 qn = qc[n];
    float s[S];
#pragma unroll
    for (int c = 0; c < S; ++c) s[c] = 0.f;
    for (unsigned int i = b0 + t; i < e_end; i += 256) {
        const unsigned int v = sorted_pt[i];
        const float we = sw[i], wne = swn[i], wse = sw_use[i], wnse = swn_use[i];
        const float ax = a[3 * v], ay = a[3 * v + 1], az = a[3 * v + 2];
        const float m[3] = {we * qn.x - wne * ax, we * qn.y - wne * ay, we * qn.z - wne * az};
        const float ms[3] = {wse * qn.x - wnse * ax, wse * qn.y - wnse * ay, wse * qn.z - wnse * az};
        if constexpr (PLANE) {
            const float nx = nw[3 * v], ny = nw[3 * v + 1], nz = nw[3 * v + 2];
            const float h[6] = {ny * m[2] - nz * m[1], nz * m[0] - nx * m[2], nx * m[1] - ny * m[0], we * nx, we * ny, we * nz};
            const float hs[6] = {ny * ms[2] - nz * ms[1], nz * ms[0] - nx * ms[2], nx * ms[1] - ny * ms[0], wse * nx, wse * ny, wse * nz};
#pragma unroll
            for (int i6 = 0; i6 < 6; ++i6)
#pragma unroll
                for (int j6 = i6; j6 < 6; ++j6) s[SV_UP(i6, j6)] = s[SV_UP(i6, j6)] + hs[i6] * h[j6];
        } else {
            s[0] = s[0] + ms[0] * m[0]; s[1] = s[1] + ms[0] * m[1]; s[2] = s[2] + ms[0] * m[2];
            s[3] = s[3] + ms[1] * m[1]; s[4] = s[4] + ms[1] * m[2]; s[5] = s[5] + ms[2] * m[2];
            s[6] = s[6] + wse * m[0]; s[7] = s[7] + wse * m[1]; s[8] = s[8] + wse * m[2];
            s[9] = s[9] + wse * we;
        }
    }
    sv_node_tree(s, lds, [&]() {
        float B[21];
        if constexpr (PLANE) {
#pragma unroll
            for (int c = 0; c < 21; ++c) B[c] = s[c];
        } else {
#pragma unroll
            for (int c = 0; c < 21; ++c) B[c] = 0.f;
            const float P[6] = {s[0], s[1], s[2], s[3], s[4], s[5]};
            float oo[6];
            sv_pc_rotation_part(P, oo);
            B[SV_UP(0, 0)] = oo[0]; B[SV_UP(0, 1)] = oo[1]; B[SV_UP(0, 2)] = oo[2]; B[SV_UP(1, 1)] = oo[3]; B[SV_UP(1, 2)] = oo[4]; B[SV_UP(2, 2)] = oo[5];
            B[SV_UP(0, 4)] = s[8]; B[SV_UP(0, 5)] = -s[7]; B[SV_UP(1, 3)] = -s[8]; B[SV_UP(1, 5)] = s[6]; B[SV_UP(2, 3)] = s[7]; B[SV_UP(2, 4)] = -s[6];
            B[SV_UP(3, 3)] = s[9]; B[SV_UP(4, 4)] = s[9]; B[SV_UP(5, 5)] = s[9];
        }
        if (kg > 0) {
            float Q[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, KB[3] = {0.f, 0.f, 0.f}, AT = 0.f;
            for (int sl = 0; sl < kg; ++sl) {
                const int e = n * kg + sl;
                const float al = alpha[e];
                const float bx = arm[3 * e], by = arm[3 * e + 1], bz = arm[3 * e + 2];
                const float abx = al * bx, aby = al * by, abz = al * bz;
                Q[0] = Q[0] + abx * bx; Q[1] = Q[1] + abx * by; Q[2] = Q[2] + abx * bz; Q[3] = Q[3] + aby * by; Q[4] = Q[4] + aby * bz; Q[5] = Q[5] + abz * bz;
                KB[0] = KB[0] + abx; KB[1] = KB[1] + aby; KB[2] = KB[2] + abz;
                AT = AT + al;
            }
            for (unsigned int i = in_off[n]; i < in_off[n + 1]; ++i) AT = AT + alpha[in_edge[i]];
            float oo[6];
            sv_pc_rotation_part(Q, oo);
            B[SV_UP(0, 0)] = B[SV_UP(0, 0)] + lambda_reg * oo[0]; B[SV_UP(0, 1)] = B[SV_UP(0, 1)] + lambda_reg * oo[1];
            B[SV_UP(0, 2)] = B[SV_UP(0, 2)] + lambda_reg * oo[2]; B[SV_UP(1, 1)] = B[SV_UP(1, 1)] + lambda_reg * oo[3];
            B[SV_UP(1, 2)] = B[SV_UP(1, 2)] + lambda_reg * oo[4]; B[SV_UP(2, 2)] = B[SV_UP(2, 2)] + lambda_reg * oo[5];
            B[SV_UP(0, 4)] = B[SV_UP(0, 4)] + lambda_reg * -KB[2]; B[SV_UP(0, 5)] = B[SV_UP(0, 5)] + lambda_reg * KB[1];
            B[SV_UP(1, 3)] = B[SV_UP(1, 3)] + lambda_reg * KB[2]; B[SV_UP(1, 5)] = B[SV_UP(1, 5)] + lambda_reg * -KB[0];
            B[SV_UP(2, 3)] = B[SV_UP(2, 3)] + lambda_reg * -KB[1]; B[SV_UP(2, 4)] = B[SV_UP(2, 4)] + lambda_reg * KB[0];
            const float tt = lambda_reg * AT;
            B[SV_UP(3, 3)] = B[SV_UP(3, 3)] + tt; B[SV_UP(4, 4)] = B[SV_UP(4, 4)] + tt; B[SV_UP(5, 5)] = B[SV_UP(5, 5)] + tt;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) { B[SV_UP(i, i)] = B[SV_UP(i, i)] + lambda_rot; B[SV_UP(i + 3, i + 3)] = B[SV_UP(i + 3, i + 3)] + lambda; }
        // Cholesky by rows; a pivot that is not > 0 or not finite makes the node's preconditioner the identity
        float L[21];
        bool ok = true;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                float sum = B[SV_UP(j, i)];
#pragma unroll
                for (int k = 0; k < j; ++k) sum = sum - L[SV_LO(i, k)] * L[SV_LO(j, k)];
                if (i == j) { ok = ok && sum > 0.f && isfinite(sum); L[SV_LO(i, i)] = sqrtf(sum); }
                else L[SV_LO(i, j)] = sum / L[SV_LO(j, j)];
            }
#pragma unroll
        for (int c = 0; c < 21; ++c) fac[(size_t)c * M + n] = L[c];
        fac[(size_t)21 * M + n] = ok ? 1.f : 0.f;
    });
}

// z = B_n^-1 r for the six values of node n (r[0..2] omega, r[3..5] tau): forward and back substitution, k ascending in both
__device__ __forceinline__ void sv_pc_apply(const float* __restrict__ fac, int M, int n, const float (&r)[6], float (&z)[6])
{
    float L[21];
#pragma unroll
    for (int c = 0; c < 21; ++c) L[c] = fac[(size_t)c * M + n];
    const bool ok = fac[(size_t)21 * M + n] != 0.f;
    float y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        float t = r[i];
#pragma unroll
        for (int k = 0; k < i; ++k) t = t - L[SV_LO(i, k)] * y[k];
        y[i] = t / L[SV_LO(i, i)];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        float t = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) t = t - L[SV_LO(k, i)] * z[k];
        z[i] = t / L[SV_LO(i, i)];
    }
    if (!ok) {
#pragma unroll
        for (int i = 0; i < 6; ++i) z[i] = r[i];
    }
}

// The vector kernels of the preconditioned recurrence are organised by node: thread t owns nodes t, t + 1024, ... with all six values
// of each (entry n and entry M + n of the 2M-entry arrays).  A dot product adds, per node and component, the omega product and then the
// tau product to the thread's partial; then sv_block_sum3 and the coupling (s0 + s1) + s2.  scal[SV_RR] holds r . z.
__device__ __forceinline__ void sv_pc_load(const float* __restrict__ v, int M, int n, float (&o)[6])
{
#pragma unroll
    for (int c = 0; c < 3; ++c) { o[c] = v[3 * n + c]; o[3 + c] = v[3 * ((size_t)M + n) + c]; }
}
__device__ __forceinline__ void sv_pc_store(float* __restrict__ v, int M, int n, const float (&o)[6])
{
#pragma unroll
    for (int c = 0; c < 3; ++c) { v[3 * n + c] = o[c]; v[3 * ((size_t)M + n) + c] = o[3 + c]; }
}
__device__ __forceinline__ void sv_pc_dot(float (&s)[3], const float (&u)[6], const float (&v)[6])
{
#pragma unroll
    for (int c = 0; c < 3; ++c) { s[c] = s[c] + u[c] * v[c]; s[c] = s[c] + u[3 + c] * v[3 + c]; }
}

// x0 = 0, z0 = B^-1 r0, p0 = z0, r . z
__global__ __launch_bounds__(SV_BLOCK) void df_sv_pc_init_kernel(const float* __restrict__ r, int M, float* __restrict__ x, float* __restrict__ p,
                                                                 float* __restrict__ scal, const float* __restrict__ fac)
{
    __shared__ float lds[3 * SV_BLOCK];
    float s[3] = {0.f, 0.f, 0.f};
    const float zero[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int n = threadIdx.x; n < M; n += SV_BLOCK) {
        float rv[6], zv[6];
        sv_pc_load(r, M, n, rv);
        sv_pc_apply(fac, M, n, rv, zv);
        sv_pc_store(x, M, n, zero);
        sv_pc_store(p, M, n, zv);
        sv_pc_dot(s, rv, zv);
    }
    sv_block_sum3(s, lds);
    sv_cg_couple<true>(s);
    if (threadIdx.x == 0) {
        for (int c = 0; c < 3; ++c) { scal[SV_RR + c] = s[c]; scal[SV_RR0 + c] = s[c]; }
        scal[SV_ACTIVE] = (float)(s[0] > 0.f);
    }
}

// A step: alpha = r.z / p.q ; x += alpha p ; r -= alpha q ; z = B^-1 r ; beta = (r.z)_new / (r.z)_old ; p = z + beta p ; frozen once
// (r.z)_new <= 1e-10 (r.z)_0 or alpha == 0 (sv_cg_alpha / sv_cg_beta / sv_cg_freeze on r . z).  NPT > 0: M <= NPT * SV_BLOCK, and p and
// q -- then z in q's place -- are read once and stay in registers through the three passes (df_sv_step_reg_kernel's variants, counted in
// nodes: 1, 3 and 4 for 2M <= 2, 5, 8 x 1024; x, r and the factor are needed by the middle pass alone, which reads them node by node);
// NPT = 0: any M, every pass reads what it needs.  Same node -> thread assignment, same sums, same trees either way.
template <int NPT>
__global__ __launch_bounds__(SV_BLOCK) void df_sv_pc_step_kernel(const float* __restrict__ q, int M, float* __restrict__ x, float* __restrict__ r,
                                                                 float* __restrict__ p, float* __restrict__ scal, const float* __restrict__ fac)
{
    __shared__ float lds[3 * SV_BLOCK];
    if (scal[SV_ACTIVE] == 0.f) return;                                 // frozen: the step would change nothing
    constexpr int R = NPT > 0 ? NPT : 1;
    float pv[R][6], qv[R][6];
    float pq[3] = {0.f, 0.f, 0.f};
    if constexpr (NPT > 0) {
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            const int n = threadIdx.x + j * SV_BLOCK;
            if (n < M) { sv_pc_load(p, M, n, pv[j]); sv_pc_load(q, M, n, qv[j]); }
        }
#pragma unroll
        for (int j = 0; j < NPT; ++j)
            if (threadIdx.x + j * SV_BLOCK < M) sv_pc_dot(pq, pv[j], qv[j]);
    } else {
        for (int n = threadIdx.x; n < M; n += SV_BLOCK) {
            sv_pc_load(p, M, n, pv[0]); sv_pc_load(q, M, n, qv[0]);
            sv_pc_dot(pq, pv[0], qv[0]);
        }
    }
    sv_block_sum3(pq, lds);
    sv_cg_couple<true>(pq);
    float alpha[3], rz_old[3];
    for (int c = 0; c < 3; ++c) { rz_old[c] = scal[SV_RR + c]; alpha[c] = sv_cg_alpha(pq[c], rz_old[c]); }
    float rz[3] = {0.f, 0.f, 0.f};
    // x, r and z of one node; z takes q's place in qn, which has served
    auto update = [&](int n, const float (&pn)[6], float (&qn)[6]) {
        float xn[6], rn[6];
        sv_pc_load(x, M, n, xn); sv_pc_load(r, M, n, rn);
#pragma unroll
        for (int c = 0; c < 6; ++c) { xn[c] = xn[c] + alpha[c % 3] * pn[c]; rn[c] = rn[c] - alpha[c % 3] * qn[c]; }
        sv_pc_store(x, M, n, xn); sv_pc_store(r, M, n, rn);
        sv_pc_apply(fac, M, n, rn, qn);
        sv_pc_dot(rz, rn, qn);
    };
    if constexpr (NPT > 0) {
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            const int n = threadIdx.x + j * SV_BLOCK;
            if (n < M) update(n, pv[j], qv[j]);
        }
    } else {
        for (int n = threadIdx.x; n < M; n += SV_BLOCK) {
            sv_pc_load(p, M, n, pv[0]); sv_pc_load(q, M, n, qv[0]);
            update(n, pv[0], qv[0]);
        }
        __syncthreads();                                                // (the last pass reads r back)
    }
    sv_block_sum3(rz, lds);
    sv_cg_couple<true>(rz);
    float beta[3];
    for (int c = 0; c < 3; ++c) beta[c] = sv_cg_beta(alpha[c], rz[c], rz_old[c]);
    if constexpr (NPT > 0) {
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            const int n = threadIdx.x + j * SV_BLOCK;
            if (n < M) {
#pragma unroll
                for (int c = 0; c < 6; ++c) pv[j][c] = qv[j][c] + beta[c % 3] * pv[j][c];
                sv_pc_store(p, M, n, pv[j]);
            }
        }
    } else {
        // z is recomputed from the stored r: the same operations on the same values, so the same bits as in the pass above
        for (int n = threadIdx.x; n < M; n += SV_BLOCK) {
            float rn[6];
            sv_pc_load(p, M, n, pv[0]); sv_pc_load(r, M, n, rn);
            sv_pc_apply(fac, M, n, rn, qv[0]);
#pragma unroll
            for (int c = 0; c < 6; ++c) pv[0][c] = qv[0][c] + beta[c % 3] * pv[0][c];
            sv_pc_store(p, M, n, pv[0]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) sv_cg_freeze<true>(alpha, rz, scal);
}

// ---------------------------------------------------------------- host side
// 256-byte aligned pieces of one buffer.  A carve-up is written once and run twice: from base 0, where `at` ends as the size to
// reserve, and from the reserved buffer's address.
struct SvBump {
    uintptr_t at;
    template <typename T> T* take(size_t count)
    {
        T* const p = (T*)at;
        at += (count * sizeof(T) + 255) & ~(uintptr_t)255;
        return p;
    }
};

// scratch bytes of the stable radix sort of E (key, value) pairs of unsigned int on key bits [0, end_bit)
static int df_sv_sort_bytes(size_t E, int end_bit, hipStream_t st, size_t* bytes)
{
    *bytes = 0;
    DF_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, *bytes, (const unsigned int*)nullptr, (unsigned int*)nullptr, (const unsigned int*)nullptr,
                                              (unsigned int*)nullptr, (int)E, 0, end_bit, st));
    return DF_OK;
}

// The node graph of the handle for `kg` neighbours, made on first use and kept until the node set or the hierarchy setting changes
// (graph_kg = 0).
static int df_sv_graph(DfWarpField* wf, int kg, dfStream stream)
{
    if (wf->graph_kg == kg) return DF_OK;
    hipStream_t st = (hipStream_t)stream;
    const int M = wf->M, kq = kg + 1;
    const size_t E = (size_t)M * kg;
    wf->graph_kg = 0;
    int rc;
    if ((rc = wf->graph_nbr.reserve(E)) || (rc = wf->graph_alpha.reserve(E)) || (rc = wf->graph_in_off.reserve((size_t)M + 2)) ||
        (rc = wf->graph_in_edge.reserve(E))) return rc;
    size_t sort_bytes;
    if ((rc = df_sv_sort_bytes(E, 16, st, &sort_bytes))) return rc;
    float *pos3, *d2; int* idx; unsigned int *keys, *vals, *skeys; char* sort;
    auto carve = [&](char* base) {
        SvBump b{(uintptr_t)base};
        pos3 = b.take<float>((size_t)M * 3); idx = b.take<int>((size_t)M * kq); d2 = b.take<float>((size_t)M * kq);
        keys = b.take<unsigned int>(E); vals = b.take<unsigned int>(E); skeys = b.take<unsigned int>(E); sort = b.take<char>(sort_bytes);
        return (size_t)(b.at - (uintptr_t)base);
    };
    if ((rc = wf->graph_ws.reserve(carve(nullptr)))) return rc;
    carve(wf->graph_ws);
    const dim3 gM((M + 255) / 256);
    // the edges: the hierarchy's (dfusion_warp_graph.hip) where the handle asks for one and it has a level to offer, else the flat graph
    memset(wf->graph_sizes, 0, sizeof(wf->graph_sizes));
    wf->graph_sizes[0] = M; wf->graph_eff = 0;                         // (without the setting there are no levels: S_0 alone)
    if (wf->hier_levels > 0 && (rc = df_hg_build(wf, kg, keys, vals, st))) return rc;
    if (wf->graph_eff == 0) {
        hipLaunchKernelGGL(df_sv_graph_pos_kernel, gM, dim3(256), 0, st, wf->pos_sigma, M, pos3);
        DF_LAUNCH_CHECK();
        if ((rc = dfusion_knn(wf, kq, pos3, M, idx, d2, stream))) return rc;
        hipLaunchKernelGGL(df_sv_graph_kernel, gM, dim3(256), 0, st, idx, wf->pos_sigma, M, kg, wf->graph_nbr.p, wf->graph_alpha.p, keys, vals);
        DF_LAUNCH_CHECK();
    }
    DF_HIP(hipcub::DeviceRadixSort::SortPairs(sort, sort_bytes, keys, skeys, vals, wf->graph_in_edge.p, (int)E, 0, 16, st));   // stable
    hipLaunchKernelGGL(df_sv_offsets_kernel, dim3((unsigned)((E + 1 + 255) / 256)), dim3(256), 0, st, skeys, (int)E, M, wf->graph_in_off);
    DF_LAUNCH_CHECK();
    wf->graph_kg = kg;
    return DF_OK;
}

// The solve's scratch, carved from wf->solver_ws.  E = N * k entries, Eg = M * kg graph edges.
struct SvWorkspace {
    int* idx; float* d2;                                    // [E] the k-NN's output
    float* w; unsigned int *keys, *vals;                    // [E] point-major entries: weight, node id (M: invalid point), entry id
    unsigned int *skeys, *svals;                            // [E] the sort's output
    unsigned int* spt; float* sw;                           // [E] node-major entries: point id, weight
    float *e0, *u;                                          // [3N] residual the round starts at ; W p, then the final residual
    unsigned int* off;                                      // [M + 2] node offsets into the node-major entries
    float *x, *r, *p, *q;                                   // [3M] conjugate gradients
    float* scal;                                            // [SV_SCAL_N]
    float* dq;                                              // [8M] the transforms a round writes
    float* g;                                               // [3Eg] edge values
    float* rho;                                             // [N] point-to-plane: n . e (otherwise empty)
    float *omega, *sw_scaled;                               // [N], [E] Tukey: point weights, sorted_w' (no Tukey: empty)
    float *alpha_scaled, *omega_e;                          // [Eg] Huber: alpha', edge weights (no Huber: empty)
    float *y, *nw, *a; float4 *c, *qc, *rec; float* arm;    // rigid: [3N] warped points, warped normals (with normals), a_v ; [M] node
    float *wn, *swn, *swn_scaled;                           // centres c_n, q_n ; [2N] J^T's point records ; [3Eg] edge arms ; [E] normalised
                                                            // weights point-major, node-major, Tukey (otherwise empty; x, r, p, q: 6M floats)
    float* fac;                                             // rigid with the preconditioner: [SV_PC_PLANES][M] block factors (otherwise empty)
    char* sort; size_t sort_bytes;
};

static int df_sv_workspace(DfWarpField* wf, int N, int k, int M, int Eg, bool plane, bool tukey, bool huber, bool rigid, bool precond, hipStream_t st,
                           SvWorkspace* ws)
{
    const size_t E = (size_t)N * k, n = N, m = M, eg = Eg, mx = rigid ? 2 * m : m;
    int rc;
    if ((rc = df_sv_sort_bytes(E, 17, st, &ws->sort_bytes))) return rc;
    auto carve = [&](char* base) {
        SvBump b{(uintptr_t)base};
        ws->idx = b.take<int>(E); ws->d2 = b.take<float>(E); ws->w = b.take<float>(E);
        ws->keys = b.take<unsigned int>(E); ws->vals = b.take<unsigned int>(E);
        ws->skeys = b.take<unsigned int>(E); ws->svals = b.take<unsigned int>(E);
        ws->spt = b.take<unsigned int>(E); ws->sw = b.take<float>(E);
        ws->e0 = b.take<float>(3 * n); ws->u = b.take<float>(3 * n); ws->off = b.take<unsigned int>(m + 2);
        ws->x = b.take<float>(3 * mx); ws->r = b.take<float>(3 * mx); ws->p = b.take<float>(3 * mx); ws->q = b.take<float>(3 * mx);
        ws->scal = b.take<float>(SV_SCAL_N); ws->dq = b.take<float>(8 * m); ws->g = b.take<float>(3 * eg);
        ws->rho = b.take<float>(plane ? n : 0);
        ws->omega = b.take<float>(tukey ? n : 0); ws->sw_scaled = b.take<float>(tukey ? E : 0);
        ws->alpha_scaled = b.take<float>(huber ? eg : 0); ws->omega_e = b.take<float>(huber ? eg : 0);
        ws->y = b.take<float>(rigid ? 3 * n : 0); ws->nw = b.take<float>(rigid && plane ? 3 * n : 0);
        ws->a = b.take<float>(rigid ? 3 * n : 0); ws->c = b.take<float4>(rigid ? m : 0); ws->qc = b.take<float4>(rigid ? m : 0); ws->rec = b.take<float4>(rigid ? 2 * n : 0);
        ws->arm = b.take<float>(rigid ? 3 * eg : 0); ws->wn = b.take<float>(rigid ? E : 0); ws->swn = b.take<float>(rigid ? E : 0);
        ws->swn_scaled = b.take<float>(rigid && tukey ? E : 0);
        ws->fac = b.take<float>(precond ? SV_PC_PLANES * m : 0);
        ws->sort = b.take<char>(ws->sort_bytes);
        return (size_t)(b.at - (uintptr_t)base);
    };
    if ((rc = wf->solver_ws.reserve(carve(nullptr)))) return rc;
    carve(wf->solver_ws);
    return DF_OK;
}

// The node-major side of the entries, from the point-major keys / vals the setup kernel wrote: the stable sort by node id, the node
// offsets, and the node-major copy of the point ids with the weights `w` (and, for the solve with rotations, of a second weight list).
static int df_sv_lists(const SvWorkspace& ws, int E, int k, int M, const float* w, float* sw, const float* w2, float* sw2, hipStream_t st)
{
    size_t sort_bytes = ws.sort_bytes;
    const dim3 gE((unsigned)(((size_t)E + 255) / 256));
    DF_HIP(hipcub::DeviceRadixSort::SortPairs(ws.sort, sort_bytes, ws.keys, ws.skeys, ws.vals, ws.svals, E, 0, 17, st));   // stable
    hipLaunchKernelGGL(df_sv_offsets_kernel, dim3((unsigned)(((size_t)E + 1 + 255) / 256)), dim3(256), 0, st, ws.skeys, E, M, ws.off);
    DF_LAUNCH_CHECK();
    hipLaunchKernelGGL(df_sv_sorted_kernel, gE, dim3(256), 0, st, ws.svals, w, E, k, ws.spt, sw);
    if (w2) hipLaunchKernelGGL(df_sv_sorted_kernel, gE, dim3(256), 0, st, ws.svals, w2, E, k, ws.spt, sw2);
    DF_LAUNCH_CHECK();
    return DF_OK;
}

// One solve, as its entry point describes it and df_sv_check has checked and normalised it (kg = 0 means no regularisation).
// `rounds` solves, each from the transforms the one before wrote; tukey_c / huber_delta = 0: that penalty is quadratic and its kernels
// are not launched, so rounds = 1 with both 0 is the plain solve, launch for launch.  `energy` (nullable) holds n_energy floats:
// 2 = {E_data before, after}, 4 = with {E_reg before, after}, which are 0 without the term.  `normals` (nullable) switches the data term
// to point-to-plane; lambda_rot is the solve with rotations' alone.
struct SvSolve {
    DfWarpField* wf; int k; const float *canonical, *live, *normals; int N;
    int iters; float lambda, lambda_rot; int kg; float lambda_reg; int rounds; float tukey_c, huber_delta;
    float *dq_out, *energy; int n_energy; float *point_weights, *edge_weights; dfStream stream;
    int precond;                                            // dfusion_warp_solve_rigid alone: the handle's preconditioner setting (others leave it 0)
};

// The CG kernels by the number of unknown entries X (x, r, p, q stay in registers up to 8 * SV_BLOCK of them), and an apply kernel
// template <K, PLANE> by the neighbour count (compile-time for 8 and 4).
typedef void (*SvInitKernel)(const float*, int, float*, float*, float*);
typedef void (*SvStepKernel)(const float*, int, float*, float*, float*, float*);
typedef void (*SvPcStepKernel)(const float*, int, float*, float*, float*, float*, const float*);   // the preconditioned step, by M nodes
static SvPcStepKernel df_sv_pc_step_for(int M)
{
    return 2 * M <= 2 * SV_BLOCK ? df_sv_pc_step_kernel<1> : 2 * M <= 5 * SV_BLOCK ? df_sv_pc_step_kernel<3>
         : 2 * M <= 8 * SV_BLOCK ? df_sv_pc_step_kernel<4> : df_sv_pc_step_kernel<0>;
}
template <bool COUPLED> static SvStepKernel df_sv_step_for(int X)
{
    return X <= 2 * SV_BLOCK ? df_sv_step_reg_kernel<2, COUPLED> : X <= 5 * SV_BLOCK ? df_sv_step_reg_kernel<5, COUPLED>
         : X <= 8 * SV_BLOCK ? df_sv_step_reg_kernel<8, COUPLED> : df_sv_step_kernel<COUPLED>;
}
#define SV_APPLY_FOR(kernel, PLANE, k) ((k) == 8 ? kernel<8, PLANE> : (k) == 4 ? kernel<4, PLANE> : kernel<0, PLANE>)

// What both round loops work with, made once per call by df_sv_context: the flags, the sizes and grids, the workspace, the pointers to
// what W^T / J^T and the regularisation read (the scaled copies, or the lists as they are; the handle's cached alpha is only read), the CG
// kernels -- and the stages both loops launch, in which a term that is switched off launches nothing.
struct SvContext {                                          // (df_sv_context fills the members in this order)
    SvSolve s; hipStream_t st;
    bool rigid, reg, tukey, huber, plane;
    int M, X, E, Eg;                                        // X: the unknown entries, M or (rigid) 2M
    float c2, dd2;
    dim3 gN, gM, gE, gG, gW, one;
    SvWorkspace ws;
    const float *sw_use, *swn_use, *alpha_use, *active; float* en;
    SvInitKernel init; SvStepKernel step;
    SvPcStepKernel pc_step;                                 // non-null: the recurrence is preconditioned with the node blocks in ws.fac
    // Once per call, what depends only on the canonical points and the node positions (the graph is the context's already): the k-NN,
    // `setup` (the entries' weights and node ids, point-major), the node offsets and the node-major lists (w2 / sw2: see df_sv_lists)
    template <typename Setup> int prepare(Setup setup, const float* w2, float* sw2) const
    {
        int rc;
        if ((rc = dfusion_knn(s.wf, s.k, s.canonical, s.N, ws.idx, ws.d2, s.stream))) return rc;   // getWeightsAndUpdateKNN's k-NN (NaN queries are masked by `setup`)
        if ((rc = setup())) return rc;
        DF_LAUNCH_CHECK();
        return df_sv_lists(ws, E, s.k, M, ws.w, ws.sw, w2, sw2, st);
    }
    // rho = n . e in ws.rho and, with b, b = n rho
    void plane_rho(const float* e, const float* n, float* b) const { hipLaunchKernelGGL(df_sv_plane_rho_kernel, gN, dim3(256), 0, st, e, n, ws.keys, s.N, s.k, M, ws.rho, b); }
    // Tukey: omega from the residual the round starts at (ws.e0; plane: ws.rho), multiplied into copies of the node-major lists
    int tukey_weights() const
    {
        hipLaunchKernelGGL(plane ? df_sv_tukey_kernel<true> : df_sv_tukey_kernel<false>, gN, dim3(256), 0, st, plane ? ws.rho : ws.e0, s.N, c2, ws.omega);
        hipLaunchKernelGGL(df_sv_scale_list_kernel, gE, dim3(256), 0, st, ws.spt, ws.sw, ws.omega, E, ws.sw_scaled);
        if (rigid) hipLaunchKernelGGL(df_sv_scale_list_kernel, gE, dim3(256), 0, st, ws.spt, ws.swn, ws.omega, E, ws.swn_scaled);
        DF_LAUNCH_CHECK();
        return DF_OK;
    }
    // Huber: omega_e from the round's g_e, multiplied into a copy of alpha
    void huber_weights() const { hipLaunchKernelGGL(df_sv_huber_kernel, gG, dim3(256), 0, st, ws.g, s.wf->graph_alpha.p, Eg, s.huber_delta, dd2, ws.omega_e, ws.alpha_scaled); }
    // the data energy of the residual e (plane: of ws.rho, which holds n . e)
    void data_energy(const float* e, float* out) const
    {
        if (plane || tukey) {
            const auto one_value = !plane ? df_sv_point_energy_kernel<false, true> : tukey ? df_sv_point_energy_kernel<true, true> : df_sv_point_energy_kernel<true, false>;
            hipLaunchKernelGGL(one_value, one, dim3(SV_BLOCK), 0, st, plane ? ws.rho : e, s.N, c2, out);
        }
        else hipLaunchKernelGGL(df_sv_energy_kernel, one, dim3(SV_BLOCK), 0, st, e, s.N, out);
    }
    // the regularisation energy of ws.g at the update x (nullable = 0); the energies weigh an edge with alpha_e itself, not alpha'_e
    void reg_energy(const float* x, float* out) const
    {
        const DfWarpField* wf = s.wf;
        if (huber) hipLaunchKernelGGL(df_sv_huber_energy_kernel, one, dim3(SV_BLOCK), 0, st, wf->graph_nbr.p, wf->graph_alpha.p, ws.g, x, Eg, s.kg, s.huber_delta, dd2, out);
        else hipLaunchKernelGGL(df_sv_reg_energy_kernel, one, dim3(SV_BLOCK), 0, st, wf->graph_nbr.p, wf->graph_alpha.p, ws.g, x, Eg, s.kg, out);
    }
    // conjugate gradients from the right-hand side in ws.r: x0 = 0, p0 = r0, then `iters` steps of q = A p by the caller's launches
    // (apply: ws.p -> the point side ; apply_t: the point side -> ws.q, damping included ; reg_apply: ws.q += lambda_reg L ws.p).
    // With pc_step the init and the step are the preconditioned ones over ws.fac: the same number of launches.
    template <typename Apply, typename ApplyT, typename RegApply> int cg(Apply apply, ApplyT apply_t, RegApply reg_apply) const
    {
        if (pc_step) hipLaunchKernelGGL(df_sv_pc_init_kernel, one, dim3(SV_BLOCK), 0, st, ws.r, M, ws.x, ws.p, ws.scal, ws.fac);
        else hipLaunchKernelGGL(init, one, dim3(SV_BLOCK), 0, st, ws.r, X, ws.x, ws.p, ws.scal);
        DF_LAUNCH_CHECK();
        for (int it = 0; it < s.iters; ++it) {
            apply();
            apply_t();
            if (reg) reg_apply();
            if (pc_step) hipLaunchKernelGGL(pc_step, one, dim3(SV_BLOCK), 0, st, ws.q, M, ws.x, ws.r, ws.p, ws.scal, ws.fac);
            else hipLaunchKernelGGL(step, one, dim3(SV_BLOCK), 0, st, ws.q, X, ws.x, ws.r, ws.p, ws.scal);
            DF_LAUNCH_CHECK();
        }
        return DF_OK;
    }
    // What a solve hands back besides the transforms it set: the energies (a call without the regularisation term reports 0 for it),
    // the last round's transforms and weights (1 everywhere for a penalty that is off).
    int outputs() const
    {
        if (s.energy) {
            DF_HIP(hipMemcpyAsync(s.energy, en, (reg ? s.n_energy : 2) * sizeof(float), hipMemcpyDeviceToDevice, st));
            static const float zeros[2] = {0.f, 0.f};                   // (a copy from the host, not a fill: no kernel of any kind is added)
            if (!reg && s.n_energy == 4) DF_HIP(hipMemcpyAsync(s.energy + 2, zeros, sizeof(zeros), hipMemcpyHostToDevice, st));
        }
        if (s.dq_out) DF_HIP(hipMemcpyAsync(s.dq_out, ws.dq, (size_t)M * 32, hipMemcpyDeviceToDevice, st));
        if (s.point_weights) {
            if (tukey) DF_HIP(hipMemcpyAsync(s.point_weights, ws.omega, (size_t)s.N * 4, hipMemcpyDeviceToDevice, st));
            else DF_HIP(hipMemsetD32Async((hipDeviceptr_t)s.point_weights, 0x3f800000, (size_t)s.N, st));
        }
        if (s.edge_weights) {
            if (huber) DF_HIP(hipMemcpyAsync(s.edge_weights, ws.omega_e, (size_t)Eg * 4, hipMemcpyDeviceToDevice, st));
            else DF_HIP(hipMemsetD32Async((hipDeviceptr_t)s.edge_weights, 0x3f800000, (size_t)Eg, st));
        }
        return DF_OK;
    }
};

static int df_sv_context(const SvSolve& s, bool rigid, SvContext* cx)
{
    DfWarpField* const wf = s.wf;
    SvWorkspace ws;
    const bool reg = s.kg > 0, tukey = s.tukey_c != 0.f, huber = reg && s.huber_delta != 0.f, plane = s.normals != nullptr;
    const int M = wf->M, X = rigid ? 2 * M : M, E = s.N * s.k, Eg = M * s.kg;
    int rc;
    const bool precond = rigid && s.precond == 1;
    if ((rc = df_sv_workspace(wf, s.N, s.k, M, Eg, plane, tukey, huber, rigid, precond, (hipStream_t)s.stream, &ws))) return rc;
    if (reg && (rc = df_sv_graph(wf, s.kg, s.stream))) return rc;     // (the first call on a handle allocates graph_alpha, read just below)
    // one recurrence over all components where the matrix mixes them: point-to-plane, and the six unknowns of a node
    const bool coupled = plane || rigid;
    *cx = SvContext{s, (hipStream_t)s.stream, rigid, reg, tukey, huber, plane, M, X, E, Eg, s.tukey_c * s.tukey_c, s.huber_delta * s.huber_delta,
                    dim3((s.N + 255) / 256), dim3((M + 255) / 256), dim3((unsigned)(((size_t)E + 255) / 256)), dim3((Eg + 255) / 256), dim3(M), dim3(1), ws,
                    tukey ? ws.sw_scaled : ws.sw, tukey ? ws.swn_scaled : ws.swn, huber ? ws.alpha_scaled : wf->graph_alpha.p,
                    ws.scal + SV_ACTIVE, ws.scal + SV_ENERGY, coupled ? df_sv_init_kernel<true> : df_sv_init_kernel<false>,
                    coupled ? df_sv_step_for<true>(X) : df_sv_step_for<false>(X), precond ? df_sv_pc_step_for(M) : nullptr};
    return DF_OK;
}

// The translation solve behind the first four entry points.  With `normals` the residual a round starts at becomes rho = n . e0 (the
// energies and the Tukey weights read it), the right-hand side W^T (n rho), W p is projected, and the three CG recurrences become one.
static int df_sv_rounds(const SvSolve& s)
{
    SvContext cx;
    int rc;
    if ((rc = df_sv_context(s, false, &cx))) return rc;
    DfWarpField* const wf = s.wf; const SvWorkspace& ws = cx.ws; hipStream_t st = cx.st;
    const int N = s.N, k = s.k, kg = s.kg, M = cx.M; const bool plane = cx.plane; const dim3 gN = cx.gN, gM = cx.gM, gW = cx.gW;
    const auto w_apply = SV_APPLY_FOR(df_sv_w_apply_kernel, false, k);
    const auto wp_apply = plane ? SV_APPLY_FOR(df_sv_w_apply_kernel, true, k) : w_apply;   // W p inside the CG loop: projected on the normals
    // the entries' weights and node ids, with e0 at the transforms the handle holds now; the normals only add to what makes a point invalid
    if ((rc = cx.prepare([&]() {
            hipLaunchKernelGGL(plane ? df_sv_setup_kernel<true> : df_sv_setup_kernel<false>, gN, dim3(256), 0, st, s.canonical, s.live, s.normals, N, k, ws.idx, ws.d2,
                               wf->pos_sigma, wf->node_t, M, ws.w, ws.keys, ws.vals, ws.e0);
            return DF_OK;
        }, nullptr, nullptr))) return rc;
    for (int round = 0; round < s.rounds; ++round) {
        const bool first = round == 0, last = round == s.rounds - 1;
        if (!first) {                                                   // e0 at the transforms the previous round wrote
            hipLaunchKernelGGL(df_sv_round_e0_kernel, gN, dim3(256), 0, st, s.canonical, s.live, N, k, ws.keys, ws.w, wf->node_t.p, M, ws.e0);
            DF_LAUNCH_CHECK();
        }
        if (plane) {                                                    // rho of e0, and b = n rho in u
            cx.plane_rho(ws.e0, s.normals, ws.u);
            DF_LAUNCH_CHECK();
        }
        if (cx.tukey && (rc = cx.tukey_weights())) return rc;
        if (s.energy && first) { cx.data_energy(ws.e0, cx.en); DF_LAUNCH_CHECK(); }
        // r0 = W^T Omega e0 - lambda_reg * b' (plane: W^T Omega n rho)
        hipLaunchKernelGGL(df_sv_wt_apply_kernel, gW, dim3(256), 0, st, ws.off, ws.spt, cx.sw_use, M, plane ? ws.u : ws.e0, 0.f, (const float*)nullptr, ws.r, (const float*)nullptr);
        DF_LAUNCH_CHECK();
        if (cx.reg) {
            hipLaunchKernelGGL(df_sv_reg_edge_kernel, cx.gG, dim3(256), 0, st, wf->graph_nbr.p, wf->pos_sigma.p, wf->rot.p, wf->dual.p, cx.Eg, kg, ws.g);
            if (cx.huber) cx.huber_weights();
            hipLaunchKernelGGL(df_sv_reg_rhs_kernel, gM, dim3(256), 0, st, cx.alpha_use, wf->graph_in_off.p, wf->graph_in_edge.p, M, kg, ws.g, s.lambda_reg, ws.r);
            if (s.energy && first) cx.reg_energy(nullptr, cx.en + 2);
            DF_LAUNCH_CHECK();
        }
        rc = cx.cg([&]() { hipLaunchKernelGGL(wp_apply, gN, dim3(256), 0, st, ws.w, ws.keys, N, k, M, ws.p, ws.u, cx.active, s.normals); },
                   [&]() { hipLaunchKernelGGL(df_sv_wt_apply_kernel, gW, dim3(256), 0, st, ws.off, ws.spt, cx.sw_use, M, ws.u, s.lambda, ws.p, ws.q, cx.active); },
                   [&]() { hipLaunchKernelGGL(df_sv_reg_apply_kernel, gM, dim3(256), 0, st, wf->graph_nbr.p, cx.alpha_use, wf->graph_in_off.p, wf->graph_in_edge.p, M, kg,
                                              ws.p, s.lambda_reg, ws.q, cx.active); });
        if (rc) return rc;
        if (s.energy && last) {                                         // the energies of the final residual e0 - W x, which is linear in x
            hipLaunchKernelGGL(w_apply, gN, dim3(256), 0, st, ws.w, ws.keys, N, k, M, ws.x, ws.u, (const float*)nullptr, (const float*)nullptr);
            hipLaunchKernelGGL(df_sv_residual_kernel, dim3((unsigned)((3 * (size_t)N + 255) / 256)), dim3(256), 0, st, ws.e0, ws.u, 3 * N, ws.u);
            if (plane) cx.plane_rho(ws.u, s.normals, nullptr);
            cx.data_energy(ws.u, cx.en + 1);
            if (cx.reg) cx.reg_energy(ws.x, cx.en + 3);
            DF_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(df_sv_writeback_kernel, gM, dim3(256), 0, st, wf->rot.p, wf->node_t.p, ws.x, M, ws.dq);
        DF_LAUNCH_CHECK();
        if ((rc = dfusion_warp_set_transforms(wf, ws.dq, s.stream))) return rc;   // (the handle's rot / dual / node_t are the new ones from here on)
    }
    return cx.outputs();
}

// The solve behind dfusion_warp_solve_rigid (arguments checked by df_sv_check and the entry point).  df_sv_rounds'
// shape: one workspace, one preparation, `rounds` rounds, a term that is switched off launches nothing -- but every round starts with the
// warp of the canonical points (and normals) at the transforms the handle holds, and the unknowns are 2M entries.
static int df_sv_rigid_rounds(const SvSolve& s)
{
    static const float ident[12] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
    SvContext cx;
    int rc;
    if ((rc = df_sv_context(s, true, &cx))) return rc;
    DfWarpField* const wf = s.wf; const SvWorkspace& ws = cx.ws; hipStream_t st = cx.st;
    const int N = s.N, k = s.k, kg = s.kg, M = cx.M; const bool plane = cx.plane; const dim3 gN = cx.gN, gM = cx.gM, gW = cx.gW;
    const auto j_apply = plane ? SV_APPLY_FOR(df_sv_rigid_j_apply_kernel, true, k) : SV_APPLY_FOR(df_sv_rigid_j_apply_kernel, false, k);
    // y, n' at the transforms the handle holds now: copies through the point path with an identity warp_to_live
    auto warp = [&]() -> int {
        DF_HIP(hipMemcpyAsync(ws.y, s.canonical, (size_t)N * 12, hipMemcpyDeviceToDevice, st));
        if (plane) DF_HIP(hipMemcpyAsync(ws.nw, s.normals, (size_t)N * 12, hipMemcpyDeviceToDevice, st));
        return dfusion_warp_points(wf, k, ws.y, plane ? ws.nw : nullptr, N, ident, s.stream);
    };
    // e = live - y in e0 (plane: rho = n' . e in ws.rho); with b for a round's solve: a_v too, and (plane) n' rho in u
    auto residual = [&](bool b) {
        hipLaunchKernelGGL(df_sv_rigid_residual_kernel, gN, dim3(256), 0, st, s.live, ws.y, ws.keys, ws.w, wf->node_t.p, N, k, M, ws.e0, b ? ws.a : (float*)nullptr);
        if (plane) cx.plane_rho(ws.e0, ws.nw, b ? ws.u : nullptr);
    };
    auto centres = [&]() { hipLaunchKernelGGL(df_sv_rigid_centre_kernel, gM, dim3(256), 0, st, wf->pos_sigma.p, wf->rot.p, wf->dual.p, wf->node_t.p, M, ws.c, ws.qc); };
    auto edges = [&]() {
        hipLaunchKernelGGL(df_sv_rigid_edge_kernel, cx.gG, dim3(256), 0, st, wf->graph_nbr.p, wf->pos_sigma.p, wf->rot.p, wf->dual.p, ws.c, cx.Eg, kg, ws.g, ws.arm);
    };
    // the first round's warp (it decides validity too), then the entries with their normalised weights as a second list
    if ((rc = cx.prepare([&]() -> int {
            const int rw = warp();
            if (rw) return rw;
            hipLaunchKernelGGL(df_sv_rigid_setup_kernel, gN, dim3(256), 0, st, s.canonical, s.live, s.normals, ws.y, ws.nw, N, k, ws.idx, ws.d2, wf->pos_sigma.p, M,
                               ws.w, ws.wn, ws.keys, ws.vals);
            return DF_OK;
        }, ws.wn, ws.swn))) return rc;
    for (int round = 0; round < s.rounds; ++round) {
        const bool first = round == 0;
        if (!first && (rc = warp())) return rc;
        centres();
        residual(true);
        DF_LAUNCH_CHECK();
        if (cx.tukey && (rc = cx.tukey_weights())) return rc;
        if (s.energy && first) { cx.data_energy(ws.e0, cx.en); DF_LAUNCH_CHECK(); }
        // r0 = J^T Omega b - lambda_reg * acc(g)
        hipLaunchKernelGGL(df_sv_rigid_pack_kernel, gN, dim3(256), 0, st, plane ? ws.u : ws.e0, ws.a, N, ws.rec);
        hipLaunchKernelGGL(df_sv_rigid_jt_apply_kernel, gW, dim3(256), 0, st, ws.off, ws.spt, cx.sw_use, cx.swn_use, M, ws.rec, ws.qc, 0.f, 0.f,
                           (const float*)nullptr, ws.r, (const float*)nullptr);
        DF_LAUNCH_CHECK();
        if (cx.reg) {
            edges();
            if (cx.huber) cx.huber_weights();
            hipLaunchKernelGGL(df_sv_rigid_reg_kernel<true>, gM, dim3(256), 0, st, wf->graph_nbr.p, cx.alpha_use, wf->graph_in_off.p, wf->graph_in_edge.p, M, kg, ws.g,
                               ws.arm, (const float*)nullptr, s.lambda_reg, ws.r, (const float*)nullptr);
            if (s.energy && first) cx.reg_energy(nullptr, cx.en + 2);
            DF_LAUNCH_CHECK();
        }
        if (cx.pc_step) {                                               // the round's node blocks, factored (one launch a round)
            hipLaunchKernelGGL(plane ? df_sv_pc_blocks_kernel<true> : df_sv_pc_blocks_kernel<false>, gW, dim3(256), 0, st, ws.off, ws.spt, ws.sw, ws.swn,
                               cx.sw_use, cx.swn_use, M, ws.a, ws.qc, ws.nw, cx.alpha_use, wf->graph_in_off.p, wf->graph_in_edge.p, kg, ws.arm, s.lambda_reg,
                               s.lambda, s.lambda_rot, ws.fac);
            DF_LAUNCH_CHECK();
        }
        rc = cx.cg([&]() { hipLaunchKernelGGL(j_apply, gN, dim3(256), 0, st, ws.w, ws.wn, ws.keys, N, k, M, ws.p, ws.a, ws.qc, ws.rec, cx.active, ws.nw); },
                   [&]() { hipLaunchKernelGGL(df_sv_rigid_jt_apply_kernel, gW, dim3(256), 0, st, ws.off, ws.spt, cx.sw_use, cx.swn_use, M, ws.rec, ws.qc, s.lambda,
                                              s.lambda_rot, ws.p, ws.q, cx.active); },
                   [&]() { hipLaunchKernelGGL(df_sv_rigid_reg_kernel<false>, gM, dim3(256), 0, st, wf->graph_nbr.p, cx.alpha_use, wf->graph_in_off.p, wf->graph_in_edge.p,
                                              M, kg, ws.g, ws.arm, ws.p, s.lambda_reg, ws.q, cx.active); });
        if (rc) return rc;
        hipLaunchKernelGGL(df_sv_rigid_writeback_kernel, gM, dim3(256), 0, st, wf->rot.p, wf->dual.p, wf->node_t.p, ws.c, ws.x, M, ws.dq);
        DF_LAUNCH_CHECK();
        if ((rc = dfusion_warp_set_transforms(wf, ws.dq, s.stream))) return rc;   // (the handle's rot / dual / node_t are the new ones from here on)
    }
    if (s.energy) {                                                     // the true energies behind the last write-back
        if ((rc = warp())) return rc;
        residual(false);
        cx.data_energy(ws.e0, cx.en + 1);
        if (cx.reg) { centres(); edges(); cx.reg_energy(nullptr, cx.en + 3); }
        DF_LAUNCH_CHECK();
    }
    return cx.outputs();
}

// The arguments of every entry point, in the order they have always been checked: the ones all share, `own_ok` (what only the calling
// entry point takes: the normals it requires, lambda_rot), the robust ones.  DF_OK, with s->kg = 0 where the regularisation is switched
// off (kg == 0 or lambda_reg == 0: checked first, so an out-of-range kg is refused whatever lambda_reg is), or DF_E_INVALID.
static int df_sv_check(SvSolve* s, bool own_ok = true)
{
    const DfWarpField* wf = s->wf;
    if (!wf || !s->canonical || !s->live || s->N <= 0 || s->iters < 0 || !(s->lambda >= 0.f) || wf->M <= 0 || s->k < 1 || s->k > 8 || wf->M < s->k) return DF_E_INVALID;
    if ((size_t)s->N * s->k > 0x7fffffffu) return DF_E_INVALID;
    if (s->kg < 0 || s->kg > 7 || (s->kg > 0 && wf->M < s->kg + 1) || !(s->lambda_reg >= 0.f)) return DF_E_INVALID;
    if (s->lambda_reg == 0.f) s->kg = 0;
    if (!own_ok) return DF_E_INVALID;
    if (s->rounds < 1 || !(s->tukey_c >= 0.f) || !(s->huber_delta >= 0.f) || (s->edge_weights && s->kg == 0)) return DF_E_INVALID;
    return DF_OK;
}

extern "C" int dfusion_warp_solve_data_term(DfWarpField* wf, int k, const float* canonical, const float* live, int N, int iters, float lambda,
                                            float* dq_out, float* energy, dfStream stream)
{
    SvSolve s = {wf, k, canonical, live, nullptr, N, iters, lambda, 0.f, 0, 0.f, 1, 0.f, 0.f, dq_out, energy, 2, nullptr, nullptr, stream};
    return df_sv_check(&s) ? DF_E_INVALID : df_sv_rounds(s);
}

extern "C" int dfusion_warp_solve(DfWarpField* wf, int k, const float* canonical, const float* live, int N, int iters, float lambda, int kg,
                                  float lambda_reg, float* dq_out, float* energy, dfStream stream)
{
    SvSolve s = {wf, k, canonical, live, nullptr, N, iters, lambda, 0.f, kg, lambda_reg, 1, 0.f, 0.f, dq_out, energy, 4, nullptr, nullptr, stream};
    return df_sv_check(&s) ? DF_E_INVALID : df_sv_rounds(s);
}

extern "C" int dfusion_warp_solve_robust(DfWarpField* wf, int k, const float* canonical, const float* live, int N, int iters, float lambda, int kg,
                                         float lambda_reg, int rounds, float tukey_c, float huber_delta, float* dq_out, float* energy,
                                         float* point_weights, float* edge_weights, dfStream stream)
{
    SvSolve s = {wf, k, canonical, live, nullptr, N, iters, lambda, 0.f, kg, lambda_reg, rounds, tukey_c, huber_delta, dq_out, energy, 4, point_weights, edge_weights, stream};
    return df_sv_check(&s) ? DF_E_INVALID : df_sv_rounds(s);
}

extern "C" int dfusion_warp_solve_plane(DfWarpField* wf, int k, const float* canonical, const float* live, const float* normals, int N, int iters,
                                        float lambda, int kg, float lambda_reg, int rounds, float tukey_c, float huber_delta, float* dq_out,
                                        float* energy, float* point_weights, float* edge_weights, dfStream stream)
{
    SvSolve s = {wf, k, canonical, live, normals, N, iters, lambda, 0.f, kg, lambda_reg, rounds, tukey_c, huber_delta, dq_out, energy, 4, point_weights, edge_weights, stream};
    return df_sv_check(&s, normals != nullptr) ? DF_E_INVALID : df_sv_rounds(s);
}

extern "C" int dfusion_warp_solve_rigid(DfWarpField* wf, int k, const float* canonical, const float* live, const float* normals, int N, int iters,
                                        float lambda, float lambda_rot, int kg, float lambda_reg, int rounds, float tukey_c, float huber_delta,
                                        float* dq_out, float* energy, float* point_weights, float* edge_weights, dfStream stream)
{
    SvSolve s = {wf, k, canonical, live, normals, N, iters, lambda, lambda_rot, kg, lambda_reg, rounds, tukey_c, huber_delta, dq_out, energy, 4, point_weights, edge_weights, stream, wf ? wf->precond : 0};
    return df_sv_check(&s, lambda_rot >= 0.f) ? DF_E_INVALID : df_sv_rigid_rounds(s);
}

extern "C" int dfusion_warp_set_preconditioner(DfWarpField* wf, int mode)
{
    if (!wf || (mode != 0 && mode != 1)) return DF_E_INVALID;
    wf->precond = mode;
    return DF_OK;
}

extern "C" int dfusion_warp_preconditioner(const DfWarpField* wf, int* mode)
{
    if (!wf || !mode) return DF_E_INVALID;
    *mode = wf->precond;
    return DF_OK;
}

extern "C" int dfusion_warp_node_graph(DfWarpField* wf, int kg, int* nbr, float* alpha, dfStream stream)
{
    if (!wf || !nbr || kg < 1 || kg > 7 || wf->M < kg + 1) return DF_E_INVALID;
    const int rc = df_sv_graph(wf, kg, stream);
    if (rc) return rc;
    const size_t E = (size_t)wf->M * kg;
    DF_HIP(hipMemcpyAsync(nbr, wf->graph_nbr, E * sizeof(int), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (alpha) DF_HIP(hipMemcpyAsync(alpha, wf->graph_alpha, E * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return DF_OK;
}

extern "C" int dfusion_warp_graph_levels(DfWarpField* wf, int kg, int* top, int* sizes, int* effective, dfStream stream)
{
    if (!wf || kg < 1 || kg > 7 || wf->M < kg + 1) return DF_E_INVALID;
    const int rc = df_sv_graph(wf, kg, stream);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool hier = wf->hier_levels > 0;                             // (without the setting no top[] is made: every node's is 0)
    if (top && hier) DF_HIP(hipMemcpyAsync(top, wf->graph_top, (size_t)wf->M * sizeof(int), hipMemcpyDeviceToDevice, st));
    if (top && !hier) DF_HIP(hipMemsetAsync(top, 0, (size_t)wf->M * sizeof(int), st));
    if (sizes) DF_HIP(hipMemcpyAsync(sizes, wf->graph_sizes, sizeof(wf->graph_sizes), hipMemcpyHostToDevice, st));
    if (effective) DF_HIP(hipMemcpyAsync(effective, &wf->graph_eff, sizeof(int), hipMemcpyHostToDevice, st));
    return DF_OK;
}
