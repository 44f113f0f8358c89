// dfusion_mesh.hip -- dfusion_extract_mesh: a triangle mesh of the fused surface (no reference counterpart: the reference stops at the
// unordered cloud of fetchCloud).  Marching tetrahedra on the Kuhn subdivision of every voxel cell; the rule -- which edges carry a
// vertex, where it lies, which triangles a tetrahedron gives, and the order of everything -- is stated in include/dfusion.h and
// DESIGN.md and restated in numpy by tests/mesh_ref.py, against which the output is compared bit for bit.
//
// Work unit: a wave-item of 256 x-adjacent voxels (a lane owns 4; dims[0] % 4 == 0, so a lane never straddles a row, an item may).
//   count     streams the owner planes like df_extract_kernel's scan phase (contiguous 16 KiB runs per workgroup, non-temporal
//             16-byte loads); a wave whose item holds a valid voxel fetches the +x / +y / +z / +y+z neighbours, counts the item's
//             vertices and triangles and writes both.  No LDS and no barrier: the waves of a workgroup never wait for each other.
//   scan      hipcub exclusive sums over the two per-item count arrays (one spare element at the end receives the total).
//   vertices  every item with vertices recomputes its edge masks, writes its vertices at base + ballot / popcount prefix (voxel, then
//             slot) and leaves, per lane that has any, {index of its first vertex, 28-bit edge mask} in a compact table.  Table
//             entries are handed out by an atomic counter, which orders NOTHING a caller sees: the item's record {lanes with an
//             entry, first entry} finds them.  The table has min(vertex_capacity, lanes) entries (a lane with an entry has a vertex),
//             so the workspace is bounded by what the caller asked for: 8 bytes per vertex, not bytes per voxel.
//   triangles every item with triangles reads the table records of the 8 lane-quads its cells' edges belong to (own + next quad of
//             rows y, y+1 in planes z, z+1) and writes its triangles at the item's scanned base in cell, tetrahedron, triangle order.
// The order of the output is part of the contract, so nothing a caller sees depends on an atomic or on a float reduction.
#include <hipcub/hipcub.hpp>
#include "dfusion_internal.h"

// ---- the case table, derived by geometry at compile time
// Tetrahedron t of a cell belongs to the axis permutation (a, b, c) = DF_MT_PERM[t] (lexicographic: xyz, xzy, yxz, yzx, zxy, zyx); its
// corners are the cell corners (bit 0 = +x, bit 1 = +y, bit 2 = +z) v0 = 0, v1 = e_a, v2 = e_a + e_b, v3 = 7.  The edge between local
// corners i < j is owned by v_i, in slot (v_j - v_i) - 1.  A case m has bit i set iff v_i is inside.
//   one corner i apart from j < k < l   (ij, ik, il)
//   i < j inside, k < l outside         (ik, il, jl), (ik, jl, jk)
// A triangle is then turned so that (p1 - p0) x (p2 - p0) points from the inside corners to the outside ones; the test below runs on
// the edge midpoints of the unit cell (in doubled integer coordinates), which have the orientation of any points on the open edges.
// Entry: bits 0-1 = number of triangles, then six 6-bit edge codes (owner corner << 3 | slot).
struct DfMtTable { unsigned long long e[6 * 16]; };
constexpr int DF_MT_PERM[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

constexpr DfMtTable df_mt_make()
{
    DfMtTable T{};
    for (int t = 0; t < 6; ++t) {
        const int v[4] = {0, 1 << DF_MT_PERM[t][0], (1 << DF_MT_PERM[t][0]) | (1 << DF_MT_PERM[t][1]), 7};
        for (int m = 0; m < 16; ++m) {
            int in[4] = {}, out[4] = {}, n_in = 0, n_out = 0;
            for (int i = 0; i < 4; ++i) { if ((m >> i) & 1) in[n_in++] = i; else out[n_out++] = i; }
            int tri[2][3][2] = {}, n = 0;                                  // [triangle][vertex] = local corner pair
            if (n_in == 1 || n_in == 3) {
                const int i = n_in == 1 ? in[0] : out[0];
                const int* o = n_in == 1 ? out : in;                        // j < k < l
                for (int q = 0; q < 3; ++q) { tri[0][q][0] = i; tri[0][q][1] = o[q]; }
                n = 1;
            } else if (n_in == 2) {
                const int i = in[0], j = in[1], k = out[0], l = out[1];
                const int quad[4][2] = {{i, k}, {i, l}, {j, l}, {j, k}};
                const int pick[2][3] = {{0, 1, 2}, {0, 2, 3}};
                for (int r = 0; r < 2; ++r) for (int q = 0; q < 3; ++q) { tri[r][q][0] = quad[pick[r][q]][0]; tri[r][q][1] = quad[pick[r][q]][1]; }
                n = 2;
            }
            bool flip = false;
            if (n) {
                int p[3][3] = {}, d[3] = {};                               // doubled midpoints of triangle 0; n_in * sum(out) - n_out * sum(in)
                for (int q = 0; q < 3; ++q) for (int c = 0; c < 3; ++c) p[q][c] = ((v[tri[0][q][0]] >> c) & 1) + ((v[tri[0][q][1]] >> c) & 1);
                for (int c = 0; c < 3; ++c) {
                    int so = 0, si = 0;
                    for (int q = 0; q < n_out; ++q) so += (v[out[q]] >> c) & 1;
                    for (int q = 0; q < n_in; ++q) si += (v[in[q]] >> c) & 1;
                    d[c] = n_in * so - n_out * si;
                }
                const int a[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
                const int b[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
                const int nx = a[1] * b[2] - a[2] * b[1], ny = a[2] * b[0] - a[0] * b[2], nz = a[0] * b[1] - a[1] * b[0];
                flip = nx * d[0] + ny * d[1] + nz * d[2] < 0;
            }
            unsigned long long e = (unsigned long long)n;
            for (int r = 0; r < n; ++r)
                for (int q = 0; q < 3; ++q) {
                    const int s = flip && q ? 3 - q : q;                   // (p0, p2, p1); both triangles of a quad together
                    int lo = tri[r][s][0], hi = tri[r][s][1];
                    if (lo > hi) { const int x = lo; lo = hi; hi = x; }
                    const unsigned long long code = (unsigned long long)((v[lo] << 3) | ((v[hi] - v[lo]) - 1));
                    e |= code << (2 + 6 * (3 * r + q));
                }
            T.e[t * 16 + m] = e;
        }
    }
    return T;
}
__constant__ const DfMtTable c_df_mt = df_mt_make();

// ---- arguments
struct DfMeshItemQ { unsigned long long lanes; unsigned int first; unsigned int pad; };   // lanes with a table entry; the first one's index
struct DfMeshArgs {
    const uint32_t* vol;               // plane z_own0
    int X, Y, nz, z_own0;              // owner planes [z_own0, z_own0 + nz); cells in all of them but the last
    float vsx, vsy, vsz;
    DfAff aff;
    size_t n4, n_items;                // lane-items (4 voxels), wave-items (256 voxels)
    unsigned long long *vbase, *tbase; // [n_items + 1] counts, then exclusive sums
    DfMeshItemQ* itemq;                // [n_items]
    uint2* qtab; unsigned long long qcap; unsigned int* qcount;
    float4* verts; unsigned long long vcap;
    uint32_t* tris; unsigned long long tcap;
};

// a voxel counts iff W != 0 && F != 1.f (dfusion_raycast.hip ex_valid: the extractor's rule); inside iff its tsdf is < 0
__device__ __forceinline__ bool mt_valid(uint32_t v) { return (v >> 16) != 0u && (v & 0xffffu) != 0x3c00u; }

// A lane's 4 voxels (x0 .. x0 + 3, y, z) and everything their edges and cells touch: w[(dz * 2 + dy) * 5 + i] = voxel (x0 + i, y + dy,
// z + dz), i = 0 .. 4, zero (weight 0: not valid) outside the range.  ok / in: bit r * 5 + i = that voxel is valid / valid and inside.
struct MtRows { uint32_t w[20]; unsigned ok, in; int x0, y, zr; size_t v0; bool act, has_x, has_y, has_z; };

__device__ __forceinline__ void mt_load(const DfMeshArgs& a, size_t item, int lane, MtRows& r)
{
    const size_t plane = (size_t)a.X * a.Y;
    const size_t li = item * 64 + (size_t)lane;
    r.act = li < a.n4;
    r.v0 = r.act ? 4 * li : 0;
    r.zr = (int)(r.v0 / plane);
    const int rem = (int)(r.v0 - (size_t)r.zr * plane);
    r.y = rem / a.X; r.x0 = rem - r.y * a.X;
    r.has_x = r.act && r.x0 + 4 < a.X; r.has_y = r.act && r.y + 1 < a.Y; r.has_z = r.act && r.zr + 1 < a.nz;
    const uint32_t* p = a.vol + r.v0;
    const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const bool on = r.act && (!(q & 1) || r.has_y) && (!(q & 2) || r.has_z);
        const uint32_t* pq = p + ((q & 1) ? (size_t)a.X : 0) + ((q & 2) ? plane : 0);
        const uint4 c = on ? *reinterpret_cast<const uint4*>(pq) : zero4;
        r.w[q * 5 + 0] = c.x; r.w[q * 5 + 1] = c.y; r.w[q * 5 + 2] = c.z; r.w[q * 5 + 3] = c.w;
        r.w[q * 5 + 4] = on && r.has_x ? pq[4] : 0u;
    }
    r.ok = 0u; r.in = 0u;
#pragma unroll
    for (int j = 0; j < 20; ++j) {
        const bool ok = mt_valid(r.w[j]);
        if (ok) r.ok |= 1u << j;
        if (ok && h2f_bits(r.w[j]) < 0.f) r.in |= 1u << j;
    }
}

// bit 7 k + s: voxel k's edge to (dx, dy, dz), s = dx + 2 dy + 4 dz - 1, carries a vertex (both ends valid, exactly one inside)
__device__ __forceinline__ unsigned mt_edges(const MtRows& r)
{
    unsigned m = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int s = 0; s < 7; ++s) {
            const int d = s + 1, j = (d >> 1) * 5 + k + (d & 1);
            if ((r.ok >> k) & (r.ok >> j) & ((r.in >> k) ^ (r.in >> j)) & 1u) m |= 1u << (7 * k + s);
        }
    return m;
}

// cell k: all 8 corners valid -> true, and in8 bit (dx + 2 dy + 4 dz) = that corner is inside
__device__ __forceinline__ bool mt_cell(const MtRows& r, int k, unsigned& in8)
{
    bool all = true; in8 = 0u;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int j = (c >> 1) * 5 + k + (c & 1);
        all = all && ((r.ok >> j) & 1u);
        in8 |= ((r.in >> j) & 1u) << c;
    }
    return all;
}
__device__ __forceinline__ unsigned mt_case(unsigned in8, int t)
{
    const int v1 = 1 << DF_MT_PERM[t][0], v2 = v1 | (1 << DF_MT_PERM[t][1]);
    return (in8 & 1u) | (((in8 >> v1) & 1u) << 1) | (((in8 >> v2) & 1u) << 2) | (((in8 >> 7) & 1u) << 3);
}
__device__ __forceinline__ unsigned mt_cell_triangles(unsigned in8)
{
    unsigned n = 0u;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const unsigned c = (unsigned)__popc(mt_case(in8, t));               // inside corners: 0 1 2 3 4 -> triangles 0 1 2 1 0
        n += c == 2u ? 2u : (c & 1u);
    }
    return n;
}
__device__ __forceinline__ unsigned mt_lane_triangles(const MtRows& r)
{
    unsigned n = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) { unsigned in8; if (mt_cell(r, k, in8)) n += mt_cell_triangles(in8); }
    return n;
}

__device__ __forceinline__ unsigned mt_wave_sum(unsigned v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ unsigned mt_wave_excl(unsigned v, int lane)
{
    unsigned s = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const unsigned t = __shfl_up(s, d, 64); if (lane >= d) s += t; }
    return s - v;
}

// ---- count
template <int U>      // 16-byte loads in flight per lane
__global__ __launch_bounds__(256) void df_mesh_count_kernel(const DfMeshArgs a)
{
    typedef unsigned int df_mt_u4 __attribute__((ext_vector_type(4)));
    const df_mt_u4* base4 = reinterpret_cast<const df_mt_u4*>(a.vol);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t chunk = (size_t)256 * U;
    for (size_t c0 = (size_t)blockIdx.x * chunk; c0 < a.n4; c0 += (size_t)gridDim.x * chunk) {
        df_mt_u4 own[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t i = c0 + (size_t)u * 256 + threadIdx.x;
            own[u] = i < a.n4 ? __builtin_nontemporal_load(base4 + i) : df_mt_u4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool ownv = mt_valid(own[u].x) | mt_valid(own[u].y) | mt_valid(own[u].z) | mt_valid(own[u].w);
            if (!__any(ownv)) continue;                                     // wave-uniform: only the truncation shell goes on
            const size_t item = (c0 + (size_t)u * 256 + (size_t)wave * 64) >> 6;
            MtRows r;
            mt_load(a, item, lane, r);
            const unsigned nv = mt_wave_sum((unsigned)__popc(mt_edges(r)));
            const unsigned nt = mt_wave_sum(mt_lane_triangles(r));
            if (lane == 0) { a.vbase[item] = nv; a.tbase[item] = nt; }
        }
    }
}

__global__ void df_mesh_totals_kernel(const unsigned long long* vbase, const unsigned long long* tbase, size_t n_items, unsigned long long* counts)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) { counts[0] = vbase[n_items]; counts[1] = tbase[n_items]; }
}

// ---- vertices
__device__ __forceinline__ void mt_item_vertices(const DfMeshArgs& a, size_t item, int lane, unsigned long long base)
{
    MtRows r;
    mt_load(a, item, lane, r);
    const unsigned m = mt_edges(r);
    const unsigned long long first = base + mt_wave_excl((unsigned)__popc(m), lane);
    const unsigned long long lanes = __ballot(m != 0u);
    unsigned int q0 = 0u;
    if (lane == 0) q0 = atomicAdd(a.qcount, (unsigned int)__popcll(lanes));           // hands out table entries; orders no output
    q0 = __shfl(q0, 0, 64);
    const bool fits = (unsigned long long)q0 + (unsigned long long)__popcll(lanes) <= a.qcap;   // else: more vertices than capacity
    if (lane == 0) { DfMeshItemQ q; q.lanes = fits ? lanes : 0ull; q.first = q0; q.pad = 0u; a.itemq[item] = q; }
    if (!m) return;
    if (fits) a.qtab[q0 + (unsigned int)__popcll(lanes & lane_mask_lt())] = make_uint2((unsigned int)first, m);
    unsigned long long o = first;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int s = 0; s < 7; ++s) {
            if (!((m >> (7 * k + s)) & 1u)) continue;
            const int d = s + 1, j = (d >> 1) * 5 + k + (d & 1);
            const float F = fabsf(h2f_bits(r.w[k])), Fn = fabsf(h2f_bits(r.w[j]));
            f3 V = mk3(((float)(r.x0 + k) + 0.5f) * a.vsx, ((float)r.y + 0.5f) * a.vsy, ((float)(a.z_own0 + r.zr) + 0.5f) * a.vsz);
            const float d_inv = 1.f / (F + Fn);
            if (d & 1) { const float Vn = V.x + a.vsx; V.x = (V.x * Fn + Vn * F) * d_inv; }
            if (d & 2) { const float Vn = V.y + a.vsy; V.y = (V.y * Fn + Vn * F) * d_inv; }
            if (d & 4) { const float Vn = V.z + a.vsz; V.z = (V.z * Fn + Vn * F) * d_inv; }
            const f3 q = aff_mul(a.aff, V);
            if (o < a.vcap) a.verts[o] = make_float4(q.x, q.y, q.z, 0.f);
            ++o;
        }
}

// ---- triangles
// table record {first vertex, edge mask} of the lane-quad that starts at voxel `vlin` (range-linear); {0, 0}: it has no vertex
__device__ __forceinline__ uint2 mt_quad(const DfMeshArgs& a, size_t vlin)
{
    const DfMeshItemQ q = a.itemq[vlin >> 8];
    const int l = (int)((vlin >> 2) & 63);
    if (!((q.lanes >> l) & 1ull)) return make_uint2(0u, 0u);
    const unsigned long long e = (unsigned long long)q.first + (unsigned long long)__popcll(q.lanes & ((1ull << l) - 1ull));
    return e < a.qcap ? a.qtab[e] : make_uint2(0u, 0u);
}

__device__ __forceinline__ void mt_item_triangles(const DfMeshArgs& a, size_t item, int lane, unsigned long long base)
{
    MtRows r;
    mt_load(a, item, lane, r);
    const unsigned nt = mt_lane_triangles(r);
    unsigned long long o = base + mt_wave_excl(nt, lane);
    if (!nt) return;
    const size_t plane = (size_t)a.X * a.Y;
    uint2 Q[8];                                                            // [(dz * 2 + dy) * 2 + (0: own quad, 1: the next one in x)]
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const bool on = (!(q & 1) || r.has_x) && (!(q & 2) || r.has_y) && (!(q & 4) || r.has_z);
        Q[q] = on ? mt_quad(a, r.v0 + ((q & 1) ? 4 : 0) + ((q & 2) ? (size_t)a.X : 0) + ((q & 4) ? plane : 0)) : make_uint2(0u, 0u);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        unsigned in8;
        if (!mt_cell(r, k, in8)) continue;
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const unsigned long long e = c_df_mt.e[t * 16 + mt_case(in8, t)];
            const int n = (int)(e & 3ull);
            for (int tr = 0; tr < n; ++tr) {
                uint32_t idx[3];
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const unsigned code = (unsigned)(e >> (2 + 6 * (3 * tr + q))) & 63u;
                    const unsigned cc = code >> 3, s = code & 7u;
                    const int i = k + (int)(cc & 1u);                       // 0 .. 4: x position among the lane's voxels and the next quad's first
                    const int sel = (int)(cc >> 1) * 2 + (i >> 2);
                    uint2 rec = Q[0];
#pragma unroll
                    for (int c = 1; c < 8; ++c) if (sel == c) rec = Q[c];
                    idx[q] = rec.x + (uint32_t)__popc(rec.y & ((1u << (7 * (i & 3) + (int)s)) - 1u));
                }
                if (o < a.tcap) { a.tris[3 * o] = idx[0]; a.tris[3 * o + 1] = idx[1]; a.tris[3 * o + 2] = idx[2]; }
                ++o;
            }
        }
    }
}

// A wave looks at 64 consecutive items and works through those that have output (their scanned bases differ).
template <bool TRIANGLES>
__global__ __launch_bounds__(256) void df_mesh_emit_kernel(const DfMeshArgs a)
{
    const int lane = threadIdx.x & 63;
    const size_t item0 = ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    if (item0 >= a.n_items) return;
    const unsigned long long* b = TRIANGLES ? a.tbase : a.vbase;
    const size_t i = item0 + (size_t)lane;
    const unsigned long long b0 = i < a.n_items ? b[i] : 0ull, b1 = i < a.n_items ? b[i + 1] : 0ull;
    unsigned long long todo = __ballot(b1 > b0);
    while (todo) {                                                          // wave-uniform
        const int s = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1ull;
        const unsigned long long base = __shfl(b0, s, 64);
        if (TRIANGLES) mt_item_triangles(a, item0 + (size_t)s, lane, base);
        else mt_item_vertices(a, item0 + (size_t)s, lane, base);
    }
}

extern "C" int dfusion_extract_mesh(DfVolume v, const DfSlab* slab, const float aff[12], float* vertices, unsigned long long vertex_capacity,
                                    unsigned int* triangles, unsigned long long triangle_capacity, unsigned long long* counts, dfStream stream)
{
    if (!aff || !counts || !df_volume_valid(v)) return DF_E_INVALID;
    if ((vertex_capacity && !vertices) || (triangle_capacity && !triangles)) return DF_E_INVALID;
    DfSlab s = df_slab_or_full(v, slab);
    if (!df_slab_valid(v, s)) return DF_E_INVALID;
    const int z_end = min(s.z_own0 + s.z_own_n, v.dims[2] - 1);
    if (z_end > s.z_store0 + s.z_store_n - 1) return DF_E_INVALID;                              // plane z_end: the cells' +z corners, and owners itself
    hipStream_t st = (hipStream_t)stream;
    if (z_end < s.z_own0) { DF_HIP(hipMemsetAsync(counts, 0, 16, st)); return DF_OK; }
    DfMeshArgs a;
    memset(&a, 0, sizeof(a));
    a.X = v.dims[0]; a.Y = v.dims[1]; a.nz = z_end - s.z_own0 + 1; a.z_own0 = s.z_own0;
    const size_t plane = (size_t)a.X * a.Y;
    a.vol = (const uint32_t*)v.data + (size_t)(s.z_own0 - s.z_store0) * plane;
    a.vsx = v.voxel_size[0]; a.vsy = v.voxel_size[1]; a.vsz = v.voxel_size[2];
    a.aff = df_aff(aff);
    a.n4 = plane * (size_t)a.nz / 4;
    a.n_items = (a.n4 + 63) / 64;
    if (a.n_items + 1 > 0x7fffffffull) return DF_E_INVALID;
    const bool emit = vertex_capacity != 0 || triangle_capacity != 0;
    a.qcap = emit ? (vertex_capacity < a.n4 ? vertex_capacity : (unsigned long long)a.n4) : 0ull;
    if (a.qcap > 0xffffffffull) a.qcap = 0xffffffffull;                                         // (vertex indices are 32-bit)
    a.verts = (float4*)vertices; a.vcap = vertex_capacity; a.tris = triangles; a.tcap = triangle_capacity;
    // workspace: [counts / bases: vertices, triangles | item records | entry counter] (zeroed), the table, hipcub's temporary storage
    size_t scan_bytes = 0;
    DF_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (int)(a.n_items + 1), st));
    const size_t o_v = 0, o_t = o_v + (a.n_items + 1) * 8, o_q = (o_t + (a.n_items + 1) * 8 + 15) / 16 * 16;
    const size_t o_cnt = o_q + (emit ? a.n_items * sizeof(DfMeshItemQ) : 0), zero_bytes = o_cnt + 16;
    const size_t o_tab = zero_bytes, o_scan = (o_tab + (size_t)a.qcap * sizeof(uint2) + 255) / 256 * 256;
    DfScratchHold hold(st, o_scan + scan_bytes);                                                // held until the last launch is enqueued
    if (!hold.entry) return (int)hipErrorOutOfMemory;
    char* const ws = hold.mem;
    a.vbase = (unsigned long long*)(ws + o_v); a.tbase = (unsigned long long*)(ws + o_t);
    a.itemq = (DfMeshItemQ*)(ws + o_q); a.qcount = (unsigned int*)(ws + o_cnt); a.qtab = (uint2*)(ws + o_tab);
    DF_HIP(hipMemsetAsync(ws, 0, zero_bytes, st));
    const int U = 4;
    size_t blocks = (a.n4 + 256 * U - 1) / (256 * U);
    if (blocks > 256 * 32) blocks = 256 * 32;
    hipLaunchKernelGGL(df_mesh_count_kernel<U>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    DF_LAUNCH_CHECK();
    DF_HIP(hipcub::DeviceScan::ExclusiveSum(ws + o_scan, scan_bytes, a.vbase, a.vbase, (int)(a.n_items + 1), st));
    DF_HIP(hipcub::DeviceScan::ExclusiveSum(ws + o_scan, scan_bytes, a.tbase, a.tbase, (int)(a.n_items + 1), st));
    hipLaunchKernelGGL(df_mesh_totals_kernel, dim3(1), dim3(64), 0, st, a.vbase, a.tbase, a.n_items, counts);
    DF_LAUNCH_CHECK();
    if (!emit) return DF_OK;
    const unsigned eblocks = (unsigned)((a.n_items + 255) / 256);
    hipLaunchKernelGGL(df_mesh_emit_kernel<false>, dim3(eblocks), dim3(256), 0, st, a);         // every first-vertex record, then the triangles that read them
    DF_LAUNCH_CHECK();
    hipLaunchKernelGGL(df_mesh_emit_kernel<true>, dim3(eblocks), dim3(256), 0, st, a);
    DF_LAUNCH_CHECK();
    return DF_OK;
}
