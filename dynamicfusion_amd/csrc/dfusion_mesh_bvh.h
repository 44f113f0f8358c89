// dfusion_mesh_bvh.h -- what the two users of the linear BVH over an indexed triangle mesh share: dfusion_mesh_closest_points
// (dfusion_mesh_bvh.hip) and dfusion_mesh_ray_hits (dfusion_mesh_rays.hip).  The build stages -- bounds, codes, sort, tree, boxes; DESIGN
// section 28 -- exist ONCE, as kernels of dfusion_mesh_bvh.hip behind df_mbv_build; this header holds the argument block, the workspace
// layout and the order-preserving float keys the boxes are stored as; grids, the overlap test and the counting are the mesh kit's
// (dfusion_mesh_kit.h).  The tree lives in the caller's workspace and is rebuilt by every call: nothing here outlives the call that built it.
#pragma once
#include "dfusion_mesh_kit.h"

#define DF_MBV_NONE 0xffffffffu
#define DF_MBV_STACK 64                              // (dfusion_mesh_bvh.hip derives it: at most 62 internal nodes on a root-to-leaf path)
#define DF_MBV_LEFT_LEAF 1u
#define DF_MBV_RIGHT_LEAF 2u

struct DfMbvArgs {
    size_t V, T, Q;
    const float4* P; const uint32_t* tris; const float4* q; float max_d2;
    uint32_t* bounds;                                        // [8] keys: min x y z -, max x y z - of the eligible centroids
    unsigned long long *keys_in, *keys;                      // [T] as emitted, sorted
    uint32_t* split; uint8_t* flags;                         // [T] per internal node: children are split and split + 1; which of them are leaves
    uint32_t *par_i, *par_l;                                 // [T] the parent (an internal node) of an internal node / of a sorted leaf
    uint32_t *box_i, *box_l;                                 // [6 T] keys {min x y z, max x y z} of an internal node / of a sorted leaf
    unsigned long long* top;                                 // the largest winning d2: bits << 32 | ~q
    unsigned long long* counts;
    uint32_t* out_t; float4* out_p; float4* out_b;
};

// An order-preserving map of the finite and infinite floats onto uint32 (-0 below +0), and back.
__device__ __forceinline__ uint32_t mbv_key(float f) { const uint32_t b = __float_as_uint(f); return (b & 0x80000000u) ? ~b : b ^ 0x80000000u; }
__device__ __forceinline__ float mbv_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? k ^ 0x80000000u : ~k); }
__device__ __forceinline__ bool mbv_finite(float f) { return (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u; }

// The workspace, front to back (every array rounded up to 16 bytes): [keys as emitted 8 T] [sorted keys 8 T] [split 4 T] [flags T]
// [parents of internal nodes 4 T, of leaves 4 T] [boxes of internal nodes 24 T, of leaves 24 T] [bounds 32] [top 16]
// [hipcub's sort storage, 256-byte aligned]: 77 T + 48 bytes and that storage.
struct DfMbvLayout { size_t o_keys, o_split, o_flags, o_par_i, o_par_l, o_box_i, o_box_l, o_bounds, o_top, o_cub, cub_bytes, total; };

// The layout for T triangles (asks hipcub for its storage; nothing is launched).
DF_LOCAL int df_mbv_plan(size_t T, hipStream_t st, DfMbvLayout* l);

// Enqueues the build on `st` into `ws` (l.total bytes): a.V, T, P, tris and counts are the caller's (counts zeroed before); the
// workspace pointers of `a` are set here.  The bounds stage always runs and leaves counts [2] = E eligible and [3] skipped triangles;
// with `tree` the codes, the sort, the tree and the boxes follow, after which a.keys [E] are the sorted leaves, a.split / a.flags
// [E - 1] the internal nodes (node 0 the root) and a.box_i / a.box_l their boxes as keys, to be read from the NEXT launch on.
DF_LOCAL int df_mbv_build(DfMbvArgs& a, const DfMbvLayout& l, char* ws, bool tree, hipStream_t st);
