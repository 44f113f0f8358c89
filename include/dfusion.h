/*
 * dfusion.h -- C-ABI of the MI355X (gfx950) DynamicFusion hot path.
 *
 * This is the drop-in boundary.  The reference has no FFI: its seam is the link-time set of
 * free functions kfusion::device::* declared in the private header
 * /root/reference/kfusion/src/internal.hpp:104-115 and called from the public class
 * kfusion::cuda::TsdfVolume (kfusion/src/tsdf_volume.cpp).  Every entry point below names the
 * reference interface it replaces.  Plain C types only: raw device pointers, byte pitches,
 * row-major float arrays; no torch / OpenCV / HIP types in any signature (a stream is an opaque
 * void* holding a hipStream_t; NULL = the default stream).
 *
 * Conventions
 *   - every function returns 0 on success, otherwise a hipError_t value or a DF_E_* code;
 *     nothing prints, nothing calls exit() (the reference's cudaSafeCall prints and exit(0)s,
 *     kfusion/src/safe_call.hpp:13-27; the C++ wrapper maps non-zero to kfusion::cuda::error).
 *   - pointers named *_dev are DEVICE pointers; small parameter blocks (affines, intrinsics)
 *     are HOST pointers read before the call returns (the reference passes them by value).
 *   - images are pitched: row y starts at base + y * pitch, the pitch a byte count of the caller's choice
 *     (hipMallocPitch / cudaMallocPitch steps, row bands and column windows of larger images).  Every image
 *     argument returns DF_E_INVALID when its pitch is smaller than cols * bytes per pixel (u16 2, float4 16,
 *     BGRA 4; dfusion_transform_points: cols * stride * 4; dfusion_icp_estimate: each level's images).
 *   - an affine is 12 floats: R row-major [9] then t [3]  (device::Aff3f, internal.hpp:26-27,
 *     filled by device_cast, kfusion/src/precomp.hpp:19-28).
 *   - kernels are enqueued on `stream` and NOT synchronised (the reference's integrate ends in
 *     cudaDeviceSynchronize, tsdf_volume.cu:160; the C++ wrapper restores that behaviour).
 *   - no global state: any number of volumes and warp fields may be used concurrently, each from its own stream
 *     (the reference is not re-entrant: global texture ref tsdf_volume.cu:50, host globals
 *     warp_field.cpp:11-15).  ONE warp-field handle, though, is single-stream: its calls rewrite
 *     scratch it owns (the point queries' fallback list, the solver workspace, the cull's device
 *     scalars, the dists max-pyramid and the launch plan of the warped sweep), so calls on the same
 *     DfWarpField must be issued on one stream or serialised by the caller.  (The handle also owns one
 *     internal side stream, on which dfusion_integrate_warped makes look-ahead tables beside its sweep;
 *     the next call on the handle waits for it on the device -- invisible to the caller.)  dfusion_integrate keeps
 *     its pyramid and launch plan in a scratch buffer cached per (device, stream) -- calls on one
 *     stream are ordered, calls on different streams use different buffers; dfusion_release_scratch()
 *     frees them.  At most 8 buffers are kept per device (the least recently used idle one goes); a
 *     buffer is held for the whole of the call that uses it, so host threads may call on different
 *     streams concurrently (two threads on the SAME stream are serialised for the enqueue).
 *     Validation switches and measurement counters are per call / per handle (ABI 4).
 */
#ifndef DFUSION_H
#define DFUSION_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DFUSION_ABI_VERSION 7   /* 7: dfusion_warp_extend (additive); dfusion_raycast_min_pieces (the sharded cast's key merge as direct exchanges: all-to-all of row bands, local MIN, all-gather); 6: dfusion_cloud_to_depth; the planned warped sweep takes every node count (no LDS node table: DF_WARP_NO_LDS now only selects the plain gather kernel), a prepared plan is also voided by set_nodes / build_index / a second set_transforms; 5: dfusion_integrate_warped_prepare / _sweep (the frame's integrate in two calls, for cross-frame overlap), dfusion_raycast_sum_pieces (direct row-band merge), DF_WARP_STEADY_PREFETCH, dfusion_selftest_exact_forms takes TEN counters ([8], [9]: the f32-division form of the blend's first normalisation), DF_WARP_NO_CODES + dfusion_warp_coded_blocks (4-bit neighbour codes of modelled blocks); 4: no process-wide state left: dfusion_integrate_ex (validation flags + swept counter per call) replaces dfusion_debug_rigid / dfusion_debug_rigid_counters, dfusion_warp_debug_counters (per handle) replaces dfusion_debug_warp_counters; dfusion_warp_alive_blocks; dfusion_raycast_points_of_keys_rows; DF_WARP_NO_PREFETCH; 3: dfusion_raycast_points_of_keys (dfusion_raycast_shade's points nullable), dfusion_release_scratch, DF_INDEX_TABLES_ON_DEMAND, DF_WARP_*_BLOCK_MODEL flags; 2: sharded cast merges on one key (no vertex exchange), dfusion_debug_rigid_counters, selftest counts[6] */

typedef void *dfStream; /* hipStream_t */

/* device::TsdfVolume, kfusion/src/internal.hpp:29-49, field for field.
 * Voxel = ushort2 {half tsdf, u16 weight} (device.hpp:53-61); linear index
 * x + y*dims[0] + z*dims[0]*dims[1] (device.hpp:17-18).                                      */
typedef struct DfVolume {
    void *data;          /* DEVICE pointer to the first STORED plane (see DfSlab)            */
    int dims[3];         /* global voxel counts (x, y, z); dims[0] % 4 == 0                  */
    float voxel_size[3]; /* metres                                                            */
    float trunc_dist;    /* metres                                                            */
    int max_weight;
} DfVolume;

/* Z-slab view for multi-GPU sharding (no reference counterpart: the reference is single-GPU).
 * `data` holds planes [z_store0, z_store0+z_store_n) (own planes + halos); this shard integrates
 * and owns ray steps for planes [z_own0, z_own0+z_own_n).  NULL = the whole volume.           */
typedef struct DfSlab {
    int z_store0, z_store_n;
    int z_own0, z_own_n;
} DfSlab;

/* Opaque warp-field handle: device copy of the deformation nodes (WarpField::nodes_,
 * kfusion/include/kfusion/warp_field.hpp:35-40) plus the k-NN brick index that replaces the
 * nanoflann kd-tree (warp_field.cpp:275-282).                                                 */
typedef struct DfWarpField DfWarpField;

enum {
    DF_OK = 0,
    DF_E_INVALID = 100001,   /* bad argument (null pointer, dims, k not in {1..8}, M < k, ...) */
    DF_E_NO_INDEX = 100002,  /* dfusion_warp_build_index not called for this geometry / k       */
    DF_E_NO_DEVICE = 100003  /* no HIP device / kernel image not loadable                       */
};

/* flags for dfusion_integrate_warped */
#define DF_WARP_NO_CULL 1u   /* disable the (result-identical) conservative brick culling     */
#define DF_WARP_NO_TABLE 2u  /* ignore the per-voxel k-NN table even if built (re-rank per frame) */
#define DF_WARP_NO_WEIGHT_TABLE 4u /* ignore the per-voxel weight table (recompute exp per frame)   */
#define DF_WARP_NO_LDS 8u    /* the plain gather kernel: node transforms from global memory per neighbour, no launch
                                plan, no verdict pass, no codes, no prepare / sweep split; validation switch.  (Until
                                round 6 this was also the path of node sets whose table exceeds the 160 KiB LDS,
                                M > 5120; the planned sweep now needs no LDS node table and takes every node count.) */
#define DF_WARP_NO_PIPELINE 16u /* batched instead of software-pipelined table loads; validation switch */
#define DF_WARP_NO_ZERO_SKIP 32u /* also sweep tiles whose blend weights are all so small that the reference's
                                 normalisation divides by zero (they cannot update); validation switch  */
#define DF_WARP_NO_DEPTH_PYRAMID 64u /* cull against the image-wide maximum of dists only, not against the maximum
                                 over the pixels a tile can project to; validation switch                  */
#define DF_WARP_NO_BLOCK_MODEL 128u /* launch plan from the ball test alone: do not build / use the per-block blend models
                                 (bounds of each 8x8x8 block's blend weights, made from the weight table for the blocks
                                 a sweep finds alive, from the second sweep over a table on; 10 bytes x 16 per block);
                                 validation switch                                                              */
#define DF_WARP_BLOCK_MODEL_NOW 256u /* make block models from the FIRST sweep over a new weight table on (default: the
                                 second, so that a node set that changes every frame never pays for them)       */
#define DF_WARP_NO_PREFETCH 512u /* everything on the caller's stream, in order: no look-ahead builds on the handle's side stream
                                 (by default the tables / blend models of blocks NEAR the frame's alive set -- what a moving camera
                                 or a changing warp brings in over the next few frames -- are made beside the sweep, on a stream the
                                 handle owns, so that a block is usually built before it is first swept); validation switch     */
#define DF_WARP_NO_CODES 2048u /* the sweep reads the 16-byte neighbour-index record of every voxel and gathers its neighbours' transforms
                                 * from global memory, instead of the 4-bit codes into the per-wave copies of the 4 x 4 x 4 sub-block unions
                                 * (k = 8; every block the model pass has visited); validation / A/B switch (ABI 5)                      */
#define DF_WARP_NO_SUB_VERDICT 4096u /* the launch plan keeps or drops whole 8 x 8 x 8 blocks: no second verdict per 4 x 4 x 4 sub-block (from blend
                                 * models of the sub-blocks, made beside the block models at k = 8), by which the sweep skips a half layer
                                 * (8 x 8 x 4 voxels) none of whose four sub-blocks can update; validation / A/B switch.  Implied by
                                 * DF_WARP_NO_BLOCK_MODEL and DF_WARP_NO_CULL.                                                        */
#define DF_WARP_STEADY_PREFETCH 1024u /* keep the look-ahead side stream on in EVERY frame.  By default a handle whose last plan-kernel report
                                 * listed nothing to build switches it off until the next probe (every 8th sweep); that report is read from
                                 * pinned host memory WITHOUT a synchronisation, so which frame switches depends on host / GPU timing --
                                 * never any result, but swept-voxel counters and frame times of a run.  For tests and measurements that
                                 * compare such counters between runs (ABI 5).                                                         */
/* flags for dfusion_warp_build_index */
#define DF_INDEX_VOXEL_TABLE 1u /* also cache the exact k-NN of EVERY voxel of the slab in HBM:
                                   k * 2 bytes per voxel (2 GiB at 512^3, k = 8) -- the per-frame
                                   sweep then streams it instead of re-running the k-NN search   */
#define DF_INDEX_WEIGHT_TABLE 2u /* implies the above, and also caches the k blend weights
                                   exp(-d^2/(2 dg_w^2)) of every voxel (k * 4 bytes per voxel, 4 GiB
                                   at 512^3, k = 8): they too depend only on canonical geometry     */
#define DF_INDEX_TABLES_ON_DEMAND 4u /* with DF_INDEX_WEIGHT_TABLE: allocate the tables but fill them 8x8x8 block by
                                   block, when a warped integrate's launch plan first finds a block alive (a frame
                                   sweeps a third of the volume; the build is the cost of a node-set change).
                                   Sweeps that take no verdicts (DF_WARP_NO_CULL, DF_WARP_NO_PIPELINE, ...) build what
                                   is missing first.  Results are identical either way                          */

int dfusion_abi_version(void);
const char *dfusion_error_string(int err);

/* ---- volume -------------------------------------------------------------------------------
 * device::clear_volume (internal.hpp:105; tsdf_volume.cu:15-41): every stored voxel <- 0.     */
int dfusion_clear(DfVolume v, const DfSlab *slab, dfStream stream);

/* device::compute_dists (internal.hpp:124; kfusion/src/cuda/imgproc.cu:259-294): depth mm (u16)
 * -> ray length in metres as IEEE-half bits.  intr = {fx, fy, cx, cy}.                         */
int dfusion_compute_dists(const uint16_t *depth_dev, size_t depth_pitch, uint16_t *dists_dev, size_t dists_pitch,
                          int cols, int rows, const float intr[4], dfStream stream);

/* device::project_and_remove / device::project (internal.hpp:107-109; project_kernel tsdf_volume.cu:113-139, launched
 * by :163-192) fused with the per-point arithmetic of TsdfVolume::psdf (tsdf_volume.cpp:266-292).
 * points_dev: n float4 (camera frame), updated in place: NaN points untouched; points projecting outside the image ->
 * (qnan, qnan, qnan, 0); otherwise (coo.x*Dp, coo.y*Dp, Dp, 0) with Dp = dists(coo) and the dists pixel "removed" (<- 0).
 * The reference samples and zeroes ONE image concurrently (a second point on the same pixel may see 0 or the old
 * value); here samples come from dists_in and the zeros go to dists_out (nullable; must not alias dists_in; the caller
 * seeds it with a copy of dists_in).  ro_dev (nullable): n floats, psdf's return value
 * (K^-1 * new_point)[2] - old_point.z, NaN for NaN / outside points.  n_inside_dev (nullable) is INCREMENTED by the
 * number of points that landed inside the image.                                                                  */
int dfusion_project_and_remove(const uint16_t *dists_in_dev, size_t in_pitch, uint16_t *dists_out_dev, size_t out_pitch,
                               int cols, int rows, float *points_dev, unsigned long long n, const float proj[4],
                               float *ro_dev, unsigned long long *n_inside_dev, dfStream stream);

/* device::integrate (internal.hpp:106; tsdf_volume.cu:51-112,141-161): rigid projective TSDF
 * update.  proj = {fx, fy, cx, cy} (device::Projector).  n_updated_dev (nullable) is
 * INCREMENTED by the number of voxels whose update branch (tsdf_volume.cu:91) was taken.
 * Scratch: a launch plan, the chunk starts of every column patch (16 bytes per column and 32-plane chunk: 64 MiB at 512^3, 512 MiB at
 * 1024^3), the plan's bins and a max-pyramid of `dists`, + 25 % growth headroom -- about 84 MB at 512^3, 0.65 GB at 1024^3 -- in a
 * buffer the library keeps per (device, stream) and grows on demand.  It is KEPT until dfusion_release_scratch(); at most 8
 * (device, stream) pairs are cached, the least recently used one is evicted (the runtime's stream-ordered allocator was tried and
 * gave wrong plans in processes that also hipMalloc / hipFree between the calls).  Limit: (columns / 64, rounded up to whole patches) x
 * (32-plane chunks of the slab) < 2^30, i.e. any volume that fits the device.                                                   */
int dfusion_integrate(const uint16_t *dists_dev, size_t dists_pitch, int cols, int rows, DfVolume v,
                      const DfSlab *slab, const float vol2cam[12], const float proj[4],
                      unsigned long long *n_updated_dev, dfStream stream);

/* The same with the validation switches and the measurement counter of THIS call (no reference counterpart; tests assert the
 * volumes are identical with and without each switch).  flags = 0: everything on.  n_swept_dev (nullable, device, 8 bytes) is
 * INCREMENTED by the number of voxels the sweep put through the projective sample (tsdf_volume.cu:77-93) -- the voxels of the
 * launch plan's alive sub-chunks; beside n_updated_dev this gives swept / updated, the sweep's over-work.                        */
#define DF_RIGID_NO_DEPTH_CULL 1u  /* no behind-the-surface test (a conservative skip of voxels more than trunc_dist behind every
                                      depth value they can be compared with; per-frame max-pyramid of dists)                     */
#define DF_RIGID_NO_SHORT_FORMS 2u /* the generic correctly rounded divisions / square root everywhere                           */
#define DF_RIGID_KEEP_ALL 4u       /* the launch plan keeps every sub-chunk (no frustum test either): every voxel goes through the
                                      reference's own tests                                                                       */
#define DF_RIGID_NO_SAT 8u         /* no saturated-sample shortcuts (batches of voxels all farther than trunc_dist from the surface
                                      skip the exact square root and, onto stored 1.0 / cleared voxels, the fuse division)        */
#define DF_RIGID_POISON_SCRATCH 16u /* fill the call's scratch (launch plan, chunk starts, pyramid) with 0xFF bytes first: the buffer is
                                      kept between calls, and a read of plan data THIS call did not write would otherwise see the
                                      previous call's valid-looking values                                                        */
int dfusion_integrate_ex(const uint16_t *dists_dev, size_t dists_pitch, int cols, int rows, DfVolume v,
                         const DfSlab *slab, const float vol2cam[12], const float proj[4], unsigned flags,
                         unsigned long long *n_updated_dev, unsigned long long *n_swept_dev, dfStream stream);

/* Frees the scratch buffers dfusion_integrate keeps per (device, stream), after a device synchronise (a cached stream handle may no
 * longer exist); the caller's current device is restored.  Optional; for hosts that tear devices down or count allocations.       */
int dfusion_release_scratch(void);

/* device::raycast, Points variant (internal.hpp:113-114; tsdf_volume.cu:340-405,459-474).
 * points/normals: float4 per pixel, byte pitches, misses = all-NaN.  reproj = {1/fx, 1/fy, cx,
 * cy} (device::Reprojector, precomp.cpp:55).  keys_dev (nullable, cols*rows uint32): per-pixel
 * first-event key (step<<1 | hit) on steps this slab owns, 0xffffffff = none (sharded merge).  */
int dfusion_raycast_points(DfVolume v, const DfSlab *slab, const float cam2vol[12], const float Rinv[9],
                           const float reproj[4], float *points_dev, size_t points_pitch, float *normals_dev,
                           size_t normals_pitch, int cols, int rows, float step_factor, float delta_factor,
                           uint32_t *keys_dev, dfStream stream);

/* device::raycast, Depth variant (internal.hpp:110-111; tsdf_volume.cu:272-338,441-456).       */
int dfusion_raycast_depth(DfVolume v, const DfSlab *slab, const float cam2vol[12], const float Rinv[9],
                          const float reproj[4], uint16_t *depth_dev, size_t depth_pitch, float *normals_dev,
                          size_t normals_pitch, int cols, int rows, float step_factor, float delta_factor,
                          dfStream stream);

/* Z-slab (multi-GPU) cast in two stages; no reference counterpart.  The zero-crossing refinement
 * Ts = t - step*Ft/(Ftdt-Ft) (tsdf_volume.cu:389) may EXTRAPOLATE arbitrarily far along the ray, so the
 * vertex of a hit can lie in another GPU's slab: stage 1 finds, on the steps this slab owns, the first
 * event and (for hits) Ts; the host MIN-merges the 64-bit keys over the ranks -- ONE collective, which
 * delivers the first event along every ray, its owner and its Ts; stage 2 lets the slab that owns the
 * vertex' nearest plane compute the normal (needs a 2-plane halo) and write the final camera-frame
 * point/normal, with vertex = origin + direction * Ts recomputed from the pixel exactly as the unsharded
 * cast computes it (:390).  Pixels a slab does not resolve are written as all-zero BITS (the slab owning
 * plane 0 writes the NaN fill of misses), so integer-summing the slabs' outputs equals the unsharded cast.
 *
 * key layout (a non-negative int64, so ncclMin on ncclInt64 orders it):
 *   bit 63 = 0 | bits 62..40 step index k | bit 39 kind (1 = hit, 0 = back-face break) | bits 38..32 rank_tag | bits 31..0 Ts (f32 bits)
 * DF_RC_KEY_NONE (no event on this slab's steps) is larger than every event key.  dfusion_raycast_march returns DF_E_INVALID when
 * (volume diagonal) / (trunc_dist * step_factor) could reach 2^23 steps -- the index would not fit its field.                   */
#define DF_RC_KEY_NONE 0x7fffffffffffffffull
#define DF_RC_KEY_MAX_RANK 127u
int dfusion_raycast_march(DfVolume v, const DfSlab *slab, const float cam2vol[12], const float reproj[4], int cols,
                          int rows, float step_factor, unsigned int rank_tag, unsigned long long *keys64_dev,
                          dfStream stream);
int dfusion_raycast_shade(DfVolume v, const DfSlab *slab, const float cam2vol[12], const float Rinv[9],
                          const float reproj[4], const unsigned long long *merged_keys64_dev,
                          float *points_dev, size_t points_pitch, float *normals_dev, size_t normals_pitch, int cols,
                          int rows, float delta_factor, dfStream stream);
/* Stage 3, on the rank that wants the image: the camera-frame POINTS from the merged keys and the summed normals -- they need no
 * exchange (the vertex is origin + direction * Ts, and a hit stands iff the owner's normal is not the NaN fill: 4th component 0), so
 * dfusion_raycast_shade may be given points_dev = NULL and only the normals cross GPUs.  Equals the points image of the unsharded
 * cast bit for bit.  Needs no volume.                                                                                            */
int dfusion_raycast_points_of_keys(const float cam2vol[12], const float Rinv[9], const float reproj[4],
                                   const unsigned long long *merged_keys64_dev, const float *normals_dev, size_t normals_pitch,
                                   float *points_dev, size_t points_pitch, int cols, int rows, dfStream stream);
/* The same for a BAND of pixel rows [row0, row0 + rows) of a cols x image_rows image: merged_keys64_dev is the whole image's (every
 * rank holds it after the merge), normals_dev / points_dev point at the band's first row.  For the row-banded merge: the normals are
 * reduce-scattered by pixel rows, every rank finishes its own band, and no rank receives the whole image (ABI 4).              */
int dfusion_raycast_points_of_keys_rows(const float cam2vol[12], const float Rinv[9], const float reproj[4],
                                        const unsigned long long *merged_keys64_dev, const float *normals_dev, size_t normals_pitch,
                                        float *points_dev, size_t points_pitch, int cols, int image_rows, int row0, int rows,
                                        dfStream stream);

/* The receiving end of the DIRECT form of the sharded cast's second collective (ABI 5): rank r gets, from every rank p, p's piece of r's row
 * band of the normals image (fixed-size pieces: one all-to-all, no counts; every pixel's normal is non-zero in exactly one piece) and adds
 * them: out[i] = sum over p < n_pieces of pieces[p * n_words + i], 32-bit integer adds on the bit patterns (all summands but one are zero, so
 * the sum IS the owner's bits -- the same arithmetic a reduce_scatter(SUM) on the int32 view performs).  n_words: 32-bit words per piece.   */
int dfusion_raycast_sum_pieces(const uint32_t *pieces_dev, int n_pieces, unsigned long long n_words, uint32_t *out_dev, dfStream stream);

/* The local step of the DIRECT form of the sharded cast's FIRST collective (ABI 7).  ncclAllReduce(MIN) of the key image walks a ring of
 * 2 (N - 1) sequential steps; xGMI links every pair of GPUs of a node directly, so the same result takes two exchanges of ONE step each:
 * every rank sends rank r its copy of r's band of pixel rows (one all-to-all of fixed-size pieces, as for the normals), r takes the per-key
 * minimum of the N pieces -- this call -- and one all-gather hands every rank the merged image.  out[i] = min over p < n_pieces of
 * pieces[p * n_keys + i]; keys are the non-negative int64 merge keys above (DF_RC_KEY_NONE in padding rows).  n_keys even unless
 * n_pieces == 1; pieces_dev / out_dev 16-byte aligned.                                                                                */
int dfusion_raycast_min_pieces(const unsigned long long *pieces_dev, int n_pieces, unsigned long long n_keys, unsigned long long *out_dev, dfStream stream);

/* ---- surface extraction -------------------------------------------------------
 * device::extractCloud (internal.hpp:142; tsdf_volume.cu:511-710,798-817): zero crossings between every voxel and its
 * +x/+y/+z neighbour, linearly interpolated, transformed by aff (= volume pose).  points_dev: float4 x capacity;
 * *count_dev (device, zero it first) is INCREMENTED by the number of crossings found -- the number written is
 * min(count, capacity); output order is unspecified (as in the reference).  A slab needs one halo plane above.  */
int dfusion_extract_cloud(DfVolume v, const DfSlab *slab, const float aff[12], float *points_dev,
                          unsigned long long capacity, unsigned long long *count_dev, dfStream stream);
/* device::extractNormals (internal.hpp:143; tsdf_volume.cu:714-795,819-831): TSDF gradient at each extracted point. */
int dfusion_extract_normals(DfVolume v, const DfSlab *slab, const float aff[12], const float Rinv[9],
                            const float *points_dev, unsigned long long n, float gradient_delta_factor,
                            float *normals_dev, dfStream stream);

/* A triangle mesh of the same surface (no reference counterpart; additive, ABI 7): marching tetrahedra on the Kuhn subdivision of
 * every voxel cell -- no ambiguous cases, consistent across cell faces, so the mesh is closed wherever the cells around the surface
 * are meshed.  DESIGN.md states the rule in full; tests/mesh_ref.py restates it in numpy and the output equals it bit for bit.
 *   - a voxel is valid by the extractor's rule (weight != 0, tsdf != 1), inside iff its tsdf < 0 (+0 and -0 are outside), and sits
 *     at ((x + .5) vsx, (y + .5) vsy, (z + .5) vsz);
 *   - voxel p owns the 7 edges p -> p + d, d in {0,1}^3 \ 0, slot s = dx + 2 dy + 4 dz - 1 (axis edges 0, 1, 3; face diagonals
 *     2, 4, 5; the body diagonal 6); an edge carries a vertex iff both ends are valid and exactly one is inside: with F, Fn the
 *     absolute tsdf of p and p + d and d_inv = 1.f / (F + Fn), every coordinate c with d_c = 1 becomes (V_c Fn + (V_c + vs_c) F)
 *     d_inv; then aff.  On an axis edge this is dfusion_extract_cloud's point, bit for bit.  vertices_dev: float4 (x, y, z, 0)
 *     in ascending (linear voxel index of the owner, slot);
 *   - a cell (corners p + {0,1}^3) is meshed iff all 8 corners are valid; its 6 tetrahedra (axis permutations xyz, xzy, yxz, yzx,
 *     zxy, zyx; corners p, p + e_a, p + e_a + e_b, p + (1,1,1)) give 0, 1 or 2 triangles each, turned so that the normal
 *     (p1 - p0) x (p2 - p0) points from inside to outside.  triangles_dev: 3 uint32 vertex indices each, in ascending (linear cell
 *     index, tetrahedron, triangle).  Triangles with coincident vertices (a corner's tsdf is exactly 0) are kept.
 * With a slab: cells in planes [z_own0, z_end), z_end = min(z_own0 + z_own_n, dims[2] - 1), owners in planes [z_own0, z_end]
 * restricted to edges that end in a plane <= z_end; plane z_end must be stored (one halo plane above, as for
 * dfusion_extract_cloud).  A slab's mesh is complete on its own; neighbouring slabs repeat the vertices of the shared plane.
 * counts_dev[0], [1] (device) are WRITTEN (not incremented): the number of vertices and of triangles the rule yields.  Nothing is
 * written past either capacity; if a count exceeds its capacity the contents of BOTH arrays are unspecified (size the buffers
 * and call again).  Both capacities 0 (arrays may be NULL): counts only, one pass over the volume.  Workspace: 32 bytes per 256
 * voxels + 8 bytes per vertex of capacity, from the per-(device, stream) scratch of dfusion_integrate (dfusion_release_scratch).
 * Vertex indices are 32-bit: meshes with more than 2^32 - 1 vertices are out of scope.  DF_E_INVALID for what
 * dfusion_extract_cloud refuses, and for a NULL array with a non-zero capacity.                                                  */
int dfusion_extract_mesh(DfVolume v, const DfSlab *slab, const float aff[12], float *vertices_dev,
                         unsigned long long vertex_capacity, unsigned int *triangles_dev,
                         unsigned long long triangle_capacity, unsigned long long *counts_dev, dfStream stream);

/* Connected components of an indexed triangle mesh, and the mesh without its small pieces (no reference counterpart; additive, ABI 7).
 * DESIGN.md section 22 has the kernels; tests/mesh_components_ref.py restates the rule in numpy and every output equals it.
 * Inputs: T triangles of three uint32 indices and a vertex count V.  Positions play no part: coincident vertices do not connect, only
 * shared indices do.
 *   - triangle t is VALID iff all three indices are < V (tested before anything is indexed); an invalid triangle connects nothing and
 *     is never kept;
 *   - the graph has the vertices 0 .. V-1 and an edge between any two different indices of a valid triangle ((a, a, b) is valid and
 *     connects a and b; (a, a, a) connects nothing and is a triangle of a's component);
 *   - vertex_label[v] = the smallest vertex index in v's component; a vertex used by no valid triangle labels itself;
 *   - triangle_count[r] = the number of valid triangles whose vertices carry label r, 0 for every r that is not a label (all V
 *     entries are written);
 *   - counts[4] (u64, WRITTEN, not incremented): [0] components holding at least one triangle, [1] vertices used by no valid triangle,
 *     [2] invalid triangles, [3] the triangle count of the largest component.
 * dfusion_mesh_filter, given the mesh and those two arrays: a triangle is KEPT iff it is valid, triangle_count[label] >= min_triangles
 * (inclusive) and -- with keep_largest != 0 -- its label is that of the component with the most triangles, an exact tie going to the
 * smaller label.  A vertex is kept iff a kept triangle uses it.  Kept triangles and kept vertices keep their relative order (stable
 * compaction); triangles_out_dev holds the kept triangles with the NEW indices; vertex_src_dev[i] = the old index of new vertex i,
 * the gather list for any per-vertex attribute (dfusion_gather_rows); vertex_map_dev[v] (nullable, V entries) = the new index of
 * old vertex v, or 0xffffffff.  counts_dev[0], [1] are WRITTEN: kept vertices and kept triangles, always the full numbers.  Nothing is
 * written past a capacity; if a count exceeds its capacity the contents of the output arrays are unspecified (dfusion_extract_mesh's
 * contract).  Both capacities 0: counts only (vertex_map_dev is not written either).
 * T == 0 or V == 0 is valid input, to which the rule applies as it stands: no component, nothing kept, every vertex unused (T == 0),
 * every triangle invalid (V == 0).  Arrays of length 0 may be NULL.
 * DF_E_INVALID: V or T > 2^32 - 1 (indices and triangle counts are 32-bit), NULL where not nullable, a NULL output array with a non-zero
 * capacity.  Without a device DF_E_NO_DEVICE.  No device-to-host copy and no synchronisation; every launch covers T and V with 64-bit
 * indices.  The union is a lock-free union-find in which a root is only ever linked under a smaller index: vertex_label_dev itself is
 * the forest, so a label is final only when the call's work on the stream is done.  Workspace, from the per-(device, stream) scratch of
 * dfusion_extract_mesh (dfusion_release_scratch): components V bytes (+ 4 V when triangle_count_dev is NULL and counts_dev is not;
 * none when both are NULL), filter 4 (T + 1) + 4 (V + 1) + 16 bytes and hipcub's scan storage.  Integer atomics only: no output depends
 * on scheduling.                                                                                                                      */
int dfusion_mesh_components(const unsigned int *triangles_dev, unsigned long long n_triangles,
                            unsigned long long n_vertices, unsigned int *vertex_label_dev,
                            unsigned int *triangle_count_dev /* nullable */,
                            unsigned long long *counts_dev /* [4], nullable */, dfStream stream);
int dfusion_mesh_filter(const unsigned int *triangles_dev, unsigned long long n_triangles,
                        unsigned long long n_vertices, const unsigned int *vertex_label_dev,
                        const unsigned int *triangle_count_dev, unsigned long long min_triangles,
                        int keep_largest, unsigned int *triangles_out_dev,
                        unsigned long long triangle_capacity, unsigned int *vertex_src_dev,
                        unsigned long long vertex_capacity, unsigned int *vertex_map_dev /* nullable */,
                        unsigned long long *counts_dev /* [2] */, dfStream stream);
/* dst row i = src row index_dev[i] for i < n, rows of row_bytes = 4, 12 or 16 bytes (anything else: DF_E_INVALID), both arrays 4-byte
 * aligned and not overlapping; the indices are not checked against the source's length.  n == 0: nothing (the arrays may be NULL).  */
int dfusion_gather_rows(const void *src_dev, unsigned int row_bytes /* 4, 12 or 16 */,
                        const unsigned int *index_dev, unsigned long long n, void *dst_dev,
                        dfStream stream);

/* A triangle mesh simplified by vertex clustering (no reference counterpart; additive, ABI 7).  DESIGN.md section 23 has the kernels;
 * tests/mesh_simplify_ref.py restates the rule in numpy and every output equals it bit for bit.
 * Inputs: V vertices of four floats (x, y, z, w), T triangles of three uint32 indices, a cell size `cell` (f32, finite, > 0), flags.
 *   CELL      per axis a, t_a = p_a / cell (IEEE f32 division).  A vertex is CLUSTERABLE iff |t_a| < 2^30 on all three axes (NaN and
 *             inf fail); its cell is c_a = (int)floorf(t_a) -- the cell rule of dfusion_warp_extend.  A vertex at k * cell opens cell k;
 *             +0 and -0 share cell 0.
 *   VALID     a triangle is valid iff all three indices are < V (tested before anything is indexed) and all three vertices are
 *             clusterable; an invalid triangle connects nothing and is never kept.  A vertex is a MEMBER iff a valid triangle uses it.
 *   CLUSTER   the members of one cell: n its member count, src its smallest member index, and per axis S_a = the sum over its members
 *             of q_a = (uint32)(f_a * 16777216.f), truncated, with f_a = t_a - floorf(t_a) (IEEE f32 subtraction; exact for t_a >= 0,
 *             rounded for some t_a < 0, where a tiny negative t_a gives f_a = 1 and q_a = 2^24), as an unsigned 64-bit sum.
 *   TRIANGLE  every valid triangle's indices are mapped to clusters.  It is COLLAPSED (dropped) unless the three clusters are pairwise
 *             different.  The others are grouped by their unordered cluster triple; in a group, P are the triangles that are an even
 *             permutation of the triple taken in ascending src, N the odd ones.  |P| == |N|: the group is a FIN and all of it is
 *             dropped -- two faces of one surface folded onto each other enclose nothing, and dropping only one of them would leave
 *             the surface open.  Otherwise the lowest-index triangle of the larger side is kept and the group's others are
 *             DUPLICATES.  With DF_SIMPLIFY_KEEP_DUPLICATES every non-collapsed triangle is kept and nothing is grouped.  Kept
 *             triangles come in their original order, their indices in their original rotation.
 *   VERTICES  one output vertex per cluster that a kept triangle uses, in ascending src.  vertex_src_dev[j] is that src (the gather
 *             list for any per-vertex attribute, dfusion_gather_rows); vertex_map_dev[v] is the new index of member v's cluster,
 *             0xffffffff for a non-member and for a cluster no kept triangle uses.
 *   POSITION  in f64 without contraction: m_a = (double)S_a / (double)n, pos_a = (float)(((double)c_a + m_a * 2^-24) * (double)cell),
 *             w = 0 -- the members' mean inside the cell, independent of the order of the sums.  With DF_SIMPLIFY_KEEP_FIRST the
 *             output vertex is the 16 bytes of vertex src as they are.
 *   counts_dev[8] (u64, WRITTEN, always the full numbers): [0] output vertices, [1] output triangles, [2] invalid, [3] collapsed,
 *             [4] fin and [5] duplicate triangles ([1] .. [5] add up to T), [6] clusters, [7] the unclusterable vertices among those
 *             that a triangle with all three indices < V uses.
 * Nothing is written past a capacity; if a count exceeds its capacity the contents of the output arrays are unspecified
 * (dfusion_mesh_filter's contract).  Both capacities 0: counts only (vertex_map_dev is not written either).  T == 0 or V == 0 is valid
 * input: nothing is kept, and with V == 0 every triangle is invalid.  Arrays of length 0 may be NULL.
 * DF_E_INVALID: V or T > 2^32 - 1, a NULL input or output array with a non-zero size or capacity, counts_dev NULL, cell not finite
 * or <= 0, a flag bit other than the two below, an output array (counts_dev included) that overlaps vertices_dev or triangles_dev.
 * Without a device DF_E_NO_DEVICE.  No device-to-host copy, no synchronisation, no floating-point atomics; every launch covers T and V
 * with 64-bit indices.  Workspace, from the per-(device, stream) scratch of dfusion_extract_mesh (dfusion_release_scratch): 53 V + 4 T
 * bytes, + 32 T for the groups unless DF_SIMPLIFY_KEEP_DUPLICATES is set, and hipcub's scan storage.                                    */
#define DF_SIMPLIFY_KEEP_FIRST 1u
#define DF_SIMPLIFY_KEEP_DUPLICATES 2u
int dfusion_mesh_simplify(const float *vertices_dev, unsigned long long n_vertices,
                          const unsigned int *triangles_dev, unsigned long long n_triangles,
                          float cell, unsigned int flags,
                          float *vertices_out_dev, unsigned long long vertex_capacity,
                          unsigned int *triangles_out_dev, unsigned long long triangle_capacity,
                          unsigned int *vertex_src_dev /* nullable, vertex_capacity */,
                          unsigned int *vertex_map_dev /* nullable, n_vertices */,
                          unsigned long long *counts_dev /* [8] */, dfStream stream);

/* The vertex adjacency of an indexed triangle mesh, with its edge statistics (no reference counterpart; additive, ABI 7).  DESIGN.md
 * section 24 has the kernels; tests/mesh_smooth_ref.py restates the rule in numpy and every output equals it bit for bit.
 * Inputs: T triangles of three uint32 indices over V vertices (the positions take no part).
 *   VALID       a triangle is valid iff its three indices are < V (tested before anything is indexed); an invalid one contributes
 *               nothing.  A valid triangle with two equal indices is DEGENERATE; it still contributes the pairs whose ends differ.
 *   HALF-EDGES  of a valid triangle (a, b, c): a -> b, b -> c, c -> a, leaving out those with equal ends.
 *   NEIGHBOUR   u is a neighbour of v iff a half-edge u -> v or v -> u exists.
 *   CSR         row v of neighbours_dev, [row_start_dev[v], row_start_dev[v + 1]), holds v's neighbours, each once, in ascending
 *               index; row_start_dev[0] = 0, the difference of two consecutive entries is v's degree, row_start_dev[V] the total.
 *   EDGE        for an undirected edge {lo < hi}, f = the number of half-edges lo -> hi and b = the number hi -> lo.  INTERIOR iff
 *               f == 1 and b == 1, BOUNDARY iff f + b == 1, everything else IRREGULAR: an edge used three or more times, and an
 *               edge used twice in the same direction (two faces that do not agree on the surface's side).
 *   vertex_class_dev[v] (one byte)  0 = no neighbour; 3 = an irregular edge ends at v; 2 = otherwise, a boundary edge ends at v;
 *               1 = otherwise.
 *   counts_dev[8] (u64, WRITTEN, always the full numbers): [0] CSR entries (= 2 E), [1] undirected edges E, [2] boundary edges,
 *               [3] irregular edges, [4] vertices with a neighbour, [5] invalid triangles, [6] degenerate triangles, [7] vertices of
 *               class 2 or 3.  For a mesh without degenerate triangles the Euler characteristic is [4] - [1] + (T - [5]).
 * Nothing is written past neighbour_capacity; if [0] exceeds it the contents of neighbours_dev are unspecified, row_start_dev and
 * vertex_class_dev are complete all the same.  Capacity 0 is valid (counts, rows and classes only); 6 T entries always suffice.
 * row_start_dev [V + 1] and vertex_class_dev [V] may be NULL.  T == 0 or V == 0 is valid input.  Arrays of length 0 may be NULL.
 * DF_E_INVALID: V > 2^32 - 1, 6 T > 2^32 - 1 (row offsets are 32-bit), triangles_dev NULL with T > 0, neighbours_dev NULL with a
 * capacity > 0, counts_dev NULL, an output array (counts_dev included) that overlaps triangles_dev.  Without a device DF_E_NO_DEVICE.
 * No device-to-host copy, no synchronisation, no floating-point atomics; every launch covers its range with 64-bit indices.  The
 * time of the edges launch grows with the longest run of uses of ONE edge, which one lane counts.  Workspace, from the
 * per-(device, stream) scratch of dfusion_extract_mesh (dfusion_release_scratch): 108 T + 4 V bytes (two copies of the 6 T 64-bit
 * keys and of their value bytes; the positions reuse the first copy), + 4 (V + 1) if row_start_dev is NULL, and hipcub's sort and
 * scan storage.                                                                                                                      */
int dfusion_mesh_adjacency(const unsigned int *triangles_dev, unsigned long long n_triangles,
                           unsigned long long n_vertices,
                           unsigned int *row_start_dev /* nullable, n_vertices + 1 */,
                           unsigned int *neighbours_dev, unsigned long long neighbour_capacity,
                           unsigned char *vertex_class_dev /* nullable, n_vertices */,
                           unsigned long long *counts_dev /* [8] */, dfStream stream);

/* Taubin's lambda | mu smoothing of a mesh's vertices over that adjacency (no reference counterpart; additive, ABI 7).  Restated in
 * tests/mesh_smooth_ref.py; every output equals it bit for bit (a NaN where it has a NaN).
 * Inputs: V vertices of four floats (x, y, z, w), the CSR of dfusion_mesh_adjacency (row_start_dev [V + 1], neighbours_dev
 * [n_neighbours = row_start[V]]), vertex_class_dev [V] or NULL (= every vertex with a neighbour is of class 1).
 *   STEP       with a factor s, from a buffer P to another buffer Q, for every vertex v (a Jacobi step: no step reads what it writes).
 *              v is MOVABLE iff its degree d > 0 and -- with DF_SMOOTH_FIX_BOUNDARY -- its class is 1.  A vertex that is not movable
 *              is copied, all 16 bytes.  For a movable one, per axis a: acc = 0.f; for each neighbour u in the row's order
 *              acc = acc + P[u].a (f32 adds, one after the other); mean = acc / (float)d (IEEE f32 division); delta = mean - P[v].a;
 *              Q[v].a = P[v].a + s * delta (a multiply, then an add: two roundings, no fma).  w is copied as it is.  NaN and inf
 *              propagate as that arithmetic propagates them.
 *   ITERATION  a step with lambda, then -- unless mu == 0 -- a step with mu on its result.  mu == 0 is plain Laplacian smoothing,
 *              one step an iteration.  iterations == 0 copies the input.
 * vertices_out_dev [V] may be vertices_dev itself (in place, through the scratch).  The neighbour indices and row offsets are
 * TRUSTED, as dfusion_gather_rows trusts its index list: every entry of a row must be < V and row_start_dev ascending within
 * n_neighbours.
 * DF_E_INVALID: iterations < 0, lambda or mu not finite, a flag bit other than DF_SMOOTH_FIX_BOUNDARY, V or n_neighbours > 2^32 - 1,
 * a NULL array (vertex_class_dev apart) with a non-zero length, vertices_out_dev overlapping an input other than by being
 * vertices_dev.  Without a device DF_E_NO_DEVICE.  No device-to-host copy, no synchronisation, no atomics.  Workspace, from the same
 * scratch: 16 V bytes (none for a single step out of place).                                                                        */
#define DF_SMOOTH_FIX_BOUNDARY 1u
int dfusion_mesh_smooth(const float *vertices_dev, unsigned long long n_vertices,
                        const unsigned int *row_start_dev /* n_vertices + 1 */,
                        const unsigned int *neighbours_dev, unsigned long long n_neighbours,
                        const unsigned char *vertex_class_dev /* nullable, n_vertices */,
                        int iterations, float lambda, float mu, unsigned int flags,
                        float *vertices_out_dev, dfStream stream);

/* The closed loops of boundary half-edges of an indexed triangle mesh (no reference counterpart; additive, ABI 7).  DESIGN.md section
 * 27 has the kernels; tests/mesh_holes_ref.py restates the rule in numpy and every output equals it bit for bit.
 * Inputs: T triangles of three uint32 indices over V vertices (the positions take no part).  VALID, HALF-EDGES and the EDGE classes
 * are dfusion_mesh_adjacency's, word for word.
 *   BOUNDARY HALF-EDGE  a half-edge a -> b whose undirected edge is BOUNDARY (f + b == 1).  out(v) and in(v) count those that leave
 *               and enter v.
 *   SIMPLE      v is simple iff out(v) == 1, in(v) == 1 and no IRREGULAR edge ends at v.  Every simple vertex has adjacency class 2;
 *               the reverse does not hold (a vertex where two sheets touch has out == in == 2).
 *   next(v)     of a simple v: the head of its one outgoing boundary half-edge.
 *   LOOP        a simple v is on a loop iff following next from v comes back to v having met only simple vertices.  Every simple
 *               vertex has in == 1, so next is injective on the simple vertices: a walk either closes or ends at a vertex that is not
 *               simple.  Simple vertices whose walk ends are on an OPEN CHAIN and belong to no loop.
 *   LABEL       of a loop: its smallest vertex index.  rank(v) = the number of next steps from the label vertex to v; the loop's
 *               LENGTH L = its vertex count.  L >= 3 always: next(v) != v because a half-edge has different ends, and L == 2 would be
 *               the half-edges a -> b and b -> a, which make the edge {a, b} INTERIOR, not BOUNDARY.
 *   Loops are numbered in ascending label.
 *   vertex_next_dev[v] (nullable)  next(v), or 0xffffffff for a v that is not simple.
 *   vertex_loop_dev[v]             the label of v's loop, or 0xffffffff.
 *   vertex_rank_dev[v] (nullable)  rank(v), or 0xffffffff.
 *   loop_start_dev [loop_capacity + 1], loop_vertices_dev [vertex_capacity]: a CSR of the loops -- loop number i holds
 *               loop_vertices_dev[loop_start_dev[i] .. loop_start_dev[i + 1]), starting at its label vertex and following next.
 *   counts_dev[8] (u64, WRITTEN, always the full numbers): [0] loops, [1] vertices on loops, [2] boundary half-edges (=
 *               dfusion_mesh_adjacency's counts[2]), [3] vertices that are not simple and have out + in > 0, [4] simple vertices on
 *               open chains, [5] the longest loop's length, [6] invalid triangles, [7] degenerate triangles.
 * Nothing is written past a capacity; if [0] exceeds loop_capacity or [1] vertex_capacity the contents of the two CSR arrays are
 * unspecified, the per-vertex arrays and the counts are complete all the same (dfusion_mesh_filter's contract).  Both capacities 0:
 * per-vertex arrays and counts only (neither CSR array is touched).  T == 0 or V == 0 is valid input.  Arrays of length 0 may be NULL.
 * DF_E_INVALID: V > 2^32 - 1, 6 T > 2^32 - 1, a capacity > 2^32 - 1, triangles_dev NULL with T > 0, vertex_loop_dev NULL with V > 0,
 * loop_start_dev NULL unless both capacities are 0, loop_vertices_dev NULL with vertex_capacity > 0, counts_dev NULL, an output array
 * (counts_dev included) that overlaps triangles_dev.  Without a device DF_E_NO_DEVICE.  No device-to-host copy, no synchronisation,
 * integer atomics only (no output depends on scheduling); every launch covers its range with 64-bit indices.  Labels and ranks come
 * from ceil(log2 V) pointer-doubling rounds between two buffers, each a launch over V.  As in dfusion_mesh_adjacency the time of the
 * runs launch grows with the longest run of uses of ONE edge.  Workspace, from the per-(device, stream) scratch of
 * dfusion_extract_mesh (dfusion_release_scratch): 108 T + 76 V bytes and hipcub's sort and scan storage.                              */
int dfusion_mesh_boundary_loops(const unsigned int *triangles_dev, unsigned long long n_triangles,
                                unsigned long long n_vertices,
                                unsigned int *vertex_next_dev /* nullable, n_vertices */,
                                unsigned int *vertex_loop_dev /* n_vertices */,
                                unsigned int *vertex_rank_dev /* nullable, n_vertices */,
                                unsigned int *loop_start_dev /* loop_capacity + 1 */,
                                unsigned long long loop_capacity,
                                unsigned int *loop_vertices_dev, unsigned long long vertex_capacity,
                                unsigned long long *counts_dev /* [8] */, dfStream stream);

/* The mesh with its small holes closed: every loop of dfusion_mesh_boundary_loops of at most max_edges edges gets a fan of triangles
 * around a new vertex at its centroid (no reference counterpart; additive, ABI 7).  Restated in tests/mesh_holes_ref.py; every output
 * equals it bit for bit (a NaN where it has a NaN).
 * Inputs: V vertices of four floats (x, y, z, w), T triangles of three uint32 indices, max_edges, flags (none defined).
 *   FILLED     a loop is filled iff L <= max_edges.  max_edges of 0 to 2 fills nothing (L >= 3) and the mesh is copied.
 *   VERTICES   the V input vertices as they are (16 bytes each), then one new vertex m per filled loop, in ascending label.
 *   TRIANGLES  the T input triangles as they are, invalid ones included, then per filled loop in ascending label L triangles:
 *              triangle j is (v_(j+1) mod L, v_j, m), v_j the loop's vertex of rank j.  Every old boundary edge v_j -> v_(j+1) gets
 *              its opposite half-edge, and each spoke {v_j, m} is used once each way.
 *   POSITION   of m, per axis a: acc = 0.f; for j = 0 .. L-1 in rank order acc = acc + P[v_j].a (f32 adds, one after the other);
 *              m.a = acc / (float)L (IEEE f32 division); w = 0.f.  NaN and inf propagate as that arithmetic propagates them.
 *   vertex_src_dev[i] (nullable, vertex_capacity)  i for i < V, 0xffffffff for a new vertex: it has no source row.
 *   counts_dev[8] (u64, WRITTEN, always the full numbers): [0] output vertices, [1] output triangles, [2] loops filled, [3] loops
 *              left open, [4] triangles added, [5] the longest filled loop, [6] the longest loop left open (0 if none), [7] simple
 *              vertices on open chains.
 * Boundary edges fall by the sum of the filled L, irregular edges are unchanged, the Euler characteristic rises by one per filled
 * loop, and filling the result again with the same max_edges adds nothing.  New indices are 32-bit: V + [2] must stay below 2^32 - 1.
 * The input triangles go across as they are: an INVALID one that names an index in V .. V + [2] - 1 is a valid triangle on a new
 * vertex in the output, and the four statements above are made for meshes without such a triangle.
 * Nothing is written past a capacity; if a count exceeds its capacity the contents of the output arrays are unspecified
 * (dfusion_mesh_filter's contract).  Both capacities 0: counts only.  T == 0 or V == 0 is valid input: the mesh is copied.
 * DF_E_INVALID: a flag bit, V > 2^32 - 1, 6 T > 2^32 - 1, a capacity > 2^32 - 1, a NULL input or output array with a non-zero size
 * or capacity, counts_dev NULL, an output array (counts_dev included) that overlaps vertices_dev or triangles_dev.  Without a device
 * DF_E_NO_DEVICE.  No device-to-host copy, no synchronisation, integer atomics only.  The loop stage runs inside the call, through
 * the same scratch (dfusion_mesh_boundary_loops' workspace); the old arrays go across as device-to-device copies.  ONE lane walks a
 * filled loop for its centroid, L <= max_edges dependent loads: the time of that launch grows with max_edges.                        */
int dfusion_mesh_fill_holes(const float *vertices_dev, unsigned long long n_vertices,
                            const unsigned int *triangles_dev, unsigned long long n_triangles,
                            unsigned int max_edges, unsigned int flags,
                            float *vertices_out_dev, unsigned long long vertex_capacity,
                            unsigned int *triangles_out_dev, unsigned long long triangle_capacity,
                            unsigned int *vertex_src_dev /* nullable, vertex_capacity */,
                            unsigned long long *counts_dev /* [8] */, dfStream stream);

/* Closest point on a triangle mesh: for every query point the nearest eligible triangle, the closest point on it, the squared distance
 * and the barycentrics, through a linear BVH built inside the call (no reference counterpart; additive, ABI 7).  DESIGN.md section 28
 * has the kernels, the slack of the pruning bound and the stack bound; tests/mesh_closest_ref.py restates the rule in numpy by brute
 * force over all triangles, and triangle, point, bary and counts [0] - [5] equal it bit for bit: the tree only prunes.
 * Inputs: V vertices of four floats (x, y, z, w; w ignored), T triangles of three uint32 indices, Q query points of four floats (w
 * ignored), max_dist2 (f32; +inf: no limit).
 *   ELIGIBLE   a triangle whose three indices are < V and pairwise different and whose nine coordinates are finite.  Every other one is
 *              skipped and counted.  A geometrically degenerate triangle with three different indices stays eligible: the arithmetic
 *              below decides what it yields.
 *   DISTANCE   of the query p to the triangle (a, b, c): the Voronoi-region routine of Ericson, Real-Time Collision Detection 5.1.5, in
 *              its published order of tests.  Every operation is ONE f32 operation, nothing is fused, dot(x, y) = x.x*y.x + x.y*y.y +
 *              x.z*y.z added left to right, divisions are IEEE f32:
 *                ab = b - a; ac = c - a; ap = p - a; d1 = dot(ab, ap); d2 = dot(ac, ap);
 *                bp = p - b; d3 = dot(ab, bp); d4 = dot(ac, bp);  cp = p - c; d5 = dot(ab, cp); d6 = dot(ac, cp);
 *                vc = d1*d4 - d3*d2; vb = d5*d2 - d1*d6; va = d3*d6 - d5*d4;
 *                1 vertex A  if d1 <= 0 && d2 <= 0:                      v = 0, w = 0
 *                2 vertex B  else if d3 >= 0 && d4 <= d3:                v = 1, w = 0
 *                3 edge AB   else if vc <= 0 && d1 >= 0 && d3 <= 0:      v = d1 / (d1 - d3), w = 0
 *                4 vertex C  else if d6 >= 0 && d5 <= d6:                v = 0, w = 1
 *                5 edge AC   else if vb <= 0 && d2 >= 0 && d6 <= 0:      v = 0, w = d2 / (d2 - d6)
 *                6 edge BC   else if va <= 0 && d4 - d3 >= 0 && d5 - d6 >= 0:  w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), v = 1 - w
 *                7 face      else:  denom = 1 / ((va + vb) + vc); v = vb * denom; w = vc * denom
 *              u = (1 - v) - w; point = (a + ab*v) + ac*w per axis (each product rounded, then the two adds); e = p - point;
 *              d2 = dot(e, e).  A NaN anywhere makes the comparisons false, falls through to the face case and gives a NaN d2.
 *   WINNER     the routine is applied to every eligible triangle t.  The candidate (d2, t) is admissible iff d2 <= max_dist2 (a NaN
 *              never is); it beats the best so far iff its d2 is smaller, or equal with a smaller t.
 *   NO WINNER  (no eligible triangle, a query with a non-finite x, y or z, nothing within max_dist2): triangle 0xffffffff, point x, y,
 *              z = the bits 0x7fc00000, d2 = +inf, barycentrics 0.
 *   triangle_dev[q]           the winner's index.
 *   point_dev[4 q ..]         (x, y, z, d2).
 *   bary_dev[4 q ..] (nullable)  (u, v, w, 0).
 *   counts_dev[8] (u64, WRITTEN, always): [0] queries with a winner, [1] without, [2] eligible triangles, [3] skipped triangles, [4] the
 *              f32 bits of the largest winning d2 (0 if [0] == 0), [5] the smallest query index that attains it (0xffffffff if none) --
 *              both from one 64-bit integer atomic max over {bits, ~q} --, [6] triangle tests made and [7] tree nodes visited, summed
 *              over the queries: integer sums, reproducible for one input, but a property of the tree and not of the rule.
 * T == 0, V == 0 and Q == 0 are valid inputs; with Q == 0 the triangles are still counted.  Arrays of length 0 may be NULL.
 * DF_E_INVALID: V, T or Q > 2^32 - 1, a NULL array (bary_dev apart) with a non-zero length, counts_dev NULL, an output array
 * (counts_dev included) that overlaps vertices_dev, triangles_dev or queries_dev.  Without a device DF_E_NO_DEVICE.  No device-to-host
 * copy, no synchronisation, integer atomics only (no output but [6] and [7] depends on the tree, none on scheduling); every launch
 * covers its range with 64-bit indices.  The tree lives in the workspace and is rebuilt by every call.  Workspace, from the
 * per-(device, stream) scratch of dfusion_extract_mesh (dfusion_release_scratch): 77 T + 48 bytes, every array rounded up to 16, and
 * hipcub's storage for one sort of T 64-bit keys.                                                                                    */
int dfusion_mesh_closest_points(const float *vertices_dev, unsigned long long n_vertices,
                                const unsigned int *triangles_dev, unsigned long long n_triangles,
                                const float *queries_dev, unsigned long long n_queries, float max_dist2,
                                unsigned int *triangle_dev /* n_queries */, float *point_dev /* 4 n_queries */,
                                float *bary_dev /* nullable, 4 n_queries */,
                                unsigned long long *counts_dev /* [8] */, dfStream stream);

/* Ray queries against a triangle mesh: for every ray the first eligible triangle it hits -- or, with DF_RAYS_ANY_HIT, whether it hits
 * any --, the hit point with its parameter and the barycentrics, through the linear BVH of dfusion_mesh_closest_points, built inside
 * the call (no reference counterpart; additive, ABI 7).  DESIGN.md section 29 has the kernel and the proof that the tree only prunes;
 * tests/mesh_rays_ref.py restates the rule in numpy by brute force over all triangles, and triangle, hit, bary and counts [0] - [5]
 * equal it bit for bit.
 * Inputs: V vertices of four floats (w ignored), T triangles of three uint32 indices, R rays as origins o and directions d of four
 * floats each (w ignored), t_min and t_max (f32, for every ray).  d is used as given, never normalised: t is in units of d.
 * Every operation below is ONE f32 operation, nothing is fused, dot(x, y) = x.x*y.x + x.y*y.y + x.z*y.z added left to right, a cross
 * product component is a*b - c*d as two products and one difference, divisions are IEEE f32.  min(a, b) and max(a, b) are fminf and
 * fmaxf -- a NaN operand is dropped -- with the one case IEEE leaves open pinned: of two EQUAL operands (zeros of either sign included)
 * the second is returned: max(a, b) = (b is NaN || a > b) ? a : b, min alike with <.
 *   ELIGIBLE   a triangle as for dfusion_mesh_closest_points: three indices < V, pairwise different, nine finite coordinates.  Every
 *              other one is skipped and counted.
 *   VALID      a ray whose o.x, o.y, o.z, d.x, d.y, d.z are finite and whose d is not (+-0, +-0, +-0).  An invalid ray hits nothing and
 *              is counted.
 *   TEST       Moeller-Trumbore, two-sided, of a valid ray against the triangle (A, B, C):
 *                e1 = B - A; e2 = C - A; p = d x e2; det = dot(e1, p); inv = 1 / det;
 *                s = o - A; u = dot(s, p) * inv; q = s x e1; v = dot(d, q) * inv; t = dot(e2, q) * inv;
 *              the triangle is a CANDIDATE iff det != 0 && u >= 0 && v >= 0 && u + v <= 1 && t >= t_min && t <= t_max (a NaN anywhere
 *              fails it); side = det > 0 ? +1 : -1.
 *   BOX        Moeller-Trumbore's t has no bounded error for a long sliver hit at a grazing angle, so the rule itself carries the
 *              triangle's vertex box [lo, hi] (per axis the fminf / fmaxf of the three coordinates) and a tree over unions of such
 *              boxes stays exact by monotone rounding alone.  slack = m * 2^-18 + 2^-126, m = the largest |coordinate| of all
 *              eligible triangles and of o.  slab(lo, hi), on the box grown to [lo - slack, hi + slack]: tn = -inf, tf = +inf; per
 *              axis k = x, y, z, with inv_k = 1 / d_k: where inv_k is +-inf (d_k is zero or so small that its reciprocal overflows) the
 *              axis is PARALLEL -- the box fails unless lo_k - slack <= o_k <= hi_k + slack, and t is not constrained --, otherwise
 *              a = ((lo_k - slack) - o_k) * inv_k; b = ((hi_k + slack) - o_k) * inv_k; tn = max(tn, min(a, b)); tf = min(tf, max(a, b)).
 *              Then tn = max(tn, t_min); tf = min(tf, t_max); the box PASSES iff tn <= tf.
 *   ACCEPTED   a candidate whose own vertex box passes; t_hit = min(max(t, tn), tf) with that box's tn and tf.
 *   WINNER     the accepted candidate with the smallest t_hit, ties to the smaller triangle index.
 *   NO HIT     (no accepted candidate, an invalid ray): triangle 0xffffffff, hit x, y, z = the bits 0x7fc00000 and w = +inf, bary 0.
 *   triangle_dev[r]           the winner's index; with DF_RAYS_ANY_HIT 0 if ANY candidate is accepted (whichever), else 0xffffffff.
 *   hit_dev[4 r ..]           (o.x + d.x * t_hit, o.y + d.y * t_hit, o.z + d.z * t_hit, t_hit): one product and one sum per axis.
 *   bary_dev[4 r ..] (nullable)  ((1 - u) - v, u, v, side).
 *   counts_dev[8] (u64, WRITTEN, always): [0] rays with a hit, [1] without (invalid ones included), [2] eligible triangles, [3] skipped
 *              triangles, [4] invalid rays, [5] 0, [6] triangle tests made and [7] tree nodes visited, summed over the rays: integer
 *              sums, reproducible for one input, but a property of the tree and not of the rule.
 * With DF_RAYS_ANY_HIT the walk stops at a ray's first accepted candidate and hit_dev and bary_dev must be NULL.
 * T == 0, V == 0 and R == 0 are valid inputs; with R == 0 the triangles are still counted.  Arrays of length 0 may be NULL.
 * DF_E_INVALID: V, T or R > 2^32 - 1, a flag bit other than DF_RAYS_ANY_HIT, a NULL array (bary_dev apart; hit_dev too with
 * DF_RAYS_ANY_HIT) with a non-zero length, hit_dev or bary_dev given with DF_RAYS_ANY_HIT, counts_dev NULL, an output array (counts_dev
 * included) that overlaps vertices_dev, triangles_dev, origins_dev or directions_dev.  Without a device DF_E_NO_DEVICE.  No
 * device-to-host copy, no synchronisation, integer atomics only; every launch covers its range with 64-bit indices.  The tree lives in
 * the workspace and is rebuilt by every call.  Workspace: that of dfusion_mesh_closest_points for T triangles.                          */
#define DF_RAYS_ANY_HIT 1u
int dfusion_mesh_ray_hits(const float *vertices_dev, unsigned long long n_vertices,
                          const unsigned int *triangles_dev, unsigned long long n_triangles,
                          const float *origins_dev, const float *directions_dev, unsigned long long n_rays,
                          float t_min, float t_max, unsigned int flags,
                          unsigned int *triangle_dev /* n_rays */, float *hit_dev /* 4 n_rays; NULL with DF_RAYS_ANY_HIT */,
                          float *bary_dev /* nullable, 4 n_rays */,
                          unsigned long long *counts_dev /* [8] */, dfStream stream);

/* ---- colour volume (no reference counterpart: KinFu::operator() drops its colour image; additive, ABI 7) ----------------------
 * A colour volume belongs to a TSDF volume: the same dims, linear layout (x + y X + z X Y) and stored planes (DfSlab), 4 bytes a
 * voxel {c0, c1, c2, w}: three channels in the byte order of the input image (the kernels treat them alike) and a weight byte;
 * cleared = all zero.  `geometry` is the TSDF volume's DfVolume; its data pointer is not looked at.  DESIGN.md states the rule in
 * full; tests/color_ref.py restates it in numpy and the bytes equal it.
 *
 * dfusion_color_integrate fuses one image (rgb_dev: 4 bytes a pixel, the 4th ignored; same cols x rows as dists) through the
 * composition of dfusion_integrate_warped.  It READS the TSDF volume as it is when the call runs (in a frame: after that frame's
 * depth integrate) and never writes it.
 *   select   voxels of the slab's own planes with stored weight > 0 and fabsf(tsdf) < band (0 < band <= 1; strict, so saturated
 *            free space is out), in ascending linear index; at most `capacity` of them, lowest indices first, are processed;
 *            *n_selected_dev (nullable) is WRITTEN with the full count, so a caller can see a truncation;
 *   project  x_c = vol2world * (x vsx, y vsy, z vsz); x_w = DQB(x_c).transform(x_c) over the k nearest nodes in nanoflann's tie order
 *            (wf NULL: x_w = x_c; k is then ignored); vc = world2cam * x_w; u = fmaf(fx, vc.x / vc.z, cx), v alike; skipped unless
 *            u >= 0 && v >= 0 && u < cols && v < rows (NaN skips); Dp = dists[(int)v][(int)u]; skipped if Dp == 0 || vc.z <= 0;
 *            sdf = Dp - sqrtf(dot(vc, vc)); the voxel is OBSERVED iff fabsf(sdf) < band * trunc_dist -- the occlusion test: a voxel
 *            behind what the camera sees keeps its colour;
 *   fuse     integer arithmetic, c = the bytes of pixel [(int)v][(int)u], w = the stored weight byte: every channel becomes
 *            (old w + c + ((w + 1) >> 1)) / (w + 1), then w <- min(w + 1, max_weight), 1 <= max_weight <= 255.  One thread writes a
 *            voxel; *n_fused_dev (nullable) is WRITTEN with the number of voxels fused.
 * No device-to-host copy and no synchronisation: the launches cover the capacity and the device-side count bounds the work.
 * Workspace: 8 bytes per 256 voxels + 16 bytes per voxel of capacity, from the per-(device, stream) scratch of dfusion_integrate.
 * DF_E_INVALID: a NULL pointer (wf, the counters excepted), a pitch shorter than a row, rgb_dev or its pitch not 4-byte aligned, band outside (0, 1] or NaN, max_weight outside
 * 1..255, capacity <= 0, with a warp field k outside 1..8 or fewer nodes than k, more than 2^32 - 1 stored voxels.
 *
 * dfusion_color_fetch reads the colour of N points (float4, as dfusion_extract_cloud / _mesh return them) into rgba_out_dev (4 bytes
 * a point): p = world2vol * point (the caller inverts the volume pose); cf = p / voxel_size per axis; g = floorf(cf), a, b, c = cf - g;
 * the eight taps g + (dx, dy, dz) in the order z fastest, then y, then x, each with weight ((dx ? a : 1 - a) (dy ? b : 1 - b))
 * (dz ? c : 1 - c); a tap outside the stored volume or with weight byte 0 is left out; sw and the three channel sums add up in tap
 * order (products rounded before the add); sw > 0: every channel is min(255, (int)floorf(sc / sw + 0.5f)) and the 4th byte 255, else
 * all four bytes are 0, as for a point with a non-finite component.                                                              */
int dfusion_color_clear(void *color_dev, DfVolume geometry, const DfSlab *slab, dfStream stream);
int dfusion_color_integrate(const unsigned char *rgb_dev, size_t rgb_pitch, const uint16_t *dists_dev, size_t dists_pitch, int cols,
                            int rows, DfVolume v, const DfSlab *slab, void *color_dev, const float vol2world[12],
                            const float world2cam[12], const float proj[4], DfWarpField *wf, int k, float band, int max_weight,
                            long long capacity, unsigned long long *n_selected_dev, unsigned long long *n_fused_dev, dfStream stream);
int dfusion_color_fetch(const void *color_dev, DfVolume geometry, const DfSlab *slab, const float world2vol[12],
                        const float *points_dev, unsigned long long N, unsigned char *rgba_out_dev, dfStream stream);

/* ---- warp field -----------------------------------------------------------------------------
 * WarpField::WarpField / ~WarpField (warp_field.cpp:17-34).                                    */
int dfusion_warp_create(DfWarpField **out);
int dfusion_warp_destroy(DfWarpField *wf);

/* WarpField::init + buildKDTree (warp_field.cpp:41-88,275-282): upload M nodes.
 *   pos_dev[M*3]   deformation_node::vertex
 *   dq_dev[M*8]    deformation_node::transform = {rotation_ (w,x,y,z), translation_ (w,x,y,z)},
 *                  the first 32 bytes of utils::DualQuaternion<float> (dual_quaternion.hpp:231-232)
 *   sigma_dev[M]   deformation_node::weight (dg_w)
 * Invalidates the k-NN index (node positions changed).                                        */
int dfusion_warp_set_nodes(DfWarpField *wf, const float *pos_dev, const float *dq_dev, const float *sigma_dev,
                           int M, dfStream stream);

/* Per-frame transform update (what WarpFieldOptimiser writes back, CombinedSolver.h:189-197);
 * node positions, hence the k-NN index, are unchanged.                                        */
int dfusion_warp_set_transforms(DfWarpField *wf, const float *dq_dev, dfStream stream);

/* Builds the exact k-NN acceleration index for voxel queries of this volume geometry: for each
 * 8x8x8 brick the list of nodes that can be among the k nearest of ANY of its voxels, and (flag
 * DF_INDEX_VOXEL_TABLE) the per-voxel k-NN table of the slab's own planes.  Replaces the kd-tree
 * build (warp_field.cpp:275-282); needed again only when node POSITIONS change (they do not between
 * frames: only transforms are optimised).  `geometry.data` is not dereferenced.  Blocks until built. */
int dfusion_warp_build_index(DfWarpField *wf, DfVolume geometry, const DfSlab *slab, const float vol2world[12], int k,
                             unsigned flags, dfStream stream);

/* Grows the warp field (DynamicFusion section 3.4, "extending the warp field"; the reference never adds nodes) -- an ABI-7 addition.
 * points_dev[N*3] are canonical surface points.  With the current M nodes {v_i, dq_i, sigma_i}:
 *   - p is UNSUPPORTED when it is finite, M >= k, and d2_i >= sigma_i * sigma_i (f32) for each of its k nearest nodes i (what
 *     dfusion_knn returns, nanoflann's tie order included);
 *   - cell of p = ((int)floorf(p.x / radius), (int)floorf(p.y / radius), (int)floorf(p.z / radius)), IEEE f32 division; points with
 *     |p / radius| >= 2^30 on an axis are skipped; in each cell the unsupported point with the LOWEST index wins;
 *   - the winners with the lowest indices, at most min(max_new, 65535 - M) of them, are appended as nodes M, M+1, ... in increasing
 *     point index: vertex = p, dg_w = sigma_new, transform = WarpField::DQB(p) over the OLD nodes (warp_field.cpp:203-217) -- or, when
 *     all k weights are 0, the transform of p's nearest node.  Old nodes keep their index, position, transform and dg_w.
 * Afterwards every result of the handle (k-NN, warp, solver, warped integrate, index info) is, bit for bit, that of
 * dfusion_warp_set_nodes(grown set) + dfusion_warp_build_index(geometry, k and flags of the last build, if there was one) on a fresh
 * handle.  The index is updated in place: brick lists re-made, and only the per-voxel table blocks whose brick list changed or whose
 * build met an exact distance tie are re-made (on demand, or inside this call for eager tables).  A prepared plan is voided when
 * nodes are added.  If a step after the nodes went in fails, *n_added still reports them and the handle has no index.
 *   new_pos_dev[max_new*3], new_dq_dev[max_new*8], new_sigma_dev[max_new]  nullable: the added nodes (layout of dfusion_warp_set_nodes)
 *   n_added, n_winners  host: nodes added, and cells won (n_added < n_winners when truncated)
 * N = 0 or no winner: DF_OK, *n_added = 0, the handle untouched.  DF_E_INVALID: k outside 1..8, M < k, radius <= 0 or not finite,
 * sigma_new not finite, N < 0 or > 2^28, max_new < 0.  Blocks until done.                                                                      */
int dfusion_warp_extend(DfWarpField *wf, int k, const float *points_dev, int N, float radius, float sigma_new, int max_new,
                        float *new_pos_dev, float *new_dq_dev, float *new_sigma_dev, int *n_added, int *n_winners, dfStream stream);

/* Introspection of the k-NN index (blocking): total candidate-list entries, number of 8^3 bricks, k it was built for. */
int dfusion_warp_index_info(const DfWarpField *wf, unsigned long long *total_entries, unsigned int *n_bricks, int *k_built);

/* Locality hint for dfusion_knn / dfusion_warp_points (and the solver's k-NN): the query points are the pixels of an image
 * `image_cols` wide in row-major order (the ray-cast cloud KinFu::dynamicfusion warps, kinfu.cpp:353-391).  Queries whose count is a
 * whole number of 8-row bands are then processed in 8 x 8 pixel tiles per wave instead of 64-pixel row segments; results are
 * identical, only faster (fewer distinct index bricks per wave).  0 switches it off (default).                                   */
int dfusion_warp_set_point_tiling(DfWarpField *wf, int image_cols);

/* Device self-test of the sweeps' short arithmetic forms (dfusion_device.h) against the generic ones they replace; no reference
 * counterpart, used by the parity tests.  counts_dev: TEN device entries (ABI 5; eight in ABI 2-4, six in ABI 1), cleared by the call, receive
 * mismatch counts: [0] short sqrtf over every f32 of its domain, [1] short f64 reciprocal over every positive normal f32, [2] packed
 * quaternion products on n_random random pairs (specials included), [3] near-unit normalisation on the normalised quaternions among
 * them, [4] how many of those there were, [5] the short fuse division on every finite stored half x 97 weights x (n_random >> 21)
 * tsdf values, [6] the projective sample -- tsdf_sample_fast and the two-stage saturation form of the rigid sweep -- against the
 * generic statements on n_random positions inside the forms' domain and on its edges, [7] how many of those samples updated,
 * [8] the blend's first normalisation as an f32 division (q_div_f32) against (float)((1.0 / (double)n) * (double)c) on the quaternions
 * its domain test accepts out of n_random random and edge-of-domain ones, [9] how many quaternions that were.                       */
int dfusion_selftest_exact_forms(unsigned long long n_random, unsigned long long *counts_dev, dfStream stream);

/* Measurement hook of dfusion_integrate_warped's cached sweep, per warp-field handle (NULL switches it off): while set, every
 * launch through this handle ADDS to *swept_dev (device, 8 bytes) the voxels of the (8 x 8 column patch, 4-plane half layer) cells its
 * launch plan keeps, i.e. the voxels that go through blend -> transform -> project.                                              */
int dfusion_warp_debug_counters(DfWarpField *wf, unsigned long long *swept_dev);

/* What the last dfusion_integrate_warped through this handle found alive: per_layer_dev[l] (device, n_layers entries, l = global
 * plane / 8) is INCREMENTED by the number of 8 x 8 x 8 blocks of layer l that its verdict pass kept, for the layers that lie
 * entirely inside planes [z0, z0 + zn).  Z-slab re-balancing reads it (one all-reduce over the ranks gives the global profile of the
 * sweep's real work per plane).  DF_E_NO_INDEX when no sweep with verdicts has run since the index was built.                       */
int dfusion_warp_alive_blocks(DfWarpField *wf, int z0, int zn, unsigned long long *per_layer_dev, int n_layers, dfStream stream);
/* Same, counting only the kept blocks that had 4-bit neighbour codes for the sweep to read (blocks with a blend model made in an
 * earlier frame; DF_WARP_NO_CODES makes a sweep ignore them, the count is of what was available).  A measurement hook: tests use it
 * to see that the coded path engaged.                                                                                              */
int dfusion_warp_coded_blocks(DfWarpField *wf, int z0, int zn, unsigned long long *per_layer_dev, int n_layers, dfStream stream);

/* WarpField::KNN (warp_field.cpp:247-251) for N query points [N*3]: idx[N*k] int32, d2[N*k], ascending distance; exactly
 * equidistant nodes in the order the reference's nanoflann walk meets them (nanoflann.hpp:110-131,1200-1254).                    */
int dfusion_knn(DfWarpField *wf, int k, const float *queries_dev, int N, int *idx_dev, float *d2_dev, dfStream stream);

/* WarpField::warp (warp_field.cpp:180-195) on device: points/normals [N*3] in place
 * (normals_dev nullable); NaN points are skipped; warp_to_live = WarpField::warp_to_live_.     */
int dfusion_warp_points(DfWarpField *wf, int k, float *points_dev, float *normals_dev, int N,
                        const float warp_to_live[12], dfStream stream);

/* WarpFieldOptimiser::optimiseWarpData (CombinedSolver / Opt energy kfusion/solvers/dynamicfusion.t:26-52) and
 * WarpField::energy_data (Ceres, warp_field.cpp:117-163, functor optimisation.hpp:36-71): the DATA term
 *     E(T) = sum_v | (live_v - canonical_v) - sum_{i<k} w_vi * T_{n_vi} |^2
 * over the node translations T (n_vi, w_vi: the k nearest nodes of canonical_v and their weights; rotations are not
 * unknowns and there is no regularisation term in the reference either).  Linear least squares: `iters` conjugate-
 * gradient steps on (W^T W + lambda I) delta = W^T e(T_now), all on the device, then T <- T_now + delta and every node's
 * translation_ <- 0.5 * (0, T) * rotation_ (encodeTranslation, dual_quaternion.hpp:82-85) -- the node transforms of `wf`
 * are updated in place (the k-NN index stays valid: positions are untouched).
 *   canonical_dev, live_dev  [N*3] packed; a NaN component in either skips the point (warp_field.cpp:130-136)
 *   dq_out_dev (nullable)    [M*8] the updated transforms, layout of dfusion_warp_set_nodes
 *   energy_dev (nullable)    2 floats: E before, E after
 * Float sums use fixed trees (no atomics): the result is reproducible run to run.                                      */
int dfusion_warp_solve_data_term(DfWarpField *wf, int k, const float *canonical_dev, const float *live_dev, int N, int iters,
                                 float lambda, float *dq_out_dev, float *energy_dev, dfStream stream);

/* The same solve with DynamicFusion's regularisation term (section 3.3, eq. 8; declared and left empty by the reference: WarpField::energy_reg,
 * DynamicFusionRegEnergy) over a node graph -- additions to ABI 7.  Edge e = i * kg + s runs from node i to the s-th of its kg nearest
 * OTHER nodes j: dfusion_knn with k = kg + 1 on the node positions (nanoflann's tie order) without the entry whose id is i, or without
 * the last entry when none is (duplicate positions).  With g_e = T_i(v_j) - T_j(v_j) at the transforms the handle holds when the call
 * starts (v_j node j's position, T_n = DualQuaternion::transform of node n) and alpha_e = max(dg_w_i, dg_w_j):
 *     E_reg(delta) = sum_e alpha_e | g_e + delta_i - delta_j |^2                       (psi quadratic; rotations stay fixed)
 * and the call takes `iters` conjugate-gradient steps on (W^T W + lambda I + lambda_reg L) delta = W^T e0 - lambda_reg b, where
 * L delta and b are the node sums of alpha_e (delta_i - delta_j) and alpha_e g_e: + over a node's outgoing edges in slot order, then
 * - over its incoming edges in ascending edge id.  Fixed sum orders, no atomics: reproducible, and restated in tests/solver_reg_ref.py.
 *   kg          graph neighbours, 0..7; kg > 0 needs M >= kg + 1
 *   lambda_reg  weight of E_reg, >= 0
 *   energy_dev  (nullable) 4 floats: E_data before, E_data after, E_reg before, E_reg after (E_reg without lambda_reg)
 * kg == 0 or lambda_reg == 0 switches the term off: the call is dfusion_warp_solve_data_term, launch for launch and bit for bit, and
 * energy_dev[2..3] = 0.  The graph is kept on the handle for (node set, kg); dfusion_warp_set_nodes and a dfusion_warp_extend that adds
 * nodes drop it and the next regularised solve rebuilds it; dfusion_warp_set_transforms leaves it alone.
 * DF_E_INVALID: what dfusion_warp_solve_data_term refuses, kg outside 0..7, kg > 0 with M < kg + 1, lambda_reg negative or NaN.         */
int dfusion_warp_solve(DfWarpField *wf, int k, const float *canonical_dev, const float *live_dev, int N, int iters, float lambda,
                       int kg, float lambda_reg, float *dq_out_dev, float *energy_dev, dfStream stream);
/* The robust form of dfusion_warp_solve (DynamicFusion section 3.3: Tukey penalty on the point residuals, eq. 7; Huber penalty on the
 * edges, eq. 8) by iteratively re-weighted least squares -- an addition to ABI 7.  The call runs `rounds` rounds; a round is one
 * dfusion_warp_solve with weights, starting from the transforms the previous round wrote:
 *     e0 at the handle's transforms;   omega_v = (1 - s_v / c^2)^2 for s_v = |e0_v|^2 < c^2, else 0          (c = tukey_c)
 *     g_e at the handle's transforms;  omega_e = 1 for s_e = |g_e|^2 <= delta^2, else delta / sqrt(s_e)      (delta = huber_delta)
 *     `iters` conjugate-gradient steps on (W^T Omega W + lambda I + lambda_reg L') delta = W^T Omega e0 - lambda_reg b',
 *     L' and b' with alpha'_e = alpha_e * omega_e; write back; dfusion_warp_set_transforms.
 * The k-NN, the exp weights and the node-major lists are made once per call.  Omega enters through a scaled copy of the node-major entry
 * weights, alpha' is a copy in the call's workspace: the handle's cached graph is only read.  Nothing returns to the host between rounds.
 *   tukey_c      0 = quadratic data term;  huber_delta  0 = quadratic regularisation (also when kg == 0 or lambda_reg == 0: no edges)
 *   energy_dev   (nullable) 4 floats: E_data before round 1, E_data after the last round, E_reg before, E_reg after -- the robust
 *                energies sum_v c^2/3 (1 - (1 - s/c^2)^3) (c^2/3 from c^2 on) and sum_e alpha_e (s up to delta^2, 2 delta sqrt(s) - delta^2
 *                above), which tend to the quadratic ones as the thresholds grow; a term switched off reports dfusion_warp_solve's value
 *   point_weights_dev (nullable) [N] the last round's omega_v (1 everywhere with tukey_c == 0)
 *   edge_weights_dev  (nullable) [M*kg] the last round's omega_e (1 everywhere with huber_delta == 0)
 * Both thresholds 0 and rounds == 1: the call is dfusion_warp_solve, launch for launch; with rounds == R the transforms are those of R
 * successive dfusion_warp_solve calls.  Restated in tests/solver_robust_ref.py.
 * DF_E_INVALID: what dfusion_warp_solve refuses, rounds < 1, tukey_c or huber_delta negative or NaN, edge_weights_dev without edges.    */
int dfusion_warp_solve_robust(DfWarpField *wf, int k, const float *canonical_dev, const float *live_dev, int N, int iters, float lambda,
                              int kg, float lambda_reg, int rounds, float tukey_c, float huber_delta, float *dq_out_dev,
                              float *energy_dev, float *point_weights_dev, float *edge_weights_dev, dfStream stream);
/* dfusion_warp_solve_robust with the paper's point-to-plane data term (DynamicFusion section 3.3, eq. 7: the residual along the predicted
 * model normal) -- an addition to ABI 7.  normals_dev [N*3] packed, in the frame of canonical_dev and live_dev, used as given (never
 * normalised).  With e0 as above and n_v the point's normal:
 *     rho_v = (nx ex + ny ey) + nz ez;     E_data = sum_v rho_v^2;     omega_v from s_v = rho_v^2
 *     `iters` conjugate-gradient steps on (W^T N Omega N^T W + lambda I + lambda_reg L') delta = W^T Omega (n rho) - lambda_reg b',
 * N N^T the per-point projection u -> n (n . u).  The matrix differs between x, y and z, so the three components are ONE conjugate-
 * gradient recurrence: every dot product is the three per-component sums combined as (s0 + s1) + s2.  A point is also skipped when a
 * component of its normal is NaN or infinite; a zero normal leaves a valid point that contributes nothing.  Everything else -- the
 * rounds, Huber, the energies' layout (E_data of rho), point_weights_dev, edge_weights_dev -- is dfusion_warp_solve_robust's; tangential
 * slip of the live points along the surface, which projective association leaves behind, does not move the nodes.
 * Restated in tests/solver_plane_ref.py.
 * DF_E_INVALID: what dfusion_warp_solve_robust refuses, normals_dev == NULL.                                                              */
int dfusion_warp_solve_plane(DfWarpField *wf, int k, const float *canonical_dev, const float *live_dev, const float *normals_dev, int N,
                             int iters, float lambda, int kg, float lambda_reg, int rounds, float tukey_c, float huber_delta,
                             float *dq_out_dev, float *energy_dev, float *point_weights_dev, float *edge_weights_dev, dfStream stream);
/* The warp solve with the node ROTATIONS as unknowns too, against the warp the rest of the pipeline applies (DynamicFusion section 3.3:
 * SE(3) per node) -- an addition to ABI 7.  With y_v = DQB(canonical_v).transform(canonical_v) and n'_v the normal as
 * dfusion_warp_points warps them at the transforms the handle holds (identity warp_to_live), c_n = T_n(pos_n):
 *     E = sum_v Omega_v |n'_v . (live_v - y_v)|^2 + lambda_reg sum_e alpha_e |T_i v_j - T_j v_j|^2
 * (normals_dev == NULL: the full 3-vector residual).  `rounds` Gauss-Newton rounds, each re-linearised at the transforms the one before
 * wrote, each `iters` conjugate-gradient steps on six unknowns a node (omega_n, a rotation about c_n, and tau_n), ONE recurrence over
 * the 3-component array of 2M entries (omega_n at n, tau_n at M + n).  f32, no contraction, sums in slot / list / edge order:
 *   once per call   k-NN of canonical; w_vi = exp(-d2 / 2 sigma^2), S_v = ((w_0 + w_1) + ...), wn_vi = w_vi / S_v.  A point is skipped
 *                   when canonical or live has a NaN, S_v == 0, a normal component is NaN or infinite, or a component of y_v or n'_v
 *                   of the FIRST round is.  Node-major lists and the graph as in dfusion_warp_solve.
 *   per round       e_v = live_v - y_v, rho_v = (n'x ex + n'y ey) + n'z ez; T_v = sum_i w_vi t_i, a_v = y_v - T_v; q_n = c_n - t_n; per edge
 *                   e = (i -> j): g_e = T_i v_j - c_j, b_e = T_i v_j - c_i; Tukey on rho^2 (or |e|^2) and Huber on g as in
 *                   dfusion_warp_solve_robust.
 *   J p             the blend turns a point by the normalised sum of the weighted node rotations and adds the node translations under
 *                   the UNNORMALISED weights, so per point: st = st + w (p_tau_n - (p_om_n x q_n)), sr = sr + wn p_om_n over the slots,
 *                   u = st + (sr x a_v); with normals u = n' (n' . u)
 *   J^T u           per node over its list: S1 = sum w u, S2 = sum wn (a_v x u); tau = S1 + lambda p_tau,
 *                   om = (S2 - (q_n x S1)) + lambda_rot p_om
 *   regularisation  d_e = (p_tau_i + (p_om_i x b_e)) - p_tau_j; tau_n: + alpha_e d_e over the outgoing edges in slot order, then
 *                   - alpha_e d_e over the incoming edges in ascending edge id; om_n: + alpha_e (b_e x d_e) over the outgoing edges.
 *                   Right-hand side: the same with d_e = g_e, r0 = J^T Omega b - lambda_reg acc.
 *   write-back      a node whose six components are all exactly 0 keeps its eight floats; otherwise qo = normalize((1, om / 2)),
 *                   r' = qo * normalize(rot), t' = (qo (t - c) + c) + tau, dual' = 0.5 (0, t') r'.
 *   energy_dev      E_data before (the first round's) and after (one more warp behind the last write-back: the true energy, not the
 *                   linearised one), E_reg = sum_e alpha_e |g_e|^2 (Huber: psi) before and after.
 * lambda_rot damps rotations that few or badly placed points determine.  point_weights_dev, edge_weights_dev, dq_out_dev: as in
 * dfusion_warp_solve_robust.  canonical_dev and normals_dev are the UNWARPED model points and normals.  Restated in
 * tests/solver_rigid_ref.py.
 * DF_E_INVALID: what dfusion_warp_solve_robust refuses, lambda_rot negative or NaN.                                                       */
int dfusion_warp_solve_rigid(DfWarpField *wf, int k, const float *canonical_dev, const float *live_dev, const float *normals_dev, int N,
                             int iters, float lambda, float lambda_rot, int kg, float lambda_reg, int rounds, float tukey_c,
                             float huber_delta, float *dq_out_dev, float *energy_dev, float *point_weights_dev, float *edge_weights_dev,
                             dfStream stream);
/* The node graph dfusion_warp_solve uses for `kg` (1..7, M >= kg + 1; built now if the handle does not hold it):
 * nbr_dev[M*kg] int32 the head node of every edge, alpha_dev[M*kg] (nullable) the edge weights.                                      */
int dfusion_warp_node_graph(DfWarpField *wf, int kg, int *nbr_dev, float *alpha_dev, dfStream stream);
/* The HIERARCHICAL node graph (DynamicFusion section 3.3 eq. 8 and section 3.4: the regularisation graph is a hierarchy of nodes, level
 * l + 1 a coarser subsampling of level l, edges from a node to its nearest nodes one level up) -- additions to ABI 7.  A setting of the
 * handle, off (levels = 0) on every new handle; with it on, the four regularised solves and dfusion_warp_node_graph use this graph in
 * place of the flat one, in the same layout (kg outgoing edges a node, e = i * kg + s):
 *   levels    S_0 = every node.  S_l is made from S_{l-1} by dfusion_warp_extend's decimation with cell edge c_l, c_1 = radius,
 *             c_{l+1} = f32(c_l * beta): the cell of p is floorf(p / c_l) per axis (IEEE f32 division); a node with a non-finite
 *             coordinate or |p / c_l| >= 2^30 on an axis is never a member; the lowest node index of a cell is.  A c_l that overflows to
 *             infinity leaves level l and all above it empty.
 *   depth     L' = the largest l <= levels with |S_l| >= kg + 1;  top(i) = the highest l <= L' with i in S_l.
 *   edges     node i's kg targets are the nearest members of S_t \ {i}, t = min(top(i) + 1, L'), by (d2, node index) ascending,
 *             d2 = (dx dx + dy dy) + dz dz in f32 (query minus candidate, no contraction), a NaN d2 after every finite one;
 *             alpha_e = max(dg_w_i, dg_w_j).
 * L' = 0 (few nodes, or all in one cell): the flat graph, bit for bit.  The setting outlives the graph: dfusion_warp_set_nodes and a
 * dfusion_warp_extend that adds nodes drop the graph, and the next solve builds the hierarchy of the new node set.  Restated in
 * tests/solver_hier_ref.py.
 *   levels  0..8 (0 = off; radius and beta are then stored and not looked at)   radius  finite, > 0   beta  finite, >= 1
 * The call stores the three values and drops the graph.  DF_E_INVALID (the handle stays as it was): anything outside these ranges.    */
int dfusion_warp_set_graph_hierarchy(DfWarpField *wf, int levels, float radius, float beta);
/* The levels behind the graph the handle's setting selects for `kg` (1..7, M >= kg + 1; built now if the handle does not hold it).  Every
 * pointer may be NULL:  top_dev[M] int32 top(i);  sizes_dev[9] int32 |S_0| .. |S_8|, 0 past `levels`;  effective_dev[1] int32 L'
 * (0: the graph is the flat one).  With the hierarchy off: top = 0, sizes = {M, 0, ...}, L' = 0.                                       */
int dfusion_warp_graph_levels(DfWarpField *wf, int kg, int *top_dev, int *sizes_dev, int *effective_dev, dfStream stream);
/* The preconditioner of dfusion_warp_solve_rigid's conjugate gradients -- additions to ABI 7.  A setting of the handle, 0 on every new
 * handle, kept through dfusion_warp_extend, dfusion_warp_set_nodes and dfusion_warp_set_transforms; no other entry point reads it.
 *   mode 0  none: the launches and the bits of before.
 *   mode 1  6x6 node blocks (block Jacobi).  Every round the diagonal block of each node's six unknowns (omega_n, tau_n) of the round's
 *           normal matrix -- the data term with the round's Tukey weights, the graph term with its Huber-scaled edge weights, lambda_rot
 *           and lambda -- is summed in a fixed order and factored by Cholesky in f32 (one launch a round); the recurrence is
 *           preconditioned with them, z = B^-1 r by two triangular substitutions per node inside the step kernel (no launch more per
 *           step), and stops once r.z <= 1e-10 (r.z)_0.  A node whose block has a pivot that is not > 0 or not finite (no entries and no
 *           edges under zero damping, a NaN) takes the identity.  Restated in tests/solver_precond_ref.py; DESIGN.md 21.
 * DF_E_INVALID: a NULL handle (or mode_out), a mode other than 0 or 1 (the handle stays as it was).                                 */
int dfusion_warp_set_preconditioner(DfWarpField *wf, int mode);
int dfusion_warp_preconditioner(const DfWarpField *wf, int *mode_out);

/* The north-star kernel: per-voxel DQB (WarpField::DQB, warp_field.cpp:203-217) composed with
 * TsdfIntegrator (tsdf_volume.cu:77-104): x_c = vol2world*voxel, x_w = DQB(x_c).transform(x_c),
 * vc = world2cam*x_w, then the projective update.  Requires dfusion_warp_build_index.         */
int dfusion_integrate_warped(const uint16_t *dists_dev, size_t dists_pitch, int cols, int rows, DfVolume v,
                             const DfSlab *slab, const float vol2world[12], const float world2cam[12],
                             const float proj[4], DfWarpField *wf, int k, unsigned flags,
                             unsigned long long *n_updated_dev, dfStream stream);

/* The same frame in TWO calls (ABI 5), for hosts that pipeline frames: everything of the warped integrate that does not touch the volume --
 * the dists max-pyramid, the per-block verdict pass, on-demand table / model builds, the launch plan: ~70 us of small kernels at the
 * headline size -- and the sweep.  `prepare` (and the dfusion_warp_set_transforms before it) may be issued on another stream than `sweep` and
 * then runs BESIDE the previous frame's sweep and ray-cast: what a sweep reads of the handle -- the node transform arrays, the launch plan --
 * is double-buffered, and the handle orders the rest itself (a sweep waits for its prepare on the device; set_transforms / prepare wait
 * for the sweep TWO frames back, whose buffers they reuse).  The caller owns the dists image: give consecutive frames different buffers.
 * All sweeps of a handle go on ONE stream; every other call on the handle must still be ordered by the caller, and a handle is driven
 * either through these two calls or through dfusion_integrate_warped on one stream (mixing them is safe only on that one stream).
 * Results are those of dfusion_integrate_warped, bit for bit.  Only the cached path has a plan to
 * prepare: DF_E_INVALID without the per-voxel weight tables, with DF_WARP_NO_PIPELINE / NO_LDS / NO_TABLE, or k other than 4 / 8.
 * geometry.data is not dereferenced by prepare (may be NULL); sweep wants the same dims / voxel size / slab.  A prepared plan is void
 * -- its sweep call returns DF_E_INVALID -- after any other integrate on the handle, after dfusion_warp_set_nodes or
 * dfusion_warp_build_index (they free or re-make what the plan points at), and after a SECOND dfusion_warp_set_transforms since the
 * prepare (the first writes the alternate node set; the second would rewrite the one the plan reads).                                 */
int dfusion_integrate_warped_prepare(const uint16_t *dists_dev, size_t dists_pitch, int cols, int rows, DfVolume geometry,
                                     const DfSlab *slab, const float vol2world[12], const float world2cam[12], const float proj[4],
                                     DfWarpField *wf, int k, unsigned flags, dfStream stream);
int dfusion_integrate_warped_sweep(DfVolume v, const DfSlab *slab, DfWarpField *wf, unsigned long long *n_updated_dev, dfStream stream);


/* ---- depth front-end + projective ICP -----------------------------------------------------
 * All images are pitched device memory: depth u16 mm, points / normals float4.  `intr` = {fx, fy, cx, cy} of the
 * pyramid LEVEL the images belong to (Intr::operator()(level) / setLevelIntr divide by 2^level).
 * The reference's __expf (bilateral weight) and rsqrt (normalisation) are hardware approximations; this library uses
 * (float)exp((double)x) and 1/sqrtf -- see oracle/dfusion_frontend_oracle.c.                                          */

/* device::bilateralFilter (internal.hpp:128; kfusion/src/cuda/imgproc.cu:11-59).  sigma_depth in metres. src != dst. */
int dfusion_bilateral_filter(const uint16_t *src_dev, size_t src_pitch, uint16_t *dst_dev, size_t dst_pitch, int cols, int rows,
                             int kernel_size, float sigma_spatial, float sigma_depth, dfStream stream);
/* device::truncateDepth (internal.hpp:127; imgproc.cu:66-85): depth > max_dist (metres) <- 0, in place.            */
int dfusion_truncate_depth(uint16_t *depth_dev, size_t pitch, int cols, int rows, float max_dist, dfStream stream);
/* device::cloud_to_depth (internal.hpp:125; imgproc.cu:273-282, 296-303), behind cuda::cloudToDepth (imgproc.cpp:98-103): depth (mm) =
 * points.z (metres) * 1000, float -> ushort toward zero and saturating, NaN (a ray-cast miss) -> 0 (ABI 6).                          */
int dfusion_cloud_to_depth(const float *points_dev, size_t points_pitch, uint16_t *depth_dev, size_t depth_pitch, int cols, int rows, dfStream stream);
/* device::depthPyr (internal.hpp:129; imgproc.cu:94-137): dst is (src_rows/2) x (src_cols/2).                       */
int dfusion_depth_pyramid(const uint16_t *src_dev, size_t src_pitch, int src_cols, int src_rows, uint16_t *dst_dev, size_t dst_pitch,
                          float sigma_depth, dfStream stream);
/* device::computeNormalsAndMaskDepth (internal.hpp:134; imgproc.cu:145-201): normals (x,y,z,0) or (qnan,qnan,qnan,0);
 * depth pixels without a normal are zeroed in place.                                                                 */
int dfusion_compute_normals_mask_depth(uint16_t *depth_dev, size_t depth_pitch, float *normals_dev, size_t normals_pitch, int cols,
                                       int rows, const float intr[4], dfStream stream);
/* device::computePointNormals (internal.hpp:135; imgproc.cu:210-252): invalid pixels are all-NaN in both outputs.    */
int dfusion_compute_point_normals(const uint16_t *depth_dev, size_t depth_pitch, float *points_dev, size_t points_pitch,
                                  float *normals_dev, size_t normals_pitch, int cols, int rows, const float intr[4], dfStream stream);
/* device::resizeDepthNormals / resizePointsNormals (internal.hpp:131-132; imgproc.cu:309-414): outputs are half size. */
int dfusion_resize_depth_normals(const uint16_t *depth_dev, size_t depth_pitch, const float *normals_dev, size_t normals_pitch,
                                 int src_cols, int src_rows, uint16_t *depth_out_dev, size_t depth_out_pitch, float *normals_out_dev,
                                 size_t normals_out_pitch, dfStream stream);
int dfusion_resize_points_normals(const float *points_dev, size_t points_pitch, const float *normals_dev, size_t normals_pitch,
                                  int src_cols, int src_rows, float *points_out_dev, size_t points_out_pitch, float *normals_out_dev,
                                  size_t normals_out_pitch, dfStream stream);

/* device::renderImage (Points and Depth variants) and renderTangentColors (internal.hpp:134-136; kernels imgproc.cu:420-583): the
 * Phong view KinFu::renderImage produces (kinfu.cpp:312-343,408-436).  image: cols x rows BGRA bytes (device), light_pose in metres
 * (KinFuParams::light_pose), intr = (fx, fy, cx, cy) of the depth image (the Points variant shades the points as given).             */
int dfusion_render_image_points(const float *points_dev, size_t points_pitch, const float *normals_dev, size_t normals_pitch, int cols,
                                int rows, const float light_pose[3], unsigned char *image_dev, size_t image_pitch, dfStream stream);
int dfusion_render_image_depth(const uint16_t *depth_dev, size_t depth_pitch, const float *normals_dev, size_t normals_pitch, int cols,
                               int rows, const float intr[4], const float light_pose[3], unsigned char *image_dev, size_t image_pitch,
                               dfStream stream);
int dfusion_render_tangent_colors(const float *normals_dev, size_t normals_pitch, int cols, int rows, unsigned char *image_dev,
                                  size_t image_pitch, dfStream stream);

/* The host loops of KinFu::dynamicfusion (kinfu.cpp:353-383) on the device: out(y,x) = aff * in(y,x) for a rows x cols grid of
 * 3-vectors (aff nullable = plain re-striding), with cv::Affine3f * Vec3f float arithmetic (products summed left to right,
 * then + t).  Element strides in floats (input >= 3, output 3 or 4; a 4th output component is set to 0), row pitches in
 * bytes; a flat list of n points is rows = 1, cols = n.  NaN components propagate.  in != out.                        */
int dfusion_transform_points(const float *in_dev, size_t in_pitch, int in_stride, float *out_dev, size_t out_pitch, int out_stride,
                             int cols, int rows, const float aff[12], dfStream stream);

/* Projective data association for the warp solve (no reference counterpart: KinFu::dynamicfusion pairs ray-cast point i with live
 * point i; additive, ABI 7).  Every predicted point p (packed float3 [N], in the camera frame of the live image, e.g. the warped
 * ray-cast points) with its normal n (nullable, together with live_normals_dev) is paired with the sample of the live points image
 * (float4, byte pitch) at the pixel it projects to, visible surface only.  intr = {fx, fy, cx, cy} of that image.  Arithmetic is f32
 * without contraction; the FIRST failing test names the point's status:
 *   1 invalid   a component of p (with normals: or of n) is not finite
 *   2 behind    !(p.z > 0)
 *   3 outside   u = fmaf(fx, p.x / p.z, cx), v = fmaf(fy, p.y / p.z, cy) (the ICP's projection, dfusion_icp_sums_points); rejected unless
 *               u >= 0 && v >= 0 && u < (float)cols && v < (float)rows.  The pixel is (ui, vi) = ((int)u, (int)v)
 *   4 occluded  zmin = the smallest p.z over ALL points that passed tests 1-3 and fall on the same pixel; rejected iff
 *               occlusion_margin >= 0 and p.z - zmin > occlusion_margin (margin 0 keeps exact ties; a negative -- or NaN -- margin
 *               switches the test off)
 *   5 hole      q = live_points(vi, ui); rejected iff isnan(q.x) (the ICP's rule)
 *   6 far       d = p - q; rejected iff dot(d, d) > dist_thres * dist_thres, dot(a, b) = fmaf(a.x, b.x, fmaf(a.y, b.y, a.z * b.z))
 *               (equality is kept)
 *   7 normal    with normals only: rejected unless fabsf(dot(n, live_normals(vi, ui))) >= min_cosine (a NaN live normal rejects,
 *               equality is kept)
 *   0 paired    live_out[i] = (q.x, q.y, q.z)
 * On any rejection all three words of live_out[i] are 0x7fffffff: dfusion_warp_solve* skip such pairs.  status_dev (nullable) [N]
 * receives the statuses, counts_dev (nullable) [8] is OVERWRITTEN with the number of points per status (they sum to N).
 * DF_E_INVALID: N < 0, cols <= 0, rows <= 0, exactly one of the two normal pointers NULL, a pitch < 16 * cols, dist_thres negative or
 * NaN, min_cosine NaN, intr NULL, and -- for N > 0 -- points_dev, live_points_dev or live_out_dev NULL.  N == 0 enqueues nothing but
 * the zeroing of counts_dev.  Three short launches (depth-buffer fill, integer atomic-min splat, resolve; the resolve alone when the
 * occlusion test is off); the depth buffer (4 bytes per pixel) lives in the per-(device, stream) scratch dfusion_integrate uses, so
 * dfusion_release_scratch() frees it.  No float atomics: the output does not depend on scheduling.                                   */
int dfusion_associate_projective(const float *points_dev, const float *normals_dev, int N, const float *live_points_dev,
                                 size_t live_points_pitch, const float *live_normals_dev, size_t live_normals_pitch, int cols, int rows,
                                 const float intr[4], float dist_thres, float min_cosine, float occlusion_margin, float *live_out_dev,
                                 unsigned char *status_dev, unsigned long long *counts_dev, dfStream stream);

/* A z-buffered rasteriser: the vertex map, normal map, colour image and an interpolated per-vertex attribute of a triangle mesh seen by a
 * pinhole camera (no reference counterpart; additive, ABI 7).  Every output point lies on its pixel's ray, so pairing it by pixel index
 * with a depth frame IS projective association.  vertices_dev float4 [V] (dfusion_extract_mesh / dfusion_warp_points), triangles_dev
 * u32 [3 T], world2cam (nullable: vertices as given) 12 floats, per-vertex normals_dev float4 [V], attr_dev float4 [V] (interpolated
 * plainly, e.g. the canonical positions), colors_dev 4 bytes [V] -- each nullable; intr = {fx, fy, cx, cy}; max_extent 1..64 pixels.
 * Arithmetic is f32 without contraction; the sample point of pixel (x, y) is its integer coordinate (the ray of the ray-cast).
 *   vertex     pc = aff_mul(world2cam, v); u = fmaf(fx, pc.x / pc.z, cx), v = fmaf(fy, pc.y / pc.z, cy).  Valid iff pc is finite,
 *              pc.z > 0, fabsf(u) < 65536 and fabsf(v) < 65536.  X = (int)rintf(16 u), Y = (int)rintf(16 v) (1/16 pixel, half-even),
 *              iz = 1 / pc.z
 *   triangle t = (i0, i1, i2); the FIRST failing test names its status:
 *     1 invalid     an index >= V (tested before any vertex is read) or an invalid vertex
 *     2 degenerate  area2 = (X1 - X0)(Y2 - Y0) - (X2 - X0)(Y1 - Y0), an exact integer, is 0
 *     3 stretched   maxX - minX > 16 max_extent or maxY - minY > 16 max_extent (a tear of the warp, not surface)
 *     4 off-screen  x0 = max(ceil(minX / 16), 0), x1 = min(floor(maxX / 16), cols - 1), y0, y1 alike: the box is empty
 *     0 drawn       (it may still cover no sample point)
 *   orientation  area2 < 0: vertices 1 and 2 swap, with their attributes, and area2 is negated; no back-face culling, no clipping
 *   coverage     P = (16 x, 16 y); w0 = (X2 - X1)(Py - Y1) - (Y2 - Y1)(Px - X1), w1 of vertices (2, 0), w2 of (0, 1); covered iff
 *                w0 >= 0 && w1 >= 0 && w2 >= 0 (inclusive, no fill rule: shared edges are drawn twice); w0 + w1 + w2 == area2
 *   depth        b_i = (float)w_i / (float)area2; iz = (b0 iz0 + b1 iz1) + b2 iz2; z = 1 / iz; dropped unless z > 0 and finite; else a
 *                64-bit integer atomic min of (bits(z) << 32) | t at the pixel: the nearest sample wins, an exact tie in z goes to the
 *                lower triangle index
 *   resolve      an untouched pixel is a miss: the float4 outputs get four 0x7fffffff words (what dfusion_raycast_points writes), the
 *                colour four 0 bytes, tri_out -1.  Else, with c_i = (b_i iz_i) z:
 *                  point  = (((float)x - cx) / fx * z, ((float)y - cy) / fy * z, z, 0)
 *                  attr   = (c0 a0 + c1 a1) + c2 a2 per component, w = 0
 *                  normal = m / sqrtf(l2) per component, w = 0, with m formed as attr and l2 = dot(m, m); four NaN words unless l2 > 0
 *                  colour = min(255, (int)floorf(((c0 k0 + c1 k1) + c2 k2) + 0.5f)) per channel, the 4th byte 255
 *                  tri    = t
 * All outputs are pitched images (byte pitches; float4 16-byte, colour and tri 4-byte aligned); all but points_out are nullable.
 * counts_dev (nullable) u64 [6] is OVERWRITTEN: [0..4] triangles per status, [5] covered pixels.  T == 0 or V == 0 draws nothing: all
 * misses, zero counts.  DF_E_INVALID: vertices_dev NULL with V > 0, triangles_dev NULL with T > 0, V or T > 2^32 - 1, intr or
 * points_out NULL, cols <= 0, rows <= 0, a pitch shorter than a row or misaligned, max_extent outside 1..64, a non-finite intr,
 * fx == 0 or fy == 0, and -- with V, T > 0 -- an output image whose per-vertex input is NULL.  Three launches (key fill, raster with
 * one lane per triangle, resolve with one lane per pixel); the key buffer (8 bytes per pixel) lives in the per-(device, stream)
 * scratch dfusion_integrate uses, so dfusion_release_scratch() frees it.  No float atomics, no device-to-host copy: the output does
 * not depend on scheduling.                                                                                                          */
int dfusion_render_mesh(const float *vertices_dev, unsigned long long V, const unsigned int *triangles_dev, unsigned long long T,
                        const float world2cam[12], const float *normals_dev, const float *attr_dev, const unsigned char *colors_dev,
                        int cols, int rows, const float intr[4], int max_extent, float *points_out, size_t points_pitch,
                        float *normals_out, size_t normals_pitch, float *attr_out, size_t attr_pitch, unsigned char *colors_out,
                        size_t colors_pitch, int *tri_out, size_t tri_pitch, unsigned long long *counts_dev, dfStream stream);

/* device::ComputeIcpHelper::operator() (internal.hpp:91-92; kfusion/src/cuda/proj_icp.cu:30-441): one Gauss-Newton
 * accumulation of point-to-plane ICP.  aff = current estimate curr -> prev; dist2_thres = dist_thres^2 and
 * min_cosine = cos(angle_thres) (projective_icp.cpp:11-15).  sums_dev[27] = the upper triangle of A (6x6) interleaved
 * with b exactly as StreamHelper::get unpacks it (projective_icp.cpp:43-61): for i in 0..5, for j in i..6.
 * The float sums are taken over the reference's reduction tree (32x8-pixel blocks, strides 128..1, then 256 strided
 * partial sums), so they are reproducible bit for bit.  workspace_dev: dfusion_icp_workspace_floats(cols, rows) floats
 * (ComputeIcpHelper::allocate_buffer, proj_icp.cu:446-464).  accepted_dev (nullable) is INCREMENTED by the number of
 * accepted correspondences.  The 6x6 solve stays on the host (cv::solve in the reference).                           */
int dfusion_icp_workspace_floats(int cols, int rows);
int dfusion_icp_sums_points(const float *vcurr_dev, size_t vcurr_pitch, const float *ncurr_dev, size_t ncurr_pitch,
                            const float *vprev_dev, size_t vprev_pitch, const float *nprev_dev, size_t nprev_pitch, int cols, int rows,
                            const float aff[12], const float intr[4], float dist2_thres, float min_cosine, float *workspace_dev,
                            float *sums_dev, int *accepted_dev, dfStream stream);
int dfusion_icp_sums_depth(const uint16_t *dcurr_dev, size_t dcurr_pitch, const float *ncurr_dev, size_t ncurr_pitch,
                           const uint16_t *dprev_dev, size_t dprev_pitch, const float *nprev_dev, size_t nprev_pitch, int cols, int rows,
                           const float aff[12], const float intr[4], float dist2_thres, float min_cosine, float *workspace_dev,
                           float *sums_dev, int *accepted_dev, dfStream stream);

/* ProjectiveICP::estimateTransform (projective_icp.cpp:129-213) as ONE enqueue: for every pyramid level from the coarsest,
 * `iters` times { correspondences + 27 sums (as dfusion_icp_sums_*), 6x6 solve, Tinc * estimate } with the estimate kept in
 * device memory -- no host round trip per iteration (the reference synchronises a stream and solves on the host each time).
 *   levels[l]     images of pyramid level l (curr / prev are float4 points, or u16 depth when depth_variant != 0)
 *   intr          level-0 intrinsics {fx, fy, cx, cy}; level l uses intr / 2^l (setLevelIntr)
 *   workspace_dev dfusion_icp_workspace_floats(level-0 cols, rows) + 27 floats
 *   state_dev     13 floats out: curr -> prev estimate {R[9] row-major, t[3]} and ok (1, or 0 once a normal matrix was singular:
 *                 |det| < 1e-15 or NaN -- estimateTransform returns false there)
 * The 6x6 solve is LU with partial pivoting in double (cv::solve DECOMP_SVD in the reference; OpenCV is not in its tree).    */
typedef struct DfIcpLevel {
    const void *curr; size_t curr_pitch; const float *ncurr; size_t ncurr_pitch;
    const void *prev; size_t prev_pitch; const float *nprev; size_t nprev_pitch;
    int cols, rows, iters;
} DfIcpLevel;
int dfusion_icp_estimate(const DfIcpLevel *levels, int n_levels, int depth_variant, const float intr[4], float dist2_thres,
                         float min_cosine, float *workspace_dev, float *state_dev, dfStream stream);

/* ---- measurement helper: plain device copy used as the MEASURED HBM roofline denominator ---- */
int dfusion_copy_bandwidth_probe(void *dst_dev, const void *src_dev, size_t bytes, dfStream stream);
/* read-only stream of `bytes` (sink4_dev: 4 writable device bytes): the measured denominator for scan kernels */
int dfusion_read_bandwidth_probe(const void *src_dev, size_t bytes, void *sink4_dev, dfStream stream);

#ifdef __cplusplus
}
#endif
#endif /* DFUSION_H */
