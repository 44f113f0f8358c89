// kfusion/cuda/render_mesh.hpp -- kfusion::cuda::renderMesh: a z-buffered rasteriser of a triangle mesh into a pinhole camera (no
// reference counterpart: the reference shows the ray-cast of the canonical volume only).  Forwards to dfusion_render_mesh of
// include/dfusion.h, where the rule is stated; no kernels of its own.  Same call as the Python mirror (frontend.renderMesh).
#pragma once
#include <kfusion/types.hpp>

namespace kfusion { namespace cuda {

/// Per-vertex inputs and the images wanted of them.  An EMPTY input array switches its image off; `tri` / `counts` are made when the
/// pointer is set (tri: the winning triangle of every pixel, -1 = miss; counts: triangles drawn / invalid / degenerate / stretched /
/// off-screen, then covered pixels).  Images are created rows x cols; a miss is four NaN words (0x7fffffff) / four 0 bytes.
struct RenderMeshOutputs
{
    Cloud points;                      // camera frame, on the pixel's ray (always made)
    Normals normals;                   // interpolated and normalised, in the frame the input normals are in
    Cloud attr;                        // interpolated plainly (e.g. the canonical positions)
    Image colors;
    DeviceArray2D<int>* tri = nullptr;
    DeviceArray<unsigned long long>* counts = nullptr;
};

/// vertices / triangles as TsdfVolume::fetchMesh returns them (the vertices possibly warped since); world2cam = nullptr: the vertices are
/// in the camera frame.  max_extent (1..64 pixels): triangles wider or taller on the screen are tears of the warp and not drawn.
/// Enqueued only: nothing synchronises.
void renderMesh(const Intr& intr, const DeviceArray<Point>& vertices, const DeviceArray<int>& triangles, int cols, int rows,
                const Affine3f* world2cam, const DeviceArray<Normal>& normals, const DeviceArray<Point>& attr, const DeviceArray<RGB>& colors,
                RenderMeshOutputs& out, int max_extent = 16);

} }
