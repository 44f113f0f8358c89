// kfusion/cuda/color_volume.hpp -- kfusion::cuda::ColorVolume: the colour of the fused surface (no reference counterpart: the
// reference's KinFu::operator() accepts a colour image and drops it).  A colour volume belongs to a TsdfVolume and has its dims,
// stored planes and pose: 4 bytes a voxel {c0, c1, c2, w}, the channels in the byte order of the images it is given (kfusion::cuda::RGB
// is b, g, r, a).  Every compute method forwards to the C-ABI of include/dfusion.h (dfusion_color_*), where the rule is stated; the
// class holds no kernels of its own.  Same methods as the Python mirror (dynamicfusion_amd/color_volume.py).
#pragma once
#include <vector>
#include <kfusion/types.hpp>

namespace kfusion {
class WarpField;
namespace cuda {

class TsdfVolume;

class ColorVolume
{
public:
    /// Allocates and clears 4 bytes per stored voxel of `volume`, which must outlive this object and keep its dims and slab (after
    /// TsdfVolume::create / setSlab make a new ColorVolume).
    explicit ColorVolume(const TsdfVolume& volume);

    void clear();
    /// voxels with |tsdf| < band (0 < band <= 1) take colour, and a voxel is observed within band * trunc_dist of the measured surface
    float getBand() const { return band_; }             void setBand(float band) { band_ = band; }
    /// cap of the weight byte (1..255): the running average forgets at this rate
    int getMaxWeight() const { return max_weight_; }    void setMaxWeight(int weight) { max_weight_ = weight; }
    /// voxels a frame can colour (lowest linear indices first); 0 = a sixteenth of the slab's own voxels, at least 65536
    long long getCapacity() const { return capacity_; } void setCapacity(long long capacity) { capacity_ = capacity; }

    /// One frame.  Call it after the frame's depth integrate: the TSDF volume is read as it is, and never written.  `dists` is the
    /// frame's dists image (cuda::computeDists), as large as `image`.  Enqueued only: nothing synchronises.
    void integrate(const Image& image, const Dists& dists, const Affine3f& camera_pose, const Intr& intr);                         // rigid
    void integrate(const Image& image, const Dists& dists, const Affine3f& camera_pose, const Intr& intr, const WarpField& warp);  // per-voxel DQB warp first
    /// device counters of the last integrate: [0] voxels selected (> capacity: the highest indices were left out), [1] voxels fused
    const DeviceArray<unsigned long long>& counts() const { return counts_; }

    /// colours of points (fetchCloud / fetchMesh vertices, world frame): the three channels and 255, or four zeros where no coloured
    /// voxel surrounds the point
    void fetchColors(const DeviceArray<Point>& points, DeviceArray<RGB>& colors) const;
    /// the stored planes, 4 bytes a voxel, x fastest
    void download(std::vector<unsigned char>& bytes) const;
    const CudaData data() const { return data_; }

private:
    void integrate_impl(const Image& image, const Dists& dists, const Affine3f& camera_pose, const Intr& intr, const WarpField* warp);
    const TsdfVolume* volume_;
    CudaData data_;
    DeviceArray<unsigned long long> counts_;
    float band_ = 1.f;
    int max_weight_ = 64;
    long long capacity_ = 0;
};

} }
