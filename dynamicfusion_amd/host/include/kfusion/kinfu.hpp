// kfusion/kinfu.hpp -- kfusion::KinFuParams / kfusion::KinFu with the reference's interface
// (/root/reference/kfusion/include/kfusion/kinfu.hpp:15-112) minus the Opt/Ceres solver (the data term is solved on the GPU instead).
// Extensions: max_warp_nodes (node ids are 16-bit here; the seed cloud's stride-50 sampling, warp_field.cpp:49-60, widens if needed),
// warped_fusion (call the per-voxel warped integrate instead of surface_fusion; default off = the reference's behaviour) and
// device_resident (default on: same results as the reference's host staging, bit for bit, without the ~50 MB/frame of PCIe traffic;
// switch off when optimiseWarp is overridden, which needs the host vectors).
#pragma once
#include <array>
#include <memory>
#include <vector>
#include <kfusion/types.hpp>
#include <kfusion/cuda/projective_icp.hpp>
#include <kfusion/cuda/tsdf_volume.hpp>
#include <kfusion/cuda/color_volume.hpp>
#include <kfusion/cuda/render_mesh.hpp>
#include <kfusion/warp_field.hpp>

namespace kfusion
{
    // The knobs of the pipeline, field for field those of the reference's KinFuParams (kinfu.hpp:15-48), followed by the extensions
    // of this implementation.  Units: pixels, metres, radians, frames.
    struct KinFuParams
    {
        static KinFuParams default_params();                   // 512^3 / 3 m volume, fx = fy = 525                    kinfu.cpp:55-89
        static KinFuParams default_params_dynamicfusion();     // 256^3 / 1 m volume, fx = fy = 570.342 (what demo.cpp uses)  :15-50

        // sensor
        int cols, rows;
        Intr intr;
        // TSDF volume
        Vec3i volume_dims;                   // voxels per axis (dims[0] % 32 == 0)
        Vec3f volume_size;                   // metres per axis
        Affine3f volume_pose;                // volume -> world
        float tsdf_trunc_dist;               // clamped to >= 2.1 voxels by TsdfVolume::setTruncDist
        int tsdf_max_weight;
        float tsdf_min_camera_movement;      // unused by the pipeline, as in the reference
        float raycast_step_factor, gradient_delta_factor;      // in voxel sizes
        // depth front-end
        float bilateral_sigma_depth, bilateral_sigma_spatial;
        int bilateral_kernel_size;
        float icp_truncate_depth_dist;       // 0 = no truncation
        // tracker
        float icp_dist_thres, icp_angle_thres;
        std::vector<int> icp_iter_num;       // per pyramid level, finest first
        Vec3f light_pose;                    // metres, camera frame: renderImage's light

        // ---- extensions (defaults reproduce the reference's observable behaviour unless noted)
        int max_warp_nodes = 65535;          // node ids are 16-bit: the stride-50 sampling of the seed cloud widens if it must
        bool warped_fusion = false;          // true: per-voxel warped integrate (the north-star kernel) instead of surface_fusion
        bool use_depth_pyramids = false;     // the reference's USE_DEPTH build (internal.hpp:6): depth pyramids + masked-depth ICP
        bool device_resident = true;         // dynamicfusion() keeps its point sets on the GPU; false = the reference's host staging
        int warp_solver_iterations = 40;     // CG steps of the warp data term per frame, 0 = off (Opt's cap is linearIter = 100,
                                             // kinfu.cpp:118; the synthetic sequence has converged to 4 digits by 40)
        int warp_reg_neighbours = 0;         // regularisation of the warp solve (WarpField::setRegularisation): graph neighbours per node,
        float warp_reg_lambda = 0.f;         // and the term's weight; 0 = off, the data term alone as in the reference
        int warp_reg_levels = 0;             // the term over the paper's node hierarchy (WarpField::setRegularisationHierarchy): levels, 0 = the
        float warp_reg_radius = 0.05f;       // flat graph; the cell edge of level 1 (metres: twice the seed nodes' spacing is a start) and
        float warp_reg_beta = 4.f;           // its growth from a level to the next
        int warp_robust_rounds = 1;          // robust warp solve (WarpField::setRobust): re-weighted rounds per frame,
        float warp_tukey_c = 0.f;            // the Tukey threshold of the point residuals (metres; 0 = quadratic data term)
        float warp_huber_delta = 0.f;        // and the Huber threshold of the graph edges (0 = quadratic regularisation); default: off
        bool warp_point_to_plane = false;    // device-resident dynamicfusion(): the warp solve's data term along the warped model normals
                                             // (WarpField::setPointToPlane) instead of point-to-point; default off = the reference's energy
        bool warp_solve_rotations = false;   // device-resident dynamicfusion(): the node ROTATIONS are unknowns of the warp solve too
        float warp_rot_lambda = 0.f;         // (WarpField::setNodeRotations, with this damping of the rotations); the solve then gets copies of
                                             // the canonical points and normals from before the first warp; default off = the launches of before
        bool warp_precondition = false;      // that solve's conjugate gradients preconditioned with the 6x6 node blocks
                                             // (WarpField::setPreconditioner(1)): several times fewer steps to the round's solution, one launch
                                             // more per round; default off = the plain recurrence
        bool warp_projective_association = false;   // device-resident dynamicfusion(): pair every warped point with the live sample at the
                                             // pixel it projects to (cuda::associateProjective) instead of by pixel index; default off =
                                             // the reference's pairing
        float warp_assoc_dist_thres = 0.05f; // its distance gate (metres),
        float warp_assoc_angle_thres = 0.52359878f;   // its normal gate (radians: 30 degrees, used as its cosine)
        float warp_assoc_occlusion_margin = 0.02f;    // and how far behind the nearest warped point of its pixel a point may lie (< 0: off)
        bool integrate_color = false;        // fuse operator()'s colour image into a colour volume (cuda::ColorVolume) after the frame's depth
                                             // integrate -- through the warp field when warped_fusion is on; default off = the image is
                                             // dropped, as in the reference, and no launch is added
        float color_band = 1.f;              // its band (ColorVolume::setBand)
        int color_max_weight = 64;           // and the cap of its weight byte (ColorVolume::setMaxWeight)
    };

    class KinFu
    {
    public:
#ifdef KFUSION_USE_OPENCV
        typedef cv::Ptr<KinFu> Ptr;                                         // kinfu.hpp:52
#else
        typedef std::shared_ptr<KinFu> Ptr;
#endif
        KinFu(const KinFuParams& params);
        virtual ~KinFu() {}

        const KinFuParams& params() const { return params_; }
        KinFuParams& params() { return params_; }
        const cuda::TsdfVolume& tsdf() const { return *volume_; }
        cuda::TsdfVolume& tsdf() { return *volume_; }
        const cuda::ProjectiveICP& icp() const { return *icp_; }
        cuda::ProjectiveICP& icp() { return *icp_; }
        const WarpField& getWarp() const { return *warp_; }
        WarpField& getWarp() { return *warp_; }
        /// the colour volume integrate_color fuses into (allocated on first use: 4 bytes a voxel)
        cuda::ColorVolume& colorVolume();

        void reset();
        bool operator()(const cuda::Depth& depth, const cuda::Image& image = cuda::Image());
        /// kinfu.cpp:312-343: the model as the tracker last saw it (prev_ pyramid level 0).  flags 1 (and anything outside 1..3): Phong
        /// shading, 2: normals as colours, 3: both side by side (image is then 2 * cols wide)
        void renderImage(cuda::Image& image, int flags = 0);
        void dynamicfusion(cuda::Depth& depth, cuda::Cloud live_frame, cuda::Normals current_normals);
        /// kinfu.cpp:408-436: the same views of a fresh ray-cast from `pose`
        void renderImage(cuda::Image& image, const Affine3f& pose, int flags = 0);
        /// No reference counterpart: the same views of the LIVE model -- the canonical mesh (fetchMesh, fetchNormals; the colour volume's
        /// colours if there is one) warped by the warp field and rendered into the current camera pose (cuda::renderMesh), shaded by
        /// cuda::renderImage(points, normals).  A viewer call outside the frame loop: it allocates, and changes nothing the frames use.
        /// liveModel() is what the last renderLive rendered (point, normal, canonical-point and colour images).
        void renderLive(cuda::Image& image, int flags = 0);
        const cuda::RenderMeshOutputs& liveModel() const { return live_model_; }
        Affine3f getCameraPose(int time = -1) const;
        /// the last frame's association: points per status (0 paired, 1 invalid, 2 behind, 3 outside, 4 occluded, 5 hole, 6 far,
        /// 7 normal); all zero until a frame ran with warp_projective_association.  Waits for the device.
        std::array<unsigned long long, 8> associationCounts() const;

    protected:
        /// optimiser_->optimiseWarpData(canonical, canonical_normals, live, canonical_normals) (kinfu.cpp:389) on the host-staged data
        /// flow (device_resident = false); the default runs WarpField::energy_data, the GPU data-term solve
        virtual void optimiseWarp(std::vector<Vec3f>& canonical, std::vector<Vec3f>& canonical_normals, const std::vector<Vec3f>& live);
    private:
        void allocate_buffers();
        void fuse_color(const cuda::Dists& dists, const Affine3f& camera_pose, bool warped);
        void color_dists_before_surface_fusion(const cuda::Depth& depth);
        int frame_counter_;
        KinFuParams params_;
        std::vector<Affine3f> poses_;
        cuda::Dists dists_;
        cuda::Frame curr_, prev_, first_;
        cuda::Cloud points_; cuda::Normals normals_; cuda::Depth depths_;   // renderImage(image, pose, flags)
        cuda::RenderMeshOutputs live_model_;                                // renderLive(image, flags)
        std::unique_ptr<cuda::TsdfVolume> volume_;
        std::unique_ptr<cuda::ProjectiveICP> icp_;
        std::unique_ptr<WarpField> warp_;
        std::unique_ptr<cuda::ColorVolume> color_; cuda::Dists color_dists_;
        const cuda::Image* frame_image_ = nullptr;                          // operator()'s image while the frame runs
        // scratch of the device-resident dynamicfusion()
        cuda::Cloud df_cloud_; cuda::Normals df_normals_;
        cuda::DeviceArray<float> df_points3_, df_normals3_, df_live3_, df_assoc3_, df_plane_normals3_, df_unwarped_points3_, df_unwarped_normals3_;
        cuda::DeviceArray<unsigned long long> df_assoc_counts_; bool df_assoc_valid_ = false;
        cuda::DeviceArray<Point> df_warped4_;
        cuda::Normals df_live_normals_;
    };
}
