// kinfu_headless.cpp -- apps/demo.cpp (/root/reference/apps/demo.cpp:60-110) without OpenNI capture and the viz window: feeds depth
// frames from a file to kfusion::KinFu::operator() and records what the demo would display -- the camera pose per frame.
//   kinfu_headless <cols> <rows> <frames> <dims> <size_m> <in.bin> <out.bin> [warped|host|warped-host]
//   (warped: per-voxel warped integrate instead of surface_fusion; host: the reference's host-staged data flow; nosolver: skip the
//   warp data-term solve; depth: the reference's USE_DEPTH build -- depth pyramids and masked-depth ICP; assoc: projective data
//   association in front of the warp solve, KinFuParams::warp_projective_association -- under trace its counts are printed per frame;
//   plane: the warp solve's point-to-plane data term, KinFuParams::warp_point_to_plane; rigid: the node rotations as unknowns of the warp
//   solve, KinFuParams::warp_solve_rotations with warp_rot_lambda = 1e-3 and 4 graph neighbours at weight 1; pcg (beside rigid): that solve
//   preconditioned with the node blocks, KinFuParams::warp_precondition; hier: the regularisation over
//   the node hierarchy, KinFuParams::warp_reg_levels = 3 with radius 0.05 and beta 4, and 4 graph neighbours at weight 1; renderlive: after the
//   last frame KinFu::renderLive, and what a caller needs to repeat it appended to out.bin)
// in.bin : intrinsics fx fy cx cy f32[4], then per frame depth u16[rows*cols] (mm).
// out.bin: per frame { tracked i32 (operator()'s return value), pose f32[12] (R row-major, t) }, then the extracted surface
//          count u64 and the volume u32[dims^3].  renderlive: then i32[2] M, k; per node pos f32[3], dq f32[8], dg_w f32; world2cam
//          f32[12] (the last pose, inverted); warp_to_live f32[12]; light pose f32[3]; the live model's point, normal and canonical-point
//          images f32[rows * cols * 4] each; the shaded image u8[rows * cols * 4].
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <string>
#include <vector>
#include <kfusion/kinfu.hpp>
#include <kfusion/cuda/imgproc.hpp>

using namespace kfusion;

int main(int argc, char** argv)
{
    if (argc != 8 && argc != 9) { std::fprintf(stderr, "usage: %s cols rows frames dims size in.bin out.bin [warped|host|nosolver|depth|assoc|plane|rigid|pcg|hier|trace, '-' separated]\n", argv[0]); return 2; }
    const int cols = std::atoi(argv[1]), rows = std::atoi(argv[2]), frames = std::atoi(argv[3]), dims = std::atoi(argv[4]);
    const float size = (float)std::atof(argv[5]);
    FILE* in = std::fopen(argv[6], "rb");
    if (!in) { std::perror("in"); return 2; }
    float iv[4];
    if (std::fread(iv, 4, 4, in) != 4) return 2;

    KinFuParams p = KinFuParams::default_params_dynamicfusion();        // demo.cpp:120
    p.cols = cols; p.rows = rows;
    p.intr = Intr(iv[0], iv[1], iv[2], iv[3]);
    p.volume_dims = Vec3i::all(dims);
    p.volume_size = Vec3f::all(size);
    p.volume_pose = Affine3f().translate(Vec3f(-size / 2, -size / 2, 0.5f));
    const std::string mode = argc == 9 ? argv[8] : "";
    p.warped_fusion = mode.find("warped") != std::string::npos;
    p.device_resident = mode.find("host") == std::string::npos;
    if (mode.find("nosolver") != std::string::npos) p.warp_solver_iterations = 0;
    p.use_depth_pyramids = mode.find("depth") != std::string::npos;
    p.warp_projective_association = mode.find("assoc") != std::string::npos;
    p.warp_point_to_plane = mode.find("plane") != std::string::npos;
    if (mode.find("rigid") != std::string::npos) {
        p.warp_solve_rotations = true; p.warp_rot_lambda = 1e-3f;
        p.warp_reg_neighbours = 4; p.warp_reg_lambda = 1.f;              // rotations that few points determine follow their neighbours
    }
    p.warp_precondition = mode.find("pcg") != std::string::npos;
    if (mode.find("hier") != std::string::npos) {
        p.warp_reg_neighbours = 4; p.warp_reg_lambda = 1.f;
        p.warp_reg_levels = 3; p.warp_reg_radius = 0.05f; p.warp_reg_beta = 4.f;
    }
    KinFu kinfu(p);

    FILE* out = std::fopen(argv[7], "wb");
    if (!out) { std::perror("out"); return 2; }
    std::vector<unsigned short> depth((size_t)rows * cols);
    cuda::Depth depth_device;
    double total_ms = 0.0; int timed = 0;
    for (int f = 0; f < frames; ++f) {
        if (std::fread(depth.data(), 2, depth.size(), in) != depth.size()) return 2;
        depth_device.upload(depth.data(), (size_t)cols * 2, rows, cols);    // demo.cpp:89
        const auto t0 = std::chrono::steady_clock::now();
        const int tracked = kinfu(depth_device) ? 1 : 0;                    // demo.cpp:93
        cuda::waitAllDefaultStream();
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (f >= 2) { total_ms += ms; ++timed; }
        float pose[12]; affine_to_aff12(kinfu.getCameraPose(), pose);
        if (mode.find("trace") != std::string::npos) {                      // per-frame checksums (debugging aid): volume, node transforms
            std::vector<unsigned int> v((size_t)dims * dims * dims);
            kinfu.tsdf().data().download(v.data());
            unsigned long long hv = 1469598103934665603ull, hn = hv;
            for (unsigned int w : v) { hv ^= w; hv *= 1099511628211ull; }
            for (const auto& nd : *kinfu.getWarp().getNodes()) {
                const unsigned int* r = (const unsigned int*)nd.transform.raw();
                for (int i = 0; i < 8; ++i) { hn ^= r[i]; hn *= 1099511628211ull; }
            }
            std::fprintf(stderr, "trace frame %d volume %016llx nodes %016llx pose %08x\n", f, hv, hn, *(unsigned int*)&pose[9]);
            if (p.warp_projective_association) {
                const auto c = kinfu.associationCounts();
                std::fprintf(stderr, "assoc frame %d tracked %d counts %llu %llu %llu %llu %llu %llu %llu %llu\n", f, tracked, c[0], c[1], c[2], c[3],
                             c[4], c[5], c[6], c[7]);
            }
        }
        std::fwrite(&tracked, 4, 1, out);
        std::fwrite(pose, 4, 12, out);
    }
    std::fclose(in);
    kinfu.tsdf().compute_points();
    const unsigned long long cnt = kinfu.tsdf().get_cloud_host().size();
    std::fwrite(&cnt, 8, 1, out);
    std::vector<unsigned int> vol((size_t)dims * dims * dims);
    kinfu.tsdf().data().download(vol.data());
    std::fwrite(vol.data(), 4, vol.size(), out);
    if (mode.find("renderlive") != std::string::npos) {
        cuda::Image image;
        kinfu.renderLive(image);
        cuda::waitAllDefaultStream();
        const std::vector<deformation_node>& nodes = *kinfu.getWarp().getNodes();
        const int hd[2] = {(int)nodes.size(), kinfu.getWarp().k()};
        std::fwrite(hd, 4, 2, out);
        for (const deformation_node& n : nodes) { std::fwrite(n.vertex.val, 4, 3, out); std::fwrite(n.transform.raw(), 4, 8, out); std::fwrite(&n.weight, 4, 1, out); }
        float a12[12];
        affine_to_aff12(kinfu.getCameraPose().inv(), a12); std::fwrite(a12, 4, 12, out);
        affine_to_aff12(kinfu.getWarp().getWarpToLive(), a12); std::fwrite(a12, 4, 12, out);
        std::fwrite(p.light_pose.val, 4, 3, out);
        std::vector<char> h((size_t)rows * cols * 16);
        const cuda::RenderMeshOutputs& m = kinfu.liveModel();
        m.points.download(h.data(), (size_t)cols * 16); std::fwrite(h.data(), 1, h.size(), out);
        m.normals.download(h.data(), (size_t)cols * 16); std::fwrite(h.data(), 1, h.size(), out);
        m.attr.download(h.data(), (size_t)cols * 16); std::fwrite(h.data(), 1, h.size(), out);
        image.download(h.data(), (size_t)cols * 4); std::fwrite(h.data(), 1, (size_t)rows * cols * 4, out);
    }
    std::fclose(out);
    std::printf("kinfu_headless ok: %d frames, %zu warp nodes, %llu surface points, %.3f ms/frame (KinFu::operator(), frames 2.., wall clock)\n",
                frames, kinfu.getWarp().getNodes()->size(), cnt, timed ? total_ms / timed : 0.0);
    return 0;
}
