// color_frame.cpp -- a few RGB-D frames through kfusion::KinFu with KinFuParams::integrate_color, and everything a test needs to repeat
// the colour fusion through the Python mirror: per frame the pose, the warp nodes and the TSDF volume the colour was fused on; at the
// end the colour volume and the vertex colours of fetchMesh (tests/test_gpu_cxx_color.py).
//   color_frame <cols> <rows> <frames> <dims> <size_m> <in.bin> <out.bin> [color|warped|nosolver, '-' separated]
//   (color: KinFuParams::integrate_color; warped: per-voxel warped integrate, and the colour through the warp field; nosolver: skip the
//   warp solve)
// in.bin : intrinsics fx fy cx cy f32[4], then per frame depth u16[rows * cols] (mm) and image u8[rows * cols * 4] (b, g, r, a).
// out.bin: i32[2] bilateral kernel size, k; f32[4] bilateral sigma_spatial, sigma_depth, icp_truncate_depth_dist, the volume's
//          trunc_dist; then per frame { tracked i32, pose f32[12], warp_to_live f32[12], M i32, node positions f32[3 M], transforms
//          f32[8 M], dg_w f32[M], colour counts u64[2] (selected, fused; zeros without colour), volume u32[dims^3] }; then colour i32
//          (1: a colour volume follows), colour volume u8[4 dims^3], vertices nv u64, f32[4 nv], vertex colours u8[4 nv] (b, g, r, 255).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include <kfusion/kinfu.hpp>
#include <kfusion/cuda/imgproc.hpp>

using namespace kfusion;

int main(int argc, char** argv)
{
    if (argc != 8 && argc != 9) { std::fprintf(stderr, "usage: %s cols rows frames dims size in.bin out.bin [color|warped|nosolver, '-' separated]\n", argv[0]); return 2; }
    const int cols = std::atoi(argv[1]), rows = std::atoi(argv[2]), frames = std::atoi(argv[3]), dims = std::atoi(argv[4]);
    const float size = (float)std::atof(argv[5]);
    FILE* in = std::fopen(argv[6], "rb");
    if (!in) { std::perror("in"); return 2; }
    float iv[4];
    if (std::fread(iv, 4, 4, in) != 4) return 2;

    KinFuParams p = KinFuParams::default_params_dynamicfusion();
    p.cols = cols; p.rows = rows;
    p.intr = Intr(iv[0], iv[1], iv[2], iv[3]);
    p.volume_dims = Vec3i::all(dims);
    p.volume_size = Vec3f::all(size);
    p.volume_pose = Affine3f().translate(Vec3f(-size / 2, -size / 2, 0.5f));
    const std::string mode = argc == 9 ? argv[8] : "";
    p.integrate_color = mode.find("color") != std::string::npos;
    p.warped_fusion = mode.find("warped") != std::string::npos;
    if (mode.find("nosolver") != std::string::npos) p.warp_solver_iterations = 0;
    KinFu kinfu(p);

    FILE* out = std::fopen(argv[7], "wb");
    if (!out) { std::perror("out"); return 2; }
    const int hi[2] = {p.bilateral_kernel_size, kinfu.getWarp().k()};
    const float hf[4] = {p.bilateral_sigma_spatial, p.bilateral_sigma_depth, p.icp_truncate_depth_dist, kinfu.tsdf().getTruncDist()};
    std::fwrite(hi, 4, 2, out);
    std::fwrite(hf, 4, 4, out);
    std::vector<unsigned short> depth((size_t)rows * cols);
    std::vector<unsigned char> image((size_t)rows * cols * 4);
    std::vector<unsigned int> vol((size_t)dims * dims * dims);
    cuda::Depth depth_device; cuda::Image image_device;
    for (int f = 0; f < frames; ++f) {
        if (std::fread(depth.data(), 2, depth.size(), in) != depth.size() || std::fread(image.data(), 1, image.size(), in) != image.size()) return 2;
        depth_device.upload(depth.data(), (size_t)cols * 2, rows, cols);
        image_device.upload(image.data(), (size_t)cols * 4, rows, cols);
        const int tracked = kinfu(depth_device, image_device) ? 1 : 0;
        cuda::waitAllDefaultStream();
        float pose[12], w2l[12];
        affine_to_aff12(kinfu.getCameraPose(), pose);
        affine_to_aff12(kinfu.getWarp().getWarpToLive(), w2l);
        const std::vector<deformation_node>& nodes = *kinfu.getWarp().getNodes();
        const int M = (int)nodes.size();
        std::vector<float> pos(3 * (size_t)M), dq(8 * (size_t)M), sigma((size_t)M);
        for (int i = 0; i < M; ++i) {
            for (int c = 0; c < 3; ++c) pos[3 * i + c] = nodes[i].vertex[c];
            for (int c = 0; c < 8; ++c) dq[8 * i + c] = nodes[i].transform.raw()[c];
            sigma[i] = nodes[i].weight;
        }
        unsigned long long counts[2] = {0, 0};
        if (p.integrate_color) kinfu.colorVolume().counts().download(counts);
        kinfu.tsdf().data().download(vol.data());
        std::fwrite(&tracked, 4, 1, out);
        std::fwrite(pose, 4, 12, out);
        std::fwrite(w2l, 4, 12, out);
        std::fwrite(&M, 4, 1, out);
        std::fwrite(pos.data(), 4, pos.size(), out);
        std::fwrite(dq.data(), 4, dq.size(), out);
        std::fwrite(sigma.data(), 4, sigma.size(), out);
        std::fwrite(counts, 8, 2, out);
        std::fwrite(vol.data(), 4, vol.size(), out);
    }
    std::fclose(in);
    const int has_color = p.integrate_color ? 1 : 0;
    std::fwrite(&has_color, 4, 1, out);
    unsigned long long nv = 0;
    if (has_color) {
        std::vector<unsigned char> bytes;
        kinfu.colorVolume().download(bytes);
        std::fwrite(bytes.data(), 1, bytes.size(), out);
        cuda::DeviceArray<Point> vertices; cuda::DeviceArray<int> triangles; cuda::DeviceArray<cuda::RGB> colors;
        kinfu.tsdf().fetchMesh(vertices, triangles);
        kinfu.colorVolume().fetchColors(vertices, colors);
        cuda::waitAllDefaultStream();
        nv = vertices.size();
        std::vector<Point> vh; std::vector<cuda::RGB> ch;
        vertices.download(vh); colors.download(ch);
        std::fwrite(&nv, 8, 1, out);
        std::fwrite(vh.data(), sizeof(Point), vh.size(), out);
        std::fwrite(ch.data(), sizeof(cuda::RGB), ch.size(), out);
    }
    std::fclose(out);
    std::printf("color_frame ok: %d frames, %zu warp nodes, colour %s, %llu coloured vertices\n", frames, kinfu.getWarp().getNodes()->size(),
                has_color ? "on" : "off", nv);
    return 0;
}
