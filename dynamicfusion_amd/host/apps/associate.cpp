// associate.cpp -- one projective data association through the C++ mirror (kfusion::cuda::associateProjective over
// dfusion_associate_projective), inputs from a file, outputs to a file, so that tests/test_gpu_cxx_associate.py can compare the bits
// with the numpy restatement.
//   associate <in.bin> <out.bin>
// in.bin : i32[4] N, cols, rows, with_normals; f32[7] fx, fy, cx, cy, dist_thres, min_cosine, occlusion_margin; points f32[3 N];
//          normals f32[3 N] (with_normals); live points f32[rows * cols * 4]; live normals f32[rows * cols * 4] (with_normals).
// out.bin: live f32[3 N], status u8[N], counts u64[8].
#include <cstdio>
#include <vector>
#include <kfusion/cuda/imgproc.hpp>

using namespace kfusion;

template <class T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::perror("in"); return 2; }
    int hd[4]; float fv[7];
    if (std::fread(hd, 4, 4, in) != 4 || std::fread(fv, 4, 7, in) != 7) return 2;
    const int N = hd[0], cols = hd[1], rows = hd[2]; const bool with_normals = hd[3] != 0;
    if (N < 0 || cols <= 0 || rows <= 0) return 2;
    std::vector<float> pts, nrm, lp, ln;
    const size_t px = (size_t)rows * cols * 4;
    if (!read_n(in, pts, 3 * (size_t)N) || !read_n(in, nrm, with_normals ? 3 * (size_t)N : 0) || !read_n(in, lp, px) ||
        !read_n(in, ln, with_normals ? px : 0)) return 2;
    std::fclose(in);

    cuda::DeviceArray<float> points, normals, live;
    cuda::DeviceArray<unsigned char> status;
    cuda::DeviceArray<unsigned long long> counts;
    cuda::Cloud live_points; cuda::Normals live_normals;
    if (N) points.upload(pts);
    if (N && with_normals) normals.upload(nrm);
    live_points.upload(lp.data(), (size_t)cols * 16, rows, cols);
    if (with_normals) live_normals.upload(ln.data(), (size_t)cols * 16, rows, cols);
    cuda::associateProjective(Intr(fv[0], fv[1], fv[2], fv[3]), points, normals, N, live_points, live_normals, fv[4], fv[5], fv[6], live, &status,
                              &counts);
    cuda::waitAllDefaultStream();

    std::vector<float> live_h(3 * (size_t)N); std::vector<unsigned char> status_h((size_t)N); std::vector<unsigned long long> counts_h(8);
    if (N) { live.download(live_h.data()); status.download(status_h.data()); }
    counts.download(counts_h.data());
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::perror("out"); return 2; }
    std::fwrite(live_h.data(), 4, live_h.size(), out);
    std::fwrite(status_h.data(), 1, status_h.size(), out);
    std::fwrite(counts_h.data(), 8, 8, out);
    std::fclose(out);
    std::printf("associate ok: %d points, %llu paired\n", N, counts_h[0]);
    return 0;
}
