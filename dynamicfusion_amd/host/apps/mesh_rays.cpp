// mesh_rays.cpp -- ray queries against a triangle mesh through the C++ mirror (kfusion::cuda::rayHits and visiblePoints over
// dfusion_mesh_ray_hits), inputs from files, outputs to a file, so that tests/test_gpu_cxx_mesh_rays.py can compare the bytes with the
// Python mirror's.
//   mesh_rays <mesh.bin> <rays.bin> <out.bin>
// mesh.bin: u32[2] V, T; vertices f32[4 V]; triangles u32[3 T].
// rays.bin: u32 R; f32[2] t_min, t_max; f32[3] eye; f32 margin; origins f32[4 R]; directions f32[4 R].
// out.bin:  the nearest hits: counts u64[8]; triangle u32[R]; hit f32[4 R]; bary f32[4 R]; then any-hit: counts u64[8]; triangle
//           u32[R]; then visiblePoints of the mesh's own vertices from the eye: u8[V].  A summary goes to stdout.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <kfusion/cuda/mesh_ops.hpp>
#include <kfusion/cuda/imgproc.hpp>
#include "dfusion.h"

using namespace kfusion;

template <class T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n; }

template <class T>
static void write_array(FILE* out, const cuda::DeviceArray<T>& a)
{
    std::vector<T> h;
    a.download(h);
    if (!h.empty()) std::fwrite(h.data(), sizeof(T), h.size(), out);
}

static void write_counts(FILE* out, const cuda::DeviceArray<unsigned long long>& counts, unsigned long long* n)
{
    counts.download(n);
    std::fwrite(n, 8, 8, out);
}

int main(int argc, char** argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: %s mesh.bin rays.bin out.bin\n", argv[0]); return 2; }
    cuda::DeviceArray<Point> vertices, origins, directions; cuda::DeviceArray<int> triangles;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::perror(argv[1]); return 2; }
    unsigned int hd[2];
    std::vector<float> vtx; std::vector<int> tri;
    bool ok = std::fread(hd, 4, 2, in) == 2 && read_n(in, vtx, 4 * (size_t)hd[0]) && read_n(in, tri, 3 * (size_t)hd[1]);
    std::fclose(in);
    if (!ok) { std::fprintf(stderr, "%s: short\n", argv[1]); return 2; }
    if (hd[0]) vertices.upload((const Point*)vtx.data(), hd[0]);
    if (hd[1]) triangles.upload(tri.data(), 3 * (size_t)hd[1]);
    in = std::fopen(argv[2], "rb");
    if (!in) { std::perror(argv[2]); return 2; }
    unsigned int R;
    float par[6];                                                         // t_min, t_max, eye x y z, margin
    std::vector<float> o, d;
    ok = std::fread(&R, 4, 1, in) == 1 && std::fread(par, 4, 6, in) == 6 && read_n(in, o, 4 * (size_t)R) && read_n(in, d, 4 * (size_t)R);
    std::fclose(in);
    if (!ok) { std::fprintf(stderr, "%s: short\n", argv[2]); return 2; }
    if (R) { origins.upload((const Point*)o.data(), R); directions.upload((const Point*)d.data(), R); }
    FILE* fo = std::fopen(argv[3], "wb");
    if (!fo) { std::perror("out"); return 2; }

    cuda::DeviceArray<int> triangle; cuda::DeviceArray<Point> hit, bary; cuda::DeviceArray<unsigned long long> counts;
    unsigned long long near[8], any[8];
    cuda::rayHits(vertices, triangles, origins, directions, par[0], par[1], 0u, triangle, hit, &bary, &counts);
    cuda::waitAllDefaultStream();
    write_counts(fo, counts, near);
    write_array(fo, triangle);
    write_array(fo, hit);
    write_array(fo, bary);
    cuda::rayHits(vertices, triangles, origins, directions, par[0], par[1], DF_RAYS_ANY_HIT, triangle, hit, nullptr, &counts);
    cuda::waitAllDefaultStream();
    write_counts(fo, counts, any);
    write_array(fo, triangle);
    std::vector<unsigned char> visible;
    cuda::visiblePoints(vertices, triangles, vertices, par + 2, par[5], visible);
    if (!visible.empty()) std::fwrite(visible.data(), 1, visible.size(), fo);
    std::fclose(fo);
    size_t seen = 0;
    for (unsigned char b : visible) seen += b;
    std::printf("mesh_rays ok: rays %u hits %llu misses %llu invalid %llu tests %llu nodes %llu; any-hit hits %llu tests %llu; visible %zu of %zu\n",
                R, near[0], near[1], near[4], near[6], near[7], any[0], any[6], seen, visible.size());
    return 0;
}
