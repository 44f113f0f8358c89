// mesh_distance.cpp -- the closest points and the distances between two triangle meshes through the C++ mirror
// (kfusion::cuda::closestPoints and meshDistance over dfusion_mesh_closest_points), inputs from files, outputs to a file, so that
// tests/test_gpu_cxx_mesh_closest.py can compare the bytes with the Python mirror's.
//   mesh_distance <a.bin> <b.bin> <out.bin>
// a.bin, b.bin: u32[2] V, T; vertices f32[4 V]; triangles u32[3 T].
// out.bin: for A's vertices against mesh B, then for B's against mesh A: counts u64[8]; triangle u32[n]; point f32[4 n]; bary f32[4 n]
//          (n = the number of samples).  The summary of meshDistance goes to stdout.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>
#include <kfusion/cuda/mesh_ops.hpp>
#include <kfusion/cuda/imgproc.hpp>

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

static bool load(const char* path, cuda::DeviceArray<Point>& vertices, cuda::DeviceArray<int>& triangles)
{
    FILE* in = std::fopen(path, "rb");
    if (!in) { std::perror(path); return false; }
    unsigned int hd[2];
    std::vector<float> vtx; std::vector<int> tri;
    const bool ok = std::fread(hd, 4, 2, in) == 2 && read_n(in, vtx, 4 * (size_t)hd[0]) && read_n(in, tri, 3 * (size_t)hd[1]);
    std::fclose(in);
    if (!ok) return false;
    if (hd[0]) vertices.upload((const Point*)vtx.data(), hd[0]);
    if (hd[1]) triangles.upload(tri.data(), 3 * (size_t)hd[1]);
    return true;
}

static void one_side(FILE* fo, const cuda::DeviceArray<Point>& samples, const cuda::DeviceArray<Point>& vertices, const cuda::DeviceArray<int>& triangles)
{
    cuda::DeviceArray<int> triangle; cuda::DeviceArray<Point> point, bary; cuda::DeviceArray<unsigned long long> counts;
    cuda::closestPoints(vertices, triangles, samples, std::numeric_limits<float>::infinity(), triangle, point, &bary, &counts);
    cuda::waitAllDefaultStream();
    std::vector<unsigned long long> n(8);
    counts.download(n.data());
    std::fwrite(n.data(), 8, 8, fo);
    write_array(fo, triangle);
    write_array(fo, point);
    write_array(fo, bary);
}

int main(int argc, char** argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: %s a.bin b.bin out.bin\n", argv[0]); return 2; }
    cuda::DeviceArray<Point> va, vb; cuda::DeviceArray<int> ta, tb;
    if (!load(argv[1], va, ta) || !load(argv[2], vb, tb)) return 2;
    FILE* fo = std::fopen(argv[3], "wb");
    if (!fo) { std::perror("out"); return 2; }
    one_side(fo, va, vb, tb);
    one_side(fo, vb, va, ta);
    std::fclose(fo);
    const cuda::MeshDistance d = cuda::meshDistance(va, ta, vb, tb);
    std::printf("mesh_distance ok: a_to_b answered %llu unanswered %llu max %.17g at %lld mean %.17g rms %.17g; "
                "b_to_a answered %llu unanswered %llu max %.17g at %lld mean %.17g rms %.17g; hausdorff %.17g\n",
                d.a_to_b.answered, d.a_to_b.unanswered, d.a_to_b.max, d.a_to_b.max_vertex, d.a_to_b.mean, d.a_to_b.rms,
                d.b_to_a.answered, d.b_to_a.unanswered, d.b_to_a.max, d.b_to_a.max_vertex, d.b_to_a.mean, d.b_to_a.rms, d.hausdorff);
    return 0;
}
