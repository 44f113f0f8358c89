// simplify_mesh.cpp -- one simplification of a triangle mesh through the C++ mirror (kfusion::cuda::simplifyMesh over
// dfusion_mesh_simplify), inputs from a file, outputs to a file, so that tests/test_gpu_cxx_mesh_simplify.py can compare the bytes with
// the Python mirror's.
//   simplify_mesh <in.bin> <out.bin>
// in.bin : u32[3] V, T, flags (DF_SIMPLIFY_*); f32 cell; vertices f32[4 V]; triangles u32[3 T].
// out.bin: counts u64[8]; vertices f32[4 n]; triangles u32[3 m]; vertex_src u32[n] (n = counts[0], m = counts[1]).
#include <cstdio>
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

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::perror("in"); return 2; }
    unsigned int hd[3]; float cell;
    if (std::fread(hd, 4, 3, in) != 3 || std::fread(&cell, 4, 1, in) != 1) return 2;
    const size_t V = hd[0], T = hd[1];
    std::vector<float> vtx; std::vector<int> tri;
    if (!read_n(in, vtx, 4 * V) || !read_n(in, tri, 3 * T)) return 2;
    std::fclose(in);

    cuda::DeviceArray<Point> vertices, out_vertices; cuda::DeviceArray<int> triangles, out_triangles, vertex_src;
    if (V) vertices.upload((const Point*)vtx.data(), V);
    if (T) triangles.upload(tri.data(), 3 * T);
    cuda::DeviceArray<unsigned long long> counts;
    cuda::simplifyMesh(vertices, triangles, cell, hd[2], out_vertices, out_triangles, vertex_src, &counts);
    cuda::waitAllDefaultStream();

    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo) { std::perror("out"); return 2; }
    std::vector<unsigned long long> counts_h(8);
    counts.download(counts_h.data());
    std::fwrite(counts_h.data(), 8, 8, fo);
    write_array(fo, out_vertices);
    write_array(fo, out_triangles);
    write_array(fo, vertex_src);
    std::fclose(fo);
    std::printf("simplify_mesh ok: %zu vertices, %zu triangles -> %llu, %llu\n", V, T, counts_h[0], counts_h[1]);
    return 0;
}
