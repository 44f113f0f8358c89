// smooth_mesh.cpp -- the adjacency of a triangle mesh and its Taubin smoothing through the C++ mirror (kfusion::cuda::meshAdjacency and
// smoothMesh over dfusion_mesh_adjacency / dfusion_mesh_smooth), inputs from a file, outputs to a file, so that
// tests/test_gpu_cxx_mesh_smooth.py can compare the bytes with the Python mirror's.
//   smooth_mesh <in.bin> <out.bin>
// in.bin : u32[4] V, T, flags (DF_SMOOTH_*), iterations; f32[2] lambda, mu; vertices f32[4 V]; triangles u32[3 T].
// out.bin: counts u64[8]; row_start u32[V + 1]; neighbours u32[counts[0]]; vertex_class u8[V]; smoothed vertices f32[4 V].
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
    unsigned int hd[4]; float factors[2];
    if (std::fread(hd, 4, 4, in) != 4 || std::fread(factors, 4, 2, in) != 2) return 2;
    const size_t V = hd[0], T = hd[1];
    std::vector<float> vtx; std::vector<int> tri;
    if (!read_n(in, vtx, 4 * V) || !read_n(in, tri, 3 * T)) return 2;
    std::fclose(in);

    cuda::DeviceArray<Point> vertices, smoothed; cuda::DeviceArray<int> triangles, row_start, neighbours;
    cuda::DeviceArray<unsigned char> vertex_class; cuda::DeviceArray<unsigned long long> counts;
    if (V) vertices.upload((const Point*)vtx.data(), V);
    if (T) triangles.upload(tri.data(), 3 * T);
    cuda::meshAdjacency(triangles, V, row_start, neighbours, vertex_class, &counts);
    cuda::smoothMesh(vertices, row_start, neighbours, vertex_class, (int)hd[3], factors[0], factors[1], hd[2], smoothed);
    cuda::waitAllDefaultStream();

    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo) { std::perror("out"); return 2; }
    std::vector<unsigned long long> counts_h(8);
    counts.download(counts_h.data());
    std::fwrite(counts_h.data(), 8, 8, fo);
    write_array(fo, row_start);
    write_array(fo, neighbours);
    write_array(fo, vertex_class);
    write_array(fo, smoothed);
    std::fclose(fo);
    std::printf("smooth_mesh ok: %zu vertices, %zu triangles, %llu edges (%llu boundary, %llu irregular), %u iterations\n", V, T, counts_h[1], counts_h[2],
                counts_h[3], hd[3]);
    return 0;
}
