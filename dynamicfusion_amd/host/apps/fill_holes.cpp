// fill_holes.cpp -- the boundary loops of a triangle mesh and the mesh with its small holes filled through the C++ mirror
// (kfusion::cuda::boundaryLoops and fillHoles over dfusion_mesh_boundary_loops / dfusion_mesh_fill_holes), inputs from a file, outputs
// to a file, so that tests/test_gpu_cxx_mesh_holes.py can compare the bytes with the Python mirror's.
//   fill_holes <in.bin> <out.bin> <MAX_EDGES>
// in.bin : u32[2] V, T; vertices f32[4 V]; triangles u32[3 T].
// out.bin: loop counts u64[8]; vertex_next, vertex_loop, vertex_rank u32[V] each; loop_start u32[counts[0] + 1]; loop_vertices
//          u32[counts[1]]; fill counts u64[8]; vertices f32[4 n]; triangles u32[3 m]; vertex_src u32[n] (n, m = fill counts [0], [1]).
#include <cstdio>
#include <cstdlib>
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
    if (argc != 4) { std::fprintf(stderr, "usage: %s in.bin out.bin MAX_EDGES\n", argv[0]); return 2; }
    char* end = nullptr;
    const unsigned long long max_edges = std::strtoull(argv[3], &end, 10);
    if (!*argv[3] || *end || max_edges > 0xffffffffull) { std::fprintf(stderr, "MAX_EDGES: 0 .. 4294967295\n"); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::perror("in"); return 2; }
    unsigned int hd[2];
    if (std::fread(hd, 4, 2, in) != 2) return 2;
    const size_t V = hd[0], T = hd[1];
    std::vector<float> vtx; std::vector<int> tri;
    if (!read_n(in, vtx, 4 * V) || !read_n(in, tri, 3 * T)) return 2;
    std::fclose(in);

    cuda::DeviceArray<Point> vertices, filled; cuda::DeviceArray<int> triangles, next, loop, rank, loop_start, loop_vertices, filled_triangles, vertex_src;
    cuda::DeviceArray<unsigned long long> loop_counts, fill_counts;
    if (V) vertices.upload((const Point*)vtx.data(), V);
    if (T) triangles.upload(tri.data(), 3 * T);
    cuda::boundaryLoops(triangles, V, next, loop, rank, loop_start, loop_vertices, &loop_counts);
    cuda::fillHoles(vertices, triangles, (unsigned int)max_edges, filled, filled_triangles, vertex_src, &fill_counts);
    cuda::waitAllDefaultStream();

    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo) { std::perror("out"); return 2; }
    std::vector<unsigned long long> lc(8), fc(8);
    loop_counts.download(lc.data());
    fill_counts.download(fc.data());
    std::fwrite(lc.data(), 8, 8, fo);
    write_array(fo, next);
    write_array(fo, loop);
    write_array(fo, rank);
    write_array(fo, loop_start);
    write_array(fo, loop_vertices);
    std::fwrite(fc.data(), 8, 8, fo);
    write_array(fo, filled);
    write_array(fo, filled_triangles);
    write_array(fo, vertex_src);
    std::fclose(fo);
    std::printf("fill_holes ok: %zu vertices, %zu triangles, %llu loops (longest %llu), %llu filled at max_edges %llu, %llu triangles added\n", V, T, lc[0],
                lc[5], fc[2], max_edges, fc[4]);
    return 0;
}
