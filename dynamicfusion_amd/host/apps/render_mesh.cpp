// render_mesh.cpp -- one render of a triangle mesh through the C++ mirror (kfusion::cuda::renderMesh over dfusion_render_mesh), inputs
// from a file, outputs to a file, so that tests/test_gpu_cxx_render.py can compare the bytes with the Python mirror's.
//   render_mesh <in.bin> <out.bin>
// in.bin : i32[6] V, T, cols, rows, max_extent, flags (1 world2cam, 2 normals, 4 attr, 8 colours); f32[4] fx, fy, cx, cy; f32[12]
//          world2cam R row-major then t (flag 1); vertices f32[4 V]; triangles u32[3 T]; normals f32[4 V] (flag 2); attr f32[4 V]
//          (flag 4); colours u8[4 V] (flag 8).
// out.bin: points f32[rows * cols * 4]; normals, attr likewise and colours u8[rows * cols * 4] (each with its flag); tri i32[rows * cols];
//          counts u64[6].
#include <cstdio>
#include <vector>
#include <kfusion/cuda/imgproc.hpp>
#include <kfusion/cuda/render_mesh.hpp>

using namespace kfusion;

template <class T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n; }

template <class A>
static void write_image(FILE* out, const A& img, int rows, int cols)
{
    std::vector<char> h((size_t)rows * cols * A::elem_size);
    img.download(h.data(), (size_t)cols * A::elem_size);
    std::fwrite(h.data(), 1, h.size(), out);
}

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::perror("in"); return 2; }
    int hd[6]; float fv[4]; float w2c[12];
    if (std::fread(hd, 4, 6, in) != 6 || std::fread(fv, 4, 4, in) != 4) return 2;
    const int V = hd[0], T = hd[1], cols = hd[2], rows = hd[3], max_extent = hd[4], flags = hd[5];
    if (V < 0 || T < 0 || cols <= 0 || rows <= 0) return 2;
    if ((flags & 1) && std::fread(w2c, 4, 12, in) != 12) return 2;
    std::vector<float> vtx, nrm, att; std::vector<int> tri; std::vector<unsigned char> col;
    if (!read_n(in, vtx, 4 * (size_t)V) || !read_n(in, tri, 3 * (size_t)T) || !read_n(in, nrm, (flags & 2) ? 4 * (size_t)V : 0) ||
        !read_n(in, att, (flags & 4) ? 4 * (size_t)V : 0) || !read_n(in, col, (flags & 8) ? 4 * (size_t)V : 0)) return 2;
    std::fclose(in);

    cuda::DeviceArray<Point> vertices, attr; cuda::DeviceArray<Normal> normals; cuda::DeviceArray<cuda::RGB> colors; cuda::DeviceArray<int> triangles;
    if (V) vertices.upload((const Point*)vtx.data(), (size_t)V);
    if (T) triangles.upload(tri.data(), 3 * (size_t)T);
    if (V && (flags & 2)) normals.upload((const Normal*)nrm.data(), (size_t)V);
    if (V && (flags & 4)) attr.upload((const Point*)att.data(), (size_t)V);
    if (V && (flags & 8)) colors.upload((const cuda::RGB*)col.data(), (size_t)V);
    Affine3f pose = Affine3f::Identity();
    if (flags & 1) {
        Mat3f R;
        for (int i = 0; i < 9; ++i) R.val[i] = w2c[i];
        pose = Affine3f(R, Vec3f(w2c[9], w2c[10], w2c[11]));
    }
    cuda::DeviceArray2D<int> tri_img; cuda::DeviceArray<unsigned long long> counts;
    cuda::RenderMeshOutputs out;
    out.tri = &tri_img; out.counts = &counts;
    cuda::renderMesh(Intr(fv[0], fv[1], fv[2], fv[3]), vertices, triangles, cols, rows, (flags & 1) ? &pose : nullptr, normals, attr, colors, out, max_extent);
    cuda::waitAllDefaultStream();

    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo) { std::perror("out"); return 2; }
    write_image(fo, out.points, rows, cols);
    if (normals.size()) write_image(fo, out.normals, rows, cols);
    if (attr.size()) write_image(fo, out.attr, rows, cols);
    if (colors.size()) write_image(fo, out.colors, rows, cols);
    write_image(fo, tri_img, rows, cols);
    std::vector<unsigned long long> counts_h(6);
    counts.download(counts_h.data());
    std::fwrite(counts_h.data(), 8, 6, fo);
    std::fclose(fo);
    std::printf("render_mesh ok: %d triangles, %llu drawn, %llu pixels covered\n", T, counts_h[0], counts_h[5]);
    return 0;
}
