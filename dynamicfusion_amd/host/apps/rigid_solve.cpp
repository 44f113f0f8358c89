// rigid_solve.cpp -- one fixed, seeded problem (plane_solve.cpp's) through the C++ mirror's warp solve with node rotations as unknowns:
// WarpField::setRegularisation + setRobust + setPointToPlane + setNodeRotations + energy_data (dfusion_warp_solve_rigid) on the unwarped
// points and normals, the resulting node transforms printed as hex words, eight a line, then one line with the four energies.
//   rigid_solve [neighbours lambda rounds tukey_c huber_delta]      default 4 1 3 0.02 0.01      (lambda_rot = 0.01)
// The inputs come from 32-bit linear congruential generators and exact float arithmetic (the normals from a second one, after everything
// else: components in [-1, 1), not unit length), so that tests/test_gpu_solver_rigid.py can make the same problem and compare the bits.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <kfusion/warp_field.hpp>

using kfusion::Vec3f;

static uint32_t g_state = 12345u;
static float unit()                                                        // [0, 1), 24 bits: exact in float
{
    g_state = g_state * 1664525u + 1013904223u;
    return (float)(g_state >> 8) * (1.0f / 16777216.0f);
}

int main(int argc, char** argv)
{
    const int neighbours = argc > 5 ? std::atoi(argv[1]) : 4;
    const float lambda = argc > 5 ? (float)std::atof(argv[2]) : 1.0f;
    const int rounds = argc > 5 ? std::atoi(argv[3]) : 3;
    const float tukey_c = argc > 5 ? (float)std::atof(argv[4]) : 0.02f;
    const float huber_delta = argc > 5 ? (float)std::atof(argv[5]) : 0.01f;
    const int M = 50, N = 1000;
    std::vector<Vec3f> pos(M), src(N), dst(N), normals(N);
    for (int i = 0; i < M; ++i) for (int c = 0; c < 3; ++c) pos[i][c] = 2.0f * unit() - 1.0f;
    kfusion::WarpField wf(8);
    wf.init(pos);
    std::vector<kfusion::deformation_node>& nodes = *wf.getNodes();
    for (int i = 0; i < M; ++i) {
        float dq[8] = {0.96f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        dq[1 + i % 3] = 0.28f;                                              // a unit rotation about one of the axes
        for (int c = 0; c < 4; ++c) dq[4 + c] = (unit() - 0.5f) * 0.0625f;
        std::memcpy((void*)nodes[i].transform.raw(), dq, sizeof(dq));
        nodes[i].weight = 0.25f + 0.25f * unit();
    }
    wf.commit(true);
    for (int v = 0; v < N; ++v)
        for (int c = 0; c < 3; ++c) { src[v][c] = 2.0f * unit() - 1.0f; dst[v][c] = src[v][c] + (unit() - 0.5f) * 0.0625f; }
    g_state = 2463534242u;
    for (int v = 0; v < N; ++v) for (int c = 0; c < 3; ++c) normals[v][c] = 2.0f * unit() - 1.0f;
    wf.setSolverIterations(20);
    wf.setSolverDamping(1e-3f);
    wf.setRegularisation(neighbours, lambda);
    wf.setRobust(rounds, tukey_c, huber_delta);
    wf.setPointToPlane(true);
    wf.setNodeRotations(true, 0.01f);
    wf.setTrackEnergy(true);
    wf.energy_data(src, normals, dst, normals);
    const std::vector<kfusion::deformation_node>& out = *wf.getNodes();
    for (int i = 0; i < M; ++i) {
        uint32_t w[8];
        std::memcpy(w, out[i].transform.raw(), sizeof(w));
        std::printf("%08x %08x %08x %08x %08x %08x %08x %08x\n", w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]);
    }
    const float en[4] = {wf.lastEnergyBefore(), wf.lastEnergyAfter(), wf.lastRegEnergyBefore(), wf.lastRegEnergyAfter()};
    uint32_t w[4];
    std::memcpy(w, en, sizeof(w));
    std::printf("%08x %08x %08x %08x\n", w[0], w[1], w[2], w[3]);
    return 0;
}
