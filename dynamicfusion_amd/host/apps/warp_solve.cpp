// warp_solve.cpp -- one fixed, seeded problem through the C++ mirror's warp solves: the WarpField setters of the mode + energy_data, the
// resulting node transforms printed as hex words, eight a line, then (every mode but `reg`) one line with the four energies.
//   warp_solve reg    [neighbours lambda]                                  default 4 1; 0 0 = regularisation off (plain energy_data)
//       setRegularisation                                                      -> dfusion_warp_solve
//   warp_solve robust [neighbours lambda rounds tukey_c huber_delta]       default 4 1 3 0.04 0.01
//       + setRobust                                                            -> dfusion_warp_solve_robust
//   warp_solve plane  [neighbours lambda rounds tukey_c huber_delta]       default 4 1 3 0.02 0.01
//       + setPointToPlane                                                      -> dfusion_warp_solve_plane
//   warp_solve rigid  [neighbours lambda rounds tukey_c huber_delta]       default 4 1 3 0.02 0.01      (lambda_rot = 0.01)
//       + setNodeRotations, on the unwarped points and normals                 -> dfusion_warp_solve_rigid
// A last word `hier` (after the mode's arguments, or after the mode alone) puts the hierarchy under the regularisation term:
//       + setRegularisationHierarchy(2, 0.5, 2)
// and a last word `pcg` (behind `hier` where both are given) preconditions the `rigid` solve with the node blocks:
//       + setPreconditioner(1)
// The inputs come from 32-bit linear congruential generators and exact float arithmetic (the normals of `plane` and `rigid` from a second
// one, after everything else: components in [-1, 1), not unit length), so that tests/solver_cases.py can make the same problem for the
// Python mirror and the restatements, and the tests compare the bits.
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
    const char* const mode = argc > 1 ? argv[1] : "";
    const bool reg = !std::strcmp(mode, "reg"), robust = !std::strcmp(mode, "robust"), plane = !std::strcmp(mode, "plane"), rigid = !std::strcmp(mode, "rigid");
    if (!reg && !robust && !plane && !rigid) {
        std::fprintf(stderr, "usage: warp_solve reg [neighbours lambda] [hier]\n       warp_solve robust|plane|rigid [neighbours lambda rounds tukey_c huber_delta] [hier] [pcg]\n");
        return 2;
    }
    const bool pcg = argc > 2 && !std::strcmp(argv[argc - 1], "pcg");
    if (pcg) --argc;
    const bool hier = argc > 2 && !std::strcmp(argv[argc - 1], "hier");
    if (hier) --argc;
    const bool given = argc > (reg ? 3 : 6);                                // all of the mode's arguments, or the defaults
    const int neighbours = given ? std::atoi(argv[2]) : 4;
    const float lambda = given ? (float)std::atof(argv[3]) : 1.0f;
    const int rounds = given && !reg ? std::atoi(argv[4]) : 3;
    const float tukey_c = given && !reg ? (float)std::atof(argv[5]) : robust ? 0.04f : 0.02f;
    const float huber_delta = given && !reg ? (float)std::atof(argv[6]) : 0.01f;
    const bool with_normals = plane || rigid;
    const int M = 50, N = 1000;
    std::vector<Vec3f> pos(M), src(N), dst(N), normals(N, Vec3f(0, 0, 1));
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
    if (with_normals) {
        g_state = 2463534242u;
        for (int v = 0; v < N; ++v) for (int c = 0; c < 3; ++c) normals[v][c] = 2.0f * unit() - 1.0f;
    }
    wf.setSolverIterations(20);
    wf.setSolverDamping(1e-3f);
    wf.setRegularisation(neighbours, lambda);
    if (hier) wf.setRegularisationHierarchy(2, 0.5f, 2.f);
    if (!reg) wf.setRobust(rounds, tukey_c, huber_delta);
    if (with_normals) wf.setPointToPlane(true);
    if (rigid) wf.setNodeRotations(true, 0.01f);
    if (pcg) wf.setPreconditioner(1);
    if (!reg) wf.setTrackEnergy(true);
    wf.energy_data(src, normals, dst, normals);
    const std::vector<kfusion::deformation_node>& out = *wf.getNodes();
    for (int i = 0; i < M; ++i) {
        uint32_t w[8];
        std::memcpy(w, out[i].transform.raw(), sizeof(w));
        std::printf("%08x %08x %08x %08x %08x %08x %08x %08x\n", w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]);
    }
    if (reg) return 0;
    const float en[4] = {wf.lastEnergyBefore(), wf.lastEnergyAfter(), wf.lastRegEnergyBefore(), wf.lastRegEnergyAfter()};
    uint32_t w[4];
    std::memcpy(w, en, sizeof(w));
    std::printf("%08x %08x %08x %08x\n", w[0], w[1], w[2], w[3]);
    return 0;
}
