// Stand-alone check of dynamicfusion_amd/csrc/dfusion_plan_halves.h, the integer logic the warped sweep's launch plan and the sweep share:
// random verdicts, sub-verdict bytes and slab cuts go through the plan kernel's packing, then through the sweep's dealing of half-layer
// cells over NW waves and its walk of each segment's planes (as df_warp_rows_pipe_kernel does it, U planes per batch); every plane of
// every patch must come out swept exactly once where the plan says so, and never otherwise.  Built and run by tests/test_plan_halves.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <random>
#include <vector>
#include "dfusion_plan_halves.h"

static int popc(uint32_t x) { return __builtin_popcount(x); }

int main()
{
    std::mt19937 rng(12345);
    long checked = 0;
    for (uint32_t x = 0; x < 65536; ++x) {
        if (df_unspread16(df_spread16(x)) != x || (df_spread16(x) & 0xaaaaaaaau)) { printf("spread16 %u\n", x); return 1; }
    }
    for (int trial = 0; trial < 4000; ++trial) {
        const int NW = 1 << (rng() % 3 + 2);                 // 4, 8, 16 waves
        const int SPW = NW / 4, U = 1 + (int)(rng() % 2), zt = 1 + (int)(rng() % 16), lt0 = (int)(rng() % 5);
        const int Z = (lt0 + zt) * 8 - (int)(rng() % 8);
        int own0 = (int)(rng() % (Z + 1)), own1 = (int)(rng() % (Z + 1));
        if (own0 > own1) { const int t = own0; own0 = own1; own1 = t; }
        if (trial % 3 == 0) { own0 = 0; own1 = Z; }
        const int mode = (int)(rng() % 4);                   // sub-verdict bytes: all set, random, lower halves only, upper halves only
        std::vector<uint32_t> words(4 * SPW);
        std::vector<std::vector<int>> want(4 * SPW, std::vector<int>(zt * 8, 0)), got = want;
        unsigned total2 = 0;
        for (int p = 0; p < 4 * SPW; ++p) {
            uint32_t lower = 0, upper = 0;
            for (int l = 0; l < zt; ++l) {
                const bool alive = rng() % 4 != 0;
                const unsigned sub = mode == 0 ? 0xffu : mode == 1 ? (rng() & 0xffu) : mode == 2 ? (rng() & 0x0fu) : (rng() & 0xf0u);
                const int zl = (lt0 + l) * 8;
                const int n0 = alive && (sub & 0x0fu) ? df_half_planes(zl, 0, own0, own1) : 0, n1 = alive && (sub & 0xf0u) ? df_half_planes(zl, 1, own0, own1) : 0;
                if (n0) lower |= 1u << l;
                if (n1) upper |= 1u << l;
                for (int z = 0; z < 8; ++z) {
                    const bool half_on = z < 4 ? n0 != 0 : n1 != 0;
                    want[p][l * 8 + z] = half_on && zl + z >= own0 && zl + z < own1 ? 1 : 0;
                }
                int n = 0;
                for (int z = 0; z < 4; ++z) n += want[p][l * 8 + z];
                if (n != n0) { printf("df_half_planes lower\n"); return 1; }
            }
            words[p] = df_halves_word(lower, upper);
            if (df_halves_layers(words[p]) != (lower | upper)) { printf("df_halves_layers\n"); return 1; }
            total2 += (unsigned)popc(words[p]);
        }
        for (int share = 0; share < NW; ++share) {
            const unsigned c0 = total2 * (unsigned)share / (unsigned)NW, c1 = total2 * (unsigned)(share + 1) / (unsigned)NW;
            unsigned pre = 0;
            for (int q = 0; q < 4 * SPW; ++q) {
                const uint32_t h32 = words[q];
                const unsigned n2 = (unsigned)popc(h32);
                const unsigned seg_lo = c0 > pre ? c0 : pre, seg_hi = c1 < pre + n2 ? c1 : pre + n2;
                const unsigned pre0 = pre;
                pre += n2;
                if (seg_lo >= seg_hi) continue;
                const uint32_t seg = df_halves_segment(h32, seg_lo - pre0, seg_hi - pre0);
                if ((unsigned)popc(seg) != seg_hi - seg_lo || (seg & ~h32)) { printf("df_halves_segment\n"); return 1; }
                const uint32_t alive = df_halves_layers(seg);
                auto zb = [&](int l) { const int z = (lt0 + l) * 8 + df_halves_z0(seg, l); return z > own0 ? z : own0; };
                auto ze = [&](int l) { const int z = (lt0 + l) * 8 + df_halves_z1(seg, l); return z < own1 ? z : own1; };
                int l = __builtin_ctz(alive), z0 = zb(l);
                while (l >= 0) {
                    if (z0 >= ze(l)) { printf("empty layer in a segment (trial %d)\n", trial); return 1; }
                    for (int u = 0; u < U; ++u) if (z0 + u < ze(l)) { ++got[q][z0 + u - lt0 * 8]; ++checked; }
                    z0 += U;
                    if (z0 >= ze(l)) {
                        const uint32_t rem = alive >> (l + 1);
                        l = rem ? l + 1 + __builtin_ctz(rem) : -1;
                        if (l >= 0) z0 = zb(l);
                    }
                }
            }
        }
        for (int p = 0; p < 4 * SPW; ++p)
            for (int z = 0; z < zt * 8; ++z)
                if (got[p][z] != want[p][z]) {
                    printf("trial %d (NW %d U %d zt %d lt0 %d own %d..%d mode %d): patch %d plane %d swept %d times, expected %d\n", trial, NW, U, zt, lt0, own0,
                           own1, mode, p, z + lt0 * 8, got[p][z], want[p][z]);
                    return 1;
                }
    }
    printf("plan halves ok: %ld planes walked\n", checked);
    return 0;
}
