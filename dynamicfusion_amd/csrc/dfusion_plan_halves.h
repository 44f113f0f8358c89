// dfusion_plan_halves.h -- the half-layer bits of the pipelined warped sweep's launch plan: plain integer functions, shared by the plan
// kernel and the sweep (dfusion_warp_pipe.h) and compiled for the host by tests/cxx/plan_halves_test.cpp.
//
// A (patch, layer) cell of a strip item is 8 x 8 x 8 voxels; the plan judges its two HALVES -- planes 0..3 and 4..7 of the layer -- apart.
// The 16 layers of a patch are one 32-bit word, bit 2 l + h = half h of layer l is swept: the halves in the order the sweep walks them.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__) || defined(__CUDACC__)
#define DF_HD __host__ __device__ __forceinline__
#else
#define DF_HD static inline
#endif

// bit i of a 16-bit word to bit 2 i, and back (bits 2 i of a 32-bit word to bit i; the odd bits are ignored)
DF_HD uint32_t df_spread16(uint32_t x)
{
    x &= 0xffffu;
    x = (x | (x << 8)) & 0x00ff00ffu; x = (x | (x << 4)) & 0x0f0f0f0fu; x = (x | (x << 2)) & 0x33333333u; x = (x | (x << 1)) & 0x55555555u;
    return x;
}
DF_HD uint32_t df_unspread16(uint32_t x)
{
    x &= 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u; x = (x | (x >> 2)) & 0x0f0f0f0fu; x = (x | (x >> 4)) & 0x00ff00ffu; x = (x | (x >> 8)) & 0x0000ffffu;
    return x;
}
// a patch's word from the 16-bit layer masks of its lower and upper halves
DF_HD uint32_t df_halves_word(uint32_t lower16, uint32_t upper16) { return df_spread16(lower16) | (df_spread16(upper16) << 1); }
// the layers with a half set, as a 16-bit mask
DF_HD uint32_t df_halves_layers(uint32_t hw) { return df_unspread16(hw | (hw >> 1)); }
// the set bits number lo .. hi - 1 of hw, counted from the lowest (lo <= hi <= popcount): a wave's SEGMENT of a patch's half layers
DF_HD uint32_t df_halves_segment(uint32_t hw, unsigned lo, unsigned hi)
{
    for (unsigned i = 0; i < lo; ++i) hw &= hw - 1u;
    uint32_t seg = 0u;
    for (unsigned i = lo; i < hi; ++i) { const uint32_t low = hw & (0u - hw); seg |= low; hw ^= low; }
    return seg;
}
// first and one-past-last plane, inside the layer (0, 4 or 8), of layer l of a segment; the layer has a half set
DF_HD int df_halves_z0(uint32_t seg, int l) { return ((seg >> (2 * l)) & 1u) ? 0 : 4; }
DF_HD int df_halves_z1(uint32_t seg, int l) { return ((seg >> (2 * l + 1)) & 1u) ? 8 : 4; }
// planes of half h of the layer that starts at plane zl which lie in [own0, own1): the slab's own planes (0 = none)
DF_HD int df_half_planes(int zl, int h, int own0, int own1)
{
    const int a = zl + 4 * h > own0 ? zl + 4 * h : own0, b = zl + 4 * h + 4 < own1 ? zl + 4 * h + 4 : own1;
    return b > a ? b - a : 0;
}
