// dfusion_mesh_cc.h -- the find / union step of dfusion_mesh_components (dfusion_mesh_components.hip) as plain C++ over a memory policy:
// the same text runs in the kernels (relaxed agent-scope atomics on device memory) and on the host, where tests/cxx/mesh_cc_test.cpp
// compiles it with the compiler's address and undefined-behaviour checks over plain arrays and over std::atomic with 8 threads.
// No HIP types.
//
// A policy `Mem` gives three accesses to parent[]:
//   uint32_t load(uint32_t i)                             a read that sees every earlier successful cas / store of the same call stack,
//                                                         and sooner or later those of others
//   void     store(uint32_t i, uint32_t v)                a write that may be lost to a concurrent one (path shortening only)
//   uint32_t cas(uint32_t i, uint32_t expect, uint32_t v) compare-and-swap, returns what parent[i] held
//
// THE INVARIANT: parent[x] == x (x is a root) or parent[x] < x, and the only value ever stored into parent[x] is smaller than x.
//   - df_cc_union links a root a under b only with a > b, by a compare-and-swap that expects parent[a] == a;
//   - df_cc_find stores parent[parent[x]] over parent[x], and only after it has seen parent[x] != x: an ancestor of x, so smaller than
//     x, and x is not a root any more, so no compare-and-swap on x can succeed later and none is undone.
// Hence indices strictly decrease along every path (no cycle, at any time, under any interleaving), the root of a finished component is
// its smallest index, and a vertex never leaves the tree of a vertex it was united with.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DF_CC_HD __host__ __device__ __forceinline__
#else
#define DF_CC_HD static inline
#endif

// The root of x's tree at some moment during the call.  Ends: every step goes to a smaller index (the invariant), so at most x steps.
template <class Mem>
DF_CC_HD uint32_t df_cc_find(Mem& m, uint32_t x)
{
    uint32_t p = m.load(x);
    while (p != x) {
        const uint32_t g = m.load(p);                       // g <= p < x
        if (g != p) m.store(x, g);                          // path halving: an ancestor of x, smaller than x
        x = p; p = g;
    }
    return x;
}

// As df_cc_find, without a store (the flatten pass writes its own entry only).
template <class Mem>
DF_CC_HD uint32_t df_cc_root(Mem& m, uint32_t x)
{
    uint32_t p = m.load(x);
    while (p != x) { x = p; p = m.load(x); }
    return x;
}

template <class Mem>
DF_CC_HD void df_cc_union(Mem& m, uint32_t u, uint32_t v)
{
    uint32_t a = df_cc_find(m, u), b = df_cc_find(m, v);
    // Termination.  Before every compare-and-swap a > b.  It fails only if parent[a] != a, and then `old`, what parent[a] holds, is
    // smaller than a (the invariant): the next a = find(old) <= old < a, and the next b = find(b) <= b < a.  So max(a, b) strictly
    // decreases from trip to trip, it is never negative, and the loop ends after at most V trips whatever the other lanes do; each
    // find ends because indices strictly decrease along a path.  Correctness: old is in a's tree, so uniting the roots of old and b
    // is the union that was asked for; a success links a's whole tree under b < a, which keeps the invariant even if b has been
    // linked further down in the meantime.
    while (a != b) {
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = m.cas(a, a, b);
        if (old == a) break;
        a = df_cc_find(m, old);
        b = df_cc_find(m, b);
    }
}
