// Stand-alone check of dynamicfusion_amd/csrc/dfusion_mesh_cc.h, the find / union step of dfusion_mesh_components: the very text the
// kernels run, here over a plain array (one thread) and over std::atomic with relaxed accesses (8 threads, each a share of the triangles),
// compared with a sequential union-find that keeps the smallest index per set.  Built with the compiler's address and
// undefined-behaviour checks and run by tests/test_mesh_cc_host.py.
#include <stdio.h>
#include <stdint.h>
#include <atomic>
#include <numeric>
#include <random>
#include <thread>
#include <vector>
#include "dfusion_mesh_cc.h"

#define CHECK(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)

struct PlainMem {
    std::vector<uint32_t>& p;
    uint32_t load(uint32_t i) const { return p.at(i); }
    void store(uint32_t i, uint32_t v) const { p.at(i) = v; }
    uint32_t cas(uint32_t i, uint32_t expect, uint32_t v) const { const uint32_t old = p.at(i); if (old == expect) p.at(i) = v; return old; }
};
struct AtomicMem {
    std::vector<std::atomic<uint32_t> >& p;
    uint32_t load(uint32_t i) const { return p.at(i).load(std::memory_order_relaxed); }
    void store(uint32_t i, uint32_t v) const { p.at(i).store(v, std::memory_order_relaxed); }
    uint32_t cas(uint32_t i, uint32_t expect, uint32_t v) const
    {
        p.at(i).compare_exchange_strong(expect, v, std::memory_order_relaxed);      // (on failure `expect` receives what was there)
        return expect;
    }
};

typedef std::vector<uint32_t> Tris;                  // 3 indices a triangle

// the smallest index of every vertex's component, by a sequential union-find
static std::vector<uint32_t> reference_labels(const Tris& t, uint32_t V)
{
    std::vector<uint32_t> p(V);
    std::iota(p.begin(), p.end(), 0u);
    auto find = [&](uint32_t x) { while (p[x] != x) x = p[x]; return x; };
    auto unite = [&](uint32_t a, uint32_t b) { a = find(a); b = find(b); if (a < b) p[b] = a; else p[a] = b; };
    for (size_t i = 0; i + 2 < t.size(); i += 3) {
        if (t[i] >= V || t[i + 1] >= V || t[i + 2] >= V) continue;
        unite(t[i], t[i + 1]); unite(t[i + 1], t[i + 2]);
    }
    std::vector<uint32_t> label(V);
    for (uint32_t v = 0; v < V; ++v) label[v] = find(v);
    return label;
}

template <class Mem>
static void unite_range(Mem m, const Tris& t, uint32_t V, size_t first, size_t step)
{
    for (size_t i = 3 * first; i + 2 < t.size(); i += 3 * step) {
        if (t[i] >= V || t[i + 1] >= V || t[i + 2] >= V) continue;
        if (t[i] != t[i + 1]) df_cc_union(m, t[i], t[i + 1]);
        if (t[i + 1] != t[i + 2]) df_cc_union(m, t[i + 1], t[i + 2]);
    }
}

// every entry obeys the invariant (parent[x] <= x) and its root is the reference's label
template <class Mem>
static int check_forest(Mem m, uint32_t V, const std::vector<uint32_t>& want)
{
    for (uint32_t v = 0; v < V; ++v) {
        CHECK(m.load(v) <= v);
        CHECK(df_cc_root(m, v) == want[v]);
    }
    for (uint32_t v = 0; v < V; ++v) CHECK(df_cc_find(m, v) == want[v]);            // (and with path shortening)
    for (uint32_t v = 0; v < V; ++v) CHECK(m.load(v) <= v);
    return 0;
}

static int run_plain(const Tris& t, uint32_t V)
{
    std::vector<uint32_t> p(V);
    std::iota(p.begin(), p.end(), 0u);
    unite_range(PlainMem{p}, t, V, 0, 1);
    return check_forest(PlainMem{p}, V, reference_labels(t, V));
}

static int run_threads(const Tris& t, uint32_t V, int n_threads)
{
    std::vector<std::atomic<uint32_t> > p(V);
    for (uint32_t v = 0; v < V; ++v) p[v].store(v);
    std::vector<std::thread> pool;
    for (int k = 0; k < n_threads; ++k) pool.emplace_back([&, k] { unite_range(AtomicMem{p}, t, V, (size_t)k, (size_t)n_threads); });
    for (std::thread& th : pool) th.join();
    return check_forest(AtomicMem{p}, V, reference_labels(t, V));
}

static Tris random_soup(std::mt19937& rng, size_t n, uint32_t V, bool with_bad)
{
    Tris t(3 * n);
    for (uint32_t& i : t) {
        i = (uint32_t)(rng() % V);
        if (with_bad && rng() % 50 == 0) i = rng() % 2 ? V : 0xffffffffu;
    }
    return t;
}

int main()
{
    {   // a descending chain: every union links the current root under a smaller one, the labels travel against the index order
        const uint32_t V = 20000;
        Tris t;
        for (uint32_t v = V - 1; v >= 2; --v) { t.push_back(v); t.push_back(v - 1); t.push_back(v - 2); }
        CHECK(run_plain(t, V) == 0);
        CHECK(run_threads(t, V, 8) == 0);
        Tris up(t.rbegin(), t.rend());                                               // the same chain from the other end
        CHECK(run_plain(up, V) == 0);
        CHECK(run_threads(up, V, 8) == 0);
    }
    {   // a star: everything hangs on one vertex, the largest index -- then on the smallest
        const uint32_t V = 5000;
        for (uint32_t hub : {V - 1, 0u, 2500u}) {
            Tris t;
            for (uint32_t v = 0; v + 1 < V; v += 2) { t.push_back(hub); t.push_back(v); t.push_back(v + 1); }
            CHECK(run_plain(t, V) == 0);
            CHECK(run_threads(t, V, 8) == 0);
        }
    }
    std::mt19937 rng(12345);
    const struct { size_t n; uint32_t V; } soups[] = {{0, 7}, {1, 3}, {50, 200}, {300, 200}, {2000, 3000}, {2000, 9000}, {30000, 20000}, {100000, 70000}};
    for (const auto& s : soups)
        for (int bad = 0; bad < 2; ++bad) {
            const Tris t = random_soup(rng, s.n, s.V, bad != 0);
            CHECK(run_plain(t, s.V) == 0);
            CHECK(run_threads(t, s.V, 8) == 0);
        }
    // many small sets under contention: 8 threads over the same few vertices
    for (int round = 0; round < 50; ++round) {
        const Tris t = random_soup(rng, 400, 24, false);
        CHECK(run_threads(t, 24, 8) == 0);
    }
    printf("mesh cc ok\n");
    return 0;
}
