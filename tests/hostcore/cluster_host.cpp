// Driver of tests/test_cluster_hostcore.py: the host rules of the clustering calls (finch_rs_amd/csrc/fh_cluster.h) on their own
// (nothing else of the library).  `cluster_host` runs every check, prints "ok <graphs> <bounds>" and returns 0, or says which
// check failed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <utility>
#include <vector>

#include "fh_cluster.h"

#define CHECK(c)                                                                \
    do {                                                                        \
        if (!(c)) {                                                             \
            fprintf(stderr, "line %d: check failed: %s\n", __LINE__, #c);       \
            fflush(stderr);                                                     \
            _Exit(1);                                                           \
        }                                                                       \
    } while (0)

namespace C = fh::cluster;

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) { // splitmix64
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)((z ^ (z >> 31)) % n);
}

// the smallest index of every component by flood fill from each unvisited vertex in ascending order
static std::vector<uint32_t> flood(uint32_t n, const std::vector<std::pair<uint32_t, uint32_t>> &edges) {
    std::vector<std::vector<uint32_t>> adj(n);
    for (const auto &e : edges) adj[e.first].push_back(e.second), adj[e.second].push_back(e.first);
    std::vector<uint32_t> label(n, UINT32_MAX), stack;
    for (uint32_t s = 0; s < n; ++s) {
        if (label[s] != UINT32_MAX) continue;
        label[s] = s;
        stack.assign(1, s);
        while (!stack.empty()) {
            const uint32_t v = stack.back();
            stack.pop_back();
            for (uint32_t w : adj[v])
                if (label[w] == UINT32_MAX) label[w] = s, stack.push_back(w);
        }
    }
    return label;
}

static int graphs() {
    int n_graphs = 0;
    for (uint32_t n : {0u, 1u, 2u, 3u, 17u, 64u, 199u, 200u})
        for (uint32_t density : {0u, 1u, 2u, 8u}) // edges = n * density / 4
            for (int rep = 0; rep < 4; ++rep) {
                std::vector<std::pair<uint32_t, uint32_t>> edges;
                for (uint32_t t = 0; n && t < n * density / 4; ++t) edges.push_back({rnd(n), rnd(n)}); // (loops and repeats too)
                if (rep == 3) // a chain whose links arrive from the far end
                    for (uint32_t v = n; v-- > 1;) edges.push_back({v, v - 1});
                C::UnionFind uf(n);
                uint64_t merges = 0;
                for (const auto &e : edges) merges += uf.unite(e.first, e.second);
                for (uint32_t v = 0; v < n; ++v) CHECK(uf.parent[v] <= v);
                std::vector<uint32_t> got(n + 1, 0xabcdefu);
                const uint64_t roots = uf.labels(got.data());
                CHECK(got[n] == 0xabcdefu);
                const std::vector<uint32_t> want = flood(n, edges);
                uint64_t distinct = 0;
                for (uint32_t v = 0; v < n; ++v) {
                    CHECK(got[v] == want[v]);
                    distinct += want[v] == v;
                }
                CHECK(roots == distinct && merges == n - distinct);
                if (rep == 3 && n) CHECK(roots == 1);
                for (const auto &e : edges) CHECK(!uf.unite(e.first, e.second)); // (all united already)
                ++n_graphs;
            }
    return n_graphs;
}

static void margins() {
    double m = -1.;
    CHECK(C::margin_parse(nullptr, &m) && m == 0x1p-20);
    CHECK(C::margin_parse("0.25", &m) && m == 0.25);
    CHECK(C::margin_parse("0.5", &m) && m == 0.5);
    CHECK(C::margin_parse("9.5367431640625e-07", &m) && m == 0x1p-20);
    m = 7.;
    for (const char *bad : {"4.76837158203125e-07", "0.6", "0", "-0.25", "nan", "inf", "", "x", "0.25x", "0.25 "})
        CHECK(!C::margin_parse(bad, &m) && m == 7.);
    CHECK(C::margin_valid(0x1p-20) && C::margin_valid(0.5) && !C::margin_valid(0x1p-21) && !C::margin_valid(0.6));
    CHECK(!C::margin_valid(std::nan("")) && !C::margin_valid(std::nextafter(0x1p-20, 0.)) && !C::margin_valid(std::nextafter(0.5, 1.)));
}

static int bounds() {
    const double inf = std::numeric_limits<double>::infinity();
    int n = 0;
    for (uint32_t k : {0u, 1u, 4u, 11u, 21u, 31u, 32u, 51u, 64u, 700u, 745u, 800u, 0xffffffffu})
        for (double d : {0., -0., 5e-324, 1e-12, 1e-6, 0.01, 0.05, 0.1, 0.25, 0.5, 0.75, 0.999, std::nextafter(1., 0.), -1.})
            for (double m : {0x1p-20, 0.25, 0.5}) {
                const double lo = C::jlo(k, d), hi = C::jhi(k, d, m), at = C::jaccard_at(k, d);
                CHECK(lo >= 0. && lo <= at && lo < hi);
                CHECK(hi == inf || (std::isnormal(hi) && hi > at));
                if (at >= 0x1p-1000) CHECK(hi == at * (1. + m) && lo < at);
                ++n;
            }
    CHECK(C::jhi(21, 0., 0x1p-20) == 1. + 0x1p-20);      // above every jaccard: only jaccard 1 unites at D = 0
    CHECK(C::jhi(800, 0.999, 0.25) == inf && C::jlo(800, 0.999) == 0.); // x underflowed
    C::Edges e;
    e.united = 5, e.kept_host = 7, e.empty_side = 11, e.copied = 100;
    CHECK(e.edges() == 23);
    return n;
}

int main() {
    const int g = graphs();
    margins();
    const int b = bounds();
    printf("ok %d %d\n", g, b);
    return 0;
}
