// fh_cluster.h -- the host rules of finch_index_cluster and finch_cluster_host (fh_library.cpp), each written
// once: the two jaccard bounds the device sorts a touched pair by, the validation of option index_cluster_margin, the host's
// union-find with smallest-index labels, and the bookkeeping of edges.  No HIP and no globals: the standard library only, so that
// tests/hostcore/cluster_host.cpp runs all of it on the host.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <limits>
#include <numeric>
#include <vector>

namespace fh {
namespace cluster {

// option index_cluster_margin: m of the upper bound, a double in [2^-20, 0.5].  Nothing sweeps the bands' soundness below
// 2^-20 (tests/test_index_cluster_model.py), so a smaller value is refused; 0.5 is where the upper bound of every k and D
// above 0 is still a number a jaccard can reach.
constexpr double MARGIN_MIN = 0x1p-20, MARGIN_MAX = 0.5, MARGIN_DEFAULT = MARGIN_MIN;

inline bool margin_valid(double m) { return m >= MARGIN_MIN && m <= MARGIN_MAX; } // (a NaN is neither)

// the option's text (nullptr: not set) -> *m; false for text that is no number in the range, *m untouched
inline bool margin_parse(const char *text, double *m) {
    if (!text) {
        *m = MARGIN_DEFAULT;
        return true;
    }
    char *end = nullptr;
    const double v = std::strtod(text, &end);
    if (end == text || *end != 0 || !margin_valid(v)) return false;
    *m = v;
    return true;
}

// the jaccard at which the distance is max_distance, in real numbers: x / (2 - x), x = exp(-k d)
inline double jaccard_at(uint32_t kmer_length, double max_distance) {
    const double x = std::exp(-(double)kmer_length * std::max(max_distance, 0.));
    return x / (2. - x);
}

// the lower bound: a pair below it is dropped on the device.  finch_index_dist's jmin (fh_library.cpp: index_dist_jmin), whose
// expression this is.
inline double jlo(uint32_t kmer_length, double max_distance) { return jaccard_at(kmer_length, max_distance) * (1. - 0x1p-20); }

// the upper bound: a pair at or above it is within max_distance whatever the host's log says, and the device unites it by
// itself.  Raised by m of itself -- at the default some 2^32 ulps against the few ulps between this figure and
// distance_from_counts' test.  Where that is no normal positive number (x underflowed: k d above some 700) nothing but
// jaccard 1 is sure: +inf.
inline double jhi(uint32_t kmer_length, double max_distance, double m) {
    const double v = jaccard_at(kmer_length, max_distance) * (1. + m);
    return std::isnormal(v) && v > 0. ? v : std::numeric_limits<double>::infinity();
}

// union-find over 0 .. n - 1 whose roots are their components' smallest members: the larger root goes under the smaller, so
// parent[v] <= v always, and labels() needs no second pass over the components.
struct UnionFind {
    std::vector<uint32_t> parent;
    explicit UnionFind(uint32_t n) : parent(n) { std::iota(parent.begin(), parent.end(), 0u); }
    uint32_t find(uint32_t v) {
        while (parent[v] != v) {
            parent[v] = parent[parent[v]]; // path halving
            v = parent[v];
        }
        return v;
    }
    // -> whether a and b were in two components
    bool unite(uint32_t a, uint32_t b) {
        a = find(a), b = find(b);
        if (a == b) return false;
        if (a < b) parent[b] = a;
        else parent[a] = b;
        return true;
    }
    // labels[v] = the smallest index of v's component; -> the components
    uint64_t labels(uint32_t *out) {
        uint64_t roots = 0;
        for (uint32_t v = 0; v < (uint32_t)parent.size(); ++v) { // (ascending: parent[v] < v has its label already)
            out[v] = parent[v] == v ? v : out[parent[v]];
            roots += parent[v] == v;
        }
        return roots;
    }
};

// what a call counts: every figure of finch_cluster_stats but the device's own times
struct Edges {
    uint64_t united = 0;    // ordered pairs, q != r, the device decided by itself
    uint64_t copied = 0;    // entries that crossed to the host
    uint64_t kept_host = 0; // ... of which q != r and the exact test kept
    uint64_t empty_side = 0; // host-made pairs with an empty side, q != r, that pass
    uint64_t edges() const { return united + kept_host + empty_side; }
};

} // namespace cluster
} // namespace fh
