// Driver of tests/test_index_update_host.py: the diagonal search of the index's merge (finch_rs_amd/csrc/fh_merge_path.h) on the
// host, exhaustively over small inputs with heavy ties.  For every pair of ascending lists a (up to MAX_A long) and b (up to
// MAX_B long) over an alphabet of three keys -- 0, a middle value and 2^64 - 1 --, every diagonal's cut is held against the two
// rank formulas of the merge, out[i + #{b < a_i}] = a_i and out[j + #{a <= b_j}] = b_j, by the binary search and by the
// search in rounds of 1, 2, 3 and 128 probes that the kernel's workgroup makes, and every tiling of the output (tile 1
// .. na + nb) is merged tile by tile the way the kernel does it, from the two cuts and the ranks inside the runs alone.
// Prints "ok <cases>" and returns 0, or says which check failed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fh_merge_path.h"

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "line %d: check failed: %s\n", __LINE__, #c); \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

static const uint64_t KEYS[3] = {0, 0x8000000000000000ull, 0xffffffffffffffffull};
static constexpr uint32_t MAX_A = 6, MAX_B = 5;

// every ascending list of n keys over KEYS: n0 of the first, n1 of the second, the rest of the third
static std::vector<std::vector<uint64_t>> lists(uint32_t n) {
    std::vector<std::vector<uint64_t>> out;
    for (uint32_t n0 = 0; n0 <= n; ++n0)
        for (uint32_t n1 = 0; n0 + n1 <= n; ++n1) {
            std::vector<uint64_t> v;
            for (uint32_t i = 0; i < n; ++i) v.push_back(KEYS[i < n0 ? 0 : i < n0 + n1 ? 1 : 2]);
            out.push_back(v);
        }
    return out;
}

int main() {
    unsigned long long cases = 0;
    for (uint32_t na = 0; na <= MAX_A; ++na)
        for (uint32_t nb = 0; nb <= MAX_B; ++nb)
            for (const std::vector<uint64_t> &a : lists(na))
                for (const std::vector<uint64_t> &b : lists(nb)) {
                    const uint32_t n = na + nb;
                    // the merge by the two rank formulas; which side each output place comes from
                    std::vector<uint64_t> want(n);
                    std::vector<int> from_a(n, -1);
                    for (uint32_t i = 0; i < na; ++i) {
                        uint32_t below = 0;
                        for (uint64_t y : b) below += y < a[i];
                        CHECK(from_a[i + below] == -1);
                        want[i + below] = a[i], from_a[i + below] = 1;
                    }
                    for (uint32_t j = 0; j < nb; ++j) {
                        uint32_t upto = 0;
                        for (uint64_t x : a) upto += x <= b[j];
                        CHECK(from_a[j + upto] == -1);
                        want[j + upto] = b[j], from_a[j + upto] = 0;
                    }
                    // a diagonal's cut = the a's among the first d outputs; monotone, and so is d - cut
                    std::vector<uint32_t> cut(n + 1);
                    for (uint32_t d = 0; d <= n; ++d) {
                        cut[d] = fh::merge_path_cut(a.data(), na, b.data(), nb, d);
                        uint32_t as = 0;
                        for (uint32_t p = 0; p < d; ++p) as += from_a[p];
                        CHECK(cut[d] == as);
                        CHECK(cut[d] <= na && d - cut[d] <= nb);
                        if (d) CHECK(cut[d] >= cut[d - 1] && d - cut[d] >= d - 1 - cut[d - 1]);
                        // the same cut by rounds of `ways` probes, as a workgroup finds it; the range shrinks every round
                        for (uint32_t ways : {1u, 2u, 3u, 128u}) {
                            uint32_t lo = fh::merge_path_lo(nb, d), hi = fh::merge_path_hi(na, d), rounds = 0;
                            while (lo < hi) {
                                const uint32_t step = fh::merge_path_step(lo, hi, ways), width = hi - lo;
                                uint32_t n_true = 0;
                                bool before = true;
                                for (uint32_t t = 0; t < ways; ++t) {
                                    const bool p = fh::merge_path_probe(a.data(), b.data(), d, lo, hi, step, t);
                                    CHECK(before || !p); // monotone: no true probe after a false one
                                    before = p;
                                    n_true += p;
                                }
                                fh::merge_path_narrow(lo, hi, step, n_true);
                                CHECK(lo <= hi && hi - lo < width && ++rounds <= na + 1);
                            }
                            CHECK(lo == cut[d]);
                        }
                    }
                    // every tiling: a tile's output from its two runs alone
                    for (uint32_t tile = 1; tile <= (n ? n : 1); ++tile) {
                        std::vector<uint64_t> got(n, 0x1234);
                        std::vector<int> side(n, -1);
                        for (uint32_t d0 = 0; d0 < n; d0 += tile) {
                            const uint32_t d1 = d0 + tile < n ? d0 + tile : n;
                            const uint32_t a0 = cut[d0], a1 = cut[d1], b0 = d0 - a0, b1 = d1 - a1, la = a1 - a0, lb = b1 - b0;
                            CHECK(la + lb == d1 - d0);
                            for (uint32_t x = 0; x < la; ++x) {
                                const uint32_t pos = x + fh::merge_rank<false>(b.data() + b0, lb, a[a0 + x]);
                                CHECK(pos < la + lb && side[d0 + pos] == -1);
                                got[d0 + pos] = a[a0 + x], side[d0 + pos] = 1;
                            }
                            for (uint32_t y = 0; y < lb; ++y) {
                                const uint32_t pos = y + fh::merge_rank<true>(a.data() + a0, la, b[b0 + y]);
                                CHECK(pos < la + lb && side[d0 + pos] == -1);
                                got[d0 + pos] = b[b0 + y], side[d0 + pos] = 0;
                            }
                        }
                        CHECK(got == want && side == from_a);
                        ++cases;
                    }
                }
    printf("ok %llu\n", cases);
    return 0;
}
