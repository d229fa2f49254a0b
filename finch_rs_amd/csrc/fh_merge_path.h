// fh_merge_path.h -- the diagonal search of the index's merge (fh_index.hip: k_index_merge).  Two ascending
// lists a (the index's postings) and b (the added ones) are merged so that on equal keys every a comes before every b:
//     out[i + #{b < a_i}] = a_i,    out[j + #{a <= b_j}] = b_j.
// merge_path_cut(d) says how many of the first d outputs are a's; the other d - cut are b's.  Cuts at d0 < d1 bound a tile of
// the output whose inputs are a[cut(d0) .. cut(d1)) and b[d0 - cut(d0) .. d1 - cut(d1)), and within those two runs the rank
// formulas hold with the counts taken over the runs alone.  Plain C++ on the host (tests/hostcore/merge_path_host.cpp), device
// code under hipcc.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FH_MP_HD __host__ __device__
#else
#define FH_MP_HD
#endif

namespace fh {

// the least i in [max(0, d - nb), min(d, na)] with i == na, or d == i, or a[i] > b[d - i - 1]: below it a[i] <= b[d - i - 1]
// and a[i] goes out before that b.  a[i] ascends and b[d - i - 1] descends with i, so the test is monotone.  d <= na + nb.
FH_MP_HD inline uint32_t merge_path_cut(const uint64_t *a, uint32_t na, const uint64_t *b, uint32_t nb, uint32_t d) {
    uint32_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2; // mid < hi <= min(d, na); d - mid - 1 < nb as mid >= d - nb
        if (a[mid] <= b[d - mid - 1]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The same cut found by `ways` probes at a time (a workgroup's threads): the range [lo, hi] starts as merge_path_cut's, and
// while lo < hi it is cut into `ways` segments of merge_path_step() candidates; probe t tests the LAST candidate of segment t
// (false beyond hi: the cut is at most hi); the test being monotone, the first n_true probes are the true ones and the cut lies
// in segment n_true, which merge_path_narrow() makes the new range.  The range shrinks to less than a `ways`-th each time: a cut
// among 10^8 postings takes four rounds of 128 probes where the binary search makes 27 dependent loads.
FH_MP_HD inline uint32_t merge_path_lo(uint32_t nb, uint32_t d) { return d > nb ? d - nb : 0; }
FH_MP_HD inline uint32_t merge_path_hi(uint32_t na, uint32_t d) { return d < na ? d : na; }
FH_MP_HD inline uint32_t merge_path_step(uint32_t lo, uint32_t hi, uint32_t ways) { return (uint32_t)(((uint64_t)(hi - lo) + ways - 1) / ways); }
FH_MP_HD inline bool merge_path_probe(const uint64_t *a, const uint64_t *b, uint32_t d, uint32_t lo, uint32_t hi, uint32_t step, uint32_t t) {
    const uint64_t i = lo + ((uint64_t)t + 1) * step - 1; // (lo <= i < hi <= min(d, na), and d - i - 1 < nb as i >= d - nb)
    return lo < hi && i < hi && a[i] <= b[d - i - 1];
}
FH_MP_HD inline void merge_path_narrow(uint32_t &lo, uint32_t &hi, uint32_t step, uint32_t n_true) {
    if (lo >= hi) return;
    const uint64_t from = lo + (uint64_t)n_true * step; // (n_true probes were below hi: from <= hi)
    lo = (uint32_t)(from < hi ? from : hi);
    hi = (uint32_t)(from + step - 1 < hi ? from + step - 1 : hi);
}

// #{s[0 .. n) < x} (LE: <= x) of an ascending run
template <bool LE>
FH_MP_HD inline uint32_t merge_rank(const uint64_t *s, uint32_t n, uint64_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (LE ? s[mid] <= x : s[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

} // namespace fh
