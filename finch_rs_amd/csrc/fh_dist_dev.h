// fh_dist_dev.h -- the device functions the pair kernels share (fh_dist.hip: k_dist_counts and the search's selection;
// fh_index.hip: the index search and dist): the pair's scale step, the branchless bound search and the containment's and the
// jaccard's divisions.  One statement of each, so that two kernels that must agree on a pair's (c, i, j) and on its containment
// cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fh {

// the pair's scale step (distance.rs:16-29 + raw_distance's `scale > 0` test): min_scale = f64::min(q, r), which ignores a NaN
// argument (std::fmin): the reference's scale if r < q or q is NaN -- exact comparisons; both NaN picks r, which has no step --
// and M of the chosen sketch as the host computed it.  A: a kernel's argument block with qflag / rflag / qscale / rscale /
// qmax / rmax (flags: fh_dist.h's DistSide; the scales and M are read only where the flags ask for them).
template <class A>
__device__ inline bool pair_max_hash(const A &a, uint32_t q, uint32_t r, uint64_t &m) {
    const uint32_t fq = a.qflag[q], fr = a.rflag[r];
    if (!(fq & 1) || !(fr & 1)) return false;
    const double qs = a.qscale[q], rs = a.rscale[r];
    const bool pick_r = rs < qs || qs != qs;
    if (!((pick_r ? fr : fq) & 2)) return false;
    m = pick_r ? a.rmax[r] : a.qmax[q];
    return true;
}

// #{s[0..n) < x} (LE: <= x) over ascending s; top = the largest power of two <= n (0 for n = 0).  The same number of steps in
// every lane (the wave's n is uniform), no branch; the index is clamped so that no read leaves s[0..n)
// (pos + step < 2 * top <= 2^32: no wrap for any n).
template <bool LE>
__device__ inline uint32_t count_below(const uint64_t *s, uint32_t n, uint32_t top, uint64_t x) {
    uint32_t pos = 0;
    for (uint32_t step = top; step; step >>= 1) {
        const uint32_t p = pos + step;
        const uint64_t v = s[min(p, n) - 1];
        const bool take = p <= n && (LE ? v <= x : v < x);
        pos = take ? p : pos;
    }
    return pos;
}

// distance.rs:109-113 on the device.  No fast-math flag in this build: the division is IEEE's, the double finch_distance gets on
// the host; c <= j, so it is never negative and two of them order as their bit patterns do.
__device__ inline double containment_of(uint32_t c, uint32_t j) { return j ? (double)c / (double)j : 0.0; }

// distance_from_counts' jaccard (distance.rs:120-125; old mode distance.rs:150-151 with i = total = |R|, c <= total) on the
// device: the same u64 sums and the same IEEE division of the same two doubles, so the host's jaccard bit for bit.
__device__ inline double jaccard_of(bool old_mode, uint32_t c, uint32_t i, uint32_t j) {
    if (old_mode) return (double)c / (double)(c + 2 * ((uint64_t)i - c));
    const uint64_t total = (uint64_t)i - c + j;
    return total ? (double)c / (double)total : 1.0;
}

} // namespace fh
