// fh_index.hip -- an inverted index over a sketch library and the search through it (finch_index_new / finch_index_search,
// include/finch_host.h).  finch_search counts every (query, reference) pair; a search with a threshold above 0
// can only return pairs that share a hash, and those are what an index over the library's hashes enumerates.
//
// The index is the library's postings (hash, reference), sorted by hash with a stable sort -- equal hashes in ascending reference
// order --, duplicates kept: a hash's references are the run between its lower and its upper bound.  A search launch takes a
// chunk of queries, a workgroup each:
//   * k_index_count: per query hash the posting run (two bound searches per thread), then the runs of 256 query hashes walked
//     flat by the whole workgroup over the prefix sum of their lengths -- a hash every reference holds is 256 threads' work, not
//     one thread's loop; per posting one atomicAdd on the query's counter of that reference, and the add that returns 0 appends
//     the reference to the query's touched list;
//   * k_index_finish: per touched pair c is read and 0 stored back -- the counters are clean for the next launch without a
//     memset of the dense array --, i and j follow in closed form from each side's last hash and the pair's M (DESIGN.md §3.7:
//     two to four bound searches), and the pair is appended to the chunk's list where c / j >= min_containment.
//   * k_index_dist_finish: finch_index_dist's finish after the same count: c, and 0 back; (i, j) as above, or
//     old mode's total = |R|; the pair is appended where its jaccard reaches the host's conservative bound for the query.  The
//     queries may be the library's own sketches (pairwise), read from the CSR the index holds.
// finch_index_cluster turns the same pairwise finish into single-linkage clusters:
//   * k_index_cluster_finish: k_index_dist_finish's sibling with a bound on either side: a pair above the upper one is united on
//     the device in a lock-free union-find of one word per reference, a pair below the lower one is dropped, and only the band
//     between crosses to the host's exact test;
//   * k_index_cluster_labels: after an entry's last chunk, every reference's root.
// finch_index_gather keeps the counters of the same count live through the rounds of finch_gather's loop:
//   * k_index_gather_candidates: per touched pair c is read and LEFT; (q, r, c) is appended where c >= min_overlap;
//   * k_index_gather_rounds: one workgroup of 1024 per query, the whole loop inside.  cnt[r] == |S_t n H_r| for every touched r:
//     a round's winner is an arg-max over the candidates' counters, and removing S_t n H_w lowers by one the counter of every
//     reference in the posting run of every removed hash, the runs dealt flat over the workgroup as the count deals them.  The
//     remaining set is a bitmask over query positions in LDS, as in fh_gather.hip; no position arrays are built.  The tail
//     stores 0 to every touched counter, so the index is clean for the next launch.
// finch_index_compare_counts walks only the pairs whose count passes:
//   * k_index_moments_select: per touched pair c is read and 0 stored back; (q, r, c) is appended where c >= min_common;
//   * k_index_moments (fh_moments.hip, the object without fused multiply-adds): one wave per appended pair, over this file's
//     arrays and the library's counts that finch_index_attach_counts left beside its hashes.
// The order in which atomics land decides only where an entry sits in a list; the host sorts.
// finch_index_add / finch_index_keep change the library in place, and there order is the contract -- the
// postings they leave are the postings a build leaves:
//   * k_index_merge: the added sketches' postings, sorted like the build's, merged into the index's by a tiled merge path
//     (fh_merge_path.h); on equal hashes every old reference before every new one;
//   * k_index_compact / k_index_tile_scan: the postings of the kept references, in their order, renamed; places from scans;
//   * k_index_keep_refs: the kept references' hashes, counts and per-reference values to their new places.
// Both build beside the arrays in use (IndexStage); index_commit swaps.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../../include/finch_hip.h"
#include "fh_core.h"
#include "fh_device.h"
#include "fh_dist_dev.h"
#include "fh_index.h"
#include "fh_internal.h"
#include "fh_kernels.h"
#include "fh_merge_path.h"
#include "fh_moments.h"
#include "fh_screen.h"

using namespace fh;

namespace {

#define IHIP_TRY(expr)                                                                                      \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess) return api_fail(FH_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

constexpr uint32_t THREADS = 256; // four waves
constexpr uint32_t WAVES = THREADS / 64;

struct IndexArgs {
    // the library: its hashes as the CSR the dense path uploads; per reference its length, last hash, flags, scale and M
    const uint64_t *rh, *roff, *rlast, *rmax;
    const uint32_t *rlen, *rflag;
    const double *rscale;
    const uint64_t *keys; // the postings, ascending by hash
    const uint32_t *vals; // ... and their references
    uint32_t n_post, post_top, nr;
    // the chunk's queries: hashes from qbase on, qoff[0 .. n] as the whole call has them, the rest per query of the chunk
    const uint64_t *qh, *qoff, *qmax;
    const uint32_t *qflag;
    const double *qscale;
    uint64_t qbase;
    uint32_t q0; // the chunk's first query: what an entry names
    // per query of the chunk: nr counters (zero between launches), nr places of its touched list, the list's length
    uint32_t *cnt, *touched, *tcount;
    double min_c;
    uint32_t *sel, *cursor; // the chunk's list of entries (q, r, c, i, j) and its cursor (zero before k_index_finish)
    uint32_t sel_cap;
};

__device__ inline uint32_t top_of(uint32_t n) { return n ? 1u << (31 - __clz(n)) : 0; }

// grid: x = reference block.  Posting t of reference r -- (its t-th hash, r) -- goes to where the hash is in the CSR: reference order.
// The build forms every reference's (first = 0); an add forms those of the references first .. nr - 1 only, and keys / vals start
// at the first of them.
__global__ void __launch_bounds__(THREADS) k_index_postings(const uint64_t *rh, const uint64_t *roff, uint32_t first, uint32_t nr, uint64_t *keys,
                                                            uint32_t *vals) {
    const uint64_t t0 = roff[first];
    for (uint32_t r = first + blockIdx.x; r < nr; r += gridDim.x) {
        const uint64_t r0 = roff[r], r1 = roff[r + 1];
        for (uint64_t t = r0 + threadIdx.x; t < r1; t += THREADS) {
            keys[t - t0] = rh[t];
            vals[t - t0] = r;
        }
    }
}

// ---- finch_index_add / finch_index_keep ---------------------------------------------------------------
// Here, unlike every list above, output order is the contract: the postings stay sorted by hash with a hash's references
// ascending, which is what a build leaves.  Positions come from searches and scans; no atomic cursor decides one.

constexpr uint32_t UPDATE_MAX_TILE = 2048;

constexpr uint32_t MERGE_ITEMS = UPDATE_MAX_TILE / THREADS; // postings of a tile per thread, at most

// grid: x = tile of `tile` output postings (blocks go round).  a = the index's postings, b = the added ones, both ascending by
// key, b's references all above a's: on equal keys every a goes before every b (fh_merge_path.h).  The tile's two diagonal cuts
// are searched by the whole workgroup, 128 probes a round each (threads 0..127 the cut at the tile's start, 128..255 the one at
// its end); the tile's runs of a and b are staged in LDS; every thread ranks its postings in the other run and keeps them in
// registers; they go back to LDS at their ranks -- the same 24 KiB, six workgroups to a CU -- and the tile is written in order.
__global__ void __launch_bounds__(THREADS) k_index_merge(const uint64_t *ak, const uint32_t *av, uint32_t na, const uint64_t *bk, const uint32_t *bv,
                                                         uint32_t nb, uint64_t *ok, uint32_t *ov, uint32_t tile, uint32_t n_tiles) {
    __shared__ uint64_t s_k[UPDATE_MAX_TILE];
    __shared__ uint32_t s_v[UPDATE_MAX_TILE];
    const uint64_t n = (uint64_t)na + nb; // (below 2^32: the host's bound on an index)
    const uint32_t end = threadIdx.x >> 7, t = threadIdx.x & 127; // which cut this thread probes, and its probe
    for (uint32_t ti = blockIdx.x; ti < n_tiles; ti += gridDim.x) {
        const uint64_t d0 = min((uint64_t)ti * tile, n), d1 = min(d0 + tile, n);
        // every thread follows both ranges: the loop and its barriers are uniform
        uint32_t lo0 = merge_path_lo(nb, (uint32_t)d0), hi0 = merge_path_hi(na, (uint32_t)d0);
        uint32_t lo1 = merge_path_lo(nb, (uint32_t)d1), hi1 = merge_path_hi(na, (uint32_t)d1);
        while (lo0 < hi0 || lo1 < hi1) {
            const uint32_t step0 = merge_path_step(lo0, hi0, 128), step1 = merge_path_step(lo1, hi1, 128);
            const bool p = end ? merge_path_probe(ak, bk, (uint32_t)d1, lo1, hi1, step1, t) : merge_path_probe(ak, bk, (uint32_t)d0, lo0, hi0, step0, t);
            const uint32_t n0 = (uint32_t)__syncthreads_count(p && !end), n1 = (uint32_t)__syncthreads_count(p && end);
            merge_path_narrow(lo0, hi0, step0, n0);
            merge_path_narrow(lo1, hi1, step1, n1);
        }
        const uint32_t a0 = lo0, a1 = lo1;
        const uint32_t b0 = (uint32_t)d0 - a0, b1 = (uint32_t)d1 - a1;
        // (a cut is at most na and at least d - nb, and it is monotone in d as d - cut is: la + lb = d1 - d0 <= tile; the
        // guards keep every read inside a and b whatever the input)
        const uint32_t la = a1 > a0 ? min(a1 - a0, tile) : 0, lb = b1 > b0 ? min(b1 - b0, tile - la) : 0;
        for (uint32_t x = threadIdx.x; x < la + lb; x += THREADS) {
            const bool from_a = x < la;
            s_k[x] = from_a ? ak[a0 + x] : bk[b0 + (x - la)];
            s_v[x] = from_a ? av[a0 + x] : bv[b0 + (x - la)];
        }
        __syncthreads();
        uint64_t key[MERGE_ITEMS];
        uint32_t val[MERGE_ITEMS], pos[MERGE_ITEMS];
#pragma unroll
        for (uint32_t m = 0; m < MERGE_ITEMS; ++m) {
            const uint32_t x = threadIdx.x + m * THREADS;
            key[m] = 0, val[m] = 0, pos[m] = UPDATE_MAX_TILE;
            if (x < la + lb) {
                key[m] = s_k[x], val[m] = s_v[x];
                pos[m] = x < la ? x + merge_rank<false>(s_k + la, lb, key[m]) : (x - la) + merge_rank<true>(s_k, la, key[m]);
            }
        }
        __syncthreads(); // every rank is taken from the runs as staged
#pragma unroll
        for (uint32_t m = 0; m < MERGE_ITEMS; ++m)
            if (pos[m] < la + lb) s_k[pos[m]] = key[m], s_v[pos[m]] = val[m];
        __syncthreads();
        for (uint32_t x = threadIdx.x; x < la + lb; x += THREADS) {
            ok[d0 + x] = s_k[x];
            ov[d0 + x] = s_v[x];
        }
        __syncthreads(); // the next tile stages over what was just read
    }
}

// grid: x = tile of `tile` postings (blocks go round).  A posting survives where map[its reference] is not NONE_REF.  WRITE =
// false: count[ti] = the tile's survivors.  WRITE = true: count[] holds the exclusive scan of those, and the tile's survivors go,
// in their order, to ok / ov from count[ti] on, the reference renamed through map.  256 postings at a time: a lane's place among
// its wave's survivors by mbcnt, the waves' sums through LDS, the batches' through a running carry.
constexpr uint32_t NONE_REF = 0xffffffffu;
template <bool WRITE>
__global__ void __launch_bounds__(THREADS) k_index_compact(const uint64_t *keys, const uint32_t *vals, uint32_t n, const uint32_t *map, uint32_t nr,
                                                           uint32_t tile, uint32_t n_tiles, uint32_t *count, uint64_t *ok, uint32_t *ov, uint32_t n_out) {
    __shared__ uint32_t s_w[WAVES];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t ti = blockIdx.x; ti < n_tiles; ti += gridDim.x) {
        const uint64_t p0 = (uint64_t)ti * tile, p1 = min(p0 + tile, (uint64_t)n);
        uint32_t carry = WRITE ? count[ti] : 0;
        for (uint64_t base = p0; base < p1; base += THREADS) { // (whole workgroups go round: the barriers see every thread)
            const uint64_t p = base + threadIdx.x;
            uint32_t to = NONE_REF;
            if (p < p1) {
                const uint32_t r = vals[p];
                to = r < nr ? map[r] : NONE_REF;
            }
            const bool live = to != NONE_REF;
            const uint64_t mask = __ballot(live);
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
            if (lane == 0) s_w[wave] = (uint32_t)__popcll(mask);
            __syncthreads();
            uint32_t before = 0, total = 0;
            for (uint32_t w = 0; w < WAVES; ++w) {
                before += w < wave ? s_w[w] : 0;
                total += s_w[w];
            }
            if (WRITE && live) {
                const uint32_t o = carry + before + rank;
                if (o < n_out) ok[o] = keys[p], ov[o] = to;
            }
            carry += total;
            __syncthreads(); // the next batch writes s_w again
        }
        if (!WRITE && threadIdx.x == 0) count[ti] = carry;
    }
}

// one workgroup of 1024: count[0 .. n) becomes its exclusive scan, 1024 at a time with a running carry; *total = the sum
__global__ void __launch_bounds__(1024) k_index_tile_scan(uint32_t *count, uint32_t n, uint32_t *total) {
    __shared__ uint32_t s_w[16];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint64_t base = 0; base < n; base += 1024) { // (whole workgroups go round)
        const uint64_t t = base + threadIdx.x;
        const uint32_t c = t < n ? count[t] : 0;
        uint32_t inc = c;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = __shfl_up(inc, o, 64);
            if ((int)lane >= o) inc += v;
        }
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        uint32_t before = 0, sum = 0;
        for (uint32_t w = 0; w < 16; ++w) {
            before += w < wave ? s_w[w] : 0;
            sum += s_w[w];
        }
        if (t < n) count[t] = carry + before + inc - c;
        carry += sum;
        __syncthreads(); // the next batch writes s_w again
    }
    if (threadIdx.x == 0) *total = carry;
}

struct KeepRefsArgs {
    const uint64_t *rh, *roff, *rlast, *rmax; // the library as it is
    const uint32_t *rlen, *rflag, *rcnt;      // (rcnt: nullptr where no counts are attached)
    const double *rscale;
    uint32_t nr;
    const uint32_t *keep; // the survivors, ascending
    uint32_t n_keep;
    const uint64_t *noff; // ... and their offsets in the new CSR, n_keep + 1
    uint64_t *nh, *nlast, *nmax;
    uint32_t *nlen, *nflag, *ncnt;
    double *nscale;
};

// grid: x = surviving reference (blocks go round): its run of hashes (and of counts) moves to its new offset, its per-reference
// values to its new index
__global__ void __launch_bounds__(THREADS) k_index_keep_refs(KeepRefsArgs k) {
    for (uint32_t s = blockIdx.x; s < k.n_keep; s += gridDim.x) {
        const uint32_t r = k.keep[s];
        if (r >= k.nr) continue; // (the host checked the list)
        const uint64_t o0 = k.roff[r], n0 = k.noff[s];
        const uint64_t len = min(k.roff[r + 1] - o0, k.noff[s + 1] - n0); // (equal: the host made noff from these lengths)
        for (uint64_t t = threadIdx.x; t < len; t += THREADS) {
            k.nh[n0 + t] = k.rh[o0 + t];
            if (k.rcnt) k.ncnt[n0 + t] = k.rcnt[o0 + t];
        }
        if (threadIdx.x == 0) {
            k.nlast[s] = k.rlast[r], k.nmax[s] = k.rmax[r], k.nlen[s] = k.rlen[r], k.nflag[s] = k.rflag[r];
            k.nscale[s] = k.rscale[r];
        }
    }
}

// grid: x = query of the chunk.  256 query hashes at a time: thread t finds the posting run of hash t, the run lengths are
// scanned, and the postings of all 256 runs -- disjoint, the hashes being distinct: fewer than 2^32 in all -- are dealt flat
// over the threads.
__global__ void __launch_bounds__(THREADS) k_index_count(IndexArgs a) {
    __shared__ uint32_t s_lo[THREADS], s_start[THREADS], s_wsum[WAVES], s_tcount;
    const uint32_t qi = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t nqh = (uint32_t)(a.qoff[qi + 1] - a.qoff[qi]);
    const uint64_t *Q = a.qh + (a.qoff[qi] - a.qbase);
    uint32_t *cnt = a.cnt + (uint64_t)qi * a.nr, *touched = a.touched + (uint64_t)qi * a.nr;
    if (threadIdx.x == 0) s_tcount = 0;
    for (uint64_t base = 0; base < nqh; base += THREADS) { // (whole workgroups go round: the barriers see every thread)
        const uint64_t t = base + threadIdx.x;
        uint32_t lo = 0, len = 0;
        if (t < nqh) {
            const uint64_t x = Q[t];
            lo = count_below<false>(a.keys, a.n_post, a.post_top, x);
            len = count_below<true>(a.keys, a.n_post, a.post_top, x) - lo;
        }
        uint32_t inc = len; // inclusive scan over the wave, then over the four waves
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = __shfl_up(inc, o, 64);
            if ((int)lane >= o) inc += v;
        }
        if (lane == 63) s_wsum[wave] = inc;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < WAVES; ++w) {
            before += w < wave ? s_wsum[w] : 0;
            total += s_wsum[w];
        }
        s_lo[threadIdx.x] = lo;
        s_start[threadIdx.x] = before + inc - len;
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < total; k += THREADS) {
            // posting k of the batch is in the last run that starts at or before k (empty runs share their start with the next
            // run and come before it; s_start[0] = 0)
            uint32_t run = 0;
            for (uint32_t step = THREADS / 2; step; step >>= 1) run = s_start[run + step] <= k ? run + step : run;
            const uint32_t r = a.vals[s_lo[run] + (k - s_start[run])];
            if (r < a.nr && atomicAdd(&cnt[r], 1u) == 0) {
                const uint32_t slot = atomicAdd(&s_tcount, 1u); // (at most once per reference: below nr)
                if (slot < a.nr) touched[slot] = r;
            }
        }
        __syncthreads(); // the next batch writes s_lo, s_start and s_wsum again
    }
    __syncthreads();
    if (threadIdx.x == 0) a.tcount[qi] = min(s_tcount, a.nr);
}

// grid: x = query of the chunk.  Per touched pair: c, and 0 back; i0 = #{q <= max R}, j0 = #{r <= max Q} and the scale step as
// k_dist_counts has them (c > 0: neither side is empty); the entry where the containment passes, appended as k_search_all
// appends: one atomic per wave, the lanes' ranks by mbcnt.
__global__ void __launch_bounds__(THREADS) k_index_finish(IndexArgs a) {
    const uint32_t qi = blockIdx.x, n = a.tcount[qi];
    const uint32_t nqh = (uint32_t)(a.qoff[qi + 1] - a.qoff[qi]);
    const uint64_t *Q = a.qh + (a.qoff[qi] - a.qbase);
    const uint32_t qtop = top_of(nqh);
    const uint64_t max_q = nqh ? Q[nqh - 1] : 0;
    uint32_t *cnt = a.cnt + (uint64_t)qi * a.nr;
    const uint32_t *touched = a.touched + (uint64_t)qi * a.nr;
    for (uint32_t base = 0; base < n; base += THREADS) { // (whole waves go round: the ballot sees every lane)
        const uint32_t t = base + threadIdx.x;
        uint32_t r = 0, c = 0, i = 0, j = 0;
        bool pass = false;
        if (t < n) {
            r = touched[t];
            c = cnt[r];
            cnt[r] = 0;
            const uint32_t nrh = a.rlen[r];
            if (nqh && nrh) {
                const uint64_t *R = a.rh + a.roff[r];
                const uint32_t rtop = top_of(nrh);
                i = count_below<true>(Q, nqh, qtop, a.rlast[r]);
                j = count_below<true>(R, nrh, rtop, max_q);
                uint64_t m = 0;
                if (pair_max_hash(a, qi, r, m)) {
                    i = max(i, count_below<false>(Q, nqh, qtop, m));
                    j = max(j, count_below<false>(R, nrh, rtop, m));
                }
            }
            pass = containment_of(c, j) >= a.min_c;
        }
        const uint64_t mask = __ballot(pass);
        if (!mask) continue;
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        uint32_t first = 0;
        if (pass && rank == 0) first = atomicAdd(a.cursor, (uint32_t)__popcll(mask));
        first = __shfl(first, __ffsll((unsigned long long)mask) - 1, 64);
        if (pass && first + rank < a.sel_cap) { // (the host sized the list to the chunk's touched pairs)
            uint32_t *e = a.sel + (uint64_t)(first + rank) * 5;
            e[0] = a.q0 + qi, e[1] = r, e[2] = c, e[3] = i, e[4] = j;
        }
    }
}

// grid: x = query of the chunk.  finch_index_dist's finish: per touched pair c, and 0 back, as above; new mode completes (i, j)
// as k_index_finish does, old mode has total = |R| and no bound search (old_distance: c = |Q n R| for ascending hashes).  The
// pair's jaccard is the division distance_from_counts makes on the host; the entry (q, r, c, i, j) -- old mode: i = |R|, j = 0 --
// is appended where it reaches jmin[q], the host's conservative bound for the query's k and the call's max_distance: the host
// makes the decision, with its own log.
__global__ void __launch_bounds__(THREADS) k_index_dist_finish(IndexArgs a, const double *jmin, uint32_t old_mode) {
    const uint32_t qi = blockIdx.x, n = a.tcount[qi];
    const uint32_t nqh = (uint32_t)(a.qoff[qi + 1] - a.qoff[qi]);
    const uint64_t *Q = a.qh + (a.qoff[qi] - a.qbase);
    const uint32_t qtop = top_of(nqh);
    const uint64_t max_q = nqh ? Q[nqh - 1] : 0;
    const double jm = jmin[qi];
    uint32_t *cnt = a.cnt + (uint64_t)qi * a.nr;
    const uint32_t *touched = a.touched + (uint64_t)qi * a.nr;
    for (uint32_t base = 0; base < n; base += THREADS) { // (whole waves go round: the ballot sees every lane)
        const uint32_t t = base + threadIdx.x;
        uint32_t r = 0, c = 0, i = 0, j = 0;
        bool pass = false;
        if (t < n) {
            r = touched[t];
            c = cnt[r];
            cnt[r] = 0;
            const uint32_t nrh = a.rlen[r];
            if (old_mode) {
                i = nrh;
            } else if (nqh && nrh) {
                const uint64_t *R = a.rh + a.roff[r];
                const uint32_t rtop = top_of(nrh);
                i = count_below<true>(Q, nqh, qtop, a.rlast[r]);
                j = count_below<true>(R, nrh, rtop, max_q);
                uint64_t m = 0;
                if (pair_max_hash(a, qi, r, m)) {
                    i = max(i, count_below<false>(Q, nqh, qtop, m));
                    j = max(j, count_below<false>(R, nrh, rtop, m));
                }
            }
            pass = jaccard_of(old_mode != 0, c, i, j) >= jm;
        }
        const uint64_t mask = __ballot(pass);
        if (!mask) continue;
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        uint32_t first = 0;
        if (pass && rank == 0) first = atomicAdd(a.cursor, (uint32_t)__popcll(mask));
        first = __shfl(first, __ffsll((unsigned long long)mask) - 1, 64);
        if (pass && first + rank < a.sel_cap) { // (the host sized the list to the chunk's touched pairs)
            uint32_t *e = a.sel + (uint64_t)(first + rank) * 5;
            e[0] = a.q0 + qi, e[1] = r, e[2] = c, e[3] = i, e[4] = j;
        }
    }
}

// ---- finch_index_cluster -----------------------------------------------------------------------------------------------
// A lock-free union-find over the references, one word each.  What holds at every moment, whatever the lanes'
// order:
//   (1) parent[v] <= v;
//   (2) a word that has stopped being a root (parent[v] < v) never becomes one again, and only ever moves to a smaller member
//       of its own tree -- an ancestor it had;
//   (3) a root (parent[v] == v) is only ever changed by the one atomicCAS(&parent[v], v, lo) of cluster_unite, lo < v a root
//       of another tree when it was read.
// So trees only merge, a walk up the parents descends and ends by itself, no lane waits for another, and the root of a tree is
// its smallest member: when every union has run, the root of a component is its smallest index whatever the order was.  Every
// value a read can return -- a stale one included -- is one the word has held, and (1)-(3) make each of those as good as the
// newest for a walk: what a stale read costs is a CAS that fails.  The word is the data: no payload, no fence.

// every read of parent inside the finish: relaxed, agent scope -- not a value kept in a register, not a line of this CU's L1
__device__ inline uint32_t cluster_parent(const uint32_t *parent, uint32_t v) {
    return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// v's root as far as this lane can see, halving the path on the way: parent[v] to the grandparent by atomicMin, which keeps (2)
// against a lane that has moved it further meanwhile.  Every index read is below v: inside parent[0 .. nr).
__device__ inline uint32_t cluster_root(uint32_t *parent, uint32_t v) {
    for (;;) {
        const uint32_t p = cluster_parent(parent, v);
        if (p >= v) return v;
        const uint32_t g = cluster_parent(parent, p);
        if (g < p) atomicMin(&parent[v], g);
        v = p;
    }
}

// the larger root under the smaller by one CAS; a CAS that fails returns the word's value -- the root has a parent now --, and
// the loop goes round from there: the larger of the two indices falls with every round, so it ends.
__device__ inline void cluster_unite(uint32_t *parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = cluster_root(parent, a), b = cluster_root(parent, b);
        if (a == b) return;
        const uint32_t hi = max(a, b), lo = min(a, b);
        const uint32_t seen = atomicCAS(&parent[hi], hi, lo);
        if (seen == hi) return;
        a = seen, b = lo;
    }
}

// grid: x = query of the chunk (pairwise: the library's own sketch q0 + x).  finch_index_cluster's finish, k_index_dist_finish's
// sibling: per touched pair c, and 0 back, (i, j) and the jaccard as there.  Then three bands: jaccard >= jhi[q], or jaccard 1
// -- distance exactly 0 at every k --: sure, q and r are united here and nothing crosses; jaccard < jlo[q]: dropped; between:
// (q, r, c, i, j) is appended as k_index_dist_finish appends it, for the host's exact test.  A self pair is neither united nor
// counted.  *united: the sure pairs with q != r, added once per wave as the cursor is.
__global__ void __launch_bounds__(THREADS) k_index_cluster_finish(IndexArgs a, const double *jlo, const double *jhi, uint32_t old_mode,
                                                                  uint32_t *parent, unsigned long long *united) {
    const uint32_t qi = blockIdx.x, n = a.tcount[qi];
    const uint32_t nqh = (uint32_t)(a.qoff[qi + 1] - a.qoff[qi]);
    const uint64_t *Q = a.qh + (a.qoff[qi] - a.qbase);
    const uint32_t qtop = top_of(nqh);
    const uint64_t max_q = nqh ? Q[nqh - 1] : 0;
    const double jl = jlo[qi], jh = jhi[qi];
    const uint32_t q = a.q0 + qi;
    uint32_t *cnt = a.cnt + (uint64_t)qi * a.nr;
    const uint32_t *touched = a.touched + (uint64_t)qi * a.nr;
    for (uint32_t base = 0; base < n; base += THREADS) { // (whole waves go round: the ballots see every lane)
        const uint32_t t = base + threadIdx.x;
        uint32_t r = 0, c = 0, i = 0, j = 0;
        bool sure = false, band = false;
        if (t < n) {
            r = touched[t];
            c = cnt[r];
            cnt[r] = 0;
            const uint32_t nrh = a.rlen[r];
            if (old_mode) {
                i = nrh;
            } else if (nqh && nrh) {
                const uint64_t *R = a.rh + a.roff[r];
                const uint32_t rtop = top_of(nrh);
                i = count_below<true>(Q, nqh, qtop, a.rlast[r]);
                j = count_below<true>(R, nrh, rtop, max_q);
                uint64_t m = 0;
                if (pair_max_hash(a, qi, r, m)) {
                    i = max(i, count_below<false>(Q, nqh, qtop, m));
                    j = max(j, count_below<false>(R, nrh, rtop, m));
                }
            }
            const double jac = jaccard_of(old_mode != 0, c, i, j);
            sure = jac >= jh || jac == 1.0;
            band = !sure && jac >= jl;
        }
        const bool mine = sure && q != r && q < a.nr; // (q < nr: pairwise; r < nr: k_index_count)
        if (mine) cluster_unite(parent, q, r);
        const uint64_t done = __ballot(mine);
        if (done && (threadIdx.x & 63) == (uint32_t)(__ffsll((unsigned long long)done) - 1))
            atomicAdd(united, (unsigned long long)__popcll(done));
        const uint64_t mask = __ballot(band);
        if (!mask) continue;
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        uint32_t first = 0;
        if (band && rank == 0) first = atomicAdd(a.cursor, (uint32_t)__popcll(mask));
        first = __shfl(first, __ffsll((unsigned long long)mask) - 1, 64);
        if (band && first + rank < a.sel_cap) { // (the host sized the list to the chunk's touched pairs)
            uint32_t *e = a.sel + (uint64_t)(first + rank) * 5;
            e[0] = q, e[1] = r, e[2] = c, e[3] = i, e[4] = j;
        }
    }
}

// grid: x = block of references.  After an entry's last chunk: labels[v] = v's root, a walk that reads only -- the kernel
// boundary has made every finish kernel's atomics visible --, into an array of its own: 4 bytes per reference cross.
__global__ void __launch_bounds__(THREADS) k_index_cluster_labels(const uint32_t *parent, uint32_t nr, uint32_t *labels) {
    for (uint64_t v = (uint64_t)blockIdx.x * THREADS + threadIdx.x; v < nr; v += (uint64_t)gridDim.x * THREADS) {
        uint32_t x = (uint32_t)v, p;
        while ((p = parent[x]) < x) x = p; // ((1): every index read is below v)
        labels[v] = x;
    }
}

// ---- finch_index_gather ------------------------------------------------------------------------------------------------

constexpr uint32_t ROUND_THREADS = 1024, ROUND_WAVES = ROUND_THREADS / 64;
constexpr uint32_t NONE = 0xffffffffu;
// bits of the error word: a counter decremented at 0; a round that cleared another number of bits than its winner's counter
// said; a winner whose counter is not 0 after its round; a query with candidates that is longer than the launch's mask
constexpr uint32_t GERR_UNDERFLOW = 1, GERR_CLEARED = 2, GERR_WINNER = 4, GERR_MASK = 8;

struct IndexGatherArgs {
    uint32_t min_overlap, max_rounds;
    const uint32_t *qcnt;     // the chunk's counts, parallel to qh
    GatherCand *list;         // k_index_gather_candidates: the chunk's list, list_cap entries, and its cursor (zero before)
    uint32_t list_cap;
    uint32_t *cursor;
    const uint2 *cand;        // k_index_gather_rounds: the chunk's candidates (r, common) by (q, r) ...
    const uint32_t *cand_off; // ... query q0 + b's are cand[cand_off[b] .. cand_off[b + 1])
    GatherRecord *rec;
    uint32_t rec_cap;
    uint32_t *rec_cursor;     // zero before the launch
    uint32_t *err;            // zero before the launch
    uint32_t mask_words;      // the launch's dynamic LDS, in u32
};

// grid: x = query of the chunk.  Per touched pair c is read and the counter LEFT AS IT IS: the rounds go on from it.  The entry
// (q, r, c) where c >= min_overlap, appended as k_index_finish appends.
__global__ void __launch_bounds__(THREADS) k_index_gather_candidates(IndexArgs a, IndexGatherArgs g) {
    const uint32_t qi = blockIdx.x, n = a.tcount[qi];
    const uint32_t *cnt = a.cnt + (uint64_t)qi * a.nr;
    const uint32_t *touched = a.touched + (uint64_t)qi * a.nr;
    for (uint32_t base = 0; base < n; base += THREADS) { // (whole waves go round: the ballot sees every lane)
        const uint32_t t = base + threadIdx.x;
        uint32_t r = 0, c = 0;
        if (t < n) {
            r = touched[t];
            c = r < a.nr ? cnt[r] : 0;
        }
        const bool pass = t < n && c >= g.min_overlap;
        const uint64_t mask = __ballot(pass);
        if (!mask) continue;
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        uint32_t first = 0;
        if (pass && rank == 0) first = atomicAdd(g.cursor, (uint32_t)__popcll(mask));
        first = __shfl(first, __ffsll((unsigned long long)mask) - 1, 64);
        if (pass && first + rank < g.list_cap) { // (the host sized the list to the chunk's touched pairs)
            GatherCand e;
            e.q = a.q0 + qi, e.r = r, e.common = c;
            g.list[first + rank] = e;
        }
    }
}

// grid: x = query of the chunk.  finch_index_compare_counts' selection: per touched pair c, and 0 back -- the
// counters are clean after this kernel, whatever the moment walk does --; the entry (q, r, c) where c >= min_common, appended as
// k_index_finish appends.
__global__ void __launch_bounds__(THREADS) k_index_moments_select(IndexArgs a, uint32_t min_common, IndexPass *list, uint32_t list_cap,
                                                                  uint32_t *cursor) {
    const uint32_t qi = blockIdx.x, n = a.tcount[qi];
    uint32_t *cnt = a.cnt + (uint64_t)qi * a.nr;
    const uint32_t *touched = a.touched + (uint64_t)qi * a.nr;
    for (uint32_t base = 0; base < n; base += THREADS) { // (whole waves go round: the ballot sees every lane)
        const uint32_t t = base + threadIdx.x;
        uint32_t r = 0, c = 0;
        if (t < n) {
            r = touched[t];
            if (r < a.nr) c = cnt[r], cnt[r] = 0;
        }
        const bool pass = t < n && c >= min_common; // (min_common >= 1: a c of 0 never passes)
        const uint64_t mask = __ballot(pass);
        if (!mask) continue;
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        uint32_t first = 0;
        if (pass && rank == 0) first = atomicAdd(cursor, (uint32_t)__popcll(mask));
        first = __shfl(first, __ffsll((unsigned long long)mask) - 1, 64);
        if (pass && first + rank < list_cap) { // (the host sized the list to the chunk's touched pairs)
            IndexPass e;
            e.q = a.q0 + qi, e.r = r, e.c = c;
            list[first + rank] = e;
        }
    }
}

enum { W_BOUND = 0, W_WIN = 1, W_COUNT = 2, W_REF = 3, W_LEN = 4, W_N = 5 };

// (count descending, candidate ascending): does (c2, i2) come before (c1, i1)?  NONE is no candidate
__device__ inline bool gather_better(uint32_t c2, uint32_t i2, uint32_t c1, uint32_t i1) {
    return i2 != NONE && (i1 == NONE || c2 > c1 || (c2 == c1 && i2 < i1));
}

// grid: x = query of the chunk; dynamic LDS: g.mask_words u32, one bit per hash of the longest of the chunk's queries that have
// candidates.  A query without candidates runs no round and touches no mask: it may be longer than the mask.  Every branch
// that holds a barrier is taken on an LDS word every thread reads (s_word; fh_batch_large.hip's rule).
__global__ void __launch_bounds__(ROUND_THREADS) k_index_gather_rounds(IndexArgs a, IndexGatherArgs g) {
    extern __shared__ uint32_t s_mask[];
    __shared__ uint32_t s_lo[ROUND_THREADS], s_start[ROUND_THREADS], s_wsum[ROUND_WAVES];
    __shared__ uint32_t s_cnt[ROUND_WAVES], s_idx[ROUND_WAVES], s_clr[ROUND_WAVES];
    __shared__ uint64_t s_ab[ROUND_WAVES];
    __shared__ uint32_t s_word[W_N];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t qi = blockIdx.x;
    const uint32_t nqh = (uint32_t)(a.qoff[qi + 1] - a.qoff[qi]);
    const uint64_t *Q = a.qh + (a.qoff[qi] - a.qbase);
    const uint32_t *QC = g.qcnt + (a.qoff[qi] - a.qbase);
    const uint32_t qtop = top_of(nqh);
    const uint32_t c0 = g.cand_off[qi], ncand = g.cand_off[qi + 1] - c0;
    const uint2 *cand = g.cand + c0;
    uint32_t *cnt = a.cnt + (uint64_t)qi * a.nr;
    const bool fits = (nqh + 31) / 32 <= g.mask_words;
    uint32_t bad = 0;
    if (ncand && fits) // (no barrier inside; the host sized the mask for every query that gets here)
        for (uint32_t w = tid; w < (nqh + 31) / 32; w += ROUND_THREADS) s_mask[w] = w * 32 + 32 <= nqh ? ~0u : (1u << (nqh & 31)) - 1;
    if (tid == 0) {
        if (ncand && !fits) bad |= GERR_MASK;
        s_word[W_BOUND] = !fits ? 0 : g.max_rounds ? min(g.max_rounds, ncand) : ncand;
    }
    __syncthreads();
    const uint32_t bound = s_word[W_BOUND];
    uint32_t remaining = nqh;
    for (uint32_t t = 0; t < bound; ++t) {
        // the arg-max over the live counters.  Other waves' atomics have changed them at L2 since this thread last read them:
        // an agent-scope atomic load, so that nothing rests on what the CU's vector cache holds of such a line
        uint32_t best_c = 0, best_i = NONE;
        for (uint32_t i = tid; i < ncand; i += ROUND_THREADS) { // (i ascends: among equal counts the first stays)
            const uint32_t r = cand[i].x;
            const uint32_t c = r < a.nr ? __hip_atomic_load(&cnt[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
            if (c >= g.min_overlap && c > best_c) best_c = c, best_i = i;
        }
        for (int o = 32; o; o >>= 1) {
            const uint32_t c2 = __shfl_xor(best_c, o, 64), i2 = __shfl_xor(best_i, o, 64);
            if (gather_better(c2, i2, best_c, best_i)) best_c = c2, best_i = i2;
        }
        if (lane == 0) s_cnt[wave] = best_c, s_idx[wave] = best_i;
        __syncthreads();
        if (tid == 0) {
            uint32_t wc = 0, wi = NONE;
            for (uint32_t w = 0; w < ROUND_WAVES; ++w)
                if (gather_better(s_cnt[w], s_idx[w], wc, wi)) wc = s_cnt[w], wi = s_idx[w];
            const uint32_t r = wi != NONE ? cand[wi].x : 0;
            s_word[W_WIN] = wi; // NONE: no candidate reaches min_overlap
            s_word[W_COUNT] = wc;
            s_word[W_REF] = r;
            s_word[W_LEN] = wi != NONE ? a.rlen[r] : 0;
        }
        __syncthreads();
        const uint32_t wi = s_word[W_WIN], wc = s_word[W_COUNT], wr = s_word[W_REF], nrh = s_word[W_LEN];
        if (wi == NONE) break; // the same LDS word in every thread
        // S_{t+1} = S_t \ H_w.  1024 of the winner's hashes at a time: thread t looks hash t up in the query; a hit whose bit is
        // set clears it, adds the query's count of it and finds the hash's posting run; the runs are scanned and dealt flat over
        // the workgroup as k_index_count deals them, one decrement per posting
        const uint64_t *R = a.rh + a.roff[wr];
        uint64_t ab = 0;
        uint32_t clr = 0;
        for (uint32_t base = 0; base < nrh; base += ROUND_THREADS) { // (nrh: an LDS word; whole workgroups go round)
            const uint32_t k0 = base + tid;
            uint32_t lo = 0, len = 0;
            if (k0 < nrh) {
                const uint64_t x = R[k0];
                const uint32_t p = count_below<true>(Q, nqh, qtop, x);
                if (p && Q[p - 1] == x) {
                    const uint32_t bit = 1u << ((p - 1) & 31);
                    if (atomicAnd(&s_mask[(p - 1) >> 5], ~bit) & bit) {
                        ab += QC[p - 1], ++clr;
                        lo = count_below<false>(a.keys, a.n_post, a.post_top, x);
                        len = count_below<true>(a.keys, a.n_post, a.post_top, x) - lo;
                    }
                }
            }
            uint32_t inc = len; // inclusive scan over the wave, then over the sixteen waves
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t v = __shfl_up(inc, o, 64);
                if ((int)lane >= o) inc += v;
            }
            if (lane == 63) s_wsum[wave] = inc;
            __syncthreads();
            uint32_t before = 0, total = 0;
            for (uint32_t w = 0; w < ROUND_WAVES; ++w) {
                before += w < wave ? s_wsum[w] : 0;
                total += s_wsum[w];
            }
            s_lo[tid] = lo;
            s_start[tid] = before + inc - len;
            __syncthreads();
            for (uint32_t k = tid; k < total; k += ROUND_THREADS) {
                // posting k of the batch is in the last run that starts at or before k (k_index_count's search)
                uint32_t run = 0;
                for (uint32_t step = ROUND_THREADS / 2; step; step >>= 1) run = s_start[run + step] <= k ? run + step : run;
                const uint32_t r = a.vals[s_lo[run] + (k - s_start[run])];
                if (r < a.nr && atomicSub(&cnt[r], 1u) == 0) bad |= GERR_UNDERFLOW;
            }
            __syncthreads(); // the next batch writes s_lo, s_start and s_wsum again; every decrement of this one has landed
        }
        for (int o = 32; o; o >>= 1) ab += __shfl_xor(ab, o, 64), clr += __shfl_xor(clr, o, 64);
        if (lane == 0) s_ab[wave] = ab, s_clr[wave] = clr;
        __syncthreads();
        remaining -= wc;
        if (tid == 0) {
            uint64_t abund = 0;
            uint32_t cleared = 0;
            for (uint32_t w = 0; w < ROUND_WAVES; ++w) abund += s_ab[w], cleared += s_clr[w];
            if (cleared != wc) bad |= GERR_CLEARED;
            if (__hip_atomic_load(&cnt[wr], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) bad |= GERR_WINNER;
            GatherRecord rec;
            rec.q = a.q0 + qi, rec.r = wr, rec.round = t, rec.overlap = wc, rec.common = cand[wi].y;
            rec.ref_len = nrh, rec.query_len = nqh, rec.remaining = remaining, rec.abund = abund, rec.cand = wi, rec.pad = 0;
            const uint32_t at = atomicAdd(g.rec_cursor, 1u);
            if (at < g.rec_cap) g.rec[at] = rec;
        }
    }
    if (bad) atomicOr(g.err, bad);
    // the tail, for every query, with or without candidates, whatever the error word says: 0 to the counter of every touched
    // reference -- non-candidates were touched and decremented too --, so the index is clean for the next launch
    __syncthreads();
    const uint32_t n = a.tcount[qi];
    const uint32_t *touched = a.touched + (uint64_t)qi * a.nr;
    for (uint32_t i = tid; i < n; i += ROUND_THREADS) {
        const uint32_t r = touched[i];
        if (r < a.nr) cnt[r] = 0;
    }
}

} // namespace

namespace fh {

// what an update has built beside the arrays in use, until index_commit swaps it in or index_discard drops it
struct IndexStage {
    bool ready = false;
    uint32_t nr = 0, n_post = 0, chunk = 0;
    void *lib[9] = {};
    uint32_t *rcnt = nullptr, *cnt = nullptr, *touched = nullptr, *tcount = nullptr, *back_h = nullptr;
    std::vector<uint32_t> rlen_h;
};

struct IndexDevice {
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t nr = 0, n_post = 0, chunk = 0;
    void *lib[9] = {};            // rh roff rlast rmax rlen rflag rscale keys vals
    void *qry[5] = {};            // qh qoff qmax qflag qscale, grown to the largest chunk so far
    size_t qry_hashes = 0;        // u64 that qry[0] holds
    uint32_t *cnt = nullptr, *touched = nullptr, *tcount = nullptr, *cursor = nullptr, *sel = nullptr;
    uint64_t sel_cap = 0;         // entries that sel holds
    uint32_t *back_h = nullptr;   // pinned: chunk touched-list lengths, then the cursor
    double *jmin = nullptr;       // finch_index_dist: the chunk's jaccard bounds, one per query (allocated by its first chunk)
    // finch_index_cluster, from index_cluster_begin to index_cluster_end: the chunk's upper bounds, the union-find's nr words and
    // the labels' nr, the count of united pairs
    double *jhi = nullptr;
    uint32_t *parent = nullptr, *labels = nullptr;
    unsigned long long *united = nullptr;
    // finch_index_gather, grown as needed: the chunk's counts, its list of (q, r, common), the candidates (r, common) by (q, r),
    // each query's range of them, the records; two words -- the records' cursor, the error word -- and their pinned copy
    void *gat[5] = {};
    size_t gat_cap[5] = {};
    uint32_t *gwords = nullptr, *gwords_h = nullptr;
    // finch_index_compare_counts: the library's counts, parallel to lib[0] (finch_index_attach_counts; none until then); grown as
    // needed: the chunk's counts, its pass list of (q, r, c), the records; the error word with the pair it names, and their
    // pinned copy
    uint32_t *rcnt = nullptr;
    void *cmp[3] = {};
    size_t cmp_cap[3] = {};
    uint32_t *cwords = nullptr, *cwords_h = nullptr;
    bool rounds_lds_set = false;  // k_index_gather_rounds may ask for more dynamic LDS than a launch gets unasked
    std::vector<uint32_t> rlen_h; // the library's lengths: what a candidate's `common` is checked against
    hipEvent_t ev[6] = {};
    bool dirty = false;           // a launch failed between the count and the finish: the counters are not known to be zero
    IndexStage next;              // index_add / index_keep: the arrays of the updated library
};

// frees what a stage holds; the device is current
static void stage_drop(IndexStage *s) {
    for (void *p : s->lib)
        if (p) (void)hipFree(p);
    for (uint32_t *p : {s->rcnt, s->cnt, s->touched, s->tcount})
        if (p) (void)hipFree(p);
    if (s->back_h) (void)hipHostFree(s->back_h);
    *s = IndexStage();
}

// frees what a cluster call holds; the device is current
static void cluster_drop(IndexDevice *d) {
    if (d->jhi) (void)hipFree(d->jhi);
    if (d->parent) (void)hipFree(d->parent);
    if (d->labels) (void)hipFree(d->labels);
    if (d->united) (void)hipFree(d->united);
    d->jhi = nullptr, d->parent = d->labels = nullptr, d->united = nullptr;
}

// what finch_index_screen reads (fh_screen.h): the arrays in use now -- after an update, the updated library's
void index_screen_view(IndexDevice *d, ScreenView *v) {
    v->rh = (const uint64_t *)d->lib[0], v->roff = (const uint64_t *)d->lib[1];
    v->keys = (const uint64_t *)d->lib[7], v->vals = (const uint32_t *)d->lib[8];
    v->nr = d->nr, v->n_post = d->n_post;
    v->device = d->device;
    v->stream = (void *)d->stream;
}

void index_close(IndexDevice *d) {
    if (!d) return;
    if (hipSetDevice(d->device) == hipSuccess) {
        if (d->stream) (void)hipStreamSynchronize(d->stream);
        stage_drop(&d->next);
        for (void *p : d->lib)
            if (p) (void)hipFree(p);
        for (void *p : d->qry)
            if (p) (void)hipFree(p);
        for (uint32_t *p : {d->cnt, d->touched, d->tcount, d->cursor, d->sel})
            if (p) (void)hipFree(p);
        if (d->jmin) (void)hipFree(d->jmin);
        cluster_drop(d);
        for (void *p : d->gat)
            if (p) (void)hipFree(p);
        if (d->gwords) (void)hipFree(d->gwords);
        if (d->rcnt) (void)hipFree(d->rcnt);
        for (void *p : d->cmp)
            if (p) (void)hipFree(p);
        if (d->cwords) (void)hipFree(d->cwords);
        if (d->cwords_h) (void)hipHostFree(d->cwords_h);
        if (d->gwords_h) (void)hipHostFree(d->gwords_h);
        if (d->back_h) (void)hipHostFree(d->back_h);
        for (hipEvent_t e : d->ev)
            if (e) (void)hipEventDestroy(e);
        if (d->stream) (void)hipStreamDestroy(d->stream);
    }
    (void)hipGetLastError();
    delete d;
}

static int upload(void **dst, const void *src, size_t bytes, uint64_t *total) {
    const size_t b = std::max<size_t>(bytes, 8); // (an empty array still gets a valid pointer)
    IHIP_TRY(api_dev_malloc(dst, b));
    if (bytes) IHIP_TRY(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
    *total += b;
    return FH_OK;
}

static int open_into(IndexDevice *d, const DistSide &r, uint64_t *device_bytes, double *build_ms) {
    IHIP_TRY(hipSetDevice(d->device));
    IHIP_TRY(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
    for (hipEvent_t &e : d->ev) IHIP_TRY(hipEventCreate(&e));
    const uint64_t P = r.offsets[r.n];
    std::vector<uint64_t> rlast(r.n);
    std::vector<uint32_t> rlen(r.n);
    for (uint32_t s = 0; s < r.n; ++s) {
        rlen[s] = (uint32_t)(r.offsets[s + 1] - r.offsets[s]);
        rlast[s] = rlen[s] ? r.hashes[r.offsets[s + 1] - 1] : 0;
    }
    d->rlen_h = rlen;
    uint64_t total = 0;
    if (int rc = upload(&d->lib[0], r.hashes, P * sizeof(uint64_t), &total)) return rc;
    if (int rc = upload(&d->lib[1], r.offsets, ((size_t)r.n + 1) * sizeof(uint64_t), &total)) return rc;
    if (int rc = upload(&d->lib[2], rlast.data(), r.n * sizeof(uint64_t), &total)) return rc;
    if (int rc = upload(&d->lib[3], r.max_hash, r.n * sizeof(uint64_t), &total)) return rc;
    if (int rc = upload(&d->lib[4], rlen.data(), r.n * sizeof(uint32_t), &total)) return rc;
    if (int rc = upload(&d->lib[5], r.flags, r.n * sizeof(uint32_t), &total)) return rc;
    if (int rc = upload(&d->lib[6], r.scale, r.n * sizeof(double), &total)) return rc;
    IHIP_TRY(api_dev_malloc(&d->lib[7], P * sizeof(uint64_t)));
    IHIP_TRY(api_dev_malloc(&d->lib[8], P * sizeof(uint32_t)));
    total += P * (sizeof(uint64_t) + sizeof(uint32_t));

    // the postings in reference order, then sorted by hash: the sort is stable, so a hash's references ascend
    struct Scratch {
        void *keys = nullptr, *vals = nullptr, *tmp = nullptr;
        ~Scratch() {
            for (void *p : {keys, vals, tmp})
                if (p) (void)hipFree(p);
        }
    } scratch;
    size_t tmp_bytes = 0;
    IHIP_TRY(big_sort_tmp_bytes(d->n_post, &tmp_bytes));
    IHIP_TRY(api_dev_malloc(&scratch.keys, P * sizeof(uint64_t)));
    IHIP_TRY(api_dev_malloc(&scratch.vals, P * sizeof(uint32_t)));
    IHIP_TRY(api_dev_malloc(&scratch.tmp, tmp_bytes));
    IHIP_TRY(hipEventRecord(d->ev[0], d->stream));
    hipLaunchKernelGGL(k_index_postings, dim3(std::min(d->nr, 4096u)), dim3(THREADS), 0, d->stream, (const uint64_t *)d->lib[0],
                       (const uint64_t *)d->lib[1], 0u, d->nr, (uint64_t *)d->lib[7], (uint32_t *)d->lib[8]);
    IHIP_TRY(hipGetLastError());
    IHIP_TRY(big_sort_pairs(scratch.tmp, tmp_bytes, (uint64_t *)d->lib[7], (uint64_t *)scratch.keys, (uint32_t *)d->lib[8],
                            (uint32_t *)scratch.vals, d->n_post, d->stream));
    IHIP_TRY(hipEventRecord(d->ev[1], d->stream));

    const size_t dense = (size_t)d->chunk * d->nr * sizeof(uint32_t);
    IHIP_TRY(api_dev_malloc((void **)&d->cnt, dense));
    IHIP_TRY(api_dev_malloc((void **)&d->touched, dense));
    IHIP_TRY(api_dev_malloc((void **)&d->tcount, d->chunk * sizeof(uint32_t)));
    IHIP_TRY(api_dev_malloc((void **)&d->cursor, sizeof(uint32_t)));
    IHIP_TRY(api_host_malloc((void **)&d->back_h, ((size_t)d->chunk + 1) * sizeof(uint32_t)));
    total += 2 * dense + ((size_t)d->chunk + 1) * sizeof(uint32_t);
    IHIP_TRY(hipMemsetAsync(d->cnt, 0, dense, d->stream)); // once: every search stores its zeros back
    IHIP_TRY(hipStreamSynchronize(d->stream));
    float ms = 0.f;
    IHIP_TRY(hipEventElapsedTime(&ms, d->ev[0], d->ev[1]));
    *build_ms = ms;
    *device_bytes = total;
    return FH_OK;
}

int index_open(int device, const DistSide &refs, uint32_t chunk_queries, IndexDevice **out, uint64_t *device_bytes, double *build_ms) {
    const uint64_t P = refs.offsets[refs.n];
    if (refs.n == 0 || P == 0 || P > INDEX_MAX_POSTINGS || chunk_queries == 0 || (uint64_t)chunk_queries * refs.n > (1ull << 31))
        return api_fail(FH_ERR_INVALID, "index_open: %u references, %llu postings, %u queries per launch", refs.n, (unsigned long long)P, chunk_queries);
    IndexDevice *d = new (std::nothrow) IndexDevice;
    if (!d) return api_fail(FH_ERR_CAPACITY, "out of host memory");
    d->device = device;
    d->nr = refs.n;
    d->n_post = (uint32_t)P;
    d->chunk = chunk_queries;
    if (int rc = open_into(d, refs, device_bytes, build_ms)) {
        index_close(d);
        return rc;
    }
    *out = d;
    return FH_OK;
}

// device memory of at least `bytes` at *p, which held `have`: the old block goes first
static int grow(void **p, size_t *have, size_t bytes) {
    if (*p && *have >= bytes) return FH_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr, *have = 0;
    IHIP_TRY(api_dev_malloc(p, std::max<size_t>(bytes, 8)));
    *have = bytes;
    return FH_OK;
}

// the queries [q0, q1) of `q` to the device (q = nullptr: the library's own sketches, which are there) and the argument block of
// the chunk's kernels
static int chunk_args(IndexDevice *d, const DistSide *q, uint32_t q0, uint32_t q1, IndexArgs *out) {
    const uint32_t n = q1 - q0;
    uint64_t h0 = 0;
    if (q) {
        h0 = q->offsets[q0];
        const uint64_t nh = q->offsets[q1] - h0;
        if (int rc = grow(&d->qry[0], &d->qry_hashes, nh * sizeof(uint64_t))) return rc;
        if (!d->qry[1]) { // the per-query arrays: a chunk never has more than d->chunk queries
            IHIP_TRY(api_dev_malloc(&d->qry[1], ((size_t)d->chunk + 1) * sizeof(uint64_t)));
            IHIP_TRY(api_dev_malloc(&d->qry[2], (size_t)d->chunk * sizeof(uint64_t)));
            IHIP_TRY(api_dev_malloc(&d->qry[3], (size_t)d->chunk * sizeof(uint32_t)));
            IHIP_TRY(api_dev_malloc(&d->qry[4], (size_t)d->chunk * sizeof(double)));
        }
        if (nh) IHIP_TRY(hipMemcpy(d->qry[0], q->hashes + h0, nh * sizeof(uint64_t), hipMemcpyHostToDevice));
        IHIP_TRY(hipMemcpy(d->qry[1], q->offsets + q0, ((size_t)n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
        IHIP_TRY(hipMemcpy(d->qry[2], q->max_hash + q0, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice));
        IHIP_TRY(hipMemcpy(d->qry[3], q->flags + q0, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
        IHIP_TRY(hipMemcpy(d->qry[4], q->scale + q0, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    }
    IndexArgs a;
    a.rh = (const uint64_t *)d->lib[0], a.roff = (const uint64_t *)d->lib[1], a.rlast = (const uint64_t *)d->lib[2];
    a.rmax = (const uint64_t *)d->lib[3], a.rlen = (const uint32_t *)d->lib[4], a.rflag = (const uint32_t *)d->lib[5];
    a.rscale = (const double *)d->lib[6], a.keys = (const uint64_t *)d->lib[7], a.vals = (const uint32_t *)d->lib[8];
    a.n_post = d->n_post, a.post_top = 1u << (31 - __builtin_clz(d->n_post)), a.nr = d->nr;
    if (q) {
        a.qh = (const uint64_t *)d->qry[0], a.qoff = (const uint64_t *)d->qry[1], a.qmax = (const uint64_t *)d->qry[2];
        a.qflag = (const uint32_t *)d->qry[3], a.qscale = (const double *)d->qry[4];
    } else { // the library's own CSR: hashes from 0 on, the per-sketch arrays from sketch q0 on (roff has nr + 1 entries)
        a.qh = a.rh, a.qoff = a.roff + q0, a.qmax = a.rmax + q0, a.qflag = a.rflag + q0, a.qscale = a.rscale + q0;
    }
    a.qbase = h0, a.q0 = q0;
    a.cnt = d->cnt, a.touched = d->touched, a.tcount = d->tcount;
    a.min_c = 0.;
    a.sel = d->sel, a.cursor = d->cursor, a.sel_cap = 0;
    *out = a;
    return FH_OK;
}

// one chunk of either route.  q = nullptr: the queries are the library's own sketches q0 .. q1 (pairwise), read where the index
// keeps them.  jmin = nullptr: the search's finish with min_containment; else finch_index_dist's with the chunk's bounds, or --
// jhi too -- finch_index_cluster's with both, over the call's union-find (index_cluster_begin).
static int run_chunk(IndexDevice *d, const DistSide *q, uint32_t q0, uint32_t q1, double min_containment, const double *jmin, const double *jhi,
                     bool old_mode, std::vector<uint32_t> *entries, uint64_t *touched, double *kernel_ms) {
    const uint32_t n = q1 - q0;
    IHIP_TRY(hipSetDevice(d->device));
    IndexArgs a;
    if (int rc = chunk_args(d, q, q0, q1, &a)) return rc;
    a.min_c = min_containment;
    if (jmin) {
        if (!d->jmin) IHIP_TRY(api_dev_malloc((void **)&d->jmin, (size_t)d->chunk * sizeof(double)));
        IHIP_TRY(hipMemcpy(d->jmin, jmin, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    }
    if (jhi) IHIP_TRY(hipMemcpy(d->jhi, jhi, (size_t)n * sizeof(double), hipMemcpyHostToDevice));

    // the count; the touched lists' lengths cross, so that the chunk's list can be sized to what may pass
    d->dirty = true; // until the finish has stored the zeros back
    IHIP_TRY(hipEventRecord(d->ev[0], d->stream));
    hipLaunchKernelGGL(k_index_count, dim3(n), dim3(THREADS), 0, d->stream, a);
    IHIP_TRY(hipGetLastError());
    IHIP_TRY(hipEventRecord(d->ev[1], d->stream));
    IHIP_TRY(hipMemcpyAsync(d->back_h, d->tcount, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
    IHIP_TRY(hipStreamSynchronize(d->stream));
    uint64_t pairs = 0;
    for (uint32_t i = 0; i < n; ++i) pairs += d->back_h[i];
    float ms = 0.f;
    IHIP_TRY(hipEventElapsedTime(&ms, d->ev[0], d->ev[1]));
    *kernel_ms += ms;
    *touched += pairs;
    if (pairs == 0) { // (nothing was counted: nothing to store back)
        d->dirty = false;
        return FH_OK;
    }
    if (d->sel_cap < pairs) { // (pairs <= chunk x nr <= 2^31: index_open)
        size_t have = d->sel_cap * 5 * sizeof(uint32_t);
        const uint64_t want = std::max<uint64_t>(pairs, std::min<uint64_t>(2 * d->sel_cap, (uint64_t)d->chunk * d->nr));
        if (int rc = grow((void **)&d->sel, &have, want * 5 * sizeof(uint32_t))) {
            d->sel_cap = 0;
            return rc;
        }
        d->sel_cap = have / (5 * sizeof(uint32_t));
    }
    a.sel = d->sel, a.sel_cap = (uint32_t)d->sel_cap;

    IHIP_TRY(hipMemsetAsync(d->cursor, 0, sizeof(uint32_t), d->stream));
    IHIP_TRY(hipEventRecord(d->ev[2], d->stream));
    if (jhi)
        hipLaunchKernelGGL(k_index_cluster_finish, dim3(n), dim3(THREADS), 0, d->stream, a, (const double *)d->jmin, (const double *)d->jhi,
                           old_mode ? 1u : 0u, d->parent, d->united);
    else if (jmin) hipLaunchKernelGGL(k_index_dist_finish, dim3(n), dim3(THREADS), 0, d->stream, a, (const double *)d->jmin, old_mode ? 1u : 0u);
    else hipLaunchKernelGGL(k_index_finish, dim3(n), dim3(THREADS), 0, d->stream, a);
    IHIP_TRY(hipGetLastError());
    IHIP_TRY(hipEventRecord(d->ev[3], d->stream));
    IHIP_TRY(hipMemcpyAsync(d->back_h + d->chunk, d->cursor, sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
    IHIP_TRY(hipStreamSynchronize(d->stream));
    d->dirty = false;
    IHIP_TRY(hipEventElapsedTime(&ms, d->ev[2], d->ev[3]));
    *kernel_ms += ms;
    const uint32_t cursor = d->back_h[d->chunk];
    if (cursor > pairs) return api_fail(FH_ERR_STATE, "index search: %u entries from %llu pairs", cursor, (unsigned long long)pairs);
    const size_t at = entries->size();
    entries->resize(at + (size_t)cursor * 5);
    if (cursor) IHIP_TRY(hipMemcpy(entries->data() + at, d->sel, (size_t)cursor * 5 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return FH_OK;
}

int index_search_chunk(IndexDevice *d, const DistSide &queries, uint32_t q0, uint32_t q1, double min_containment,
                       std::vector<uint32_t> *entries, uint64_t *touched, double *kernel_ms) {
    if (q1 <= q0 || q1 > queries.n || q1 - q0 > d->chunk)
        return api_fail(FH_ERR_INVALID, "index_search_chunk: queries %u..%u of %u, %u per launch", q0, q1, queries.n, d->chunk);
    if (d->dirty) return api_fail(FH_ERR_STATE, "index search: an earlier search on this index failed between its two kernels; build the index again");
    return run_chunk(d, &queries, q0, q1, min_containment, nullptr, nullptr, false, entries, touched, kernel_ms);
}

int index_dist_chunk(IndexDevice *d, const DistSide *queries, uint32_t q0, uint32_t q1, bool old_mode, const double *jmin,
                     std::vector<uint32_t> *entries, uint64_t *touched, double *kernel_ms) {
    if (!jmin || q1 <= q0 || q1 > (queries ? queries->n : d->nr) || q1 - q0 > d->chunk)
        return api_fail(FH_ERR_INVALID, "index_dist_chunk: queries %u..%u of %u, %u per launch", q0, q1, queries ? queries->n : d->nr, d->chunk);
    if (d->dirty) return api_fail(FH_ERR_STATE, "index dist: an earlier call on this index failed between its two kernels; build the index again");
    return run_chunk(d, queries, q0, q1, 0., jmin, nullptr, old_mode, entries, touched, kernel_ms);
}

int index_cluster_begin(IndexDevice *d) {
    if (d->dirty) return api_fail(FH_ERR_STATE, "index cluster: an earlier call on this index failed between its two kernels; build the index again");
    IHIP_TRY(hipSetDevice(d->device));
    cluster_drop(d); // (what a failed call may have left)
    IHIP_TRY(api_dev_malloc((void **)&d->jhi, (size_t)d->chunk * sizeof(double)));
    IHIP_TRY(api_dev_malloc((void **)&d->parent, (size_t)d->nr * sizeof(uint32_t)));
    IHIP_TRY(api_dev_malloc((void **)&d->labels, (size_t)d->nr * sizeof(uint32_t)));
    IHIP_TRY(api_dev_malloc((void **)&d->united, sizeof(unsigned long long)));
    std::vector<uint32_t> identity(d->nr);
    for (uint32_t v = 0; v < d->nr; ++v) identity[v] = v;
    IHIP_TRY(hipMemcpy(d->parent, identity.data(), (size_t)d->nr * sizeof(uint32_t), hipMemcpyHostToDevice));
    IHIP_TRY(hipMemsetAsync(d->united, 0, sizeof(unsigned long long), d->stream)); // (in front of the first chunk's kernels)
    return FH_OK;
}

int index_cluster_chunk(IndexDevice *d, uint32_t q0, uint32_t q1, bool old_mode, const double *jlo, const double *jhi,
                        std::vector<uint32_t> *entries, uint64_t *touched, double *kernel_ms) {
    if (!jlo || !jhi || !d->parent || q1 <= q0 || q1 > d->nr || q1 - q0 > d->chunk)
        return api_fail(FH_ERR_INVALID, "index_cluster_chunk: queries %u..%u of %u, %u per launch", q0, q1, d->nr, d->chunk);
    if (d->dirty) return api_fail(FH_ERR_STATE, "index cluster: an earlier call on this index failed between its two kernels; build the index again");
    return run_chunk(d, nullptr, q0, q1, 0., jlo, jhi, old_mode, entries, touched, kernel_ms);
}

int index_cluster_end(IndexDevice *d, uint32_t *labels, uint64_t *united, double *kernel_ms) {
    if (hipSetDevice(d->device) != hipSuccess || !d->parent || !labels) { // (a call that failed: only the freeing)
        cluster_drop(d);
        (void)hipGetLastError();
        return labels ? api_fail(FH_ERR_STATE, "index_cluster_end: no cluster call is open on this index") : FH_OK;
    }
    struct Drop {
        IndexDevice *d;
        ~Drop() { cluster_drop(d); }
    } drop{d};
    IHIP_TRY(hipEventRecord(d->ev[0], d->stream));
    hipLaunchKernelGGL(k_index_cluster_labels, dim3(std::min((d->nr + THREADS - 1) / THREADS, 4096u)), dim3(THREADS), 0, d->stream,
                       (const uint32_t *)d->parent, d->nr, d->labels);
    IHIP_TRY(hipGetLastError());
    IHIP_TRY(hipEventRecord(d->ev[1], d->stream));
    IHIP_TRY(hipStreamSynchronize(d->stream));
    float ms = 0.f;
    IHIP_TRY(hipEventElapsedTime(&ms, d->ev[0], d->ev[1]));
    *kernel_ms += ms;
    unsigned long long n = 0;
    IHIP_TRY(hipMemcpy(labels, d->labels, (size_t)d->nr * sizeof(uint32_t), hipMemcpyDeviceToHost));
    IHIP_TRY(hipMemcpy(&n, d->united, sizeof n, hipMemcpyDeviceToHost));
    *united += n;
    return FH_OK;
}

// finch_index_gather's chunk: the count as above, the candidates, then every round of every query in one launch.
static int gather_chunk(IndexDevice *d, const DistSide &q, const uint32_t *counts, uint32_t q0, uint32_t q1, uint32_t min_overlap,
                        uint32_t max_rounds, std::vector<GatherCand> *cands, std::vector<GatherRecord> *recs, uint64_t *touched,
                        double *kernel_ms, uint64_t *launches) {
    const uint32_t n = q1 - q0;
    IHIP_TRY(hipSetDevice(d->device));
    IndexArgs a;
    if (int rc = chunk_args(d, &q, q0, q1, &a)) return rc;
    const uint64_t nh = q.offsets[q1] - a.qbase;
    if (int rc = grow(&d->gat[0], &d->gat_cap[0], nh * sizeof(uint32_t))) return rc;
    if (nh) IHIP_TRY(hipMemcpy(d->gat[0], counts + a.qbase, nh * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (int rc = grow(&d->gat[3], &d->gat_cap[3], ((size_t)n + 1) * sizeof(uint32_t))) return rc;
    if (!d->gwords) {
        IHIP_TRY(api_dev_malloc((void **)&d->gwords, 2 * sizeof(uint32_t)));
        IHIP_TRY(api_host_malloc((void **)&d->gwords_h, 2 * sizeof(uint32_t)));
    }
    if (!d->rounds_lds_set) { // the mask may take all of GATHER_MAX_QUERY bits: above the 64 KiB a launch gets unasked
        IHIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_index_gather_rounds), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)(GATHER_MAX_QUERY / 8)));
        d->rounds_lds_set = true;
    }
    IndexGatherArgs g{};
    g.min_overlap = std::max(min_overlap, 1u), g.max_rounds = max_rounds;
    g.qcnt = (const uint32_t *)d->gat[0];
    g.cursor = d->cursor;
    g.rec_cursor = d->gwords, g.err = d->gwords + 1;

    // 1. the count; the touched lists' lengths cross, so that the chunk's list can be sized to what may pass
    d->dirty = true; // until the rounds kernel's tail has stored the zeros back
    IHIP_TRY(hipEventRecord(d->ev[0], d->stream));
    hipLaunchKernelGGL(k_index_count, dim3(n), dim3(THREADS), 0, d->stream, a);
    IHIP_TRY(hipGetLastError());
    IHIP_TRY(hipEventRecord(d->ev[1], d->stream));
    IHIP_TRY(hipMemcpyAsync(d->back_h, d->tcount, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
    IHIP_TRY(hipStreamSynchronize(d->stream));
    uint64_t pairs = 0;
    for (uint32_t i = 0; i < n; ++i) pairs += d->back_h[i];
    *touched += pairs;

    // 2. the candidates: the cursor crosses, then that many entries (pairs <= chunk x nr <= 2^31: index_open)
    if (int rc = grow(&d->gat[1], &d->gat_cap[1], pairs * sizeof(GatherCand))) return rc;
    g.list = (GatherCand *)d->gat[1], g.list_cap = (uint32_t)pairs;
    IHIP_TRY(hipMemsetAsync(d->cursor, 0, sizeof(uint32_t), d->stream));
    IHIP_TRY(hipEventRecord(d->ev[2], d->stream));
    hipLaunchKernelGGL(k_index_gather_candidates, dim3(n), dim3(THREADS), 0, d->stream, a, g);
    IHIP_TRY(hipGetLastError());
    IHIP_TRY(hipEventRecord(d->ev[3], d->stream));
    IHIP_TRY(hipMemcpyAsync(d->back_h + d->chunk, d->cursor, sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
    IHIP_TRY(hipStreamSynchronize(d->stream));
    const uint32_t nc = d->back_h[d->chunk];
    if (nc > pairs) return api_fail(FH_ERR_STATE, "index gather: %u candidates from %llu pairs", nc, (unsigned long long)pairs);
    cands->resize(nc);
    if (nc) IHIP_TRY(hipMemcpy(cands->data(), d->gat[1], (size_t)nc * sizeof(GatherCand), hipMemcpyDeviceToHost));
    for (const GatherCand &c : *cands)
        if (c.q < q0 || c.q >= q1 || c.r >= d->nr || c.common == 0 || c.common > q.offsets[c.q + 1] - q.offsets[c.q] || c.common > d->rlen_h[c.r])
            return api_fail(FH_ERR_STATE, "index gather: candidate (%u, %u) with %u common hashes", c.q, c.r, c.common);
    std::sort(cands->begin(), cands->end(), [](const GatherCand &x, const GatherCand &y) { return x.q < y.q || (x.q == y.q && x.r < y.r); });
    // each query's range, (r, common) per candidate, the records the chunk can give at most -- a round removes at least one
    // hash --, the longest query that has candidates
    std::vector<uint32_t> off((size_t)n + 1, 0);
    std::vector<uint32_t> rc2((size_t)nc * 2);
    for (uint32_t i = 0; i < nc; ++i) {
        const GatherCand &c = (*cands)[i];
        if (i && (*cands)[i - 1].q == c.q && (*cands)[i - 1].r == c.r)
            return api_fail(FH_ERR_STATE, "index gather: candidate (%u, %u) twice", c.q, c.r);
        rc2[2 * (size_t)i] = c.r, rc2[2 * (size_t)i + 1] = c.common;
        ++off[c.q - q0 + 1];
    }
    uint64_t n_rec = 0, longest = 1;
    for (uint32_t b = 0; b < n; ++b) {
        const uint64_t len = q.offsets[q0 + b + 1] - q.offsets[q0 + b];
        n_rec += std::min<uint64_t>(max_rounds ? std::min<uint64_t>(max_rounds, off[b + 1]) : off[b + 1], len);
        if (off[b + 1]) longest = std::max(longest, len);
        off[b + 1] += off[b];
    }
    if (longest > GATHER_MAX_QUERY) return api_fail(FH_ERR_STATE, "index gather: a query of %llu hashes", (unsigned long long)longest);
    if (int rc = grow(&d->gat[2], &d->gat_cap[2], (size_t)nc * 2 * sizeof(uint32_t))) return rc;
    if (int rc = grow(&d->gat[4], &d->gat_cap[4], n_rec * sizeof(GatherRecord))) return rc;
    if (nc) IHIP_TRY(hipMemcpyAsync(d->gat[2], rc2.data(), (size_t)nc * 2 * sizeof(uint32_t), hipMemcpyHostToDevice, d->stream));
    IHIP_TRY(hipMemcpyAsync(d->gat[3], off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, d->stream));
    IHIP_TRY(hipMemsetAsync(d->gwords, 0, 2 * sizeof(uint32_t), d->stream));
    g.cand = (const uint2 *)d->gat[2], g.cand_off = (const uint32_t *)d->gat[3];
    g.rec = (GatherRecord *)d->gat[4], g.rec_cap = (uint32_t)n_rec;
    g.mask_words = (uint32_t)((longest + 31) / 32);

    // 3. the rounds, and the tail that leaves the counters zero
    IHIP_TRY(hipEventRecord(d->ev[4], d->stream));
    hipLaunchKernelGGL(k_index_gather_rounds, dim3(n), dim3(ROUND_THREADS), (size_t)g.mask_words * sizeof(uint32_t), d->stream, a, g);
    IHIP_TRY(hipGetLastError());
    IHIP_TRY(hipEventRecord(d->ev[5], d->stream));
    IHIP_TRY(hipMemcpyAsync(d->gwords_h, d->gwords, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
    IHIP_TRY(hipStreamSynchronize(d->stream)); // (rc2 and off are this frame's)
    d->dirty = false;
    *launches += 3;
    for (int e = 0; e < 6; e += 2) {
        float ms = 0.f;
        IHIP_TRY(hipEventElapsedTime(&ms, d->ev[e], d->ev[e + 1]));
        *kernel_ms += ms;
    }
    const uint32_t rows = d->gwords_h[0], err = d->gwords_h[1];
    if (err)
        return api_fail(FH_ERR_STATE, "index gather: the rounds kernel's counters do not match its mask (error word %u: %s)", err,
                        err & GERR_UNDERFLOW ? "a counter decremented at 0" : err & GERR_CLEARED ? "a round cleared another number of bits than its count"
                        : err & GERR_WINNER ? "a winner's counter is not 0 after its round" : "a query longer than the mask");
    if (rows > n_rec) return api_fail(FH_ERR_STATE, "index gather: %u records where at most %llu can be", rows, (unsigned long long)n_rec);
    recs->resize(rows);
    if (rows) IHIP_TRY(hipMemcpy(recs->data(), d->gat[4], (size_t)rows * sizeof(GatherRecord), hipMemcpyDeviceToHost));
    return FH_OK;
}

int index_gather_chunk(IndexDevice *d, const DistSide &queries, const uint32_t *counts, uint32_t q0, uint32_t q1, uint32_t min_overlap,
                       uint32_t max_rounds, std::vector<GatherCand> *cands, std::vector<GatherRecord> *recs, uint64_t *touched,
                       double *kernel_ms, uint64_t *launches) {
    if (!counts || q1 <= q0 || q1 > queries.n || q1 - q0 > d->chunk)
        return api_fail(FH_ERR_INVALID, "index_gather_chunk: queries %u..%u of %u, %u per launch", q0, q1, queries.n, d->chunk);
    if (d->dirty) return api_fail(FH_ERR_STATE, "index gather: an earlier call on this index failed between its kernels; build the index again");
    return gather_chunk(d, queries, counts, q0, q1, min_overlap, max_rounds, cands, recs, touched, kernel_ms, launches);
}

// ---- finch_index_compare_counts ----------------------------------------------------------------------------------------

int index_attach_counts(IndexDevice *d, const uint32_t *counts, uint64_t n, uint64_t *device_bytes) {
    if (!d || !counts || n != d->n_post)
        return api_fail(FH_ERR_INVALID, "index_attach_counts: %llu counts for %u postings", (unsigned long long)n, d ? d->n_post : 0);
    IHIP_TRY(hipSetDevice(d->device));
    const size_t bytes = (size_t)d->n_post * sizeof(uint32_t);
    if (!d->rcnt) IHIP_TRY(api_dev_malloc((void **)&d->rcnt, bytes));
    IHIP_TRY(hipMemcpy(d->rcnt, counts, bytes, hipMemcpyHostToDevice));
    *device_bytes = bytes;
    return FH_OK;
}

void index_drop_counts(IndexDevice *d) {
    if (!d || !d->rcnt) return;
    if (hipSetDevice(d->device) == hipSuccess && d->stream) (void)hipStreamSynchronize(d->stream);
    (void)hipFree(d->rcnt);
    d->rcnt = nullptr;
    (void)hipGetLastError();
}

// finch_index_compare_counts' chunk: the count as above, the selection that also stores the zeros back, the moment walk.
static int compare_counts_chunk(IndexDevice *d, const DistSide &q, const uint32_t *counts, uint32_t q0, uint32_t q1, uint32_t min_common,
                                std::vector<MomentsRecord> *recs, uint64_t *touched, double *kernel_ms, uint64_t *launches) {
    const uint32_t n = q1 - q0;
    recs->clear();
    IHIP_TRY(hipSetDevice(d->device));
    IndexArgs a;
    if (int rc = chunk_args(d, &q, q0, q1, &a)) return rc;
    const uint64_t nh = q.offsets[q1] - a.qbase;
    if (int rc = grow(&d->cmp[0], &d->cmp_cap[0], nh * sizeof(uint32_t))) return rc;
    if (nh) IHIP_TRY(hipMemcpy(d->cmp[0], counts + a.qbase, nh * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (!d->cwords) {
        IHIP_TRY(api_dev_malloc((void **)&d->cwords, 3 * sizeof(uint32_t)));
        IHIP_TRY(api_host_malloc((void **)&d->cwords_h, 3 * sizeof(uint32_t)));
    }

    // 1. the count; the touched lists' lengths cross, so that the pass list can be sized to what may pass
    d->dirty = true; // until the selection has stored the zeros back
    IHIP_TRY(hipEventRecord(d->ev[0], d->stream));
    hipLaunchKernelGGL(k_index_count, dim3(n), dim3(THREADS), 0, d->stream, a);
    IHIP_TRY(hipGetLastError());
    IHIP_TRY(hipEventRecord(d->ev[1], d->stream));
    IHIP_TRY(hipMemcpyAsync(d->back_h, d->tcount, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
    IHIP_TRY(hipStreamSynchronize(d->stream));
    uint64_t pairs = 0;
    for (uint32_t i = 0; i < n; ++i) pairs += d->back_h[i];
    float ms = 0.f;
    IHIP_TRY(hipEventElapsedTime(&ms, d->ev[0], d->ev[1]));
    *kernel_ms += ms;
    *touched += pairs;
    *launches += 1;
    if (pairs == 0) { // (nothing was counted: nothing to store back)
        d->dirty = false;
        return FH_OK;
    }

    // 2. the selection: c, and 0 back; the cursor crosses (pairs <= chunk x nr <= 2^31: index_open)
    if (int rc = grow(&d->cmp[1], &d->cmp_cap[1], pairs * sizeof(IndexPass))) return rc;
    IHIP_TRY(hipMemsetAsync(d->cursor, 0, sizeof(uint32_t), d->stream));
    IHIP_TRY(hipEventRecord(d->ev[2], d->stream));
    hipLaunchKernelGGL(k_index_moments_select, dim3(n), dim3(THREADS), 0, d->stream, a, min_common, (IndexPass *)d->cmp[1], (uint32_t)pairs,
                       d->cursor);
    IHIP_TRY(hipGetLastError());
    IHIP_TRY(hipEventRecord(d->ev[3], d->stream));
    IHIP_TRY(hipMemcpyAsync(d->back_h + d->chunk, d->cursor, sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
    IHIP_TRY(hipStreamSynchronize(d->stream));
    d->dirty = false; // the counters are clean, whatever the walk does
    IHIP_TRY(hipEventElapsedTime(&ms, d->ev[2], d->ev[3]));
    *kernel_ms += ms;
    *launches += 1;
    const uint32_t np = d->back_h[d->chunk];
    if (np > pairs) return api_fail(FH_ERR_STATE, "index compare_counts: %u pairs pass of %llu", np, (unsigned long long)pairs);
    if (np == 0) return FH_OK;

    // 3. the moment walk, one wave per passing pair; the records at their pairs' places in the pass list
    if (int rc = grow(&d->cmp[2], &d->cmp_cap[2], (size_t)np * sizeof(MomentsRecord))) return rc;
    IHIP_TRY(hipMemsetAsync(d->cwords, 0, 3 * sizeof(uint32_t), d->stream));
    IndexMomentsArgs m;
    m.qh = a.qh, m.qoff = a.qoff, m.qc = (const uint32_t *)d->cmp[0], m.qbase = a.qbase, m.q0 = q0, m.nq = n;
    m.rh = a.rh, m.roff = a.roff, m.rc = d->rcnt, m.nr = d->nr;
    m.pass = (const IndexPass *)d->cmp[1], m.n_pass = np, m.rec = (MomentsRecord *)d->cmp[2], m.err = d->cwords;
    IHIP_TRY(hipEventRecord(d->ev[4], d->stream));
    if (int rc = index_moments_launch(m, d->stream)) return rc;
    IHIP_TRY(hipEventRecord(d->ev[5], d->stream));
    IHIP_TRY(hipMemcpyAsync(d->cwords_h, d->cwords, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
    IHIP_TRY(hipStreamSynchronize(d->stream));
    IHIP_TRY(hipEventElapsedTime(&ms, d->ev[4], d->ev[5]));
    *kernel_ms += ms;
    *launches += 1;
    if (d->cwords_h[0])
        return api_fail(FH_ERR_STATE, "index compare_counts: index counters and walk disagree for pair (%u, %u)", d->cwords_h[1], d->cwords_h[2]);
    recs->resize(np);
    IHIP_TRY(hipMemcpy(recs->data(), d->cmp[2], (size_t)np * sizeof(MomentsRecord), hipMemcpyDeviceToHost));
    return FH_OK;
}

int index_compare_counts_chunk(IndexDevice *d, const DistSide &queries, const uint32_t *counts, uint32_t q0, uint32_t q1, uint32_t min_common,
                               std::vector<MomentsRecord> *recs, uint64_t *touched, double *kernel_ms, uint64_t *launches) {
    if (!counts || !min_common || q1 <= q0 || q1 > queries.n || q1 - q0 > d->chunk)
        return api_fail(FH_ERR_INVALID, "index_compare_counts_chunk: queries %u..%u of %u, %u per launch, min_common %u", q0, q1, queries.n,
                        d->chunk, min_common);
    if (!d->rcnt) return api_fail(FH_ERR_STATE, "index compare_counts: no counts are attached to the index (finch_index_attach_counts)");
    if (d->dirty) return api_fail(FH_ERR_STATE, "index compare_counts: an earlier call on this index failed between its kernels; build the index again");
    return compare_counts_chunk(d, queries, counts, q0, q1, min_common, recs, touched, kernel_ms, launches);
}

// ---- finch_index_add / finch_index_keep ---------------------------------------------------------------

// what open_into counts for a library of these sizes
static uint64_t kept_bytes(uint32_t nr, uint64_t P, uint32_t chunk) {
    auto up = [](uint64_t b) { return std::max<uint64_t>(b, 8); };
    return up(P * 8) + up(((uint64_t)nr + 1) * 8) + 3 * up((uint64_t)nr * 8) + 2 * up((uint64_t)nr * 4) + P * 12 +
           2 * (uint64_t)chunk * nr * sizeof(uint32_t) + ((uint64_t)chunk + 1) * sizeof(uint32_t);
}

// the stage's per-launch state as open_into makes it: the counters zeroed (on the stream)
static int stage_state(IndexDevice *d, IndexStage *s) {
    const size_t dense = (size_t)s->chunk * s->nr * sizeof(uint32_t);
    IHIP_TRY(api_dev_malloc((void **)&s->cnt, dense));
    IHIP_TRY(api_dev_malloc((void **)&s->touched, dense));
    IHIP_TRY(api_dev_malloc((void **)&s->tcount, s->chunk * sizeof(uint32_t)));
    IHIP_TRY(api_host_malloc((void **)&s->back_h, ((size_t)s->chunk + 1) * sizeof(uint32_t)));
    IHIP_TRY(hipMemsetAsync(s->cnt, 0, dense, d->stream));
    return FH_OK;
}

// a stage array: the first n_old elements from the device's `old` (on the stream), then n_more from the host's `more`
static int extend(IndexDevice *d, void **dst, const void *old, size_t n_old, const void *more, size_t n_more, size_t elem) {
    IHIP_TRY(api_dev_malloc(dst, std::max<size_t>((n_old + n_more) * elem, 8)));
    if (n_old) IHIP_TRY(hipMemcpyAsync(*dst, old, n_old * elem, hipMemcpyDeviceToDevice, d->stream));
    if (n_more) IHIP_TRY(hipMemcpy((char *)*dst + n_old * elem, more, n_more * elem, hipMemcpyHostToDevice));
    return FH_OK;
}

struct UpdateScratch {
    void *p[5] = {};
    ~UpdateScratch() {
        for (void *q : p)
            if (q) (void)hipFree(q);
    }
};

static uint32_t update_grid(uint32_t n_tiles) { return std::max(1u, std::min(n_tiles, 1u << 19)); }

static int add_into(IndexDevice *d, const DistSide &m, const uint32_t *counts, uint32_t tile, double *kernel_ms) {
    IndexStage *s = &d->next;
    const uint32_t nm = m.n;
    const uint64_t Pm = m.offsets[nm];
    std::vector<uint64_t> rlast(nm), roff((size_t)s->nr + 1, 0);
    std::vector<uint32_t> rlen(nm);
    s->rlen_h = d->rlen_h;
    for (uint32_t t = 0; t < nm; ++t) {
        rlen[t] = (uint32_t)(m.offsets[t + 1] - m.offsets[t]);
        rlast[t] = rlen[t] ? m.hashes[m.offsets[t + 1] - 1] : 0;
        s->rlen_h.push_back(rlen[t]);
    }
    for (uint32_t r = 0; r < s->nr; ++r) roff[r + 1] = roff[r] + s->rlen_h[r];
    if (roff[d->nr] != d->n_post || roff[s->nr] != s->n_post)
        return api_fail(FH_ERR_STATE, "index add: the lengths the index keeps sum to %llu, it holds %u postings", (unsigned long long)roff[d->nr], d->n_post);

    // the CSR and the per-reference arrays: what is there device to device, what is new from the host
    if (int rc = extend(d, &s->lib[0], d->lib[0], d->n_post, m.hashes, Pm, sizeof(uint64_t))) return rc;
    if (int rc = extend(d, &s->lib[1], nullptr, 0, roff.data(), roff.size(), sizeof(uint64_t))) return rc;
    if (int rc = extend(d, &s->lib[2], d->lib[2], d->nr, rlast.data(), nm, sizeof(uint64_t))) return rc;
    if (int rc = extend(d, &s->lib[3], d->lib[3], d->nr, m.max_hash, nm, sizeof(uint64_t))) return rc;
    if (int rc = extend(d, &s->lib[4], d->lib[4], d->nr, rlen.data(), nm, sizeof(uint32_t))) return rc;
    if (int rc = extend(d, &s->lib[5], d->lib[5], d->nr, m.flags, nm, sizeof(uint32_t))) return rc;
    if (int rc = extend(d, &s->lib[6], d->lib[6], d->nr, m.scale, nm, sizeof(double))) return rc;
    if (d->rcnt)
        if (int rc = extend(d, (void **)&s->rcnt, d->rcnt, d->n_post, counts, Pm, sizeof(uint32_t))) return rc;
    IHIP_TRY(api_dev_malloc(&s->lib[7], (size_t)s->n_post * sizeof(uint64_t)));
    IHIP_TRY(api_dev_malloc(&s->lib[8], (size_t)s->n_post * sizeof(uint32_t)));

    // the added postings in reference order, sorted by hash -- stable: a hash's new references ascend --, then merged in
    UpdateScratch x; // keys, vals, their sort scratch, the sort's histogram space
    size_t tmp_bytes = 0;
    if (Pm) {
        IHIP_TRY(big_sort_tmp_bytes((uint32_t)Pm, &tmp_bytes));
        IHIP_TRY(api_dev_malloc(&x.p[0], Pm * sizeof(uint64_t)));
        IHIP_TRY(api_dev_malloc(&x.p[1], Pm * sizeof(uint32_t)));
        IHIP_TRY(api_dev_malloc(&x.p[2], Pm * sizeof(uint64_t)));
        IHIP_TRY(api_dev_malloc(&x.p[3], Pm * sizeof(uint32_t)));
        IHIP_TRY(api_dev_malloc(&x.p[4], std::max<size_t>(tmp_bytes, 8)));
    }
    IHIP_TRY(hipEventRecord(d->ev[0], d->stream));
    if (Pm) {
        hipLaunchKernelGGL(k_index_postings, dim3(std::min(nm, 4096u)), dim3(THREADS), 0, d->stream, (const uint64_t *)s->lib[0],
                           (const uint64_t *)s->lib[1], d->nr, s->nr, (uint64_t *)x.p[0], (uint32_t *)x.p[1]);
        IHIP_TRY(hipGetLastError());
        IHIP_TRY(big_sort_pairs(x.p[4], tmp_bytes, (uint64_t *)x.p[0], (uint64_t *)x.p[2], (uint32_t *)x.p[1], (uint32_t *)x.p[3], (uint32_t)Pm,
                                d->stream));
    }
    const uint32_t n_tiles = (uint32_t)(((uint64_t)s->n_post + tile - 1) / tile);
    hipLaunchKernelGGL(k_index_merge, dim3(update_grid(n_tiles)), dim3(THREADS), 0, d->stream, (const uint64_t *)d->lib[7],
                       (const uint32_t *)d->lib[8], d->n_post, (const uint64_t *)x.p[0], (const uint32_t *)x.p[1], (uint32_t)Pm, (uint64_t *)s->lib[7],
                       (uint32_t *)s->lib[8], tile, n_tiles);
    IHIP_TRY(hipGetLastError());
    IHIP_TRY(hipEventRecord(d->ev[1], d->stream));
    if (int rc = stage_state(d, s)) return rc;
    IHIP_TRY(hipStreamSynchronize(d->stream)); // (the scratch and this frame's vectors are free to go)
    float ms = 0.f;
    IHIP_TRY(hipEventElapsedTime(&ms, d->ev[0], d->ev[1]));
    *kernel_ms += ms;
    return FH_OK;
}

static int keep_into(IndexDevice *d, const uint32_t *keep, uint32_t n_keep, uint32_t tile, double *kernel_ms) {
    IndexStage *s = &d->next;
    std::vector<uint32_t> map(d->nr, NONE_REF);
    std::vector<uint64_t> noff((size_t)n_keep + 1, 0);
    s->rlen_h.resize(n_keep);
    for (uint32_t t = 0; t < n_keep; ++t) {
        map[keep[t]] = t;
        s->rlen_h[t] = d->rlen_h[keep[t]];
        noff[t + 1] = noff[t] + s->rlen_h[t];
    }
    if (noff[n_keep] != s->n_post)
        return api_fail(FH_ERR_STATE, "index keep: the survivors' lengths sum to %llu, not %u", (unsigned long long)noff[n_keep], s->n_post);

    const size_t P = s->n_post;
    IHIP_TRY(api_dev_malloc(&s->lib[0], P * sizeof(uint64_t)));
    if (int rc = extend(d, &s->lib[1], nullptr, 0, noff.data(), noff.size(), sizeof(uint64_t))) return rc;
    IHIP_TRY(api_dev_malloc(&s->lib[2], (size_t)n_keep * sizeof(uint64_t)));
    IHIP_TRY(api_dev_malloc(&s->lib[3], (size_t)n_keep * sizeof(uint64_t)));
    IHIP_TRY(api_dev_malloc(&s->lib[4], (size_t)n_keep * sizeof(uint32_t)));
    IHIP_TRY(api_dev_malloc(&s->lib[5], (size_t)n_keep * sizeof(uint32_t)));
    IHIP_TRY(api_dev_malloc(&s->lib[6], (size_t)n_keep * sizeof(double)));
    IHIP_TRY(api_dev_malloc(&s->lib[7], P * sizeof(uint64_t)));
    IHIP_TRY(api_dev_malloc(&s->lib[8], P * sizeof(uint32_t)));
    if (d->rcnt) IHIP_TRY(api_dev_malloc((void **)&s->rcnt, P * sizeof(uint32_t)));

    const uint32_t n_tiles = (uint32_t)(((uint64_t)d->n_post + tile - 1) / tile);
    UpdateScratch x; // map, the survivors, the tiles' counts and after them their sum
    if (int rc = extend(d, &x.p[0], nullptr, 0, map.data(), map.size(), sizeof(uint32_t))) return rc;
    if (int rc = extend(d, &x.p[1], nullptr, 0, keep, n_keep, sizeof(uint32_t))) return rc;
    IHIP_TRY(api_dev_malloc(&x.p[2], ((size_t)n_tiles + 1) * sizeof(uint32_t)));
    uint32_t *count = (uint32_t *)x.p[2];
    const uint64_t *keys = (const uint64_t *)d->lib[7];
    const uint32_t *vals = (const uint32_t *)d->lib[8], *map_d = (const uint32_t *)x.p[0];

    IHIP_TRY(hipEventRecord(d->ev[0], d->stream));
    hipLaunchKernelGGL(k_index_compact<false>, dim3(update_grid(n_tiles)), dim3(THREADS), 0, d->stream, keys, vals, d->n_post, map_d, d->nr, tile,
                       n_tiles, count, (uint64_t *)nullptr, (uint32_t *)nullptr, 0u);
    IHIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_index_tile_scan, dim3(1), dim3(1024), 0, d->stream, count, n_tiles, count + n_tiles);
    IHIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_index_compact<true>, dim3(update_grid(n_tiles)), dim3(THREADS), 0, d->stream, keys, vals, d->n_post, map_d, d->nr, tile,
                       n_tiles, count, (uint64_t *)s->lib[7], (uint32_t *)s->lib[8], s->n_post);
    IHIP_TRY(hipGetLastError());
    KeepRefsArgs k;
    k.rh = (const uint64_t *)d->lib[0], k.roff = (const uint64_t *)d->lib[1], k.rlast = (const uint64_t *)d->lib[2];
    k.rmax = (const uint64_t *)d->lib[3], k.rlen = (const uint32_t *)d->lib[4], k.rflag = (const uint32_t *)d->lib[5], k.rcnt = d->rcnt;
    k.rscale = (const double *)d->lib[6], k.nr = d->nr;
    k.keep = (const uint32_t *)x.p[1], k.n_keep = n_keep, k.noff = (const uint64_t *)s->lib[1];
    k.nh = (uint64_t *)s->lib[0], k.nlast = (uint64_t *)s->lib[2], k.nmax = (uint64_t *)s->lib[3];
    k.nlen = (uint32_t *)s->lib[4], k.nflag = (uint32_t *)s->lib[5], k.ncnt = s->rcnt, k.nscale = (double *)s->lib[6];
    hipLaunchKernelGGL(k_index_keep_refs, dim3(std::min(n_keep, 4096u)), dim3(THREADS), 0, d->stream, k);
    IHIP_TRY(hipGetLastError());
    IHIP_TRY(hipEventRecord(d->ev[1], d->stream));
    if (int rc = stage_state(d, s)) return rc;
    IHIP_TRY(hipStreamSynchronize(d->stream)); // (the scratch and this frame's vectors are free to go)
    uint32_t total = 0;
    IHIP_TRY(hipMemcpy(&total, count + n_tiles, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (total != s->n_post) return api_fail(FH_ERR_STATE, "index keep: %u postings survive where the lengths say %u", total, s->n_post);
    float ms = 0.f;
    IHIP_TRY(hipEventElapsedTime(&ms, d->ev[0], d->ev[1]));
    *kernel_ms += ms;
    return FH_OK;
}

// what both updates check and set before they build: the stage is empty and knows the sizes it is built for
static int stage_begin(IndexDevice *d, const char *what, uint64_t nr, uint64_t P, uint32_t chunk_queries, uint32_t tile) {
    if (!d || nr == 0 || nr > UINT32_MAX || P == 0 || P > INDEX_MAX_POSTINGS || chunk_queries == 0 || (uint64_t)chunk_queries * nr > (1ull << 31) ||
        tile == 0 || tile > UPDATE_MAX_TILE)
        return api_fail(FH_ERR_INVALID, "%s: %llu references, %llu postings, %u queries per launch, tiles of %u", what, (unsigned long long)nr,
                        (unsigned long long)P, chunk_queries, tile);
    IHIP_TRY(hipSetDevice(d->device));
    IHIP_TRY(hipStreamSynchronize(d->stream));
    stage_drop(&d->next);
    d->next.nr = (uint32_t)nr, d->next.n_post = (uint32_t)P, d->next.chunk = chunk_queries;
    return FH_OK;
}

int index_add(IndexDevice *d, const DistSide &more, const uint32_t *counts, uint32_t chunk_queries, uint32_t tile, double *kernel_ms) {
    // (sketches without a hash bring no counts: an empty array may well be a null pointer)
    if (d && d->rcnt && !counts && more.offsets[more.n] != 0)
        return api_fail(FH_ERR_INVALID, "index_add: counts are attached to the index and none come with the sketches");
    if (int rc = stage_begin(d, "index_add", (uint64_t)(d ? d->nr : 0) + more.n, (uint64_t)(d ? d->n_post : 0) + more.offsets[more.n], chunk_queries, tile))
        return rc;
    if (int rc = add_into(d, more, counts, tile, kernel_ms)) {
        index_discard(d);
        return rc;
    }
    d->next.ready = true;
    return FH_OK;
}

int index_keep(IndexDevice *d, const uint32_t *keep, uint32_t n_keep, uint32_t chunk_queries, uint32_t tile, double *kernel_ms) {
    uint64_t P = 0;
    for (uint32_t t = 0; d && keep && t < n_keep; ++t) {
        if (keep[t] >= d->nr || (t && keep[t] <= keep[t - 1])) return api_fail(FH_ERR_INVALID, "index_keep: keep[%u] = %u", t, keep[t]);
        P += d->rlen_h[keep[t]];
    }
    if (!keep) return api_fail(FH_ERR_INVALID, "index_keep: null argument");
    if (int rc = stage_begin(d, "index_keep", n_keep, P, chunk_queries, tile)) return rc;
    if (int rc = keep_into(d, keep, n_keep, tile, kernel_ms)) {
        index_discard(d);
        return rc;
    }
    d->next.ready = true;
    return FH_OK;
}

void index_discard(IndexDevice *d) {
    if (!d) return;
    if (hipSetDevice(d->device) == hipSuccess && d->stream) (void)hipStreamSynchronize(d->stream); // nothing in flight reads the stage
    stage_drop(&d->next);
    (void)hipGetLastError();
}

uint64_t index_commit(IndexDevice *d) {
    IndexStage &s = d->next;
    if (s.ready) {
        (void)hipSetDevice(d->device);
        (void)hipStreamSynchronize(d->stream);
        for (void *p : d->lib) (void)hipFree(p);
        for (uint32_t *p : {d->rcnt, d->cnt, d->touched, d->tcount, d->sel})
            if (p) (void)hipFree(p);
        (void)hipHostFree(d->back_h);
        // what a chunk allocates by the old `chunk`: its first use allocates it again
        for (void *&p : d->qry) {
            if (p) (void)hipFree(p);
            p = nullptr;
        }
        if (d->jmin) (void)hipFree(d->jmin);
        d->qry_hashes = 0, d->jmin = nullptr, d->sel = nullptr, d->sel_cap = 0;
        for (int i = 0; i < 9; ++i) d->lib[i] = s.lib[i], s.lib[i] = nullptr;
        d->rcnt = s.rcnt, d->cnt = s.cnt, d->touched = s.touched, d->tcount = s.tcount, d->back_h = s.back_h;
        s.rcnt = s.cnt = s.touched = s.tcount = s.back_h = nullptr;
        d->nr = s.nr, d->n_post = s.n_post, d->chunk = s.chunk;
        d->rlen_h.swap(s.rlen_h);
        d->dirty = false; // the counters are new, and zero
        s = IndexStage();
        (void)hipGetLastError();
    }
    return kept_bytes(d->nr, d->n_post, d->chunk);
}

} // namespace fh
