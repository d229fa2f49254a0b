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
// The order in which atomics land decides only where an entry sits in a list; the host sorts.
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
__global__ void __launch_bounds__(THREADS) k_index_postings(const uint64_t *rh, const uint64_t *roff, uint32_t nr, uint64_t *keys, uint32_t *vals) {
    for (uint32_t r = blockIdx.x; r < nr; r += gridDim.x) {
        const uint64_t r0 = roff[r], r1 = roff[r + 1];
        for (uint64_t t = r0 + threadIdx.x; t < r1; t += THREADS) {
            keys[t] = rh[t];
            vals[t] = r;
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

} // namespace

namespace fh {

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
    hipEvent_t ev[4] = {};
    bool dirty = false;           // a launch failed between the count and the finish: the counters are not known to be zero
};

void index_close(IndexDevice *d) {
    if (!d) return;
    if (hipSetDevice(d->device) == hipSuccess) {
        if (d->stream) (void)hipStreamSynchronize(d->stream);
        for (void *p : d->lib)
            if (p) (void)hipFree(p);
        for (void *p : d->qry)
            if (p) (void)hipFree(p);
        for (uint32_t *p : {d->cnt, d->touched, d->tcount, d->cursor, d->sel})
            if (p) (void)hipFree(p);
        if (d->jmin) (void)hipFree(d->jmin);
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
                       (const uint64_t *)d->lib[1], d->nr, (uint64_t *)d->lib[7], (uint32_t *)d->lib[8]);
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

// one chunk of either route.  q = nullptr: the queries are the library's own sketches q0 .. q1 (pairwise), read where the index
// keeps them.  jmin = nullptr: the search's finish with min_containment; else finch_index_dist's with the chunk's bounds.
static int run_chunk(IndexDevice *d, const DistSide *q, uint32_t q0, uint32_t q1, double min_containment, const double *jmin, bool old_mode,
                     std::vector<uint32_t> *entries, uint64_t *touched, double *kernel_ms) {
    const uint32_t n = q1 - q0;
    IHIP_TRY(hipSetDevice(d->device));
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
    if (jmin) {
        if (!d->jmin) IHIP_TRY(api_dev_malloc((void **)&d->jmin, (size_t)d->chunk * sizeof(double)));
        IHIP_TRY(hipMemcpy(d->jmin, jmin, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
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
    a.min_c = min_containment;
    a.sel = d->sel, a.cursor = d->cursor, a.sel_cap = 0;

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
    if (jmin) hipLaunchKernelGGL(k_index_dist_finish, dim3(n), dim3(THREADS), 0, d->stream, a, (const double *)d->jmin, old_mode ? 1u : 0u);
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
    return run_chunk(d, &queries, q0, q1, min_containment, nullptr, false, entries, touched, kernel_ms);
}

int index_dist_chunk(IndexDevice *d, const DistSide *queries, uint32_t q0, uint32_t q1, bool old_mode, const double *jmin,
                     std::vector<uint32_t> *entries, uint64_t *touched, double *kernel_ms) {
    if (!jmin || q1 <= q0 || q1 > (queries ? queries->n : d->nr) || q1 - q0 > d->chunk)
        return api_fail(FH_ERR_INVALID, "index_dist_chunk: queries %u..%u of %u, %u per launch", q0, q1, queries ? queries->n : d->nr, d->chunk);
    if (d->dirty) return api_fail(FH_ERR_STATE, "index dist: an earlier call on this index failed between its two kernels; build the index again");
    return run_chunk(d, queries, q0, q1, 0., jmin, old_mode, entries, touched, kernel_ms);
}

} // namespace fh
