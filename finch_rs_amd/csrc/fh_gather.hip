// fh_gather.hip -- finch_gather (include/finch_host.h): the greedy decomposition of each query sketch over a
// library, hand-written for gfx950.  Round t takes the reference that shares the most hashes with what is left of the query
// (ties: the lowest index), writes a record and removes that reference's hashes from the query.  Plain set semantics over the
// hashes as stored: this is deliberately NOT raw_distance's walk (no max_hash cut, no early stop).
//
//   counting    the query-major instantiation of the distance kernel (fh_dist.hip, §3.7 / §3.10) leaves c = |Q n R| of every
//               pair of a reference chunk in device memory;
//   candidates  k_gather_candidates appends (q, r, common) for common >= min_overlap to the chunk's list, a wave taking its places
//               with one atomic add; the host copies the cursor, then that many entries, sorts each query's by reference and
//               makes the exclusive scan of their `common`: each candidate's segment of the position array, exact;
//   positions   k_gather_positions, one wave per candidate: the query's hashes come through LDS a slice at a time, the reference's
//               hashes are looked up 64 per step (§3.7's branchless search), and the indices of the query hashes that match go
//               to the candidate's segment at the wave's own running cursor (ballot + prefix popcount; no atomics).  Slices,
//               steps and lanes ascend, so a segment ascends.  A cursor that does not end at `common` sets the error word;
//   rounds      k_gather_rounds, one workgroup of 1024 per query, the whole loop inside: the remaining set is a bitmask over
//               query positions in LDS; per round every wave recounts its candidates against the mask (c_j(t) never grows, so a
//               candidate whose last count cannot beat the wave's best so far, or is below min_overlap, is not recounted), a
//               workgroup arg-max on (count descending, reference ascending) picks the winner, whose bits are cleared with LDS
//               atomic ANDs while the query's counts of them are summed, and one thread appends the 48-byte record.
//
// Barriers in k_gather_rounds: every branch that holds a barrier is taken on a value all 1024 threads read from the same LDS
// word (s_word), the rule fh_batch_large.hip states at its top.  Results are written with plain vector stores.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../../include/finch_hip.h"
#include "fh_dist.h"
#include "fh_internal.h"

using namespace fh;

namespace {

#define GHIP_TRY(expr)                                                                                      \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess) return api_fail(FH_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

constexpr uint32_t CAND_THREADS = 256;
constexpr uint32_t ROUND_THREADS = 1024, ROUND_WAVES = ROUND_THREADS / 64;
constexpr uint32_t NONE = 0xffffffffu;
constexpr uint32_t ERR_POSITIONS = 1, ERR_ROUNDS = 2; // bits of the error word

// a candidate on the device: `live` is its count against the remaining set as of the last round that recounted it (an upper
// bound of the current one), `seg` where its `common` positions start in the chunk's position array
struct CandDev {
    uint32_t q, r, common, live;
    uint64_t seg;
};

// #{s[0..n) <= x} over ascending s; top = the largest power of two <= n (n >= 1).  The same steps in every lane, no branch; the
// index is clamped so that no read leaves s[0..n).  (fh_dist.hip's count_below<true>.)
__device__ inline uint32_t count_le(const uint64_t *s, uint32_t n, uint32_t top, uint64_t x) {
    uint32_t pos = 0;
    for (uint32_t step = top; step; step >>= 1) {
        const uint32_t p = pos + step;
        const uint64_t v = s[min(p, n) - 1];
        pos = (p <= n && v <= x) ? p : pos;
    }
    return pos;
}

__device__ inline uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ inline uint64_t wave_sum64(uint64_t v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ inline uint32_t lane_rank(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

struct CandArgs {
    const uint32_t *cnt; // the chunk's counts, query-major, 3 u32 per pair
    uint32_t n, r0;      // references of the chunk, the first one's index
    uint32_t min_overlap;
    uint32_t cap;        // entries the list holds: the chunk's pairs
    GatherCand *list;
    uint32_t *cursor;    // zero before the launch
};

// grid: x = query.  Every pair of the chunk with common >= min_overlap, appended to the chunk's list as k_search_all appends.
__global__ void __launch_bounds__(CAND_THREADS) k_gather_candidates(CandArgs a) {
    const uint32_t q = blockIdx.x;
    const uint32_t *cnt = a.cnt + (uint64_t)q * a.n * 3;
    for (uint32_t base = 0; base < a.n; base += CAND_THREADS) { // (whole waves go round: the ballot sees every lane)
        const uint32_t t = base + threadIdx.x;
        uint32_t c = 0;
        if (t < a.n) c = cnt[(uint64_t)t * 3];
        const bool pass = t < a.n && c >= a.min_overlap;
        const uint64_t mask = __ballot(pass);
        if (!mask) continue;
        const uint32_t rank = lane_rank(mask);
        uint32_t first = 0;
        if (pass && rank == 0) first = atomicAdd(a.cursor, (uint32_t)__popcll(mask));
        first = __shfl(first, __ffsll((unsigned long long)mask) - 1, 64);
        if (pass && first + rank < a.cap) {
            GatherCand e;
            e.q = q, e.r = a.r0 + t, e.common = c;
            a.list[first + rank] = e;
        }
    }
}

struct PosArgs {
    const uint64_t *qh, *qoff, *rh, *roff;
    const CandDev *cand;
    uint32_t *pos;
    uint32_t slice;
    uint32_t *err;
};

// grid: x = candidate, one wave each; dynamic LDS: a.slice u64
__global__ void __launch_bounds__(64) k_gather_positions(PosArgs a) {
    extern __shared__ uint64_t s_q[];
    const CandDev cd = a.cand[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    const uint64_t qa = a.qoff[cd.q], ra = a.roff[cd.r];
    const uint32_t nqh = (uint32_t)(a.qoff[cd.q + 1] - qa), nrh = (uint32_t)(a.roff[cd.r + 1] - ra);
    const uint64_t *Q = a.qh + qa, *R = a.rh + ra;
    uint32_t *seg = a.pos + cd.seg;
    uint32_t cursor = 0; // the same in every lane
    for (uint32_t s0 = 0; s0 < nqh; s0 += a.slice) {
        const uint32_t ns = min(a.slice, nqh - s0);
        const uint32_t top = 1u << (31 - __clz(ns));
        __syncthreads(); // the previous slice is no longer read
        for (uint32_t i = lane; i < ns; i += 64) s_q[i] = Q[s0 + i];
        __syncthreads();
        for (uint32_t base = 0; base < nrh; base += 64) { // (the whole wave goes round: the ballot sees every lane)
            const uint32_t t = base + lane;
            bool hit = false;
            uint32_t p = 0;
            if (t < nrh) {
                const uint64_t x = R[t];
                p = count_le(s_q, ns, top, x);
                hit = p && s_q[p ? p - 1 : 0] == x;
            }
            const uint64_t mask = __ballot(hit);
            const uint32_t at = cursor + lane_rank(mask);
            if (hit && at < cd.common) seg[at] = s0 + p - 1; // (never past the segment, whatever the counts said)
            cursor += (uint32_t)__popcll(mask);
        }
    }
    if (lane == 0 && cursor != cd.common) atomicOr(a.err, ERR_POSITIONS);
}

struct RoundArgs {
    const uint64_t *qoff, *roff;
    const uint32_t *qcnt;     // the queries' counts, parallel to their hashes
    CandDev *cand;            // the chunk's candidates, by (q, r)
    const uint64_t *cand_off; // query q0 + b's are cand[cand_off[b] .. cand_off[b + 1])
    const uint32_t *pos;
    uint32_t q0, min_overlap, max_rounds;
    GatherRecord *rec;
    uint32_t rec_cap;
    uint32_t *cursor; // zero before the launch
    uint32_t *err;
    uint32_t mask_words; // the launch's dynamic LDS, in u32
};

enum { W_BOUND = 0, W_WIN = 1, W_COUNT = 2, W_N = 3 };

// grid: x = query of the chunk; dynamic LDS: a.mask_words u32, one bit per hash of the longest of the chunk's queries that have
// candidates.  A query without candidates runs no round and touches no mask: it may be longer than the mask.
__global__ void __launch_bounds__(ROUND_THREADS) k_gather_rounds(RoundArgs a) {
    extern __shared__ uint32_t s_mask[];
    __shared__ uint32_t s_cnt[ROUND_WAVES], s_idx[ROUND_WAVES], s_clr[ROUND_WAVES];
    __shared__ uint64_t s_ab[ROUND_WAVES];
    __shared__ uint32_t s_word[W_N];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t q = a.q0 + blockIdx.x;
    const uint64_t qa = a.qoff[q];
    const uint32_t nqh = (uint32_t)(a.qoff[q + 1] - qa);
    const uint32_t *qcnt = a.qcnt + qa;
    const uint64_t c0 = a.cand_off[blockIdx.x];
    const uint32_t ncand = (uint32_t)(a.cand_off[blockIdx.x + 1] - c0);
    CandDev *const cand = a.cand + c0;
    if (ncand) // (no barrier inside; the host sized the mask for every query that gets here)
        for (uint32_t w = tid; w < min((nqh + 31) / 32, a.mask_words); w += ROUND_THREADS) s_mask[w] = w * 32 + 32 <= nqh ? ~0u : (1u << (nqh & 31)) - 1;
    if (tid == 0) // (nothing runs on positions the kernel before could not complete)
        s_word[W_BOUND] = (*a.err || (nqh + 31) / 32 > a.mask_words) ? 0 : a.max_rounds ? min(a.max_rounds, ncand) : ncand;
    __syncthreads();
    const uint32_t bound = s_word[W_BOUND];
    uint32_t remaining = nqh;
    for (uint32_t t = 0; t < bound; ++t) {
        // c_j(t) of this wave's candidates, in reference order: the first of the largest wins the wave
        uint32_t best_c = 0, best_i = NONE;
        for (uint32_t i = wave; i < ncand; i += ROUND_WAVES) {
            uint32_t live = 0;
            if (lane == 0) live = cand[i].live; // (the lane that wrote it)
            live = __shfl(live, 0, 64);
            if (live < a.min_overlap || live <= best_c) continue; // out for good / cannot beat an earlier one: counts never grow
            const uint32_t n = cand[i].common;
            const uint32_t *seg = a.pos + cand[i].seg;
            uint32_t c = 0;
            for (uint32_t k = lane; k < n; k += 64) {
                const uint32_t p = seg[k];
                if (p < nqh) c += (s_mask[p >> 5] >> (p & 31)) & 1;
            }
            c = wave_sum(c);
            if (lane == 0) cand[i].live = c;
            if (c >= a.min_overlap && c > best_c) best_c = c, best_i = i;
        }
        if (lane == 0) s_cnt[wave] = best_c, s_idx[wave] = best_i;
        __syncthreads();
        if (tid == 0) { // count descending, then candidate (= reference) ascending
            uint32_t wc = 0, wi = NONE;
            for (uint32_t w = 0; w < ROUND_WAVES; ++w) {
                const uint32_t c = s_cnt[w], i = s_idx[w];
                if (i != NONE && (wi == NONE || c > wc || (c == wc && i < wi))) wc = c, wi = i;
            }
            s_word[W_WIN] = wi; // NONE: no candidate reaches min_overlap
            s_word[W_COUNT] = wc;
        }
        __syncthreads();
        const uint32_t wi = s_word[W_WIN], wc = s_word[W_COUNT];
        if (wi == NONE) break; // the same LDS word in every thread
        // S_{t+1} = S_t \ H_w: the winner's set bits cleared, the query's counts of them summed
        const uint32_t n = cand[wi].common;
        const uint32_t *seg = a.pos + cand[wi].seg;
        uint64_t ab = 0;
        uint32_t clr = 0;
        for (uint32_t k = tid; k < n; k += ROUND_THREADS) {
            const uint32_t p = seg[k];
            if (p < nqh) {
                const uint32_t bit = 1u << (p & 31);
                if (atomicAnd(&s_mask[p >> 5], ~bit) & bit) ab += qcnt[p], ++clr;
            }
        }
        ab = wave_sum64(ab);
        clr = wave_sum(clr);
        if (lane == 0) s_ab[wave] = ab, s_clr[wave] = clr;
        __syncthreads();
        remaining -= wc;
        if (tid == 0) {
            uint64_t abund = 0;
            uint32_t cleared = 0;
            for (uint32_t w = 0; w < ROUND_WAVES; ++w) abund += s_ab[w], cleared += s_clr[w];
            if (cleared != wc) atomicOr(a.err, ERR_ROUNDS);
            const uint32_t r = cand[wi].r;
            GatherRecord rec;
            rec.q = q, rec.r = r, rec.round = t, rec.overlap = wc, rec.common = n;
            rec.ref_len = (uint32_t)(a.roff[r + 1] - a.roff[r]);
            rec.query_len = nqh, rec.remaining = remaining, rec.abund = abund, rec.cand = wi, rec.pad = 0;
            const uint32_t at = atomicAdd(a.cursor, 1u);
            if (at < a.rec_cap) a.rec[at] = rec;
        }
    }
}

} // namespace

namespace fh {

struct GatherDevice {
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t nq = 0, nr = 0, dist_slice = 0, gather_slice = 0, min_overlap = 1;
    uint64_t max_pairs = 0;
    uint64_t *qh = nullptr, *qoff = nullptr, *rh = nullptr, *roff = nullptr;
    uint32_t *qcnt = nullptr, *qflag = nullptr, *rflag = nullptr;
    uint32_t *cnt = nullptr;      // the counting pass: 3 u32 per pair
    GatherCand *list = nullptr;   // ... and its list, max_pairs entries
    uint32_t *words = nullptr;    // cursor, error word
    uint32_t *words_h = nullptr;  // pinned
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // a chunk of queries (gather_rounds): grown as needed
    void *cand = nullptr, *cand_off = nullptr, *pos = nullptr, *rec = nullptr;
    size_t cand_cap = 0, cand_off_cap = 0, pos_cap = 0, rec_cap = 0;
    std::vector<uint64_t> qoff_h, roff_h;
};

static int upload(void **dst, const void *src, size_t bytes) {
    const size_t b = std::max<size_t>(bytes, 8); // (an empty side still gets a valid pointer)
    GHIP_TRY(api_dev_malloc(dst, b));
    if (bytes) GHIP_TRY(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
    return FH_OK;
}

// zeroed in the handle's own stream, in front of every kernel that reads it: the stream is non-blocking, so a memset in the
// null stream is not ordered before its launches, and the counting kernel follows a set flag bit to arrays this path does not
// have (dist_counts_query_major: qscale, qmax) -- freshly allocated memory may hold anything another entry just freed
static int zeros(void **dst, size_t bytes, hipStream_t stream) {
    const size_t b = std::max<size_t>(bytes, 8);
    GHIP_TRY(api_dev_malloc(dst, b));
    GHIP_TRY(hipMemsetAsync(*dst, 0, b, stream));
    return FH_OK;
}

static int grow(void **p, size_t *cap, size_t bytes) {
    if (*p && bytes <= *cap) return FH_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr, *cap = 0;
    GHIP_TRY(api_dev_malloc(p, std::max<size_t>(bytes, 8)));
    *cap = std::max<size_t>(bytes, 8);
    return FH_OK;
}

void gather_close(GatherDevice *d) {
    if (!d) return;
    if (hipSetDevice(d->device) == hipSuccess) {
        if (d->stream) (void)hipStreamSynchronize(d->stream);
        for (void *p : {(void *)d->qh, (void *)d->qoff, (void *)d->rh, (void *)d->roff, (void *)d->qcnt, (void *)d->qflag, (void *)d->rflag,
                        (void *)d->cnt, (void *)d->list, (void *)d->words, d->cand, d->cand_off, d->pos, d->rec})
            if (p) (void)hipFree(p);
        if (d->words_h) (void)hipHostFree(d->words_h);
        if (d->ev0) (void)hipEventDestroy(d->ev0);
        if (d->ev1) (void)hipEventDestroy(d->ev1);
        if (d->stream) (void)hipStreamDestroy(d->stream);
    }
    (void)hipGetLastError();
    delete d;
}

static int open_into(GatherDevice *d, const GatherSide &q, const GatherSide &r) {
    GHIP_TRY(hipSetDevice(d->device));
    GHIP_TRY(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
    if (int rc = upload((void **)&d->qh, q.hashes, q.offsets[q.n] * sizeof(uint64_t))) return rc;
    if (int rc = upload((void **)&d->qcnt, q.counts, q.offsets[q.n] * sizeof(uint32_t))) return rc;
    if (int rc = upload((void **)&d->qoff, q.offsets, ((size_t)q.n + 1) * sizeof(uint64_t))) return rc;
    if (int rc = upload((void **)&d->rh, r.hashes, r.offsets[r.n] * sizeof(uint64_t))) return rc;
    if (int rc = upload((void **)&d->roff, r.offsets, ((size_t)r.n + 1) * sizeof(uint64_t))) return rc;
    if (int rc = zeros((void **)&d->qflag, q.n * sizeof(uint32_t), d->stream)) return rc;
    if (int rc = zeros((void **)&d->rflag, r.n * sizeof(uint32_t), d->stream)) return rc;
    GHIP_TRY(api_dev_malloc((void **)&d->cnt, std::max<uint64_t>(d->max_pairs, 1) * 3 * sizeof(uint32_t)));
    GHIP_TRY(api_dev_malloc((void **)&d->list, std::max<uint64_t>(d->max_pairs, 1) * sizeof(GatherCand)));
    if (int rc = zeros((void **)&d->words, 2 * sizeof(uint32_t), d->stream)) return rc;
    GHIP_TRY(api_host_malloc((void **)&d->words_h, 2 * sizeof(uint32_t)));
    GHIP_TRY(hipEventCreate(&d->ev0));
    GHIP_TRY(hipEventCreate(&d->ev1));
    // the rounds kernel's mask may take all of GATHER_MAX_QUERY bits: above the 64 KiB a launch gets unasked
    GHIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_gather_rounds), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)(GATHER_MAX_QUERY / 8)));
    return FH_OK;
}

int gather_open(int device, const GatherSide &q, const GatherSide &r, uint32_t dist_slice, uint32_t gather_slice, uint64_t max_pairs,
                uint32_t min_overlap, GatherDevice **out) {
    if (max_pairs > (1ull << 31)) return api_fail(FH_ERR_INVALID, "gather_open: %llu pairs per launch", (unsigned long long)max_pairs);
    GatherDevice *d = new (std::nothrow) GatherDevice;
    if (!d) return api_fail(FH_ERR_CAPACITY, "out of host memory");
    d->device = device;
    d->nq = q.n, d->nr = r.n;
    d->max_pairs = max_pairs;
    d->min_overlap = std::max(min_overlap, 1u);
    uint64_t longest = 1;
    for (uint32_t s = 0; s < q.n; ++s) longest = std::max<uint64_t>(longest, q.offsets[s + 1] - q.offsets[s]);
    d->dist_slice = (uint32_t)std::min<uint64_t>(std::min(std::max(dist_slice, 1u), DIST_MAX_SLICE), longest);
    d->gather_slice = (uint32_t)std::min<uint64_t>(std::min(std::max(gather_slice, 1u), GATHER_MAX_SLICE), longest);
    d->qoff_h.assign(q.offsets, q.offsets + q.n + 1);
    d->roff_h.assign(r.offsets, r.offsets + r.n + 1);
    if (longest > GATHER_MAX_QUERY) {
        delete d;
        return api_fail(FH_ERR_UNSUPPORTED, "gather_open: a query of %llu hashes", (unsigned long long)longest);
    }
    if (int rc = open_into(d, q, r)) {
        gather_close(d);
        return rc;
    }
    *out = d;
    return FH_OK;
}

static int elapsed(GatherDevice *d, double *kernel_ms) {
    float ms = 0.f;
    GHIP_TRY(hipEventElapsedTime(&ms, d->ev0, d->ev1));
    if (kernel_ms) *kernel_ms += ms;
    return FH_OK;
}

int gather_count(GatherDevice *d, uint32_t r0, uint32_t r1, std::vector<GatherCand> *out, double *kernel_ms, uint64_t *launches) {
    if (r1 <= r0 || r1 > d->nr || d->nq == 0 || (uint64_t)(r1 - r0) * d->nq > d->max_pairs)
        return api_fail(FH_ERR_INVALID, "gather_count: %u references do not fit the count buffer", r1 - r0);
    GHIP_TRY(hipSetDevice(d->device));
    const uint32_t pairs = (uint32_t)((uint64_t)(r1 - r0) * d->nq);
    DistDeviceArrays da{d->qh, d->qoff, d->rh, d->roff, d->qflag, d->rflag, d->nq, d->dist_slice};
    CandArgs ca;
    ca.cnt = d->cnt;
    ca.n = r1 - r0;
    ca.r0 = r0;
    ca.min_overlap = d->min_overlap;
    ca.cap = pairs;
    ca.list = d->list;
    ca.cursor = d->words;
    GHIP_TRY(hipEventRecord(d->ev0, d->stream));
    GHIP_TRY(hipMemsetAsync(d->words, 0, sizeof(uint32_t), d->stream));
    if (int rc = dist_counts_query_major(da, r0, r1, d->cnt, d->stream)) return rc;
    hipLaunchKernelGGL(k_gather_candidates, dim3(d->nq), dim3(CAND_THREADS), 0, d->stream, ca);
    GHIP_TRY(hipGetLastError());
    GHIP_TRY(hipEventRecord(d->ev1, d->stream));
    GHIP_TRY(hipMemcpyAsync(d->words_h, d->words, sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
    GHIP_TRY(hipStreamSynchronize(d->stream));
    if (int rc = elapsed(d, kernel_ms)) return rc;
    if (launches) *launches += 2;
    const uint32_t n = d->words_h[0];
    if (n > pairs) return api_fail(FH_ERR_STATE, "gather: %u candidates from %u pairs", n, pairs);
    const size_t had = out->size();
    out->resize(had + n);
    if (n) GHIP_TRY(hipMemcpy(out->data() + had, d->list, (size_t)n * sizeof(GatherCand), hipMemcpyDeviceToHost));
    return FH_OK;
}

int gather_rounds(GatherDevice *d, uint32_t q0, uint32_t q1, const GatherCand *cands, uint64_t n, uint32_t max_rounds,
                  std::vector<GatherRecord> *out, double *kernel_ms, uint64_t *launches) {
    if (q0 >= q1 || q1 > d->nq || n == 0 || n >= (1ull << 31)) return api_fail(FH_ERR_INVALID, "gather_rounds: queries [%u, %u), %llu candidates", q0, q1, (unsigned long long)n);
    GHIP_TRY(hipSetDevice(d->device));
    // the candidates in the device's form, each query's range, the records the chunk can give at most, its longest query
    std::vector<CandDev> cd(n);
    std::vector<uint64_t> off((size_t)(q1 - q0) + 1, 0);
    uint64_t n_pos = 0, n_rec = 0, longest = 1;
    for (uint64_t i = 0; i < n; ++i) {
        const GatherCand &c = cands[i];
        const bool ordered = i == 0 || cands[i - 1].q < c.q || (cands[i - 1].q == c.q && cands[i - 1].r < c.r);
        if (c.q < q0 || c.q >= q1 || c.r >= d->nr || !ordered || c.common == 0 || c.common > d->qoff_h[c.q + 1] - d->qoff_h[c.q] ||
            c.common > d->roff_h[c.r + 1] - d->roff_h[c.r])
            return api_fail(FH_ERR_STATE, "gather: candidate (%u, %u) with %u common hashes", c.q, c.r, c.common);
        cd[i] = CandDev{c.q, c.r, c.common, c.common, n_pos};
        n_pos += c.common;
        ++off[c.q - q0 + 1];
    }
    for (uint32_t b = 0; b < q1 - q0; ++b) {
        n_rec += max_rounds ? std::min<uint64_t>(max_rounds, off[b + 1]) : off[b + 1];
        if (off[b + 1]) longest = std::max<uint64_t>(longest, d->qoff_h[q0 + b + 1] - d->qoff_h[q0 + b]);
        off[b + 1] += off[b];
    }
    if (n_rec >= (1ull << 31)) return api_fail(FH_ERR_STATE, "gather: %llu records in one chunk", (unsigned long long)n_rec);
    if (int rc = grow(&d->cand, &d->cand_cap, n * sizeof(CandDev))) return rc;
    if (int rc = grow(&d->cand_off, &d->cand_off_cap, off.size() * sizeof(uint64_t))) return rc;
    if (int rc = grow(&d->pos, &d->pos_cap, n_pos * sizeof(uint32_t))) return rc;
    if (int rc = grow(&d->rec, &d->rec_cap, n_rec * sizeof(GatherRecord))) return rc;
    GHIP_TRY(hipMemcpyAsync(d->cand, cd.data(), n * sizeof(CandDev), hipMemcpyHostToDevice, d->stream));
    GHIP_TRY(hipMemcpyAsync(d->cand_off, off.data(), off.size() * sizeof(uint64_t), hipMemcpyHostToDevice, d->stream));
    GHIP_TRY(hipMemsetAsync(d->words, 0, 2 * sizeof(uint32_t), d->stream));
    PosArgs pa;
    pa.qh = d->qh, pa.qoff = d->qoff, pa.rh = d->rh, pa.roff = d->roff;
    pa.cand = (const CandDev *)d->cand;
    pa.pos = (uint32_t *)d->pos;
    pa.slice = d->gather_slice;
    pa.err = d->words + 1;
    RoundArgs ra;
    ra.qoff = d->qoff, ra.roff = d->roff, ra.qcnt = d->qcnt;
    ra.cand = (CandDev *)d->cand;
    ra.cand_off = (const uint64_t *)d->cand_off;
    ra.pos = (const uint32_t *)d->pos;
    ra.q0 = q0, ra.min_overlap = d->min_overlap, ra.max_rounds = max_rounds;
    ra.rec = (GatherRecord *)d->rec;
    ra.rec_cap = (uint32_t)n_rec;
    ra.cursor = d->words;
    ra.err = d->words + 1;
    ra.mask_words = (uint32_t)((longest + 31) / 32); // longest: over the queries that have candidates
    const size_t mask_bytes = (size_t)ra.mask_words * sizeof(uint32_t);
    GHIP_TRY(hipEventRecord(d->ev0, d->stream));
    hipLaunchKernelGGL(k_gather_positions, dim3((uint32_t)n), dim3(64), d->gather_slice * sizeof(uint64_t), d->stream, pa);
    GHIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_gather_rounds, dim3(q1 - q0), dim3(ROUND_THREADS), mask_bytes, d->stream, ra);
    GHIP_TRY(hipGetLastError());
    GHIP_TRY(hipEventRecord(d->ev1, d->stream));
    GHIP_TRY(hipMemcpyAsync(d->words_h, d->words, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
    GHIP_TRY(hipStreamSynchronize(d->stream)); // (cd and off are this frame's)
    if (int rc = elapsed(d, kernel_ms)) return rc;
    if (launches) *launches += 2;
    const uint32_t rows = d->words_h[0], err = d->words_h[1];
    if (err) return api_fail(FH_ERR_STATE, "gather: the %s kernel found positions that do not match the counts", err & ERR_POSITIONS ? "positions" : "rounds");
    if (rows > n_rec) return api_fail(FH_ERR_STATE, "gather: %u records where at most %llu can be", rows, (unsigned long long)n_rec);
    const size_t had = out->size();
    out->resize(had + rows);
    if (rows) GHIP_TRY(hipMemcpy(out->data() + had, d->rec, (size_t)rows * sizeof(GatherRecord), hipMemcpyDeviceToHost));
    return FH_OK;
}

} // namespace fh
