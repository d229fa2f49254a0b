// fh_moments.hip -- Sketch.compare_counts (lib/src/python.rs:496-559) for many (query, reference) pairs on the device: per pair
// the integers the merge walk ends with, the summed counts of the shared hashes on each side, and the sums m2, m3, m4 of the
// one-pass moment recurrence (python.rs:524-535) over the query's counts of the shared hashes.  DESIGN.md §3.11.
//
// The integers do not depend on visiting order (§3.7's reduction with scale 0); the recurrence does, but only over the matches
// of a pair, in hash order.  That fits a wave:
//   * a workgroup holds a slice of one query's (hash, count) entries in LDS; its four waves take the references of its block
//     one at a time;
//   * step m of a reference looks up its entries 64 m .. 64 m + 63, one per lane, with fh_dist.hip's branchless binary search,
//     one equality test, and reads the matching query count;
//   * the lanes' matches are balloted and the wave walks the set bits from low to high -- lanes ascend with the reference's
//     hashes, so that is hash order --, reads each match's query count across the wave and advances the recurrence, the same
//     scalars in every lane;
//   * a query longer than a slice is walked slice by slice: the slices hold disjoint ascending ranges, so the matches still come
//     in hash order, and each reference's running state waits in LDS between slices;
//   * after the last slice one wave ballots the block's pairs that pass common >= min_common, takes their places in the chunk's
//     list with one atomic add and writes a 64-byte record per pair.
// finch_index_compare_counts has the pairs that pass before anything is walked -- the index counted them --:
// k_index_moments gives each a wave, which walks the shorter side from global memory and searches the longer one; no LDS, no
// slices, the same recurrence.
// The recurrence is IEEE double arithmetic as written: no contraction into fused multiply-adds in this file, no fast-math flag
// in the build.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../../include/finch_hip.h"
#include "fh_dist_dev.h"
#include "fh_internal.h"
#include "fh_moments.h"

using namespace fh;

namespace {

#define CHIP_TRY(expr)                                                                                      \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess) return api_fail(FH_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

constexpr uint32_t THREADS = 256; // four waves
constexpr uint32_t WAVES = THREADS / 64;
constexpr uint32_t RB = 64;       // references per workgroup

struct MomentsArgs {
    const uint64_t *qh, *qoff, *rh, *roff;
    const uint32_t *qc, *rc;
    uint32_t nq, r0, r1, slice, min_common;
    MomentsRecord *list; // the chunk's records
    uint32_t *cursor;    // records written (zero before the launch)
};

// a pair's running state between the slices of its query
struct PairState {
    uint32_t common, ref_pos, query_pos, pad;
    uint64_t ref_count, query_count;
    double mean, m2, m3, m4;
};
static_assert(sizeof(PairState) == 64, "64 of them are the workgroup's static LDS");

// #{s[0..n) <= x} over ascending s, n >= 1; top = the largest power of two <= n.  fh_dist.hip's count_below<true>: the same
// number of steps in every lane (the workgroup's n is uniform), no branch; the index is clamped so that no read leaves s[0..n).
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

// python.rs:524-535 for one shared hash whose query count is `count`: the statements in their order and association
__device__ inline void moment_step(PairState &st, uint32_t count) {
#pragma clang fp contract(off)
    const double n = (double)st.common + 1.;
    const double float_count = (double)count;
    const double delta = float_count - st.mean;
    const double delta_n = delta / n;
    const double delta_n2 = delta_n * delta_n;
    const double term1 = delta * delta_n * (n - 1.);
    st.mean += delta_n;
    st.m4 += term1 * delta_n2 * (n * n - 3. * n + 3.) + 6. * delta_n2 * st.m2 - 4. * delta_n * st.m3;
    st.m3 += term1 * delta_n * (n - 2.) - 3. * delta_n * st.m2;
    st.m2 += term1;
    st.common += 1;
}

// grid: x = query, y = block of RB references from a.r0; dynamic LDS: a.slice u64 hashes, then a.slice u32 counts
__global__ void __launch_bounds__(THREADS) k_compare_counts(MomentsArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) uint64_t s_h[];
    __shared__ PairState s_st[RB];
    uint32_t *s_c = (uint32_t *)(s_h + a.slice);
    const uint32_t q = blockIdx.x;
    const uint32_t rb0 = a.r0 + blockIdx.y * RB, rb1 = min(rb0 + RB, a.r1);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t qa = a.qoff[q];
    const uint32_t nqh = (uint32_t)(a.qoff[q + 1] - qa);
    const uint64_t *Q = a.qh + qa;
    const uint32_t *QC = a.qc + qa;
    const uint64_t max_q = nqh ? Q[nqh - 1] : 0;
    for (uint32_t i = threadIdx.x; i < RB * sizeof(PairState) / sizeof(uint32_t); i += THREADS) ((uint32_t *)s_st)[i] = 0; // (0.0 is all zero bits)
    for (uint32_t s0 = 0; s0 < nqh; s0 += a.slice) { // (an empty query: every pair's state stays zero)
        const uint32_t ns = min(a.slice, nqh - s0); // >= 1
        const uint32_t top = 1u << (31 - __clz(ns));
        __syncthreads(); // the previous slice is no longer read
        for (uint32_t i = threadIdx.x; i < ns; i += THREADS) {
            s_h[i] = Q[s0 + i];
            s_c[i] = QC[s0 + i];
        }
        __syncthreads();
        for (uint32_t r = rb0 + wave; r < rb1; r += WAVES) { // (a wave writes and reads only its own references' states)
            const uint64_t ra = a.roff[r];
            const uint32_t nrh = (uint32_t)(a.roff[r + 1] - ra);
            const uint64_t *R = a.rh + ra;
            const uint32_t *RC = a.rc + ra;
            PairState st = s_st[r - rb0];
            uint32_t rle = 0;
            uint64_t rsum = 0, qsum = 0;
            for (uint32_t t0 = 0; t0 < nrh; t0 += 64) { // (whole waves go round: the ballot sees every lane)
                const uint32_t t = t0 + lane;
                const bool valid = t < nrh;
                const uint64_t x = valid ? R[t] : 0;
                const uint32_t p = count_le(s_h, ns, top, x);
                const uint32_t at = p ? p - 1 : 0;
                const bool match = valid && p && s_h[at] == x;
                const uint32_t qcnt = match ? s_c[at] : 0;
                qsum += qcnt;
                if (match) rsum += RC[t];
                rle += valid && x <= max_q;
                uint64_t mask = __ballot(match);
                while (mask) { // lanes ascend with the reference's hashes: low to high is hash order
                    const int b = __ffsll((unsigned long long)mask) - 1;
                    mask &= mask - 1;
                    moment_step(st, (uint32_t)__shfl((int)qcnt, b, 64));
                }
            }
            st.ref_count += wave_sum64(rsum);
            st.query_count += wave_sum64(qsum);
            if (s0 == 0) st.ref_pos = wave_sum(rle); // #{r <= max Q}: every reference hash is read anyway
            st.query_pos += nrh ? count_le(s_h, ns, top, R[nrh - 1]) : 0; // #{q <= max R}: the slices' shares add
            if (lane == 0) s_st[r - rb0] = st;
        }
    }
    __syncthreads();
    if (wave == 0) { // the block's references are final: lane l has reference rb0 + l
        const uint32_t r = rb0 + lane;
        const PairState st = s_st[lane];
        const bool pass = r < rb1 && st.common >= a.min_common;
        const uint64_t mask = __ballot(pass);
        if (mask) {
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
            uint32_t first = 0;
            if (pass && rank == 0) first = atomicAdd(a.cursor, (uint32_t)__popcll(mask));
            first = __shfl(first, __ffsll((unsigned long long)mask) - 1, 64);
            if (pass) {
                MomentsRecord rec;
                rec.q = q, rec.r = r, rec.common = st.common, rec.ref_pos = st.ref_pos, rec.query_pos = st.query_pos, rec.pad = 0;
                rec.ref_count = st.ref_count, rec.query_count = st.query_count;
                rec.m2 = st.m2, rec.m3 = st.m3, rec.m4 = st.m4;
                a.list[first + rank] = rec;
            }
        }
    }
}

// finch_index_compare_counts.  grid-stride over the pass list, one wave per pair, no LDS: the wave walks the
// shorter side, 64 consecutive entries a step, one per lane, and each lane looks its hash up in the longer side with the
// clamped bound search over global memory (no read leaves either side).  Lanes ascend with the walked side's hashes and steps
// ascend, so the ballot's bits from low to high are hash order whichever side is walked; the recurrence is k_compare_counts':
// every lane advances the same scalars with the match's query count.  The record goes to the pair's own place in the list.
__global__ void __launch_bounds__(THREADS) k_index_moments(IndexMomentsArgs a) {
#pragma clang fp contract(off)
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); // (what follows is the same in every lane)
    for (uint32_t p = blockIdx.x * WAVES + wave; p < a.n_pass; p += gridDim.x * WAVES) {
        const IndexPass e = a.pass[p];
        const uint32_t b = e.q - a.q0;
        PairState st = {};
        bool bad = b >= a.nq || e.r >= a.nr;
        if (!bad) {
            const uint64_t qa = a.qoff[b], ra = a.roff[e.r];
            const uint32_t nqh = (uint32_t)(a.qoff[b + 1] - qa), nrh = (uint32_t)(a.roff[e.r + 1] - ra);
            bad = !nqh || !nrh; // (c > 0: neither side is empty)
            if (!bad) {
                const uint64_t *Q = a.qh + (qa - a.qbase), *R = a.rh + ra;
                const uint32_t *QC = a.qc + (qa - a.qbase), *RC = a.rc + ra;
                const bool walk_q = nqh <= nrh;
                const uint64_t *W = walk_q ? Q : R, *S = walk_q ? R : Q; // walked, searched
                const uint32_t *WC = walk_q ? QC : RC, *SC = walk_q ? RC : QC;
                const uint32_t nw = walk_q ? nqh : nrh, ns = walk_q ? nrh : nqh;
                const uint32_t stop = 1u << (31 - __clz(ns));
                uint64_t wsum = 0, ssum = 0;
                for (uint32_t t0 = 0; t0 < nw; t0 += 64) { // (whole waves go round: the ballot sees every lane)
                    const uint32_t t = t0 + lane;
                    const bool valid = t < nw;
                    const uint64_t x = valid ? W[t] : 0;
                    const uint32_t pos = count_below<true>(S, ns, stop, x);
                    const uint32_t at = pos ? pos - 1 : 0;
                    const bool match = valid && pos && S[at] == x;
                    const uint32_t wcnt = match ? WC[t] : 0, scnt = match ? SC[at] : 0;
                    wsum += wcnt, ssum += scnt;
                    const uint32_t qcnt = walk_q ? wcnt : scnt;
                    uint64_t mask = __ballot(match);
                    while (mask) {
                        const int bit = __ffsll((unsigned long long)mask) - 1;
                        mask &= mask - 1;
                        moment_step(st, (uint32_t)__shfl((int)qcnt, bit, 64));
                    }
                }
                wsum = wave_sum64(wsum), ssum = wave_sum64(ssum);
                st.query_count = walk_q ? wsum : ssum;
                st.ref_count = walk_q ? ssum : wsum;
                st.ref_pos = count_below<true>(R, nrh, 1u << (31 - __clz(nrh)), Q[nqh - 1]); // #{r <= max Q}
                st.query_pos = count_below<true>(Q, nqh, 1u << (31 - __clz(nqh)), R[nrh - 1]); // #{q <= max R}
                bad = st.common != e.c;
            }
        }
        if (lane == 0) {
            if (bad && atomicCAS(&a.err[0], 0u, 1u) == 0) a.err[1] = e.q, a.err[2] = e.r; // (the first such pair is named)
            MomentsRecord rec;
            rec.q = e.q, rec.r = e.r, rec.common = st.common, rec.ref_pos = st.ref_pos, rec.query_pos = st.query_pos, rec.pad = 0;
            rec.ref_count = st.ref_count, rec.query_count = st.query_count;
            rec.m2 = st.m2, rec.m3 = st.m3, rec.m4 = st.m4;
            a.rec[p] = rec;
        }
    }
}

} // namespace

namespace fh {

int index_moments_launch(const IndexMomentsArgs &a, void *stream) {
    if (!a.n_pass || !a.pass || !a.rec || !a.err || !a.qc || !a.rc)
        return api_fail(FH_ERR_INVALID, "index_moments_launch: %u pairs, or an array is missing", a.n_pass);
    const uint32_t blocks = std::min<uint32_t>((a.n_pass + WAVES - 1) / WAVES, 8192u); // (a grid-stride loop takes the rest)
    hipLaunchKernelGGL(k_index_moments, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, a);
    CHIP_TRY(hipGetLastError());
    return FH_OK;
}

struct MomentsDevice {
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t nq = 0, nr = 0, lds_slice = 0, min_common = 0;
    uint64_t max_pairs = 0;
    void *dev[6] = {}; // qh qc qoff rh rc roff
    MomentsRecord *list_d[2] = {};
    uint32_t *cursor_d[2] = {}, *cursor_h[2] = {};
    hipEvent_t ev0[2] = {}, ev1[2] = {}, done[2] = {};
    uint32_t launched_pairs[2] = {};
    std::vector<MomentsRecord> list_h[2];
};

static int upload(void **dst, const void *src, size_t bytes) {
    const size_t b = std::max<size_t>(bytes, 8); // (an empty side still gets a valid pointer)
    CHIP_TRY(api_dev_malloc(dst, b));
    if (bytes) CHIP_TRY(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
    return FH_OK;
}

void moments_close(MomentsDevice *d) {
    if (!d) return;
    if (hipSetDevice(d->device) == hipSuccess) {
        if (d->stream) (void)hipStreamSynchronize(d->stream);
        for (void *p : d->dev)
            if (p) (void)hipFree(p);
        for (int b = 0; b < 2; ++b) {
            if (d->list_d[b]) (void)hipFree(d->list_d[b]);
            if (d->cursor_d[b]) (void)hipFree(d->cursor_d[b]);
            if (d->cursor_h[b]) (void)hipHostFree(d->cursor_h[b]);
            if (d->ev0[b]) (void)hipEventDestroy(d->ev0[b]);
            if (d->ev1[b]) (void)hipEventDestroy(d->ev1[b]);
            if (d->done[b]) (void)hipEventDestroy(d->done[b]);
        }
        if (d->stream) (void)hipStreamDestroy(d->stream);
    }
    (void)hipGetLastError();
    delete d;
}

static int open_into(MomentsDevice *d, const MomentsSide &q, const MomentsSide &r) {
    CHIP_TRY(hipSetDevice(d->device));
    CHIP_TRY(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
    const MomentsSide *side[2] = {&q, &r};
    for (int s = 0; s < 2; ++s) {
        const MomentsSide &x = *side[s];
        void **p = d->dev + 3 * s;
        if (int rc = upload(&p[0], x.hashes, x.offsets[x.n] * sizeof(uint64_t))) return rc;
        if (int rc = upload(&p[1], x.counts, x.offsets[x.n] * sizeof(uint32_t))) return rc;
        if (int rc = upload(&p[2], x.offsets, ((size_t)x.n + 1) * sizeof(uint64_t))) return rc;
    }
    for (int b = 0; b < 2; ++b) {
        CHIP_TRY(api_dev_malloc((void **)&d->list_d[b], std::max<uint64_t>(d->max_pairs, 1) * sizeof(MomentsRecord)));
        CHIP_TRY(api_dev_malloc((void **)&d->cursor_d[b], sizeof(uint32_t)));
        CHIP_TRY(api_host_malloc((void **)&d->cursor_h[b], sizeof(uint32_t)));
        CHIP_TRY(hipEventCreate(&d->ev0[b]));
        CHIP_TRY(hipEventCreate(&d->ev1[b]));
        CHIP_TRY(hipEventCreateWithFlags(&d->done[b], hipEventDisableTiming));
    }
    return FH_OK;
}

// a side's offsets as the kernel reads them: from 0, ascending, no sketch of 2^32 - 1 entries or more; *longest = its longest sketch
static int check_side(const MomentsSide &x, const char *what, uint64_t *longest) {
    if (!x.offsets || x.offsets[0] != 0) return api_fail(FH_ERR_INVALID, "moments_open: the %s offsets do not start at 0", what);
    *longest = 0;
    for (uint32_t s = 0; s < x.n; ++s) {
        if (x.offsets[s + 1] < x.offsets[s] || x.offsets[s + 1] - x.offsets[s] >= UINT32_MAX)
            return api_fail(FH_ERR_INVALID, "moments_open: offsets of %s sketch %u", what, s);
        *longest = std::max(*longest, x.offsets[s + 1] - x.offsets[s]);
    }
    if (x.offsets[x.n] && (!x.hashes || !x.counts)) return api_fail(FH_ERR_INVALID, "moments_open: the %s side has no entries", what);
    return FH_OK;
}

int moments_open(int device, const MomentsSide &q, const MomentsSide &r, uint32_t slice, uint64_t max_pairs, uint32_t min_common,
                 MomentsDevice **out) {
    if (!out || !q.n || !r.n || !max_pairs || max_pairs > (1ull << 31)) // (the cursor is a u32)
        return api_fail(FH_ERR_INVALID, "moments_open: %u queries, %u references, %llu pairs per launch", q.n, r.n, (unsigned long long)max_pairs);
    uint64_t longest = 0, longest_r = 0;
    if (int rc = check_side(q, "query", &longest)) return rc;
    if (int rc = check_side(r, "reference", &longest_r)) return rc;
    MomentsDevice *d = new (std::nothrow) MomentsDevice;
    if (!d) return api_fail(FH_ERR_CAPACITY, "out of host memory");
    d->device = device;
    d->nq = q.n;
    d->nr = r.n;
    d->min_common = min_common;
    d->max_pairs = max_pairs;
    // LDS the launches ask for: no more than the longest query needs
    d->lds_slice = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({std::max(slice, 1u), MOMENTS_MAX_SLICE, longest}));
    if (int rc = open_into(d, q, r)) {
        moments_close(d);
        return rc;
    }
    *out = d;
    return FH_OK;
}

int moments_launch(MomentsDevice *d, int buf, uint32_t r0, uint32_t r1) {
    // everything the kernel indexes with: references inside what was uploaded, no more pairs than the list holds, a grid that fits
    if (!d || (buf != 0 && buf != 1)) return api_fail(FH_ERR_INVALID, "moments_launch: handle or buffer");
    if (r1 <= r0 || r1 > d->nr || (uint64_t)(r1 - r0) * d->nq > d->max_pairs || (r1 - r0 + RB - 1) / RB > 65535u)
        return api_fail(FH_ERR_INVALID, "moments_launch: references %u .. %u of %u do not fit the record list", r0, r1, d->nr);
    CHIP_TRY(hipSetDevice(d->device));
    MomentsArgs a;
    a.qh = (const uint64_t *)d->dev[0];
    a.qc = (const uint32_t *)d->dev[1];
    a.qoff = (const uint64_t *)d->dev[2];
    a.rh = (const uint64_t *)d->dev[3];
    a.rc = (const uint32_t *)d->dev[4];
    a.roff = (const uint64_t *)d->dev[5];
    a.nq = d->nq;
    a.r0 = r0;
    a.r1 = r1;
    a.slice = d->lds_slice;
    a.min_common = d->min_common;
    a.list = d->list_d[buf];
    a.cursor = d->cursor_d[buf];
    d->launched_pairs[buf] = (uint32_t)((uint64_t)(r1 - r0) * d->nq);
    CHIP_TRY(hipEventRecord(d->ev0[buf], d->stream));
    CHIP_TRY(hipMemsetAsync(d->cursor_d[buf], 0, sizeof(uint32_t), d->stream));
    const size_t lds = (size_t)d->lds_slice * (sizeof(uint64_t) + sizeof(uint32_t));
    hipLaunchKernelGGL(k_compare_counts, dim3(d->nq, (r1 - r0 + RB - 1) / RB), dim3(THREADS), lds, d->stream, a);
    CHIP_TRY(hipGetLastError());
    CHIP_TRY(hipEventRecord(d->ev1[buf], d->stream));
    CHIP_TRY(hipMemcpyAsync(d->cursor_h[buf], d->cursor_d[buf], sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
    CHIP_TRY(hipEventRecord(d->done[buf], d->stream));
    return FH_OK;
}

int moments_wait(MomentsDevice *d, int buf, const MomentsRecord **records, uint64_t *n, double *kernel_ms) {
    CHIP_TRY(hipSetDevice(d->device));
    CHIP_TRY(hipEventSynchronize(d->done[buf]));
    float ms = 0.f;
    CHIP_TRY(hipEventElapsedTime(&ms, d->ev0[buf], d->ev1[buf]));
    if (kernel_ms) *kernel_ms = ms;
    const uint32_t cursor = d->cursor_h[buf][0];
    if (cursor > d->launched_pairs[buf]) return api_fail(FH_ERR_STATE, "compare_counts: %u records from %u pairs", cursor, d->launched_pairs[buf]);
    std::vector<MomentsRecord> &list = d->list_h[buf];
    list.resize(cursor);
    // (not on the handle's stream, where the next chunk's kernel may already wait: the records are complete, `done` says so)
    if (cursor) CHIP_TRY(hipMemcpy(list.data(), d->list_d[buf], (size_t)cursor * sizeof(MomentsRecord), hipMemcpyDeviceToHost));
    *records = list.data();
    *n = cursor;
    return FH_OK;
}

} // namespace fh
