// fh_dist.hip -- many-vs-many sketch comparison (finch dist, cli/src/main.rs:85-125 / 315-333) on the device: for every
// (query, reference) pair the integer counts that distance.rs:66-126's merge walk ends with; the host (fh_host.cpp, finch_dist)
// turns them into the doubles with the same function finch_distance uses.  DESIGN.md §3.7 has the reduction.
//
// For strictly ascending Q (query) and R (reference) the walk stops with c = |Q n R|, i0 = #{q <= max R}, j0 = #{r <= max Q}
// (both 0 if either list is empty); the scale step makes i = max(i0, #{q < M}), j = max(j0, #{r < M}).  None of that depends on
// visiting pairs in order:
//   * a workgroup holds a slice of one query's hashes in LDS; its four waves take the references of its block one at a time,
//     each lane looks up the reference hashes t = lane, lane + 64, ... with a branchless binary search in the slice;
//   * #{r <= max Q} and #{r < M} are counted by the same lanes on the way (every reference hash is read anyway), #{q <= max R}
//     and #{q < M} are one wave-uniform binary search each in the slice;
//   * a query longer than a slice is walked slice by slice: the slices hold disjoint value ranges, so every count adds.
// The per-reference sums live in LDS until the last slice; the result is 3 u32 per pair, written with plain stores.
//
// The search (finch_search) keeps those counts on the device: a second kernel per chunk, one workgroup per query,
// selects from them by containment = c / j and only what it selected crosses to the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../../include/finch_hip.h"
#include "fh_dist.h"
#include "fh_dist_dev.h"
#include "fh_internal.h"

using namespace fh;

namespace {

#define DHIP_TRY(expr)                                                                                      \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess) return api_fail(FH_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

constexpr uint32_t THREADS = 256; // four waves
constexpr uint32_t WAVES = THREADS / 64;
constexpr uint32_t RB = 64;       // references per workgroup

struct DistArgs {
    const uint64_t *qh, *qoff, *rh, *roff, *qmax, *rmax;
    const uint32_t *qflag, *rflag;
    const double *qscale, *rscale;
    uint32_t nq, r0, r1, slice;
    uint32_t *out;
};

__device__ inline uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// grid: x = query, y = block of RB references from a.r0; dynamic LDS: a.slice u64.  The counts of pair (q, r) go to
// ((r - r0) * nq + q) * 3, finch_dist's order, or -- QUERY_MAJOR, the search's -- to (q * (r1 - r0) + (r - r0)) * 3: there a query's
// counts of the chunk are contiguous for k_search_top / k_search_all, and the stores below, which walk r across threads, coalesce.
template <bool QUERY_MAJOR>
__global__ void __launch_bounds__(THREADS) k_dist_counts(DistArgs a) {
    extern __shared__ uint64_t s_q[];
    __shared__ uint32_t s_acc[RB][5]; // c, #{q <= max R}, #{q < M}, #{r <= max Q}, #{r < M}
    const uint32_t q = blockIdx.x;
    const uint32_t rb0 = a.r0 + blockIdx.y * RB, rb1 = min(rb0 + RB, a.r1);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t qa = a.qoff[q];
    const uint32_t nqh = (uint32_t)(a.qoff[q + 1] - qa);
    const uint64_t *Q = a.qh + qa;
    const uint64_t max_q = nqh ? Q[nqh - 1] : 0;
    for (uint32_t i = threadIdx.x; i < RB * 5; i += THREADS) (&s_acc[0][0])[i] = 0;
    for (uint32_t s0 = 0; s0 == 0 || s0 < nqh; s0 += a.slice) { // (one pass for an empty query: the reference-side counts)
        const uint32_t ns = nqh ? min(a.slice, nqh - s0) : 0;
        const uint32_t top = ns ? 1u << (31 - __clz(ns)) : 0;
        __syncthreads(); // the previous slice is no longer read
        for (uint32_t i = threadIdx.x; i < ns; i += THREADS) s_q[i] = Q[s0 + i];
        __syncthreads();
        for (uint32_t r = rb0 + wave; r < rb1; r += WAVES) {
            const uint64_t ra = a.roff[r];
            const uint32_t nrh = (uint32_t)(a.roff[r + 1] - ra);
            const uint64_t *R = a.rh + ra;
            uint64_t m = 0;
            const bool has_m = pair_max_hash(a, q, r, m);
            uint32_t c = 0, rle = 0, rlt = 0;
            if (ns) {
                for (uint32_t t = lane; t < nrh; t += 64) {
                    const uint64_t x = R[t];
                    const uint32_t p = count_below<true>(s_q, ns, top, x);
                    const uint64_t v = s_q[p ? p - 1 : 0];
                    c += p && v == x;
                    rle += x <= max_q;
                    rlt += has_m && x < m;
                }
            } else {
                for (uint32_t t = lane; t < nrh; t += 64) rlt += has_m && R[t] < m;
            }
            c = wave_sum(c);
            if (s0 == 0) {
                rle = wave_sum(rle);
                rlt = wave_sum(rlt);
            }
            const uint32_t qle = nrh ? count_below<true>(s_q, ns, top, R[nrh - 1]) : 0;
            const uint32_t qlt = has_m ? count_below<false>(s_q, ns, top, m) : 0;
            if (lane == 0) {
                uint32_t *acc = s_acc[r - rb0];
                acc[0] += c;
                acc[1] += qle;
                acc[2] += qlt;
                if (s0 == 0) {
                    acc[3] = rle;
                    acc[4] = rlt;
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t r = rb0 + threadIdx.x; r < rb1; r += THREADS) {
        const uint32_t *acc = s_acc[r - rb0];
        const uint32_t nrh = (uint32_t)(a.roff[r + 1] - a.roff[r]);
        const bool both = nqh && nrh;
        uint32_t i = both ? acc[1] : 0, j = both ? acc[3] : 0;
        uint64_t m = 0;
        if (pair_max_hash(a, q, r, m)) {
            i = max(i, acc[2]);
            j = max(j, acc[4]);
        }
        uint32_t *o = a.out + (QUERY_MAJOR ? (uint64_t)q * (a.r1 - a.r0) + (r - a.r0) : (uint64_t)(r - a.r0) * a.nq + q) * 3;
        o[0] = acc[0];
        o[1] = i;
        o[2] = j;
    }
}

// ---- the search's selection: what of a chunk's counts the host gets to see ----
struct SearchArgs {
    const uint32_t *cnt; // the chunk's counts, query-major
    uint32_t n, r0;      // references of the chunk, the first one's index
    uint32_t top_n;      // top mode: entries per query
    double min_c;
    uint32_t *sel;       // top mode: nq x top_n entries (r, c, i, j); all mode: the chunk's list of entries (q, r, c, i, j)
    uint32_t *count;     // top mode: nq, the entries each query got; all mode: the list's cursor (zero before the launch)
};

constexpr uint32_t NONE = 0xffffffffu;

// is candidate (xb, xt) ahead of (yb, yt) in the search's order: containment descending, then index ascending; NONE loses
__device__ inline bool ahead(uint64_t xb, uint32_t xt, uint64_t yb, uint32_t yt) {
    return xt != NONE && (yt == NONE || xb > yb || (xb == yb && xt < yt));
}

// grid: x = query.  top_n rounds of a workgroup arg-max over the chunk's pairs with containment >= min_c; round k looks only at
// what comes strictly after round k - 1's winner in that order, so nothing is marked and nothing depends on timing.
__global__ void __launch_bounds__(THREADS) k_search_top(SearchArgs a) {
    __shared__ uint64_t s_bits[WAVES];
    __shared__ uint32_t s_t[WAVES];
    const uint32_t q = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t *cnt = a.cnt + (uint64_t)q * a.n * 3;
    uint64_t prev_bits = ~0ull; // (above every double's pattern: the first round takes any)
    uint32_t prev_t = 0, emitted = 0;
    for (uint32_t k = 0; k < a.top_n; ++k) {
        uint64_t best_bits = 0;
        uint32_t best_t = NONE;
        for (uint32_t t = threadIdx.x; t < a.n; t += THREADS) { // (t ascends: of equal containments the thread keeps its first)
            const double x = containment_of(cnt[(uint64_t)t * 3], cnt[(uint64_t)t * 3 + 2]);
            const uint64_t bits = (uint64_t)__double_as_longlong(x);
            const bool after = bits < prev_bits || (bits == prev_bits && t > prev_t);
            if (x >= a.min_c && after && (best_t == NONE || bits > best_bits)) best_bits = bits, best_t = t;
        }
        for (int o = 32; o; o >>= 1) {
            const uint64_t ob = __shfl_xor(best_bits, o, 64);
            const uint32_t ot = __shfl_xor(best_t, o, 64);
            if (ahead(ob, ot, best_bits, best_t)) best_bits = ob, best_t = ot;
        }
        if (lane == 0) s_bits[wave] = best_bits, s_t[wave] = best_t;
        __syncthreads();
        best_bits = s_bits[0], best_t = s_t[0];
        for (uint32_t w = 1; w < WAVES; ++w)
            if (ahead(s_bits[w], s_t[w], best_bits, best_t)) best_bits = s_bits[w], best_t = s_t[w];
        __syncthreads(); // (the next round writes s_bits again)
        if (best_t == NONE) break; // the same in every thread
        if (threadIdx.x == 0) {
            const uint32_t *x = cnt + (uint64_t)best_t * 3;
            *(uint4 *)(a.sel + ((uint64_t)q * a.top_n + k) * 4) = make_uint4(a.r0 + best_t, x[0], x[1], x[2]);
        }
        prev_bits = best_bits, prev_t = best_t, ++emitted;
    }
    if (threadIdx.x == 0) a.count[q] = emitted;
}

// grid: x = query.  Every pair of the chunk with containment >= min_c, appended to the chunk's list: a wave takes its places with
// one atomic (ballot, the lanes' ranks by mbcnt), in no particular order -- the host sorts.
__global__ void __launch_bounds__(THREADS) k_search_all(SearchArgs a) {
    const uint32_t q = blockIdx.x;
    const uint32_t *cnt = a.cnt + (uint64_t)q * a.n * 3;
    for (uint32_t base = 0; base < a.n; base += THREADS) { // (whole waves go round: the ballot sees every lane)
        const uint32_t t = base + threadIdx.x;
        uint32_t c = 0, i = 0, j = 0;
        bool pass = false;
        if (t < a.n) {
            const uint32_t *x = cnt + (uint64_t)t * 3;
            c = x[0], i = x[1], j = x[2];
            pass = containment_of(c, j) >= a.min_c;
        }
        const uint64_t mask = __ballot(pass);
        if (!mask) continue;
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        uint32_t first = 0;
        if (pass && rank == 0) first = atomicAdd(a.count, (uint32_t)__popcll(mask));
        first = __shfl(first, __ffsll((unsigned long long)mask) - 1, 64);
        if (pass) {
            uint32_t *e = a.sel + (uint64_t)(first + rank) * 5;
            e[0] = q, e[1] = a.r0 + t, e[2] = c, e[3] = i, e[4] = j;
        }
    }
}

} // namespace

namespace fh {

struct DistDevice {
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t nq = 0, slice = 0, lds_slice = 0;
    uint64_t max_pairs = 0;
    void *dev[10] = {}; // qh qoff qmax qflag qscale rh roff rmax rflag rscale
    uint32_t *out_d[2] = {}, *out_h[2] = {};
    hipEvent_t ev0[2] = {}, ev1[2] = {}, done[2] = {};
    uint32_t launched_pairs[2] = {};
    // the search only (search_open): what the selection leaves per buffer, and where the host receives it
    bool search = false, top_mode = false;
    uint32_t top_n = 0;
    double min_c = 0.;
    uint32_t *sel_d[2] = {}, *count_d[2] = {}; // SearchArgs' sel and count
    uint32_t *sel_h[2] = {}, *count_h[2] = {}; // pinned: the counts (all mode: the cursor); top mode: the entries too
    std::vector<uint32_t> list_h[2];           // all mode: the entries, as many as the cursor says
};

static int upload(void **dst, const void *src, size_t bytes) {
    const size_t b = std::max<size_t>(bytes, 8); // (an empty side still gets a valid pointer)
    DHIP_TRY(api_dev_malloc(dst, b));
    if (bytes) DHIP_TRY(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
    return FH_OK;
}

void dist_close(DistDevice *d) {
    if (!d) return;
    if (hipSetDevice(d->device) == hipSuccess) {
        if (d->stream) (void)hipStreamSynchronize(d->stream);
        for (void *p : d->dev)
            if (p) (void)hipFree(p);
        for (int b = 0; b < 2; ++b) {
            if (d->out_d[b]) (void)hipFree(d->out_d[b]);
            if (d->out_h[b]) (void)hipHostFree(d->out_h[b]);
            if (d->sel_d[b]) (void)hipFree(d->sel_d[b]);
            if (d->count_d[b]) (void)hipFree(d->count_d[b]);
            if (d->sel_h[b]) (void)hipHostFree(d->sel_h[b]);
            if (d->count_h[b]) (void)hipHostFree(d->count_h[b]);
            if (d->ev0[b]) (void)hipEventDestroy(d->ev0[b]);
            if (d->ev1[b]) (void)hipEventDestroy(d->ev1[b]);
            if (d->done[b]) (void)hipEventDestroy(d->done[b]);
        }
        if (d->stream) (void)hipStreamDestroy(d->stream);
    }
    (void)hipGetLastError();
    delete d;
}

static int open_into(DistDevice *d, const DistSide &q, const DistSide &r) {
    DHIP_TRY(hipSetDevice(d->device));
    DHIP_TRY(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
    const DistSide *side[2] = {&q, &r};
    for (int s = 0; s < 2; ++s) {
        const DistSide &x = *side[s];
        void **p = d->dev + 5 * s;
        if (int rc = upload(&p[0], x.hashes, x.offsets[x.n] * sizeof(uint64_t))) return rc;
        if (int rc = upload(&p[1], x.offsets, (x.n + 1) * sizeof(uint64_t))) return rc;
        if (int rc = upload(&p[2], x.max_hash, x.n * sizeof(uint64_t))) return rc;
        if (int rc = upload(&p[3], x.flags, x.n * sizeof(uint32_t))) return rc;
        if (int rc = upload(&p[4], x.scale, x.n * sizeof(double))) return rc;
    }
    for (int b = 0; b < 2; ++b) {
        const size_t bytes = std::max<uint64_t>(d->max_pairs, 1) * 3 * sizeof(uint32_t);
        DHIP_TRY(api_dev_malloc((void **)&d->out_d[b], bytes));
        if (d->search) { // the counts stay on the device
            const size_t n_count = d->top_mode ? std::max(d->nq, 1u) : 1;
            const size_t n_sel = d->top_mode ? (size_t)std::max(d->nq, 1u) * d->top_n * 4 : std::max<uint64_t>(d->max_pairs, 1) * 5;
            DHIP_TRY(api_dev_malloc((void **)&d->sel_d[b], n_sel * sizeof(uint32_t)));
            DHIP_TRY(api_dev_malloc((void **)&d->count_d[b], n_count * sizeof(uint32_t)));
            DHIP_TRY(api_host_malloc((void **)&d->count_h[b], n_count * sizeof(uint32_t)));
            if (d->top_mode) DHIP_TRY(api_host_malloc((void **)&d->sel_h[b], n_sel * sizeof(uint32_t)));
        } else {
            DHIP_TRY(api_host_malloc((void **)&d->out_h[b], bytes));
        }
        DHIP_TRY(hipEventCreate(&d->ev0[b]));
        DHIP_TRY(hipEventCreate(&d->ev1[b]));
        DHIP_TRY(hipEventCreateWithFlags(&d->done[b], hipEventDisableTiming));
    }
    return FH_OK;
}

static int open_device(int device, const DistSide &q, const DistSide &r, uint32_t slice, uint64_t max_pairs, bool search, uint32_t top_n,
                       double min_containment, DistDevice **out) {
    DistDevice *d = new (std::nothrow) DistDevice;
    if (!d) return api_fail(FH_ERR_CAPACITY, "out of host memory");
    d->device = device;
    d->search = search;
    d->top_mode = search && top_n >= 1 && top_n <= SEARCH_TOP_MAX;
    d->top_n = d->top_mode ? top_n : 0;
    d->min_c = min_containment;
    d->nq = q.n;
    d->slice = std::min(std::max(slice, 1u), DIST_MAX_SLICE);
    uint64_t longest = 1;
    for (uint32_t s = 0; s < q.n; ++s) longest = std::max<uint64_t>(longest, q.offsets[s + 1] - q.offsets[s]);
    d->lds_slice = (uint32_t)std::min<uint64_t>(d->slice, longest); // LDS the launch asks for: no more than the longest query
    d->slice = d->lds_slice;
    d->max_pairs = max_pairs;
    if (int rc = open_into(d, q, r)) {
        dist_close(d);
        return rc;
    }
    *out = d;
    return FH_OK;
}

int dist_open(int device, const DistSide &q, const DistSide &r, uint32_t slice, uint64_t max_pairs, DistDevice **out) {
    return open_device(device, q, r, slice, max_pairs, false, 0, 0., out);
}

int search_open(int device, const DistSide &q, const DistSide &r, uint32_t slice, uint64_t max_pairs, uint32_t top_n, double min_containment,
                DistDevice **out) {
    return open_device(device, q, r, slice, max_pairs, true, top_n, min_containment, out);
}

static DistArgs dist_args(const DistDevice *d, int buf, uint32_t r0, uint32_t r1) {
    DistArgs a;
    a.qh = (const uint64_t *)d->dev[0];
    a.qoff = (const uint64_t *)d->dev[1];
    a.qmax = (const uint64_t *)d->dev[2];
    a.qflag = (const uint32_t *)d->dev[3];
    a.qscale = (const double *)d->dev[4];
    a.rh = (const uint64_t *)d->dev[5];
    a.roff = (const uint64_t *)d->dev[6];
    a.rmax = (const uint64_t *)d->dev[7];
    a.rflag = (const uint32_t *)d->dev[8];
    a.rscale = (const double *)d->dev[9];
    a.nq = d->nq;
    a.r0 = r0;
    a.r1 = r1;
    a.slice = d->slice;
    a.out = d->out_d[buf];
    return a;
}

int dist_launch(DistDevice *d, int buf, uint32_t r0, uint32_t r1) {
    if (r1 < r0 || (uint64_t)(r1 - r0) * d->nq > d->max_pairs || (r1 - r0 + RB - 1) / RB > 65535u)
        return api_fail(FH_ERR_INVALID, "dist_launch: %u references do not fit the result buffer", r1 - r0);
    if (d->search) return api_fail(FH_ERR_STATE, "dist_launch on a search handle");
    DHIP_TRY(hipSetDevice(d->device));
    const DistArgs a = dist_args(d, buf, r0, r1);
    const uint64_t pairs = (uint64_t)(r1 - r0) * d->nq;
    d->launched_pairs[buf] = (uint32_t)pairs;
    DHIP_TRY(hipEventRecord(d->ev0[buf], d->stream));
    if (pairs) {
        const dim3 grid(d->nq, (r1 - r0 + RB - 1) / RB);
        hipLaunchKernelGGL(k_dist_counts<false>, grid, dim3(THREADS), d->lds_slice * sizeof(uint64_t), d->stream, a);
        DHIP_TRY(hipGetLastError());
    }
    DHIP_TRY(hipEventRecord(d->ev1[buf], d->stream));
    if (pairs) DHIP_TRY(hipMemcpyAsync(d->out_h[buf], d->out_d[buf], pairs * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
    DHIP_TRY(hipEventRecord(d->done[buf], d->stream));
    return FH_OK;
}

int dist_wait(DistDevice *d, int buf, const uint32_t **out, double *kernel_ms) {
    DHIP_TRY(hipSetDevice(d->device));
    DHIP_TRY(hipEventSynchronize(d->done[buf]));
    float ms = 0.f;
    DHIP_TRY(hipEventElapsedTime(&ms, d->ev0[buf], d->ev1[buf]));
    *out = d->out_h[buf];
    if (kernel_ms) *kernel_ms = ms;
    return FH_OK;
}

int dist_counts_query_major(const DistDeviceArrays &v, uint32_t r0, uint32_t r1, uint32_t *out, void *stream) {
    if (r1 <= r0 || v.nq == 0 || v.slice == 0 || v.slice > DIST_MAX_SLICE || (r1 - r0 + RB - 1) / RB > 65535u)
        return api_fail(FH_ERR_INVALID, "dist_counts_query_major: %u references, slice %u", r1 - r0, v.slice);
    DistArgs a;
    a.qh = v.qh, a.qoff = v.qoff, a.rh = v.rh, a.roff = v.roff;
    a.qmax = a.rmax = nullptr; // (read only where a flag's bit 1 is set)
    a.qscale = a.rscale = nullptr;
    a.qflag = v.qflag, a.rflag = v.rflag;
    a.nq = v.nq, a.r0 = r0, a.r1 = r1, a.slice = v.slice;
    a.out = out;
    hipLaunchKernelGGL(k_dist_counts<true>, dim3(v.nq, (r1 - r0 + RB - 1) / RB), dim3(THREADS), v.slice * sizeof(uint64_t), (hipStream_t)stream, a);
    DHIP_TRY(hipGetLastError());
    return FH_OK;
}

int search_launch(DistDevice *d, int buf, uint32_t r0, uint32_t r1) {
    if (!d->search) return api_fail(FH_ERR_STATE, "search_launch on a handle of dist_open");
    if (r1 <= r0 || d->nq == 0 || (uint64_t)(r1 - r0) * d->nq > d->max_pairs || (r1 - r0 + RB - 1) / RB > 65535u)
        return api_fail(FH_ERR_INVALID, "search_launch: %u references do not fit the result buffer", r1 - r0);
    DHIP_TRY(hipSetDevice(d->device));
    const DistArgs a = dist_args(d, buf, r0, r1);
    SearchArgs sa;
    sa.cnt = d->out_d[buf];
    sa.n = r1 - r0;
    sa.r0 = r0;
    sa.top_n = d->top_n;
    sa.min_c = d->min_c;
    sa.sel = d->sel_d[buf];
    sa.count = d->count_d[buf];
    d->launched_pairs[buf] = (uint32_t)((uint64_t)(r1 - r0) * d->nq);
    DHIP_TRY(hipEventRecord(d->ev0[buf], d->stream));
    if (!d->top_mode) DHIP_TRY(hipMemsetAsync(d->count_d[buf], 0, sizeof(uint32_t), d->stream));
    hipLaunchKernelGGL(k_dist_counts<true>, dim3(d->nq, (r1 - r0 + RB - 1) / RB), dim3(THREADS), d->lds_slice * sizeof(uint64_t), d->stream, a);
    DHIP_TRY(hipGetLastError());
    if (d->top_mode) hipLaunchKernelGGL(k_search_top, dim3(d->nq), dim3(THREADS), 0, d->stream, sa);
    else hipLaunchKernelGGL(k_search_all, dim3(d->nq), dim3(THREADS), 0, d->stream, sa);
    DHIP_TRY(hipGetLastError());
    DHIP_TRY(hipEventRecord(d->ev1[buf], d->stream));
    if (d->top_mode) {
        DHIP_TRY(hipMemcpyAsync(d->count_h[buf], d->count_d[buf], d->nq * sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
        DHIP_TRY(hipMemcpyAsync(d->sel_h[buf], d->sel_d[buf], (size_t)d->nq * d->top_n * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
    } else {
        DHIP_TRY(hipMemcpyAsync(d->count_h[buf], d->count_d[buf], sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
    }
    DHIP_TRY(hipEventRecord(d->done[buf], d->stream));
    return FH_OK;
}

int search_wait(DistDevice *d, int buf, const uint32_t **entries, const uint32_t **per_query, uint64_t *n, double *kernel_ms) {
    DHIP_TRY(hipSetDevice(d->device));
    DHIP_TRY(hipEventSynchronize(d->done[buf]));
    float ms = 0.f;
    DHIP_TRY(hipEventElapsedTime(&ms, d->ev0[buf], d->ev1[buf]));
    if (kernel_ms) *kernel_ms = ms;
    if (d->top_mode) {
        *entries = d->sel_h[buf];
        *per_query = d->count_h[buf];
        *n = (uint64_t)d->nq * d->top_n;
        return FH_OK;
    }
    const uint32_t cursor = d->count_h[buf][0];
    if (cursor > d->launched_pairs[buf]) return api_fail(FH_ERR_STATE, "search: %u entries from %u pairs", cursor, d->launched_pairs[buf]);
    std::vector<uint32_t> &list = d->list_h[buf];
    list.resize((size_t)cursor * 5);
    // (not on the handle's stream, where the next chunk's kernels may already wait: the entries are complete, `done` says so)
    if (cursor) DHIP_TRY(hipMemcpy(list.data(), d->sel_d[buf], list.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    *entries = list.data();
    *per_query = nullptr;
    *n = cursor;
    return FH_OK;
}

} // namespace fh
