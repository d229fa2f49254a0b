// fh_merge_lib.hip -- Sketch.merge (merge_sketches, lib/src/python.rs:24-100) folded over many groups of sketches on the
// device: group (m0, m1, ...) is a copy of m0 merged with m1, then with m2, ..., each merge clipped.  DESIGN.md §3.12.
//
// One workgroup per group runs the fold step by step, which is exact for every clip mode and every order of the members by
// construction.  The accumulator is a list of 24-byte records (hash, count, extra, whose k-mer text) in global memory; a step
// reads it from one of the group's two buffers and writes the next one into the other.  One step, an accumulator A of la
// records against a member B of lb:
//   * the reference's walk stops when either list runs out, so only the records <= bound = min(A[la - 1], B[lb - 1]) take
//     part: a' of A and b' of B, one of the two the whole list;
//   * the walk's a' + b' positions are cut into tiles and a tile into one chunk per thread along merge-path diagonals (ties put
//     A first); a thread finds its chunk's co-ranks by binary search and walks the chunk;
//   * both lists ascend strictly, so a shared hash is an adjacent (A, B) pair of the walk: B[j] is dropped iff the A record
//     before it in the walk equals it, A[i] takes B[j]'s counts iff B[j] is the next B record and equals it -- each test needs
//     the thread's own co-ranks only, also across chunk and tile ends;
//   * an exclusive scan of "emits a record" over the workgroup gives every record its rank in the step's output, the base
//     carries over the tiles;
//   * the clip is a predicate of (rank, hash) that, once false, stays false: each thread tests its own records, the step's
//     output ends at the first failing rank and the step's remaining tiles are skipped, the same decision in every thread.
// The u32 sums wrap (a release build of the reference); nothing saturates.  After the last step the workgroup takes its place in
// the launch's packed record list with one atomic add and copies its result there, so that the host fetches one list.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <vector>

#include "../../include/finch_hip.h"
#include "fh_internal.h"
#include "fh_merge_lib.h"

using namespace fh;

namespace {

#define CHIP_TRY(expr)                                                                                      \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess) return api_fail(FH_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

constexpr uint32_t THREADS = 256; // four waves
constexpr uint32_t WAVES = THREADS / 64;
constexpr uint32_t NONE = 0xffffffffu;

struct MergeLibArgs {
    const uint64_t *in_h, *in_off; // the input (MergeLibInput)
    const uint32_t *in_c, *in_e;
    const MergeLibGroup *groups;
    const uint32_t *members;
    MergeLibRecord *acc[2]; // the accumulators' two buffers
    MergeLibRecord *res;    // the launch's packed results
    MergeLibOut *outs;
    uint32_t *cursor;       // records in res (zero before the launch)
    uint32_t *status;       // set if a step's output did not fit its group's cap (the host's bound was wrong)
    uint64_t size, res_cap;
    uint32_t has_size, tile, items; // items = ceil(tile / THREADS): walk positions per thread
};

// #{s[0..n).hash <= x} over ascending records, the same steps in every thread of the workgroup
__device__ inline uint32_t count_le_rec(const MergeLibRecord *s, uint32_t n, uint64_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (s[mid].hash <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ inline uint32_t count_le(const uint64_t *s, uint32_t n, uint64_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (s[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the A records among the first d of the walk over A[0..ap) and B[0..bp), d <= ap + bp; on equal hashes A goes first
__device__ inline uint32_t co_rank(const MergeLibRecord *A, uint32_t ap, const uint64_t *B, uint32_t bp, uint32_t d) {
    uint32_t lo = d > bp ? d - bp : 0, hi = min(d, ap);
    while (lo < hi) { // the smallest i with B[d - i - 1] < A[i]; inside the loop i < ap and 1 <= d - i <= bp
        const uint32_t mid = lo + (hi - lo) / 2;
        if (A[mid].hash <= B[d - mid - 1]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// grid: x = group of the launch
__global__ void __launch_bounds__(THREADS) k_merge_groups(MergeLibArgs a) {
    __shared__ uint32_t s_wsum[WAVES], s_fail[WAVES], s_place;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const MergeLibGroup g = a.groups[blockIdx.x];
    const uint32_t *mem = a.members + g.mem_begin;
    MergeLibRecord *const buf0 = a.acc[0] + g.buf_off, *const buf1 = a.acc[1] + g.buf_off;

    // the accumulator starts as a copy of the first member (the host made cap >= its length)
    uint32_t la;
    {
        const uint64_t o = a.in_off[mem[0]];
        la = min((uint32_t)(a.in_off[mem[0] + 1] - o), g.cap);
        for (uint32_t i = tid; i < la; i += THREADS) buf0[i] = MergeLibRecord{a.in_h[o + i], a.in_c[o + i], a.in_e[o + i], 0u, i};
    }
    __syncthreads();

    for (uint32_t s = 1; s < g.n_members; ++s) {
        const uint64_t o = a.in_off[mem[s]];
        const uint32_t lb = (uint32_t)(a.in_off[mem[s] + 1] - o);
        const MergeLibRecord *A = s & 1 ? buf0 : buf1; // (selected, not indexed: no array of pointers in scratch)
        MergeLibRecord *D = s & 1 ? buf1 : buf0;
        if (la == 0 || lb == 0) { // the walk ends before it starts: empty now and for good
            la = 0;
            continue;
        }
        const uint64_t *Bh = a.in_h + o;
        const uint32_t *Bc = a.in_c + o, *Be = a.in_e + o;
        const uint64_t last_a = A[la - 1].hash, last_b = Bh[lb - 1];
        const uint32_t ap = last_a <= last_b ? la : count_le_rec(A, la, last_b);
        const uint32_t bp = last_a <= last_b ? count_le(Bh, lb, last_a) : lb;
        const uint32_t n = ap + bp; // (the host refuses a group of 2^32 records or more)
        uint32_t base = 0, new_len = NONE;
        for (uint64_t t0 = 0; t0 < n; t0 += a.tile) {
            const uint32_t tl = (uint32_t)min((uint64_t)a.tile, n - t0);
            const uint32_t d0 = (uint32_t)t0 + min(tid * a.items, tl), d1 = (uint32_t)t0 + min((tid + 1) * a.items, tl);
            const uint32_t i0 = co_rank(A, ap, Bh, bp, d0), j0 = d0 - i0;
            // first walk: how many records the chunk emits
            uint32_t emit = 0;
            {
                uint32_t i = i0, j = j0;
                for (uint32_t d = d0; d < d1; ++d) {
                    if (j >= bp || (i < ap && A[i].hash <= Bh[j])) {
                        ++emit, ++i;
                    } else {
                        emit += !(i > 0 && A[i - 1].hash == Bh[j]);
                        ++j;
                    }
                }
            }
            uint32_t incl = emit;
            for (uint32_t off = 1; off < 64; off <<= 1) {
                const uint32_t v = __shfl_up(incl, off, 64);
                if (lane >= off) incl += v;
            }
            if (lane == 63) s_wsum[wave] = incl;
            __syncthreads();
            uint32_t rank = base + incl - emit, total = 0;
            for (uint32_t w = 0; w < WAVES; ++w) {
                const uint32_t v = s_wsum[w];
                rank += w < wave ? v : 0;
                total += v;
            }
            // second walk: the records, each to its rank if the clip keeps it
            uint32_t fail = NONE;
            {
                uint32_t i = i0, j = j0;
                for (uint32_t d = d0; d < d1; ++d) {
                    MergeLibRecord r;
                    bool out = true;
                    if (j >= bp || (i < ap && A[i].hash <= Bh[j])) {
                        r = A[i];
                        if (j < bp && Bh[j] == r.hash) r.count += Bc[j], r.extra += Be[j]; // (u32: wraps)
                        ++i;
                    } else {
                        out = !(i > 0 && A[i - 1].hash == Bh[j]);
                        r = MergeLibRecord{Bh[j], Bc[j], Be[j], s, j};
                        ++j;
                    }
                    if (out) {
                        const bool keep = (!a.has_size && !g.has_scale) || (g.has_scale && r.hash <= g.max_hash) || (a.has_size && rank < a.size);
                        if (keep && rank < g.cap) D[rank] = r;
                        else if (keep) *a.status = 1;
                        else fail = min(fail, rank);
                        ++rank;
                    }
                }
            }
            for (int off = 32; off; off >>= 1) fail = min(fail, (uint32_t)__shfl_xor(fail, off, 64));
            if (lane == 0) s_fail[wave] = fail;
            __syncthreads(); // (also: this tile's records are written before the next step reads them)
            fail = min(min(s_fail[0], s_fail[1]), min(s_fail[2], s_fail[3]));
            base += total;
            if (fail != NONE) { // every thread reads the same four words: the workgroup leaves the step together
                new_len = fail;
                break;
            }
        }
        la = min(new_len != NONE ? new_len : base, g.cap);
    }

    // the result into the launch's list
    const MergeLibRecord *F = (g.n_members - 1) & 1 ? buf1 : buf0;
    if (tid == 0) {
        const uint32_t place = atomicAdd(a.cursor, la);
        a.outs[blockIdx.x] = MergeLibOut{la, place};
        s_place = place;
    }
    __syncthreads();
    const uint64_t place = s_place;
    for (uint32_t i = tid; i < la; i += THREADS)
        if (place + i < a.res_cap) a.res[place + i] = F[i];
}

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

} // namespace

namespace fh {

struct MergeLibDevice {
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t n_in = 0, max_groups = 0, tile = 0, has_size = 0;
    uint64_t max_members = 0, max_records = 0, size = 0;
    std::vector<uint64_t> in_len; // the input sketches' lengths (launch checks)
    void *in[4] = {};             // hashes counts extras offsets
    struct Set {
        MergeLibRecord *acc[2] = {}, *res = nullptr;
        MergeLibGroup *groups = nullptr;
        uint32_t *members = nullptr, *words = nullptr; // words: cursor, status
        MergeLibOut *outs = nullptr;
        uint32_t *words_h = nullptr; // pinned
        MergeLibOut *outs_h = nullptr;
        hipEvent_t ev0 = nullptr, ev1 = nullptr, done = nullptr;
        uint32_t n_groups = 0;
        uint64_t records = 0; // the launched groups' caps, summed
        std::vector<MergeLibGroup> groups_h;
        std::vector<uint32_t> members_h;
        std::vector<MergeLibRecord> res_h;
    } set[2];
};

static int upload(void **dst, const void *src, size_t bytes) {
    const size_t b = std::max<size_t>(bytes, 8); // (an empty input still gets a valid pointer)
    CHIP_TRY(api_dev_malloc(dst, b));
    if (bytes) CHIP_TRY(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
    return FH_OK;
}

void merge_lib_close(MergeLibDevice *d) {
    if (!d) return;
    if (hipSetDevice(d->device) == hipSuccess) {
        if (d->stream) (void)hipStreamSynchronize(d->stream);
        for (void *p : d->in)
            if (p) (void)hipFree(p);
        for (MergeLibDevice::Set &s : d->set) {
            for (void *p : {(void *)s.acc[0], (void *)s.acc[1], (void *)s.res, (void *)s.groups, (void *)s.members, (void *)s.words, (void *)s.outs})
                if (p) (void)hipFree(p);
            if (s.words_h) (void)hipHostFree(s.words_h);
            if (s.outs_h) (void)hipHostFree(s.outs_h);
            if (s.ev0) (void)hipEventDestroy(s.ev0);
            if (s.ev1) (void)hipEventDestroy(s.ev1);
            if (s.done) (void)hipEventDestroy(s.done);
        }
        if (d->stream) (void)hipStreamDestroy(d->stream);
    }
    (void)hipGetLastError();
    delete d;
}

static int open_into(MergeLibDevice *d, const MergeLibInput &in, double *upload_ms) {
    CHIP_TRY(hipSetDevice(d->device));
    CHIP_TRY(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
    const double t0 = now_ms();
    const uint64_t total = in.offsets[in.n];
    if (int rc = upload(&d->in[0], in.hashes, total * sizeof(uint64_t))) return rc;
    if (int rc = upload(&d->in[1], in.counts, total * sizeof(uint32_t))) return rc;
    if (int rc = upload(&d->in[2], in.extras, total * sizeof(uint32_t))) return rc;
    if (int rc = upload(&d->in[3], in.offsets, ((size_t)in.n + 1) * sizeof(uint64_t))) return rc;
    if (upload_ms) *upload_ms = now_ms() - t0;
    for (MergeLibDevice::Set &s : d->set) {
        for (MergeLibRecord **p : {&s.acc[0], &s.acc[1], &s.res}) CHIP_TRY(api_dev_malloc((void **)p, d->max_records * sizeof(MergeLibRecord)));
        CHIP_TRY(api_dev_malloc((void **)&s.groups, (size_t)d->max_groups * sizeof(MergeLibGroup)));
        CHIP_TRY(api_dev_malloc((void **)&s.members, d->max_members * sizeof(uint32_t)));
        CHIP_TRY(api_dev_malloc((void **)&s.words, 16));
        CHIP_TRY(api_dev_malloc((void **)&s.outs, (size_t)d->max_groups * sizeof(MergeLibOut)));
        CHIP_TRY(api_host_malloc((void **)&s.words_h, 16));
        CHIP_TRY(api_host_malloc((void **)&s.outs_h, (size_t)d->max_groups * sizeof(MergeLibOut)));
        CHIP_TRY(hipEventCreate(&s.ev0));
        CHIP_TRY(hipEventCreate(&s.ev1));
        CHIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    }
    return FH_OK;
}

int merge_lib_open(int device, const MergeLibInput &in, uint32_t max_groups, uint64_t max_members, uint64_t max_records, uint32_t tile,
                   const uint64_t *size, MergeLibDevice **out, double *upload_ms) {
    // (a launch's cursor and a group's ranks are u32)
    if (!out || !in.n || !max_groups || max_groups > (1u << 30) || max_members < 2 || !max_records || max_records > UINT32_MAX)
        return api_fail(FH_ERR_INVALID, "merge_lib_open: %u sketches, launches of %u groups, %llu members, %llu records", in.n, max_groups,
                        (unsigned long long)max_members, (unsigned long long)max_records);
    if (!in.offsets || in.offsets[0] != 0) return api_fail(FH_ERR_INVALID, "merge_lib_open: the offsets do not start at 0");
    MergeLibDevice *d = new (std::nothrow) MergeLibDevice;
    if (!d) return api_fail(FH_ERR_CAPACITY, "out of host memory");
    d->in_len.resize(in.n);
    for (uint32_t s = 0; s < in.n; ++s) {
        if (in.offsets[s + 1] < in.offsets[s] || in.offsets[s + 1] - in.offsets[s] >= UINT32_MAX) {
            delete d;
            return api_fail(FH_ERR_INVALID, "merge_lib_open: offsets of sketch %u", s);
        }
        d->in_len[s] = in.offsets[s + 1] - in.offsets[s];
    }
    if (in.offsets[in.n] && (!in.hashes || !in.counts || !in.extras)) {
        delete d;
        return api_fail(FH_ERR_INVALID, "merge_lib_open: the input has no entries");
    }
    d->device = device;
    d->n_in = in.n;
    d->max_groups = max_groups;
    d->max_members = max_members;
    d->max_records = max_records;
    d->tile = std::min(std::max(tile, 1u), MERGE_LIB_MAX_TILE);
    d->has_size = size ? 1 : 0;
    d->size = size ? *size : 0;
    if (int rc = open_into(d, in, upload_ms)) {
        merge_lib_close(d);
        return rc;
    }
    *out = d;
    return FH_OK;
}

int merge_lib_launch(MergeLibDevice *d, int buf, const MergeLibGroup *groups, uint32_t n_groups, const uint32_t *members, uint64_t n_members) {
    if (!d || (buf != 0 && buf != 1) || !groups || !members) return api_fail(FH_ERR_INVALID, "merge_lib_launch: handle, buffer or lists");
    if (!n_groups || n_groups > d->max_groups || n_members > d->max_members)
        return api_fail(FH_ERR_INVALID, "merge_lib_launch: %u groups, %llu members do not fit the handle", n_groups, (unsigned long long)n_members);
    // everything the kernel indexes with: the members inside the input, the groups' buffers inside the set's and apart
    uint64_t at = 0;
    for (uint32_t g = 0; g < n_groups; ++g) {
        const MergeLibGroup &x = groups[g];
        if (x.n_members < 2 || x.mem_begin > n_members || x.n_members > n_members - x.mem_begin)
            return api_fail(FH_ERR_INVALID, "merge_lib_launch: members of group %u", g);
        for (uint32_t m = 0; m < x.n_members; ++m)
            if (members[x.mem_begin + m] >= d->n_in) return api_fail(FH_ERR_INVALID, "merge_lib_launch: group %u member %u is not in the input", g, m);
        if (x.buf_off != at || x.cap > d->max_records - at || x.cap < d->in_len[members[x.mem_begin]])
            return api_fail(FH_ERR_INVALID, "merge_lib_launch: buffer of group %u", g);
        at += x.cap;
    }
    CHIP_TRY(hipSetDevice(d->device));
    MergeLibDevice::Set &s = d->set[buf];
    s.groups_h.assign(groups, groups + n_groups); // (the copies read these until the launch is waited for)
    s.members_h.assign(members, members + n_members);
    s.n_groups = n_groups;
    s.records = at;
    MergeLibArgs a;
    a.in_h = (const uint64_t *)d->in[0];
    a.in_c = (const uint32_t *)d->in[1];
    a.in_e = (const uint32_t *)d->in[2];
    a.in_off = (const uint64_t *)d->in[3];
    a.groups = s.groups;
    a.members = s.members;
    a.acc[0] = s.acc[0];
    a.acc[1] = s.acc[1];
    a.res = s.res;
    a.outs = s.outs;
    a.cursor = s.words;
    a.status = s.words + 1;
    a.size = d->size;
    a.res_cap = d->max_records;
    a.has_size = d->has_size;
    a.tile = d->tile;
    a.items = (d->tile + THREADS - 1) / THREADS;
    CHIP_TRY(hipMemcpyAsync(s.groups, s.groups_h.data(), (size_t)n_groups * sizeof(MergeLibGroup), hipMemcpyHostToDevice, d->stream));
    CHIP_TRY(hipMemcpyAsync(s.members, s.members_h.data(), n_members * sizeof(uint32_t), hipMemcpyHostToDevice, d->stream));
    CHIP_TRY(hipMemsetAsync(s.words, 0, 16, d->stream));
    CHIP_TRY(hipEventRecord(s.ev0, d->stream));
    hipLaunchKernelGGL(k_merge_groups, dim3(n_groups), dim3(THREADS), 0, d->stream, a);
    CHIP_TRY(hipGetLastError());
    CHIP_TRY(hipEventRecord(s.ev1, d->stream));
    CHIP_TRY(hipMemcpyAsync(s.words_h, s.words, 16, hipMemcpyDeviceToHost, d->stream));
    CHIP_TRY(hipMemcpyAsync(s.outs_h, s.outs, (size_t)n_groups * sizeof(MergeLibOut), hipMemcpyDeviceToHost, d->stream));
    CHIP_TRY(hipEventRecord(s.done, d->stream));
    return FH_OK;
}

int merge_lib_wait(MergeLibDevice *d, int buf, const MergeLibOut **outs, const MergeLibRecord **records, uint64_t *n_records,
                   double *kernel_ms, double *copy_ms) {
    if (!d || (buf != 0 && buf != 1) || !outs || !records || !n_records) return api_fail(FH_ERR_INVALID, "merge_lib_wait: handle, buffer or outputs");
    CHIP_TRY(hipSetDevice(d->device));
    MergeLibDevice::Set &s = d->set[buf];
    CHIP_TRY(hipEventSynchronize(s.done));
    float ms = 0.f;
    CHIP_TRY(hipEventElapsedTime(&ms, s.ev0, s.ev1));
    if (kernel_ms) *kernel_ms = ms;
    const uint32_t cursor = s.words_h[0];
    if (s.words_h[1]) return api_fail(FH_ERR_STATE, "merge: a step's output did not fit its group's buffer");
    if (cursor > s.records) return api_fail(FH_ERR_STATE, "merge: %u records from groups of %llu at most", cursor, (unsigned long long)s.records);
    uint64_t sum = 0;
    for (uint32_t g = 0; g < s.n_groups; ++g) {
        const MergeLibOut &o = s.outs_h[g];
        if (o.len > s.groups_h[g].cap || o.place > cursor || o.len > cursor - o.place)
            return api_fail(FH_ERR_STATE, "merge: group %u's result (%u records at %u of %u)", g, o.len, o.place, cursor);
        sum += o.len;
    }
    if (sum != cursor) return api_fail(FH_ERR_STATE, "merge: %llu records in the groups' results, %u in the list", (unsigned long long)sum, cursor);
    const double t0 = now_ms();
    s.res_h.resize(cursor);
    // (not on the handle's stream, where the next launch may already wait: the records are complete, `done` says so)
    if (cursor) CHIP_TRY(hipMemcpy(s.res_h.data(), s.res, (size_t)cursor * sizeof(MergeLibRecord), hipMemcpyDeviceToHost));
    if (copy_ms) *copy_ms = now_ms() - t0;
    *outs = s.outs_h;
    *records = s.res_h.data();
    *n_records = cursor;
    return FH_OK;
}

} // namespace fh
