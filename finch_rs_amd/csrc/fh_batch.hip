// fh_batch.hip -- host side of the batch sketcher (include/finch_hip.h, "many sketches per launch"): the files a worker of
// finch::sketch_files (lib/src/lib.rs:29-49) has staged are sketched by ONE launch of k2_batch (fh_k2b.hip) and finished by
// ONE launch of k_batch_epilogue (fh_kernels.hip, a workgroup per file), behind ONE host-to-device copy and in front of ONE
// synchronisation -- where a file through an fh_sketcher costs a copy, three launches and a synchronisation of its own.
//
// What is resident per batch handle: max_files partitions (control block, table partition of PART_CAP entries, live / dead
// lists, 256 shard lists), and per slot (two: the caller fills one while the device works on the other) a pinned staging
// buffer, its device twin, the pinned result columns and mirrored control blocks of max_files sketches.  The staging
// buffer begins with the batch's file descriptors (BatchFile, fh_device.h), so descriptors and sequence cross the link
// in one copy.
//
// Exactness: a file is sketched at ONE threshold below which E = 4 n (3 n for n > 2000) of its positions' hashes are
// expected; the epilogue keeps the n smallest of what was admitted.  That IS the reference's sketch (mash.rs:34-63: the
// bottom n distinct hashes with their exact occurrence counts) whenever at least n distinct hashes lie at or below the
// threshold -- or the threshold admitted everything -- and nothing overflowed and no two k-mers shared a 64-bit hash; in
// every other case the file is reported as not taken (status 1) and the caller sketches it through an fh_sketcher.  There
// is no other outcome: the batch path never returns an approximate sketch.
//
// Scaled sketches (FH_KIND_SCALED): the threshold is no guess but max_hash (scaled.rs:22-34), known before the file is read.
// Reading scaled.rs:37-61: a hash <= max_hash is always admitted and never evicted (the pop fires only when the heap's top is
// above max_hash); a hash above it is admitted only while len <= size, and popped after any push that leaves len > size with
// such a hash on top.  So with D = the file's distinct hashes <= max_hash: if D >= size (or size == 0) the sketch is exactly
// those D hashes, ascending, with their exact counts -- a function of the multiset of k-mers -- and the file is taken iff
// additionally D <= FH_BATCH_SCALED_MAX, nothing overflowed and no two k-mers shared a hash.  If D < size the reference's
// sketch also holds hashes above max_hash whose counts depend on the order of the input: not taken.
//
// AllCounts (fh_batch_new_counts, k = 1..7): a handle of its own kind behind the same functions.  No partitions: a table of
// 4^k u32 per file, counted by ONE launch of k_ac_batch_count and turned into to_vec's rows by ONE launch of
// k_ac_batch_epilogue (fh_counts.hip, a workgroup per file), which leaves the tables zeroed.  A count is exact for any input:
// every file is taken.
//
// k = 33..64 (fh_batch_new_wide): the same handle with the two-word sketch kernel (k2_batch_w, fh_k2bw.hip) in k2_batch's
// place.  Every partition owns the high k-mer words of its table (PART_CAP u64, Ctl::kmer_hi), the epilogue writes them as a
// column of their own (EpiArgs::wide: 40 bytes per row) and the copy-outs decode a row's k bases from both words.  The rule
// for "taken" is unchanged; what is new is that the collision log also receives occurrences that are no collision
// (wide_kmer_update, fh_k2_common.h: the 64-mers with a word of all ones, the value that doubles as "not written"), and any
// record sends the file the long way, where fh_finish resolves it.  A k-mer that repeats inside one drain leaves none.
//
// Mash sizes 3001..FH_BATCH_LARGE_MAX_N, k = 1..32 (fh_batch_new_large): the same handle and the same k2_batch -- which takes a
// partition's geometry from its control block at run time -- over LARGER partitions, sized for the handle's n (geometry,
// fh_batch_plan.h), and k_batch_epilogue_large (fh_batch_large.hip) in k_batch_epilogue's place: a file's ~4 n live entries no longer fit
// a workgroup's LDS, so its select runs over a key scratch in device memory, one per file.  The rule for "taken" is unchanged.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/finch_hip.h"
#include "fh_batch_plan.h"
#include "fh_core.h"
#include "fh_counts.h"
#include "fh_device.h"
#include "fh_internal.h"
#include "fh_kernels.h"
#include "fh_options.h"
#include "fh_pack2.h"

using namespace fh;

namespace {

#define BHIP_TRY(expr)                                                                                      \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess) return api_fail(FH_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

namespace bp = fh::bplan;
using bp::Form;

// what fh_batch_plan.h mirrors of the device's headers
static_assert(bp::EMPTY == EMPTY64 && bp::FIN_OK == FIN_OK_RESET && bp::SMALL_ROWS == (uint64_t)SMALL_MAX && bp::LARGE_ROWS == (uint64_t)LARGE_MAX_ROWS &&
                  bp::COUNTS_MAX_K == (uint32_t)AC_LDS_MAX_K && bp::MAX_K == (uint32_t)FH_MAX_K && bp::SHARDS == (uint64_t)N_SHARDS &&
                  bp::SHARD_CURSOR_STRIDE == (uint64_t)SHARD_STRIDE && bp::TWO_BIT_TILE == fh_pack2::TILE_BYTES,
              "fh_batch_plan.h restates a constant of fh_device.h, fh_kernels.h or fh_pack2.h");
static_assert(bp::ENTRY_BYTES == sizeof(Entry) && bp::CTL_BYTES == sizeof(Ctl) && bp::COLL_BYTES == sizeof(CollRec) && bp::FILE_BYTES == sizeof(BatchFile),
              "fh_batch_plan.h restates the size of a structure of fh_device.h");
constexpr uint32_t PART_CLOG = bp::PART_CLOG;
constexpr uint64_t BATCH_MAX_WAVES = 4096; // 16 per CU x 256 CUs

} // namespace

// (its sizes -- cap, live_cap, shard_cap, out_stride, out_words, header_bytes, data_bytes, dev_bytes -- are the plan's Geometry)
struct fh_batch : bp::Geometry {
    fh_batch(Form f, const fh_params &params, int dev, uint32_t files, uint64_t stage_bytes)
        : bp::Geometry(bp::geometry(f, params, files, stage_bytes)), form(f), p(params), counts(f == Form::Counts), large(f == Form::Large),
          max_hash(params.kind == FH_KIND_SCALED ? api_scaled_max_hash(params.scale) : 0), device(dev), max_files(files) {}
    bp::PoolKey key() const { return bp::PoolKey{form, device, max_files, data_bytes, p}; }
    const Form form;       // the door it was made through
    const fh_params p;     // (counts: p.kind == FH_KIND_ALL_COUNTS, p.k = 1..7, the rest unused)
    const bool counts, large;
    const uint64_t max_hash; // FH_KIND_SCALED: the threshold of every file (EMPTY64 at scale 1: everything is admitted)
    const int device;
    hipStream_t stream = nullptr;
    const uint32_t max_files;
    // partitions
    Ctl *ctls = nullptr;
    Entry *tables = nullptr;
    uint32_t *live = nullptr, *dead = nullptr, *shard_cnt = nullptr, *shard_buf = nullptr;
    CollRec *clog = nullptr;
    uint64_t *kmer_hi = nullptr; // k > 32: max_files x PART_CAP high k-mer words (EMPTY64 = not written)
    uint64_t *keys = nullptr;    // large: max_files x live_cap words of key scratch
    BatchPartition *d_parts = nullptr;
    uint32_t *ac_tables = nullptr; // counts: max_files tables of 4^k forward counts, zero between batches
    struct Slot {
        uint8_t *h_stage = nullptr, *d_stage = nullptr;
        EpiArgs *d_epi = nullptr;
        EpiLargeArgs *d_epi_large = nullptr; // large: in d_epi's place
        Ctl *h_ctl = nullptr;
        AcBatchResult *h_res = nullptr; // counts: rows and total_kmers per file, in place of h_ctl
        uint64_t *h_out = nullptr;      // counts: three u32 columns per file (ix | count | extra_count)
        hipEvent_t done = nullptr, k0 = nullptr, k1 = nullptr;
        bool in_flight = false, waited = false;
        uint32_t n_files = 0;
        std::vector<uint64_t> tau, len;
        std::vector<uint8_t> status;
        uint64_t positions = 0;
    } slot[2];
    bool profiling = false;
    double prof_ms = 0.0;
    uint64_t prof_launches = 0, prof_positions = 0;
    uint64_t n_taken = 0, n_not_taken = 0;
};

namespace {

void destroy(fh_batch *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    for (auto &s : b->slot) {
        if (s.h_stage) (void)hipHostFree(s.h_stage);
        if (s.d_stage) (void)hipFree(s.d_stage);
        if (s.d_epi) (void)hipFree(s.d_epi);
        if (s.d_epi_large) (void)hipFree(s.d_epi_large);
        if (s.h_ctl) (void)hipHostFree(s.h_ctl);
        if (s.h_res) (void)hipHostFree(s.h_res);
        if (s.h_out) (void)hipHostFree(s.h_out);
        if (s.done) (void)hipEventDestroy(s.done);
        if (s.k0) (void)hipEventDestroy(s.k0);
        if (s.k1) (void)hipEventDestroy(s.k1);
    }
    if (b->ctls) (void)hipFree(b->ctls);
    if (b->tables) (void)hipFree(b->tables);
    if (b->live) (void)hipFree(b->live);
    if (b->dead) (void)hipFree(b->dead);
    if (b->shard_cnt) (void)hipFree(b->shard_cnt);
    if (b->shard_buf) (void)hipFree(b->shard_buf);
    if (b->clog) (void)hipFree(b->clog);
    if (b->kmer_hi) (void)hipFree(b->kmer_hi);
    if (b->keys) (void)hipFree(b->keys);
    if (b->d_parts) (void)hipFree(b->d_parts);
    if (b->ac_tables) (void)hipFree(b->ac_tables);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
}

// what a handle of any door holds, every size from the plan (the handle's Geometry base): the partitions (or a count's tables),
// and per slot the staging buffers, the result columns and the epilogue's arguments
int build(fh_batch *b) {
    const uint32_t F = b->max_files;
    const bool wide = b->form == Form::Wide, scaled = b->p.kind == FH_KIND_SCALED;
    const uint32_t PCAP = b->cap, PLIVE = b->live_cap, PSHARD = b->shard_cap;
    BHIP_TRY(hipSetDevice(b->device));
    BHIP_TRY(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    std::vector<BatchPartition> parts(b->counts ? 0 : F);
    if (b->counts) {
        const size_t bytes = (size_t)F * (size_t)ac_bins((int)b->p.k) * sizeof(uint32_t);
        BHIP_TRY(api_dev_malloc((void **)&b->ac_tables, bytes));
        BHIP_TRY(hipMemsetAsync(b->ac_tables, 0, bytes, b->stream));
    } else {
        if (wide) BHIP_TRY(api_dev_malloc((void **)&b->kmer_hi, (size_t)F * PCAP * sizeof(uint64_t)));
        if (b->large) BHIP_TRY(api_dev_malloc((void **)&b->keys, (size_t)F * PLIVE * sizeof(uint64_t)));
        BHIP_TRY(api_dev_malloc((void **)&b->ctls, (size_t)F * sizeof(Ctl)));
        BHIP_TRY(api_dev_malloc((void **)&b->tables, (size_t)F * PCAP * sizeof(Entry)));
        BHIP_TRY(api_dev_malloc((void **)&b->live, (size_t)F * PLIVE * sizeof(uint32_t)));
        BHIP_TRY(api_dev_malloc((void **)&b->dead, (size_t)F * PLIVE * sizeof(uint32_t)));
        BHIP_TRY(api_dev_malloc((void **)&b->shard_cnt, (size_t)F * N_SHARDS * SHARD_STRIDE * sizeof(uint32_t)));
        BHIP_TRY(api_dev_malloc((void **)&b->shard_buf, (size_t)F * N_SHARDS * PSHARD * sizeof(uint32_t)));
        BHIP_TRY(api_dev_malloc((void **)&b->clog, (size_t)F * PART_CLOG * sizeof(CollRec)));
        BHIP_TRY(api_dev_malloc((void **)&b->d_parts, (size_t)F * sizeof(BatchPartition)));
        for (uint32_t f = 0; f < F; ++f) {
            BatchPartition &q = parts[f];
            q.ctl = b->ctls + f;
            q.table = b->tables + (size_t)f * PCAP;
            q.live = b->live + (size_t)f * PLIVE;
            q.shard_cnt = b->shard_cnt + (size_t)f * N_SHARDS * SHARD_STRIDE;
            q.shard_buf = b->shard_buf + (size_t)f * N_SHARDS * PSHARD;
            q.clog = b->clog + (size_t)f * PART_CLOG;
            q.cap = PCAP;
            q.live_cap = PLIVE;
            q.clog_cap = PART_CLOG;
            q.shard_cap = PSHARD;
            q.kmer_hi = wide ? b->kmer_hi + (size_t)f * PCAP : nullptr;
        }
        BHIP_TRY(hipMemcpyAsync(b->d_parts, parts.data(), (size_t)F * sizeof(BatchPartition), hipMemcpyHostToDevice, b->stream));
        BHIP_TRY(launch_batch_init(b->d_parts, F, b->p.size, scaled ? b->max_hash : EMPTY64, scaled ? b->max_hash : 0ull, 1u, b->stream));
    }
    // what the two epilogues' arguments share: file f's partition and where its result goes
    auto epi_common = [&](auto &e, const fh_batch::Slot &s, uint32_t f) {
        e.table = parts[f].table;
        e.live = parts[f].live;
        e.dead = b->dead + (size_t)f * PLIVE;
        e.dead_cap = PLIVE;
        e.ctl = parts[f].ctl;
        e.size = b->p.size;
        e.out = s.h_out + (size_t)f * b->out_words;
        e.out_stride = b->out_stride;
        e.h_ctl = s.h_ctl + f;
    };
    std::vector<EpiArgs> epi(b->counts || b->large ? 0 : F);
    std::vector<EpiLargeArgs> epi_large(b->large ? F : 0);
    for (auto &s : b->slot) {
        BHIP_TRY(api_host_malloc((void **)&s.h_stage, b->header_bytes + b->data_bytes + 64));
        BHIP_TRY(api_dev_malloc((void **)&s.d_stage, b->header_bytes + b->data_bytes + 64));
        BHIP_TRY(api_host_malloc((void **)&s.h_out, (size_t)F * b->out_words * sizeof(uint64_t)));
        BHIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
        BHIP_TRY(hipEventCreate(&s.k0));
        BHIP_TRY(hipEventCreate(&s.k1));
        s.len.resize(F);
        s.status.resize(F);
        if (b->counts) {
            BHIP_TRY(api_host_malloc((void **)&s.h_res, (size_t)F * sizeof(AcBatchResult)));
            continue;
        }
        s.tau.resize(F);
        BHIP_TRY(api_host_malloc((void **)&s.h_ctl, (size_t)F * sizeof(Ctl)));
        for (EpiLargeArgs &e : epi_large) {
            const uint32_t f = (uint32_t)(&e - epi_large.data());
            e = EpiLargeArgs{};
            epi_common(e, s, f);
            e.shard_cnt = parts[f].shard_cnt;
            e.shard_buf = parts[f].shard_buf;
            e.keys = b->keys + (size_t)f * PLIVE;
            e.cap = PCAP;
            e.live_cap = PLIVE;
            e.shard_cap = PSHARD;
        }
        for (EpiArgs &e : epi) {
            e = EpiArgs{};
            epi_common(e, s, (uint32_t)(&e - epi.data()));
            e.kind = b->p.kind;
            e.max_hash = b->max_hash;
            e.flags = EPI_FLATTEN | EPI_PRUNE_FORCE | EPI_SORT | EPI_GATHER | EPI_RESET | (scaled ? EPI_KEEP_ALL : 0u);
            e.tau0 = scaled ? b->max_hash : EMPTY64;
            e.wide = wide ? 1u : 0u;
        }
        if (b->large) {
            BHIP_TRY(api_dev_malloc((void **)&s.d_epi_large, (size_t)F * sizeof(EpiLargeArgs)));
            BHIP_TRY(hipMemcpyAsync(s.d_epi_large, epi_large.data(), (size_t)F * sizeof(EpiLargeArgs), hipMemcpyHostToDevice, b->stream));
        } else {
            BHIP_TRY(api_dev_malloc((void **)&s.d_epi, (size_t)F * sizeof(EpiArgs)));
            BHIP_TRY(hipMemcpyAsync(s.d_epi, epi.data(), (size_t)F * sizeof(EpiArgs), hipMemcpyHostToDevice, b->stream));
        }
        BHIP_TRY(hipStreamSynchronize(b->stream)); // (the next slot refills epi / epi_large; parts is a local)
    }
    BHIP_TRY(hipStreamSynchronize(b->stream));
    return FH_OK;
}


std::mutex g_pool_mu;
std::vector<fh_batch *> g_pool;
constexpr size_t BATCH_POOL_MAX = 64;

} // namespace

namespace fh {
void batch_release_cached() {
    std::vector<fh_batch *> v;
    {
        std::lock_guard<std::mutex> g(g_pool_mu);
        v.swap(g_pool);
    }
    for (fh_batch *b : v) destroy(b);
}
} // namespace fh

static bool device_ok(int device) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
        (void)hipGetLastError();
        api_fail(FH_ERR_NO_DEVICE, "no usable HIP device (this library has no CPU path)");
        return false;
    }
    if (device < 0 || device >= n_dev) {
        api_fail(FH_ERR_NO_DEVICE, "device %d out of range (%d visible)", device, n_dev);
        return false;
    }
    return true;
}

// what the four doors share: the door's parameter check (fh_batch_plan.h), the device, a parked handle the plan's predicate
// lets out through this door, or a new one
static fh_batch *batch_new(Form form, const fh_params *params, int device, uint32_t max_files, uint64_t stage_bytes) {
    if (!params) {
        api_fail(FH_ERR_INVALID, "null params");
        return nullptr;
    }
    const bp::Verdict v = bp::check(form, params, max_files, stage_bytes);
    if (v.code != FH_OK) {
        api_fail(v.code, "%s", v.msg);
        return nullptr;
    }
    if (!device_ok(device)) return nullptr;
    {
        const bp::PoolKey want{form, device, max_files, bp::stage_rounded(stage_bytes), *params};
        std::lock_guard<std::mutex> g(g_pool_mu);
        for (size_t i = 0; i < g_pool.size(); ++i) {
            fh_batch *c = g_pool[i];
            if (bp::pool_match(c->key(), want)) {
                g_pool.erase(g_pool.begin() + (long)i);
                return c;
            }
        }
    }
    fh_batch *b = nullptr;
    try {
        b = new fh_batch(form, *params, device, max_files, stage_bytes);
        if (build(b) == FH_OK) return b;
    } catch (...) {
        api_fail(FH_ERR_CAPACITY, "out of host memory");
    }
    destroy(b);
    return nullptr;
}

extern "C" {

fh_batch *fh_batch_new(const fh_params *params, int device, uint32_t max_files, uint64_t stage_bytes) {
    return batch_new(Form::Small, params, device, max_files, stage_bytes);
}

fh_batch *fh_batch_new_large(const fh_params *params, int device, uint32_t max_files, uint64_t stage_bytes) {
    return batch_new(Form::Large, params, device, max_files, stage_bytes);
}

fh_batch *fh_batch_new_wide(const fh_params *params, int device, uint32_t max_files, uint64_t stage_bytes) {
    return batch_new(Form::Wide, params, device, max_files, stage_bytes);
}

fh_batch *fh_batch_new_counts(uint32_t k, int device, uint32_t max_files, uint64_t stage_bytes) {
    fh_params p{};
    p.kind = FH_KIND_ALL_COUNTS;
    p.k = k;
    return batch_new(Form::Counts, &p, device, max_files, stage_bytes);
}


// A batch handle owns ~130 MiB of pinned and ~200 MiB of device memory, and pinning alone takes tens of milliseconds:
// like fh_free, fh_batch_free parks an idle handle (state clean: every partition is left reset by its epilogue) and
// fh_batch_new hands a parked one back when parameters, device and sizes match.  fh_release_cached frees what is parked.
void fh_batch_free(fh_batch *b) {
    if (!b) return;
    bool idle = !b->slot[0].in_flight && !b->slot[1].in_flight;
    // a large handle is parked only within the options `pool` (handles; 0 = none) and `pool_bytes` (device memory, the default
    // of the sketchers' pool: the smaller of 24 GiB and a tenth of the device), counted over the parked large handles
    uint64_t large_max = 0, large_max_bytes = 0;
    if (idle && b->large) {
        large_max = cfg_u64("pool", 64);
        if (cfg("pool_bytes")) {
            large_max_bytes = cfg_u64("pool_bytes", 0);
        } else {
            size_t free_b = 0, total_b = 0;
            large_max_bytes = 24ull << 30;
            if (hipSetDevice(b->device) == hipSuccess && hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b)
                large_max_bytes = std::min<uint64_t>(large_max_bytes, (uint64_t)total_b / 10);
            else (void)hipGetLastError();
        }
    }
    if (idle) {
        std::lock_guard<std::mutex> g(g_pool_mu);
        bool room = g_pool.size() < BATCH_POOL_MAX;
        if (b->large) {
            uint64_t n_large = 0, bytes = b->dev_bytes;
            for (const fh_batch *c : g_pool)
                if (c->large) n_large++, bytes += c->dev_bytes;
            room = room && n_large < large_max && bytes <= large_max_bytes;
        }
        if (room) {
            b->profiling = false;
            b->prof_ms = 0.0;
            b->prof_launches = b->prof_positions = 0;
            b->n_taken = b->n_not_taken = 0;
            b->slot[0].waited = b->slot[1].waited = false;
            g_pool.push_back(b);
            return;
        }
    }
    destroy(b);
}

int fh_batch_parked(uint64_t *handles, uint64_t *large_handles, uint64_t *large_device_bytes) {
    std::lock_guard<std::mutex> g(g_pool_mu);
    uint64_t n_large = 0, bytes = 0;
    for (const fh_batch *c : g_pool)
        if (c->large) n_large++, bytes += c->dev_bytes;
    if (handles) *handles = g_pool.size();
    if (large_handles) *large_handles = n_large;
    if (large_device_bytes) *large_device_bytes = bytes;
    return FH_OK;
}

int fh_batch_stage(fh_batch *b, int slot, uint8_t **buf, uint64_t *cap) {
    if (!b || slot < 0 || slot > 1 || !buf || !cap) return api_fail(FH_ERR_INVALID, "bad argument");
    if (b->slot[slot].in_flight) return api_fail(FH_ERR_STATE, "slot %d is in flight: fh_batch_wait first", slot);
    *buf = b->slot[slot].h_stage + b->header_bytes;
    *cap = b->data_bytes;
    return FH_OK;
}

static int batch_submit(fh_batch *b, int slot, const uint64_t *offsets, const uint64_t *lens, uint32_t n_files, bool two_bit) try {
    if (!b || slot < 0 || slot > 1 || (n_files && (!offsets || !lens))) return api_fail(FH_ERR_INVALID, "bad argument");
    fh_batch::Slot &s = b->slot[slot];
    if (s.in_flight) return api_fail(FH_ERR_STATE, "slot %d is in flight: fh_batch_wait first", slot);
    if (n_files > b->max_files) return api_fail(FH_ERR_INVALID, "%u files in a batch of at most %u", n_files, b->max_files);
    BHIP_TRY(hipSetDevice(b->device));
    BatchFile *hd = reinterpret_cast<BatchFile *>(s.h_stage);
    uint64_t end = 0, tiles = 0, positions = 0, prev_end = 0;
    for (uint32_t f = 0; f < n_files; ++f) {
        // bytes the file occupies in the staging buffer: its stream, or its region in the two-bit form (fh_pack2.h)
        if (two_bit && lens[f] > (1ull << 40)) return api_fail(FH_ERR_INVALID, "file %u: %llu positions", f, (unsigned long long)lens[f]);
        const uint64_t bytes = two_bit ? fh_pack2::region_bytes(lens[f]) : lens[f];
        const uint64_t align = two_bit ? 63u : 15u;
        if ((offsets[f] & align) || offsets[f] > b->data_bytes || bytes > b->data_bytes - offsets[f])
            return api_fail(FH_ERR_INVALID, "file %u: [%llu, +%llu) is not a %u-byte aligned range of the staging buffer", f,
                            (unsigned long long)offsets[f], (unsigned long long)bytes, (unsigned)align + 1u);
        if (f && offsets[f] < prev_end) return api_fail(FH_ERR_INVALID, "file %u overlaps file %u (offsets ascend)", f, f - 1);
        prev_end = offsets[f] + bytes;
        const uint64_t n_tiles = (lens[f] + TILE_POS - 1) / TILE_POS;
        if (tiles + n_tiles > 0xFFFFFFF0ull) return api_fail(FH_ERR_INVALID, "batch too large");
        BatchFile &d = hd[f];
        d.seq = s.d_stage + b->header_bytes + offsets[f];
        d.len = lens[f];
        d.ctl = b->counts ? nullptr : b->ctls + f;
        // (large: option batch_large_want in place of the plan's factor -- tests force a short guess or a full live list with it)
        const uint64_t tau = bp::tau(b->form, b->p.kind, b->p.size, b->max_hash, lens[f], b->large ? cfg_u64("batch_large_want", bp::LARGE_WANT) : 0);
        d.tau = tau;
        d.tile0 = (uint32_t)tiles;
        d.n_tiles = (uint32_t)n_tiles;
        if (!b->counts) s.tau[f] = tau;
        s.len[f] = lens[f];
        tiles += n_tiles;
        positions += lens[f];
        end = std::max(end, prev_end);
    }
    s.n_files = n_files;
    s.positions = positions;
    s.waited = false;
    if (n_files == 0) {
        s.in_flight = true;
        BHIP_TRY(hipEventRecord(s.done, b->stream));
        return FH_OK;
    }
    BHIP_TRY(hipMemcpyAsync(s.d_stage, s.h_stage, b->header_bytes + ((end + 15) & ~15ull), hipMemcpyHostToDevice, b->stream));
    if (b->counts) {
        if (tiles) {
            AcBatchArgs a{};
            a.files = reinterpret_cast<const BatchFile *>(s.d_stage);
            a.n_files = n_files;
            a.tiles_total = (uint32_t)tiles;
            a.two_bit = two_bit ? 1u : 0u;
            a.tables = b->ac_tables;
            if (b->profiling) BHIP_TRY(hipEventRecord(s.k0, b->stream));
            BHIP_TRY(launch_ac_batch_count((int)b->p.k, a, b->stream));
            if (b->profiling) BHIP_TRY(hipEventRecord(s.k1, b->stream));
        }
        BHIP_TRY(launch_ac_batch_epilogue(b->ac_tables, (int)b->p.k, n_files, reinterpret_cast<uint32_t *>(s.h_out), b->out_stride, s.h_res, b->stream));
        BHIP_TRY(hipEventRecord(s.done, b->stream));
        s.in_flight = true;
        return FH_OK;
    }
    if (tiles) {
        BatchArgs a{};
        a.files = reinterpret_cast<const BatchFile *>(s.d_stage);
        a.n_files = n_files;
        a.tiles_total = (uint32_t)tiles;
        const bool wide = b->p.k > 32;
        const uint64_t wpb = (uint64_t)k2_waves_per_block((int)b->p.k); // (WAVES_PER_BLOCK for k > 32)
        a.tiles_per_wave = (uint32_t)std::max<uint64_t>(1, (tiles + BATCH_MAX_WAVES - 1) / BATCH_MAX_WAVES);
        const uint64_t waves = ((tiles + a.tiles_per_wave - 1) / a.tiles_per_wave + wpb - 1) / wpb * wpb;
        a.seed = b->p.seed;
        a.two_bit = two_bit ? 1u : 0u;
        if (b->profiling) BHIP_TRY(hipEventRecord(s.k0, b->stream));
        BHIP_TRY(wide ? launch_k2bw((int)b->p.k, a, (uint32_t)waves, b->stream) : launch_k2b((int)b->p.k, a, (uint32_t)waves, b->stream));
        if (b->profiling) BHIP_TRY(hipEventRecord(s.k1, b->stream));
    }
    BHIP_TRY(b->large ? launch_batch_epilogue_large(s.d_epi_large, n_files, 1u, b->stream) : launch_batch_epilogue(s.d_epi, n_files, 1u, b->stream));
    BHIP_TRY(hipEventRecord(s.done, b->stream));
    s.in_flight = true;
    return FH_OK;
} catch (...) {
    return api_fail(FH_ERR_CAPACITY, "out of host memory");
}

int fh_batch_submit(fh_batch *b, int slot, const uint64_t *offsets, const uint64_t *lens, uint32_t n_files) {
    return batch_submit(b, slot, offsets, lens, n_files, false);
}

int fh_batch_submit_packed(fh_batch *b, int slot, const uint64_t *offsets, const uint64_t *lens, uint32_t n_files) {
    return batch_submit(b, slot, offsets, lens, n_files, true);
}

uint64_t fh_batch_packed_bytes(uint64_t len) { return fh_pack2::region_bytes(len); }

int fh_batch_pack(const uint8_t *stream, uint64_t len, uint8_t *region, uint64_t region_cap) {
    if ((len && !stream) || !region) return api_fail(FH_ERR_INVALID, "bad argument");
    if (len > (1ull << 40) || fh_pack2::region_bytes(len) > region_cap)
        return api_fail(FH_ERR_CAPACITY, "%llu positions take %llu bytes in the two-bit form, the region has %llu", (unsigned long long)len,
                        (unsigned long long)fh_pack2::region_bytes(len), (unsigned long long)region_cap);
    const bool avx2 = fh_pack2::have_avx2() && !cfg_on("pack_scalar");
    const uint64_t whole = len / 32;
    fh_pack2::pack_groups(stream, (size_t)whole, region, 0, avx2);
    uint64_t groups = whole;
    if (len & 31u) {
        uint8_t last[32] = {0};
        memcpy(last, stream + 32 * whole, (size_t)(len & 31u));
        fh_pack2::pack_groups(last, 1, region, groups++, avx2);
    }
    const uint64_t n_tiles = (len + TILE_POS - 1) / TILE_POS;
    for (uint64_t g = groups; g < n_tiles * 64; ++g) {
        uint8_t *const tile = region + (g >> 6) * fh_pack2::TILE_BYTES;
        memset(tile + 8 * (g & 63), 0, 8);
        memset(tile + fh_pack2::CODES_BYTES + 4 * (g & 63), 0, 4);
    }
    memset(region + n_tiles * fh_pack2::TILE_BYTES, 0, fh_pack2::TILE_BYTES);
    return FH_OK;
}

int fh_batch_wait(fh_batch *b, int slot, uint8_t *status) {
    if (!b || slot < 0 || slot > 1) return api_fail(FH_ERR_INVALID, "bad argument");
    fh_batch::Slot &s = b->slot[slot];
    if (!s.in_flight) return api_fail(FH_ERR_STATE, "slot %d has nothing in flight", slot);
    BHIP_TRY(hipSetDevice(b->device));
    BHIP_TRY(hipEventSynchronize(s.done));
    s.in_flight = false;
    if (!s.waited) {
        s.waited = true;
        if (b->profiling && s.n_files && s.positions) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, s.k0, s.k1) == hipSuccess) {
                b->prof_ms += ms;
                b->prof_launches++;
                b->prof_positions += s.positions;
            } else {
                (void)hipGetLastError();
            }
        }
        if (b->counts) { // the epilogue has run for every file: a count is exact whatever the input
            std::fill(s.status.begin(), s.status.begin() + s.n_files, (uint8_t)0);
            b->n_taken += s.n_files;
        }
        for (uint32_t f = 0; !b->counts && f < s.n_files; ++f) {
            const Ctl &c = s.h_ctl[f];
            const bool ok = bp::taken(b->p.kind, b->p.size, bp::Outcome{c.sorted, c.overflow, c.need_big, c.n_coll, c.n_live, c.sp_count, c.inserted_total}, s.tau[f]);
            s.status[f] = ok ? 0 : 1;
            if (ok) b->n_taken++;
            else b->n_not_taken++;
        }
    }
    if (status) memcpy(status, s.status.data(), s.n_files);
    return FH_OK;
}

static int batch_file(fh_batch *b, int slot, uint32_t i, const Ctl **c, const uint64_t **cols) {
    if (!b || slot < 0 || slot > 1) return api_fail(FH_ERR_INVALID, "bad argument");
    const fh_batch::Slot &s = b->slot[slot];
    if (s.in_flight || !s.waited) return api_fail(FH_ERR_STATE, "slot %d: fh_batch_wait first", slot);
    if (i >= s.n_files) return api_fail(FH_ERR_INVALID, "file %u of a batch of %u", i, s.n_files);
    if (s.status[i] != 0) return api_fail(FH_ERR_STATE, "file %u was not taken by the batch path", i);
    *c = b->counts ? nullptr : &s.h_ctl[i];
    *cols = s.h_out + (size_t)i * b->out_words;
    return FH_OK;
}

// a file of a counts handle: to_vec's rows as the epilogue left them (ix | count | extra_count).  hash = ix, the k-mer is the
// text of ix, first_pos is 0 (as an AllCounts fh_sketcher gives them)
static void counts_rows(const fh_batch *b, int slot, uint32_t i, const uint64_t *cols, uint64_t *hashes, uint32_t *counts, uint32_t *extra_counts,
                        fh_kmer_count *records, uint8_t *kmers, uint64_t *first_pos) {
    const size_t n = b->slot[slot].h_res[i].n_out, st = b->out_stride;
    const uint32_t *ix = reinterpret_cast<const uint32_t *>(cols), *cc = ix + st, *ee = cc + st;
    if (counts) memcpy(counts, cc, n * 4);
    if (extra_counts) memcpy(extra_counts, ee, n * 4);
    if (first_pos) memset(first_pos, 0, n * 8);
    for (size_t j = 0; j < n; ++j) {
        if (hashes) hashes[j] = ix[j];
        if (records) records[j] = fh_kmer_count{ix[j], cc[j], ee[j]};
        if (kmers) api_kmer_ascii(ix[j], 0, (int)b->p.k, kmers + j * b->p.k);
    }
}

// the columns of one file's rows as the epilogue laid them out (small_epilogue_body, fh_kernels.hip): the high k-mer words sit
// between the first positions and the counts when k > 32
struct BatchCols {
    const uint64_t *hash, *kmer, *pos, *kmer_hi;
    const uint32_t *count, *extra;
};
static BatchCols batch_cols(const fh_batch *b, const uint64_t *cols) {
    const size_t st = b->out_stride;
    BatchCols v;
    v.hash = cols;
    v.kmer = v.hash + st;
    v.pos = v.kmer + st;
    v.kmer_hi = b->p.k > 32 ? v.pos + st : nullptr;
    v.count = reinterpret_cast<const uint32_t *>((v.kmer_hi ? v.kmer_hi : v.pos) + st);
    v.extra = v.count + st;
    return v;
}

int fh_batch_result(fh_batch *b, int slot, uint32_t i, uint64_t *n_out, uint64_t *total_kmers) {
    const Ctl *c = nullptr;
    const uint64_t *cols = nullptr;
    if (int rc = batch_file(b, slot, i, &c, &cols)) return rc;
    if (b->counts) {
        if (n_out) *n_out = b->slot[slot].h_res[i].n_out;
        if (total_kmers) *total_kmers = b->slot[slot].h_res[i].total_kmers;
        return FH_OK;
    }
    if (n_out) *n_out = c->n_live;
    if (total_kmers) {
        uint64_t t = 0;
        for (int j = 0; j < 256; ++j) t += c->kmer_counts[j];
        *total_kmers = t;
    }
    return FH_OK;
}

int fh_batch_copy_out(fh_batch *b, int slot, uint32_t i, uint64_t *hashes, uint32_t *counts, uint32_t *extra_counts, uint8_t *kmers,
                      uint64_t *first_pos) {
    const Ctl *c = nullptr;
    const uint64_t *cols = nullptr;
    if (int rc = batch_file(b, slot, i, &c, &cols)) return rc;
    if (b->counts) {
        counts_rows(b, slot, i, cols, hashes, counts, extra_counts, nullptr, kmers, first_pos);
        return FH_OK;
    }
    const size_t n = c->n_live;
    const BatchCols v = batch_cols(b, cols);
    if (hashes) memcpy(hashes, v.hash, n * 8);
    if (counts) memcpy(counts, v.count, n * 4);
    if (extra_counts) memcpy(extra_counts, v.extra, n * 4);
    if (first_pos) memcpy(first_pos, v.pos, n * 8);
    if (kmers)
        for (size_t j = 0; j < n; ++j) api_kmer_ascii(v.kmer[j], v.kmer_hi ? v.kmer_hi[j] : 0, (int)b->p.k, kmers + j * b->p.k);
    return FH_OK;
}

int fh_batch_copy_out_records(fh_batch *b, int slot, uint32_t i, fh_kmer_count *records, uint8_t *kmers) {
    const Ctl *c = nullptr;
    const uint64_t *cols = nullptr;
    if (int rc = batch_file(b, slot, i, &c, &cols)) return rc;
    if (b->counts) {
        counts_rows(b, slot, i, cols, nullptr, nullptr, nullptr, records, kmers, nullptr);
        return FH_OK;
    }
    const size_t n = c->n_live;
    const BatchCols v = batch_cols(b, cols);
    if (records)
        for (size_t j = 0; j < n; ++j) records[j] = fh_kmer_count{v.hash[j], v.count[j], v.extra[j]};
    if (kmers)
        for (size_t j = 0; j < n; ++j) api_kmer_ascii(v.kmer[j], v.kmer_hi ? v.kmer_hi[j] : 0, (int)b->p.k, kmers + j * b->p.k);
    return FH_OK;
}

int fh_batch_set_profiling(fh_batch *b, int enable) {
    if (!b) return api_fail(FH_ERR_INVALID, "null handle");
    b->profiling = enable != 0;
    return FH_OK;
}

int fh_batch_kernel_time(fh_batch *b, double *total_ms, uint64_t *launches, uint64_t *positions) {
    if (!b) return api_fail(FH_ERR_INVALID, "null handle");
    if (total_ms) *total_ms = b->prof_ms;
    if (launches) *launches = b->prof_launches;
    if (positions) *positions = b->prof_positions;
    b->prof_ms = 0.0;
    b->prof_launches = b->prof_positions = 0;
    return FH_OK;
}

int fh_batch_counters(fh_batch *b, uint64_t *taken, uint64_t *not_taken) {
    if (!b) return api_fail(FH_ERR_INVALID, "null handle");
    if (taken) *taken = b->n_taken;
    if (not_taken) *not_taken = b->n_not_taken;
    return FH_OK;
}

} // extern "C"
