// fh_batch_plan.h -- the host rules of the batch sketcher (fh_batch.hip, finch_sketch_files in fh_host.cpp), each written once:
// which parameters a door of the sketcher takes and what it says to the others, the sizes of a handle, when a parked handle may
// be handed out again, the threshold a file is sketched at, when its result is taken, and which door serves a call of
// finch_sketch_files.  No HIP and no globals: the standard library, the C ABI's types and fh_counts.h (for ac_max_rows), so
// that tests/hostcore/batch_plan_host.cpp runs all of it on the host.  The constants that mirror the device headers are held to
// them by static_asserts in fh_batch.hip.
#pragma once

#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/finch_hip.h"
#include "fh_counts.h"

namespace fh {
namespace bplan {

// the door a handle was made through: fh_batch_new, _new_wide (k = 33..64), _new_large (Mash sizes above 3000), _new_counts
enum class Form { Small, Wide, Large, Counts };

// --- mirrors of fh_device.h, fh_kernels.h and fh_pack2.h (fh_batch.hip: static_asserts) ---
constexpr uint64_t EMPTY = ~0ull;         // EMPTY64
constexpr uint32_t FIN_OK = 2;            // FIN_OK_RESET: the epilogue finished the sketch and left the partition reset
constexpr uint64_t SMALL_ROWS = 12288;    // SMALL_MAX: keys the small epilogue's workgroup holds in LDS
constexpr uint64_t LARGE_ROWS = 16384;    // LARGE_MAX_ROWS: sorted keys the large epilogue keeps in LDS
constexpr uint32_t COUNTS_MAX_K = 7;      // AC_LDS_MAX_K
constexpr uint32_t MAX_K = 64;            // FH_MAX_K
constexpr uint64_t SHARDS = 256, SHARD_CURSOR_STRIDE = 32; // N_SHARDS, SHARD_STRIDE
constexpr uint64_t ENTRY_BYTES = 40, CTL_BYTES = 3680, COLL_BYTES = 32, FILE_BYTES = 40; // sizeof Entry, Ctl, CollRec, BatchFile
constexpr uint64_t TWO_BIT_TILE = 768;    // fh_pack2::TILE_BYTES

// --- the batch sketcher's own ---
constexpr uint32_t PART_CAP = 32768;      // table entries per file: at most SMALL_ROWS hashes are ever wanted in one
constexpr uint32_t PART_LIVE = 16384;     // live / dead list entries per file (> SMALL_ROWS)
constexpr uint32_t PART_SHARD_CAP = 512;  // entries per shard list (inserts are dealt over the 256 lists drain by drain)
constexpr uint32_t PART_CLOG = 64;        // collision records per file (any collision sends the file the long way)
constexpr uint64_t MAX_N = 3000;          // kmers_to_sketch the in-LDS selection serves (fh_api.hip SMALL_N_MAX)
constexpr uint64_t LARGE_MAX_N = FH_BATCH_LARGE_MAX_N; // ... and the selection over device memory (fh_batch_large.hip)
constexpr uint64_t LARGE_WANT = 4;        // a large file's threshold: LARGE_WANT x n hashes expected below it (option batch_large_want)
// rows of a Scaled sketch: what the epilogue's workgroup holds the keys of in LDS.  The partition does not bind it: its table is
// 37 % full at that many entries, its live and dropped-slot lists hold PART_LIVE, and the 256 shard lists take 512 each of
// inserts that are dealt over them drain by drain (48 on average).
constexpr uint64_t SCALED_MAX = FH_BATCH_SCALED_MAX;
static_assert(LARGE_MAX_N == LARGE_ROWS, "the large epilogue keeps that many sorted keys in LDS");
static_assert(SCALED_MAX == SMALL_ROWS && SCALED_MAX <= PART_LIVE && 2 * SCALED_MAX <= PART_CAP,
              "a Scaled batch sketch fits the epilogue's LDS block and the partition");
constexpr uint32_t MAX_FILES = 4096;
constexpr uint64_t MAX_STAGE = 1ull << 36;
// an AllCounts or large handle's staging buffer: below 2^21 tiles of the two-bit form, so that no file has 2^32 positions (the
// 4 KiB rounding of stage_bytes stays below it too)
constexpr uint64_t COUNTS_MAX_STAGE = (1ull << 21) * TWO_BIT_TILE - 4096;
// finch_sketch_files: a group's staging buffer and its files (a large handle: option batch_large_files, 16)
constexpr uint64_t GROUP_STAGE = 32ull << 20;
constexpr uint32_t GROUP_FILES = 64;

// ---------------------------------------------------------------------------------------------------------------------------
// What a door says to (params, max_files, stage_bytes): FH_OK, or the code and the message of its refusal.  Every door has its
// own words and its own order of checks (tests/golden/batch_refusals.json pins them); the parameters speak before the sizes.
struct Verdict {
    int code = FH_OK;
    char msg[512] = "";
};
__attribute__((format(printf, 2, 3))) inline Verdict refuse(int code, const char *fmt, ...) {
    Verdict v;
    v.code = code;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(v.msg, sizeof v.msg, fmt, ap);
    va_end(ap);
    return v;
}

inline bool scale_ok(double scale) { return scale > 0.0 && scale <= 1.0; } // (as fh_new)
inline bool sizes_ok(uint32_t max_files, uint64_t stage_bytes, uint64_t max_stage) {
    return max_files >= 1 && max_files <= MAX_FILES && stage_bytes >= 4096 && stage_bytes <= max_stage;
}

inline Verdict check(Form form, const fh_params *p, uint32_t max_files, uint64_t stage_bytes) {
    typedef unsigned long long ull;
    const bool scaled = p->kind == FH_KIND_SCALED;
    const bool small_size_ok = scaled ? p->size <= SCALED_MAX : (p->size >= 1 && p->size <= MAX_N);
    switch (form) {
    case Form::Small:
        if (p->kind == FH_KIND_ALL_COUNTS)
            return refuse(FH_ERR_UNSUPPORTED, "the batch sketcher serves Mash sketches only: AllCounts sketches go through an fh_sketcher");
        if (p->kind != FH_KIND_MASH && !scaled) return refuse(FH_ERR_INVALID, "unknown sketch kind %u", p->kind);
        if (p->k < 1 || p->k > 32 || p->hash_mask != 0 || !small_size_ok)
            return refuse(FH_ERR_UNSUPPORTED,
                          "the batch sketcher serves Mash sketches of 1..%llu hashes and Scaled sketches of size 0..%llu, k = 1..32, no test mask (k = 33..64: fh_batch_new_wide; Mash sketches of 3001..%u hashes: fh_batch_new_large)",
                          (ull)MAX_N, (ull)SCALED_MAX, (unsigned)LARGE_MAX_N);
        if (scaled && !scale_ok(p->scale)) return refuse(FH_ERR_INVALID, "scale must be in (0, 1]");
        break;
    case Form::Wide:
        if (p->kind == FH_KIND_ALL_COUNTS)
            return refuse(FH_ERR_UNSUPPORTED, "the batch sketcher for k = 33..64 serves Mash and Scaled sketches: AllCounts (kind 2) batches are fh_batch_new_counts, k = 1..%d",
                          (int)COUNTS_MAX_K);
        if (p->kind != FH_KIND_MASH && !scaled) return refuse(FH_ERR_INVALID, "unknown sketch kind %u (0 Mash, 1 Scaled)", p->kind);
        if (p->k <= 32) return refuse(FH_ERR_UNSUPPORTED, "fh_batch_new_wide serves k = 33..64: k = %u is fh_batch_new's (k = 1..32)", p->k);
        if (p->k > MAX_K) return refuse(FH_ERR_UNSUPPORTED, "fh_batch_new_wide serves k = 33..64: k = %u is beyond what the device hashes", p->k);
        if (p->hash_mask != 0) return refuse(FH_ERR_UNSUPPORTED, "the batch sketcher takes no test mask (hash_mask must be 0)");
        if (!small_size_ok)
            return refuse(FH_ERR_UNSUPPORTED, "the batch sketcher serves Mash sketches of 1..%llu hashes and Scaled sketches of size 0..%llu: size %llu",
                          (ull)MAX_N, (ull)SCALED_MAX, (ull)p->size);
        if (scaled && !scale_ok(p->scale)) return refuse(FH_ERR_INVALID, "scale must be in (0, 1]");
        break;
    case Form::Large:
        if (scaled || p->kind == FH_KIND_ALL_COUNTS)
            return refuse(FH_ERR_UNSUPPORTED, "fh_batch_new_large serves Mash sketches only: %s",
                          scaled ? "Scaled (kind 1) batches are fh_batch_new's (k = 1..32) and fh_batch_new_wide's" : "AllCounts (kind 2) batches are fh_batch_new_counts");
        if (p->kind != FH_KIND_MASH) return refuse(FH_ERR_INVALID, "unknown sketch kind %u (fh_batch_new_large: 0 Mash)", p->kind);
        if (p->size <= MAX_N)
            return refuse(FH_ERR_UNSUPPORTED, "fh_batch_new_large serves Mash sketches of %llu..%u hashes: size %llu is fh_batch_new's (1..%llu)", (ull)MAX_N + 1,
                          (unsigned)LARGE_MAX_N, (ull)p->size, (ull)MAX_N);
        if (p->size > LARGE_MAX_N)
            return refuse(FH_ERR_UNSUPPORTED, "fh_batch_new_large serves Mash sketches of %llu..%u hashes (FH_BATCH_LARGE_MAX_N): size %llu goes through an fh_sketcher",
                          (ull)MAX_N + 1, (unsigned)LARGE_MAX_N, (ull)p->size);
        if (p->k < 1 || p->k > 32) return refuse(FH_ERR_UNSUPPORTED, "fh_batch_new_large serves k = 1..32: k = %u goes through an fh_sketcher", p->k);
        if (p->hash_mask != 0) return refuse(FH_ERR_UNSUPPORTED, "the batch sketcher takes no test mask (hash_mask must be 0)");
        // (the bound of fh_batch_new_counts: with fewer than 2^21 tiles in a slot a file has fewer than 2^32 positions)
        if (!sizes_ok(max_files, stage_bytes, COUNTS_MAX_STAGE))
            return refuse(FH_ERR_INVALID, "max_files 1..%u, stage_bytes 4 KiB..%llu (a slot of fewer than 2^21 tiles of the two-bit form)", MAX_FILES, (ull)COUNTS_MAX_STAGE);
        return Verdict{};
    case Form::Counts: // (of p only k is looked at)
        if (p->k < 1) return refuse(FH_ERR_INVALID, "kmer_length must be at least 1");
        if (p->k > COUNTS_MAX_K)
            return refuse(FH_ERR_UNSUPPORTED, "the AllCounts batch sketcher serves k = 1..%d (one file's 4^k counts in a workgroup's LDS): k = %u goes through an fh_sketcher",
                          (int)COUNTS_MAX_K, p->k);
        // fewer than 2^32 positions per file, whichever form it is staged in
        if (!sizes_ok(max_files, stage_bytes, COUNTS_MAX_STAGE))
            return refuse(FH_ERR_INVALID, "max_files 1..%u, stage_bytes 4 KiB..%llu (an AllCounts file has fewer than 2^32 positions)", MAX_FILES, (ull)COUNTS_MAX_STAGE);
        return Verdict{};
    }
    if (!sizes_ok(max_files, stage_bytes, MAX_STAGE)) return refuse(FH_ERR_INVALID, "max_files 1..%u, stage_bytes 4 KiB..64 GiB", MAX_FILES);
    return Verdict{};
}

// ---------------------------------------------------------------------------------------------------------------------------
// The sizes of a handle that passed check().
//
// A large handle's partitions.  With every position a distinct k-mer and uniform hashes, the number of a file's hashes below its
// threshold is Binomial(len, want n / len): mean 4 n, standard deviation below sqrt(4 n) = 256 at n = 16 384.  The live and
// dropped-slot lists (and the key scratch) hold 4 n + 8192 -- 32 standard deviations at the largest n, more at every smaller
// one -- rounded up to 1024; the table twice that, so it is at most half full; a shard list eight times its mean share
// (live_cap / 32 against live_cap / 256: the small partitions' 512 against 48 is the same order).
struct Geometry {
    uint32_t cap = 0, live_cap = 0, shard_cap = 0; // a partition's table, its live / dead lists, a shard list (counts: none)
    uint64_t rows = 0;                             // most rows of a file's result
    uint32_t out_stride = 0;                       // entries between the columns of one result
    size_t out_words = 0;                          // u64 words of one result's columns
    uint64_t header_bytes = 0, data_bytes = 0;     // a slot's staging buffer: the file descriptors, then the files
    uint64_t dev_bytes = 0;                        // device memory the handle holds (what parking it costs, fh_batch_free)
};
inline uint64_t stage_rounded(uint64_t stage_bytes) { return (stage_bytes + 4095) & ~4095ull; }
inline Geometry geometry(Form form, const fh_params &p, uint32_t max_files, uint64_t stage_bytes) {
    Geometry g;
    const uint64_t F = max_files;
    g.header_bytes = (F * FILE_BYTES + 4095) & ~4095ull;
    g.data_bytes = stage_rounded(stage_bytes);
    const uint64_t slots = 2 * (g.header_bytes + g.data_bytes + 64);
    if (form == Form::Counts) {
        // a file's columns hold the most rows to_vec can emit from 4^k bins: (4^k + palindromes) / 2
        g.rows = ac_max_rows((int)p.k);
        g.out_stride = ((uint32_t)g.rows + 1u) & ~1u;
        g.out_words = (size_t)g.out_stride * 3 / 2; // ix | count | extra_count: 3 x 4 bytes per entry
        g.dev_bytes = F * ac_bins((int)p.k) * 4 + slots;
        return g;
    }
    const bool large = form == Form::Large, wide = form == Form::Wide;
    g.live_cap = large ? (uint32_t)((LARGE_WANT * p.size + 8192 + 1023) & ~1023ull) : PART_LIVE;
    g.cap = large ? 2 * g.live_cap : PART_CAP;
    g.shard_cap = large ? g.live_cap / 32 : PART_SHARD_CAP;
    // a sketch's columns as fh_finish lays them out: hash | k-mer | first position | [k > 32: high k-mer word] | count | extra,
    // out_stride entries apart (a Scaled sketch has up to SCALED_MAX rows whatever its size)
    g.rows = p.kind == FH_KIND_SCALED ? SCALED_MAX : std::min<uint64_t>(p.size + 1, large ? LARGE_MAX_N + 1 : SMALL_ROWS);
    g.out_stride = (uint32_t)((g.rows + 2) & ~1ull);
    g.out_words = (size_t)g.out_stride * (wide ? 5 : 4); // (3 or 4) x 8 + 2 x 4 bytes per entry
    g.dev_bytes = F * ((uint64_t)g.cap * (ENTRY_BYTES + (wide ? 8 : 0)) + (uint64_t)g.live_cap * (8 + (large ? 8 : 0)) +
                       SHARDS * (g.shard_cap + SHARD_CURSOR_STRIDE) * 4 + CTL_BYTES + PART_CLOG * COLL_BYTES) +
                  slots;
    return g;
}

// ---------------------------------------------------------------------------------------------------------------------------
// A parked handle (fh_batch_free) is handed out again to the door it was made through, for the same device and sizes, and the
// parameters that shaped it: every door k; small, wide and large the sketch's size and the seed; small and wide the kind, and
// the scale of a Scaled one.
struct PoolKey {
    Form form;
    int device;
    uint32_t max_files;
    uint64_t data_bytes;
    fh_params p;
};
inline bool pool_match(const PoolKey &parked, const PoolKey &asked) {
    const fh_params &a = parked.p, &b = asked.p;
    if (parked.form != asked.form || parked.device != asked.device || parked.max_files != asked.max_files || parked.data_bytes != asked.data_bytes || a.k != b.k)
        return false;
    if (asked.form == Form::Counts) return true;
    if (a.size != b.size || a.seed != b.seed) return false;
    if (asked.form == Form::Large) return true;
    return a.kind == b.kind && (b.kind != FH_KIND_SCALED || a.scale == b.scale);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The one threshold a file of `len` positions is sketched at: that below which E of its positions' hashes are expected (every
// position a distinct k-mer, hashes uniform), E = 4 n (3 n for n > 2000), a large handle's large_want x n; EMPTY -- everything is
// admitted -- where the file has no more positions than that.  A Scaled file's is max_hash (u64::MAX at scale 1 is EMPTY: the
// one hash that cannot be a table key is counted in sp_count, which sends the file the long way); a count has none.
inline uint64_t expected_below(uint64_t n) { return n <= 2000 ? 4 * n : 3 * n; }
inline uint64_t tau(Form form, uint32_t kind, uint64_t size, uint64_t max_hash, uint64_t len, uint64_t large_want) {
    if (form == Form::Counts) return 0; // (not looked at)
    if (kind == FH_KIND_SCALED) return max_hash;
    const uint64_t E = form == Form::Large ? std::max<uint64_t>(1, large_want) * size : expected_below(size);
    if (len <= E) return EMPTY;
    const uint64_t t = (uint64_t)((((unsigned __int128)E) << 64) / len);
    return t >= EMPTY - 1 ? EMPTY : t;
}

// What fh_batch_wait reads of a file's control block, and the rule: taken iff the epilogue finished the sketch and left the
// partition reset, the guess held (or admitted everything), no two k-mers shared a hash and the one hash value that cannot be a
// table key did not occur.  Scaled: every live entry is <= max_hash by construction; they are the sketch iff there are at
// least `size` of them (and no more than the epilogue sorts).
struct Outcome {
    uint32_t sorted, overflow, need_big, n_coll, n_live;
    uint64_t sp_count, inserted_total;
};
inline bool taken(uint32_t kind, uint64_t size, const Outcome &c, uint64_t file_tau) {
    const bool scaled = kind == FH_KIND_SCALED;
    const bool fin = c.sorted == FIN_OK && c.overflow == 0 && c.need_big == 0;
    const bool full = scaled ? (uint64_t)c.n_live >= size : (file_tau == EMPTY || c.inserted_total >= size);
    const bool rows = (uint64_t)c.n_live <= (scaled ? SCALED_MAX : size);
    return fin && full && c.n_coll == 0 && c.sp_count == 0 && rows;
}

// ---------------------------------------------------------------------------------------------------------------------------
// finch_sketch_files: the door that serves a call's files many per launch, and the size its handle is made for -- what the
// small sketcher cuts a Mash sketch to (final_size below kmers_to_sketch), a Scaled sketch's kmers_to_sketch.  None (ok = false)
// for a single file, with filtering asked for, and whenever that door's own check() refuses the parameters: there is no second
// statement of the limits.
struct FilePlan {
    bool ok = false;
    Form form = Form::Small;
    uint64_t group_n = 0;
};
inline FilePlan plan_files(uint32_t kind, uint32_t kmer_length, uint64_t kmers_to_sketch, uint64_t final_size, double scale, int filter_on, uint32_t n_files) {
    FilePlan f;
    f.group_n = kind == FH_KIND_SCALED || !(final_size >= 1 && final_size < kmers_to_sketch) ? kmers_to_sketch : final_size;
    f.form = kind == FH_KIND_ALL_COUNTS ? Form::Counts : kmer_length > 32 ? Form::Wide : (kind == FH_KIND_MASH && f.group_n > MAX_N) ? Form::Large : Form::Small;
    fh_params p{};
    p.kind = kind;
    p.k = kmer_length;
    p.size = f.group_n;
    p.scale = scale;
    f.ok = n_files > 1 && filter_on <= 0 && check(f.form, &p, GROUP_FILES, GROUP_STAGE).code == FH_OK;
    return f;
}
// A Scaled file whose size says it cannot fit is not staged at all (sending it would cost a wasted pass): if every byte began
// a distinct k-mer, st_size x max_hash / 2^64 hashes would lie at or below max_hash.  Margin: staged up to 5/4 of the cap --
// headers, line ends, N and repeated k-mers make the true number smaller than that estimate, never larger, so a file up to a
// quarter above the cap may still fit; one further above is all but certain not to (the count is a sum of ~independent
// draws: at 12 288 its standard deviation is ~110, the margin 28 of them).
inline bool scaled_may_fit(uint64_t st_size, uint64_t max_hash) {
    return (uint64_t)(((unsigned __int128)st_size * max_hash) >> 64) <= SCALED_MAX + SCALED_MAX / 4;
}

} // namespace bplan
} // namespace fh
