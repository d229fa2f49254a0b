// fh_records.hip -- ONE SKETCH PER RECORD: the record sketcher (include/finch_hip.h, fh_records_*), hand-written for gfx950.
//
// A multi-FASTA of plasmids, 16S sequences or contigs holds records of a few thousand bases, and each wants a sketch of its
// own (mash sketch -i, sourmash --singleton).  The batch sketcher (fh_k2b.hip) gives every input a table partition, shard
// lists and an epilogue workgroup and hands a wave whole tiles: machinery a short record does not need, because ALL its
// hashes fit one workgroup's LDS.  k_record_sketch does everything for a record there:
//
//   * a workgroup is persistent: it fills the murmur3 tables once (lut_rec_A / B / P, the plain layout) and takes a contiguous
//     run of the launch's records; everything about the current record is wave-uniform;
//   * the waves deal the record's tiles among themselves in units of 8 window starts per lane (a 1 500-base record is one tile:
//     dealt whole it would keep one wave of eight busy); a unit is load_tile_two_bit's layout, window_valid_mask, Windows and
//     murmur_h1_fast -- the tile kernels' arithmetic, not a second statement of it;
//   * every valid window writes (hash, position | strand << 31) into two LDS arrays, at an index from a ballot / mbcnt prefix
//     within the wave and one LDS counter across waves;
//   * the keys are padded with EMPTY64 to a power of two and sorted (bitonic_lds, fh_epilogue_dev.h); a run of equal keys is
//     one distinct hash, its head the entry whose predecessor differs; a workgroup scan numbers the heads; the lanes of the
//     kept heads sum their runs' occurrences and reverse-strand occurrences (runs are short except in repeats, where one lane
//     walks a long one) and write the row: hash | canonical k-mer word | count | extra_count;
//   * rows kept: Mash the first min(size, distinct) heads; Scaled every head at or below max_hash and the first `size` heads
//     whatever their hash -- the closed form of scaled.rs:37-61 (a hash at or below max_hash is never evicted, one above it
//     stays only while no more than `size` are held), exact here because a head carries ALL occurrences of its hash.
//
// Not taken (status 1, nothing else written for the record; the caller sketches it through an fh_sketcher): more than
// FH_RECORDS_MAX_POS positions; two adjacent equal hashes whose canonical k-mer words -- re-derived from the record's codes at
// the two positions -- differ (a 64-bit collision); a hash equal to EMPTY64, the padding key.
//
// Compiled FH_NPARTS times like fh_k2b.hip (a share of K = 1..32 each); part 0 also holds the host side: the handle and the C ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/finch_hip.h"
#include "fh_core.h"
#include "fh_device.h"
#include "fh_kernels.h"
#include "fh_k2_common.h"
#include "fh_epilogue_dev.h"
#include "fh_internal.h"
#include "fh_options.h"
#include "fh_pack2.h"
#include "fh_records_plan.h"

#ifndef FH_PART
#error "compile with -DFH_PART=<0..FH_NPARTS-1>"
#endif

namespace fh {

struct RecDesc { // a record of a submit, in front of the staged records
    u64 off;     // its two-bit region, from the first staged byte
    u32 len;     // its positions
    u32 row0;    // where its rows begin in the slot's result
};
struct RecMeta {
    u32 n_rows, status, total_kmers, pad;
};
struct RecordArgs {
    const RecDesc *recs;
    const uint8_t *data;
    u32 n_records, per_block;
    u64 seed, size, max_hash;
    u32 scaled, pad;
    u64 *o_hash, *o_kmer;
    u32 *o_count, *o_extra;
    RecMeta *meta;
};
static_assert(sizeof(RecDesc) == rplan::DESC_BYTES, "fh_records_plan.h restates the size of a record's descriptor");
static_assert(rplan::TILE_POS == (uint64_t)TILE_POS && rplan::TWO_BIT_TILE == (uint64_t)TWO_BIT_TILE_BYTES && rplan::TWO_BIT_TILE == fh_pack2::TILE_BYTES,
              "fh_records_plan.h restates a constant of fh_device.h / fh_pack2.h");

constexpr int REC_WAVES = 8, REC_THREADS = 64 * REC_WAVES;
constexpr u32 REC_MAX_POS = rplan::MAX_POS;
constexpr int REC_UNIT = 8; // window starts per lane a wave takes at a time
static_assert((REC_MAX_POS & (REC_MAX_POS - 1)) == 0 && REC_MAX_POS % TILE_POS == 0, "a power of two, whole tiles");

// one workgroup's LDS for the largest table set (K with both pair words and 1024 last-word records)
constexpr size_t REC_LDS_BYTES = 2 * 256 * sizeof(Rec4) + 2 * 256 * sizeof(Rec2) + 1024 * sizeof(Rec2) + REC_WAVES * (256 + 128) * 4 +
                                 (size_t)REC_MAX_POS * 12 + (REC_MAX_POS / 32 + 1) * 8 + 64;
static_assert(REC_LDS_BYTES <= 160 * 1024, "one workgroup's LDS");
static_assert(REC_LDS_BYTES + (size_t)REC_MAX_POS * 12 > 160 * 1024, "FH_RECORDS_MAX_POS is the largest power of two that fits");

// the canonical k-mer word (m-form: first base most significant) of the window at `pos`, from the record's codes (group g of
// 32 positions in s_codes[g], position i of it at bits [2 i, 2 i + 2)); one zero word stands behind the last group
template <int K>
__device__ __forceinline__ u64 record_word_of(u64 lo, u64 hi, u32 s);
template <int K>
__device__ __forceinline__ u64 record_word(const u64 *s_codes, u32 pos) {
    const u32 g = pos >> 5;
    return record_word_of<K>(s_codes[g], s_codes[g + 1], 2u * (pos & 31u));
}
// ... from the record's staged two-bit region in device memory (group g: tile g / 64, word g % 64 of its codes; the zero tile
// behind the last tile stands for the zero word)
template <int K>
__device__ __forceinline__ u64 record_word_region(const uint8_t *region, u32 pos) {
    const u32 g = pos >> 5, g1 = g + 1u;
    const u64 lo = *reinterpret_cast<const u64 *>(region + (u64)(g >> 6) * TWO_BIT_TILE_BYTES + 8u * (g & 63u));
    const u64 hi = *reinterpret_cast<const u64 *>(region + (u64)(g1 >> 6) * TWO_BIT_TILE_BYTES + 8u * (g1 & 63u));
    return record_word_of<K>(lo, hi, 2u * (pos & 31u));
}
template <int K>
__device__ __forceinline__ u64 record_word_of(u64 lo, u64 hi, u32 s) {
    constexpr u64 M = K == 32 ? ~0ull : ((1ull << (2 * (K & 31))) - 1ull);
    const u64 x = (s ? (lo >> s) | (hi << (64u - s)) : lo) & M; // base i of the window at bits [2 i, 2 i + 2)
    const u64 f = pairrev64(x) >> (64 - 2 * K);                 // forward: base i at digit K - 1 - i
    const u64 r = ~x & M;                                       // reverse complement: base i's complement at digit i
    return f < r ? f : r;
}

template <int K, bool SEED0>
__global__ __launch_bounds__(REC_THREADS) void k_record_sketch(const RecordArgs a) {
    __shared__ Rec4 sA1[has_pair_word(K, false) ? 256 : 1];
    __shared__ Rec4 sA2[has_pair_word(K, true) ? 256 : 1];
    __shared__ Rec2 sB1[has_pair_word(K, false) ? 256 : 1];
    __shared__ Rec2 sB2[has_pair_word(K, true) ? 256 : 1];
    __shared__ Rec2 sP[partial_entries(K)];
    __shared__ __attribute__((aligned(16))) u32 sCodes[REC_WAVES][256];
    __shared__ __attribute__((aligned(16))) u32 sGood[REC_WAVES][128];
    __shared__ u64 s_keys[REC_MAX_POS];
    __shared__ u32 s_pay[REC_MAX_POS];
    __shared__ u64 s_rcodes[REC_MAX_POS / 32 + 1];
    __shared__ u32 s_wtot[REC_WAVES];
    __shared__ u32 s_cnt, s_nvalid, s_flag, s_rows;
    static_assert(partial_entries(K) <= 1024, "REC_LDS_BYTES counts 1024 last-word records");

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (has_pair_word(K, false)) {
        for (int q = tid; q < 256; q += REC_THREADS) {
            sA1[q] = lut_rec_A((u32)q, false);
            sB1[q] = lut_rec_B((u32)q, 4, false);
        }
    }
    if (has_pair_word(K, true)) {
        for (int q = tid; q < 256; q += REC_THREADS) {
            sA2[q] = lut_rec_A((u32)q, true);
            sB2[q] = lut_rec_B((u32)q, 4, true);
        }
    }
    for (int q = tid; q < partial_entries(K); q += REC_THREADS) sP[q] = lut_rec_P<K>((u32)q);
    const LutTables LT{sA1, sA2, sB1, sB2, sP, 0u};
    u32 *const codes_ring = sCodes[wave];
    u32 *const good_ring = sGood[wave];

    const u32 r_begin = blockIdx.x * a.per_block;
    const u32 r_end = r_begin + a.per_block < a.n_records ? r_begin + a.per_block : a.n_records;
    const RecDesc *const recs = uniform_ptr(a.recs);
    for (u32 r = r_begin; r < r_end; ++r) {
        const u32 len = (u32)__builtin_amdgcn_readfirstlane((int)recs[r].len);
        const u32 row0 = (u32)__builtin_amdgcn_readfirstlane((int)recs[r].row0);
        const uint8_t *const region = a.data + recs[r].off;
        __syncthreads(); // the tables are there; the record before is done with the LDS
        if (len > REC_MAX_POS) {
            if (tid == 0) a.meta[r] = RecMeta{0u, 1u, 0u, 0u};
            continue;
        }
        const u32 n_tiles = (len + (u32)TILE_POS - 1u) / (u32)TILE_POS;
        if (tid == 0) s_cnt = 0u, s_nvalid = 0u, s_flag = 0u, s_rows = 0u;
        for (u32 g = (u32)tid; g <= n_tiles * 64u; g += REC_THREADS)
            s_rcodes[g] = g < n_tiles * 64u ? *reinterpret_cast<const u64 *>(region + (u64)(g >> 6) * TWO_BIT_TILE_BYTES + 8u * (g & 63u)) : 0ull;
        __syncthreads();

        // --- hashing: unit u = (tile u / 4, window starts [8 (u % 4), +8) of every lane's 32) ---
        u32 nvalid = 0;
        for (u32 u = (u32)wave; u < n_tiles * (u32)(LANE_POS / REC_UNIT); u += REC_WAVES) {
            const u32 tile = u / (u32)(LANE_POS / REC_UNIT), c = u % (u32)(LANE_POS / REC_UNIT);
            load_tile_two_bit(region, tile, lane, codes_ring, good_ring);
            load_tile_two_bit(region, tile + 1u, lane, codes_ring, good_ring); // (the halo of lane 63; behind the last tile: zeroes)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const u32 par = tile & 1u;
            const uint2 own = *reinterpret_cast<const uint2 *>(&codes_ring[par * 128u + 2u * (u32)lane]);
            const uint2 nbr = *reinterpret_cast<const uint2 *>(&codes_ring[(par * 128u + 2u * (u32)lane + 2u) & 255u]);
            const u32 g_own = good_ring[par * 64u + (u32)lane];
            const u32 g_nbr = good_ring[(par * 64u + (u32)lane + 1u) & 127u];
            const u64 clo = (u64)own.x | ((u64)own.y << 32);
            const u64 chi = (u64)nbr.x | ((u64)nbr.y << 32);
            const u64 g64 = (u64)g_own | ((u64)g_nbr << 32);
            const u32 lane_pos0 = tile * (u32)TILE_POS + (u32)lane * (u32)LANE_POS;
            const u32 limit = len > lane_pos0 ? (len - lane_pos0 < 32u ? len - lane_pos0 : 32u) : 0u;
            const u32 W = window_valid_mask<K>(g64) & (limit >= 32u ? 0xFFFFFFFFu : ((1u << limit) - 1u));
            const u32 Wc = (W >> (c * (u32)REC_UNIT)) & ((1u << REC_UNIT) - 1u);
            nvalid += (u32)__popc(Wc);
            Windows<K> win;
            win.init(clo, chi);
            for (u32 i = 0; i < c; ++i) win.template advance<REC_UNIT>();
#pragma unroll
            for (int j = 0; j < REC_UNIT; ++j) {
                bool is_rc;
                const u64 cm = win.canonical(j, is_rc);
                const u64 h = murmur_h1_fast<K, SEED0>(cm, a.seed, LT);
                const bool v = (Wc >> j) & 1u;
                const u64 mask = __builtin_amdgcn_ballot_w64(v);
                if (mask) { // wave-uniform
                    u32 base = 0;
                    if (lane == 0) base = atomicAdd(&s_cnt, (u32)__popcll(mask));
                    base = (u32)__builtin_amdgcn_readfirstlane((int)base);
                    if (v) { // at most `len` windows are valid (W is cut at the record's end): base + my < REC_MAX_POS
                        const u32 my = base + __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0u));
                        s_keys[my] = h;
                        s_pay[my] = (lane_pos0 + c * (u32)REC_UNIT + (u32)j) | (is_rc ? 0x80000000u : 0u);
                        if (h == EMPTY64) s_flag = 1u;
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier(); // (the next unit's tiles overwrite the ring)
        }
        for (int off = 32; off > 0; off >>= 1) nvalid += __shfl_xor(nvalid, off);
        if (lane == 0 && nvalid) atomicAdd(&s_nvalid, nvalid);
        __syncthreads();

        // --- sort ---
        const u32 n = s_cnt;
        u32 N = 1;
        while (N < n) N <<= 1;
        for (u32 i = n + (u32)tid; i < N; i += REC_THREADS) s_keys[i] = EMPTY64, s_pay[i] = 0u;
        __syncthreads();
        bitonic_lds(s_keys, s_pay, N);

        // --- equal hashes are equal k-mers, or the record is not taken ---
        for (u32 i = 1u + (u32)tid; i < n; i += REC_THREADS)
            if (s_keys[i] == s_keys[i - 1] && record_word<K>(s_rcodes, s_pay[i] & 0x7FFFFFFFu) != record_word<K>(s_rcodes, s_pay[i - 1] & 0x7FFFFFFFu)) s_flag = 1u;
        __syncthreads();
        if (s_flag) {
            if (tid == 0) a.meta[r] = RecMeta{0u, 1u, 0u, 0u};
            continue;
        }

        // --- heads numbered, kept rows written ---
        u32 heads_before = 0; // wave-uniform: heads in front of this pass's entries
        for (u32 i0 = 0; i0 < n; i0 += REC_THREADS) {
            const u32 i = i0 + (u32)tid;
            const bool head = i < n && (i == 0u || s_keys[i] != s_keys[i - 1]);
            const u64 mask = __builtin_amdgcn_ballot_w64(head);
            if (lane == 0) s_wtot[wave] = (u32)__popcll(mask);
            __syncthreads();
            u32 before = 0, total = 0;
            for (int w = 0; w < REC_WAVES; ++w) {
                const u32 t = s_wtot[w];
                before += w < wave ? t : 0u;
                total += t;
            }
            if (head) {
                const u32 rank = heads_before + before + __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0u));
                const u64 h = s_keys[i];
                const bool keep = (u64)rank < a.size || (a.scaled && h <= a.max_hash);
                if (keep) {
                    u32 cnt = 0, extra = 0;
                    for (u32 q = i; q < n && s_keys[q] == h; ++q) cnt++, extra += s_pay[q] >> 31;
                    const size_t row = (size_t)row0 + rank; // rank < min(size [Mash], distinct) <= the record's row bound
                    a.o_hash[row] = h;
                    a.o_kmer[row] = record_word<K>(s_rcodes, s_pay[i] & 0x7FFFFFFFu);
                    a.o_count[row] = cnt;
                    a.o_extra[row] = extra;
                    atomicAdd(&s_rows, 1u);
                }
            }
            heads_before += total;
            __syncthreads();
            if (!a.scaled && (u64)heads_before >= a.size) break; // (wave-uniform) a Mash sketch is complete
        }
        if (tid == 0) a.meta[r] = RecMeta{s_rows, 0u, s_nvalid, 0u};
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// k_record_stream: a record of ANY length (up to STREAM_MAX_POS) in one workgroup, streamed through LDS.
//
// A bottom-n sketch has a threshold that only falls while the record goes by, so the workgroup keeps
//   * a running list L: s_keys[0, nl) ascending distinct hashes with payload LIST | slot, and per slot the position | strand of
//     one occurrence (the k-mer word is re-derived from the staged region: record_word_region), the count and the reverse-strand
//     count, in the half `gen` of the side arrays;
//   * the threshold T: Mash the hash of L[size - 1] once L has `size` entries, 2^64 - 1 before; Scaled max(max_hash, that);
//   * pending window keys s_keys[nl, cnt): (hash, position | strand << 30) of every valid window with hash <= T.
// The record goes by in ROUNDS of one unit (8 window starts per lane) per wave: at most STREAM_ROUND_KEYS keys a round.  Behind
// every round stands a decision point, one barrier for all waves: FOLD if the key array could not take another round (or the
// record is over, or records_stream_fold says so).  A fold sorts list and pending keys together (bitonic_lds), checks equal
// hashes for equal k-mers, sums the runs (a list entry brings its stored counts), cuts (k_record_sketch's rule), and writes
// the kept heads back as the new L -- keys in place (a head's rank is never above its index, and a pass reads before it
// writes), side arrays into the other half (a kept old entry's new rank may be another old entry's slot).
// Not taken: as k_record_sketch, and a Scaled list beyond STREAM_CAP, and a record beyond the handle's bound.
struct StreamArgs {
    RecordArgs r;    // (per_block unused: records are dealt from *next)
    u32 *next;       // the launch's record counter, zero at launch
    u32 max_pos;     // the handle's bound
    u32 fold_min;    // 0: fold only when needed; else also whenever at least this many keys are pending at a decision point
};
constexpr u32 STREAM_CAP = rplan::STREAM_CAP;
constexpr u32 STREAM_KEYS = 8192;                                   // the key array
constexpr u32 STREAM_ROUND_KEYS = REC_WAVES * 64 * REC_UNIT;        // keys that can arrive between two decision points
constexpr u32 PAY_LIST = 0x80000000u, PAY_RC = 0x40000000u, PAY_POS = 0x3FFFFFFFu;
static_assert(STREAM_ROUND_KEYS == 4096, "eight waves, one unit of 8 window starts per lane each");
static_assert(STREAM_CAP + STREAM_ROUND_KEYS <= STREAM_KEYS, "a fold leaves at most STREAM_CAP keys: the next round fits behind them");
static_assert((STREAM_KEYS & (STREAM_KEYS - 1)) == 0, "bitonic_lds sorts a power of two");
static_assert(rplan::STREAM_MAX_POS <= PAY_POS + 1ull, "a window's position in its payload");
static_assert(STREAM_CAP >= 1024, "finch's default is -n 1000");
constexpr size_t STREAM_LDS_BYTES = 2 * 256 * sizeof(Rec4) + 2 * 256 * sizeof(Rec2) + 1024 * sizeof(Rec2) + REC_WAVES * (256 + 128) * 4 +
                                    (size_t)STREAM_KEYS * 12 + 2 * (size_t)STREAM_CAP * 12 + 128;
static_assert(STREAM_LDS_BYTES <= 160 * 1024, "one workgroup's LDS");
static_assert(STREAM_LDS_BYTES + 2 * (size_t)STREAM_CAP * 12 > 160 * 1024, "STREAM_CAP is the largest power of two that fits");

template <int K, bool SEED0>
__global__ __launch_bounds__(REC_THREADS) void k_record_stream(const StreamArgs sa) {
    __shared__ Rec4 sA1[has_pair_word(K, false) ? 256 : 1];
    __shared__ Rec4 sA2[has_pair_word(K, true) ? 256 : 1];
    __shared__ Rec2 sB1[has_pair_word(K, false) ? 256 : 1];
    __shared__ Rec2 sB2[has_pair_word(K, true) ? 256 : 1];
    __shared__ Rec2 sP[partial_entries(K)];
    __shared__ __attribute__((aligned(16))) u32 sCodes[REC_WAVES][256];
    __shared__ __attribute__((aligned(16))) u32 sGood[REC_WAVES][128];
    __shared__ u64 s_keys[STREAM_KEYS];
    __shared__ u32 s_pay[STREAM_KEYS];
    __shared__ u32 s_lpos[2][STREAM_CAP], s_lcnt[2][STREAM_CAP], s_lext[2][STREAM_CAP];
    __shared__ u64 s_T;
    __shared__ u32 s_wtot[REC_WAVES];
    __shared__ u32 s_cnt, s_nl, s_nvalid, s_flag, s_rows, s_rec, s_folds;
    static_assert(partial_entries(K) <= 1024, "STREAM_LDS_BYTES counts 1024 last-word records");

    const RecordArgs &a = sa.r;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (has_pair_word(K, false)) {
        for (int q = tid; q < 256; q += REC_THREADS) {
            sA1[q] = lut_rec_A((u32)q, false);
            sB1[q] = lut_rec_B((u32)q, 4, false);
        }
    }
    if (has_pair_word(K, true)) {
        for (int q = tid; q < 256; q += REC_THREADS) {
            sA2[q] = lut_rec_A((u32)q, true);
            sB2[q] = lut_rec_B((u32)q, 4, true);
        }
    }
    for (int q = tid; q < partial_entries(K); q += REC_THREADS) sP[q] = lut_rec_P<K>((u32)q);
    const LutTables LT{sA1, sA2, sB1, sB2, sP, 0u};
    u32 *const codes_ring = sCodes[wave];
    u32 *const good_ring = sGood[wave];
    const RecDesc *const recs = uniform_ptr(a.recs);

    for (;;) {
        __syncthreads(); // the tables are there; the record before is done with the LDS (s_rec too)
        if (tid == 0) {
            s_rec = atomicAdd(sa.next, 1u); // records are dealt one at a time: they differ in length by orders of magnitude
            s_cnt = 0u, s_nl = 0u, s_nvalid = 0u, s_flag = 0u, s_rows = 0u, s_folds = 0u;
            s_T = EMPTY64;
        }
        __syncthreads();
        const u32 r = (u32)__builtin_amdgcn_readfirstlane((int)s_rec);
        if (r >= a.n_records) break;
        const u32 len = (u32)__builtin_amdgcn_readfirstlane((int)recs[r].len);
        const u32 row0 = (u32)__builtin_amdgcn_readfirstlane((int)recs[r].row0);
        const uint8_t *const region = a.data + recs[r].off;
        if (len > sa.max_pos) {
            if (tid == 0) a.meta[r] = RecMeta{0u, 1u, 0u, 0u};
            continue;
        }
        const u32 n_units = (len + (u32)TILE_POS - 1u) / (u32)TILE_POS * (u32)(LANE_POS / REC_UNIT);
        const u32 n_rounds = (n_units + REC_WAVES - 1u) / REC_WAVES;
        u32 nvalid = 0, gen = 0; // gen: (wave-uniform) the half of the side arrays that holds L
        bool refused = false;

        for (u32 round = 0; round < n_rounds; ++round) {
            // --- hashing: as k_record_sketch, but a window above T is dropped at once (one equal to T is an occurrence to count) ---
            const u64 T = s_T;
            const u32 u = round * REC_WAVES + (u32)wave;
            if (u < n_units) {
                const u32 tile = u / (u32)(LANE_POS / REC_UNIT), c = u % (u32)(LANE_POS / REC_UNIT);
                load_tile_two_bit(region, tile, lane, codes_ring, good_ring);
                load_tile_two_bit(region, tile + 1u, lane, codes_ring, good_ring); // (the halo of lane 63; behind the last tile: zeroes)
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const u32 par = tile & 1u;
                const uint2 own = *reinterpret_cast<const uint2 *>(&codes_ring[par * 128u + 2u * (u32)lane]);
                const uint2 nbr = *reinterpret_cast<const uint2 *>(&codes_ring[(par * 128u + 2u * (u32)lane + 2u) & 255u]);
                const u32 g_own = good_ring[par * 64u + (u32)lane];
                const u32 g_nbr = good_ring[(par * 64u + (u32)lane + 1u) & 127u];
                const u64 clo = (u64)own.x | ((u64)own.y << 32);
                const u64 chi = (u64)nbr.x | ((u64)nbr.y << 32);
                const u64 g64 = (u64)g_own | ((u64)g_nbr << 32);
                const u32 lane_pos0 = tile * (u32)TILE_POS + (u32)lane * (u32)LANE_POS;
                const u32 limit = len > lane_pos0 ? (len - lane_pos0 < 32u ? len - lane_pos0 : 32u) : 0u;
                const u32 W = window_valid_mask<K>(g64) & (limit >= 32u ? 0xFFFFFFFFu : ((1u << limit) - 1u));
                const u32 Wc = (W >> (c * (u32)REC_UNIT)) & ((1u << REC_UNIT) - 1u);
                nvalid += (u32)__popc(Wc); // counted whether they survive or not
                Windows<K> win;
                win.init(clo, chi);
                for (u32 i = 0; i < c; ++i) win.template advance<REC_UNIT>();
#pragma unroll
                for (int j = 0; j < REC_UNIT; ++j) {
                    bool is_rc;
                    const u64 cm = win.canonical(j, is_rc);
                    const u64 h = murmur_h1_fast<K, SEED0>(cm, a.seed, LT);
                    const bool v = ((Wc >> j) & 1u) && h <= T;
                    const u64 mask = __builtin_amdgcn_ballot_w64(v);
                    if (mask) { // wave-uniform
                        u32 base = 0;
                        if (lane == 0) base = atomicAdd(&s_cnt, (u32)__popcll(mask));
                        base = (u32)__builtin_amdgcn_readfirstlane((int)base);
                        if (v) { // the decision point before this round left room for STREAM_ROUND_KEYS keys: base + my < STREAM_KEYS
                            const u32 my = base + __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0u));
                            s_keys[my] = h;
                            s_pay[my] = (lane_pos0 + c * (u32)REC_UNIT + (u32)j) | (is_rc ? PAY_RC : 0u);
                            if (h == EMPTY64) s_flag = 1u;
                        }
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier(); // (the next unit's tiles overwrite the ring)
            }

            // --- the decision point: every wave reads the same count, and nobody appends before all have read it ---
            __syncthreads();
            const u32 n = s_cnt, nl = s_nl;
            __syncthreads();
            const bool last = round + 1u == n_rounds;
            if (!(last || n + STREAM_ROUND_KEYS > STREAM_KEYS || (sa.fold_min && n - nl >= sa.fold_min))) continue;

            // --- the fold: sort L and the pending keys together ---
            u32 N = 1;
            while (N < n) N <<= 1;
            for (u32 i = n + (u32)tid; i < N; i += REC_THREADS) s_keys[i] = EMPTY64, s_pay[i] = 0u;
            __syncthreads();
            bitonic_lds(s_keys, s_pay, N);
            // equal hashes are equal k-mers, or the record is not taken
            for (u32 i = 1u + (u32)tid; i < n; i += REC_THREADS) {
                if (s_keys[i] == s_keys[i - 1]) {
                    const u32 p1 = s_pay[i], p0 = s_pay[i - 1];
                    const u32 q1 = (p1 & PAY_LIST ? s_lpos[gen][p1 & PAY_POS] : p1) & PAY_POS;
                    const u32 q0 = (p0 & PAY_LIST ? s_lpos[gen][p0 & PAY_POS] : p0) & PAY_POS;
                    if (q0 != q1 && record_word_region<K>(region, q1) != record_word_region<K>(region, q0)) s_flag = 1u;
                }
            }
            __syncthreads();
            if (s_flag) {
                refused = true;
                break;
            }
            // heads numbered; the kept ones (a prefix of the heads: both halves of the rule are monotone in the rank) become L
            u32 heads_before = 0; // wave-uniform: heads in front of this pass's entries
            for (u32 i0 = 0; i0 < n; i0 += REC_THREADS) {
                const u32 i = i0 + (u32)tid;
                const bool head = i < n && (i == 0u || s_keys[i] != s_keys[i - 1]);
                const u64 mask = __builtin_amdgcn_ballot_w64(head);
                if (lane == 0) s_wtot[wave] = (u32)__popcll(mask);
                __syncthreads();
                u32 before = 0, total = 0;
                for (int w = 0; w < REC_WAVES; ++w) {
                    const u32 t = s_wtot[w];
                    before += w < wave ? t : 0u;
                    total += t;
                }
                bool keep = false;
                u32 rank = 0, cnt = 0, extra = 0, where = 0;
                u64 h = 0;
                if (head) {
                    rank = heads_before + before + __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0u));
                    h = s_keys[i];
                    keep = (u64)rank < a.size || (a.scaled && h <= a.max_hash);
                    if (keep && rank >= STREAM_CAP) s_flag = 1u, keep = false; // (Scaled only: the constructor holds a Mash size to STREAM_CAP)
                    if (keep) {
                        for (u32 q = i; q < n && s_keys[q] == h; ++q) {
                            const u32 p = s_pay[q];
                            if (p & PAY_LIST) cnt += s_lcnt[gen][p & PAY_POS], extra += s_lext[gen][p & PAY_POS];
                            else cnt++, extra += (p >> 30) & 1u;
                        }
                        const u32 p = s_pay[i];
                        where = p & PAY_LIST ? s_lpos[gen][p & PAY_POS] : p;
                    }
                }
                heads_before += total;
                __syncthreads(); // this pass has read what it needs: its heads' ranks lie at or below their indices
                if (keep) {
                    s_keys[rank] = h;
                    s_pay[rank] = PAY_LIST | rank;
                    s_lpos[gen ^ 1u][rank] = where;
                    s_lcnt[gen ^ 1u][rank] = cnt;
                    s_lext[gen ^ 1u][rank] = extra;
                    atomicAdd(&s_rows, 1u);
                }
                if (!a.scaled && (u64)heads_before >= a.size) break; // (wave-uniform) the list is complete
            }
            __syncthreads();
            if (s_flag) {
                refused = true;
                break;
            }
            gen ^= 1u;
            if (tid == 0) {
                const u32 kept = s_rows;
                const u64 t_size = (u64)kept >= a.size ? (a.size ? s_keys[a.size - 1] : 0ull) : EMPTY64;
                s_T = a.scaled && t_size < a.max_hash ? a.max_hash : t_size;
                s_cnt = kept, s_nl = kept, s_rows = 0u;
                s_folds++;
            }
            __syncthreads();
        }
        if (refused) {
            if (tid == 0) a.meta[r] = RecMeta{0u, 1u, 0u, 0u};
            continue;
        }
        // --- the record is over: L is its sketch ---
        for (int off = 32; off > 0; off >>= 1) nvalid += __shfl_xor(nvalid, off);
        if (lane == 0 && nvalid) atomicAdd(&s_nvalid, nvalid);
        const u32 rows = s_nl;
        for (u32 q = (u32)tid; q < rows; q += REC_THREADS) { // rows <= min(size [Mash], windows, STREAM_CAP): the record's row bound
            const size_t row = (size_t)row0 + q;
            a.o_hash[row] = s_keys[q];
            a.o_kmer[row] = record_word_region<K>(region, s_lpos[gen][q] & PAY_POS);
            a.o_count[row] = s_lcnt[gen][q];
            a.o_extra[row] = s_lext[gen][q];
        }
        __syncthreads();
        if (tid == 0) a.meta[r] = RecMeta{rows, 0u, s_nvalid, s_folds};
    }
}

template <int K>
static hipError_t launch_stream_t(const StreamArgs &a, uint32_t n_blocks, hipStream_t st) {
    if (a.r.seed == 0) hipLaunchKernelGGL((k_record_stream<K, true>), dim3(n_blocks), dim3(REC_THREADS), 0, st, a);
    else hipLaunchKernelGGL((k_record_stream<K, false>), dim3(n_blocks), dim3(REC_THREADS), 0, st, a);
    return hipGetLastError();
}

template <int K>
static hipError_t launch_records_t(const RecordArgs &a, uint32_t n_blocks, hipStream_t st) {
    if (a.seed == 0) hipLaunchKernelGGL((k_record_sketch<K, true>), dim3(n_blocks), dim3(REC_THREADS), 0, st, a);
    else hipLaunchKernelGGL((k_record_sketch<K, false>), dim3(n_blocks), dim3(REC_THREADS), 0, st, a);
    return hipGetLastError();
}

#ifdef FH_ONLY_K // development builds: one K per translation unit
constexpr int PART_LO = FH_ONLY_K, PART_HI = FH_ONLY_K;
#else
constexpr int PART_LO = FH_PART * (32 / FH_NPARTS) + 1;
constexpr int PART_HI = (FH_PART + 1) * (32 / FH_NPARTS);
#endif

template <int K>
static hipError_t launch_records_dispatch(int k, const RecordArgs &a, uint32_t n_blocks, hipStream_t st) {
    if (k == K) return launch_records_t<K>(a, n_blocks, st);
    if constexpr (K > PART_LO) return launch_records_dispatch<K - 1>(k, a, n_blocks, st);
    return hipErrorInvalidValue;
}

hipError_t launch_records_part0(int k, const RecordArgs &a, uint32_t n_blocks, hipStream_t st);
hipError_t launch_records_part1(int k, const RecordArgs &a, uint32_t n_blocks, hipStream_t st);
hipError_t launch_records_part2(int k, const RecordArgs &a, uint32_t n_blocks, hipStream_t st);
hipError_t launch_records_part3(int k, const RecordArgs &a, uint32_t n_blocks, hipStream_t st);

#define FH_CAT2(a, b) a##b
#define FH_CAT(a, b) FH_CAT2(a, b)
hipError_t FH_CAT(launch_records_part, FH_PART)(int k, const RecordArgs &a, uint32_t n_blocks, hipStream_t st) {
    if (k < PART_LO || k > PART_HI) return hipErrorInvalidValue;
    return launch_records_dispatch<PART_HI>(k, a, n_blocks, st);
}

template <int K>
static hipError_t launch_stream_dispatch(int k, const StreamArgs &a, uint32_t n_blocks, hipStream_t st) {
    if (k == K) return launch_stream_t<K>(a, n_blocks, st);
    if constexpr (K > PART_LO) return launch_stream_dispatch<K - 1>(k, a, n_blocks, st);
    return hipErrorInvalidValue;
}
hipError_t launch_stream_part0(int k, const StreamArgs &a, uint32_t n_blocks, hipStream_t st);
hipError_t launch_stream_part1(int k, const StreamArgs &a, uint32_t n_blocks, hipStream_t st);
hipError_t launch_stream_part2(int k, const StreamArgs &a, uint32_t n_blocks, hipStream_t st);
hipError_t launch_stream_part3(int k, const StreamArgs &a, uint32_t n_blocks, hipStream_t st);
hipError_t FH_CAT(launch_stream_part, FH_PART)(int k, const StreamArgs &a, uint32_t n_blocks, hipStream_t st) {
    if (k < PART_LO || k > PART_HI) return hipErrorInvalidValue;
    return launch_stream_dispatch<PART_HI>(k, a, n_blocks, st);
}

} // namespace fh

#if FH_PART == 0
// ------------------------------------------------------------------------------------------------------------------------------
// The host side: the handle and the C ABI.  Per slot (two: the caller fills one while the device works on the other) a pinned
// staging buffer -- the submit's record descriptors, then the records -- and its device twin, and the pinned result: four
// columns of rows_cap rows (fh_records_plan.h: sized by the stage) and a RecMeta per record, which the kernel writes directly.
using namespace fh;
namespace rp = fh::rplan;

#define RHIP_TRY(expr)                                                                                    \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess) return api_fail(FH_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

struct fh_records : rp::Geometry {
    fh_records(const fh_params &params, int dev, uint32_t records, uint64_t stage_bytes, bool streamed, uint32_t fold)
        : rp::Geometry(streamed ? rp::stream_geometry(params, records, stage_bytes) : rp::geometry(params, records, stage_bytes)), p(params),
          max_hash(params.kind == FH_KIND_SCALED ? api_scaled_max_hash(params.scale) : 0), device(dev), max_records(records), stream_form(streamed),
          max_pos(streamed ? rp::STREAM_MAX_POS : rp::MAX_POS), fold_min(fold) {}
    const fh_params p;
    const uint64_t max_hash;
    const int device;
    const uint32_t max_records;
    const bool stream_form;  // fh_records_new_stream: k_record_stream, its bound and its row rule
    const uint32_t max_pos;  // positions of a record the handle's kernel takes
    const uint32_t fold_min; // (stream) the option records_stream_fold
    uint32_t *d_next = nullptr; // (stream) a record counter per slot: the launch deals its records from it
    uint64_t row_bound(uint64_t positions) const {
        if (positions > max_pos) return 0; // (a record beyond the bound is answered "not taken": no rows)
        return stream_form ? rp::stream_row_bound(p.kind, p.size, p.k, positions) : rp::row_bound(p.kind, p.size, p.k, positions);
    }
    uint32_t n_cus = 1;
    hipStream_t stream = nullptr;
    struct Slot {
        uint8_t *h_stage = nullptr, *d_stage = nullptr;
        uint64_t *h_hash = nullptr, *h_kmer = nullptr;
        uint32_t *h_count = nullptr, *h_extra = nullptr;
        RecMeta *h_meta = nullptr;
        hipEvent_t done = nullptr, k0 = nullptr, k1 = nullptr;
        bool in_flight = false, waited = false, launched = false;
        uint32_t n = 0;
        uint64_t positions = 0;
        std::vector<uint32_t> row0;
        std::vector<uint64_t> row0_wide; // (stream) what rplan::stream_assign_rows fills
    } slot[2];
    double prof_ms = 0.0;
    uint64_t prof_launches = 0, prof_positions = 0, n_taken = 0, n_not_taken = 0, n_folds = 0;
};

namespace {

void destroy(fh_records *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    for (auto &s : b->slot) {
        if (s.h_stage) (void)hipHostFree(s.h_stage);
        if (s.d_stage) (void)hipFree(s.d_stage);
        if (s.h_hash) (void)hipHostFree(s.h_hash);
        if (s.h_kmer) (void)hipHostFree(s.h_kmer);
        if (s.h_count) (void)hipHostFree(s.h_count);
        if (s.h_extra) (void)hipHostFree(s.h_extra);
        if (s.h_meta) (void)hipHostFree(s.h_meta);
        if (s.done) (void)hipEventDestroy(s.done);
        if (s.k0) (void)hipEventDestroy(s.k0);
        if (s.k1) (void)hipEventDestroy(s.k1);
    }
    if (b->d_next) (void)hipFree(b->d_next);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
}

int build(fh_records *b) {
    RHIP_TRY(hipSetDevice(b->device));
    int cus = 0;
    RHIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device));
    b->n_cus = (uint32_t)std::max(1, cus);
    RHIP_TRY(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    for (auto &s : b->slot) {
        RHIP_TRY(api_host_malloc((void **)&s.h_stage, b->header_bytes + b->data_bytes + 64));
        RHIP_TRY(api_dev_malloc((void **)&s.d_stage, b->header_bytes + b->data_bytes + 64));
        RHIP_TRY(api_host_malloc((void **)&s.h_hash, b->rows_cap * 8));
        RHIP_TRY(api_host_malloc((void **)&s.h_kmer, b->rows_cap * 8));
        RHIP_TRY(api_host_malloc((void **)&s.h_count, b->rows_cap * 4));
        RHIP_TRY(api_host_malloc((void **)&s.h_extra, b->rows_cap * 4));
        RHIP_TRY(api_host_malloc((void **)&s.h_meta, (size_t)b->max_records * sizeof(RecMeta)));
        RHIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
        RHIP_TRY(hipEventCreate(&s.k0));
        RHIP_TRY(hipEventCreate(&s.k1));
        s.row0.resize(b->max_records);
        if (b->stream_form) s.row0_wide.resize(b->max_records);
    }
    if (b->stream_form) RHIP_TRY(api_dev_malloc((void **)&b->d_next, 2 * 64));
    return FH_OK;
}

// A handle pins tens of MiB, which takes longer than sketching a thousand records: like fh_batch_free, fh_records_free parks an
// idle handle and fh_records_new hands a parked one back when device, sizes and parameters match; fh_release_cached frees them.
std::mutex g_pool_mu;
std::vector<fh_records *> g_pool;
constexpr size_t RECORDS_POOL_MAX = 64;
bool pool_match(const fh_records *c, const fh_params &p, int device, uint32_t max_records, uint64_t stage_bytes, bool stream_form, uint32_t fold_min) {
    return c->stream_form == stream_form && c->fold_min == fold_min && c->device == device && c->max_records == max_records && c->data_bytes == bplan::stage_rounded(stage_bytes) && c->p.kind == p.kind && c->p.k == p.k &&
           c->p.size == p.size && c->p.seed == p.seed && (p.kind != FH_KIND_SCALED || c->p.scale == p.scale);
}

hipError_t launch_records(int k, const RecordArgs &a, uint32_t n_blocks, hipStream_t st) {
    constexpr int per = 32 / FH_NPARTS;
    switch ((k - 1) / per) {
    case 0: return launch_records_part0(k, a, n_blocks, st);
    case 1: return launch_records_part1(k, a, n_blocks, st);
    case 2: return launch_records_part2(k, a, n_blocks, st);
    case 3: return launch_records_part3(k, a, n_blocks, st);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_stream(int k, const StreamArgs &a, uint32_t n_blocks, hipStream_t st) {
    constexpr int per = 32 / FH_NPARTS;
    switch ((k - 1) / per) {
    case 0: return launch_stream_part0(k, a, n_blocks, st);
    case 1: return launch_stream_part1(k, a, n_blocks, st);
    case 2: return launch_stream_part2(k, a, n_blocks, st);
    case 3: return launch_stream_part3(k, a, n_blocks, st);
    }
    return hipErrorInvalidValue;
}

// fh_records_new and fh_records_new_stream behind their checks: a parked handle of the same form, or a new one
fh_records *records_open(const fh_params *params, int device, uint32_t max_records, uint64_t stage_bytes, bool stream_form, uint32_t fold_min) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
        (void)hipGetLastError();
        api_fail(FH_ERR_NO_DEVICE, "no usable HIP device (this library has no CPU path)");
        return nullptr;
    }
    if (device < 0 || device >= n_dev) {
        api_fail(FH_ERR_NO_DEVICE, "device %d out of range (%d visible)", device, n_dev);
        return nullptr;
    }
    {
        std::lock_guard<std::mutex> g(g_pool_mu);
        for (size_t i = 0; i < g_pool.size(); ++i) {
            fh_records *c = g_pool[i];
            if (pool_match(c, *params, device, max_records, stage_bytes, stream_form, fold_min)) {
                g_pool.erase(g_pool.begin() + (long)i);
                return c;
            }
        }
    }
    fh_records *b = nullptr;
    try {
        b = new fh_records(*params, device, max_records, stage_bytes, stream_form, fold_min);
        if (build(b) == FH_OK) return b;
    } catch (...) {
        api_fail(FH_ERR_CAPACITY, "out of host memory");
    }
    destroy(b);
    return nullptr;
}

} // namespace

namespace fh {
void records_release_cached() {
    std::vector<fh_records *> v;
    {
        std::lock_guard<std::mutex> g(g_pool_mu);
        v.swap(g_pool);
    }
    for (fh_records *b : v) destroy(b);
}
} // namespace fh

extern "C" {

uint32_t fh_records_max_positions(void) { return rp::MAX_POS; }

fh_records *fh_records_new(const fh_params *params, int device, uint32_t max_records, uint64_t stage_bytes) {
    if (!params) {
        api_fail(FH_ERR_INVALID, "null params");
        return nullptr;
    }
    const rp::Verdict v = rp::check(params, max_records, stage_bytes);
    if (v.code != FH_OK) {
        api_fail(v.code, "%s", v.msg);
        return nullptr;
    }
    return records_open(params, device, max_records, stage_bytes, false, 0u);
}

uint32_t fh_records_stream_cap(void) { return rp::STREAM_CAP; }
uint32_t fh_records_max_positions_of(fh_records *r) { return r ? r->max_pos : 0; }
uint64_t fh_records_stream_folds(fh_records *r) { return r ? r->n_folds : 0; }

fh_records *fh_records_new_stream(const fh_params *params, int device, uint32_t max_records, uint64_t stage_bytes) {
    if (!params) {
        api_fail(FH_ERR_INVALID, "null params");
        return nullptr;
    }
    const rp::Verdict v = rp::check_stream(params, max_records, stage_bytes);
    if (v.code != FH_OK) {
        api_fail(v.code, "%s", v.msg);
        return nullptr;
    }
    const uint64_t fold = cfg_u64("records_stream_fold", 0);
    return records_open(params, device, max_records, stage_bytes, true, (uint32_t)std::min<uint64_t>(fold, 0xFFFFFFFFull));
}

void fh_records_free(fh_records *r) {
    if (!r) return;
    if (!r->slot[0].in_flight && !r->slot[1].in_flight) {
        std::lock_guard<std::mutex> g(g_pool_mu);
        if (g_pool.size() < RECORDS_POOL_MAX) {
            r->prof_ms = 0.0;
            r->prof_launches = r->prof_positions = r->n_taken = r->n_not_taken = r->n_folds = 0;
            for (auto &s : r->slot) s.waited = false, s.n = 0;
            g_pool.push_back(r);
            return;
        }
    }
    destroy(r);
}

uint64_t fh_records_rows_cap(fh_records *r) { return r ? r->rows_cap : 0; }

int fh_records_stage(fh_records *b, int slot, uint8_t **buf, uint64_t *cap) {
    if (!b || slot < 0 || slot > 1 || !buf || !cap) return api_fail(FH_ERR_INVALID, "bad argument");
    if (b->slot[slot].in_flight) return api_fail(FH_ERR_STATE, "slot %d is in flight: fh_records_wait first", slot);
    *buf = b->slot[slot].h_stage + b->header_bytes;
    *cap = b->data_bytes;
    return FH_OK;
}

int fh_records_submit_packed(fh_records *b, int slot, const uint64_t *offsets, const uint64_t *lens, uint32_t n) {
    if (!b || slot < 0 || slot > 1 || (n && (!offsets || !lens))) return api_fail(FH_ERR_INVALID, "bad argument");
    fh_records::Slot &s = b->slot[slot];
    if (s.in_flight) return api_fail(FH_ERR_STATE, "slot %d is in flight: fh_records_wait first", slot);
    if (n > b->max_records) return api_fail(FH_ERR_INVALID, "%u records in a submit of at most %u", n, b->max_records);
    RHIP_TRY(hipSetDevice(b->device));
    RecDesc *hd = reinterpret_cast<RecDesc *>(s.h_stage);
    uint64_t prev_end = 0, rows = 0, positions = 0;
    for (uint32_t j = 0; j < n; ++j) {
        if (lens[j] > 0xFFFFFFFFull) return api_fail(FH_ERR_INVALID, "record %u: %llu positions", j, (unsigned long long)lens[j]);
        const uint64_t bytes = rp::region_bytes(lens[j]);
        if ((offsets[j] & 63u) || offsets[j] > b->data_bytes || bytes > b->data_bytes - offsets[j])
            return api_fail(FH_ERR_INVALID, "record %u: [%llu, +%llu) is not a 64-byte aligned range of the staging buffer", j, (unsigned long long)offsets[j],
                            (unsigned long long)bytes);
        if (j && offsets[j] < prev_end) return api_fail(FH_ERR_INVALID, "record %u overlaps record %u (offsets ascend)", j, j - 1);
        prev_end = offsets[j] + bytes;
        hd[j].off = offsets[j];
        hd[j].len = (uint32_t)lens[j];
        hd[j].row0 = (uint32_t)rows;
        s.row0[j] = (uint32_t)rows;
        if (!b->stream_form) rows += b->row_bound(lens[j]);
        if (rows > b->rows_cap)
            return api_fail(FH_ERR_CAPACITY, "the rows of records 0..%u exceed the %llu rows of a slot's result: submit fewer records", j, (unsigned long long)b->rows_cap);
        positions += lens[j];
    }
    if (b->stream_form && n) { // the stream form's rows: fh_records_plan.h's rule, the one the host test asks
        uint64_t *const row0 = s.row0_wide.data();
        rows = rp::stream_assign_rows(b->p.kind, b->p.size, b->p.k, lens, n, row0);
        if (rows > b->rows_cap)
            return api_fail(FH_ERR_CAPACITY, "the rows of the %u records exceed the %llu rows of a slot's result: submit fewer records", n, (unsigned long long)b->rows_cap);
        for (uint32_t j = 0; j < n; ++j) hd[j].row0 = s.row0[j] = (uint32_t)row0[j];
    }
    s.n = n;
    s.positions = positions;
    s.waited = false;
    s.launched = false;
    if (n) {
        RHIP_TRY(hipMemcpyAsync(s.d_stage, s.h_stage, b->header_bytes + ((prev_end + 15) & ~15ull), hipMemcpyHostToDevice, b->stream));
        RecordArgs a{};
        a.recs = reinterpret_cast<const RecDesc *>(s.d_stage);
        a.data = s.d_stage + b->header_bytes;
        a.n_records = n;
        const uint32_t blocks = std::min<uint32_t>(n, b->n_cus);
        a.per_block = (n + blocks - 1) / blocks;
        a.seed = b->p.seed;
        a.size = b->p.size;
        a.max_hash = b->max_hash;
        a.scaled = b->p.kind == FH_KIND_SCALED ? 1u : 0u;
        a.o_hash = s.h_hash;
        a.o_kmer = s.h_kmer;
        a.o_count = s.h_count;
        a.o_extra = s.h_extra;
        a.meta = s.h_meta;
        StreamArgs sa{};
        if (b->stream_form) {
            sa.r = a;
            sa.next = b->d_next + 16 * slot;
            sa.max_pos = b->max_pos;
            sa.fold_min = b->fold_min;
            RHIP_TRY(hipMemsetAsync(sa.next, 0, 4, b->stream));
        }
        RHIP_TRY(hipEventRecord(s.k0, b->stream));
        if (b->stream_form) RHIP_TRY(launch_stream((int)b->p.k, sa, blocks, b->stream));
        else RHIP_TRY(launch_records((int)b->p.k, a, (n + a.per_block - 1) / a.per_block, b->stream));
        RHIP_TRY(hipEventRecord(s.k1, b->stream));
        s.launched = true;
    }
    RHIP_TRY(hipEventRecord(s.done, b->stream));
    s.in_flight = true;
    return FH_OK;
}

int fh_records_wait(fh_records *b, int slot, uint8_t *status) {
    if (!b || slot < 0 || slot > 1) return api_fail(FH_ERR_INVALID, "bad argument");
    fh_records::Slot &s = b->slot[slot];
    if (!s.in_flight) return api_fail(FH_ERR_STATE, "slot %d has nothing in flight", slot);
    RHIP_TRY(hipSetDevice(b->device));
    RHIP_TRY(hipEventSynchronize(s.done));
    s.in_flight = false;
    if (!s.waited) {
        s.waited = true;
        if (s.launched) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, s.k0, s.k1) == hipSuccess) {
                b->prof_ms += ms;
                b->prof_launches++;
                b->prof_positions += s.positions;
            } else {
                (void)hipGetLastError();
            }
        }
        for (uint32_t j = 0; j < s.n; ++j) {
            if (s.h_meta[j].status == 0) b->n_taken++, b->n_folds += s.h_meta[j].pad; // (pad: the stream kernel's folds of the record)
            else b->n_not_taken++;
        }
    }
    if (status)
        for (uint32_t j = 0; j < s.n; ++j) status[j] = s.h_meta[j].status ? 1 : 0;
    return FH_OK;
}

static int records_one(fh_records *b, int slot, uint32_t i) {
    if (!b || slot < 0 || slot > 1) return api_fail(FH_ERR_INVALID, "bad argument");
    const fh_records::Slot &s = b->slot[slot];
    if (s.in_flight || !s.waited) return api_fail(FH_ERR_STATE, "slot %d: fh_records_wait first", slot);
    if (i >= s.n) return api_fail(FH_ERR_INVALID, "record %u of a submit of %u", i, s.n);
    if (s.h_meta[i].status != 0) return api_fail(FH_ERR_STATE, "record %u was not taken by the record sketcher", i);
    return FH_OK;
}

int fh_records_result(fh_records *b, int slot, uint32_t i, uint64_t *n_out, uint64_t *total_kmers) {
    if (int rc = records_one(b, slot, i)) return rc;
    if (n_out) *n_out = b->slot[slot].h_meta[i].n_rows;
    if (total_kmers) *total_kmers = b->slot[slot].h_meta[i].total_kmers;
    return FH_OK;
}

int fh_records_copy_out_records(fh_records *b, int slot, uint32_t i, fh_kmer_count *records, uint8_t *kmers) {
    if (int rc = records_one(b, slot, i)) return rc;
    const fh_records::Slot &s = b->slot[slot];
    const size_t n = s.h_meta[i].n_rows, r0 = s.row0[i];
    if (records)
        for (size_t j = 0; j < n; ++j) records[j] = fh_kmer_count{s.h_hash[r0 + j], s.h_count[r0 + j], s.h_extra[r0 + j]};
    if (kmers)
        for (size_t j = 0; j < n; ++j) api_kmer_ascii(s.h_kmer[r0 + j], 0, (int)b->p.k, kmers + j * b->p.k);
    return FH_OK;
}

int fh_records_kernel_time(fh_records *b, double *total_ms, uint64_t *launches, uint64_t *positions) {
    if (!b) return api_fail(FH_ERR_INVALID, "null handle");
    if (total_ms) *total_ms = b->prof_ms;
    if (launches) *launches = b->prof_launches;
    if (positions) *positions = b->prof_positions;
    b->prof_ms = 0.0;
    b->prof_launches = b->prof_positions = 0;
    return FH_OK;
}

int fh_records_counters(fh_records *b, uint64_t *taken, uint64_t *not_taken) {
    if (!b) return api_fail(FH_ERR_INVALID, "null handle");
    if (taken) *taken = b->n_taken;
    if (not_taken) *not_taken = b->n_not_taken;
    return FH_OK;
}

} // extern "C"
#endif // FH_PART == 0
