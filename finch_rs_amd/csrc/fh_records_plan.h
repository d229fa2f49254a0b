// fh_records_plan.h -- the host rules of the record sketcher (fh_records.hip, finch_sketch_records in fh_host.cpp), each written
// once: what a FASTA header says of a record's name and comment, where the records of a text begin and end, which route a
// record takes, the rows a record may need and where a group's records put them, the sizes of a handle and the size it is made
// for.  No HIP and no globals, in the manner of fh_batch_plan.h (whose Verdict it borrows), so that
// tests/hostcore/records_plan_host.cpp runs all of it on the host.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/finch_hip.h"
#include "fh_batch_plan.h"

namespace fh {
namespace rplan {

using bplan::refuse;
using bplan::Verdict;

// --- the record sketcher's own ---
// positions (bytes of the packed stream) of a record one workgroup sketches in its LDS: 8 bytes of key and 4 of payload a
// position, the lookup tables (20 KiB), eight waves' tile rings (12 KiB) and the record's codes (2 KiB) make 130 KiB of the
// 160 KiB a workgroup may have; the next power of two would take 226 KiB.  The compiler agrees (fh_records.hip: static_assert).
constexpr uint32_t MAX_POS = FH_RECORDS_MAX_POS;
constexpr uint32_t MAX_RECORDS = 1u << 20;       // records per submit a handle may be made for
constexpr uint64_t MAX_STAGE = 1ull << 32;       // a slot's staging buffer
constexpr uint64_t ROWS_BUDGET = 1ull << 20;     // rows of a slot's result (24 bytes each, pinned): 24 MiB
constexpr uint64_t DESC_BYTES = 16;              // a record's descriptor in front of the staged records (fh_records.hip: RecDesc)
constexpr uint64_t ROW_BYTES = 24;               // hash | canonical k-mer word | count | extra_count
constexpr uint64_t TILE_POS = 2048, TWO_BIT_TILE = 768; // fh_pack2.h
// finch_sketch_records: a group's staging buffer and its records.  The result binds first -- a thousand 1 500-base records at
// Mash 1000 fill a slot's rows with 0.6 MiB staged -- and a thousand records are four per CU, so a launch is long against its
// own latency; what a larger group would buy is paid in pinned memory per worker (16 workers a GPU): 2 x (8 + 24) MiB each.
constexpr uint64_t GROUP_STAGE = 8ull << 20;
constexpr uint32_t GROUP_RECORDS = 4096;
inline uint64_t pow2_at_least(uint64_t v) {
    uint64_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

// ---------------------------------------------------------------------------------------------------------------------------
// What fh_records_new says to (params, max_records, stage_bytes): the parameters speak before the sizes.
inline Verdict check(const fh_params *p, uint32_t max_records, uint64_t stage_bytes) {
    if (p->kind == FH_KIND_ALL_COUNTS)
        return refuse(FH_ERR_UNSUPPORTED, "the record sketcher serves Mash and Scaled sketches: AllCounts (kind 2) records go through an fh_sketcher");
    if (p->kind != FH_KIND_MASH && p->kind != FH_KIND_SCALED) return refuse(FH_ERR_INVALID, "unknown sketch kind %u (0 Mash, 1 Scaled)", p->kind);
    if (p->k < 1) return refuse(FH_ERR_INVALID, "kmer_length must be at least 1");
    if (p->k > 32) return refuse(FH_ERR_UNSUPPORTED, "the record sketcher serves k = 1..32: k = %u goes through an fh_sketcher", p->k);
    if (p->hash_mask != 0) return refuse(FH_ERR_UNSUPPORTED, "the record sketcher takes no test mask (hash_mask must be 0)");
    if (p->kind == FH_KIND_MASH && p->size < 1) return refuse(FH_ERR_INVALID, "a Mash sketch has at least one hash (size 0)");
    if (p->kind == FH_KIND_SCALED && !bplan::scale_ok(p->scale)) return refuse(FH_ERR_INVALID, "scale must be in (0, 1]");
    if (max_records < 1 || max_records > MAX_RECORDS || stage_bytes < 4096 || stage_bytes > MAX_STAGE)
        return refuse(FH_ERR_INVALID, "max_records 1..%u, stage_bytes 4 KiB..4 GiB", MAX_RECORDS);
    return Verdict{};
}

// ---------------------------------------------------------------------------------------------------------------------------
// Rows.  A record of `positions` has positions - k + 1 windows, and no sketch of it has more rows than windows; a Mash sketch
// has no more than `size` either (a Scaled one may keep every distinct hash: scaled.rs:37-61).
inline uint64_t windows(uint64_t positions, uint32_t k) { return positions >= k ? positions - k + 1 : 0; }
inline uint64_t row_bound(uint32_t kind, uint64_t size, uint32_t k, uint64_t positions) {
    const uint64_t w = windows(positions, k);
    return kind == FH_KIND_MASH ? std::min(size, w) : w;
}
// bytes a record occupies in the staging buffer (fh_pack2::region_bytes: its tiles and the zero tile behind them)
inline uint64_t region_bytes(uint64_t positions) { return ((positions + TILE_POS - 1) / TILE_POS + 1) * TWO_BIT_TILE; }

// The sizes of a handle that passed check().  The result buffer is sized by the stage, not by max_records x size: a record
// of t tiles has at most 2048 t rows and occupies 768 (t + 1) bytes, at best (t = 4, the longest record) 8192 rows in 3840 bytes.
struct Geometry {
    uint64_t header_bytes = 0, data_bytes = 0; // a slot's staging buffer: the record descriptors, then the records
    uint64_t rows_cap = 0;                     // rows of a slot's result: the sum of a submit's row bounds may not exceed it
};
inline Geometry geometry(const fh_params &p, uint32_t max_records, uint64_t stage_bytes) {
    Geometry g;
    g.header_bytes = ((uint64_t)max_records * DESC_BYTES + 4095) & ~4095ull;
    g.data_bytes = bplan::stage_rounded(stage_bytes);
    const uint64_t per_record = p.kind == FH_KIND_MASH ? std::min<uint64_t>(p.size, MAX_POS) : MAX_POS;
    const uint64_t by_stage = g.data_bytes / 3840 * MAX_POS + MAX_POS;
    g.rows_cap = std::max<uint64_t>(MAX_POS, std::min({ROWS_BUDGET, (uint64_t)max_records * per_record, by_stage}));
    return g;
}

// Where the records of a group put their rows: row0[j] = the sum of the row bounds in front of record j; -> the sum of all
inline uint64_t assign_rows(uint32_t kind, uint64_t size, uint32_t k, const uint64_t *positions, uint32_t n, uint64_t *row0) {
    uint64_t sum = 0;
    for (uint32_t j = 0; j < n; ++j) {
        row0[j] = sum;
        sum += row_bound(kind, size, k, positions[j]);
    }
    return sum;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The route of a record: a workgroup's LDS (the device door: Mash and Scaled, k = 1..32, no more than MAX_POS positions), or
// one by one through sketch_stream, which is exact for any parameters.  lds_on: the option records_lds.
enum class Route { Lds, OneByOne };
inline Route route(uint32_t kind, uint32_t k, uint64_t positions, bool lds_on) {
    const bool served = (kind == FH_KIND_MASH || kind == FH_KIND_SCALED) && k >= 1 && k <= 32;
    return lds_on && served && positions <= MAX_POS ? Route::Lds : Route::OneByOne;
}

// The size the handle is made for (bplan::plan_files' group_n): what the small sketcher cuts a Mash sketch to, a Scaled
// sketch's kmers_to_sketch.
inline uint64_t group_n(uint32_t kind, uint64_t kmers_to_sketch, uint64_t final_size) {
    return kind == FH_KIND_SCALED || !(final_size >= 1 && final_size < kmers_to_sketch) ? kmers_to_sketch : final_size;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The STREAMED record sketcher (fh_records_new_stream, k_record_stream of fh_records.hip): a record of any length up to
// STREAM_MAX_POS goes through one workgroup piece by piece; what survives the falling threshold is folded into a running
// sorted list of at most STREAM_CAP distinct hashes in LDS.  Of the 128 KiB the tables and tile rings leave a workgroup, the key
// array takes 96 KiB (8192 keys of 8 + 4 bytes: STREAM_CAP list entries and the 4096 keys eight waves may append between two
// decision points need more than 4096, and the sort wants a power of two) and the list's side arrays 24 KiB (position | strand,
// count and reverse-strand count, 12 bytes an entry, twice: a fold reads the old list while it writes the new one).  An entry
// names its k-mer by a position of the record, not by the k-mer's word: with the word (16 bytes an entry, twice) the list would
// end at 1024 entries with nothing to spare, and the word is read once per kept row.  The compiler agrees (fh_records.hip).
constexpr uint32_t STREAM_CAP = 1024;
// A payload's top bit tells a list entry from a window, the next one is the strand, so a position has 30 bits; the bound is
// lower still: a 16 Mi-position record keeps ONE workgroup busy for tens of milliseconds, by then a sketcher of its own (every
// CU on that record) is the faster route.
constexpr uint32_t STREAM_MAX_POS = 1u << 24;
static_assert(STREAM_MAX_POS <= (1u << 30), "a window's payload: 30 bits of position, the strand, the list flag");

// What fh_records_new_stream says: check()'s rules, then the one of its own.
inline Verdict check_stream(const fh_params *p, uint32_t max_records, uint64_t stage_bytes) {
    const Verdict v = check(p, max_records, stage_bytes);
    if (v.code != FH_OK) return v;
    if (p->kind == FH_KIND_MASH && p->size > STREAM_CAP)
        return refuse(FH_ERR_UNSUPPORTED, "the streamed record sketcher keeps at most %u hashes of a record in LDS: a Mash sketch of %llu goes through an fh_sketcher",
                      STREAM_CAP, (unsigned long long)p->size);
    return Verdict{};
}

// Rows of a record on a stream handle: a Scaled record's kept list is bounded by STREAM_CAP (beyond: not taken)
inline uint64_t stream_row_bound(uint32_t kind, uint64_t size, uint32_t k, uint64_t positions) {
    const uint64_t w = windows(positions, k);
    return kind == FH_KIND_MASH ? std::min(size, w) : std::min<uint64_t>(w, STREAM_CAP);
}
inline uint64_t stream_assign_rows(uint32_t kind, uint64_t size, uint32_t k, const uint64_t *positions, uint32_t n, uint64_t *row0) {
    uint64_t sum = 0;
    for (uint32_t j = 0; j < n; ++j) {
        row0[j] = sum;
        sum += positions[j] > STREAM_MAX_POS ? 0 : stream_row_bound(kind, size, k, positions[j]);
    }
    return sum;
}
// The sizes of a stream handle that passed check_stream(): no record has more than STREAM_CAP rows, whatever the stage holds
inline Geometry stream_geometry(const fh_params &p, uint32_t max_records, uint64_t stage_bytes) {
    Geometry g;
    g.header_bytes = ((uint64_t)max_records * DESC_BYTES + 4095) & ~4095ull;
    g.data_bytes = bplan::stage_rounded(stage_bytes);
    const uint64_t per_record = p.kind == FH_KIND_MASH ? std::min<uint64_t>(p.size, STREAM_CAP) : STREAM_CAP;
    g.rows_cap = std::max<uint64_t>(STREAM_CAP, std::min<uint64_t>(ROWS_BUDGET, (uint64_t)max_records * per_record));
    return g;
}

// finch_sketch_records' stream handles.  Long records are few and large: a 1 Mi-position record occupies 394 KB staged, so
// 8 MiB hold about 20 of them -- fewer than the CUs, so a group of such records never queues two on a workgroup -- while
// 50 kb records (19 968 bytes staged) come 420 to a group, under two per CU.  A group closes at 512 records: beyond that a
// launch only grows longer, and the other slot waits.
constexpr uint64_t STREAM_GROUP_STAGE = 8ull << 20;
constexpr uint32_t STREAM_GROUP_RECORDS = 512;
// records_stream_max_pos when it is not set: the largest measured length at which streaming was not slower than one by one
// (docs/MEASUREMENTS_records_stream.md: ahead at 50 kb and 200 kb, behind at 1 Mb and 5 Mb)
constexpr uint64_t STREAM_DEFAULT_MAX_POS = 200000;

// The route of a record with the streamed sketcher beside the LDS one.  stream_on: the option records_stream; stream_max_pos:
// records_stream_max_pos, capped by STREAM_MAX_POS; group_n: the size the handles are made for.  With stream_on false this is
// route(), name for name.
enum class Route3 { Lds, Stream, OneByOne };
inline Route3 route3(uint32_t kind, uint32_t k, uint64_t positions, bool lds_on, bool stream_on, uint64_t stream_max_pos, uint64_t group_n) {
    if (route(kind, k, positions, lds_on) == Route::Lds) return Route3::Lds;
    const bool served = (kind == FH_KIND_MASH || kind == FH_KIND_SCALED) && k >= 1 && k <= 32;
    const uint64_t bound = std::min<uint64_t>(stream_max_pos, STREAM_MAX_POS);
    const bool fits = kind != FH_KIND_MASH || (group_n >= 1 && group_n <= STREAM_CAP);
    return stream_on && served && fits && positions > MAX_POS && positions <= bound ? Route3::Stream : Route3::OneByOne;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The header rule.  h[0, n): a header line behind its '>' and without its line end.  The name is what stands in front of the
// first blank or tab, the comment what follows that run of blanks and tabs (empty if nothing does).
struct HeaderSplit {
    size_t name_len = 0, comment_off = 0, comment_len = 0;
};
inline HeaderSplit split_header(const uint8_t *h, size_t n) {
    HeaderSplit s;
    size_t i = 0;
    while (i < n && h[i] != ' ' && h[i] != '\t') ++i;
    s.name_len = i;
    while (i < n && (h[i] == ' ' || h[i] == '\t')) ++i;
    s.comment_off = i;
    s.comment_len = n - i;
    return s;
}

// The records of a FASTA text t[0, n), t[0] == '>', by parse_fastx's rules (fh_host.cpp): a record begins at a '>' that
// stands at a line start; its text runs up to the next such '>' or the end; its sequence region begins behind the header's
// line end; seq_length is the region's length (internal line ends count) less one trailing line end (LF, CR LF or CR);
// positions are the region's bytes that are no blank (' ', '\t', '\r', '\n': what the packed stream keeps).
struct Record {
    uint64_t text0 = 0, text1 = 0; // [the record's '>', the next record's)
    uint64_t hdr0 = 0, hdr1 = 0;   // the header line behind the '>', without its line end (a CR in front of it neither)
    uint64_t seq0 = 0;             // the sequence region is [seq0, text1)
    uint64_t seq_length = 0, positions = 0;
};
inline void split_records(const uint8_t *t, size_t n, std::vector<Record> &out) {
    size_t pos = 0;
    while (pos < n) {
        Record r;
        r.text0 = pos;
        r.hdr0 = pos + 1;
        const uint8_t *nl = (const uint8_t *)memchr(t + pos, '\n', n - pos);
        const size_t line_end = nl ? (size_t)(nl - t) : n;
        r.hdr1 = line_end > r.hdr0 && t[line_end - 1] == '\r' ? line_end - 1 : line_end;
        r.seq0 = nl ? line_end + 1 : n;
        size_t next = n;
        for (size_t q = r.seq0; q < n;) {
            const uint8_t *g = (const uint8_t *)memchr(t + q, '>', n - q);
            if (!g) break;
            const size_t at = (size_t)(g - t);
            if (at == r.seq0 || t[at - 1] == '\n') {
                next = at;
                break;
            }
            q = at + 1;
        }
        r.text1 = next;
        const uint64_t len = next - r.seq0;
        uint64_t trim = 0;
        if (len >= 1 && t[next - 1] == '\n') trim = (len >= 2 && t[next - 2] == '\r') ? 2 : 1;
        else if (len >= 1 && t[next - 1] == '\r') trim = 1;
        r.seq_length = len - trim;
        uint64_t blanks = 0;
        for (size_t q = r.seq0; q < next; ++q) blanks += (t[q] == ' ') | (t[q] == '\t') | (t[q] == '\r') | (t[q] == '\n');
        r.positions = len - blanks;
        out.push_back(r);
        pos = next;
    }
}

} // namespace rplan
} // namespace fh
