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
