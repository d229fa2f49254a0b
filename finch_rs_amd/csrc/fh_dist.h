// fh_dist.h -- what fh_host.cpp's finch_dist (include/finch_host.h) asks of the device: the merge walk of distance.rs:66-126 for
// many (query, reference) pairs at once, reduced to integer counts.  Defined in fh_dist.hip; no HIP types here,
// fh_host.cpp is plain C++.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace fh {

// One side of a call: n sketches in CSR form (hashes[offsets[s] .. offsets[s + 1]) strictly ascending, fewer than 2^32 each),
// and per sketch the scale data of distance.rs:16-29: flags bit 0 = a Scaled sketch, bit 1 = its scale is > 0; scale = the
// f64 the pair's min_scale is chosen by (std::min, as finch_distance has it); max_hash = u64::MAX / ((1 / scale) as u64)
// where bit 1 is set.
struct DistSide {
    const uint64_t *hashes;
    const uint64_t *offsets; // n + 1
    uint32_t n;
    const uint64_t *max_hash;
    const uint32_t *flags;
    const double *scale;
};

constexpr uint32_t DIST_MAX_SLICE = 8192; // query hashes one LDS slice holds at most (64 KiB)

struct DistDevice;
// uploads both sides to `device` once and allocates two result buffers of max_pairs pairs (device + pinned host)
int dist_open(int device, const DistSide &queries, const DistSide &refs, uint32_t slice, uint64_t max_pairs, DistDevice **out);
// async on the handle's stream: the counts of every pair (q, r), r in [r0, r1), into buffer `buf` (0 / 1) and back to the host.
// (r1 - r0) * n_queries <= max_pairs.
int dist_launch(DistDevice *d, int buf, uint32_t r0, uint32_t r1);
// waits for buffer `buf`: *out = 3 u32 per pair at ((r - r0) * n_queries + q) * 3: c = |Q n R|, then i and j of the walk (the
// scale step included); *kernel_ms = the kernel's time (HIP events)
int dist_wait(DistDevice *d, int buf, const uint32_t **out, double *kernel_ms);
void dist_close(DistDevice *d);

// ---- finch_search: the same counts, kept on the device and reduced there ----
constexpr uint32_t SEARCH_TOP_MAX = 64; // top_n the device selects by rounds; 0 or more: every pair that passes goes to the host

// as dist_open, for search_launch / search_wait (dist_close closes it): per buffer the counts (device only) and what the selection
// leaves of them -- top mode (1 <= top_n <= SEARCH_TOP_MAX): top_n entries per query; all mode: up to max_pairs entries
int search_open(int device, const DistSide &queries, const DistSide &refs, uint32_t slice, uint64_t max_pairs, uint32_t top_n,
                double min_containment, DistDevice **out);
// async on the handle's stream: the counts of every pair (q, r), r in [r0, r1), r0 < r1, then per query the selection among those
// with c / j >= min_containment (0 where j = 0), ordered by c / j descending, then r ascending
int search_launch(DistDevice *d, int buf, uint32_t r0, uint32_t r1);
// waits for buffer `buf`.  Top mode: *entries = n_queries x top_n slots of 4 u32 (r, c, i, j), the first (*per_query)[q] of query
// q's slots filled, in order; *n = the slots copied.  All mode: *per_query = nullptr, *entries = *n entries of 5 u32
// (q, r, c, i, j), every pair that passed, in no order.  Valid until the buffer's next launch.
int search_wait(DistDevice *d, int buf, const uint32_t **entries, const uint32_t **per_query, uint64_t *n, double *kernel_ms);

// ---- finch_gather: greedy decomposition of each query over the library (fh_gather.hip) ----
// The counting pass is the search's: the query-major instantiation of the distance kernel, launched by fh_dist.hip over arrays
// that fh_gather.hip owns.  All pointers are device memory; `stream` is a hipStream_t.  With every flag 0 the kernel reads no
// scale and no max_hash, and c of its (c, i, j) is |Q n R| over the hashes as stored, which is all the gather takes from it.
struct DistDeviceArrays {
    const uint64_t *qh, *qoff, *rh, *roff;
    const uint32_t *qflag, *rflag; // nq / nr zeros
    uint32_t nq, slice;            // slice: 1 .. DIST_MAX_SLICE, no more than the longest query (at least 1)
};
// async on `stream`: the counts of every pair (q, r), r in [r0, r1), r0 < r1, to out[(q * (r1 - r0) + (r - r0)) * 3 ..]
int dist_counts_query_major(const DistDeviceArrays &a, uint32_t r0, uint32_t r1, uint32_t *out, void *stream);

constexpr uint32_t GATHER_MAX_QUERY = 1u << 20; // hashes of a query: one bit each in the rounds kernel's LDS mask (128 KiB)
constexpr uint32_t GATHER_MAX_SLICE = 4096;     // query hashes one LDS slice of the positions kernel holds at most (32 KiB)

// one side of a gather call in CSR form, as DistSide; counts (the queries' only) run parallel to hashes
struct GatherSide {
    const uint64_t *hashes;
    const uint32_t *counts;
    const uint64_t *offsets; // n + 1
    uint32_t n;
};
struct GatherCand { // a pair with common = |Q n R| >= min_overlap
    uint32_t q, r, common;
};
struct GatherRecord { // one round of one query, as k_gather_rounds writes it: 48 bytes
    uint32_t q, r, round, overlap, common, ref_len, query_len, remaining;
    uint64_t abund;
    uint32_t cand, pad; // the winner's place among the query's candidates
};

struct GatherDevice;
// uploads both sides to `device` once; the counting pass takes at most max_pairs pairs per launch
int gather_open(int device, const GatherSide &queries, const GatherSide &refs, uint32_t dist_slice, uint32_t gather_slice, uint64_t max_pairs,
                uint32_t min_overlap, GatherDevice **out);
// the counting pass over the references [r0, r1) and every query: the pairs with common >= min_overlap, appended to *out in no
// order (the cursor crosses to the host, then that many entries); *kernel_ms and *launches are added to
int gather_count(GatherDevice *d, uint32_t r0, uint32_t r1, std::vector<GatherCand> *out, double *kernel_ms, uint64_t *launches);
// positions and rounds for the queries [q0, q1): cands = their candidates sorted by (q, r), n of them; the records of every
// round of every one of those queries, appended to *out in no order (the cursor crosses, then that many records)
int gather_rounds(GatherDevice *d, uint32_t q0, uint32_t q1, const GatherCand *cands, uint64_t n, uint32_t max_rounds,
                  std::vector<GatherRecord> *out, double *kernel_ms, uint64_t *launches);
void gather_close(GatherDevice *d);

} // namespace fh
