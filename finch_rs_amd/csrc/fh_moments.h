// fh_moments.h -- what fh_host.cpp's finch_compare_counts (include/finch_host.h) asks of the device: Sketch.compare_counts
// (lib/src/python.rs:496-559) for many (query, reference) pairs at once -- the integers of the merge walk, the summed counts of
// the shared hashes and the moment recurrence over them, in hash order.  Defined in fh_moments.hip; no HIP
// types here, fh_host.cpp is plain C++.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace fh {

// One side of a call: n sketches in CSR form, hashes[offsets[s] .. offsets[s + 1]) strictly ascending with their counts, fewer
// than 2^32 - 1 entries each.
struct MomentsSide {
    const uint64_t *hashes;
    const uint32_t *counts;
    const uint64_t *offsets; // n + 1
    uint32_t n;
};

// What the device appends for a pair that passes common >= min_common: 64 bytes.  m2, m3, m4 are the recurrence's sums after
// the last shared hash; the host divides (var, skew, kurt).
struct MomentsRecord {
    uint32_t q, r, common, ref_pos, query_pos, pad;
    uint64_t ref_count, query_count;
    double m2, m3, m4;
};
static_assert(sizeof(MomentsRecord) == 64, "the device's record");

constexpr uint32_t MOMENTS_MAX_SLICE = 4096; // query entries (u64 hash + u32 count) one LDS slice holds at most (48 KiB)

struct MomentsDevice;
// checks both sides' offsets, uploads them to `device` once and allocates two record lists of max_pairs records (device) with
// their cursors; a launch asks for an LDS slice of min(slice, MOMENTS_MAX_SLICE, the longest query) entries
int moments_open(int device, const MomentsSide &queries, const MomentsSide &refs, uint32_t slice, uint64_t max_pairs, uint32_t min_common,
                 MomentsDevice **out);
// async on the handle's stream: every pair (q, r), r in [r0, r1), r0 < r1 <= the references opened, into buffer `buf` (0 / 1);
// (r1 - r0) * n_queries <= max_pairs, so the list cannot overflow
int moments_launch(MomentsDevice *d, int buf, uint32_t r0, uint32_t r1);
// waits for buffer `buf`: *records = the *n records of the pairs that passed, in no order (valid until the buffer's next
// launch); *kernel_ms = the kernel's time (HIP events)
int moments_wait(MomentsDevice *d, int buf, const MomentsRecord **records, uint64_t *n, double *kernel_ms);
void moments_close(MomentsDevice *d);

// finch_index_compare_counts' moment walk: k_index_moments, launched by fh_index.hip over arrays the index
// owns.  A pair that passed the index's selection: q is the caller's index, c the index's |Q n R| (> 0: neither side is empty).
struct IndexPass {
    uint32_t q, r, c;
};
// All pointers are device memory.  The chunk's queries as the index's kernels have them: hashes and counts from qbase on,
// qoff[0 .. nq] as the whole call has them, q0 the chunk's first query; the library's CSR with the attached counts.
struct IndexMomentsArgs {
    const uint64_t *qh, *qoff;
    const uint32_t *qc;
    uint64_t qbase;
    uint32_t q0, nq;
    const uint64_t *rh, *roff;
    const uint32_t *rc;
    uint32_t nr;
    const IndexPass *pass; // n_pass pairs ...
    uint32_t n_pass;
    MomentsRecord *rec;    // ... and the record of pair p at rec[p]
    uint32_t *err;         // three words, zero before the launch: set; q and r of a pair whose walk is not what its entry says
};
// async on `stream` (a hipStream_t): one wave per pair walks the shorter side, 64 entries a step, and searches the longer one
int index_moments_launch(const IndexMomentsArgs &a, void *stream);

} // namespace fh
