// fh_index.h -- what fh_host.cpp's finch_index_new / finch_index_search (include/finch_host.h) ask of the device: an inverted index
// over a library's hashes, and a search through it that counts only the (query, reference) pairs that share a hash (DESIGN.md
// §3.14).  Defined in fh_index.hip; no HIP types here, fh_host.cpp is plain C++.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "fh_dist.h"
#include "fh_moments.h"

namespace fh {

// postings an index holds at most: the sort's tiles of 2048 pairs are counted in a u32 (fh_kernels.h: big_sort_pairs)
constexpr uint64_t INDEX_MAX_POSTINGS = 0xffffffffull - 2047;

struct IndexDevice;
// uploads the library to `device`, forms and sorts its postings and allocates, zeroed, the counters of chunk_queries queries.
// refs: at least one hash in all, no more than INDEX_MAX_POSTINGS.  *device_bytes = what the handle keeps allocated; *build_ms =
// the build kernels' time (HIP events).  Synchronous.
int index_open(int device, const DistSide &refs, uint32_t chunk_queries, IndexDevice **out, uint64_t *device_bytes, double *build_ms);
// the queries [q0, q1) of `queries`, q1 - q0 <= chunk_queries: every pair (q, r) with c = |Q n R| > 0 is counted, given its
// (c, i, j) and appended to *entries as 5 u32 (q, r, c, i, j) where c / j >= min_containment, in no order.
// *touched is added the pairs with c > 0, *kernel_ms the kernels' time.  Synchronous; one call at a time per handle.
int index_search_chunk(IndexDevice *d, const DistSide &queries, uint32_t q0, uint32_t q1, double min_containment,
                       std::vector<uint32_t> *entries, uint64_t *touched, double *kernel_ms);
// finch_index_dist's chunk: the queries [q0, q1) of `queries`, or -- queries == nullptr, pairwise -- the library's own sketches
// q0 .. q1, read from the index's copy: no hashes cross.  Counted as above; a touched pair's jaccard is distance_from_counts'
// (new mode from (c, i, j); old_mode: c / (c + 2 (|R| - c))), and the pair is appended as (q, r, c, i, j) -- old mode: i = |R|,
// j = 0 -- where jaccard >= jmin[q - q0] (q1 - q0 doubles: a conservative bound; the caller decides).  The counters are zero
// again afterwards, as after a search.
int index_dist_chunk(IndexDevice *d, const DistSide *queries, uint32_t q0, uint32_t q1, bool old_mode, const double *jmin,
                     std::vector<uint32_t> *entries, uint64_t *touched, double *kernel_ms);
// finch_index_cluster on one handle, between index_cluster_begin and index_cluster_end: a union-find of one
// word per reference on the device, the identity at first, that lives for the one call and through all of its chunks.
//   index_cluster_chunk: the library's own sketches q0 .. q1 as queries, counted and completed as index_dist_chunk's pairwise
//   form does.  Per touched pair: jaccard >= jhi[q - q0] or jaccard == 1: q and r are united on the device (not where q == r)
//   and nothing crosses; jaccard < jlo[q - q0]: dropped; else (q, r, c, i, j) is appended to *entries for the caller's exact
//   test.  The counters are zero again afterwards; the dirty flag as for every chunk.
//   index_cluster_end: labels[0 .. nr) = every reference's root, the smallest index of its tree; *united is added the ordered
//   pairs q != r the device united, *kernel_ms the labels kernel's time; the call's device memory is freed whatever happens.
//   labels == nullptr (the call failed elsewhere): only the freeing, FH_OK.
int index_cluster_begin(IndexDevice *d);
int index_cluster_chunk(IndexDevice *d, uint32_t q0, uint32_t q1, bool old_mode, const double *jlo, const double *jhi,
                        std::vector<uint32_t> *entries, uint64_t *touched, double *kernel_ms);
int index_cluster_end(IndexDevice *d, uint32_t *labels, uint64_t *united, double *kernel_ms);
// finch_index_gather's chunk: the queries [q0, q1) of `queries`, q1 - q0 <= chunk_queries, `counts` parallel to
// queries.hashes.  Counted as above; *cands = the pairs with c >= min_overlap as (q, r, common), sorted by (q, r), q the caller's
// index; then every round of every query in one launch over the live counters: *recs = one record per round, in no order, q the
// caller's index, cand the winner's place among its query's candidates.  Both vectors are overwritten.  The counters are zero
// again afterwards.  *touched is added the pairs with c > 0, *kernel_ms the three kernels' time, *launches 3.  No position
// arrays are built: option gather_pos_bytes does not apply.  FH_ERR_STATE if the rounds kernel's own checks fail (its tail has
// run all the same: the handle stays clean); a failure between the count and the end of the rounds leaves the handle dirty.
int index_gather_chunk(IndexDevice *d, const DistSide &queries, const uint32_t *counts, uint32_t q0, uint32_t q1, uint32_t min_overlap,
                       uint32_t max_rounds, std::vector<GatherCand> *cands, std::vector<GatherRecord> *recs, uint64_t *touched,
                       double *kernel_ms, uint64_t *launches);
// finch_index_attach_counts' share of one handle: the library's `count` column, n = the index's postings u32
// parallel to its CSR of hashes, uploaded to the handle's device; kept until the handle is closed, replaced by the next call.
// *device_bytes = what the attachment holds.  Synchronous.
int index_attach_counts(IndexDevice *d, const uint32_t *counts, uint64_t n, uint64_t *device_bytes);
// frees what index_attach_counts left on the handle, if anything: the handle is as before its first attachment.  Cannot fail.
void index_drop_counts(IndexDevice *d);
// finch_index_compare_counts' chunk: the queries [q0, q1) of `queries`, q1 - q0 <= chunk_queries, `counts` parallel to
// queries.hashes, min_common >= 1.  Counted as above; the selection reads every touched pair's c, stores 0 back -- the counters
// are zero again after the second launch -- and keeps the pairs with c >= min_common; the third launch walks each of them
// (fh_moments.hip: k_index_moments).  *recs = one record per passing pair, in no order, q the caller's index; overwritten.
// *touched is added the pairs with c > 0, *kernel_ms the kernels' time, *launches one per kernel (3; 2 if no pair passes, 1 if
// none is touched).  FH_ERR_STATE without attached counts, and where a walk's `common` is not the index's c (the handle stays
// clean); a failure between the count and the end of the selection leaves the handle dirty.
int index_compare_counts_chunk(IndexDevice *d, const DistSide &queries, const uint32_t *counts, uint32_t q0, uint32_t q1, uint32_t min_common,
                               std::vector<MomentsRecord> *recs, uint64_t *touched, double *kernel_ms, uint64_t *launches);
// finch_index_add / finch_index_keep on one handle, in two phases.  index_add / index_keep build the updated
// library's arrays BESIDE those in use -- peak device memory is old + new -- and leave the handle answering as before; index_commit
// swaps them in and frees the old ones, and cannot fail; index_discard drops them.  A failed build has discarded its own.
// chunk_queries: the counters of the updated library are allocated afresh for it, zeroed, and a dirty handle comes out clean.
// tile: output postings per tile of the update kernels, 1..2048 (option index_update_tile).  *kernel_ms is added the update
// kernels' time (HIP events).  Synchronous; the caller holds the index's lock from the first build to the last commit.
//   index_add: `more`'s sketches become the references nr .. nr + more.n - 1.  Their postings are formed, sorted (stable) and
//   merged into the index's by a tiled merge path; on equal hashes every old reference precedes every new one.  The CSR and the
//   per-reference arrays are extended device to device plus the new part from the host; `counts`, parallel to more.hashes, are
//   appended where counts are attached (required then, ignored otherwise).  The grown library has at most INDEX_MAX_POSTINGS.
//   index_keep: keep[0 .. n_keep) strictly ascending and below nr; the survivors become 0 .. n_keep - 1.  A stable device-wide
//   compaction of the postings (tile counts, their scan, a scatter that renames the references), and a kernel that moves each
//   survivor's hashes (and counts) and gathers its per-reference values.  At least one hash must survive: a library without
//   one has no handle (the caller closes it).
int index_add(IndexDevice *d, const DistSide &more, const uint32_t *counts, uint32_t chunk_queries, uint32_t tile, double *kernel_ms);
int index_keep(IndexDevice *d, const uint32_t *keep, uint32_t n_keep, uint32_t chunk_queries, uint32_t tile, double *kernel_ms);
// -> the device memory the handle keeps allocated, as index_open counts it
uint64_t index_commit(IndexDevice *d);
void index_discard(IndexDevice *d);
void index_close(IndexDevice *d);

} // namespace fh
