/*
 * finch_host.h -- host-side mirror of finch's library entry points for the accelerated path, exported
 * by libfinch_hip.so next to the device ABI (finch_hip.h).  C++ implementation (the reference is
 * compiled code; no Rust toolchain in this image), C linkage so that any host language can bind it.
 *
 * Reference items mirrored (relative to the finch-rs tree):
 *   finch_sketch_files      finch::sketch_files        lib/src/lib.rs:29-49   (one Sketch per file, input order;
 *                                                       rayon par_iter over files -> worker threads, each with its
 *                                                       own device sketcher; files are mapped round-robin to GPUs)
 *   finch_sketch_buffer     finch::sketch_stream       lib/src/lib.rs:51-94   (in-memory FASTA/FASTQ[.gz] image)
 *   FASTX reading           needletail 0.5.0 parse_fastx_reader (lib.rs:60-68): gz / bz2 / xz sniffed by magic bytes,
 *                           '>' FASTA (multi-line), '@' FASTQ (4-line records)
 *   filtering               FilterParams::filter_counts lib/src/filtering.rs:60-87 (strand -> err -> abundance)
 *   post filter             SketchParams::process_post_filter lib/src/sketch_schemes/mod.rs:115-128
 *   .sk writer              MultiSketch / JsonSketch   lib/src/serialization/json.rs:64-89,141-158,199-218
 *
 * The per-base work (normalize, canonical k-mers, murmur3, bottom-n) is done by the device engine; this
 * layer parses, stages, filters (O(n) on <= n records) and serialises.
 */
#ifndef FINCH_HOST_H
#define FINCH_HOST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* SketchParams (mod.rs:54-71); all three kinds are sketched on the device (AllCounts: k = 1..16, FH_KIND_ALL_COUNTS) */
typedef struct finch_sketch_params {
    uint32_t kind;            /* 0 = Mash, 1 = Scaled, 2 = AllCounts (kmer_length only; seq_length is 0, as counts.rs reports it) */
    uint32_t kmer_length;
    uint64_t kmers_to_sketch;
    uint64_t final_size;      /* Mash only */
    uint32_t no_strict;       /* Mash only */
    uint32_t pad;
    uint64_t hash_seed;
    double scale;             /* Scaled only */
} finch_sketch_params;

/* FilterParams (filtering.rs:11-16) */
typedef struct finch_filter_params {
    int32_t filter_on;        /* -1 = None, 0 = Some(false), 1 = Some(true) */
    uint32_t has_abun_lo, abun_lo;
    uint32_t has_abun_hi, abun_hi;
    uint32_t pad;
    double err_filter;
    double strand_filter;
} finch_filter_params;

/* Vec<Sketch> (serialization/mod.rs:46-55) */
typedef struct finch_sketches finch_sketches;

const char *finch_last_error(void);

/* SketchParams::default() (mod.rs:73-83) and FilterParams::default() (filtering.rs:136-145) */
void finch_default_sketch_params(finch_sketch_params *out);
void finch_default_filter_params(finch_filter_params *out);

/* sketch_files: `devices` lists the HIP devices to use (NULL/0 = device 0); n_threads = worker threads
 * (0 = one per hardware thread the process may use, at least 4 and at most 16 per device).  "-" reads stdin.  Returns 0 or a negative FH_ERR_* code (message via
 * finch_last_error; the first failing file wins, as in the reference's collect()). */
int finch_sketch_files(const char *const *filenames, uint32_t n_files, const finch_sketch_params *sketch_params,
                       const finch_filter_params *filters, const int *devices, uint32_t n_devices, uint32_t n_threads,
                       finch_sketches **out);
/* ONE SKETCH PER RECORD of FASTA inputs (mash sketch -i, sourmash --singleton): `out` holds one sketch per record of every
 * input, in file order and then record order.  Let text_j be the bytes of record j as they stand in the decompressed input,
 * from the record's '>' up to, not including, the '>' that begins the next header line (a '>' at a line start), or to the end
 * of input.  Sketch j is, field for field, what finch_sketch_buffer(text_j, len_j, name_j, sketch_params, filters with
 * filter_on = 0, ...) returns -- hashes, k-mer bytes, counts, extra_counts, seq_length (internal line ends count, one trailing
 * line end is trimmed), num_valid_kmers, sketch_params, filter_params, the Mash cut to final_size and the strict error
 * "<name> had too few kmers (<n>) to sketch" unless no_strict -- except that name_j is the header up to its first blank or tab,
 * without the '>', and the comment is the rest of the header line behind that run of blanks and tabs, without the line end
 * (empty if there is none).  A header without sequence is a record of no bases.  The first failing record wins.
 * Any parameters are accepted and the result is always exact: records the record sketcher serves (include/finch_hip.h,
 * fh_records_new: Mash and Scaled, kmer_length <= 32, at most FH_RECORDS_MAX_POS positions) are sketched many per launch in a
 * workgroup's LDS; every other record -- kmer_length 33..64, AllCounts, longer records, all of them with the option
 * records_lds=0 -- and every record the device reports as not taken goes one by one through its own sketcher.
 * Input: whatever the host reader opens (plain, gzip, BGZF, bz2, xz, "-" for stdin); each input is held decompressed in host
 * memory while the call runs.  devices: at most 16 entries (an entry may repeat; NULL / 0 = device 0); n_threads workers
 * (0 = finch_sketch_files' rule), worker w on device w mod n_devices.
 * Refused before any device is touched: FH_ERR_INVALID for a null argument or more than 16 device entries;
 * FH_ERR_UNSUPPORTED for filters->filter_on == 1 (filtering a single record's sketch is not offered; -1 and 0 mean off) and
 * for an input whose first byte is '@' (one sketch per read is not offered; the message names the file); an empty input is
 * the error finch_sketch_files gives for it.
 * finch_sketch_records_stats: the last call of the calling thread -- its records, how many were sketched in LDS and how many
 * one by one (in_lds + one_by_one == records), the record kernel's event-measured milliseconds and its launches (any pointer
 * may be NULL).
 * With the option records_stream = 1 (default 0) a record of more than FH_RECORDS_MAX_POS and no more than
 * records_stream_max_pos positions goes through the streamed record sketcher (fh_records_new_stream: Mash up to
 * fh_records_stream_cap() hashes, Scaled, kmer_length <= 32) instead of one by one; such records count in in_lds, and
 * kernel_ms / launches cover both kernels.  finch_sketch_records_stream_stats: the streamed records of the calling thread's last
 * call, the streamed kernel's milliseconds and its launches. */
int finch_sketch_records(const char *const *filenames, uint32_t n_files, const finch_sketch_params *sketch_params,
                         const finch_filter_params *filters, const int *devices, uint32_t n_devices, uint32_t n_threads,
                         finch_sketches **out);
int finch_sketch_records_buffer(const uint8_t *data, uint64_t len, const finch_sketch_params *sketch_params,
                                const finch_filter_params *filters, const int *devices, uint32_t n_devices, uint32_t n_threads,
                                finch_sketches **out);
int finch_sketch_records_stats(uint64_t *records, uint64_t *in_lds, uint64_t *one_by_one, double *kernel_ms, uint64_t *launches);
int finch_sketch_records_stream_stats(uint64_t *streamed, double *kernel_ms, uint64_t *launches);
/* sketch_stream over an in-memory file image */
int finch_sketch_buffer(const uint8_t *data, uint64_t len, const char *name, const finch_sketch_params *sketch_params,
                        const finch_filter_params *filters, int device, finch_sketches **out);
/* ONE input across several devices (north_star; beyond the reference, which parallelises over files only,
 * lib.rs:34-36): a reader cuts the decompressed FASTQ / FASTA text into record- (FASTQ) or line-aligned (FASTA) chunks of
 * about `chunk_bytes` (0 = 32 MiB) and deals them round-robin to one sketcher per entry of `devices` (an entry may
 * repeat: several handles on one GPU); every handle splits and sketches its chunks on its device at the chunks' own
 * stream offsets, FASTA records that span a cut hand their last k-1 bases over as a halo; the partial sketches are
 * merged on the host (fh_merge), then filters / post filter as in sketch_stream.  The result is the Sketch
 * finch_sketch_files returns for the same file.  FASTQ the device-side splitter refuses (not plain 4-line FASTQ: blank
 * lines between records, a record longer than a chunk, ...) is read again through ONE handle and the host parser, which is
 * the judge of what needletail accepts (stdin, which cannot be read twice: FH_ERR_INVALID).  AllCounts (kind 2):
 * FH_ERR_UNSUPPORTED -- finch_sketch_files / finch_sketch_buffer sketch it. */
int finch_sketch_file_sharded(const char *filename, const finch_sketch_params *sketch_params, const finch_filter_params *filters,
                              const int *devices, uint32_t n_devices, uint64_t chunk_bytes, finch_sketches **out);
int finch_sketch_buffer_sharded(const uint8_t *data, uint64_t len, const char *name, const finch_sketch_params *sketch_params,
                                const finch_filter_params *filters, const int *devices, uint32_t n_devices, uint64_t chunk_bytes,
                                finch_sketches **out);
/* The tail of sketch_stream (lib.rs:70-93) for a caller that fed a sketcher of include/finch_hip.h itself: fh_finish, to_vec,
 * filter_counts, process_post_filter -> one Sketch.  format: 1 FASTA, 2 FASTQ (the filtering default, lib.rs:70-76). */
struct fh_sketcher;
int finch_sketch_from_sketcher(struct fh_sketcher *h, const char *name, uint64_t seq_length, int format,
                               const finch_sketch_params *sketch_params, const finch_filter_params *filters, finch_sketches **out);
void finch_sketches_free(finch_sketches *s);

uint32_t finch_sketches_len(const finch_sketches *s);
const char *finch_sketch_name(const finch_sketches *s, uint32_t i);
uint64_t finch_sketch_seq_length(const finch_sketches *s, uint32_t i);
uint64_t finch_sketch_num_valid_kmers(const finch_sketches *s, uint32_t i);
uint64_t finch_sketch_n_hashes(const finch_sketches *s, uint32_t i);
/* the (possibly updated) filter params of sketch i (lib.rs:70-76, filtering.rs:69-80) */
int finch_sketch_filter_params(const finch_sketches *s, uint32_t i, finch_filter_params *out);
/* hashes ascending; kmers = n*k ASCII bytes; any pointer may be NULL */
int finch_sketch_copy(const finch_sketches *s, uint32_t i, uint64_t *hashes, uint32_t *counts, uint32_t *extra_counts,
                      uint8_t *kmers);

/* MultiSketch::from_sketches + serde_json::to_string (the `.sk` format).  *out is malloc'ed; free with
 * finch_free_string. */
int finch_sketches_to_json(const finch_sketches *s, char **out, uint64_t *len);
void finch_free_string(char *p);

/* ---- the other sketch file formats (lib/src/serialization/) ----
 * .bsk = write_finch_file / read_finch_file (mod.rs:123-222, schema finch.capnp), .msh = write_mash_file / read_mash_file
 * (mash.rs:12-135, schema mash.capnp): Cap'n Proto messages in the standard unpacked stream framing, as the reference's
 * capnp::serialize::write_message emits them.  The writers produce single-segment messages (at most 4 GiB; beyond that
 * FH_ERR_UNSUPPORTED); the readers take any valid message, the reference's multi-segment files included.  *out is
 * malloc'ed: finch_free_bytes. */
int finch_sketches_to_bsk(const finch_sketches *s, uint8_t **out, uint64_t *len);
int finch_sketches_to_msh(const finch_sketches *s, uint8_t **out, uint64_t *len);
void finch_free_bytes(uint8_t *p);
int finch_sketches_from_bsk(const uint8_t *data, uint64_t len, finch_sketches **out);
int finch_sketches_from_msh(const uint8_t *data, uint64_t len, finch_sketches **out);
/* MultiSketch::to_sketches over serde_json::from_slice (json.rs:92-139, 160-262; filtering.rs:110-134): the `.sk` reader */
int finch_sketches_from_json(const uint8_t *data, uint64_t len, finch_sketches **out);
/* open_sketch_file (lib.rs:96-118): *.msh / *.bsk / *.sk, *.json by file name */
int finch_open_sketch_file(const char *path, finch_sketches **out);
/* the `sketch` subcommand's output step (cli/src/main.rs:53-70): format by file name */
int finch_write_sketch_file(const finch_sketches *s, const char *path);
/* SketchParams of sketch i; kind 2 = AllCounts */
int finch_sketch_params_of(const finch_sketches *s, uint32_t i, finch_sketch_params *out);
const char *finch_sketch_comment(const finch_sketches *s, uint32_t i);
int finch_sketch_set_comment(finch_sketches *s, uint32_t i, const char *comment);
/* dst.extend(src): the CLI collects the sketches of all its inputs before it writes one file (main.rs:60-70) */
int finch_sketches_append(finch_sketches *dst, const finch_sketches *src);
/* FilterParams::filter_sketch (filtering.rs:20-54) exactly as the reference has it: sketch i's filter parameters take
 * the stricter of their own and `filters`' values; its hashes are left alone (the reference drops the filtered list). */
int finch_filter_sketch(finch_sketches *s, uint32_t i, const finch_filter_params *filters);

/* distance (lib/src/distance.rs:9-47): compares sketch ia of `a` (query) with sketch ib of `b` (reference).
 * raw_distance (distance.rs:66-126) unless old_mode (old_distance, distance.rs:136-157). */
typedef struct finch_distance_out {
    double containment, jaccard, mash_distance;
    uint64_t common_hashes, total_hashes;
} finch_distance_out;
int finch_distance(const finch_sketches *a, uint32_t ia, const finch_sketches *b, uint32_t ib, int old_mode,
                   finch_distance_out *out);
/* raw_distance on bare ascending hash arrays */
int finch_raw_distance(const uint64_t *query, uint64_t nq, const uint64_t *ref, uint64_t nr, double scale,
                       finch_distance_out *out);

/* finch dist (cli/src/main.rs:85-125, calc_sketch_distances main.rs:315-333): every (query, reference) pair in the
 * reference's loop order -- for each reference, for each query --, skipping a pair whose two sketches are equal field by
 * field (Sketch's derived PartialEq), keeping the rows with mash_distance <= max_distance.  Each row is bit for bit what
 * finch_distance(queries, q, refs, r, old_mode) returns.  The set intersections run on the devices (reference ranges dealt
 * round-robin over `devices`, NULL/0 = device 0; an entry may repeat, at most 16 entries).  FH_ERR_INVALID for a null
 * argument, a sketch whose hashes are not strictly ascending (named in finch_last_error) and, in old_mode, an empty query
 * next to a non-empty reference (finch_distance's error; no rows); FH_ERR_NO_DEVICE without a usable device. */
typedef struct finch_dist_result finch_dist_result;
int finch_dist(const finch_sketches *queries, const finch_sketches *refs, int old_mode, double max_distance, const int *devices,
               uint32_t n_devices, finch_dist_result **out);
uint64_t finch_dist_len(const finch_dist_result *r);
/* row i: query index, reference index, the distance; any pointer may be NULL */
int finch_dist_copy(const finch_dist_result *r, uint32_t *query_idx, uint32_t *ref_idx, finch_distance_out *rows);
/* serde_json::to_writer(&Vec<SketchDistance>) (main.rs:117-121); *out is malloc'ed: finch_free_string */
int finch_dist_to_json(const finch_dist_result *r, char **out, uint64_t *len);
/* measurement: the kernels' time (HIP events, summed over the launches of every device entry) and the launch count */
int finch_dist_stats(const finch_dist_result *r, double *kernel_ms, uint64_t *launches);
void finch_dist_free(finch_dist_result *r);
/* the sketches idx[0..n) of s, in that order (the `--queries` selection of main.rs:97-108) */
int finch_sketches_select(const finch_sketches *s, const uint32_t *idx, uint32_t n, finch_sketches **out);

/* minmer_matrix (lib/src/distance.rs:345-364; behind Sketch.compare_matrix and Sketch.counts, python.rs:561-583): sketch ir
 * of `refs` (R hashes) against the S sketches of `sketches`.  out is the row-major S x R matrix: out[i * R + p] = the count
 * sketch i holds for the reference's p-th hash (the u32's bits as i32: a count >= 2^31 comes out negative), 0 where sketch
 * i does not have that hash.  Every cell is written.  `refs` and `sketches` may be the same handle.  The lookups run on the
 * devices: rows dealt in chunks round-robin over `devices` (as finch_dist: NULL/0 = device 0, an entry may repeat, at most
 * 16 entries); kernel_ms / launches (either may be NULL) receive the kernels' time (HIP events, summed) and the launch
 * count.  Decided before any device is touched: FH_ERR_INVALID for a null argument (out may be NULL only with out_len 0),
 * ir out of range, the reference sketch or any sketch of `sketches` not strictly ascending or of 2^32 hashes or more (named
 * in finch_last_error), an empty reference sketch next to a non-empty sketch (the reference indexes ref[0] and panics),
 * out_len != S * R; FH_OK without a device for a matrix of zero cells.  Otherwise FH_ERR_NO_DEVICE without a usable device.
 * The caller's current device is the same after the call. */
int finch_minmer_matrix(const finch_sketches *refs, uint32_t ir, const finch_sketches *sketches, const int *devices,
                        uint32_t n_devices, int32_t *out, uint64_t out_len, double *kernel_ms, uint64_t *launches);

/* search (Multisketch.best_match and filter_to_matches, lib/src/python.rs:202-234: a loop of distance(query, sketch, false)
 * over a library, judged by containment): for every query the references it looks like, best first.
 *   Which rows: the rows of query q are the references r whose finch_distance(queries, q, refs, r, 0) containment is
 *     >= min_containment.  A NaN threshold gives no rows (nothing is >= NaN); any threshold <= 0 keeps every pair.  No pair is
 *     skipped -- best_match has no self-skip, so a query that is in the library matches itself -- and there is no old_mode.
 *   Order: by containment descending, among equal containments (equal as doubles) by reference index ascending; only the
 *     first top_n of a query are returned when top_n > 0, all of them when top_n = 0.  Rows are grouped by query, in query
 *     order; finch_search_offsets gives the CSR over them (row range of query q: offsets[q] .. offsets[q + 1]).
 *   Row values: every row is bit for bit what finch_distance returns for that pair, mash_distance included: the host makes the
 *     doubles from the device's integer counts, as finch_dist does; the device's own doubles only decide the selection.
 *   Where it runs: the counts are those of finch_dist (reference ranges dealt round-robin over `devices`, NULL/0 = device 0,
 *     an entry may repeat, at most 16 entries; options dist_slice and dist_chunk_pairs apply), but they stay in device memory:
 *     per launch the device picks each query's best top_n (1 <= top_n <= 64) or appends every pair that passes the threshold
 *     to one list (top_n = 0 or > 64), and only those candidates cross to the host, which merges the launches.
 *   Decided before any device is touched: FH_ERR_INVALID for a null argument, more than 16 device entries, a sketch whose
 *     hashes are not strictly ascending (named in finch_last_error, as finch_dist names it); a sketch of 2^32 - 1 hashes or
 *     more is refused as finch_dist refuses it; zero queries or zero references: FH_OK, no rows, no device needed.  Otherwise
 *     FH_ERR_NO_DEVICE without a usable device.  The caller's current device is the same after the call.
 * finch_search_stats: the kernels' time (HIP events, summed over the launches of every device entry), the launches, and
 * candidates_copied = the candidate entries that crossed from device to host, summed over the launches (top_n slots per query
 * and launch for 1 <= top_n <= 64, else exactly the pairs that passed the threshold); any pointer may be NULL. */
typedef struct finch_search_result finch_search_result;
int finch_search(const finch_sketches *queries, const finch_sketches *refs, double min_containment, uint32_t top_n,
                 const int *devices, uint32_t n_devices, finch_search_result **out);
uint64_t finch_search_len(const finch_search_result *r);
int finch_search_offsets(const finch_search_result *r, uint64_t *offsets /* n_queries + 1 */);
/* row i: query index, reference index, the distance; any pointer may be NULL */
int finch_search_copy(const finch_search_result *r, uint32_t *query_idx, uint32_t *ref_idx, finch_distance_out *rows);
int finch_search_stats(const finch_search_result *r, double *kernel_ms, uint64_t *launches, uint64_t *candidates_copied);
void finch_search_free(finch_search_result *r);

/* index: finch_search through an inverted index of the library's hashes, built once per library.  finch_search counts every
 * (query, reference) pair; a row with containment > 0 needs a shared hash, and an index enumerates exactly the pairs that have
 * one.  THE CONTRACT: for min_containment > 0, finch_index_search(ix, queries, min_containment, top_n) returns byte for byte
 * what finch_search(queries, refs, min_containment, top_n, ...) returns for the library the index was built from -- offsets,
 * indices, rows, their order, the top_n cut.  The result is a finch_search_result: finch_search_len / _offsets / _copy / _stats /
 * _free work on it unchanged (launches = the launches of chunks of queries; candidates_copied = exactly the pairs that passed the
 * threshold, whatever top_n is: there is no device-side top-n here).
 * finch_index_new: the index of `refs` on every entry of `devices` (NULL/0 = device 0, an entry may repeat, at most 16); each
 *   entry holds the library's hashes as finch_search uploads them, per reference its length, last hash, scale and max hash, the
 *   postings (hash, reference) sorted by hash -- equal hashes in ascending reference order, duplicates kept --, and the launch
 *   state: per query of a launch one u32 counter and one u32 of touched list per reference (option index_chunk_queries: queries
 *   per launch, read here; default: as many as keep that state within 256 MiB, at most 4096, at least 1).  The index is
 *   self-contained: `refs` may be freed.  Decided before any device is touched: FH_ERR_INVALID for a null argument, more than
 *   16 device entries, a reference whose hashes are not strictly ascending (named in finch_last_error, as finch_search names
 *   it); FH_ERR_UNSUPPORTED for a library of more than 2^32 - 2048 postings (hashes of all its sketches; the message has both
 *   numbers; option index_max_postings lowers the bound); a library without a single hash: FH_OK, no device needed.  Otherwise
 *   FH_ERR_NO_DEVICE without a usable device.
 * finch_index_search: queries are dealt over the index's device entries in chunks of index_chunk_queries.  Per launch the device
 *   counts c = |Q n R| for the pairs that share a hash, completes (c, i, j) as finch_dist defines them and appends the pairs with
 *   c / j >= min_containment to a list; the host finishes as finch_search does.  Decided before any device is touched:
 *   FH_ERR_INVALID for a null argument, min_containment <= 0 (an index cannot enumerate pairs that share nothing: use
 *   finch_search), a query whose hashes are not strictly ascending (named); zero queries, or an index of a library without a
 *   hash: FH_OK, no rows, no device needed.  A NaN threshold selects nothing.  One search at a time runs on an index (others
 *   wait).  FH_ERR_STATE for every search after one that failed between its two kernels: the index must be built again.
 * finch_index_stats: references, postings, the device memory one build left allocated summed over the entries, the build
 *   kernels' time (HIP events, summed); any pointer may be NULL.
 * finch_index_search_stats: pairs_touched = the (query, reference) pairs the device counted, i.e. those with c > 0.
 *   FH_ERR_INVALID, *pairs_touched untouched, for a result that finch_index_search did not make.
 * The caller's current device is the same after each of these calls. */
typedef struct finch_index finch_index;
int finch_index_new(const finch_sketches *refs, const int *devices, uint32_t n_devices, finch_index **out);
int finch_index_search(const finch_index *ix, const finch_sketches *queries, double min_containment, uint32_t top_n,
                       finch_search_result **out);
int finch_index_stats(const finch_index *ix, uint64_t *n_refs, uint64_t *postings, uint64_t *device_bytes, double *build_kernel_ms);
int finch_index_search_stats(const finch_search_result *r, uint64_t *pairs_touched);
void finch_index_free(finch_index *ix);

/* finch dist through the index: `finch dist -d D` over a library, pairwise included, at a cost that follows the pairs that share
 * a hash.  THE CONTRACT: for max_distance < 1, finch_index_dist(ix, refs, queries, old_mode, max_distance) returns byte for byte
 * what finch_dist(queries, refs, old_mode, max_distance, ...) returns -- queries == NULL (pairwise): what finch_dist(refs, refs,
 * ...) returns --: the rows, the query and reference indices, the reference-major order with queries ascending inside a
 * reference, and the self-skip (equal names and Sketch::eq, decided by the function finch_dist uses).  The result is a
 * finch_dist_result: finch_dist_len / _copy / _to_json / _stats / _free work on it unchanged (kernel_ms: the count and finish
 * kernels; launches: the launches of chunks of queries).
 *   Why max_distance < 1: two non-empty sketches that share no hash have jaccard 0 and mash_distance exactly 1, so a bound below
 *   1 drops them, and the pairs that share a hash are what the index enumerates.  A bound >= 1 (+inf included) keeps every pair:
 *   FH_ERR_INVALID, use finch_dist.  NaN or max_distance < 0: FH_OK, no rows (-0.0 is not < 0: it keeps the distance-0 rows).
 *   Pairs that share no hash and are kept all the same have total_hashes 0, jaccard 1 (old mode: 0 / 0) and distance 0, and at
 *   least one empty side.  New mode: both sides empty, or one side empty and the other with no hash below the pair's max hash (a
 *   Mash sketch beside it: no max hash, so always).  Old mode: every pair whose reference is empty.  The host makes these pairs
 *   itself -- every empty sketch of either side against all sketches of the other, c = 0 and the cursors by bound searches, then
 *   the same distance function and the same `<= max_distance` --: O(empty x other side), nothing for a library without empty
 *   sketches.  Every pair of two non-empty sketches goes through the index.
 *   `refs` MUST be the library `ix` was built from: the index keeps no sketches, and names, kmer_length, the self-skip and the
 *   rows come from `refs`.  The call refuses (FH_ERR_INVALID) a `refs` whose sketch count or total hash count differs from the
 *   index's; the rest of that promise is the caller's.
 *   The device completes each touched pair's counts (old mode: total = |R|) and its jaccard -- the host's division, bit for bit
 *   -- and sends (q, r, c, i, j) where jaccard >= jmin[q] = x / (2 - x) * (1 - 2^-20), x = exp(-kmer_length(q) * max_distance):
 *   a conservative pre-filter; the host decides each entry with distance_from_counts.  Pairwise, the queries are read from the
 *   index's own copy of the library: 8 bytes per query cross to the device.
 *   Decided before any device is touched: FH_ERR_INVALID for a null ix, refs or out, max_distance >= 1, the refs mismatch, a
 *   sketch whose hashes are not strictly ascending (named, as finch_dist names it), old mode with an empty query next to a
 *   non-empty reference (as finch_dist); zero queries: no rows; an index of a library without a hash: every row is host-made,
 *   no device needed.  One call at a time runs on an index, searches included.  FH_ERR_STATE as for finch_index_search.
 * finch_index_dist_stats: pairs_touched = the pairs the device counted (c > 0), pairs_copied = the entries that passed the
 *   pre-filter and crossed; either pointer may be NULL.  FH_ERR_INVALID, outputs untouched, for a result finch_dist made. */
int finch_index_dist(const finch_index *ix, const finch_sketches *refs, const finch_sketches *queries /* NULL = pairwise */,
                     int old_mode, double max_distance, finch_dist_result **out);
int finch_index_dist_stats(const finch_dist_result *r, uint64_t *pairs_touched, uint64_t *pairs_copied);

/* single-linkage clusters of a library: what follows `finch dist --pairwise -d D` in a dereplication, and what finch_index_keep
 * ends one with.  Not in the reference; the contract is this comment (tests/index_cluster_model.py states it in Python).
 *   Edges.  For an ordered pair (q, r) of library sketches, q != r, let (c, i, j) be the counts finch_dist makes for query q and
 *     reference r.  The pair PASSES when distance_from_counts(old_mode, c, old_mode ? |r| : i, j, kmer_length of q) gives
 *     mash_distance <= max_distance: finch_dist's function and comparison.  a and b are LINKED when (a, b) or (b, a) passes --
 *     both orders count: old mode is not symmetric, and kmer_length is the query's.  No name-based self-skip: two entries with
 *     equal names and content are linked like any pair at distance 0.  For a library of distinct names the ordered pairs that pass
 *     are exactly the rows of a finch_dist call of the library against itself with the same mode and bound.
 *   Result.  labels[v] = the smallest index of v's connected component: deterministic, whatever happens in whatever order on
 *     the device.
 * finch_cluster_host: the contract as written, on the host: every ordered pair through finch_dist's own counting and distance
 *   functions -- O(R^2) merge walks --, then a union-find; no device.  *edges (may be NULL) = the ordered pairs q != r that pass.
 *   Any bound: NaN or max_distance < 0 links nothing (labels[v] = v), a bound >= 1 links everything.  FH_ERR_INVALID for a null
 *   argument, n_labels other than the library's size, hashes that do not ascend strictly, old mode with an empty sketch next to a
 *   non-empty one (pairwise makes it a query).
 * finch_index_cluster: the same labels through the index, and stats->edges == finch_cluster_host's edges.  The device counts the
 *   pairs that share a hash as finch_index_dist's pairwise form does, completes each one's jaccard -- the host's division, bit for
 *   bit -- and sorts it by two bounds per query, x = exp(-kmer_length(q) * max_distance), m = option index_cluster_margin:
 *     jaccard >= jhi[q] = x / (2 - x) * (1 + m), or jaccard == 1 (distance exactly 0 at every k): SURE -- q and r are united on
 *       the device, in a lock-free union-find of one word per reference, and nothing crosses (where jhi is no normal positive
 *       number it is +inf: only jaccard 1 is sure);
 *     jaccard < jlo[q] = x / (2 - x) * (1 - 2^-20), finch_index_dist's jmin: DROPPED;
 *     between: (q, r, c, i, j) crosses and the host decides with distance_from_counts, as finch_index_dist does.
 *   Each device entry ends with a label per reference (4 bytes each cross); the host merges them with the band's kept pairs and
 *   with the pairs that have an empty side, which it makes itself exactly as finch_index_dist does.
 *   Refusals and trivial cases, as finch_index_dist's: max_distance >= 1: FH_ERR_INVALID (every pair is within such a bound: the
 *   library is one cluster); NaN or max_distance < 0: FH_OK, labels[v] = v, no device touched (-0.0 is 0); FH_ERR_INVALID for a
 *   `refs` that is not the library of the index (sketch count and total hash count are checked), hashes that do not ascend
 *   strictly, old mode with an empty sketch next to a non-empty one (before any launch), n_labels other than the library's size,
 *   option index_cluster_margin outside [2^-20, 0.5] (default 2^-20; nothing sweeps the bands' soundness below it; tests use 0.25
 *   so that most pairs cross).  An index of a library without a hash has no device entries: the whole call runs on the host.
 *   One call at a time runs on an index; FH_ERR_STATE as for finch_index_search.  labels[] is unspecified after a failure.
 *   stats (may be NULL): kernel_ms = the count, finish and labels kernels; launches = the launches of chunks of queries;
 *   pairs_touched as in finch_index_dist_stats; pairs_united = ordered pairs q != r the device decided by itself; pairs_copied =
 *   entries that crossed; pairs_kept_host = of those, the ones with q != r the exact test kept; edges = pairs_united +
 *   pairs_kept_host + the host-made empty-side pairs that pass; clusters = distinct labels. */
typedef struct {
    double kernel_ms;
    uint64_t launches, pairs_touched, pairs_united, pairs_copied, pairs_kept_host, edges, clusters;
} finch_cluster_stats;
int finch_index_cluster(const finch_index *ix, const finch_sketches *refs, int old_mode, double max_distance, uint32_t *labels,
                        uint64_t n_labels, finch_cluster_stats *stats /* may be NULL */);
int finch_cluster_host(const finch_sketches *refs, int old_mode, double max_distance, uint32_t *labels, uint64_t n_labels,
                       uint64_t *edges /* may be NULL */);

/* screen: which references of a library are IN a set of raw reads, and how deep -- the question `mash screen` answers.  Every
 * other library call takes a sketch as the query; a bottom-1000 sketch of a metagenome shares next to nothing with any single
 * member genome.  A screen does not sketch the sample: it hashes EVERY k-mer of it and looks each hash up among the library's.
 * Not in the reference; the contract is this comment (tests/screen_model.py states it in Python).  Integers only:
 *   The inputs are read as ONE sample.  For every record of every input, every window of kmer_length consecutive bases counts:
 *     ACGT, acgt and U/u are bases, any other byte breaks k-mers (blanks and line ends inside a record's sequence are dropped
 *     first, as everywhere in this library); no window spans two records.  The window's hash is hash_f(canonical k-mer,
 *     hash_seed), as the sketchers compute it (mash.rs:73-79, hashing.rs:10-12).  mult(h) = the number of windows whose hash is
 *     h -- the `count` a Mash sketcher holds for h when kmers_to_sketch is at least the sample's distinct k-mers.  Two k-mers
 *     with one 64-bit hash count together, as in the reference's sketchers, which key by hash.
 *   Per reference r:  ref_len = r's hashes;  shared = r's hashes h with mult(h) > 0;  sum_mult = the sum of mult(h) over those;
 *     median_mult = with their multiplicities sorted ascending m[0 .. shared), m[(shared - 1) / 2]: the lower median, no
 *     averaging;  containment = (double)shared / (double)ref_len, one IEEE division on the host.  Plain set semantics over the
 *     hashes as stored: a Scaled reference is judged on the hashes it holds.  (mash screen's identity is
 *     pow(containment, 1. / kmer_length); it is not part of a row.)
 *   The result holds one row per reference with shared >= max(1, min_shared), in reference order.
 * finch_screen_host: the contract as written, on the host with a hash map; `data` is the image of one input, container
 *   included (plain, gzip, BGZF, bz2, xz; FASTA or FASTQ); no device.
 * finch_index_screen / finch_index_screen_buffer: the same rows through the index.  Every container finch_sketch_files reads is
 *   accepted, "-" is stdin.  The host packs the records into the two-bit form (one not-a-base position behind every record)
 *   and stages pieces of at most `screen_piece` positions (option; default 16 M, at least one tile of 2048) through two slots; a
 *   record longer than a piece continues in the next one with its last kmer_length - 1 positions repeated in front, so that no
 *   window is lost and none counts twice.  On the device, per call: a table of the library's DISTINCT hashes made from the
 *   index's current postings (a screen after finch_index_add / finch_index_keep sees the updated library) with a zeroed u64
 *   multiplicity each and a directory of 2^b buckets over them (option screen_dir_bits, 1..28, default ceil(log2 distinct)) keyed by
 *   the b bits from the highest set bit of the largest hash down; k_screen hashes every window of a piece (the sketch kernels'
 *   own arithmetic) and adds 1 to the multiplicity of a hash it finds; a finish kernel, one wave per reference, makes shared,
 *   sum_mult and the exact median (a bit-by-bit search over the reference's multiplicities: no sort, no bound on ref_len).
 *   Only three arrays of one value per reference cross to the host.  Everything the call allocates is freed when it ends.
 *   The call holds the index's lock for its whole length (finch_index_add / finch_index_keep wait), runs on the index's FIRST
 *   device entry (dealing pieces over several entries is not offered) and neither uses nor changes the index's own counters.
 *   n_threads is what the decompressors may use (0: as finch_sketch_files decides).
 *   THE EMPTY CASES.  A library without a hash, n_files == 0 or len == 0: nothing is read and no device is touched; the result
 *   has no rows and EVERY figure of finch_screen_stats is 0 (positions and distinct too).  finch_screen_host does the same
 *   for a library without a hash or len == 0.  The index is as it was.
 *   FH_ERR_INVALID: a null argument, kmer_length 0 or above 64, a file that cannot be opened, an input that is no FASTA/FASTQ.
 *   FH_ERR_UNSUPPORTED: kmer_length 33..64 ("the screen serves kmer_length <= 32").
 * finch_screen_stats (any pointer may be NULL): positions = sequence positions of the sample (breakers and repeated positions
 *   not counted); kmers = valid windows; hits = windows whose hash is a library hash (= the sum of all mult); distinct = the
 *   library's distinct hashes; table_bytes / table_ms = the per-call table (distinct hashes, multiplicities, directory) and the
 *   kernels that build it -- what caching it across calls would save; kernel_ms = k_screen's launches and the finish kernel;
 *   launches = k_screen's launches.  After finch_screen_host: table_bytes, table_ms, kernel_ms, launches are 0. */
typedef struct finch_screen_row {
    uint32_t reference, shared, ref_len, reserved;
    uint64_t median_mult, sum_mult;
    double containment;
} finch_screen_row;
typedef struct finch_screen_result finch_screen_result;
int finch_index_screen(const finch_index *ix, const char *const *filenames, uint32_t n_files, uint32_t kmer_length, uint64_t hash_seed,
                       uint32_t min_shared, uint32_t n_threads, finch_screen_result **out);
int finch_index_screen_buffer(const finch_index *ix, const uint8_t *data, uint64_t len, uint32_t kmer_length, uint64_t hash_seed,
                              uint32_t min_shared, uint32_t n_threads, finch_screen_result **out);
int finch_screen_host(const finch_sketches *refs, const uint8_t *data, uint64_t len, uint32_t kmer_length, uint64_t hash_seed,
                      uint32_t min_shared, finch_screen_result **out);
uint64_t finch_screen_len(const finch_screen_result *r);
int finch_screen_copy(const finch_screen_result *r, finch_screen_row *rows);
int finch_screen_stats(const finch_screen_result *r, uint64_t *positions, uint64_t *kmers, uint64_t *hits, uint64_t *distinct,
                       uint64_t *table_bytes, double *table_ms, double *kernel_ms, uint64_t *launches);
void finch_screen_free(finch_screen_result *r);

/* gather: the greedy decomposition of a query sketch over a library -- what follows a search whose best-first list is full of
 * near-duplicates.  Not in the reference; the contract is this comment (tests/gather_model.py states it twice in Python).
 *   gather(Q, refs, min_overlap, max_rounds) for one query sketch Q and the library refs[0 .. R):
 *     min_overlap below 1 is taken as 1 (a reference that shares nothing explains nothing); max_rounds = 0 means no cap.
 *     S_0 = the set of Q's hashes.  PLAIN SET SEMANTICS over the hashes as stored: no max_hash cut, no early stop of a merge
 *     walk -- deliberately not raw_distance's walk (distance.rs:66-126); callers compare like with like.
 *     Round t = 0, 1, ...: c_j(t) = |S_t n H_j| for every reference j; the winner w has the largest c_j(t), among equal counts
 *     the smallest j.  Stop if c_w(t) < min_overlap, or if t == max_rounds and max_rounds > 0.  Otherwise one row, and
 *     S_{t+1} = S_t \ H_w.  c_j(t) never grows with t and a chosen reference has c = 0 afterwards, so a query has at most as
 *     many rows as it has references with c_j(0) >= min_overlap.
 *   Row integers: query, reference = w, round = t, overlap = c_w(t), common = c_w(0), ref_len = |H_w|, query_len = |Q|,
 *     abund = the u64 sum of Q's `count` over S_t n H_w, remaining = |S_{t+1}|.
 *   Row doubles, made on the host by one function for both entry points, plain IEEE divisions of the integers as doubles,
 *     nothing guarded: f_unique_to_query = overlap / query_len, f_orig_query = common / query_len, f_match = common / ref_len,
 *     average_abund = abund / overlap, f_unique_weighted = abund / (the u64 sum of all of Q's counts).
 *   Rows of a query are in round order; queries are independent.
 * finch_gather_query: query iq of `queries` on the host, the loop as written above: up to `cap` rows into rows[] (NULL with cap
 *   0), *n = the rows the query has (never more than the library has sketches).  Any hash lists that ascend strictly.
 *   FH_ERR_INVALID for a null argument, an index out of range, hashes that do not ascend strictly.
 * finch_gather: every query, on the devices; rows grouped by query in query order, finch_gather_offsets gives the CSR over them
 *   as finch_search_offsets does.  Every field of every row is bit for bit what finch_gather_query gives (two NaNs count as
 *   equal).  Queries are dealt round-robin over `devices` (as finch_dist: NULL/0 = device 0, an entry may repeat, at most 16
 *   entries).  Per device entry: the counting pass of finch_search over reference chunks (options dist_slice and
 *   dist_chunk_pairs apply), whose counts stay on the device -- only the pairs with c_j(0) >= min_overlap cross, as a list --,
 *   then per chunk of queries the positions of every candidate's shared hashes in its query (option gather_slice: query hashes
 *   per LDS slice) and all rounds of every query in one launch; a chunk's position arrays hold at most gather_pos_bytes bytes
 *   (default 1 GiB; 4 bytes per shared hash of a candidate).  Down the link go the candidate list and the rows, nothing else.
 *   Decided before any device is touched: FH_ERR_INVALID for a null argument, more than 16 device entries, a sketch whose hashes
 *   are not strictly ascending (named in finch_last_error, as finch_dist names it); a sketch of 2^32 - 1 hashes or more is
 *   refused as finch_dist refuses it; FH_ERR_UNSUPPORTED for a query of more than 1 048 576 hashes (named, with the limit: one
 *   bit per query hash in the rounds kernel's 128 KiB of LDS); zero queries or zero references: FH_OK, no rows, no device
 *   needed.  Otherwise FH_ERR_NO_DEVICE without a usable device.  After the counting pass: FH_ERR_UNSUPPORTED for a query whose
 *   positions alone exceed gather_pos_bytes (named, with the bytes it needs).  FH_ERR_STATE, never a wrong row, if the device's
 *   positions disagree with its counts.  The caller's current device is the same after the call.
 * finch_gather_stats: the kernels' time (HIP events, summed over the launches of every device entry), the kernel launches,
 * candidates = the pairs with c_j(0) >= min_overlap (exactly the list entries that crossed to the host), records_copied = the
 * records that crossed: exactly the rows; any pointer may be NULL. */
typedef struct finch_gather_row {
    uint64_t query, reference, round, overlap, common, ref_len, query_len, abund, remaining;
    double f_unique_to_query, f_orig_query, f_match, average_abund, f_unique_weighted;
} finch_gather_row;
int finch_gather_query(const finch_sketches *refs, const finch_sketches *queries, uint32_t iq, uint64_t min_overlap, uint64_t max_rounds,
                       finch_gather_row *rows, uint64_t cap, uint64_t *n);
typedef struct finch_gather_result finch_gather_result;
int finch_gather(const finch_sketches *queries, const finch_sketches *refs, uint64_t min_overlap, uint64_t max_rounds, const int *devices,
                 uint32_t n_devices, finch_gather_result **out);
uint64_t finch_gather_len(const finch_gather_result *r);
int finch_gather_offsets(const finch_gather_result *r, uint64_t *offsets /* n_queries + 1 */);
/* row i: query index, reference index, the row; any pointer may be NULL */
int finch_gather_copy(const finch_gather_result *r, uint32_t *query_idx, uint32_t *ref_idx, finch_gather_row *rows);
int finch_gather_stats(const finch_gather_result *r, double *kernel_ms, uint64_t *launches, uint64_t *candidates, uint64_t *records_copied);
void finch_gather_free(finch_gather_result *r);

/* gather through the index: the same decomposition at a cost that follows the pairs that share a hash.  THE CONTRACT:
 * finch_index_gather(ix, queries, min_overlap, max_rounds) returns byte for byte what finch_gather(queries, refs, min_overlap,
 * max_rounds, ...) returns for the library the index was built from -- offsets, the rows in their order, every integer and every
 * double the same bits (two NaNs count as equal).  The gather's own contract is the comment above, unchanged: min_overlap below 1 is
 * 1, max_rounds = 0 is no cap, ties go to the lower reference index; finch_gather_query is the judge.  The result is a
 * finch_gather_result, read with finch_gather_len / _offsets / _copy / _stats and freed with finch_gather_free.
 *   No `refs`: a row needs only ref_len of the library, which the index holds.  No threshold is refused: a candidate shares at
 *   least one hash, and the index enumerates every pair that does.
 *   The device, per chunk of index_chunk_queries queries (dealt over the index's device entries as finch_index_search deals
 *   them), three launches: finch_index_search's count, which leaves |Q n H_r| in the query's counter of every reference r that
 *   shares a hash; the candidates (counter >= min_overlap), the counters left as they are; and every round of every query of the
 *   chunk, one workgroup per query: the winner is an arg-max over the candidates' counters -- nothing is recounted --, and each
 *   hash the winner removes from the query lowers the counter of every reference that holds it, so that every counter is the
 *   reference's count against what is left.  All rounds together lower no more counters than the count raised.  No position arrays
 *   are built: the options gather_slice and gather_pos_bytes do not apply, and no query is refused for its candidates' positions.
 *   FH_ERR_INVALID for a null argument, a query whose hashes are not strictly ascending (named); FH_ERR_UNSUPPORTED for a sketch of
 *   2^32 - 1 hashes or more and for a query of more than 2^20 = 1 048 576 hashes (named, with the limit: the remaining set is a
 *   bitmask in the rounds kernel's LDS, as in finch_gather) -- all before any device is touched.  Zero queries, or an index of a
 *   library without a hash: FH_OK, no rows, no device needed.  One call at a time runs on an index, searches included (others
 *   wait).  FH_ERR_STATE, never a wrong row, if the rounds kernel's own checks fail (a counter lowered below 0; a round that
 *   removed another number of hashes than its winner's counter said; a winner whose counter is not 0 after its round), and for
 *   every call after one that failed between its kernels: the index must be built again.  The caller's current device is the same
 *   after the call.
 * finch_gather_stats on the result: candidates = exactly the pairs with c_j(0) >= min_overlap, records_copied = exactly the rows,
 *   launches = three per chunk of queries, kernel_ms = their time.
 * finch_index_gather_stats: pairs_touched = the (query, reference) pairs the device counted, i.e. those that share a hash.
 *   FH_ERR_INVALID, *pairs_touched untouched, for a result that finch_gather made. */
int finch_index_gather(const finch_index *ix, const finch_sketches *queries, uint64_t min_overlap, uint64_t max_rounds,
                       finch_gather_result **out);
int finch_index_gather_stats(const finch_gather_result *r, uint64_t *pairs_touched);

/* compare_counts (Sketch.compare_counts, lib/src/python.rs:496-559): the merge walk of a reference sketch and a query sketch
 * that also sums the abundances of the shared hashes and runs the one-pass recurrence for the higher moments of the query's
 * abundances over them.  The eight values are the reference's tuple, in its order:
 *   common = |Q n R|; ref_pos / query_pos = where the walk stopped on each side (#{r <= max Q}, #{q <= max R}; both 0 if either
 *   sketch is empty); ref_count / query_count = the summed `count` of the shared hashes on each side (u64); var = m2 / common,
 *   skew = sqrt(common) * m3 / pow(m2, 1.5), kurt = common * m4 / (m2 * m2) - 3, where m2, m3, m4 come from the recurrence of
 *   python.rs:524-535 run over the shared hashes in ascending hash order, in IEEE doubles without fused multiply-adds.
 *   common = 0, common = 1 or all shared counts equal give NaNs, as the reference does: that is the contract, not an error.
 * finch_compare_counts_pair: one pair on the host, the reference's loop as written (any input the reference's loop takes).
 * FH_ERR_INVALID for a null argument or an index out of range.
 * finch_compare_counts: every (query, reference) pair with common >= min_common (0 keeps every pair), on the devices: one row
 *   per pair, ordered by query index, then by reference index ascending; every value of a row is bit for bit what
 *   finch_compare_counts_pair returns for that pair (two NaNs count as equal).  The integers and m2, m3, m4 are made on the device
 *   -- the recurrence included, in hash order --, the three finishing doubles on the host, by the function the pair call uses.
 *   Reference ranges are dealt round-robin over `devices` (as finch_dist: NULL/0 = device 0, an entry may repeat, at most 16
 *   entries; options cmpc_slice and cmpc_chunk_pairs apply); per launch only the pairs that pass cross to the host.
 *   Decided before any device is touched: FH_ERR_INVALID for a null argument, more than 16 device entries, a sketch whose hashes
 *   are not strictly ascending (named in finch_last_error, as finch_dist names it); a sketch of 2^32 - 1 hashes or more is refused
 *   as finch_dist refuses it; zero queries or zero references: FH_OK, no rows, no device needed.  Otherwise FH_ERR_NO_DEVICE
 *   without a usable device.  The caller's current device is the same after the call.
 * finch_compare_counts_stats: the kernels' time (HIP events, summed over the launches of every device entry), the launches, and
 * records_copied = the records that crossed from device to host, summed over the launches: exactly the pairs that passed; any
 * pointer may be NULL. */
typedef struct finch_count_moments {
    uint64_t common, ref_pos, query_pos, ref_count, query_count;
    double var, skew, kurt;
} finch_count_moments;
int finch_compare_counts_pair(const finch_sketches *refs, uint32_t ir, const finch_sketches *queries, uint32_t iq,
                              finch_count_moments *out);
typedef struct finch_compare_counts_result finch_compare_counts_result;
int finch_compare_counts(const finch_sketches *refs, const finch_sketches *queries, uint64_t min_common, const int *devices,
                         uint32_t n_devices, finch_compare_counts_result **out);
uint64_t finch_compare_counts_len(const finch_compare_counts_result *r);
/* row i: reference index, query index, the eight values; any pointer may be NULL */
int finch_compare_counts_copy(const finch_compare_counts_result *r, uint32_t *ref_idx, uint32_t *query_idx, finch_count_moments *rows);
int finch_compare_counts_stats(const finch_compare_counts_result *r, double *kernel_ms, uint64_t *launches, uint64_t *records_copied);
void finch_compare_counts_free(finch_compare_counts_result *r);

/* compare_counts through the index: the same rows at a cost that follows the pairs that share a hash, and a moment walk for the
 * pairs that pass only.  THE CONTRACT: for min_common >= 1, finch_index_compare_counts(ix, queries, min_common) returns byte for
 * byte what finch_compare_counts(refs, queries, min_common, ...) returns for the library the index was built from, with the
 * counts that were attached -- the rows, the query and reference indices, their order; doubles as bit patterns, NaNs as the
 * dense call produces them.  The result is a finch_compare_counts_result, read with finch_compare_counts_len / _copy / _stats and
 * freed with finch_compare_counts_free; it is made by the host code that makes the dense call's.
 * finch_index_attach_counts: the index keeps the library's hashes, not its abundances, and ref_count needs them.  The call
 *   uploads the `count` column of `refs` to every device entry of the index -- 4 bytes per posting, parallel to the index's CSR of
 *   hashes --, where it stays until finch_index_free; a second call replaces it.  `refs` must be the library the index was built
 *   from: FH_ERR_INVALID for another number of sketches or hashes (in finch_index_dist's words) and for a sketch of another length
 *   (named).  *device_bytes (may be NULL) = what the attachment holds, summed over the entries; finch_index_stats is unchanged.
 *   A call that fails on some entry leaves no counts on any: the index is as it was before its first attachment.
 *   An index of a library without a hash attaches nothing and needs no device (the call is remembered: a finch_index_add that
 *   brings the first hashes attaches their counts).  One call at a time runs on an index.
 * finch_index_compare_counts: queries are dealt over the index's device entries in chunks of index_chunk_queries, as
 *   finch_index_search deals them.  Per chunk, up to three launches: finch_index_search's count, which leaves c = |Q n R| in the
 *   query's counter of every reference that shares a hash; a selection that reads c, stores 0 back and keeps (q, r, c) where
 *   c >= min_common; and the moment walk, one wave per kept pair over the shorter side, whose 64-byte records are all that
 *   crosses to the host.  Decided before any device is touched: FH_ERR_INVALID for a null argument, for min_common == 0 (which
 *   keeps every pair, and an index cannot enumerate those: use finch_compare_counts) and for a query whose hashes are not strictly
 *   ascending (named); FH_ERR_UNSUPPORTED for a sketch of 2^32 - 1 hashes or more; FH_ERR_STATE where the library has hashes and
 *   no counts are attached (finch_index_attach_counts is named).  min_common above 2^32 - 1 is 2^32 - 1, as in the dense call.
 *   Zero queries, or an index of a library without a hash: FH_OK, no rows, no device needed.  FH_ERR_STATE, never a wrong row,
 *   where a walk's common is not the index's c ("index counters and walk disagree for pair (q, r)"; the counters are clean all
 *   the same), and for every call after one that failed between the count and the end of the selection: the index must be built
 *   again.  No pairwise form; plain set semantics over the hashes as stored, as compare_counts is.  The caller's current device
 *   is the same after the call.
 * finch_compare_counts_stats on the result: kernel_ms = all kernels of the call, launches = kernel launches (three per chunk
 *   of queries; two where no pair passes, one where none shares a hash), records_copied = exactly the pairs with
 *   common >= min_common.
 * finch_index_compare_counts_stats: pairs_touched = the pairs the device counted (c > 0), pairs_walked = the pairs the moment
 *   kernel walked (= records_copied).  FH_ERR_INVALID, outputs untouched, for a result that finch_compare_counts made. */
int finch_index_attach_counts(const finch_index *ix, const finch_sketches *refs, uint64_t *device_bytes);
int finch_index_compare_counts(const finch_index *ix, const finch_sketches *queries, uint64_t min_common,
                               finch_compare_counts_result **out);
int finch_index_compare_counts_stats(const finch_compare_counts_result *r, uint64_t *pairs_touched, uint64_t *pairs_walked);

/* the index grown and shrunk in place (Multisketch.add, __delitem__, filter_to_matches, filter_to_names: python.rs:158-248,
 * which all change the library and keep its order).  THE CONTRACT: after any sequence of finch_index_add and finch_index_keep the
 * index is indistinguishable from finch_index_new over the resulting list of sketches, through finch_index_search,
 * finch_index_dist (pairwise included), finch_index_gather and finch_index_compare_counts: the same bytes and the same
 * pairs_touched / pairs_walked / pairs_copied.  `refs` of finch_index_dist and finch_index_attach_counts is held against the
 * updated lengths.  Host work and link traffic follow what changes, not the library: the library's CSR, its per-sketch arrays
 * and its sorted postings stay on the device, and an update is a stable merge or a stable compaction of them.
 * finch_index_add: appends the sketches of `more`, in their order, after the library's last: they become the references
 *   nr .. nr + len(more) - 1.  Decided before any device work: FH_ERR_INVALID for a null argument and for a sketch of `more` whose
 *   hashes are not strictly ascending ("added sketch <i> (<name>)"); FH_ERR_UNSUPPORTED where the grown library would hold more
 *   postings than an index may (2^32 - 2048, or option index_max_postings as it is now).  An empty `more` is a no-op that
 *   succeeds.
 * finch_index_keep: keeps the references keep[0 .. n_keep), which must ascend strictly and be below the number of references
 *   (FH_ERR_INVALID otherwise, the message names the offending position: "keep[<t>] = <r>"); the survivors are renumbered
 *   0 .. n_keep - 1 in order.  n_keep == 0 (keep may be NULL then) leaves a library of no sketches.  Reordering is not offered:
 *   a reorder would have to sort every run of equal hashes again.
 * Both: *kernel_ms (may be NULL) = the update kernels' time (HIP events, summed over the device entries).  finch_index_stats
 *   reports the new n_refs, postings and device_bytes; build_kernel_ms stays the build's.  Attached counts follow: an add appends
 *   the counts of `more`, a keep compacts them, nothing is attached again; where none are attached none are made, and
 *   finch_index_compare_counts stays refused until finch_index_attach_counts.
 *   An update either happens or does not: every device entry first builds its new arrays BESIDE the old ones, and only when all
 *   entries have are they swapped in and the old ones freed, a step that cannot fail.  A refusal or a HIP error before that
 *   leaves the index answering exactly as before.  PEAK DEVICE MEMORY OF AN UPDATE IS OLD + NEW (plus the added postings' sort
 *   space, or 4 bytes per old reference and per tile).  The counters are allocated afresh, zeroed, for the queries per launch
 *   that finch_index_new's rule gives the new number of references (with index_chunk_queries as it was when the index was built);
 *   an index marked unusable by a failed search comes out usable.
 *   An index of a library without a hash has no device entries; it remembers its device list.  An add that brings the first hash
 *   opens the entries as finch_index_new would (FH_ERR_NO_DEVICE as there); a keep that leaves no hash closes them; on such an
 *   index both calls need no device while the result has no hash either.
 *   One call at a time runs on an index, updates included (others wait).  The caller's current device is the same after the
 *   call.  Option index_update_tile (1..2048, default 2048): output postings per tile of the update kernels; no result depends
 *   on it.  Values below the default are for tests on small libraries: a keep allocates 4 bytes per tile of the old postings
 *   beside old + new -- at a tile of 1 as much again as the postings' references -- and one workgroup scans them. */
int finch_index_add(finch_index *ix, const finch_sketches *more, double *kernel_ms);
int finch_index_keep(finch_index *ix, const uint32_t *keep, uint32_t n_keep, double *kernel_ms);

/* merge (Sketch.merge: merge_sketches, lib/src/python.rs:24-100).  Not fh_merge, the sharded sketcher's union of partial
 * sketches, which saturates, keeps the bottom n and both tails.  merge(first, second, size) is, in this order:
 *   1. seq_length and num_valid_kmers of the two added (u64, wrapping);
 *   2. a refusal if SketchParams::check_compatibility (mod.rs:185-212: k, hash type, hash bits, hash seed, in that order; not
 *      the variant, the scale or the sizes) finds a difference: "First sketch has <what> <v1>, but second sketch has <what> <v2>";
 *   3. one walk over the two hash lists that STOPS WHEN EITHER LIST IS EXHAUSTED (the tail of the longer list is dropped); equal
 *      hashes give one record with the first list's k-mer and label, count = count1 + count2, extra_count = extra1 + extra2.
 *      The two sums are u32 and WRAP (a release build of the reference; a debug build panics); nothing saturates;
 *   4. the clip by (size, scale), scale = that of the FIRST sketch if it is Scaled, max_hash = u64::MAX / ((1. / scale) as u64):
 *      size and scale: the longest prefix whose records have hash <= max_hash or index < size; scale alone: the prefix with
 *      hash <= max_hash; size alone: the first size records; neither: everything.  A scale whose divisor (1. / scale) as u64 is
 *      0 (above 1, negative, NaN), where the reference panics, is refused;
 *   5. name, comment, sketch parameters and filter parameters stay the first sketch's.
 * finch_merge_pair: one pair on the host, the reference's loop as written (any input it takes; size == NULL is None): *out holds
 *   the one merged sketch.  FH_ERR_INVALID for a null argument, an index out of range, step 2's refusal, step 4's refusal.
 * finch_merge_groups: n_groups groups in CSR form: group g = members[offsets[g] .. offsets[g + 1]) of s, in that order; *out
 *   holds n_groups sketches.  A group's result is the left fold: a copy of its first member merged with the second, the result
 *   with the third, ..., each with the same size -- field by field (hashes, counts, extra counts, k-mer bytes, labels, name,
 *   comment, both parameter structs, seq_length, num_valid_kmers) what folding finch_merge_pair returns.  A group of one member
 *   is that member, unchanged and unclipped.  With a scale the result depends on the order of the members; the order given is
 *   the contract.  A sketch may be in several groups and more than once in one.  The fold runs on the devices, one workgroup
 *   per group (fh_merge_lib.hip); the k-mer bytes never leave the host.  Groups of two members or more are dealt round-robin over
 *   `devices` (as finch_dist: NULL/0 = device 0, an entry may repeat, at most 16 entries; options merge_tile and
 *   merge_chunk_records apply).  The caller's current device is the same after the call.
 *   Decided before any device is touched, FH_ERR_INVALID with the group and member named in finch_last_error: a null argument,
 *   more than 16 device entries, an empty group, offsets that do not ascend, a member index out of range, a member incompatible
 *   with its group's first member (the words of step 2), a member whose hashes are not strictly ascending (every named sketch is
 *   checked, named as finch_dist names it), a member of 2^32 - 1 hashes or more, a group whose members have 2^32 records or more
 *   together, a first member of a group of two or more with a scale whose divisor is 0.  FH_OK with no device needed: n_groups ==
 *   0, or every group has one member.  Otherwise FH_ERR_NO_DEVICE without a usable device.
 *   Statistics are out-parameters, as finch_minmer_matrix's are (any may be NULL): *kernel_ms = the kernels' time (HIP events,
 *   summed over the launches of every device entry), *launches, *records_copied = the records that crossed from device to host:
 *   exactly the total length of the results of the groups of two members or more; phase_ms[0..3) = wall milliseconds, summed
 *   over the device entries, of the upload of the sketches, of the copies back, and of the k-mer gather on the host. */
int finch_merge_pair(const finch_sketches *a, uint32_t ia, const finch_sketches *b, uint32_t ib, const uint64_t *size,
                     finch_sketches **out);
int finch_merge_groups(const finch_sketches *s, const uint64_t *offsets, const uint32_t *members, uint32_t n_groups, const uint64_t *size,
                       const int *devices, uint32_t n_devices, finch_sketches **out, double *kernel_ms, uint64_t *launches,
                       uint64_t *records_copied, double *phase_ms);

/* ---- pieces that need no GPU (unit-testable on the host) ---- */
/* Build a one-sketch result from arrays (to exercise filtering / serialisation without a device).  FH_ERR_INVALID for
 * records no sketcher can emit: count == 0 or extra_count > count (mash.rs:45-56). */
int finch_sketches_from_arrays(const char *name, uint64_t seq_length, uint64_t num_valid_kmers, uint64_t n,
                               const uint64_t *hashes, const uint32_t *counts, const uint32_t *extra_counts,
                               const uint8_t *kmers, const finch_sketch_params *sketch_params,
                               const finch_filter_params *filters, finch_sketches **out);
/* filter_counts (filtering.rs:60-87) + process_post_filter (mod.rs:115-128) applied in place to sketch i;
 * `filters` is updated exactly as the reference updates its FilterParams. */
int finch_apply_filters(finch_sketches *s, uint32_t i, finch_filter_params *filters);
/* statistics.rs: cardinality (8-23: k-minimum-values estimate of the number of distinct k-mers, the reference's f32
 * arithmetic) and hist (30-47: out[c - 1] = hashes with count c; out == NULL only reports *n = the largest count) */
int finch_sketch_cardinality(const finch_sketches *s, uint32_t i, uint64_t *out);
int finch_sketch_hist(const finch_sketches *s, uint32_t i, uint64_t *out, uint64_t cap, uint64_t *n);
/* guess_filter_threshold (filtering.rs:154-195); counts must be >= 1.  Returns 0 (never a valid threshold) and sets
 * finch_last_error for a null array or a zero count. */
uint32_t finch_guess_filter_threshold(const uint32_t *counts, uint64_t n, double filter_level);
/* FASTX scan only: number of records, sum of sequence() lengths (what total_bases counts, mash.rs:72) and
 * the format of the first record (1 FASTA, 2 FASTQ).  gz images are inflated first. */
int finch_fastx_scan(const uint8_t *data, uint64_t len, uint64_t *n_records, uint64_t *total_bases, int *format);

/* Record count / total_bases exactly as the device-side FASTA path keeps them (the host reads raw text into the staging
 * buffer in chunks cut after a newline and only locates the header lines); test hook: must agree with finch_fastx_scan. */
int finch_fasta_count_chunked(const uint8_t *data, uint64_t len, uint64_t chunk, uint64_t *n_records, uint64_t *total_bases);

/* Test hook: read `path` the way the text paths read plain files (requests of `chunk` bytes; requests of >= 16 MiB on
 * a regular file are split over `read_threads` threads) into dst[0, cap); *got = bytes delivered. */
int finch_read_file_probe(const char *path, uint64_t chunk, uint32_t read_threads, uint8_t *dst, uint64_t cap, uint64_t *got);

/* Test hook: the byte stream the parsers see for an input image (magic-byte sniffing, gzip / BGZF / bzip2 / xz
 * decompression), read in requests of `chunk` bytes into dst[0, cap); *got = bytes delivered. */
int finch_source_probe(const uint8_t *data, uint64_t len, uint64_t chunk, uint8_t *dst, uint64_t cap, uint64_t *got);

/* Test hook (no device): the chunks finch_sketch_*_sharded's reader deals out for an input image.  Per chunk: meta[4i..] =
 * (offset in the decompressed text, length, FASTA start state, halo length), halos[64i..] = the halo bytes.  FASTA only:
 * n_records / total_bases as the reader counts them. */
int finch_shard_probe(const uint8_t *data, uint64_t len, uint32_t k, uint64_t chunk_bytes, uint64_t max_chunks, uint64_t *meta,
                      uint8_t *halos, uint64_t *n_chunks, uint64_t *n_records, uint64_t *total_bases);

/* Test hook (no device): the batches finch_sketch_files' reader hands to fh_push_bgzf_fastq for a BGZF image -- member
 * tables and bytes in a buffer of buf_bytes, at most max_members / text_budget bytes of text per batch --, inflated on
 * the host exactly where the tables say; text_out receives the whole text, *first_byte the reader's probe of it. */
int finch_bgzf_batch_probe(const uint8_t *data, uint64_t len, uint64_t buf_bytes, uint32_t max_members, uint64_t text_budget,
                           uint8_t *text_out, uint64_t text_cap, uint64_t *text_len, uint64_t *n_batches, int *first_byte);

/* Test hook (no device): what finch_sketch_files' reader hands to fh_push_gzip_fastq for a plain gzip image -- the probe of
 * the file's first member (*first_byte: the first byte of its text, -1 if the member is BGZF, no gzip member, or nothing can
 * be decoded from its first 64 KiB; *hdr_len: the length of its RFC 1952 header) and the bytes behind the header as the
 * reader takes them, piece_bytes at a time (*deflate_bytes of them in all, *crc_of_pieces their running CRC-32). */
int finch_gzip_probe(const uint8_t *data, uint64_t len, uint64_t piece_bytes, uint64_t *hdr_len, int *first_byte, uint64_t *deflate_bytes,
                     uint32_t *crc_of_pieces);

/* Test hook: inputs this process has sketched with the BGZF inflate on the device (finch_sketch_files /
 * finch_sketch_buffer: bgzip'd FASTQ unless option device_inflate is 0), and how many of them it had to read again through the
 * host-side inflate because the device pass refused them. */
void finch_debug_device_inflate(uint64_t *files_on_device, uint64_t *files_reread);
/* the same for plain gzip files (fh_push_gzip_fastq) */
void finch_debug_device_gzip(uint64_t *files_on_device, uint64_t *files_reread);
/* Measurement hook (bench.py --workload c5): reports the sketch kernel's own time (HIP events on every worker's stream), its
 * launches and the k-mer start positions they covered over the inputs sketched since it was switched on, then: enable = 1
 * switches it on and zeroes the sums, 0 switches it off, -1 leaves it as it is. */
void finch_debug_kernel_times(int enable, double *kernel_ms, uint64_t *launches, uint64_t *positions);
/* files of this process's finch_sketch_files calls that were sketched many-per-launch (fh_batch_*, include/finch_hip.h) and
 * files the batch path handed to a sketcher of their own instead (not taken: too few distinct k-mers below the batch's
 * threshold, ...; files that never qualified -- FASTQ, compressed, stdin, huge -- count in neither) */
void finch_debug_file_batch(uint64_t *taken, uint64_t *not_taken);
/* inputs of this process whose FASTQ text was stripped to the packed sequence stream on the host (fh_fqstrip.h: text in host
 * memory and >= 8 read threads -- headers, '+' lines and quality strings never cross the PCIe link) */
uint64_t finch_debug_fastq_host_strip(void);
/* test hook: text[0, len) -- whole records of plain 4-line FASTQ -- through that strip on `threads` threads: out (cap >= len / 2 + 64)
 * receives the packed stream (each record's sequence, blanks dropped, one 0 byte behind it); FH_ERR_INVALID if the text is not
 * plain 4-line FASTQ (what the caller then hands to the parser that is the judge of it) */
int finch_fastq_strip_probe(const uint8_t *text, uint64_t len, uint32_t threads, uint8_t *out, uint64_t cap, uint64_t *packed,
                            uint64_t *n_records, uint64_t *total_bases);

/* test hook: FASTA text (text[0] == '>') through the walk a worker of finch_sketch_files stages a genome with -- read in pieces,
 * line ends stripped, records closed by a breaker, written in the batch sketcher's two-bit form (finch_hip.h
 * fh_batch_submit_packed) -- `piece` bytes at a time; region: cap >= fh_batch_packed_bytes(len) */
int finch_fasta_two_bit_probe(const uint8_t *text, uint64_t len, uint64_t piece, uint8_t *region, uint64_t cap, uint64_t *positions,
                              uint64_t *n_records, uint64_t *total_bases);

#ifdef __cplusplus
}
#endif
#endif /* FINCH_HOST_H */
