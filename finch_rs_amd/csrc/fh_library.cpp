// fh_library.cpp -- the library calls of the C ABI (include/finch_host.h): dist, minmer_matrix, search, the index and its
// search / dist / cluster / gather / compare_counts / add / keep, gather, compare_counts, merge.  Many sketches against many, on one or several device
// entries; each call checks its arguments, deals its work over the entries (fh_entries.h) and finishes the device's integers on
// the host.
// Reading, parsing and the single-sketch calls are fh_host.cpp's.
//
// Reference items mirrored (relative to the finch-rs tree) are cited at each function.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "fh_host_model.h"
#include "fh_options.h"
#include "fh_dist.h"
#include "fh_index.h"
#include "fh_cluster.h"
#include "fh_matrix.h"
#include "fh_moments.h"
#include "fh_merge_lib.h"
#include "fh_entries.h"
#include "fh_screen.h"

namespace fh {
uint64_t api_scaled_max_hash(double scale); // fh_internal.h (which needs the HIP headers): a ScaledSketcher's max_hash, scaled.rs:23,31
}

using namespace finch;
using fh::cfg_u64;
using fh::fork_join;

// ---------------------------------------------------------------------------------------------
// what every call does around its device entries
// ---------------------------------------------------------------------------------------------
namespace {

constexpr uint32_t DIST_MAX_ENTRIES = 16; // device entries of one call, and host threads of its epilogue

int check_entry_count(uint32_t n_devices) {
    if (n_devices > DIST_MAX_ENTRIES) return hfail(FH_ERR_INVALID, "at most %u device entries (got %u)", DIST_MAX_ENTRIES, n_devices);
    return FH_OK;
}

// the call's device entries: `devices` as given (an ordinal may repeat), or device 0
int resolve_devices(const int *devices, uint32_t n_devices, std::vector<int> &devs) {
    const int ndev = fh_device_count();
    if (ndev <= 0) return hfail(FH_ERR_NO_DEVICE, "no usable HIP device (this library has no CPU path)");
    devs = n_devices ? std::vector<int>(devices, devices + n_devices) : std::vector<int>{0};
    for (int d : devs)
        if (d < 0 || d >= ndev) return hfail(FH_ERR_NO_DEVICE, "no usable HIP device: device %d requested, %d visible", d, ndev);
    return FH_OK;
}

// the caller's current device, put back when the call leaves (its thread runs the first device entry)
struct DeviceGuard {
    int prev = fh::matrix_current_device();
    ~DeviceGuard() { fh::matrix_restore_device(prev); }
};

// references per launch against nq queries: `option` pairs (at least one reference), no more than the grid takes; cap_2_31:
// a chunk's list has a u32 cursor, so no more than 2^31 pairs per launch, whatever the option says
uint32_t chunk_refs(const char *option, uint64_t dflt, uint32_t nq, uint32_t nr, bool cap_2_31) {
    uint64_t chunk_pairs = std::max<uint64_t>(1, cfg_u64(option, dflt));
    if (cap_2_31) chunk_pairs = std::min<uint64_t>(chunk_pairs, 1ull << 31);
    return (uint32_t)std::min<uint64_t>({std::max<uint64_t>(1, chunk_pairs / nq), nr, 65535ull * 64});
}

// what an entry makes of a device call's return: the call fails with the device layer's message
bool entry_failed(fh::EntryError &err, int rc) {
    if (rc != FH_OK) err.fail(rc, fh_last_error());
    return rc != FH_OK;
}

} // namespace

// ---------------------------------------------------------------------------------------------
// finch dist (cli/src/main.rs:85-125, calc_sketch_distances main.rs:315-333): every (query, reference) pair, reference-major.
// The device computes each pair's integer counts (fh_dist.hip); distance_from_counts turns them into the doubles, as it does
// for finch_distance.  DESIGN.md §3.7.
// ---------------------------------------------------------------------------------------------

struct finch_dist_result {
    struct Row {
        uint32_t q, r;
        finch_distance_out d;
    };
    std::vector<std::vector<Row>> parts; // in reference-major order
    uint64_t n = 0;
    std::vector<std::string> qnames, rnames;
    double kernel_ms = 0.;
    uint64_t launches = 0;
    bool from_index = false;          // finch_index_dist made it ...
    uint64_t touched = 0, copied = 0; // ... from this many pairs with c > 0, of which this many crossed to the host
};

namespace {

bool opt_u32_equal(uint32_t has_a, uint32_t a, uint32_t has_b, uint32_t b) { return (has_a != 0) == (has_b != 0) && (!has_a || a == b); }

// Sketch's derived PartialEq (serialization/mod.rs:45): every field by value; the f64s by ==, so a NaN is not equal to itself;
// Option<u32> by its flag, then the value; SketchParams on its own variant's fields only (padding and unused fields ignored)
bool sketch_equal(const Sketch &a, const Sketch &b) {
    if (a.name != b.name || a.seq_length != b.seq_length || a.num_valid_kmers != b.num_valid_kmers || a.comment != b.comment ||
        a.hashes.size() != b.hashes.size())
        return false;
    const finch_filter_params &fa = a.filter_params, &fb = b.filter_params;
    if (fa.filter_on != fb.filter_on || !opt_u32_equal(fa.has_abun_lo, fa.abun_lo, fb.has_abun_lo, fb.abun_lo) ||
        !opt_u32_equal(fa.has_abun_hi, fa.abun_hi, fb.has_abun_hi, fb.abun_hi) || !(fa.err_filter == fb.err_filter) ||
        !(fa.strand_filter == fb.strand_filter))
        return false;
    const finch_sketch_params &pa = a.sketch_params, &pb = b.sketch_params;
    if (pa.kind != pb.kind || pa.kmer_length != pb.kmer_length) return false;
    if (pa.kind == 0 && (pa.kmers_to_sketch != pb.kmers_to_sketch || pa.final_size != pb.final_size ||
                         (pa.no_strict != 0) != (pb.no_strict != 0) || pa.hash_seed != pb.hash_seed))
        return false;
    if (pa.kind == 1 && (pa.kmers_to_sketch != pb.kmers_to_sketch || !(pa.scale == pb.scale) || pa.hash_seed != pb.hash_seed))
        return false;
    for (size_t i = 0; i < a.hashes.size(); ++i) {
        const KmerCount &x = a.hashes[i], &y = b.hashes[i];
        if (x.hash != y.hash || x.count != y.count || x.extra_count != y.extra_count || !(x.kmer == y.kmer)) return false;
        if ((x.label != nullptr) != (y.label != nullptr) || (x.label && *x.label != *y.label)) return false;
    }
    return true;
}

// one side of a call in the device's form (fh_dist.h; with the counts: fh_moments.h, a gather's query side)
struct DistCsr {
    std::vector<uint64_t> hashes, offsets, max_hash;
    std::vector<uint32_t> flags, counts;
    std::vector<double> scale;
    void build(const std::vector<Sketch> &v, bool old_mode, bool with_counts = false) {
        offsets.assign(1, 0);
        size_t total = 0;
        for (const Sketch &s : v) total += s.hashes.size();
        hashes.reserve(total);
        if (with_counts) counts.reserve(total);
        for (const Sketch &s : v) {
            if (with_counts) // (two loops: the plain one is every dist and search call's walk over the whole library)
                for (const KmerCount &h : s.hashes) hashes.push_back(h.hash), counts.push_back(h.count);
            else
                for (const KmerCount &h : s.hashes) hashes.push_back(h.hash);
            offsets.push_back(hashes.size());
            const bool scaled = !old_mode && s.sketch_params.kind == 1, positive = scaled && s.sketch_params.scale > 0.;
            flags.push_back((scaled ? 1u : 0u) | (positive ? 2u : 0u));
            scale.push_back(scaled ? s.sketch_params.scale : 0.);
            max_hash.push_back(positive ? scale_max_hash(s.sketch_params.scale) : 0);
        }
    }
    fh::DistSide view() const { return fh::DistSide{hashes.data(), offsets.data(), (uint32_t)(offsets.size() - 1), max_hash.data(), flags.data(), scale.data()}; }
    fh::MomentsSide moments_view() const { return fh::MomentsSide{hashes.data(), counts.data(), offsets.data(), (uint32_t)(offsets.size() - 1)}; }
};

int check_ascending(const std::vector<Sketch> &v, const char *what) {
    for (size_t s = 0; s < v.size(); ++s) {
        const std::vector<KmerCount> &h = v[s].hashes;
        if (h.size() >= UINT32_MAX)
            return hfail(FH_ERR_UNSUPPORTED, "%s sketch %zu (%s) has %zu hashes (at most 2^32 - 2)", what, s, v[s].name.c_str(), h.size());
        for (size_t j = 1; j < h.size(); ++j)
            if (!(h[j - 1].hash < h[j].hash))
                return hfail(FH_ERR_INVALID, "%s sketch %zu (%s): hashes not strictly ascending at %zu", what, s, v[s].name.c_str(), j);
    }
    return FH_OK;
}

constexpr uint64_t DIST_CHUNK_PAIRS = 4u << 20; // pairs per launch: 48 MiB of counts per result buffer

} // namespace

extern "C" {

int finch_dist(const finch_sketches *queries, const finch_sketches *refs, int old_mode, double max_distance, const int *devices,
               uint32_t n_devices, finch_dist_result **out) try {
    if (!queries || !refs || !out || (n_devices && !devices)) return hfail(FH_ERR_INVALID, "null argument");
    if (int rc = check_entry_count(n_devices)) return rc;
    const std::vector<Sketch> &Qs = queries->v, &Rs = refs->v;
    if (int rc = check_ascending(Qs, "query")) return rc;
    if (int rc = check_ascending(Rs, "reference")) return rc;
    if (old_mode) { // old_distance refuses an empty query against a non-empty reference (no such pair is ever self-skipped)
        bool empty_q = false, full_r = false;
        for (const Sketch &s : Qs) empty_q = empty_q || s.hashes.empty();
        for (const Sketch &s : Rs) full_r = full_r || !s.hashes.empty();
        if (empty_q && full_r) return hfail(FH_ERR_INVALID, "old_distance: empty query sketch");
    }
    std::vector<int> devs;
    if (int rc = resolve_devices(devices, n_devices, devs)) return rc;
    DeviceGuard restore_device;

    auto res = std::make_unique<finch_dist_result>();
    for (const Sketch &s : Qs) res->qnames.push_back(s.name);
    for (const Sketch &s : Rs) res->rnames.push_back(s.name);
    const uint32_t nq = (uint32_t)Qs.size(), nr = (uint32_t)Rs.size();
    if (nq == 0 || nr == 0) {
        *out = res.release();
        return FH_OK;
    }
    // the self-skip's first test: equal names (an id per distinct name)
    std::unordered_map<std::string, uint32_t> ids;
    std::vector<uint32_t> qid(nq), rid(nr);
    for (uint32_t q = 0; q < nq; ++q) qid[q] = ids.emplace(Qs[q].name, (uint32_t)ids.size()).first->second;
    for (uint32_t r = 0; r < nr; ++r) rid[r] = ids.emplace(Rs[r].name, (uint32_t)ids.size()).first->second;

    DistCsr qc, rc_;
    qc.build(Qs, old_mode != 0);
    rc_.build(Rs, old_mode != 0);
    const uint32_t per_chunk = chunk_refs("dist_chunk_pairs", DIST_CHUNK_PAIRS, nq, nr, false);
    const uint32_t n_chunks = (nr + per_chunk - 1) / per_chunk;
    const uint32_t n_entries = (uint32_t)std::min<size_t>(devs.size(), n_chunks); // (an entry without a chunk opens nothing)
    const unsigned T = std::max(1u, DIST_MAX_ENTRIES / n_entries);
    const uint32_t slice = (uint32_t)cfg_u64("dist_slice", 4096);
    res->parts.resize((size_t)n_chunks * T);
    fh::EntryError err;
    std::mutex stat_mu;

    // chunk k's rows: its references split over T threads
    auto epilogue = [&](uint32_t k, const uint32_t *cnt) {
        const uint32_t r0 = k * per_chunk, r1 = std::min(nr, r0 + per_chunk), per = (r1 - r0 + T - 1) / T;
        // (T host threads, not device entries: for_entries for its out-of-memory catch)
        fh::for_entries(T, err, FH_ERR_CAPACITY, [&](unsigned t) {
            std::vector<finch_dist_result::Row> &rows = res->parts[(size_t)k * T + t];
            const uint32_t lo = std::min(r1, r0 + t * per), hi = std::min(r1, lo + per);
            for (uint32_t r = lo; r < hi; ++r)
                for (uint32_t q = 0; q < nq; ++q) {
                    if (qid[q] == rid[r] && sketch_equal(Qs[q], Rs[r])) continue; // main.rs:324
                    const uint32_t *x = cnt + ((size_t)(r - r0) * nq + q) * 3;
                    finch_dist_result::Row row{q, r, {}};
                    distance_from_counts(old_mode != 0, x[0], old_mode ? Rs[r].hashes.size() : x[1], x[2],
                                         Qs[q].sketch_params.kmer_length, true, &row.d);
                    if (row.d.mash_distance <= max_distance) rows.push_back(row);
                }
        });
    };
    // one thread per device entry: chunks e, e + n_entries, ...; chunk m + 1's kernel runs while chunk m's rows are made
    fh::for_entries(n_entries, err, FH_ERR_CAPACITY, [&](unsigned e) {
        fh::DistDevice *dd = nullptr;
        fh::Finally close_dd{[&] { fh::dist_close(dd); }};
        if (entry_failed(err, fh::dist_open(devs[e], qc.view(), rc_.view(), slice, (uint64_t)per_chunk * nq, &dd))) return;
        std::vector<uint32_t> mine;
        for (uint32_t k = e; k < n_chunks; k += n_entries) mine.push_back(k);
        double ms_sum = 0.;
        auto launch = [&](size_t m, int slot) {
            const uint32_t r0 = mine[m] * per_chunk;
            return fh::dist_launch(dd, slot, r0, std::min(nr, r0 + per_chunk));
        };
        auto take = [&](size_t m, int slot) {
            const uint32_t *cnt = nullptr;
            double ms = 0.;
            if (int rc = fh::dist_wait(dd, slot, &cnt, &ms)) return rc;
            ms_sum += ms;
            epilogue(mine[m], cnt);
            return FH_OK;
        };
        entry_failed(err, fh::two_slot(mine.size(), err, launch, take));
        std::lock_guard<std::mutex> g(stat_mu);
        res->kernel_ms += ms_sum;
        res->launches += mine.size();
    });
    if (err.failed()) return hfail(err.rc(), "%s", err.msg().c_str());
    for (const auto &p : res->parts) res->n += p.size();
    *out = res.release();
    return FH_OK;
} FINCH_CATCH

uint64_t finch_dist_len(const finch_dist_result *r) { return r ? r->n : 0; }

int finch_dist_copy(const finch_dist_result *r, uint32_t *query_idx, uint32_t *ref_idx, finch_distance_out *rows) try {
    if (!r) return hfail(FH_ERR_INVALID, "null argument");
    size_t o = 0;
    for (const auto &p : r->parts)
        for (const finch_dist_result::Row &x : p) {
            if (query_idx) query_idx[o] = x.q;
            if (ref_idx) ref_idx[o] = x.r;
            if (rows) rows[o] = x.d;
            ++o;
        }
    return FH_OK;
} FINCH_CATCH

// serde_json::to_writer(&Vec<SketchDistance>) (main.rs:117-121; field order serialization/mod.rs:31-43); a NaN is null
int finch_dist_to_json(const finch_dist_result *r, char **out, uint64_t *len) try {
    if (!r || !out) return hfail(FH_ERR_INVALID, "null argument");
    auto f64 = [](std::string &o, double v) { o += std::isfinite(v) ? json_f64(v) : std::string("null"); };
    std::string o = "[";
    bool first = true;
    for (const auto &p : r->parts)
        for (const finch_dist_result::Row &x : p) {
            if (!first) o.push_back(',');
            first = false;
            o += "{\"containment\":";
            f64(o, x.d.containment);
            o += ",\"jaccard\":";
            f64(o, x.d.jaccard);
            o += ",\"mashDistance\":";
            f64(o, x.d.mash_distance);
            o += ",\"commonHashes\":" + std::to_string(x.d.common_hashes);
            o += ",\"totalHashes\":" + std::to_string(x.d.total_hashes);
            o += ",\"query\":";
            json_escape(o, r->qnames[x.q]);
            o += ",\"reference\":";
            json_escape(o, r->rnames[x.r]);
            o.push_back('}');
        }
    o.push_back(']');
    char *p = (char *)malloc(o.size() + 1);
    if (!p) return hfail(FH_ERR_CAPACITY, "out of host memory");
    memcpy(p, o.data(), o.size() + 1);
    *out = p;
    if (len) *len = o.size();
    return FH_OK;
} FINCH_CATCH

int finch_dist_stats(const finch_dist_result *r, double *kernel_ms, uint64_t *launches) try {
    if (!r) return hfail(FH_ERR_INVALID, "null argument");
    if (kernel_ms) *kernel_ms = r->kernel_ms;
    if (launches) *launches = r->launches;
    return FH_OK;
} FINCH_CATCH

void finch_dist_free(finch_dist_result *r) { delete r; }

int finch_sketches_select(const finch_sketches *s, const uint32_t *idx, uint32_t n, finch_sketches **out) try {
    if (!s || !out || (n && !idx)) return hfail(FH_ERR_INVALID, "null argument");
    auto res = std::make_unique<finch_sketches>();
    res->v.reserve(n);
    for (uint32_t i = 0; i < n; ++i) {
        if (idx[i] >= s->v.size()) return hfail(FH_ERR_INVALID, "index %u of %zu sketches", idx[i], s->v.size());
        res->v.push_back(s->v[idx[i]]);
    }
    *out = res.release();
    return FH_OK;
} FINCH_CATCH

} // extern "C"

// ---------------------------------------------------------------------------------------------
// minmer_matrix (lib/src/distance.rs:345-364): the counts many sketches hold for the hashes of one reference sketch, an
// S x R matrix of i32.  The device fills whole rows (fh_matrix.hip); this side checks, deals rows and copies.  DESIGN.md §3.9.
// ---------------------------------------------------------------------------------------------
namespace {

constexpr uint64_t MATRIX_CHUNK_BYTES = 64ull << 20; // cells per result buffer (device and pinned), in bytes

int matrix_check(const Sketch &s, const char *what, size_t idx) {
    const std::vector<KmerCount> &h = s.hashes;
    if (h.size() >= UINT32_MAX)
        return hfail(FH_ERR_INVALID, "%s %zu (%s) has %zu hashes (at most 2^32 - 2)", what, idx, s.name.c_str(), h.size());
    for (size_t j = 1; j < h.size(); ++j)
        if (!(h[j - 1].hash < h[j].hash))
            return hfail(FH_ERR_INVALID, "%s %zu (%s): hashes not strictly ascending at %zu", what, idx, s.name.c_str(), j);
    return FH_OK;
}

} // namespace

extern "C" {

int finch_minmer_matrix(const finch_sketches *refs, uint32_t ir, const finch_sketches *sketches, const int *devices,
                        uint32_t n_devices, int32_t *out, uint64_t out_len, double *kernel_ms, uint64_t *launches) try {
    if (kernel_ms) *kernel_ms = 0.;
    if (launches) *launches = 0;
    if (!refs || !sketches || (n_devices && !devices) || (out_len && !out)) return hfail(FH_ERR_INVALID, "null argument");
    if (int rc = check_entry_count(n_devices)) return rc;
    if (ir >= refs->v.size()) return hfail(FH_ERR_INVALID, "reference sketch %u of %zu sketches", ir, refs->v.size());
    const Sketch &ref = refs->v[ir];
    const std::vector<Sketch> &Ss = sketches->v;
    if (int rc = matrix_check(ref, "reference sketch", ir)) return rc;
    uint64_t longest = 0;
    for (size_t i = 0; i < Ss.size(); ++i) {
        if (int rc = matrix_check(Ss[i], "sketch", i)) return rc;
        longest = std::max<uint64_t>(longest, Ss[i].hashes.size());
    }
    const uint64_t S = Ss.size(), R = ref.hashes.size();
    if (R == 0 && longest) // the reference reads ref_sketch[0] for the first hash of any sketch: a panic
        return hfail(FH_ERR_INVALID, "reference sketch %u (%s) is empty", ir, ref.name.c_str());
    if (out_len != S * R) // (S < 2^32 and R < 2^32 - 1: no overflow)
        return hfail(FH_ERR_INVALID, "out_len %llu, the matrix has %llu x %llu cells", (unsigned long long)out_len,
                     (unsigned long long)S, (unsigned long long)R);
    if (S * R == 0) return FH_OK;

    std::vector<int> devs;
    if (int rc = resolve_devices(devices, n_devices, devs)) return rc;
    DeviceGuard restore_device;

    std::vector<uint64_t> ref_hashes(R);
    for (uint64_t p = 0; p < R; ++p) ref_hashes[p] = ref.hashes[p].hash;
    const uint64_t budget_rows = std::max<uint64_t>(1, MATRIX_CHUNK_BYTES / (R * sizeof(int32_t)));
    const uint32_t per_chunk = (uint32_t)std::min<uint64_t>(
        {std::max<uint64_t>(1, cfg_u64("matrix_chunk_rows", budget_rows)), S, fh::MATRIX_MAX_ROWS});
    const uint32_t n_chunks = (uint32_t)((S + per_chunk - 1) / per_chunk);
    uint64_t max_entries = 0;
    for (uint32_t k = 0; k < n_chunks; ++k) {
        uint64_t e = 0;
        for (uint64_t i = (uint64_t)k * per_chunk; i < std::min<uint64_t>(S, (uint64_t)(k + 1) * per_chunk); ++i) e += Ss[i].hashes.size();
        max_entries = std::max(max_entries, e);
    }
    const uint32_t n_entries = (uint32_t)std::min<uint64_t>(devs.size(), n_chunks); // (an entry without a chunk opens nothing)
    const unsigned T = std::max(1u, DIST_MAX_ENTRIES / n_entries);
    const uint32_t slice = (uint32_t)std::min<uint64_t>(cfg_u64("matrix_slice", fh::MATRIX_MAX_SLICE), fh::MATRIX_MAX_SLICE);

    fh::EntryError err;
    std::mutex stat_mu;
    double ms_total = 0.;
    uint64_t launches_total = 0;

    // one thread per device entry: chunks e, e + n_entries, ...; chunk m + 1's upload and kernel run while chunk m's rows
    // cross the link and are copied out of the pinned buffer (by T threads where the chunk is large)
    fh::for_entries(n_entries, err, FH_ERR_CAPACITY, [&](unsigned e) {
        fh::MatrixDevice *md = nullptr;
        fh::Finally close_md{[&] { fh::matrix_close(md); }};
        if (entry_failed(err, fh::matrix_open(devs[e], ref_hashes.data(), (uint32_t)R, per_chunk, max_entries, (uint32_t)longest, slice, &md))) return;
        std::vector<uint32_t> mine;
        for (uint32_t k = e; k < n_chunks; k += n_entries) mine.push_back(k);
        double ms_sum = 0.;
        auto launch = [&](size_t m, int slot) {
            const uint64_t r0 = (uint64_t)mine[m] * per_chunk, r1 = std::min<uint64_t>(S, r0 + per_chunk);
            uint64_t entries = 0;
            for (uint64_t i = r0; i < r1; ++i) entries += Ss[i].hashes.size();
            uint64_t *off, *hs;
            uint32_t *cs;
            if (int rc = fh::matrix_stage(md, slot, (uint32_t)(r1 - r0), entries, &off, &hs, &cs)) return rc;
            uint64_t at = 0;
            for (uint64_t i = r0; i < r1; ++i) {
                off[i - r0] = at;
                for (const KmerCount &h : Ss[i].hashes) hs[at] = h.hash, cs[at] = h.count, ++at;
            }
            off[r1 - r0] = at;
            return fh::matrix_launch(md, slot);
        };
        auto take = [&](size_t m, int slot) {
            const int32_t *cells = nullptr;
            double ms = 0.;
            if (int rc = fh::matrix_wait(md, slot, &cells, &ms)) return rc;
            ms_sum += ms;
            const uint64_t r0 = (uint64_t)mine[m] * per_chunk, r1 = std::min<uint64_t>(S, r0 + per_chunk);
            const uint64_t n_cells = (r1 - r0) * R;
            const unsigned t_copy = (unsigned)std::min<uint64_t>(T, std::max<uint64_t>(1, n_cells >> 20)); // a thread per 4 MiB
            const uint64_t per = (n_cells + t_copy - 1) / t_copy;
            fork_join(t_copy, [&](unsigned t) {
                const uint64_t lo = std::min<uint64_t>(n_cells, t * per), hi = std::min<uint64_t>(n_cells, lo + per);
                memcpy(out + r0 * R + lo, cells + lo, (hi - lo) * sizeof(int32_t));
            });
            return FH_OK;
        };
        entry_failed(err, fh::two_slot(mine.size(), err, launch, take));
        std::lock_guard<std::mutex> g(stat_mu);
        ms_total += ms_sum;
        launches_total += mine.size();
    });
    if (err.failed()) return hfail(err.rc(), "%s", err.msg().c_str());
    if (kernel_ms) *kernel_ms = ms_total;
    if (launches) *launches = launches_total;
    return FH_OK;
} FINCH_CATCH

} // extern "C"

// ---------------------------------------------------------------------------------------------
// search (Multisketch.best_match / filter_to_matches, lib/src/python.rs:202-234): per query the references whose containment
// is at least a threshold, best first.  The counts are finch_dist's, but they stay on the device, which also selects
// (fh_dist.hip: k_search_top / k_search_all); only the selected candidates come here, to be merged over the chunks, sorted and
// turned into rows by distance_from_counts.  DESIGN.md §3.10.
// ---------------------------------------------------------------------------------------------
struct finch_search_result {
    std::vector<uint64_t> offsets; // n_queries + 1
    std::vector<uint32_t> q, r;
    std::vector<finch_distance_out> d;
    double kernel_ms = 0.;
    uint64_t launches = 0, copied = 0;
    bool from_index = false; // made by finch_index_search: `touched` = the pairs its device counted
    uint64_t touched = 0;
};

namespace {

struct SearchCand {
    uint32_t q, r, c, i, j;
};

// what finch_search and finch_index_search do with the candidates the device left (`found`: lists in any order, emptied here):
// by query, each query's sorted by (containment descending, reference ascending) and cut to top_n; the doubles are
// distance_from_counts', as finch_distance has them.  res->offsets: n_queries + 1 zeros on entry.
int search_finish(std::vector<std::vector<SearchCand>> &found, const std::vector<Sketch> &Qs, uint32_t nr, uint32_t top_n, finch_search_result *res) {
    const uint32_t nq = (uint32_t)Qs.size();
    std::vector<uint64_t> at((size_t)nq + 1, 0);
    for (const auto &f : found)
        for (const SearchCand &x : f) {
            if (x.q >= nq || x.r >= nr) return hfail(FH_ERR_STATE, "search: candidate (%u, %u) of %u x %u", x.q, x.r, nq, nr);
            ++at[x.q + 1];
        }
    for (uint32_t q = 0; q < nq; ++q) at[q + 1] += at[q];
    struct Row {
        uint32_t r;
        finch_distance_out d;
    };
    std::vector<Row> rows(at[nq]);
    {
        std::vector<uint64_t> fill(at.begin(), at.end() - 1);
        for (auto &f : found) {
            for (const SearchCand &x : f) {
                Row &row = rows[fill[x.q]++];
                row.r = x.r;
                distance_from_counts(false, x.c, x.i, x.j, Qs[x.q].sketch_params.kmer_length, true, &row.d);
            }
            std::vector<SearchCand>().swap(f);
        }
    }
    const unsigned T = (unsigned)std::min<uint64_t>(DIST_MAX_ENTRIES, std::max<uint64_t>(1, rows.size() >> 16));
    const uint32_t per = (nq + T - 1) / T;
    fork_join(T, [&](unsigned t) {
        for (uint32_t q = std::min(nq, t * per); q < std::min<uint64_t>(nq, (uint64_t)(t + 1) * per); ++q)
            std::sort(rows.begin() + at[q], rows.begin() + at[q + 1], [](const Row &a, const Row &b) {
                return a.d.containment > b.d.containment || (a.d.containment == b.d.containment && a.r < b.r);
            });
    });
    for (uint32_t q = 0; q < nq; ++q) {
        const uint64_t have = at[q + 1] - at[q];
        res->offsets[q + 1] = res->offsets[q] + (top_n ? std::min<uint64_t>(have, top_n) : have);
    }
    const uint64_t total = res->offsets[nq];
    res->q.resize(total);
    res->r.resize(total);
    res->d.resize(total);
    for (uint32_t q = 0; q < nq; ++q)
        for (uint64_t o = res->offsets[q], s = at[q]; o < res->offsets[q + 1]; ++o, ++s) {
            res->q[o] = q;
            res->r[o] = rows[s].r;
            res->d[o] = rows[s].d;
        }
    return FH_OK;
}

} // namespace

extern "C" {

int finch_search(const finch_sketches *queries, const finch_sketches *refs, double min_containment, uint32_t top_n, const int *devices,
                 uint32_t n_devices, finch_search_result **out) try {
    if (!queries || !refs || !out || (n_devices && !devices)) return hfail(FH_ERR_INVALID, "null argument");
    if (int rc = check_entry_count(n_devices)) return rc;
    const std::vector<Sketch> &Qs = queries->v, &Rs = refs->v;
    if (int rc = check_ascending(Qs, "query")) return rc;
    if (int rc = check_ascending(Rs, "reference")) return rc;
    const uint32_t nq = (uint32_t)Qs.size(), nr = (uint32_t)Rs.size();
    auto res = std::make_unique<finch_search_result>();
    res->offsets.assign((size_t)nq + 1, 0);
    if (nq == 0 || nr == 0) {
        *out = res.release();
        return FH_OK;
    }
    std::vector<int> devs;
    if (int rc = resolve_devices(devices, n_devices, devs)) return rc;
    DeviceGuard restore_device;

    DistCsr qc, rc_;
    qc.build(Qs, false);
    rc_.build(Rs, false);
    const uint32_t per_chunk = chunk_refs("dist_chunk_pairs", DIST_CHUNK_PAIRS, nq, nr, true);
    const uint32_t n_chunks = (nr + per_chunk - 1) / per_chunk;
    const uint32_t n_entries = (uint32_t)std::min<size_t>(devs.size(), n_chunks); // (an entry without a chunk opens nothing)
    const uint32_t slice = (uint32_t)cfg_u64("dist_slice", 4096);
    std::vector<std::vector<SearchCand>> found(n_chunks); // per chunk; top mode: by query, each query's best first
    fh::EntryError err;
    std::mutex stat_mu;

    // one thread per device entry: chunks e, e + n_entries, ...; chunk m + 1's kernels run while chunk m's candidates are taken
    fh::for_entries(n_entries, err, FH_ERR_CAPACITY, [&](unsigned e) {
        fh::DistDevice *dd = nullptr;
        fh::Finally close_dd{[&] { fh::dist_close(dd); }};
        if (entry_failed(err, fh::search_open(devs[e], qc.view(), rc_.view(), slice, (uint64_t)per_chunk * nq, top_n, min_containment, &dd))) return;
        std::vector<uint32_t> mine;
        for (uint32_t k = e; k < n_chunks; k += n_entries) mine.push_back(k);
        double ms_sum = 0.;
        uint64_t copied = 0;
        auto launch = [&](size_t m, int slot) {
            const uint32_t r0 = mine[m] * per_chunk;
            return fh::search_launch(dd, slot, r0, std::min(nr, r0 + per_chunk));
        };
        auto take = [&](size_t m, int slot) {
            const uint32_t *ent = nullptr, *per_query = nullptr;
            uint64_t n = 0;
            double ms = 0.;
            if (int rc = fh::search_wait(dd, slot, &ent, &per_query, &n, &ms)) return rc;
            ms_sum += ms;
            copied += n;
            std::vector<SearchCand> &to = found[mine[m]];
            if (per_query) { // n_queries x top_n slots of (r, c, i, j)
                const uint32_t slots = (uint32_t)(n / nq);
                for (uint32_t q = 0; q < nq; ++q)
                    for (uint32_t s = 0; s < std::min(per_query[q], slots); ++s) {
                        const uint32_t *x = ent + ((size_t)q * slots + s) * 4;
                        to.push_back(SearchCand{q, x[0], x[1], x[2], x[3]});
                    }
            } else {
                to.resize(n);
                static_assert(sizeof(SearchCand) == 5 * sizeof(uint32_t), "the device's entry");
                if (n) memcpy(to.data(), ent, n * sizeof(SearchCand));
            }
            return FH_OK;
        };
        entry_failed(err, fh::two_slot(mine.size(), err, launch, take));
        std::lock_guard<std::mutex> g(stat_mu);
        res->kernel_ms += ms_sum;
        res->launches += mine.size();
        res->copied += copied;
    });
    if (err.failed()) return hfail(err.rc(), "%s", err.msg().c_str());

    if (int rc = search_finish(found, Qs, nr, top_n, res.get())) return rc;
    *out = res.release();
    return FH_OK;
} FINCH_CATCH

uint64_t finch_search_len(const finch_search_result *r) { return r ? r->d.size() : 0; }

int finch_search_offsets(const finch_search_result *r, uint64_t *offsets) try {
    if (!r || !offsets) return hfail(FH_ERR_INVALID, "null argument");
    memcpy(offsets, r->offsets.data(), r->offsets.size() * sizeof(uint64_t));
    return FH_OK;
} FINCH_CATCH

int finch_search_copy(const finch_search_result *r, uint32_t *query_idx, uint32_t *ref_idx, finch_distance_out *rows) try {
    if (!r) return hfail(FH_ERR_INVALID, "null argument");
    const size_t n = r->d.size();
    if (query_idx && n) memcpy(query_idx, r->q.data(), n * sizeof(uint32_t));
    if (ref_idx && n) memcpy(ref_idx, r->r.data(), n * sizeof(uint32_t));
    if (rows && n) memcpy(rows, r->d.data(), n * sizeof(finch_distance_out));
    return FH_OK;
} FINCH_CATCH

int finch_search_stats(const finch_search_result *r, double *kernel_ms, uint64_t *launches, uint64_t *candidates_copied) try {
    if (!r) return hfail(FH_ERR_INVALID, "null argument");
    if (kernel_ms) *kernel_ms = r->kernel_ms;
    if (launches) *launches = r->launches;
    if (candidates_copied) *candidates_copied = r->copied;
    return FH_OK;
} FINCH_CATCH

void finch_search_free(finch_search_result *r) { delete r; }

} // extern "C"

// ---------------------------------------------------------------------------------------------
// index: the same search through an inverted index of the library's hashes (fh_index.hip), built once per library.  The device
// counts only the pairs that share a hash -- the only ones a threshold above 0 can keep --; their candidates come here and go
// through finch_search's own finish, so the rows are finch_search's.  DESIGN.md §3.14.
// ---------------------------------------------------------------------------------------------
struct finch_index {
    uint32_t nr = 0, chunk = 0;
    uint64_t postings = 0, device_bytes = 0;
    double build_ms = 0.;
    std::vector<fh::IndexDevice *> entries; // one per device entry; none where the library has no hash
    std::vector<uint32_t> rlen;             // the library's lengths: what finch_index_attach_counts holds its `refs` against
    bool counts_attached = false;           // finch_index_attach_counts has left the library's counts on every entry
    // what finch_index_add / finch_index_keep need beyond the device's arrays: the device list and the index_chunk_queries
    // that were in force at finch_index_new (has_chunk_opt: the option was set), and the per-sketch scale data, which an index
    // without a hash has nowhere else when an add brings its first one
    std::vector<int> devs;
    bool has_chunk_opt = false;
    uint64_t chunk_opt = 0;
    std::vector<uint32_t> rflag;
    std::vector<uint64_t> rmax;
    std::vector<double> rscale;
    mutable std::mutex mu;                  // one call at a time: the counters belong to the index, and an update swaps its arrays
    ~finch_index() {
        if (entries.empty()) return;
        const int prev = fh::matrix_current_device();
        for (fh::IndexDevice *d : entries) fh::index_close(d);
        fh::matrix_restore_device(prev);
    }
};

// what finch_index_screen (fh_host.cpp) needs of an index: fh_screen.h
namespace fh {
std::mutex &index_mutex_of(const finch_index *ix) { return ix->mu; }
IndexDevice *index_first_entry(const finch_index *ix) { return ix->entries.empty() ? nullptr : ix->entries[0]; }
const std::vector<uint32_t> &index_ref_lengths(const finch_index *ix) { return ix->rlen; }
} // namespace fh

namespace {

constexpr uint64_t INDEX_STATE_BYTES = 256ull << 20; // counters plus touched lists of a launch by default, at most
constexpr uint64_t INDEX_CHUNK_MAX = 4096;           // ... and its queries, at most

// queries per launch for a library of nr > 0 sketches: 8 bytes per (query, reference) -- a counter and a place in the touched
// list --, or the option as it was at finch_index_new; a launch's list has a u32 cursor
uint32_t index_chunk_for(const finch_index &ix, uint32_t nr) {
    const uint64_t by_memory = std::min<uint64_t>(std::max<uint64_t>(1, INDEX_STATE_BYTES / (8ull * nr)), INDEX_CHUNK_MAX);
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, ix.has_chunk_opt ? ix.chunk_opt : by_memory), std::max<uint64_t>(1, (1ull << 31) / nr));
}

uint64_t index_max_postings() { return std::min<uint64_t>(cfg_u64("index_max_postings", fh::INDEX_MAX_POSTINGS), fh::INDEX_MAX_POSTINGS); }

uint32_t index_update_tile() { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, cfg_u64("index_update_tile", 2048)), 2048); }

} // namespace

extern "C" {

int finch_index_new(const finch_sketches *refs, const int *devices, uint32_t n_devices, finch_index **out) try {
    if (!refs || !out || (n_devices && !devices)) return hfail(FH_ERR_INVALID, "null argument");
    if (int rc = check_entry_count(n_devices)) return rc;
    const std::vector<Sketch> &Rs = refs->v;
    if (int rc = check_ascending(Rs, "reference")) return rc;
    auto ix = std::make_unique<finch_index>();
    ix->nr = (uint32_t)Rs.size();
    for (const Sketch &s : Rs) ix->postings += s.hashes.size(), ix->rlen.push_back((uint32_t)s.hashes.size());
    const uint64_t max_postings = index_max_postings();
    if (ix->postings > max_postings)
        return hfail(FH_ERR_UNSUPPORTED, "reference library: %llu postings (hashes of all %u sketches), an index holds at most %llu",
                     (unsigned long long)ix->postings, ix->nr, (unsigned long long)max_postings);
    DistCsr rc_;
    rc_.build(Rs, false);
    ix->rflag = rc_.flags, ix->rmax = rc_.max_hash, ix->rscale = rc_.scale;
    ix->devs = n_devices ? std::vector<int>(devices, devices + n_devices) : std::vector<int>{0};
    ix->has_chunk_opt = fh::cfg("index_chunk_queries") != nullptr;
    ix->chunk_opt = cfg_u64("index_chunk_queries", 0);
    if (ix->postings == 0) { // no reference has a hash: no pair shares one
        *out = ix.release();
        return FH_OK;
    }
    std::vector<int> devs;
    if (int rc = resolve_devices(devices, n_devices, devs)) return rc;
    DeviceGuard restore_device;

    ix->chunk = index_chunk_for(*ix, ix->nr);
    for (int d : devs) {
        fh::IndexDevice *dev = nullptr;
        uint64_t bytes = 0;
        double ms = 0.;
        if (int rc = fh::index_open(d, rc_.view(), ix->chunk, &dev, &bytes, &ms)) return hfail(rc, "%s", fh_last_error());
        ix->entries.push_back(dev);
        ix->device_bytes += bytes;
        ix->build_ms += ms;
    }
    *out = ix.release();
    return FH_OK;
} FINCH_CATCH

int finch_index_search(const finch_index *cix, const finch_sketches *queries, double min_containment, uint32_t top_n,
                       finch_search_result **out) try {
    if (!cix || !queries || !out) return hfail(FH_ERR_INVALID, "null argument");
    finch_index *ix = const_cast<finch_index *>(cix); // (the launch state is the index's; `mu` serialises its use)
    std::lock_guard<std::mutex> one_search(ix->mu);   // (from here: finch_index_add / finch_index_keep change what is read below)
    if (min_containment <= 0.)
        return hfail(FH_ERR_INVALID, "finch_index_search: min_containment %g: an index finds only the pairs that share a hash, and a threshold "
                                     "<= 0 keeps every pair -- use finch_search", min_containment);
    const std::vector<Sketch> &Qs = queries->v;
    if (int rc = check_ascending(Qs, "query")) return rc;
    const uint32_t nq = (uint32_t)Qs.size();
    auto res = std::make_unique<finch_search_result>();
    res->from_index = true;
    res->offsets.assign((size_t)nq + 1, 0);
    if (nq == 0 || ix->entries.empty()) {
        *out = res.release();
        return FH_OK;
    }
    DeviceGuard restore_device;

    DistCsr qc;
    qc.build(Qs, false);
    const uint32_t n_chunks = (nq + ix->chunk - 1) / ix->chunk;
    const uint32_t n_entries = (uint32_t)std::min<size_t>(ix->entries.size(), n_chunks);
    std::vector<std::vector<SearchCand>> found(n_chunks);
    fh::EntryError err;
    std::mutex stat_mu;

    // one thread per device entry: chunks of queries e, e + n_entries, ...
    fh::for_entries(n_entries, err, FH_ERR_CAPACITY, [&](unsigned e) {
        std::vector<uint32_t> ent;
        double ms_sum = 0.;
        uint64_t touched = 0, copied = 0, launches = 0;
        for (uint32_t k = e; k < n_chunks && !err.failed(); k += n_entries) {
            const uint32_t q0 = k * ix->chunk, q1 = (uint32_t)std::min<uint64_t>(nq, (uint64_t)q0 + ix->chunk);
            ent.clear();
            if (entry_failed(err, fh::index_search_chunk(ix->entries[e], qc.view(), q0, q1, min_containment, &ent, &touched, &ms_sum))) break;
            static_assert(sizeof(SearchCand) == 5 * sizeof(uint32_t), "the device's entry");
            found[k].resize(ent.size() / 5);
            if (!ent.empty()) memcpy(found[k].data(), ent.data(), ent.size() * sizeof(uint32_t));
            copied += found[k].size();
            ++launches;
        }
        std::lock_guard<std::mutex> g(stat_mu);
        res->kernel_ms += ms_sum;
        res->launches += launches;
        res->copied += copied;
        res->touched += touched;
    });
    if (err.failed()) return hfail(err.rc(), "%s", err.msg().c_str());
    if (int rc = search_finish(found, Qs, ix->nr, top_n, res.get())) return rc;
    *out = res.release();
    return FH_OK;
} FINCH_CATCH

int finch_index_stats(const finch_index *ix, uint64_t *n_refs, uint64_t *postings, uint64_t *device_bytes, double *build_kernel_ms) try {
    if (!ix) return hfail(FH_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> g(ix->mu);
    if (n_refs) *n_refs = ix->nr;
    if (postings) *postings = ix->postings;
    if (device_bytes) *device_bytes = ix->device_bytes;
    if (build_kernel_ms) *build_kernel_ms = ix->build_ms;
    return FH_OK;
} FINCH_CATCH

int finch_index_search_stats(const finch_search_result *r, uint64_t *pairs_touched) try {
    if (!r) return hfail(FH_ERR_INVALID, "null argument");
    if (!r->from_index) return hfail(FH_ERR_INVALID, "finch_index_search_stats: the result was not made by finch_index_search");
    if (pairs_touched) *pairs_touched = r->touched;
    return FH_OK;
} FINCH_CATCH

void finch_index_free(finch_index *ix) { delete ix; }

} // extern "C"

// ---------------------------------------------------------------------------------------------
// finch dist through the index.  A bound below 1 keeps no pair with jaccard 0, and a pair of two non-empty sketches that shares
// no hash has jaccard 0: what is left are the pairs the index enumerates, and the pairs with an empty side, which the host
// makes itself.  The device's finish drops what a conservative jaccard bound drops; every entry that crosses goes through
// finch_dist's own self-skip, distance_from_counts and `<= max_distance`, so the rows are finch_dist's.  DESIGN.md §3.15.
// ---------------------------------------------------------------------------------------------
namespace {

constexpr uint32_t INDEX_DIST_BUCKETS = 64; // the result's parts: ranges of references, each sorted on a thread of its own

// the device's pre-filter for a query of this k: the jaccard at which the distance is max_distance, in real numbers
// x / (2 - x) with x = exp(-k d), lowered by 2^-20 of itself -- some 2^30 ulps, against the few ulps of exp, log and the
// divisions between this figure and distance_from_counts' test
double index_dist_jmin(uint32_t kmer_length, double max_distance) {
    const double x = std::exp(-(double)kmer_length * std::max(max_distance, 0.));
    return x / (2. - x) * (1. - 0x1p-20);
}

// (c, i, j) of raw_counts for a pair with an empty side: nothing is walked, c = 0, and the scale step alone moves the cursor
// of the other side to its first hash not below M
void empty_side_counts(const Sketch &qs, const Sketch &rs, uint64_t &i, uint64_t &j) {
    i = j = 0;
    const double scale = pair_min_scale(qs, rs);
    if (!(scale > 0.)) return;
    const uint64_t m = scale_max_hash(scale);
    auto below = [m](const std::vector<KmerCount> &h) {
        return (uint64_t)(std::lower_bound(h.begin(), h.end(), m, [](const KmerCount &a, uint64_t x) { return a.hash < x; }) - h.begin());
    };
    i = below(qs.hashes), j = below(rs.hashes);
}

} // namespace

extern "C" {

int finch_index_dist(const finch_index *cix, const finch_sketches *refs, const finch_sketches *queries, int old_mode, double max_distance,
                     finch_dist_result **out) try {
    if (!cix || !refs || !out) return hfail(FH_ERR_INVALID, "null argument");
    finch_index *ix = const_cast<finch_index *>(cix); // (the launch state is the index's; `mu` serialises its use)
    std::lock_guard<std::mutex> one_call(ix->mu);     // (from here: finch_index_add / finch_index_keep change what is read below)
    if (max_distance >= 1.)
        return hfail(FH_ERR_INVALID, "finch_index_dist: max_distance %g: an index finds only the pairs that share a hash, and a bound "
                                     ">= 1 keeps every pair -- use finch_dist", max_distance);
    const bool pairwise = queries == nullptr;
    const std::vector<Sketch> &Rs = refs->v, &Qs = pairwise ? refs->v : queries->v;
    uint64_t postings = 0;
    for (const Sketch &s : Rs) postings += s.hashes.size();
    if (Rs.size() != ix->nr || postings != ix->postings)
        return hfail(FH_ERR_INVALID, "finch_index_dist: refs has %zu sketches and %llu hashes, the index was built from %u and %llu: "
                                     "refs must be the library of the index", Rs.size(), (unsigned long long)postings, ix->nr,
                     (unsigned long long)ix->postings);
    if (!pairwise)
        if (int rc = check_ascending(Qs, "query")) return rc;
    if (int rc = check_ascending(Rs, "reference")) return rc;
    if (old_mode) { // as finch_dist: old_distance refuses an empty query against a non-empty reference
        bool empty_q = false;
        for (const Sketch &s : Qs) empty_q = empty_q || s.hashes.empty();
        if (empty_q && postings) return hfail(FH_ERR_INVALID, "old_distance: empty query sketch");
    }
    auto res = std::make_unique<finch_dist_result>();
    res->from_index = true;
    for (const Sketch &s : Qs) res->qnames.push_back(s.name);
    for (const Sketch &s : Rs) res->rnames.push_back(s.name);
    const uint32_t nq = (uint32_t)Qs.size(), nr = (uint32_t)Rs.size();
    if (nq == 0 || nr == 0 || !(max_distance >= 0.)) { // (a NaN or negative bound keeps nothing: every distance is in [0, 1])
        *out = res.release();
        return FH_OK;
    }
    std::unordered_map<std::string, uint32_t> ids;
    std::vector<uint32_t> qid(nq), rid(nr);
    for (uint32_t q = 0; q < nq; ++q) qid[q] = ids.emplace(Qs[q].name, (uint32_t)ids.size()).first->second;
    for (uint32_t r = 0; r < nr; ++r) rid[r] = ids.emplace(Rs[r].name, (uint32_t)ids.size()).first->second;

    const uint32_t n_buckets = std::min(nr, INDEX_DIST_BUCKETS), per_bucket = (nr + n_buckets - 1) / n_buckets;
    res->parts.resize(n_buckets);
    // the pair's row from its counts, where it is not skipped and the exact test keeps it
    auto keep = [&](std::vector<std::vector<finch_dist_result::Row>> &parts, uint32_t q, uint32_t r, uint64_t c, uint64_t i, uint64_t j) {
        if (qid[q] == rid[r] && sketch_equal(Qs[q], Rs[r])) return false; // main.rs:324
        finch_dist_result::Row row{q, r, {}};
        distance_from_counts(old_mode != 0, c, old_mode ? Rs[r].hashes.size() : i, j, Qs[q].sketch_params.kmer_length, true, &row.d);
        if (!(row.d.mash_distance <= max_distance)) return false;
        parts[r / per_bucket].push_back(row);
        return true;
    };

    // the pairs with an empty side.  Old mode: jaccard is 0 / 0 exactly where the reference is empty (an empty query has only
    // empty references beside it).  New mode: total = 0 needs c = 0 and both cursors at 0, which a walk over two non-empty
    // sketches never leaves.
    for (uint32_t r = 0; r < nr; ++r)
        if (Rs[r].hashes.empty())
            for (uint32_t q = 0; q < nq; ++q) {
                uint64_t i = 0, j = 0;
                if (!old_mode) empty_side_counts(Qs[q], Rs[r], i, j);
                keep(res->parts, q, r, 0, i, j);
            }
    if (!old_mode)
        for (uint32_t q = 0; q < nq; ++q)
            if (Qs[q].hashes.empty())
                for (uint32_t r = 0; r < nr; ++r)
                    if (!Rs[r].hashes.empty()) {
                        uint64_t i = 0, j = 0;
                        empty_side_counts(Qs[q], Rs[r], i, j);
                        keep(res->parts, q, r, 0, i, j);
                    }

    if (!ix->entries.empty()) { // (a library without a hash: every row is made above)
        DeviceGuard restore_device;

        DistCsr qc;
        if (!pairwise) qc.build(Qs, false); // (the flags of the new mode, as the index has the library's; old mode reads none)
        const fh::DistSide qview = qc.view();
        std::vector<double> jmin(nq);
        for (uint32_t q = 0; q < nq; ++q) jmin[q] = index_dist_jmin(Qs[q].sketch_params.kmer_length, max_distance);
        const uint32_t n_chunks = (nq + ix->chunk - 1) / ix->chunk;
        const uint32_t n_entries = (uint32_t)std::min<size_t>(ix->entries.size(), n_chunks);
        fh::EntryError err;
        std::mutex stat_mu;

        // one thread per device entry: chunks of queries e, e + n_entries, ...
        fh::for_entries(n_entries, err, FH_ERR_CAPACITY, [&](unsigned e) {
            std::vector<uint32_t> ent;
            std::vector<std::vector<finch_dist_result::Row>> mine(n_buckets);
            double ms_sum = 0.;
            uint64_t touched = 0, copied = 0, launches = 0;
            for (uint32_t k = e; k < n_chunks && !err.failed(); k += n_entries) {
                const uint32_t q0 = k * ix->chunk, q1 = (uint32_t)std::min<uint64_t>(nq, (uint64_t)q0 + ix->chunk);
                ent.clear();
                if (entry_failed(err, fh::index_dist_chunk(ix->entries[e], pairwise ? nullptr : &qview, q0, q1, old_mode != 0, jmin.data() + q0,
                                                           &ent, &touched, &ms_sum)))
                    break;
                ++launches;
                copied += ent.size() / 5;
                for (size_t t = 0; t + 5 <= ent.size(); t += 5) {
                    const uint32_t *x = ent.data() + t;
                    if (x[0] < q0 || x[0] >= q1 || x[1] >= nr) {
                        err.fail(FH_ERR_STATE, "index dist: an entry names pair (" + std::to_string(x[0]) + ", " + std::to_string(x[1]) + ")");
                        break;
                    }
                    keep(mine, x[0], x[1], x[2], x[3], x[4]);
                }
            }
            std::lock_guard<std::mutex> g(stat_mu);
            res->kernel_ms += ms_sum;
            res->launches += launches;
            res->copied += copied;
            res->touched += touched;
            for (uint32_t b = 0; b < n_buckets; ++b) {
                std::vector<finch_dist_result::Row> &to = res->parts[b];
                if (to.empty()) to.swap(mine[b]);
                else to.insert(to.end(), mine[b].begin(), mine[b].end());
            }
        });
        if (err.failed()) return hfail(err.rc(), "%s", err.msg().c_str());
    }
    // reference-major, queries ascending inside a reference: a pair has one row at most
    const unsigned T = std::min(n_buckets, DIST_MAX_ENTRIES);
    fork_join(T, [&](unsigned t) {
        for (uint32_t b = t; b < n_buckets; b += T)
            std::sort(res->parts[b].begin(), res->parts[b].end(), [](const finch_dist_result::Row &x, const finch_dist_result::Row &y) {
                return x.r != y.r ? x.r < y.r : x.q < y.q;
            });
    });
    for (const auto &p : res->parts) res->n += p.size();
    *out = res.release();
    return FH_OK;
} FINCH_CATCH

int finch_index_dist_stats(const finch_dist_result *r, uint64_t *pairs_touched, uint64_t *pairs_copied) try {
    if (!r) return hfail(FH_ERR_INVALID, "null argument");
    if (!r->from_index) return hfail(FH_ERR_INVALID, "finch_index_dist_stats: the result was not made by finch_index_dist");
    if (pairs_touched) *pairs_touched = r->touched;
    if (pairs_copied) *pairs_copied = r->copied;
    return FH_OK;
} FINCH_CATCH

} // extern "C"

// ---------------------------------------------------------------------------------------------
// single-linkage clusters of a library (the contract is finch_host.h's comment; not in the reference): a and b are linked when
// (a, b) or (b, a) is a row finch_dist(refs, refs) would keep within max_distance, the name-based self-skip aside;
// labels[v] = the smallest index of v's component.  finch_cluster_host is that sentence on the host, every ordered pair;
// finch_index_cluster goes through the index: the device unites what is surely within the bound in a union-find of its own,
// drops what is surely not, and only the band between crosses to distance_from_counts here.  DESIGN.md §3.20.
// ---------------------------------------------------------------------------------------------
namespace {

// what both calls decide before anything else: -> FH_OK with *trivial set where labels are the identity already
int cluster_check(const char *who, const std::vector<Sketch> &Rs, int old_mode, double max_distance, uint32_t *labels, uint64_t n_labels,
                  uint64_t postings, bool *trivial) {
    if (n_labels != Rs.size())
        return hfail(FH_ERR_INVALID, "%s: n_labels %llu, the library has %zu sketches", who, (unsigned long long)n_labels, Rs.size());
    if (n_labels && !labels) return hfail(FH_ERR_INVALID, "null argument");
    if (int rc = check_ascending(Rs, "reference")) return rc;
    if (old_mode) { // pairwise makes every sketch a query: old_distance refuses an empty query against a non-empty reference
        bool empty_q = false;
        for (const Sketch &s : Rs) empty_q = empty_q || s.hashes.empty();
        if (empty_q && postings) return hfail(FH_ERR_INVALID, "old_distance: empty query sketch");
    }
    for (uint64_t v = 0; v < n_labels; ++v) labels[v] = (uint32_t)v;
    *trivial = Rs.empty() || !(max_distance >= 0.); // (a NaN or negative bound links nothing: every distance is in [0, 1])
    return FH_OK;
}

} // namespace

extern "C" {

int finch_cluster_host(const finch_sketches *refs, int old_mode, double max_distance, uint32_t *labels, uint64_t n_labels,
                       uint64_t *edges) try {
    if (!refs) return hfail(FH_ERR_INVALID, "null argument");
    const std::vector<Sketch> &Rs = refs->v;
    uint64_t postings = 0;
    for (const Sketch &s : Rs) postings += s.hashes.size();
    bool trivial = false;
    if (int rc = cluster_check("finch_cluster_host", Rs, old_mode, max_distance, labels, n_labels, postings, &trivial)) return rc;
    if (edges) *edges = 0;
    if (trivial) return FH_OK;
    const uint32_t nr = (uint32_t)Rs.size();
    std::vector<std::vector<uint64_t>> H(nr);
    for (uint32_t s = 0; s < nr; ++s) {
        H[s].reserve(Rs[s].hashes.size());
        for (const KmerCount &h : Rs[s].hashes) H[s].push_back(h.hash);
    }
    fh::cluster::UnionFind uf(nr);
    uint64_t n_edges = 0;
    for (uint32_t r = 0; r < nr; ++r)
        for (uint32_t q = 0; q < nr; ++q) {
            if (q == r) continue;
            uint64_t c = 0, i = 0, j = 0;
            if (old_mode) {
                if (int rc = old_counts(H[q].data(), H[q].size(), H[r].data(), H[r].size(), c, i)) return rc;
            } else {
                raw_counts(H[q].data(), H[q].size(), H[r].data(), H[r].size(), pair_min_scale(Rs[q], Rs[r]), c, i, j);
            }
            finch_distance_out d;
            distance_from_counts(old_mode != 0, c, i, j, Rs[q].sketch_params.kmer_length, true, &d);
            if (!(d.mash_distance <= max_distance)) continue;
            ++n_edges;
            uf.unite(q, r);
        }
    uf.labels(labels);
    if (edges) *edges = n_edges;
    return FH_OK;
} FINCH_CATCH

int finch_index_cluster(const finch_index *cix, const finch_sketches *refs, int old_mode, double max_distance, uint32_t *labels,
                        uint64_t n_labels, finch_cluster_stats *stats) try {
    if (!cix || !refs) return hfail(FH_ERR_INVALID, "null argument");
    finch_index *ix = const_cast<finch_index *>(cix); // (the launch state is the index's; `mu` serialises its use)
    std::lock_guard<std::mutex> one_call(ix->mu);     // (from here: finch_index_add / finch_index_keep change what is read below)
    if (max_distance >= 1.)
        return hfail(FH_ERR_INVALID, "finch_index_cluster: max_distance %g: an index finds only the pairs that share a hash, and every "
                                     "pair is within a bound >= 1 -- the library is one cluster", max_distance);
    double margin = 0.;
    if (!fh::cluster::margin_parse(fh::cfg("index_cluster_margin"), &margin))
        return hfail(FH_ERR_INVALID, "finch_index_cluster: option index_cluster_margin = %s: a number in [2^-20, 0.5] (nothing sweeps the "
                                     "bands' soundness below 2^-20)", fh::cfg("index_cluster_margin"));
    const std::vector<Sketch> &Rs = refs->v;
    uint64_t postings = 0;
    for (const Sketch &s : Rs) postings += s.hashes.size();
    if (Rs.size() != ix->nr || postings != ix->postings)
        return hfail(FH_ERR_INVALID, "finch_index_cluster: refs has %zu sketches and %llu hashes, the index was built from %u and %llu: "
                                     "refs must be the library of the index", Rs.size(), (unsigned long long)postings, ix->nr,
                     (unsigned long long)ix->postings);
    bool trivial = false;
    if (int rc = cluster_check("finch_index_cluster", Rs, old_mode, max_distance, labels, n_labels, postings, &trivial)) return rc;
    finch_cluster_stats st{};
    st.clusters = n_labels;
    if (trivial) {
        if (stats) *stats = st;
        return FH_OK;
    }
    const uint32_t nr = (uint32_t)Rs.size();
    fh::cluster::UnionFind uf(nr);
    fh::cluster::Edges count;
    // the exact test of an ordered pair q != r from its counts: finch_dist's function and comparison
    auto passes = [&](uint32_t q, uint32_t r, uint64_t c, uint64_t i, uint64_t j) {
        finch_distance_out d;
        distance_from_counts(old_mode != 0, c, old_mode ? Rs[r].hashes.size() : i, j, Rs[q].sketch_params.kmer_length, true, &d);
        return d.mash_distance <= max_distance;
    };

    // the pairs with an empty side, host-made as finch_index_dist makes them
    for (uint32_t r = 0; r < nr; ++r)
        if (Rs[r].hashes.empty())
            for (uint32_t q = 0; q < nr; ++q) {
                if (q == r) continue;
                uint64_t i = 0, j = 0;
                if (!old_mode) empty_side_counts(Rs[q], Rs[r], i, j);
                if (passes(q, r, 0, i, j)) ++count.empty_side, uf.unite(q, r);
            }
    if (!old_mode)
        for (uint32_t q = 0; q < nr; ++q)
            if (Rs[q].hashes.empty())
                for (uint32_t r = 0; r < nr; ++r)
                    if (!Rs[r].hashes.empty()) {
                        uint64_t i = 0, j = 0;
                        empty_side_counts(Rs[q], Rs[r], i, j);
                        if (passes(q, r, 0, i, j)) ++count.empty_side, uf.unite(q, r);
                    }

    if (!ix->entries.empty()) { // (a library without a hash: every edge is made above)
        DeviceGuard restore_device;

        std::vector<double> jlo(nr), jhi(nr);
        for (uint32_t q = 0; q < nr; ++q) {
            jlo[q] = index_dist_jmin(Rs[q].sketch_params.kmer_length, max_distance); // (== fh::cluster::jlo)
            jhi[q] = fh::cluster::jhi(Rs[q].sketch_params.kmer_length, max_distance, margin);
        }
        const uint32_t n_chunks = (nr + ix->chunk - 1) / ix->chunk;
        const uint32_t n_entries = (uint32_t)std::min<size_t>(ix->entries.size(), n_chunks);
        fh::EntryError err;
        std::mutex stat_mu;
        struct Pair {
            uint32_t a, b;
        };

        // one thread per device entry: chunks of queries e, e + n_entries, ...; the entry's union-find lives through them
        fh::for_entries(n_entries, err, FH_ERR_CAPACITY, [&](unsigned e) {
            fh::IndexDevice *d = ix->entries[e];
            std::vector<uint32_t> ent, lab;
            std::vector<Pair> kept;
            double ms_sum = 0.;
            uint64_t touched = 0, copied = 0, kept_host = 0, launches = 0, united = 0;
            bool ok = !entry_failed(err, fh::index_cluster_begin(d));
            for (uint32_t k = e; ok && k < n_chunks && !err.failed(); k += n_entries) {
                const uint32_t q0 = k * ix->chunk, q1 = (uint32_t)std::min<uint64_t>(nr, (uint64_t)q0 + ix->chunk);
                ent.clear();
                if (entry_failed(err, fh::index_cluster_chunk(d, q0, q1, old_mode != 0, jlo.data() + q0, jhi.data() + q0, &ent, &touched, &ms_sum))) {
                    ok = false;
                    break;
                }
                ++launches;
                copied += ent.size() / 5;
                for (size_t t = 0; t + 5 <= ent.size(); t += 5) {
                    const uint32_t *x = ent.data() + t;
                    if (x[0] < q0 || x[0] >= q1 || x[1] >= nr) {
                        err.fail(FH_ERR_STATE, "index cluster: an entry names pair (" + std::to_string(x[0]) + ", " + std::to_string(x[1]) + ")");
                        ok = false;
                        break;
                    }
                    if (x[0] != x[1] && passes(x[0], x[1], x[2], x[3], x[4])) ++kept_host, kept.push_back(Pair{x[0], x[1]});
                }
            }
            ok = ok && !err.failed();
            if (ok) lab.resize(nr);
            if (entry_failed(err, fh::index_cluster_end(d, ok ? lab.data() : nullptr, &united, &ms_sum))) ok = false;
            std::lock_guard<std::mutex> g(stat_mu);
            st.kernel_ms += ms_sum;
            st.launches += launches;
            st.pairs_touched += touched;
            count.copied += copied;
            count.kept_host += kept_host;
            count.united += united;
            if (!ok) return;
            for (uint32_t v = 0; v < nr; ++v) {
                if (lab[v] > v) {
                    err.fail(FH_ERR_STATE, "index cluster: reference " + std::to_string(v) + " has label " + std::to_string(lab[v]));
                    return;
                }
                uf.unite(v, lab[v]);
            }
            for (const Pair &p : kept) uf.unite(p.a, p.b);
        });
        if (err.failed()) return hfail(err.rc(), "%s", err.msg().c_str());
    }
    st.clusters = uf.labels(labels);
    st.pairs_united = count.united, st.pairs_copied = count.copied, st.pairs_kept_host = count.kept_host, st.edges = count.edges();
    if (stats) *stats = st;
    return FH_OK;
} FINCH_CATCH

} // extern "C"

// ---------------------------------------------------------------------------------------------
// gather: the greedy decomposition of a query over a library (the contract is finch_host.h's comment; not in the reference).
// Plain set semantics over the hashes as stored -- deliberately not raw_distance's walk.  finch_gather_query is the loop as the
// contract reads, on the host; finch_gather keeps the loop on the device (fh_gather.hip): the candidate list and the records
// come here, to be put in order and given their doubles by the function the host loop uses.  DESIGN.md §3.13.
// ---------------------------------------------------------------------------------------------
struct finch_gather_result {
    std::vector<uint64_t> offsets; // n_queries + 1
    std::vector<finch_gather_row> rows;
    double kernel_ms = 0.;
    uint64_t launches = 0, candidates = 0, copied = 0;
    bool from_index = false; // made by finch_index_gather: `touched` = the pairs its device counted
    uint64_t touched = 0;
};

namespace {

// the five doubles of a row from its integers and the sum of all of the query's counts: plain IEEE divisions, nothing guarded
void gather_row_doubles(finch_gather_row *row, uint64_t query_count_sum) {
    row->f_unique_to_query = (double)row->overlap / (double)row->query_len;
    row->f_orig_query = (double)row->common / (double)row->query_len;
    row->f_match = (double)row->common / (double)row->ref_len;
    row->average_abund = (double)row->abund / (double)row->overlap;
    row->f_unique_weighted = (double)row->abund / (double)query_count_sum;
}

uint64_t gather_count_sum(const Sketch &q) {
    uint64_t s = 0;
    for (const KmerCount &h : q.hashes) s += h.count;
    return s;
}

// what both entry points make of their arguments: min_overlap below 1 is 1; no sketch has 2^32 - 1 hashes, so neither number
// means anything else above that
uint32_t gather_clamp(uint64_t v, uint64_t least) { return (uint32_t)std::min<uint64_t>(std::max(v, least), UINT32_MAX); }

int gather_check_ascending(const Sketch &s, const char *what, size_t idx) {
    const std::vector<KmerCount> &h = s.hashes;
    for (size_t j = 1; j < h.size(); ++j)
        if (!(h[j - 1].hash < h[j].hash))
            return hfail(FH_ERR_INVALID, "%s sketch %zu (%s): hashes not strictly ascending at %zu", what, idx, s.name.c_str(), j);
    return FH_OK;
}

// the contract's loop for one query: `in` marks S_t over the query's positions; c_j(t) and the sum of counts by looking every
// hash of H_j up in Q
void gather_on_host(const std::vector<Sketch> &Rs, const Sketch &Q, uint32_t iq, uint32_t min_overlap, uint32_t max_rounds,
                    std::vector<finch_gather_row> &rows) {
    const std::vector<KmerCount> &q = Q.hashes;
    std::vector<uint8_t> in(q.size(), 1);
    auto walk = [&](const Sketch &R, bool remove, uint64_t *abund) {
        uint64_t c = 0;
        for (const KmerCount &x : R.hashes) {
            auto it = std::lower_bound(q.begin(), q.end(), x.hash, [](const KmerCount &a, uint64_t h) { return a.hash < h; });
            if (it == q.end() || it->hash != x.hash || !in[it - q.begin()]) continue;
            ++c;
            if (abund) *abund += it->count;
            if (remove) in[it - q.begin()] = 0;
        }
        return c;
    };
    std::vector<uint64_t> c0(Rs.size());
    const uint64_t count_sum = gather_count_sum(Q);
    uint64_t remaining = q.size();
    for (uint64_t t = 0; max_rounds == 0 || t < max_rounds; ++t) {
        uint64_t best = 0;
        size_t w = 0;
        for (size_t j = 0; j < Rs.size(); ++j) {
            const uint64_t c = walk(Rs[j], false, nullptr);
            if (t == 0) c0[j] = c;
            if (c > best) best = c, w = j; // (among equal counts the smallest j)
        }
        if (best < min_overlap) break;
        finch_gather_row row{};
        row.query = iq, row.reference = w, row.round = t, row.overlap = best, row.common = c0[w];
        row.ref_len = Rs[w].hashes.size(), row.query_len = q.size();
        walk(Rs[w], true, &row.abund);
        remaining -= best;
        row.remaining = remaining;
        gather_row_doubles(&row, count_sum);
        rows.push_back(row);
    }
}

constexpr uint64_t GATHER_POS_BYTES = 1ull << 30; // a chunk's position arrays: a design choice, not a measurement

// what finch_gather and finch_index_gather do with the records a launch left for the queries [q0, q1) (the device's numbering):
// each is checked against the candidates -- query q's are cands[first[q - first_q] .. first[q - first_q + 1]), by reference -- and
// becomes the row of its round in rows_of[caller's index] (mine: the device's numbering -> the caller's; nullptr: the same).
// A message where a record is not what the candidates allow.
std::string gather_place_records(const std::vector<fh::GatherRecord> &recs, uint32_t q0, uint32_t q1, const fh::GatherCand *cands,
                                 const uint64_t *first, uint32_t first_q, const uint32_t *mine,
                                 std::vector<std::vector<finch_gather_row>> &rows_of) {
    for (const fh::GatherRecord &x : recs) {
        const bool in = x.q >= q0 && x.q < q1;
        const uint64_t nc = in ? first[x.q - first_q + 1] - first[x.q - first_q] : 0;
        if (x.round >= nc || x.cand >= nc || cands[first[x.q - first_q] + x.cand].r != x.r)
            return "gather: a record of query " + std::to_string(x.q) + ", round " + std::to_string(x.round);
        std::vector<finch_gather_row> &to = rows_of[mine ? mine[x.q] : x.q];
        if (to.size() <= x.round) to.resize((size_t)x.round + 1, finch_gather_row{0, 0, UINT64_MAX, 0, 0, 0, 0, 0, 0, 0., 0., 0., 0., 0.});
        finch_gather_row &row = to[x.round];
        if (row.round != UINT64_MAX) return "gather: two records of query " + std::to_string(x.q) + ", round " + std::to_string(x.round);
        row.query = mine ? mine[x.q] : x.q, row.reference = x.r, row.round = x.round, row.overlap = x.overlap, row.common = x.common;
        row.ref_len = x.ref_len, row.query_len = x.query_len, row.abund = x.abund, row.remaining = x.remaining;
    }
    return std::string();
}

// ... and with every query's rows once all records are placed: the offsets, the doubles, the rows in query order
int gather_finish(std::vector<std::vector<finch_gather_row>> &rows_of, const std::vector<Sketch> &Qs, finch_gather_result *res) {
    const uint32_t nq = (uint32_t)Qs.size();
    for (uint32_t q = 0; q < nq; ++q) res->offsets[q + 1] = res->offsets[q] + rows_of[q].size();
    res->rows.reserve(res->offsets[nq]);
    for (uint32_t q = 0; q < nq; ++q) {
        const uint64_t count_sum = gather_count_sum(Qs[q]);
        for (finch_gather_row &row : rows_of[q]) {
            if (row.round == UINT64_MAX) return hfail(FH_ERR_STATE, "gather: query %u has a round without a record", q);
            gather_row_doubles(&row, count_sum);
            res->rows.push_back(row);
        }
    }
    return FH_OK;
}

// finch_gather's refusal of a query the rounds kernels' LDS mask cannot hold, finch_index_gather's too
int gather_check_query_lengths(const std::vector<Sketch> &Qs) {
    for (size_t q = 0; q < Qs.size(); ++q)
        if (Qs[q].hashes.size() > fh::GATHER_MAX_QUERY)
            return hfail(FH_ERR_UNSUPPORTED, "query sketch %zu (%s) has %zu hashes (a gather takes at most %u: one bit each in the rounds kernel's LDS)",
                         q, Qs[q].name.c_str(), Qs[q].hashes.size(), fh::GATHER_MAX_QUERY);
    return FH_OK;
}

} // namespace

extern "C" {

int finch_gather_query(const finch_sketches *refs, const finch_sketches *queries, uint32_t iq, uint64_t min_overlap, uint64_t max_rounds,
                       finch_gather_row *rows, uint64_t cap, uint64_t *n) try {
    if (!refs || !queries || !n || (cap && !rows)) return hfail(FH_ERR_INVALID, "null argument");
    if (iq >= queries->v.size()) return hfail(FH_ERR_INVALID, "query sketch %u of %zu sketches", iq, queries->v.size());
    if (int rc = gather_check_ascending(queries->v[iq], "query", iq)) return rc;
    for (size_t j = 0; j < refs->v.size(); ++j)
        if (int rc = gather_check_ascending(refs->v[j], "reference", j)) return rc;
    std::vector<finch_gather_row> out;
    gather_on_host(refs->v, queries->v[iq], iq, gather_clamp(min_overlap, 1), gather_clamp(max_rounds, 0), out);
    for (size_t i = 0; i < out.size() && i < cap; ++i) rows[i] = out[i];
    *n = out.size();
    return FH_OK;
} FINCH_CATCH

int finch_gather(const finch_sketches *queries, const finch_sketches *refs, uint64_t min_overlap, uint64_t max_rounds, const int *devices,
                 uint32_t n_devices, finch_gather_result **out) try {
    if (!queries || !refs || !out || (n_devices && !devices)) return hfail(FH_ERR_INVALID, "null argument");
    if (int rc = check_entry_count(n_devices)) return rc;
    const std::vector<Sketch> &Qs = queries->v, &Rs = refs->v;
    if (int rc = check_ascending(Qs, "query")) return rc;
    if (int rc = check_ascending(Rs, "reference")) return rc;
    if (int rc = gather_check_query_lengths(Qs)) return rc;
    const uint32_t nq = (uint32_t)Qs.size(), nr = (uint32_t)Rs.size();
    auto res = std::make_unique<finch_gather_result>();
    res->offsets.assign((size_t)nq + 1, 0);
    if (nq == 0 || nr == 0) {
        *out = res.release();
        return FH_OK;
    }
    std::vector<int> devs;
    if (int rc = resolve_devices(devices, n_devices, devs)) return rc;
    DeviceGuard restore_device;

    const uint32_t min_ov = gather_clamp(min_overlap, 1), max_r = gather_clamp(max_rounds, 0);
    const uint32_t n_entries = (uint32_t)std::min<size_t>(devs.size(), nq); // (an entry without a query opens nothing)
    const uint32_t dist_slice = (uint32_t)std::min<uint64_t>(cfg_u64("dist_slice", 4096), UINT32_MAX);
    const uint32_t gather_slice = (uint32_t)std::min<uint64_t>(cfg_u64("gather_slice", fh::GATHER_MAX_SLICE), UINT32_MAX);
    const uint64_t pos_bytes = cfg_u64("gather_pos_bytes", GATHER_POS_BYTES);
    DistCsr rc_; // the references once, for every entry
    rc_.build(Rs, false);
    std::vector<std::vector<finch_gather_row>> rows_of(nq);
    fh::EntryError err;
    std::mutex stat_mu;

    // one thread per device entry: the queries e, e + n_entries, ...
    fh::for_entries(n_entries, err, FH_ERR_CAPACITY, [&](unsigned e) {
        fh::GatherDevice *gd = nullptr;
        fh::Finally close_gd{[&] { fh::gather_close(gd); }};
        std::vector<uint32_t> mine; // local query -> the caller's index
        for (uint32_t q = e; q < nq; q += n_entries) mine.push_back(q);
        const uint32_t nqe = (uint32_t)mine.size();
        std::vector<uint64_t> qh, qoff(1, 0);
        std::vector<uint32_t> qcnt;
        {
            size_t total = 0;
            for (uint32_t q : mine) total += Qs[q].hashes.size();
            qh.reserve(total);
            qcnt.reserve(total);
            qoff.reserve((size_t)nqe + 1);
        }
        for (uint32_t q : mine) {
            for (const KmerCount &h : Qs[q].hashes) qh.push_back(h.hash), qcnt.push_back(h.count);
            qoff.push_back(qh.size());
        }
        const uint32_t per_chunk = chunk_refs("dist_chunk_pairs", DIST_CHUNK_PAIRS, nqe, nr, true);
        if ((uint64_t)per_chunk * nqe > (1ull << 31)) { // (per_chunk = 1 here: more than 2^31 queries on one entry)
            err.fail(FH_ERR_UNSUPPORTED, "a device entry has " + std::to_string(nqe) + " queries: more than 2^31 pairs per reference");
            return;
        }
        const fh::GatherSide qside{qh.data(), qcnt.data(), qoff.data(), nqe}, rside{rc_.hashes.data(), nullptr, rc_.offsets.data(), nr};
        if (entry_failed(err, fh::gather_open(devs[e], qside, rside, dist_slice, gather_slice, (uint64_t)per_chunk * nqe, min_ov, &gd))) return;
        double ms = 0.;
        uint64_t launches = 0, copied = 0;
        int rc = FH_OK;
        // 1. the candidates of every query of this entry, reference chunk by reference chunk
        std::vector<fh::GatherCand> cands;
        for (uint32_t r0 = 0; rc == FH_OK && r0 < nr && !err.failed(); r0 += per_chunk)
            rc = fh::gather_count(gd, r0, std::min(nr, r0 + per_chunk), &cands, &ms, &launches);
        if (entry_failed(err, rc) || err.failed()) return;
        for (const fh::GatherCand &c : cands)
            if (c.q >= nqe || c.r >= nr) {
                err.fail(FH_ERR_STATE, "gather: candidate (" + std::to_string(c.q) + ", " + std::to_string(c.r) + ")");
                return;
            }
        std::sort(cands.begin(), cands.end(), [](const fh::GatherCand &a, const fh::GatherCand &b) { return a.q < b.q || (a.q == b.q && a.r < b.r); });
        std::vector<uint64_t> first((size_t)nqe + 1, 0), need(nqe, 0); // each query's candidates, the bytes of their positions
        for (const fh::GatherCand &c : cands) ++first[c.q + 1], need[c.q] += (uint64_t)c.common * sizeof(uint32_t);
        for (uint32_t q = 0; q < nqe; ++q) first[q + 1] += first[q];
        for (uint32_t q = 0; q < nqe; ++q)
            if (need[q] > pos_bytes) {
                char msg[512];
                snprintf(msg, sizeof msg, "query sketch %u (%s): the positions of its %llu candidates take %llu bytes (option gather_pos_bytes: %llu)",
                         mine[q], Qs[mine[q]].name.c_str(), (unsigned long long)(first[q + 1] - first[q]), (unsigned long long)need[q],
                         (unsigned long long)pos_bytes);
                err.fail(FH_ERR_UNSUPPORTED, msg);
                return;
            }
        // 2. chunks of queries whose position arrays fit the budget: positions, then every round, one launch each
        std::vector<fh::GatherRecord> recs;
        for (uint32_t q0 = 0; q0 < nqe && !err.failed();) {
            uint32_t q1 = q0;
            uint64_t bytes = 0;
            while (q1 < nqe && (q1 == q0 || (bytes + need[q1] <= pos_bytes && first[q1 + 1] - first[q0] < (1ull << 30)))) bytes += need[q1++];
            const uint64_t n = first[q1] - first[q0];
            recs.clear();
            if (n && entry_failed(err, fh::gather_rounds(gd, q0, q1, cands.data() + first[q0], n, max_r, &recs, &ms, &launches))) break;
            copied += recs.size();
            // the records of the chunk, each at its round
            const std::string bad = gather_place_records(recs, q0, q1, cands.data(), first.data(), 0, mine.data(), rows_of);
            if (!bad.empty()) err.fail(FH_ERR_STATE, bad);
            q0 = q1;
        }
        std::lock_guard<std::mutex> g(stat_mu);
        res->kernel_ms += ms;
        res->launches += launches;
        res->candidates += cands.size();
        res->copied += copied;
    });
    if (err.failed()) return hfail(err.rc(), "%s", err.msg().c_str());
    if (int rc = gather_finish(rows_of, Qs, res.get())) return rc;
    *out = res.release();
    return FH_OK;
} FINCH_CATCH

// the same decomposition through the library index (fh_index.hip): the index's count leaves |Q n H_r| of every
// pair that shares a hash, the rounds keep those counters live, and the records come through finch_gather's own finish.
int finch_index_gather(const finch_index *cix, const finch_sketches *queries, uint64_t min_overlap, uint64_t max_rounds,
                       finch_gather_result **out) try {
    if (!cix || !queries || !out) return hfail(FH_ERR_INVALID, "null argument");
    finch_index *ix = const_cast<finch_index *>(cix); // (the launch state is the index's; `mu` serialises its use)
    std::lock_guard<std::mutex> one_call(ix->mu);     // (from here: finch_index_add / finch_index_keep change what is read below)
    const std::vector<Sketch> &Qs = queries->v;
    if (int rc = check_ascending(Qs, "query")) return rc;
    if (int rc = gather_check_query_lengths(Qs)) return rc;
    const uint32_t nq = (uint32_t)Qs.size();
    auto res = std::make_unique<finch_gather_result>();
    res->from_index = true;
    res->offsets.assign((size_t)nq + 1, 0);
    if (nq == 0 || ix->entries.empty()) {
        *out = res.release();
        return FH_OK;
    }
    DeviceGuard restore_device;

    const uint32_t min_ov = gather_clamp(min_overlap, 1), max_r = gather_clamp(max_rounds, 0);
    DistCsr qc;
    qc.build(Qs, false, true);
    const uint32_t n_chunks = (nq + ix->chunk - 1) / ix->chunk;
    const uint32_t n_entries = (uint32_t)std::min<size_t>(ix->entries.size(), n_chunks);
    std::vector<std::vector<finch_gather_row>> rows_of(nq); // (a chunk's queries are its own: no two threads share a row list)
    fh::EntryError err;
    std::mutex stat_mu;

    // one thread per device entry: chunks of queries e, e + n_entries, ...
    fh::for_entries(n_entries, err, FH_ERR_CAPACITY, [&](unsigned e) {
        std::vector<fh::GatherCand> cands;
        std::vector<fh::GatherRecord> recs;
        std::vector<uint64_t> first;
        double ms_sum = 0.;
        uint64_t touched = 0, n_cands = 0, copied = 0, launches = 0;
        for (uint32_t k = e; k < n_chunks && !err.failed(); k += n_entries) {
            const uint32_t q0 = k * ix->chunk, q1 = (uint32_t)std::min<uint64_t>(nq, (uint64_t)q0 + ix->chunk);
            if (entry_failed(err, fh::index_gather_chunk(ix->entries[e], qc.view(), qc.counts.data(), q0, q1, min_ov, max_r, &cands, &recs,
                                                         &touched, &ms_sum, &launches)))
                break;
            n_cands += cands.size();
            copied += recs.size();
            first.assign((size_t)(q1 - q0) + 1, 0); // each query's candidates: the list is sorted by (q, r), q in [q0, q1)
            for (const fh::GatherCand &c : cands) ++first[c.q - q0 + 1];
            for (uint32_t b = 0; b < q1 - q0; ++b) first[b + 1] += first[b];
            const std::string bad = gather_place_records(recs, q0, q1, cands.data(), first.data(), q0, nullptr, rows_of);
            if (!bad.empty()) err.fail(FH_ERR_STATE, bad);
        }
        std::lock_guard<std::mutex> g(stat_mu);
        res->kernel_ms += ms_sum;
        res->launches += launches;
        res->candidates += n_cands;
        res->copied += copied;
        res->touched += touched;
    });
    if (err.failed()) return hfail(err.rc(), "%s", err.msg().c_str());
    if (int rc = gather_finish(rows_of, Qs, res.get())) return rc;
    *out = res.release();
    return FH_OK;
} FINCH_CATCH

int finch_index_gather_stats(const finch_gather_result *r, uint64_t *pairs_touched) try {
    if (!r) return hfail(FH_ERR_INVALID, "null argument");
    if (!r->from_index) return hfail(FH_ERR_INVALID, "finch_index_gather_stats: the result was not made by finch_index_gather");
    if (pairs_touched) *pairs_touched = r->touched;
    return FH_OK;
} FINCH_CATCH

uint64_t finch_gather_len(const finch_gather_result *r) { return r ? r->rows.size() : 0; }

int finch_gather_offsets(const finch_gather_result *r, uint64_t *offsets) try {
    if (!r || !offsets) return hfail(FH_ERR_INVALID, "null argument");
    memcpy(offsets, r->offsets.data(), r->offsets.size() * sizeof(uint64_t));
    return FH_OK;
} FINCH_CATCH

int finch_gather_copy(const finch_gather_result *r, uint32_t *query_idx, uint32_t *ref_idx, finch_gather_row *rows) try {
    if (!r) return hfail(FH_ERR_INVALID, "null argument");
    const size_t n = r->rows.size();
    for (size_t i = 0; i < n; ++i) {
        if (query_idx) query_idx[i] = (uint32_t)r->rows[i].query;
        if (ref_idx) ref_idx[i] = (uint32_t)r->rows[i].reference;
    }
    if (rows && n) memcpy(rows, r->rows.data(), n * sizeof(finch_gather_row));
    return FH_OK;
} FINCH_CATCH

int finch_gather_stats(const finch_gather_result *r, double *kernel_ms, uint64_t *launches, uint64_t *candidates, uint64_t *records_copied) try {
    if (!r) return hfail(FH_ERR_INVALID, "null argument");
    if (kernel_ms) *kernel_ms = r->kernel_ms;
    if (launches) *launches = r->launches;
    if (candidates) *candidates = r->candidates;
    if (records_copied) *records_copied = r->copied;
    return FH_OK;
} FINCH_CATCH

void finch_gather_free(finch_gather_result *r) { delete r; }

} // extern "C"

// ---------------------------------------------------------------------------------------------
// compare_counts (Sketch.compare_counts, lib/src/python.rs:496-559): the merge walk with the summed counts of the shared hashes
// and the moment recurrence over the query's counts of them.  finch_compare_counts_pair is the reference's loop as written, on
// the host; finch_compare_counts gets the integers and m2, m3, m4 of many pairs from the device (fh_moments.hip), sorts the
// records and finishes the three doubles with the function the pair call uses.  DESIGN.md §3.11.
// ---------------------------------------------------------------------------------------------
struct finch_compare_counts_result {
    std::vector<uint32_t> q, r;
    std::vector<finch_count_moments> rows;
    double kernel_ms = 0.;
    uint64_t launches = 0, copied = 0;
    bool from_index = false; // made by finch_index_compare_counts: `touched` = the pairs its device counted
    uint64_t touched = 0;
};

namespace {

// The recurrence and the finishing doubles are IEEE arithmetic as written, with no fused multiply-add: baseline x86-64 has
// none, and where a build targets a machine that has, these two functions still do not contract.
#if defined(__clang__)
#define FH_NO_CONTRACT_ATTR
#define FH_NO_CONTRACT_BODY _Pragma("clang fp contract(off)")
#elif defined(__GNUC__)
#define FH_NO_CONTRACT_ATTR __attribute__((optimize("fp-contract=off")))
#define FH_NO_CONTRACT_BODY
#else
#define FH_NO_CONTRACT_ATTR
#define FH_NO_CONTRACT_BODY
#endif

// python.rs:545-547
FH_NO_CONTRACT_ATTR void moments_finish(uint64_t common, double m2, double m3, double m4, finch_count_moments *out) {
    FH_NO_CONTRACT_BODY
    const double c = (double)common;
    out->var = m2 / c;
    out->skew = std::sqrt(c) * m3 / std::pow(m2, 1.5);
    out->kurt = c * m4 / (m2 * m2) - 3.;
}

// python.rs:500-559, statement by statement
FH_NO_CONTRACT_ATTR void compare_counts_walk(const std::vector<KmerCount> &reference, const std::vector<KmerCount> &query,
                                             finch_count_moments *out) {
    FH_NO_CONTRACT_BODY
    uint64_t common = 0, ref_count = 0, query_count = 0;
    size_t ref_pos = 0, query_pos = 0;
    double query_mean = 0., query_m2 = 0., query_m3 = 0., query_m4 = 0.;
    while (ref_pos < reference.size() && query_pos < query.size()) {
        if (reference[ref_pos].hash < query[query_pos].hash) {
            ref_pos += 1;
        } else if (query[query_pos].hash < reference[ref_pos].hash) {
            query_pos += 1;
        } else {
            ref_count += (uint64_t)reference[ref_pos].count;
            query_count += (uint64_t)query[query_pos].count;
            const double n = (double)common + 1.;
            const double float_count = (double)query[query_pos].count;
            const double delta = float_count - query_mean;
            const double delta_n = delta / n;
            const double delta_n2 = delta_n * delta_n;
            const double term1 = delta * delta_n * (n - 1.);
            query_mean += delta_n;
            query_m4 += term1 * delta_n2 * (n * n - 3. * n + 3.) + 6. * delta_n2 * query_m2 - 4. * delta_n * query_m3;
            query_m3 += term1 * delta_n * (n - 2.) - 3. * delta_n * query_m2;
            query_m2 += term1;
            ref_pos += 1;
            query_pos += 1;
            common += 1;
        }
    }
    out->common = common;
    out->ref_pos = ref_pos;
    out->query_pos = query_pos;
    out->ref_count = ref_count;
    out->query_count = query_count;
    moments_finish(common, query_m2, query_m3, query_m4, out);
}

// a launch's records and the pairs it covered: queries [q0, q1) x references [r0, r1)
struct MomentsFound {
    std::vector<fh::MomentsRecord> recs;
    uint32_t q0 = 0, q1 = 0, r0 = 0, r1 = 0;
};

// what finch_compare_counts and finch_index_compare_counts do with the records the device left (`found`: lists in any order,
// emptied here): by query, each query's sorted by reference; the three doubles are moments_finish's, as the pair call has them
int compare_counts_finish(std::vector<MomentsFound> &found, uint32_t nq, uint32_t nr, finch_compare_counts_result *res) {
    // the device's lists have no order: the records by query (a counting pass), each query's by reference index
    std::vector<uint64_t> at((size_t)nq + 1, 0);
    for (size_t k = 0; k < found.size(); ++k)
        for (const fh::MomentsRecord &x : found[k].recs) {
            if (x.q < found[k].q0 || x.q >= found[k].q1 || x.r < found[k].r0 || x.r >= found[k].r1)
                return hfail(FH_ERR_STATE, "compare_counts: record (%u, %u) in chunk %zu of %u x %u", x.q, x.r, k, nq, nr);
            ++at[x.q + 1];
        }
    for (uint32_t q = 0; q < nq; ++q) at[q + 1] += at[q];
    const uint64_t total = at[nq];
    std::vector<fh::MomentsRecord> recs(total);
    {
        std::vector<uint64_t> fill(at.begin(), at.end() - 1);
        for (auto &f : found) {
            for (const fh::MomentsRecord &x : f.recs) recs[fill[x.q]++] = x;
            std::vector<fh::MomentsRecord>().swap(f.recs);
        }
    }
    res->q.resize(total);
    res->r.resize(total);
    res->rows.resize(total);
    const unsigned T = (unsigned)std::min<uint64_t>(DIST_MAX_ENTRIES, std::max<uint64_t>(1, total >> 16));
    const uint32_t per = (nq + T - 1) / T;
    fork_join(T, [&](unsigned t) {
        for (uint32_t q = std::min(nq, t * per); q < std::min<uint64_t>(nq, (uint64_t)(t + 1) * per); ++q) {
            std::sort(recs.begin() + at[q], recs.begin() + at[q + 1], [](const fh::MomentsRecord &a, const fh::MomentsRecord &b) { return a.r < b.r; });
            for (uint64_t o = at[q]; o < at[q + 1]; ++o) {
                const fh::MomentsRecord &x = recs[o];
                finch_count_moments &row = res->rows[o];
                res->q[o] = x.q;
                res->r[o] = x.r;
                row.common = x.common;
                row.ref_pos = x.ref_pos;
                row.query_pos = x.query_pos;
                row.ref_count = x.ref_count;
                row.query_count = x.query_count;
                moments_finish(x.common, x.m2, x.m3, x.m4, &row);
            }
        }
    });
    return FH_OK;
}

constexpr uint64_t CMPC_CHUNK_PAIRS = 4u << 20; // pairs per launch: 256 MiB of records per list if every pair passes

} // namespace

extern "C" {

int finch_compare_counts_pair(const finch_sketches *refs, uint32_t ir, const finch_sketches *queries, uint32_t iq,
                              finch_count_moments *out) try {
    if (!refs || !queries || !out) return hfail(FH_ERR_INVALID, "null argument");
    if (ir >= refs->v.size()) return hfail(FH_ERR_INVALID, "reference sketch %u of %zu sketches", ir, refs->v.size());
    if (iq >= queries->v.size()) return hfail(FH_ERR_INVALID, "query sketch %u of %zu sketches", iq, queries->v.size());
    compare_counts_walk(refs->v[ir].hashes, queries->v[iq].hashes, out);
    return FH_OK;
} FINCH_CATCH

int finch_compare_counts(const finch_sketches *refs, const finch_sketches *queries, uint64_t min_common, const int *devices,
                         uint32_t n_devices, finch_compare_counts_result **out) try {
    if (!queries || !refs || !out || (n_devices && !devices)) return hfail(FH_ERR_INVALID, "null argument");
    if (int rc = check_entry_count(n_devices)) return rc;
    const std::vector<Sketch> &Qs = queries->v, &Rs = refs->v;
    if (int rc = check_ascending(Qs, "query")) return rc;
    if (int rc = check_ascending(Rs, "reference")) return rc;
    const uint32_t nq = (uint32_t)Qs.size(), nr = (uint32_t)Rs.size();
    auto res = std::make_unique<finch_compare_counts_result>();
    if (nq == 0 || nr == 0) {
        *out = res.release();
        return FH_OK;
    }
    std::vector<int> devs;
    if (int rc = resolve_devices(devices, n_devices, devs)) return rc;
    DeviceGuard restore_device;

    DistCsr qc, rc_;
    qc.build(Qs, false, true);
    rc_.build(Rs, false, true);
    const uint32_t per_chunk = chunk_refs("cmpc_chunk_pairs", CMPC_CHUNK_PAIRS, nq, nr, true);
    if ((uint64_t)per_chunk * nq > (1ull << 31)) // (more than 2^31 queries cannot be: nq < 2^32 and per_chunk = 1 here)
        return hfail(FH_ERR_UNSUPPORTED, "%u queries: more than 2^31 pairs per reference", nq);
    const uint32_t n_chunks = (nr + per_chunk - 1) / per_chunk;
    const uint32_t n_entries = (uint32_t)std::min<size_t>(devs.size(), n_chunks); // (an entry without a chunk opens nothing)
    const uint32_t slice = (uint32_t)std::min<uint64_t>(cfg_u64("cmpc_slice", fh::MOMENTS_MAX_SLICE), fh::MOMENTS_MAX_SLICE);
    // a sketch has fewer than 2^32 - 1 hashes, so no pair reaches a threshold above that
    const uint32_t min_c = (uint32_t)std::min<uint64_t>(min_common, UINT32_MAX);
    std::vector<MomentsFound> found(n_chunks);
    for (uint32_t k = 0; k < n_chunks; ++k) found[k].q0 = 0, found[k].q1 = nq, found[k].r0 = k * per_chunk, found[k].r1 = std::min(nr, k * per_chunk + per_chunk);
    fh::EntryError err;
    std::mutex stat_mu;

    // one thread per device entry: chunks e, e + n_entries, ...; chunk m + 1's kernel runs while chunk m's records are taken
    fh::for_entries(n_entries, err, FH_ERR_CAPACITY, [&](unsigned e) {
        fh::MomentsDevice *md = nullptr;
        fh::Finally close_md{[&] { fh::moments_close(md); }};
        if (entry_failed(err, fh::moments_open(devs[e], qc.moments_view(), rc_.moments_view(), slice, (uint64_t)per_chunk * nq, min_c, &md))) return;
        std::vector<uint32_t> mine;
        for (uint32_t k = e; k < n_chunks; k += n_entries) mine.push_back(k);
        double ms_sum = 0.;
        uint64_t copied = 0;
        auto launch = [&](size_t m, int slot) {
            const uint32_t r0 = mine[m] * per_chunk;
            return fh::moments_launch(md, slot, r0, std::min(nr, r0 + per_chunk));
        };
        auto take = [&](size_t m, int slot) {
            const fh::MomentsRecord *recs = nullptr;
            uint64_t n = 0;
            double ms = 0.;
            if (int rc = fh::moments_wait(md, slot, &recs, &n, &ms)) return rc;
            ms_sum += ms;
            copied += n;
            found[mine[m]].recs.assign(recs, recs + n);
            return FH_OK;
        };
        entry_failed(err, fh::two_slot(mine.size(), err, launch, take));
        std::lock_guard<std::mutex> g(stat_mu);
        res->kernel_ms += ms_sum;
        res->launches += mine.size();
        res->copied += copied;
    });
    if (err.failed()) return hfail(err.rc(), "%s", err.msg().c_str());

    if (int rc = compare_counts_finish(found, nq, nr, res.get())) return rc;
    *out = res.release();
    return FH_OK;
} FINCH_CATCH

uint64_t finch_compare_counts_len(const finch_compare_counts_result *r) { return r ? r->rows.size() : 0; }

int finch_compare_counts_copy(const finch_compare_counts_result *r, uint32_t *ref_idx, uint32_t *query_idx, finch_count_moments *rows) try {
    if (!r) return hfail(FH_ERR_INVALID, "null argument");
    const size_t n = r->rows.size();
    if (ref_idx && n) memcpy(ref_idx, r->r.data(), n * sizeof(uint32_t));
    if (query_idx && n) memcpy(query_idx, r->q.data(), n * sizeof(uint32_t));
    if (rows && n) memcpy(rows, r->rows.data(), n * sizeof(finch_count_moments));
    return FH_OK;
} FINCH_CATCH

int finch_compare_counts_stats(const finch_compare_counts_result *r, double *kernel_ms, uint64_t *launches, uint64_t *records_copied) try {
    if (!r) return hfail(FH_ERR_INVALID, "null argument");
    if (kernel_ms) *kernel_ms = r->kernel_ms;
    if (launches) *launches = r->launches;
    if (records_copied) *records_copied = r->copied;
    return FH_OK;
} FINCH_CATCH

void finch_compare_counts_free(finch_compare_counts_result *r) { delete r; }

// compare_counts through the library index (fh_index.hip, fh_moments.hip): a row needs common >= min_common
// >= 1, the index's count leaves common = |Q n R| of every pair that shares a hash, and only the pairs that pass are walked;
// their records come through finch_compare_counts' own finish.  The index holds the library's hashes; its counts are attached
// here, once.
int finch_index_attach_counts(const finch_index *cix, const finch_sketches *refs, uint64_t *device_bytes) try {
    if (!cix || !refs) return hfail(FH_ERR_INVALID, "null argument");
    finch_index *ix = const_cast<finch_index *>(cix); // (the attachment is the index's; `mu` serialises its use)
    std::lock_guard<std::mutex> one_call(ix->mu);
    const std::vector<Sketch> &Rs = refs->v;
    uint64_t postings = 0;
    for (const Sketch &s : Rs) postings += s.hashes.size();
    if (Rs.size() != ix->nr || postings != ix->postings)
        return hfail(FH_ERR_INVALID, "finch_index_attach_counts: refs has %zu sketches and %llu hashes, the index was built from %u and %llu: "
                                     "refs must be the library of the index", Rs.size(), (unsigned long long)postings, ix->nr,
                     (unsigned long long)ix->postings);
    for (uint32_t r = 0; r < ix->nr; ++r)
        if (Rs[r].hashes.size() != ix->rlen[r])
            return hfail(FH_ERR_INVALID, "finch_index_attach_counts: refs sketch %u (%s) has %zu hashes, the index was built from one of %u: "
                                         "refs must be the library of the index", r, Rs[r].name.c_str(), Rs[r].hashes.size(), ix->rlen[r]);
    uint64_t total = 0;
    if (ix->entries.empty()) ix->counts_attached = true; // (a library without a hash: nothing to attach, no device)
    else {
        DeviceGuard restore_device;
        std::vector<uint32_t> counts;
        counts.reserve(postings);
        for (const Sketch &s : Rs)
            for (const KmerCount &h : s.hashes) counts.push_back(h.count);
        ix->counts_attached = false; // until every entry has the new counts
        for (fh::IndexDevice *d : ix->entries) {
            uint64_t bytes = 0;
            if (int rc = fh::index_attach_counts(d, counts.data(), counts.size(), &bytes)) {
                // no half-made attachment: an entry that holds counts while the index says it has none would have
                // finch_index_add extend them on that entry alone
                const std::string why = fh_last_error();
                for (fh::IndexDevice *e : ix->entries) fh::index_drop_counts(e);
                return hfail(rc, "%s", why.c_str());
            }
            total += bytes;
        }
        ix->counts_attached = true;
    }
    if (device_bytes) *device_bytes = total;
    return FH_OK;
} FINCH_CATCH

int finch_index_compare_counts(const finch_index *cix, const finch_sketches *queries, uint64_t min_common,
                               finch_compare_counts_result **out) try {
    if (!cix || !queries || !out) return hfail(FH_ERR_INVALID, "null argument");
    finch_index *ix = const_cast<finch_index *>(cix); // (the launch state is the index's; `mu` serialises its use)
    std::lock_guard<std::mutex> one_call(ix->mu);     // (from here: finch_index_add / finch_index_keep change what is read below)
    if (min_common == 0)
        return hfail(FH_ERR_INVALID, "finch_index_compare_counts: min_common 0: an index finds only the pairs that share a hash, and a "
                                     "threshold of 0 keeps every pair -- use finch_compare_counts");
    const std::vector<Sketch> &Qs = queries->v;
    if (int rc = check_ascending(Qs, "query")) return rc;
    const uint32_t nq = (uint32_t)Qs.size();
    auto res = std::make_unique<finch_compare_counts_result>();
    res->from_index = true;
    if (nq == 0 || ix->entries.empty()) {
        *out = res.release();
        return FH_OK;
    }
    if (!ix->counts_attached)
        return hfail(FH_ERR_STATE, "finch_index_compare_counts: the index holds the library's hashes, not its counts -- call "
                                   "finch_index_attach_counts first");
    DeviceGuard restore_device;

    // a sketch has fewer than 2^32 - 1 hashes, so no pair reaches a threshold above that
    const uint32_t min_c = (uint32_t)std::min<uint64_t>(min_common, UINT32_MAX);
    DistCsr qc;
    qc.build(Qs, false, true);
    const uint32_t n_chunks = (nq + ix->chunk - 1) / ix->chunk;
    const uint32_t n_entries = (uint32_t)std::min<size_t>(ix->entries.size(), n_chunks);
    std::vector<MomentsFound> found(n_chunks);
    fh::EntryError err;
    std::mutex stat_mu;

    // one thread per device entry: chunks of queries e, e + n_entries, ...
    fh::for_entries(n_entries, err, FH_ERR_CAPACITY, [&](unsigned e) {
        double ms_sum = 0.;
        uint64_t touched = 0, copied = 0, launches = 0;
        for (uint32_t k = e; k < n_chunks && !err.failed(); k += n_entries) {
            MomentsFound &f = found[k];
            f.q0 = k * ix->chunk, f.q1 = (uint32_t)std::min<uint64_t>(nq, (uint64_t)f.q0 + ix->chunk), f.r0 = 0, f.r1 = ix->nr;
            if (entry_failed(err, fh::index_compare_counts_chunk(ix->entries[e], qc.view(), qc.counts.data(), f.q0, f.q1, min_c, &f.recs, &touched,
                                                                 &ms_sum, &launches)))
                break;
            copied += f.recs.size();
        }
        std::lock_guard<std::mutex> g(stat_mu);
        res->kernel_ms += ms_sum;
        res->launches += launches;
        res->copied += copied;
        res->touched += touched;
    });
    if (err.failed()) return hfail(err.rc(), "%s", err.msg().c_str());
    if (int rc = compare_counts_finish(found, nq, ix->nr, res.get())) return rc;
    *out = res.release();
    return FH_OK;
} FINCH_CATCH

int finch_index_compare_counts_stats(const finch_compare_counts_result *r, uint64_t *pairs_touched, uint64_t *pairs_walked) try {
    if (!r) return hfail(FH_ERR_INVALID, "null argument");
    if (!r->from_index) return hfail(FH_ERR_INVALID, "finch_index_compare_counts_stats: the result was not made by finch_index_compare_counts");
    if (pairs_touched) *pairs_touched = r->touched;
    if (pairs_walked) *pairs_walked = r->copied; // (the moment kernel walks exactly the pairs whose records cross)
    return FH_OK;
} FINCH_CATCH

} // extern "C"

// ---------------------------------------------------------------------------------------------
// the index grown and shrunk in place (Multisketch.add, __delitem__, filter_to_matches, filter_to_names: python.rs:158-248;
// fh_index.hip).  Everything an update needs of the library is on the device already; what crosses is what
// changes.  Every entry builds its new arrays beside the old ones, and only when all have are they swapped in: a refusal or a
// failure before that leaves the index as it was.
// ---------------------------------------------------------------------------------------------
namespace {

void index_discard_all(finch_index *ix) {
    for (fh::IndexDevice *d : ix->entries) fh::index_discard(d);
}

// every entry has built its stage: the swap, which cannot fail
void index_commit_all(finch_index *ix, uint32_t chunk) {
    ix->device_bytes = 0;
    for (fh::IndexDevice *d : ix->entries) ix->device_bytes += fh::index_commit(d);
    ix->chunk = chunk;
}

void index_close_all(std::vector<fh::IndexDevice *> &entries) {
    for (fh::IndexDevice *d : entries) fh::index_close(d);
    entries.clear();
}

} // namespace

extern "C" {

int finch_index_add(finch_index *ix, const finch_sketches *more, double *kernel_ms) try {
    if (!ix || !more) return hfail(FH_ERR_INVALID, "null argument");
    const std::vector<Sketch> &Ms = more->v;
    if (int rc = check_ascending(Ms, "added")) return rc;
    std::lock_guard<std::mutex> one_call(ix->mu);
    if (kernel_ms) *kernel_ms = 0.;
    if (Ms.empty()) return FH_OK;
    uint64_t added = 0;
    for (const Sketch &s : Ms) added += s.hashes.size();
    const uint64_t nr2 = (uint64_t)ix->nr + Ms.size(), P2 = ix->postings + added, max_postings = index_max_postings();
    if (nr2 > UINT32_MAX) return hfail(FH_ERR_UNSUPPORTED, "reference library: %llu sketches (at most 2^32 - 1)", (unsigned long long)nr2);
    if (P2 > max_postings)
        return hfail(FH_ERR_UNSUPPORTED, "reference library: %llu postings (hashes of all %llu sketches, %zu of them added), an index holds at most %llu",
                     (unsigned long long)P2, (unsigned long long)nr2, Ms.size(), (unsigned long long)max_postings);
    DistCsr mc;
    mc.build(Ms, false, ix->counts_attached);
    // room for the host's copies first: after the swap nothing may fail
    ix->rlen.reserve(nr2), ix->rflag.reserve(nr2), ix->rmax.reserve(nr2), ix->rscale.reserve(nr2);
    double ms = 0.;
    if (P2 && ix->entries.empty()) {
        // the first hash: the entries are opened as finch_index_new opens them, over the empty sketches there are and the added ones
        std::vector<int> devs;
        if (int rc = resolve_devices(ix->devs.data(), (uint32_t)ix->devs.size(), devs)) return rc;
        DeviceGuard restore_device;
        DistCsr all;
        all.hashes = mc.hashes;
        all.offsets.assign((size_t)ix->nr, 0);
        all.offsets.insert(all.offsets.end(), mc.offsets.begin(), mc.offsets.end());
        all.flags = ix->rflag, all.max_hash = ix->rmax, all.scale = ix->rscale;
        all.flags.insert(all.flags.end(), mc.flags.begin(), mc.flags.end());
        all.max_hash.insert(all.max_hash.end(), mc.max_hash.begin(), mc.max_hash.end());
        all.scale.insert(all.scale.end(), mc.scale.begin(), mc.scale.end());
        const uint32_t chunk = index_chunk_for(*ix, (uint32_t)nr2);
        std::vector<fh::IndexDevice *> opened;
        uint64_t bytes_sum = 0;
        for (int d : devs) {
            fh::IndexDevice *dev = nullptr;
            uint64_t bytes = 0, attached = 0;
            int rc = fh::index_open(d, all.view(), chunk, &dev, &bytes, &ms);
            if (rc == FH_OK) {
                opened.push_back(dev);
                if (ix->counts_attached) rc = fh::index_attach_counts(dev, mc.counts.data(), mc.counts.size(), &attached);
            }
            if (rc != FH_OK) {
                const std::string why = fh_last_error();
                index_close_all(opened);
                return hfail(rc, "%s", why.c_str());
            }
            bytes_sum += bytes;
        }
        ix->entries.swap(opened);
        ix->device_bytes = bytes_sum;
        ix->chunk = chunk;
    } else if (P2) {
        DeviceGuard restore_device;
        const uint32_t chunk = index_chunk_for(*ix, (uint32_t)nr2), tile = index_update_tile();
        for (fh::IndexDevice *d : ix->entries)
            if (int rc = fh::index_add(d, mc.view(), ix->counts_attached ? mc.counts.data() : nullptr, chunk, tile, &ms)) {
                const std::string why = fh_last_error();
                index_discard_all(ix);
                return hfail(rc, "%s", why.c_str());
            }
        index_commit_all(ix, chunk);
    }
    ix->nr = (uint32_t)nr2, ix->postings = P2;
    for (const Sketch &s : Ms) ix->rlen.push_back((uint32_t)s.hashes.size());
    ix->rflag.insert(ix->rflag.end(), mc.flags.begin(), mc.flags.end());
    ix->rmax.insert(ix->rmax.end(), mc.max_hash.begin(), mc.max_hash.end());
    ix->rscale.insert(ix->rscale.end(), mc.scale.begin(), mc.scale.end());
    if (kernel_ms) *kernel_ms = ms;
    return FH_OK;
} FINCH_CATCH

int finch_index_keep(finch_index *ix, const uint32_t *keep, uint32_t n_keep, double *kernel_ms) try {
    if (!ix || (n_keep && !keep)) return hfail(FH_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> one_call(ix->mu);
    if (kernel_ms) *kernel_ms = 0.;
    uint64_t P2 = 0;
    for (uint32_t t = 0; t < n_keep; ++t) {
        if (keep[t] >= ix->nr)
            return hfail(FH_ERR_INVALID, "finch_index_keep: keep[%u] = %u: the index has %u references", t, keep[t], ix->nr);
        if (t && keep[t] <= keep[t - 1])
            return hfail(FH_ERR_INVALID, "finch_index_keep: keep[%u] = %u after %u: the list must ascend strictly", t, keep[t], keep[t - 1]);
        P2 += ix->rlen[keep[t]];
    }
    // the host's copies first: if one cannot be made, nothing has changed yet
    std::vector<uint32_t> rlen(n_keep), rflag(n_keep);
    std::vector<uint64_t> rmax(n_keep);
    std::vector<double> rscale(n_keep);
    for (uint32_t t = 0; t < n_keep; ++t)
        rlen[t] = ix->rlen[keep[t]], rflag[t] = ix->rflag[keep[t]], rmax[t] = ix->rmax[keep[t]], rscale[t] = ix->rscale[keep[t]];
    double ms = 0.;
    if (!ix->entries.empty()) {
        DeviceGuard restore_device;
        if (P2 == 0) { // no hash is left: no entries, as finch_index_new leaves such a library
            index_close_all(ix->entries);
            ix->device_bytes = 0, ix->chunk = 0;
        } else {
            const uint32_t chunk = index_chunk_for(*ix, n_keep), tile = index_update_tile();
            for (fh::IndexDevice *d : ix->entries)
                if (int rc = fh::index_keep(d, keep, n_keep, chunk, tile, &ms)) {
                    const std::string why = fh_last_error();
                    index_discard_all(ix);
                    return hfail(rc, "%s", why.c_str());
                }
            index_commit_all(ix, chunk);
        }
    }
    ix->nr = n_keep, ix->postings = P2;
    ix->rlen.swap(rlen), ix->rflag.swap(rflag), ix->rmax.swap(rmax), ix->rscale.swap(rscale);
    if (kernel_ms) *kernel_ms = ms;
    return FH_OK;
} FINCH_CATCH

} // extern "C"

// ---------------------------------------------------------------------------------------------
// merge (Sketch.merge: merge_sketches, lib/src/python.rs:24-100): the walk over two sketches that stops when either runs out,
// one record per hash with the counts of a shared hash added (u32, wrapping: a release build of the reference), clipped by
// (size, the first sketch's scale).  finch_merge_pair is the reference's loop as written, on the host; finch_merge_groups folds
// ordered groups of sketches on the device (fh_merge_lib.hip), one workgroup per group, and takes the k-mer text of every
// result record from the host's own sketches by the record's provenance.  DESIGN.md §3.12.
// ---------------------------------------------------------------------------------------------
namespace {

// SketchParams::check_compatibility (mod.rs:185-212) of a pair: "" or the reference's words for the first difference
std::string merge_incompatible(const finch_sketch_params &a, const finch_sketch_params &b) {
    auto hash_type = [](const finch_sketch_params &p) { return p.kind == 2 ? "None" : "MurmurHash3_x64_128"; };
    auto hash_bits = [](const finch_sketch_params &p) { return p.kind == 2 ? 0u : 64u; };
    auto hash_seed = [](const finch_sketch_params &p) { return p.kind == 2 ? 0ull : (unsigned long long)p.hash_seed; };
    char buf[256];
    buf[0] = 0;
    if (a.kmer_length != b.kmer_length)
        snprintf(buf, sizeof buf, "First sketch has k %u, but second sketch has k %u", a.kmer_length, b.kmer_length);
    else if (strcmp(hash_type(a), hash_type(b)) != 0)
        snprintf(buf, sizeof buf, "First sketch has hash type %s, but second sketch has hash type %s", hash_type(a), hash_type(b));
    else if (hash_bits(a) != hash_bits(b))
        snprintf(buf, sizeof buf, "First sketch has hash bits %u, but second sketch has hash bits %u", hash_bits(a), hash_bits(b));
    else if (hash_seed(a) != hash_seed(b))
        snprintf(buf, sizeof buf, "First sketch has hash seed %llu, but second sketch has hash seed %llu", hash_seed(a), hash_seed(b));
    return buf;
}

// the clip's share of the first sketch: hash_info().3 and max_hash = u64::MAX / ((1. / sc) as u64) (python.rs:70-83)
struct MergeClip {
    bool has_scale = false;
    uint64_t max_hash = 0;
};

// false: the divisor (1. / sc) as u64 is 0 -- a scale above 1, below 0 or NaN --, where the reference panics
bool merge_clip_of(const finch_sketch_params &p, MergeClip *c) {
    c->has_scale = p.kind == 1;
    c->max_hash = 0;
    if (!c->has_scale) return true;
    if (!(1. / p.scale >= 1.)) return false;
    c->max_hash = fh::api_scaled_max_hash(p.scale); // (the same expression wherever the divisor is not 0)
    return true;
}

// python.rs:44-98, statement by statement; `out` is neither input
void merge_walk(const std::vector<KmerCount> &sketch1, const std::vector<KmerCount> &sketch2, const uint64_t *size, const MergeClip &clip,
                std::vector<KmerCount> &out) {
    out.clear();
    out.reserve(sketch1.size() + sketch2.size());
    size_t i = 0, j = 0;
    while (i < sketch1.size() && j < sketch2.size()) {
        if (sketch1[i].hash < sketch2[j].hash) {
            out.push_back(sketch1[i]);
            i += 1;
        } else if (sketch2[j].hash < sketch1[i].hash) {
            out.push_back(sketch2[j]);
            j += 1;
        } else {
            out.push_back(KmerCount{sketch1[i].hash, sketch1[i].kmer, (uint32_t)(sketch1[i].count + sketch2[j].count),
                                    (uint32_t)(sketch1[i].extra_count + sketch2[j].extra_count), sketch1[i].label});
            i += 1;
            j += 1;
        }
    }
    size_t keep = out.size();
    if (size && clip.has_scale) {
        for (keep = 0; keep < out.size() && (out[keep].hash <= clip.max_hash || keep < *size); ++keep) {}
    } else if (clip.has_scale) {
        for (keep = 0; keep < out.size() && out[keep].hash <= clip.max_hash; ++keep) {}
    } else if (size) {
        keep = (size_t)std::min<uint64_t>(*size, out.size());
    }
    out.resize(keep);
}

// a named member as the device reads it: strictly ascending, fewer than 2^32 - 1 hashes
int merge_check_member(const Sketch &sk, uint32_t idx, uint32_t g, uint64_t m) {
    const std::vector<KmerCount> &h = sk.hashes;
    if (h.size() >= UINT32_MAX)
        return hfail(FH_ERR_INVALID, "group %u member %llu: merge sketch %u (%s) has %zu hashes (at most 2^32 - 2)", g, (unsigned long long)m, idx,
                     sk.name.c_str(), h.size());
    for (size_t j = 1; j < h.size(); ++j)
        if (!(h[j - 1].hash < h[j].hash))
            return hfail(FH_ERR_INVALID, "group %u member %llu: merge sketch %u (%s): hashes not strictly ascending at %zu", g,
                         (unsigned long long)m, idx, sk.name.c_str(), j);
    return FH_OK;
}

double merge_now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

constexpr uint64_t MERGE_CHUNK_RECORDS = 4u << 20; // records per launch: 96 MiB for each of a buffer set's three lists
constexpr uint32_t MERGE_MAX_LAUNCH_GROUPS = 1u << 20;

} // namespace

extern "C" {

int finch_merge_pair(const finch_sketches *a, uint32_t ia, const finch_sketches *b, uint32_t ib, const uint64_t *size,
                     finch_sketches **out) try {
    if (!a || !b || !out) return hfail(FH_ERR_INVALID, "null argument");
    if (ia >= a->v.size()) return hfail(FH_ERR_INVALID, "first sketch %u of %zu sketches", ia, a->v.size());
    if (ib >= b->v.size()) return hfail(FH_ERR_INVALID, "second sketch %u of %zu sketches", ib, b->v.size());
    const Sketch &sketch = a->v[ia], &other = b->v[ib];
    const std::string bad = merge_incompatible(sketch.sketch_params, other.sketch_params);
    if (!bad.empty()) return hfail(FH_ERR_INVALID, "%s", bad.c_str());
    MergeClip clip;
    if (!merge_clip_of(sketch.sketch_params, &clip))
        return hfail(FH_ERR_INVALID, "first sketch %u (%s) has scale %g: 1 / scale as an integer is 0", ia, sketch.name.c_str(), sketch.sketch_params.scale);
    auto res = std::make_unique<finch_sketches>();
    res->v.resize(1);
    Sketch &o = res->v[0];
    o.name = sketch.name;
    o.comment = sketch.comment;
    o.sketch_params = sketch.sketch_params;
    o.filter_params = sketch.filter_params;
    o.seq_length = sketch.seq_length + other.seq_length; // (u64: wraps)
    o.num_valid_kmers = sketch.num_valid_kmers + other.num_valid_kmers;
    merge_walk(sketch.hashes, other.hashes, size, clip, o.hashes);
    *out = res.release();
    return FH_OK;
} FINCH_CATCH

int finch_merge_groups(const finch_sketches *s, const uint64_t *offsets, const uint32_t *members, uint32_t n_groups, const uint64_t *size,
                       const int *devices, uint32_t n_devices, finch_sketches **out, double *kernel_ms, uint64_t *launches,
                       uint64_t *records_copied, double *phase_ms) try {
    if (kernel_ms) *kernel_ms = 0.;
    if (launches) *launches = 0;
    if (records_copied) *records_copied = 0;
    if (phase_ms) phase_ms[0] = phase_ms[1] = phase_ms[2] = 0.;
    if (!s || !offsets || !out || (n_groups && !members) || (n_devices && !devices)) return hfail(FH_ERR_INVALID, "null argument");
    if (int rc = check_entry_count(n_devices)) return rc;
    const std::vector<Sketch> &S = s->v;
    auto res = std::make_unique<finch_sketches>();
    if (n_groups == 0) {
        *out = res.release();
        return FH_OK;
    }

    // everything that is decided without a device
    for (uint32_t g = 0; g < n_groups; ++g) {
        if (offsets[g + 1] < offsets[g]) return hfail(FH_ERR_INVALID, "group %u: the offsets do not ascend (%llu after %llu)", g,
                                                      (unsigned long long)offsets[g + 1], (unsigned long long)offsets[g]);
        if (offsets[g + 1] == offsets[g]) return hfail(FH_ERR_INVALID, "group %u is empty", g);
    }
    std::vector<uint8_t> checked(S.size(), 0);
    std::vector<MergeClip> clips(n_groups);
    std::vector<uint64_t> total(n_groups, 0);
    std::vector<uint32_t> multi; // the groups of two members or more
    for (uint32_t g = 0; g < n_groups; ++g) {
        const uint32_t *mem = members + offsets[g];
        const uint64_t nm = offsets[g + 1] - offsets[g];
        for (uint64_t m = 0; m < nm; ++m) {
            if (mem[m] >= S.size()) return hfail(FH_ERR_INVALID, "group %u member %llu: sketch %u of %zu sketches", g, (unsigned long long)m, mem[m], S.size());
            if (m > 0) {
                const std::string bad = merge_incompatible(S[mem[0]].sketch_params, S[mem[m]].sketch_params);
                if (!bad.empty()) return hfail(FH_ERR_INVALID, "group %u member %llu: %s", g, (unsigned long long)m, bad.c_str());
            }
            if (!checked[mem[m]]) {
                if (int rc = merge_check_member(S[mem[m]], mem[m], g, m)) return rc;
                checked[mem[m]] = 1;
            }
            total[g] += S[mem[m]].hashes.size();
            if (total[g] > UINT32_MAX) return hfail(FH_ERR_INVALID, "group %u: its members have 2^32 records or more together", g);
        }
        if (nm >= 2) {
            if (nm > UINT32_MAX) return hfail(FH_ERR_INVALID, "group %u has %llu members (at most 2^32 - 1)", g, (unsigned long long)nm);
            if (!merge_clip_of(S[mem[0]].sketch_params, &clips[g]))
                return hfail(FH_ERR_INVALID, "group %u member 0: sketch %u (%s) has scale %g: 1 / scale as an integer is 0", g, mem[0],
                             S[mem[0]].name.c_str(), S[mem[0]].sketch_params.scale);
            multi.push_back(g);
        }
    }

    // what does not need the walk: the first member's name, comment and parameters, the wrapping u64 sums; a group of one member
    // is that member
    res->v.resize(n_groups);
    for (uint32_t g = 0; g < n_groups; ++g) {
        const uint32_t *mem = members + offsets[g];
        const Sketch &first = S[mem[0]];
        Sketch &o = res->v[g];
        o.name = first.name;
        o.comment = first.comment;
        o.sketch_params = first.sketch_params;
        o.filter_params = first.filter_params;
        for (uint64_t m = 0; m < offsets[g + 1] - offsets[g]; ++m) o.seq_length += S[mem[m]].seq_length, o.num_valid_kmers += S[mem[m]].num_valid_kmers;
        if (offsets[g + 1] - offsets[g] == 1) o.hashes = first.hashes;
    }
    if (multi.empty()) {
        *out = res.release();
        return FH_OK;
    }

    std::vector<int> devs;
    if (int rc = resolve_devices(devices, n_devices, devs)) return rc;
    DeviceGuard restore_device;

    const uint64_t budget = std::min<uint64_t>(std::max<uint64_t>(1, cfg_u64("merge_chunk_records", MERGE_CHUNK_RECORDS)), 1ull << 31);
    const uint32_t tile = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, cfg_u64("merge_tile", 1024)), fh::MERGE_LIB_MAX_TILE);
    const uint32_t n_entries = (uint32_t)std::min<size_t>(devs.size(), multi.size()); // (an entry without a group opens nothing)
    fh::EntryError err;
    std::mutex stat_mu;
    double st_kernel = 0., st_upload = 0., st_copy = 0., st_gather = 0.;
    uint64_t st_launches = 0, st_copied = 0;

    // one thread per device entry: the groups multi[e], multi[e + n_entries], ... in launches of at most `budget` records;
    // launch m + 1's kernel runs while launch m's records are copied back and given their k-mer text
    fh::for_entries(n_entries, err, FH_ERR_CAPACITY, [&](unsigned e) {
        fh::MergeLibDevice *md = nullptr;
        fh::Finally close_md{[&] { fh::merge_lib_close(md); }};
        // the sketches this entry's groups name, once each
        std::vector<uint32_t> slot_of(S.size(), UINT32_MAX);
        std::vector<uint64_t> in_h, in_off(1, 0);
        std::vector<uint32_t> in_c, in_e;
        struct Launch {
            std::vector<fh::MergeLibGroup> groups;
            std::vector<uint32_t> members, gids;
            uint64_t records = 0;
        };
        std::vector<Launch> L;
        for (size_t k = e; k < multi.size(); k += n_entries) {
            const uint32_t g = multi[k];
            const uint32_t *mem = members + offsets[g];
            const uint32_t nm = (uint32_t)(offsets[g + 1] - offsets[g]);
            // a bound on the accumulator after every step that needs no merging: the members' lengths together; with a size
            // and no scale every step ends truncated to the size
            uint64_t cap = total[g];
            if (size && !clips[g].has_scale) cap = std::min<uint64_t>(cap, std::max<uint64_t>(S[mem[0]].hashes.size(), *size));
            if (L.empty() || L.back().records + cap > budget || L.back().groups.size() >= MERGE_MAX_LAUNCH_GROUPS ||
                L.back().members.size() + nm > UINT32_MAX)
                L.emplace_back();
            Launch &l = L.back();
            l.groups.push_back(fh::MergeLibGroup{l.records, clips[g].max_hash, (uint32_t)l.members.size(), nm, (uint32_t)cap, clips[g].has_scale ? 1u : 0u});
            l.gids.push_back(g);
            l.records += cap;
            for (uint32_t m = 0; m < nm; ++m) {
                if (slot_of[mem[m]] == UINT32_MAX) {
                    slot_of[mem[m]] = (uint32_t)(in_off.size() - 1);
                    for (const KmerCount &h : S[mem[m]].hashes) in_h.push_back(h.hash), in_c.push_back(h.count), in_e.push_back(h.extra_count);
                    in_off.push_back(in_h.size());
                }
                l.members.push_back(slot_of[mem[m]]);
            }
        }
        uint32_t max_groups = 1;
        uint64_t max_members = 2, max_records = 1;
        for (const Launch &l : L) {
            max_groups = std::max<uint32_t>(max_groups, (uint32_t)l.groups.size());
            max_members = std::max<uint64_t>(max_members, l.members.size());
            max_records = std::max(max_records, l.records);
        }
        double upload_ms = 0.;
        const fh::MergeLibInput in{in_h.data(), in_c.data(), in_e.data(), in_off.data(), (uint32_t)(in_off.size() - 1)};
        if (entry_failed(err, fh::merge_lib_open(devs[e], in, max_groups, max_members, max_records, tile, size, &md, &upload_ms))) return;
        double ms_sum = 0., copy_sum = 0., gather_sum = 0.;
        uint64_t copied = 0;
        auto launch = [&](size_t m, int slot) {
            return fh::merge_lib_launch(md, slot, L[m].groups.data(), (uint32_t)L[m].groups.size(), L[m].members.data(), L[m].members.size());
        };
        auto take = [&](size_t m, int slot) {
            const fh::MergeLibOut *outs = nullptr;
            const fh::MergeLibRecord *recs = nullptr;
            uint64_t n = 0;
            double ms = 0., copy_ms = 0.;
            if (int rc = fh::merge_lib_wait(md, slot, &outs, &recs, &n, &ms, &copy_ms)) return rc;
            ms_sum += ms;
            copy_sum += copy_ms;
            copied += n;
            // the k-mer text (and label) of every record from the member and position it came from
            const double t0 = merge_now_ms();
            for (size_t k = 0; k < L[m].gids.size(); ++k) {
                const uint32_t g = L[m].gids[k];
                const uint32_t *mem = members + offsets[g];
                const uint64_t nm = offsets[g + 1] - offsets[g];
                std::vector<KmerCount> &h = res->v[g].hashes;
                h.resize(outs[k].len);
                const fh::MergeLibRecord *r = recs + outs[k].place;
                for (uint32_t x = 0; x < outs[k].len; ++x) {
                    if (r[x].slot >= nm || r[x].pos >= S[mem[r[x].slot]].hashes.size() || S[mem[r[x].slot]].hashes[r[x].pos].hash != r[x].hash) {
                        err.fail(FH_ERR_STATE, "merge: record " + std::to_string(x) + " of group " + std::to_string(g) + " names no entry with its hash");
                        return FH_ERR_STATE;
                    }
                    const KmerCount &src = S[mem[r[x].slot]].hashes[r[x].pos];
                    h[x] = KmerCount{r[x].hash, src.kmer, r[x].count, r[x].extra, src.label};
                }
            }
            gather_sum += merge_now_ms() - t0;
            return FH_OK;
        };
        entry_failed(err, fh::two_slot(L.size(), err, launch, take)); // (a record's own message came first and stays)
        std::lock_guard<std::mutex> g(stat_mu);
        st_kernel += ms_sum;
        st_upload += upload_ms;
        st_copy += copy_sum;
        st_gather += gather_sum;
        st_launches += L.size();
        st_copied += copied;
    });
    if (err.failed()) return hfail(err.rc(), "%s", err.msg().c_str());
    if (kernel_ms) *kernel_ms = st_kernel;
    if (launches) *launches = st_launches;
    if (records_copied) *records_copied = st_copied;
    if (phase_ms) phase_ms[0] = st_upload, phase_ms[1] = st_copy, phase_ms[2] = st_gather;
    *out = res.release();
    return FH_OK;
} FINCH_CATCH

} // extern "C"
