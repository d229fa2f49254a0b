// fh_screen.h -- what finch_index_screen (fh_host.cpp; include/finch_host.h) asks of the device and of the
// index: a view of the index's arrays, the per-call table over its distinct hashes, the launches over staged two-bit pieces and
// the per-reference finish.  Defined in fh_screen.hip (part 0), fh_index.hip (the view) and fh_library.cpp (the index's lock
// and first entry); no HIP types here, fh_host.cpp is plain C++.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <mutex>
#include <vector>

struct finch_index;

namespace fh {

struct IndexDevice;

// what the screen reads of an index entry, all of it on `device`: the postings sorted by hash (keys / vals, n_post of them) and
// the library's own CSR (rh, roff[0 .. nr]); stream = the entry's hipStream_t.  Valid while the index's lock is held.
struct ScreenView {
    const uint64_t *keys = nullptr;
    const uint32_t *vals = nullptr;
    const uint64_t *rh = nullptr, *roff = nullptr;
    uint32_t nr = 0, n_post = 0;
    int device = 0;
    void *stream = nullptr;
};
void index_screen_view(IndexDevice *d, ScreenView *v); // fh_index.hip

// fh_library.cpp: the index's lock (held by the screen for its whole length), its first device entry (nullptr: the library has
// no hash) and its references' lengths
std::mutex &index_mutex_of(const finch_index *ix);
IndexDevice *index_first_entry(const finch_index *ix);
const std::vector<uint32_t> &index_ref_lengths(const finch_index *ix);

constexpr uint64_t SCREEN_PIECE_DEFAULT = 16ull << 20, SCREEN_PIECE_MAX = 1ull << 30, SCREEN_PIECE_MIN = 2048;
constexpr uint32_t SCREEN_DIR_BITS_MAX = 28;

struct ScreenStats {
    uint64_t kmers = 0, hits = 0, distinct = 0, table_bytes = 0, launches = 0;
    double table_ms = 0., kernel_ms = 0.;
};

struct ScreenDevice;
// builds the table from the view's postings -- the distinct keys, a zeroed u64 multiplicity each, the directory of 2^b buckets
// (dir_bits < 0: b = ceil(log2 distinct); at least 1, at most SCREEN_DIR_BITS_MAX) -- and allocates two staging slots of `piece` positions
// (a multiple of 2048), pinned, with their device twins.  1 <= k <= 32.  Synchronous.
int screen_open(const ScreenView &v, uint32_t k, uint64_t seed, int dir_bits, uint64_t piece, ScreenDevice **out);
// the pinned two-bit region of a slot: fh_pack2::region_bytes(piece) bytes
uint8_t *screen_slot(ScreenDevice *d, int slot);
// the slot's region, `positions` of them (fh_pack2's form, complete: Packer::finish), to the device and k_screen over its tiles;
// returns once the copy has left the pinned slot -- the slot may be filled again -- while the kernel runs on
int screen_launch(ScreenDevice *d, int slot, uint64_t positions);
// the finish: shared / sum_mult / median_mult of every reference (nr values each) and the call's figures.  Synchronous.
int screen_finish(ScreenDevice *d, uint32_t *shared, uint64_t *sum_mult, uint64_t *median_mult, ScreenStats *st);
void screen_close(ScreenDevice *d);

} // namespace fh
