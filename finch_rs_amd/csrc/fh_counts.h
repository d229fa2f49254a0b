// fh_counts.h -- the AllCounts sketcher's per-lane arithmetic (FH_KIND_ALL_COUNTS, fh_counts.hip), written once so that
// hipcc compiles it for gfx950 and g++ for the host logic test (tests/test_allcounts_model.py).
//
// What it restates (reference file:line, relative to the finch-rs tree):
//   ac_lane_windows<K> : needletail 0.5.0 seq.normalize(false).bit_kmers(k, false) as AllCountsSketcher::process drives
//                        it (counts.rs:30): the FORWARD k-mer of every start whose K bytes are all bases.  The byte rules are
//                        fh_core.h's classify_chunk (ACGT, acgt, U/u -> T; every other byte breaks k-mers; whitespace never
//                        reaches the device).  The index is the window's m-form word (fh_core.h: A 0, C 1, G 2, T 3, the
//                        first base in the most significant digit) -- bit_kmers' BitKmer.0, the ix of counts[ix].
//   ac_revcomp<K>      : needletail bitkmer::reverse_complement((ix, k)).0 on that word (counts.rs:50-51).
//   ac_emit            : to_vec's walk (counts.rs:43-64) as an order-free predicate per ix.
#pragma once
#include "fh_core.h"

namespace fh {

constexpr int AC_MAX_K = 16;    // a 4^k table of u32: 16 GiB at k = 16 (the reference holds the same on the host)
constexpr int AC_LANE_POS = 32; // window starts per lane and step: 48 bytes (three 16-byte chunks) cover them for K <= 16
constexpr int AC_LANE_BYTES = 48;

FH_HD u64 ac_bins(int k) { return 1ull << (2 * k); }
FH_HD u32 ac_mask(int k) { return k >= 16 ? 0xFFFFFFFFu : ((1u << (2 * k)) - 1u); }

// the m-form word of the reverse complement of the k-base m-form word ix
FH_HD u32 ac_revcomp(u32 ix, int k) { return pairrev32(~ix & ac_mask(k)) >> (32 - 2 * k); }

// to_vec (counts.rs:43-64), per index: c = the forward count of ix, crc = that of its reverse complement rc.  ix is emitted iff
// c > 0 and (rc >= ix or crc == 0): a pair is reported at its smaller member unless that one never occurred.  Then
// extra_count = crc and count = c + crc, a WRAPPING u32 add (release build: counts.rs:52 `count += extra_count` without
// overflow checks); a palindrome (rc == ix, even k) gives 2c and c.
FH_HD bool ac_emit(u32 ix, u32 rc, u32 c, u32 crc) { return c != 0 && (rc >= ix || crc == 0); }

// The windows of a lane from its positions' classified form: codes[c] = the 2-bit codes of positions 16 c .. 16 c + 15 (c < 3),
// bit b of g64 = position b is a base (b < 48) -> f(j, ix) for every window start j < min(32, limit) whose K positions are all
// bases, ix = the window's m-form word.  The code of a position that is no base may be anything.
template <int K, class F>
FH_HDM void ac_code_windows(const u32 *codes, u64 g64, u32 limit, F &&f) {
    static_assert(K >= 1 && K <= AC_MAX_K, "AllCounts k is 1..16");
    u32 valid = (u32)window_valid_mask64<K>(g64); // bit j: positions j .. j + K - 1 are all bases (j + K - 1 <= 46 < 48)
    if (limit < 32) valid &= (1u << limit) - 1u;
    const u32 mask = ac_mask(K);
    u32 m = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int b = 0; b < AC_LANE_POS + K - 1; ++b) { // rolling m-form: the base entering at b becomes the lowest digit
        m = ((m << 2) | ((codes[b >> 4] >> (2 * (b & 15))) & 3u)) & mask;
        const int j = b - (K - 1);
        if (j >= 0 && ((valid >> j) & 1u)) f(j, m);
    }
}

// Phase A of the counting kernel: 48 packed bytes (12 little-endian dwords, byte 0 = window start 0) -> f(j, ix) for every
// window start j < min(32, limit) whose K bytes are all bases, ix = the window's m-form word.  Bytes at or behind the end of
// the input must be passed as breakers (0).
template <int K, class F>
FH_HDM void ac_lane_windows(const u32 *d, u32 limit, F &&f) {
    u32 codes[3], good[3];
    for (int c = 0; c < 3; ++c) classify_chunk(d[4 * c], d[4 * c + 1], d[4 * c + 2], d[4 * c + 3], codes[c], good[c]);
    ac_code_windows<K>(codes, (u64)good[0] | ((u64)good[1] << 16) | ((u64)good[2] << 32), limit, f);
}

// The same for a lane of a file staged in the two-bit form (fh_pack2.h): `own` / g_own = the codes and base bits of the lane's
// group of 32 positions, `next` / g_next = those of the group behind it (the halo: only its first K - 1 positions are looked at).
template <int K, class F>
FH_HDM void ac_group_windows(u64 own, u32 g_own, u64 next, u32 g_next, F &&f) {
    const u32 codes[3] = {(u32)own, (u32)(own >> 32), (u32)next};
    ac_code_windows<K>(codes, (u64)g_own | ((u64)(g_next & 0xFFFFu) << 32), 32u, f);
}

// rows to_vec emits at most from a table of 4^k bins: one per reverse-complement pair and one per palindrome (even k: 4^(k/2))
FH_HD u32 ac_max_rows(int k) { return (u32)((ac_bins(k) + ((k & 1) ? 0ull : (1ull << k))) / 2); }

} // namespace fh
