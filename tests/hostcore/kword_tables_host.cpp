// Host build of the key-word tables and of the hash made from them (finch_rs_amd/csrc/fh_core.h), for
// tests/test_kword_tables_host.py.  Test infrastructure: nothing in the product path calls it.
//   kword_pairs   : key_word_mix from the table records of every (A, B) pair of groups of one word kind,
//                   against rotl(x * c, R) * C worked out in plain 64-bit arithmetic
//   kword_hashes  : murmur_h1_fast<K> (seeded and SEED0 forms) and murmur_h1_lut<K> of given canonical words
#include <cstdint>
#include <vector>

#include "../../finch_rs_amd/csrc/fh_core.h"

using namespace fh;

static u64 direct_word(u64 x, bool k2) {
    return k2 ? rotl64(x * MURMUR_C2, 33) * MURMUR_C1 : rotl64(x * MURMUR_C1, 31) * MURMUR_C2;
}

// One two-group word of a K-byte key: I = its index, the B record from lut_rec_B (full high group) or from table P's
// builder (short high group, NBB = 2 or 3).  Returns the number of (A, B) pairs whose word differs; *n = pairs walked.
template <int K, int I>
static u64 walk_pairs(u64 *n) {
    constexpr WordGeom g = word_geom(K, I);
    static_assert(g.kind == 2, "a two-group word");
    static_assert(!g.partial || partial_word(K) == I, "the short high group is the one table P serves");
    u64 bad = 0;
    *n = 0;
    for (u32 a = 0; a < 256; ++a) {
        const Rec4 ra = lut_rec_A(a, g.is_k2);
        for (u32 b = 0; b < (1u << (2 * g.nbB)); ++b) {
            const Rec2 rb = g.partial ? lut_rec_P<K>(b) : lut_rec_B(b, 4, g.is_k2);
            KeyWords<K> w{};
            // the records' dwords go where murmur_lookup puts them
            w.a0[I] = ra.x, w.a1[I] = ra.y, w.a2[I] = ra.z;
            w.b0[I] = g.is_k2 ? rb.x : rb.y;
            w.b1[I] = g.is_k2 ? rb.y : rb.x;
            const u64 x = ascii_group_n(a, 4) | (ascii_group_n(b, g.nbB) << 32);
            bad += key_word_mix<K>(w, I) != direct_word(x, g.is_k2);
            ++*n;
        }
    }
    return bad;
}

// what: 0 / 1 = k1 / k2 word with a full high group; otherwise the K whose last word has a short high group served by P
// (K = 6, 7: a k1 word with 2, 3 bases there; K = 14, 15: a k2 word; K = 22, 23 and 30, 31: the same behind a whole block)
extern "C" int64_t kword_pairs(int what, uint64_t *n) {
    switch (what) {
    case 0: return (int64_t)walk_pairs<16, 0>(n);
    case 1: return (int64_t)walk_pairs<16, 1>(n);
    case 6: return (int64_t)walk_pairs<6, 0>(n);
    case 7: return (int64_t)walk_pairs<7, 0>(n);
    case 14: return (int64_t)walk_pairs<14, 1>(n);
    case 15: return (int64_t)walk_pairs<15, 1>(n);
    case 22: return (int64_t)walk_pairs<22, 2>(n);
    case 23: return (int64_t)walk_pairs<23, 2>(n);
    case 30: return (int64_t)walk_pairs<30, 3>(n);
    case 31: return (int64_t)walk_pairs<31, 3>(n);
    }
    return -1;
}

// out: {is the K's last two-group word a k2 word, bases of its high group, is it served by P}; -1 where K has no such word
extern "C" int kword_last_pair(int k, int *out) {
    int found = -1;
    for (int i = 0; i < n_key_words(k); ++i)
        if (word_geom(k, i).kind == 2) found = i;
    if (found < 0) return -1;
    const WordGeom g = word_geom(k, found);
    out[0] = g.is_k2, out[1] = g.nbB, out[2] = g.partial;
    return found;
}

template <int K>
static int hashes(const uint64_t *cm, uint64_t n, uint64_t seed, uint64_t *fast, uint64_t *lut) {
    std::vector<u64> T1(256), T2(256), TP(64, 0);
    for (u32 q = 0; q < 256; ++q) {
        T1[q] = lut_entry(q, 4, MURMUR_C1);
        T2[q] = lut_entry(q, 4, MURMUR_C2);
    }
    for (u32 q = 0; partial_nb(K) && q < (1u << (2 * partial_nb(K))); ++q) TP[q] = lut_entry(q, partial_nb(K), partial_const(K));
    std::vector<Rec4> A1(256), A2(256);
    std::vector<Rec2> B1(256), B2(256), P(partial_entries(K));
    for (u32 q = 0; q < 256; ++q) {
        A1[q] = lut_rec_A(q, false);
        A2[q] = lut_rec_A(q, true);
        B1[q] = lut_rec_B(q, 4, false);
        B2[q] = lut_rec_B(q, 4, true);
    }
    for (u32 q = 0; q < (u32)partial_entries(K); ++q) P[q] = lut_rec_P<K>(q);
    const LutTables LT{A1.data(), A2.data(), B1.data(), B2.data(), P.data()};
    for (uint64_t i = 0; i < n; ++i) {
        fast[i] = murmur_h1_fast<K, false>(cm[i] << pre_shift(K), seed, LT);
        if (seed == 0 && murmur_h1_fast<K, true>(cm[i] << pre_shift(K), 0, LT) != fast[i]) return -2;
        lut[i] = murmur_h1_lut<K>(cm[i], seed, T1.data(), T2.data(), TP.data());
    }
    return 0;
}

template <int K>
static int dispatch(int k, const uint64_t *cm, uint64_t n, uint64_t seed, uint64_t *fast, uint64_t *lut) {
    if (k == K) return hashes<K>(cm, n, seed, fast, lut);
    if constexpr (K > 1) return dispatch<K - 1>(k, cm, n, seed, fast, lut);
    return -1;
}

// cm: canonical k-mers in m-form (2k bits each)
extern "C" int kword_hashes(int k, const uint64_t *cm, uint64_t n, uint64_t seed, uint64_t *fast, uint64_t *lut) {
    if (k < 1 || k > 32) return -1;
    return dispatch<32>(k, cm, n, seed, fast, lut);
}
