// Host build of the per-lane kernel arithmetic (finch_rs_amd/csrc/fh_core.h) for logic tests on a
// GPU-less machine.  Test infrastructure: it is NOT part of libfinch_hip.so and nothing in the
// product path calls it.  It walks a byte stream exactly the way one lane of the sketch kernel does
// (32 start positions per lane segment, classification of 16-byte chunks, state initialised from the
// first K-1 bases, LUT-based murmur3) and reports per-position results.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../finch_rs_amd/csrc/fh_core.h"

using namespace fh;

template <int K>
static int run(const uint8_t *seq, uint64_t len, uint64_t seed, uint64_t *hashes, uint8_t *valid, uint8_t *isrc,
               uint64_t *canon) {
    std::vector<uint8_t> buf(((len + 31) / 32) * 32 + 96, 0);
    memcpy(buf.data(), seq, len);
    std::vector<u64> T1(256), T2(256), TP(64, 0);
    for (u32 q = 0; q < 256; ++q) {
        T1[q] = lut_entry(q, 4, MURMUR_C1);
        T2[q] = lut_entry(q, 4, MURMUR_C2);
    }
    const int pnb = partial_nb(K);
    for (u32 q = 0; q < (1u << (2 * pnb)); ++q)
        if (pnb) TP[q] = lut_entry(q, pnb, partial_const(K));
    // the kernel's tables (second stage folded in), built exactly as the workgroup prologue builds them
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
    for (uint64_t s = 0; s < len; s += 32) {
        u32 cw[4], gw[4];
        for (int c = 0; c < 4; ++c) {
            u32 d[4];
            memcpy(d, buf.data() + s + 16 * c, 16);
            classify_chunk(d[0], d[1], d[2], d[3], cw[c], gw[c]);
        }
        const u64 clo = (u64)cw[0] | ((u64)cw[1] << 32), chi = (u64)cw[2] | ((u64)cw[3] << 32);
        const u64 g64 = (u64)gw[0] | ((u64)gw[1] << 16) | ((u64)gw[2] << 32) | ((u64)gw[3] << 48);
        Windows<K> win;
        win.init(clo, chi);
        const u32 W = window_valid_mask<K>(g64 & 0x7FFFFFFFFFFFFFFFull);
        for (int j = 0; j < 32; ++j) {
            const uint64_t p = s + j;
            if (p >= len) break;
            bool rc;
            const u64 cm = win.canonical(j, rc);
            valid[p] = (W >> j) & 1u;
            isrc[p] = rc ? 1 : 0;
            canon[p] = cm >> pre_shift(K);
            const u64 h_ref = murmur_h1_lut<K>(cm >> pre_shift(K), seed, T1.data(), T2.data(), TP.data());
            const u64 h_fast = murmur_h1_fast<K, false>(cm, seed, LT);
            if (h_fast != h_ref) return -2;
            if (seed == 0 && murmur_h1_fast<K, true>(cm, 0, LT) != h_ref) return -3;
            hashes[p] = h_fast;
        }
    }
    // The segment kernel's form (fh_k2s.hip): the buffer as ONE tile's three strings, a round's view cut at EVERY position p0
    // (a lane's p0 = stride * lane + round * seg_round(K) is any number), Windows<K, seg_doff(K)> and the 64-bit validity mask:
    // every window of the round against what the walk above found at that position.
    {
        const u32 NCH = (u32)(buf.size() / 16);
        std::vector<u32> Fc(NCH + 3, 0u), Rv(NCH + 2, 0u), Gd(NCH / 2 + 3, 0u);
        for (u32 i = 0; i < NCH; ++i) {
            u32 d[4], q, g;
            memcpy(d, buf.data() + 16 * (size_t)i, 16);
            classify_chunk(d[0], d[1], d[2], d[3], q, g);
            Fc[1 + i] = ~q;
            Rv[NCH - 1 - i] = pairrev32(q);
            reinterpret_cast<unsigned short *>(Gd.data())[i] = (unsigned short)g;
        }
        constexpr int R = seg_round(K), DOFF = seg_doff(K);
        static_assert(R + K - 1 <= 64, "a round's windows lie inside the 64-base view");
        for (uint64_t p0 = 0; p0 + 64 + DOFF <= 16ull * NCH && p0 < len; ++p0) {
            u32 nc[5], d[5];
            seg_cut_views<K>(Fc.data(), Rv.data(), NCH, (u32)p0, nc, d);
            Windows<K, DOFF> win;
            win.init_words(nc, d);
            const u64 W = window_valid_mask64<K>(seg_good_bits(Gd.data(), (u32)p0));
            for (int j = 0; j < R; ++j) {
                const uint64_t p = p0 + j;
                if (p >= len) break;
                if (((W >> j) & 1u) != valid[p]) return -5;
                if (!valid[p]) continue;
                bool rc;
                const u64 cm = win.canonical(j, rc);
                if ((cm >> pre_shift(K)) != canon[p] || (rc ? 1 : 0) != isrc[p]) return -6;
                if (win.canonical_word(j) != cm || win.strand_of(j) != rc) return -7;
            }
        }
    }
    return 0;
}

template <int K>
static int dispatch(int k, const uint8_t *seq, uint64_t len, uint64_t seed, uint64_t *hashes, uint8_t *valid,
                    uint8_t *isrc, uint64_t *canon) {
    if (k == K) return run<K>(seq, len, seed, hashes, valid, isrc, canon);
    if constexpr (K > 1) return dispatch<K - 1>(k, seq, len, seed, hashes, valid, isrc, canon);
    return -1;
}

extern "C" int fhcore_positions(const uint8_t *seq, uint64_t len, int k, uint64_t seed, uint64_t *hashes,
                                uint8_t *valid, uint8_t *isrc, uint64_t *canon) {
    if (k < 1 || k > 32) return -1;
    return dispatch<32>(k, seq, len, seed, hashes, valid, isrc, canon);
}

// K = 33..64 (WindowsW): the same walk with three code words per lane segment; canon receives two words per position
// (low, high) of the canonical k-mer in m-form
template <int K>
static int run_w(const uint8_t *seq, uint64_t len, uint64_t seed, uint64_t *hashes, uint8_t *valid, uint8_t *isrc,
                 uint64_t *canon) {
    std::vector<uint8_t> buf(((len + 31) / 32) * 32 + 128, 0);
    memcpy(buf.data(), seq, len);
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
    for (uint64_t s = 0; s < len; s += 32) {
        u32 cw[6], gw[6];
        for (int c = 0; c < 6; ++c) {
            u32 d[4];
            memcpy(d, buf.data() + s + 16 * c, 16);
            classify_chunk(d[0], d[1], d[2], d[3], cw[c], gw[c]);
        }
        const u64 c0 = (u64)cw[0] | ((u64)cw[1] << 32), c1 = (u64)cw[2] | ((u64)cw[3] << 32), c2 = (u64)cw[4] | ((u64)cw[5] << 32);
        WindowsW<K> win;
        win.init(c0, c1, c2);
        const u32 W = window_valid_mask_w<K>(gw[0] | (gw[1] << 16), gw[2] | (gw[3] << 16), gw[4] | (gw[5] << 16));
        for (int j = 0; j < 32; ++j) {
            const uint64_t p = s + j;
            if (p >= len) break;
            bool rc;
            u32 cm[4];
            win.canonical(j, cm, rc);
            valid[p] = (W >> j) & 1u;
            isrc[p] = rc ? 1 : 0;
            const U128 km = kmer_words_w<K>(cm);
            canon[2 * p] = km.lo;
            canon[2 * p + 1] = km.hi;
            hashes[p] = murmur_h1_fast_w<K>(cm, seed, LT);
        }
        // the kernel's form: four rounds of eight positions, the strings moved on between rounds
        WindowsW<K> adv;
        adv.init(c0, c1, c2);
        for (int c = 0; c < 4; ++c) {
            for (int u = 0; u < 8; ++u) {
                bool rc0, rc1;
                u32 a[4], b[4];
                adv.canonical(u, a, rc0);
                win.canonical(8 * c + u, b, rc1);
                if (rc0 != rc1 || memcmp(a, b, 16) != 0) return -4;
            }
            adv.advance8();
        }
    }
    return 0;
}

template <int K>
static int dispatch_w(int k, const uint8_t *seq, uint64_t len, uint64_t seed, uint64_t *hashes, uint8_t *valid,
                      uint8_t *isrc, uint64_t *canon) {
    if (k == K) return run_w<K>(seq, len, seed, hashes, valid, isrc, canon);
    if constexpr (K > 33) return dispatch_w<K - 1>(k, seq, len, seed, hashes, valid, isrc, canon);
    return -1;
}

extern "C" int fhcore_positions_w(const uint8_t *seq, uint64_t len, int k, uint64_t seed, uint64_t *hashes,
                                  uint8_t *valid, uint8_t *isrc, uint64_t *canon) {
    if (k < 33 || k > 64) return -1;
    return dispatch_w<64>(k, seq, len, seed, hashes, valid, isrc, canon);
}

extern "C" uint32_t fhcore_qoct_index(uint64_t x) { return qoct_index(x); }
extern "C" uint64_t fhcore_qoct_upper_edge(uint32_t q) { return qoct_upper_edge(q); }

extern "C" void fhcore_synth(uint8_t *genome, uint64_t glen, uint8_t *reads, uint64_t first, uint64_t n, uint32_t rl,
                             uint64_t seed, uint32_t sub_ppm, uint32_t n_ppm) {
    for (uint64_t i = 0; i < glen; ++i) genome[i] = synth_genome_base(seed, i);
    for (uint64_t r = 0; r < n; ++r)
        for (uint32_t j = 0; j <= rl; ++j)
            reads[r * (rl + 1) + j] = synth_read_byte(genome, glen, first + r, j, rl, seed, sub_ppm, n_ppm);
}

// high-word prefilter (fh_core.h HashParts): returns the number of violations of
//   parts_hash(p) <= tau  =>  parts_hi_plus1(p) <= tau_hi_bound(tau)
// over the given (a, b, tau) triples, and writes the prefilter's pass count (selectivity check)
extern "C" uint64_t fhcore_prefilter_check(const uint64_t *a, const uint64_t *b, const uint64_t *tau, uint64_t n,
                                           uint64_t *n_pass, uint64_t *n_true) {
    uint64_t bad = 0, pass = 0, tr = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const HashParts p{a[i], b[i]}; // (ka, kb)
        const bool truth = parts_hash(p) <= tau[i];
        const bool cand = parts_hi_plus1(p) <= tau_hi_bound(tau[i]);
        if (truth && !cand) ++bad;
        pass += cand;
        tr += truth;
    }
    *n_pass = pass;
    *n_true = tr;
    return bad;
}

// classification of n 16-byte chunks: codes (32 bits, base i at bits [2i, 2i+2)) and good bits per chunk
extern "C" void fhcore_classify(const uint8_t *bytes, uint64_t n_chunks, uint32_t *codes, uint32_t *good) {
    for (uint64_t c = 0; c < n_chunks; ++c) {
        u32 d[4];
        memcpy(d, bytes + 16 * c, 16);
        classify_chunk(d[0], d[1], d[2], d[3], codes[c], good[c]);
    }
}

// ---- the segment kernels' geometry (fh_core.h: seg_sub_for, seg_geom, seg_lane_take, segw_geom ...) ----
// One tile walked the way k2_sketch_seg<k> / k2_sketch_ws<k> walk it, with the helpers the kernels compile: every lane, every
// round, every position a lane may take before the launch's range and validity cut it down.  0 = all is well; otherwise which
// property fails (tests/test_seg_geometry_host.py names them):
//   1 a tile offset nobody takes      2 a tile offset taken twice (a doubled count)      3 a lane takes more than a round holds
//   4 a position outside the tile     5 a view that leaves the tile's strings            6 LDS words outside K2S_*_DW / K2WS_*_DW
//   7 rounds >= c0 and rounds < c0 do not make up the tile for some resume round c0      8 no such kernel form
// `lost`, if given, receives the number of tile offsets nobody takes.
extern "C" int fhcore_seg_check(uint32_t k, uint32_t S, uint32_t sub, uint32_t *lost) {
    if (lost) *lost = 0;
    if (k < 1 || k > 64 || S <= k || (sub != 1 && sub != 2 && sub != 4) || (k > 32 && sub != 1)) return 8;
    std::vector<uint8_t> taken;
    std::vector<u32> per_round;
    u32 tile_pos, NR;
    int rc = 0;
    auto fail = [&](int code) { if (!rc) rc = code; };
    if (k <= 32) {
        const u32 RO = (u32)seg_ro((int)k), DOFF = (u32)seg_doff((int)k), ND = DOFF ? 5u : 4u;
        const int PRE = pre_shift((int)k);
        const SegGeom g = seg_geom(k, RO, S, seg_shift(sub));
        tile_pos = g.tile_pos, NR = g.NR;
        if (tile_pos != seg_tile_pos(S, sub) || (tile_pos & 15u)) fail(4);
        taken.assign(tile_pos, 0);
        per_round.assign(NR, 0);
        // phase A: chunk i < NCH goes to Fc[1 + i], Rv[NCH - 1 - i], half-word i of Gd
        if (g.NCH > K2S_NCH_MAX || g.NCH + 1u > K2S_FC_DW || g.NCH > K2S_RV_DW || (g.NCH + 1u) / 2u > K2S_G_DW) fail(6);
        for (u32 c = 0; c < NR; ++c) {
            const u32 rc0 = seg_round_off(RO, c);
            for (u32 lane = 0; lane < 64; ++lane) {
                const u32 p0 = seg_start(g, S, lane) + rc0;
                // the views are cut for every lane of a running round, whatever it takes (seg_cut_views, seg_good_bits)
                if (!(p0 + 63u + DOFF < 16u * g.NCH)) fail(5);
                const int gc = (int)(2u * p0) - PRE;
                const u32 ic = (u32)((gc >> 5) + 1);
                const u32 gd = 2u * (16u * g.NCH - 64u - DOFF - p0), id = gd >> 5;
                if (gc < -32 || ic + 5u >= K2S_FC_DW || id + ND >= K2S_RV_DW || (p0 >> 5) + 2u >= K2S_G_DW) fail(6);
                const u32 n = seg_lane_take(g, RO, lane, rc0);
                if (n > RO) fail(3);
                for (u32 j = 0; j < n && j < RO; ++j) {
                    if (p0 + j >= tile_pos) { fail(4); continue; }
                    if (taken[p0 + j] < 255) taken[p0 + j]++;
                    per_round[c]++;
                }
            }
        }
    } else {
        const SegGeomW g = segw_geom(S);
        tile_pos = g.tile_pos, NR = g.NR;
        taken.assign(tile_pos, 0);
        per_round.assign(NR, 0);
        if (g.NCH > K2WS_NCH_MAX || g.NCH > K2WS_C_DW || (g.NCH + 1u) / 2u > K2WS_G_DW) fail(6);
        for (u32 c = 0; c < NR; ++c) {
            const u32 rc0 = 32u * c;
            for (u32 lane = 0; lane < 64; ++lane) {
                const u32 p0 = segw_start(S, lane) + rc0;
                if (!(p0 + 95u < 16u * g.NCH)) fail(5); // a 96-base view
                if ((p0 >> 4) + 6u >= K2WS_C_DW || (p0 >> 5) + 3u >= K2WS_G_DW) fail(6);
                const u32 n = segw_round_nmax(S, rc0);
                if (n > 32u) fail(3);
                for (u32 j = 0; j < n && j < 32u; ++j) {
                    if (p0 + j >= tile_pos) { fail(4); continue; }
                    if (taken[p0 + j] < 255) taken[p0 + j]++;
                    per_round[c]++;
                }
            }
        }
    }
    u32 n_lost = 0, n_twice = 0;
    for (u32 p = 0; p < tile_pos; ++p) n_lost += taken[p] == 0, n_twice += taken[p] > 1;
    if (lost) *lost = n_lost;
    if (n_twice) fail(2);
    if (n_lost) fail(1);
    // a wave that stopped behind round c0 - 1 hands (tile, c0) back; whoever resumes walks rounds c0 .. NR - 1 with the same helpers
    // (they take the round's number and nothing of the wave's past): the two parts must make up the tile, each offset once
    for (u32 c0 = 0; c0 <= NR; ++c0) {
        u64 before = 0, after = 0;
        for (u32 c = 0; c < NR; ++c) (c < c0 ? before : after) += per_round[c];
        if (before + after != tile_pos || n_twice || n_lost) fail(7);
    }
    return rc;
}

extern "C" uint32_t fhcore_seg_sub_for(uint32_t k, uint32_t S) { return seg_sub_for(k, S); }
extern "C" int fhcore_seg_launch_ok(uint32_t k, uint32_t S, uint32_t sub) { return seg_launch_ok(k, S, sub) ? 1 : 0; }
// out: RO, H, LAST, NR, tile_pos, min stride, max stride of one lane, max record stride (K > 32: rounds of 32, a lane per record)
extern "C" void fhcore_seg_geom(uint32_t k, uint32_t S, uint32_t sub, uint32_t *out) {
    if (k <= 32) {
        const u32 RO = (u32)seg_ro((int)k);
        const SegGeom g = seg_geom(k, RO, S, seg_shift(sub));
        out[0] = RO, out[1] = g.H, out[2] = g.LAST, out[3] = g.NR, out[4] = g.tile_pos;
    } else {
        const SegGeomW g = segw_geom(S);
        out[0] = 32u, out[1] = S, out[2] = S, out[3] = g.NR, out[4] = g.tile_pos;
    }
    out[5] = SEG_MIN_STRIDE, out[6] = SEG_MAX_STRIDE, out[7] = SEG_MAX_RECORD;
}
