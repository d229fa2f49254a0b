// fh_k2bw.hip -- MANY sketches per launch for K = 33..64 (two-word k-mers): the batch form of k2_sketch_w, gfx950.
//
// The scaffold is k2_batch's (fh_k2b.hip has the commentary): the files' tiles form one tile space, wave w takes the tiles
// [w q, (w + 1) q) of it and finds a tile's file by bisection of the files' first tiles; every file has its own control block,
// table partition and shard lists and runs at the ONE threshold of its descriptor; every drain goes to another shard list, the
// wave drains before it turns to another file, and counts a file's valid windows with one atomic per run.  Phase A is
// classify_tile_b, or load_tile_two_bit when the files are staged in the two-bit form.
//
// The per-lane arithmetic is k2_sketch_w's (fh_k2w.hip), statement for statement: three ring reads per lane -- its own 32
// positions and the next two lanes', lane 62's and 63's from tile tt + 1, which the ring already holds (behind a file's last
// tile that is zeroes in either form: breakers) -- window_valid_mask_w, WindowsW, murmur_lookup_w with up to 16 table lookups
// per position, the high-word reject, the AdmitQueueT<true> entry with the k-mer's high word and flush_queue<true>, whose
// upsert_w keeps the high word in the file's Ctl::kmer_hi array (fh_batch.hip owns one per partition).  The seed is a
// run-time value.  Gone, as in k2_batch: work queue, budgets, leftovers, gates, the in-launch threshold refresh, the test
// hook's hash mask and the lower threshold of a re-read.
//
// Compiled FH_NPARTS times (-DFH_PART=i), each part instantiating 8 values of K, like fh_k2w.hip.
#include <hip/hip_runtime.h>

#include "fh_core.h"
#include "fh_device.h"
#include "fh_kernels.h"
#include "fh_k2_common.h"

#ifndef FH_PART
#error "compile with -DFH_PART=<0..FH_NPARTS-1>"
#endif

namespace fh {

__device__ __forceinline__ u64 uni64(u64 v) {
    return ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(v >> 32)) << 32) | (u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)v);
}

// phase A of tile `tile` of a file, and of a file staged in the two-bit form: fh_k2b.hip's two functions, word for word
// (that file's code objects are pinned byte for byte, so they are stated again here rather than moved to a header)
__device__ __forceinline__ void classify_tile_b(const uint8_t *seq, u64 len, u64 tile, int lane, u32 *codes_ring, u32 *good_ring) {
    const u64 tile_off = tile * (u64)TILE_POS; // wave-uniform
    uint4 c0, c1;
    if (__builtin_expect(tile_off + (u64)TILE_POS <= len, 1)) {
        const uint8_t *const tb = seq + tile_off;
        const u32 vo = (u32)lane * (u32)LANE_POS;
        c0 = *reinterpret_cast<const uint4 *>(tb + (u64)vo);
        c1 = *reinterpret_cast<const uint4 *>(tb + (u64)(vo + 16u));
    } else {
        const u64 off = tile_off + (u64)lane * LANE_POS;
        c0 = load_chunk_guarded(seq, off, len);
        c1 = load_chunk_guarded(seq, off + 16, len);
    }
    u32 q0, g0, q1, g1;
    classify_chunk(c0.x, c0.y, c0.z, c0.w, q0, g0);
    classify_chunk(c1.x, c1.y, c1.z, c1.w, q1, g1);
    const u32 par = (u32)(tile & 1u);
    *reinterpret_cast<uint2 *>(&codes_ring[par * 128u + 2u * (u32)lane]) = make_uint2(q0, q1);
    good_ring[par * 64u + (u32)lane] = g0 | (g1 << 16);
}

// (the two-bit form: load_tile_two_bit, fh_k2_common.h)

template <int K>
__global__ __launch_bounds__(256, 2) void k2_batch_w(const BatchArgs a) {
    __shared__ Rec4 sA1[256];
    __shared__ Rec4 sA2[256];
    __shared__ Rec2 sB1[256];
    __shared__ Rec2 sB2[256];
    __shared__ Rec2 sP[partial_entries(K)];
    __shared__ __attribute__((aligned(16))) u32 sCodes[WAVES_PER_BLOCK][256];
    __shared__ __attribute__((aligned(16))) u32 sGood[WAVES_PER_BLOCK][128];
    __shared__ __attribute__((aligned(16))) AdmitQueueT<true> sQueue[WAVES_PER_BLOCK];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    sA1[tid] = lut_rec_A((u32)tid, false);
    sB1[tid] = lut_rec_B((u32)tid, 4, false);
    sA2[tid] = lut_rec_A((u32)tid, true);
    sB2[tid] = lut_rec_B((u32)tid, 4, true);
    for (int q = tid; q < partial_entries(K); q += 256) sP[q] = lut_rec_P<K>((u32)q);
    const LutTables LT{sA1, sA2, sB1, sB2, sP};
    __syncthreads();

    const u32 gw = blockIdx.x * (u32)WAVES_PER_BLOCK + (u32)wave;
    u32 *codes_ring = sCodes[wave];
    u32 *good_ring = sGood[wave];
    AdmitQueueT<true> *queue = &sQueue[wave];

    // this wave's stretch of the batch's tile space
    u32 t = gw * a.tiles_per_wave;
    const u32 t_stop = (t + a.tiles_per_wave < a.tiles_total) ? t + a.tiles_per_wave : a.tiles_total;
    if (t >= t_stop) return;
    // the file tile t belongs to: the last one whose first tile is <= t (files without tiles share their successor's first
    // tile and are never the last such)
    const BatchFile *const files = uniform_ptr(a.files);
    u32 f = 0;
    {
        u32 lo = 0, hi = a.n_files; // files[lo].tile0 <= t < files[hi].tile0 (hi = n_files: the end of the tile space)
        while (hi - lo > 1u) {
            const u32 mid = (lo + hi) >> 1;
            if (files[mid].tile0 <= t) lo = mid;
            else hi = mid;
        }
        f = lo;
    }
    u32 n_flush = gw * 7u; // every drain goes to another shard list (fh_k2b.hip)

#define FLUSH_BW(ctl_) ((void)flush_queue<true>(ctl_, queue, qn, (n_flush++) & (u32)(N_SHARDS - 1)))

    while (t < t_stop) {
        f = (u32)__builtin_amdgcn_readfirstlane((int)f);
        const BatchFile *const fd = files + f;
        const u32 f_tile0 = fd->tile0, f_tiles = fd->n_tiles;
        if (f_tiles == 0u || t >= f_tile0 + f_tiles) { // (an empty file, or the stretch goes on in the next one)
            ++f;
            continue;
        }
        Ctl *const ctl = (Ctl *)uni64((u64)fd->ctl);
        const u64 f_len = uni64(fd->len);
        const u64 tau = uni64(fd->tau);
        const uint8_t *const f_seq = (const uint8_t *)uni64((u64)fd->seq);
        const u32 tau_hi1 = (u32)__builtin_amdgcn_readfirstlane((int)tau_hi_bound(tau));
        const u32 rt0 = t - f_tile0;
        const u32 run_end = (t_stop < f_tile0 + f_tiles ? t_stop : f_tile0 + f_tiles);
        const u32 rt1 = run_end - f_tile0;
        u32 nvalid = 0; // per lane
        u32 qn = 0;     // occupancy of the admit queue (wave-uniform)

        if (a.two_bit) load_tile_two_bit(f_seq, rt0, lane, codes_ring, good_ring);
        else classify_tile_b(f_seq, f_len, rt0, lane, codes_ring, good_ring);
        for (u64 tt = rt0; tt < rt1; ++tt) {
            // (the tile behind: the halo of lanes 62 and 63)
            if (a.two_bit) load_tile_two_bit(f_seq, tt + 1, lane, codes_ring, good_ring);
            else classify_tile_b(f_seq, f_len, tt + 1, lane, codes_ring, good_ring);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

            const u32 par = (u32)(tt & 1u);
            const u32 ci = par * 128u + 2u * (u32)lane;
            const uint2 w0 = *reinterpret_cast<const uint2 *>(&codes_ring[ci]);
            const uint2 w1 = *reinterpret_cast<const uint2 *>(&codes_ring[(ci + 2u) & 255u]);
            const uint2 w2 = *reinterpret_cast<const uint2 *>(&codes_ring[(ci + 4u) & 255u]);
            const u32 gi = par * 64u + (u32)lane;
            const u32 g0 = good_ring[gi], g1 = good_ring[(gi + 1u) & 127u], g2 = good_ring[(gi + 2u) & 127u];

            const u64 tile_pos0 = tt * (u64)TILE_POS; // wave-uniform; a file's stream coordinates begin at 0
            const u64 lane_pos0 = tile_pos0 + (u64)lane * LANE_POS;
            const u32 limit = (f_len > lane_pos0) ? (u32)((f_len - lane_pos0) < 32 ? (f_len - lane_pos0) : 32) : 0u;
            const u32 W = window_valid_mask_w<K>(g0, g1, g2) & (limit >= 32u ? 0xFFFFFFFFu : ((1u << limit) - 1u));
            nvalid += (u32)__popc(W);

            WindowsW<K> win;
            win.init((u64)w0.x | ((u64)w0.y << 32), (u64)w1.x | ((u64)w1.y << 32), (u64)w2.x | ((u64)w2.y << 32));
            u32 Wc = W; // valid bits of the current round in its low byte
#pragma unroll 1
            for (int c = 0; c < LANE_POS / 8; ++c) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    u32 cm[4];
                    bool is_rc;
                    win.canonical(u, cm, is_rc);
                    KeyWords<K> kw;
                    murmur_lookup_w<K>(cm, LT, kw);
                    const HashParts hp = murmur_finish_parts<K, false>(kw, a.seed);
                    const bool cand = parts_hi_plus1(hp) <= tau_hi1;
                    if (__builtin_expect(__any(cand), 0)) { // wave-uniform branch
                        const u64 h = parts_hash(hp);
                        const bool take = (h <= tau) && ((Wc >> u) & 1u);
                        const u64 mask = __ballot(take);
                        const u32 cnt = (u32)__popcll(mask);
                        if (cnt) {
                            if (qn + cnt > (u32)QCAP) {
                                FLUSH_BW(ctl);
                                qn = 0;
                            }
                            const u32 my = qn + __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0u));
                            if (take) {
                                const U128 km = kmer_words_w<K>(cm);
                                queue->h[my] = h;
                                queue->k[my] = km.lo;
                                queue->khi[my] = km.hi;
                                const u64 pos = tile_pos0 + (u64)((u32)lane * (u32)LANE_POS + (u32)(8 * c + u));
                                queue->p[my] = pos | ((u64)(is_rc ? 1u : 0u) << 63);
                            }
                            qn += cnt;
                        }
                    }
                }
                win.advance8();
                Wc >>= 8;
            }
            __builtin_amdgcn_wave_barrier();
            if (qn >= (u32)(QCAP / 2) || (qn && tt + 1 == rt1)) { // drain when half full, and before the wave turns to another file
                FLUSH_BW(ctl);
                qn = 0;
            }
        }
        // total_kmers (mash.rs:35) of this file: one atomic per wave and run
        for (int off = 32; off > 0; off >>= 1) nvalid += __shfl_xor(nvalid, off);
        if (lane == 0 && nvalid) atomicAdd((unsigned long long *)&ctl->kmer_counts[gw & 255u], (unsigned long long)nvalid);
        t = run_end;
        ++f;
    }
#undef FLUSH_BW
}

constexpr int PARTBW_LO = 33 + FH_PART * (32 / FH_NPARTS);
constexpr int PARTBW_HI = 32 + (FH_PART + 1) * (32 / FH_NPARTS);

template <int K>
static hipError_t launch_k2bw_dispatch(int k, const BatchArgs &a, uint32_t n_waves, hipStream_t st) {
    if (k == K) {
        hipLaunchKernelGGL((k2_batch_w<K>), dim3((n_waves + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK), dim3(64 * WAVES_PER_BLOCK), 0, st, a);
        return hipGetLastError();
    }
    if constexpr (K > PARTBW_LO) return launch_k2bw_dispatch<K - 1>(k, a, n_waves, st);
    return hipErrorInvalidValue;
}

#define FH_CAT2(a, b) a##b
#define FH_CAT(a, b) FH_CAT2(a, b)
hipError_t FH_CAT(launch_k2bw_part, FH_PART)(int k, const BatchArgs &a, uint32_t n_waves, hipStream_t st) {
    if (k < PARTBW_LO || k > PARTBW_HI) return hipErrorInvalidValue;
    return launch_k2bw_dispatch<PARTBW_HI>(k, a, n_waves, st);
}

} // namespace fh
