// fh_batch_large.hip -- the epilogue of a batch of files sketched at Mash sizes above 3000 (fh_batch_new_large, fh_batch.hip):
// k_batch_epilogue_large, hand-written for gfx950.  One workgroup of 1024 finishes one file, like k_batch_epilogue
// (fh_kernels.hip), but a file's live set -- about 4 n hashes, up to 72 Ki -- no longer fits a workgroup's LDS, so the
// phases that need all of it work out of device memory and only the n survivors (at most 16 384) come into LDS:
//
//   flatten   the 256 shard lists of new inserts -> the live list (the scan and copy of small_epilogue_body);
//   keys      the live entries' hashes, gathered ONCE from the 40-byte entries into the file's key scratch (u64 each: 64 Ki
//             keys are 512 KiB and stay in L2 for the passes below);
//   select    the n-th smallest key, MSB first: a 2048-bin histogram in LDS over the top 11 bits any key uses, then 11 bits
//             more per pass over the keys that share the prefix found so far, until at most 1024 candidates are left; those
//             are ranked against each other in LDS.  Hashes spread evenly: 72 Ki keys leave ~36 in the bin of the first pass,
//             so the select is two passes over the scratch; keys that do not spread only cost more passes (six at most);
//   partition survivors (key <= the n-th) -> their keys into LDS, their slots into the free tail of the dropped-slot list;
//             everything else -> the dropped-slot list, which the reset clears;
//   sort      chunks of 4096 (key, slot) pairs through the LDS bitonic network, the keys in place -- all 16 384 sorted keys
//             stay in LDS (128 KiB), only one chunk's slots at a time (16 KiB) -- then every survivor takes its row by rank:
//             its index in its own chunk plus, by bisection in LDS, the keys below it in the other chunks (keys are distinct:
//             the ranks are a permutation).  Its slot goes to live[rank]: the live list is in to_vec order like after any sort;
//   gather    rows from the live list into the slot's pinned columns, coalesced; the control block mirrored last;
//   reset     FIN_OK_RESET: the slots of the live and dropped lists cleared, the control block re-initialised; anything
//             else: the whole partition swept.
//
// Barriers: every branch that holds a barrier is taken on a value all 1024 threads read from the same LDS word (s_word, s_bcast,
// s_off), never on something a thread computed from its own data.  Words of the control block that this kernel or the sketch
// kernel before it writes are read with agent-scope atomic loads (vector loads); only the descriptor comes by scalar load.
#include <hip/hip_runtime.h>

#include <atomic>

#include "fh_core.h"
#include "fh_device.h"
#include "fh_epilogue_dev.h"
#include "fh_kernels.h"

namespace fh {

namespace {

constexpr u32 LG_CH = (u32)SMALL_SORT_MAX;                                     // pairs per pass through the network
constexpr size_t LG_LDS_BYTES = (size_t)LARGE_MAX_ROWS * 8 + (size_t)LG_CH * 4; // sorted keys + one chunk's slots: 144 KiB
constexpr u32 LG_BINS = 2048, LG_BITS = 11, LG_LIST = 1024;
static_assert(LARGE_MAX_ROWS % LG_CH == 0, "whole chunks");
static_assert(LG_BINS * 4 + LG_LIST * 8 <= LG_LDS_BYTES, "the select's histogram and candidate list use the block the sort uses later");

__device__ __forceinline__ u32 ld32(const u32 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// s_word: what the whole workgroup decides on
enum { W_M = 0, W_BAD = 1, W_ND0 = 2, W_FIN = 3, W_N = 4 };

} // namespace

__global__ __launch_bounds__(1024) void k_batch_epilogue_large(const EpiLargeArgs *args, u32 read_first) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ u32 s_wsum[16];
    __shared__ u64 s_bcast[2];
    __shared__ u32 s_cnt[2];
    __shared__ u32 s_off[N_SHARDS + 1];
    __shared__ u32 s_word[W_N];
    const EpiLargeArgs a = args[blockIdx.x];
    Ctl *const ctl = a.ctl;
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    u64 *const skeys = reinterpret_cast<u64 *>(smem);                                      // [LARGE_MAX_ROWS]
    u32 *const sslots = reinterpret_cast<u32 *>(smem + (size_t)LARGE_MAX_ROWS * 8);        // [LG_CH]
    u32 *const hist = reinterpret_cast<u32 *>(smem);                                       // [LG_BINS]   } the select, before
    u64 *const list = reinterpret_cast<u64 *>(smem + (size_t)LG_BINS * 4);                 // [LG_LIST]   } the sort
    const u32 live_cap = a.live_cap, shard_cap = a.shard_cap, cap = a.cap; // (the partition's geometry, as k_batch_init put it into the control block)

    // ---- flatten: shard lists -> flat live list (small_epilogue_body's: an exclusive scan of the 256 cursors, then one entry
    // per thread and trip, its shard found by bisection of the offsets) ----
    static_assert(N_SHARDS == 256, "the scan below is written for 256 shards");
    const u32 M0 = ld32(&ctl->n_live);
    {
        u32 c = 0;
        if (tid < (u32)N_SHARDS) {
            c = ld32(&a.shard_cnt[tid * SHARD_STRIDE]);
            if (c > shard_cap) c = shard_cap; // overflow already flagged by the inserter
        }
        u32 inc = c;
        for (int off = 1; off < 64; off <<= 1) {
            const u32 t = __shfl_up(inc, off);
            if (lane >= (u32)off) inc += t;
        }
        if (tid < (u32)N_SHARDS && lane == 63u) s_wsum[wave] = inc;
        __syncthreads();
        if (tid < (u32)N_SHARDS) {
            u32 base = 0;
            for (u32 w = 0; w < wave; ++w) base += s_wsum[w];
            s_off[tid] = base + inc - c;
            if (tid == (u32)N_SHARDS - 1) s_off[N_SHARDS] = base + inc;
        }
        __syncthreads();
        const u32 total = s_off[N_SHARDS];
        const u32 *buf = a.shard_buf;
        for (u32 i = tid; i < total; i += 1024u) {
            u32 lo = 0, hi = (u32)N_SHARDS;
            while (hi - lo > 1u) {
                const u32 mid = (lo + hi) >> 1;
                if (s_off[mid] <= i) lo = mid;
                else hi = mid;
            }
            const u32 v = buf[(size_t)lo * shard_cap + (i - s_off[lo])];
            if (M0 < live_cap && i < live_cap - M0) a.live[M0 + i] = v;
            else atomicExch(&ctl->overflow, 1u);
        }
        if (tid < (u32)N_SHARDS) a.shard_cnt[tid * SHARD_STRIDE] = 0;
        __syncthreads(); // (the appended slots and an overflow flag are out)
        if (tid == 0) {
            u32 n = M0 <= live_cap ? M0 : live_cap;
            n = total < live_cap - n ? n + total : live_cap;
            if (total) {
                ctl->inserted_total += total;
                ctl->n_live = n;
                ctl->sorted = 0;
            }
            // what cannot be finished here: an overflow (table, shard list, live list), no room for the dropped slots and the
            // survivors' in the dropped-slot list, rows the columns or the LDS block do not hold
            const u32 nd0 = ld32(&ctl->n_dead);
            const u64 keep = (u64)n > a.size ? a.size : (u64)n;
            const bool bad = ld32(&ctl->overflow) != 0u || ld32(&ctl->need_big) != 0u || nd0 > a.dead_cap || n > a.dead_cap - nd0 ||
                             keep > (u64)LARGE_MAX_ROWS || keep > (u64)a.out_stride || n > live_cap; // (the key scratch holds live_cap keys)
            s_word[W_M] = n;
            s_word[W_BAD] = bad ? 1u : 0u;
            s_word[W_ND0] = nd0;
            s_word[W_FIN] = 0u;
        }
        __syncthreads();
    }
    const u32 M = s_word[W_M], nd0 = s_word[W_ND0];
    const bool bad = s_word[W_BAD] != 0u;
    const u32 keep = (u64)M > a.size ? (u32)a.size : M, ndrop = M - keep;

    if (!bad) {
        // ---- keys: one gather from the entries ----
        u64 kor = 0;
        for (u32 i = tid; i < M; i += 1024u) {
            const u64 key = a.table[a.live[i]].hash;
            a.keys[i] = key;
            kor |= key;
        }
        for (int off = 32; off > 0; off >>= 1) kor |= __shfl_xor(kor, off);
        if (tid == 0) s_bcast[0] = 0;
        if (tid < 2) s_cnt[tid] = 0;
        __syncthreads();
        if (lane == 0 && kor) atomicOr((unsigned long long *)&s_bcast[0], (unsigned long long)kor);
        __syncthreads();
        kor = s_bcast[0];
        __syncthreads();

        // ---- select: the keep-th smallest key (only if something is to be dropped) ----
        u64 tau = EMPTY64;
        if (keep < M) {
            int hi = kor ? 64 - __builtin_clzll(kor) : 0; // the keys' bits [0, hi) are still undecided
            u64 prefix = 0, pmask = 0;
            u32 rank = keep, in_bin = M;
            for (int pass = 0; pass < 8 && in_bin > LG_LIST; ++pass) { // (in_bin comes from LDS; 64 bits are gone after six passes)
                const int width = hi < (int)LG_BITS ? hi : (int)LG_BITS, lo = hi - width;
                const u32 bmask = (1u << width) - 1u;
                for (u32 i = tid; i < LG_BINS; i += 1024u) hist[i] = 0;
                __syncthreads();
                for (u32 i = tid; i < M; i += 1024u) {
                    const u64 key = a.keys[i];
                    if ((key & pmask) == prefix) atomicAdd(&hist[(u32)(key >> lo) & bmask], 1u);
                }
                __syncthreads();
                // inclusive scan of the 2048 bins, two per thread
                const u32 c0 = hist[2u * tid], c1 = hist[2u * tid + 1u];
                u32 inc = c0 + c1;
                for (int off = 1; off < 64; off <<= 1) {
                    const u32 t = __shfl_up(inc, off);
                    if (lane >= (u32)off) inc += t;
                }
                if (lane == 63u) s_wsum[wave] = inc;
                __syncthreads();
                u32 base = 0;
                for (u32 w = 0; w < wave; ++w) base += s_wsum[w];
                inc += base;
                const u32 exc = inc - c0 - c1;
                if (exc < rank && rank <= inc) { // this thread's pair of bins holds the rank-th key of the candidates
                    const bool second = rank > exc + c0;
                    s_bcast[0] = (u64)(2u * tid + (second ? 1u : 0u));                             // the bin
                    s_bcast[1] = (u64)(second ? exc + c0 : exc) | ((u64)(second ? c1 : c0) << 32); // candidates below it | in it
                }
                __syncthreads();
                const u32 bin = (u32)s_bcast[0], below = (u32)s_bcast[1];
                in_bin = (u32)(s_bcast[1] >> 32);
                __syncthreads();
                rank -= below;
                prefix |= (u64)bin << lo;
                pmask |= (u64)bmask << lo;
                hi = lo;
            }
            // the candidates left (distinct keys: one, once every bit is decided) ranked against each other
            for (u32 i = tid; i < M; i += 1024u) {
                const u64 key = a.keys[i];
                if ((key & pmask) == prefix) {
                    const u32 at = atomicAdd(&s_cnt[0], 1u);
                    if (at < LG_LIST) list[at] = key;
                }
            }
            if (tid == 0) s_bcast[0] = EMPTY64;
            __syncthreads();
            const u32 n_list = s_cnt[0] < LG_LIST ? s_cnt[0] : LG_LIST;
            if (tid < n_list) {
                const u64 mine = list[tid];
                u32 smaller = 0;
                for (u32 j = 0; j < n_list; ++j) smaller += list[j] < mine ? 1u : 0u;
                if (smaller + 1u == rank) s_bcast[0] = mine;
            }
            __syncthreads();
            tau = s_bcast[0];
            __syncthreads();
            if (tid == 0) s_cnt[0] = 0;
            __syncthreads();
        }

        // ---- partition: survivors' keys -> LDS, their slots -> the free tail of the dropped-slot list; the rest -> dropped ----
        u32 *const surv = a.dead + nd0 + ndrop; // [keep]
        for (u32 i0 = wave * 64u; i0 < M; i0 += 1024u) { // (a wave's lanes make the same trips)
            const u32 i = i0 + lane;
            const bool act = i < M;
            const u64 key = act ? a.keys[i] : 0ull;
            const u32 sl = act ? a.live[i] : 0u;
            const bool is_s = act && (keep == M || key <= tau), is_d = act && !is_s;
            const u64 ms = __ballot(is_s), md = __ballot(is_d);
            u32 bs = 0, bd = 0;
            if (lane == 0) {
                if (ms) bs = atomicAdd(&s_cnt[0], (u32)__popcll(ms));
                if (md) bd = atomicAdd(&s_cnt[1], (u32)__popcll(md));
            }
            bs = __shfl(bs, 0);
            bd = __shfl(bd, 0);
            const u64 below = (1ull << lane) - 1ull;
            if (is_s) {
                const u32 at = bs + (u32)__popcll(ms & below);
                if (at < keep) {
                    skeys[at] = key;
                    surv[at] = sl;
                }
            } else if (is_d) {
                const u32 at = bd + (u32)__popcll(md & below);
                if (at < ndrop) a.dead[nd0 + at] = sl;
            }
        }
        __syncthreads();
        if (tid == 0 && (s_cnt[0] != keep || s_cnt[1] != ndrop)) { // (keys are distinct, so this cannot be; were it, the file goes the long way)
            ctl->need_big = 1u;
            s_word[W_BAD] = 1u;
        }
        __syncthreads();
    }
    const bool bad2 = s_word[W_BAD] != 0u;
    if (!bad2) {
        u32 *const surv = a.dead + nd0 + ndrop;
        // ---- sort: chunk by chunk through the network, keys in place ----
        const u32 nchunks = (keep + LG_CH - 1u) / LG_CH;
        for (u32 c = 0; c < nchunks; ++c) {
            const u32 base = c * LG_CH, n = keep - base < LG_CH ? keep - base : LG_CH;
            u32 N = 1;
            while (N < n) N <<= 1;
            for (u32 i = tid; i < N; i += 1024u) {
                if (i < n) {
                    sslots[i] = surv[base + i];
                } else {
                    skeys[base + i] = EMPTY64;
                    sslots[i] = 0xFFFFFFFFu;
                }
            }
            __syncthreads();
            bitonic_lds(skeys + base, sslots, N);
            for (u32 i = tid; i < n; i += 1024u) surv[base + i] = sslots[i];
            __syncthreads();
        }
        // ---- rows by rank: the live list in to_vec order ----
        for (u32 i = tid; i < keep; i += 1024u) {
            const u64 key = skeys[i];
            const u32 own = i / LG_CH;
            u32 rank = i - own * LG_CH;
            for (u32 o = 0; o < nchunks; ++o) {
                if (o == own) continue;
                u32 lo = o * LG_CH, hi = lo + LG_CH < keep ? lo + LG_CH : keep; // first index in [lo, hi] whose key is not below `key`
                const u32 first = lo;
                while (lo < hi) {
                    const u32 mid = (lo + hi) >> 1;
                    if (skeys[mid] < key) lo = mid + 1u;
                    else hi = mid;
                }
                rank += lo - first;
            }
            a.live[rank] = surv[i];
        }
        if (tid == 0) {
            ctl->n_live = keep;
            ctl->sorted = 1u;
            ctl->n_dead = nd0 + ndrop;
        }
        __syncthreads();
        // ---- gather: to_vec (mash.rs:86-102) into the host's columns ----
        const size_t st = a.out_stride;
        u64 *o_hash = a.out, *o_kmer = o_hash + st, *o_pos = o_kmer + st;
        u32 *o_count = (u32 *)(o_pos + st), *o_extra = o_count + st;
        for (u32 i = tid; i < keep; i += 1024u) {
            const Entry e = a.table[a.live[i]];
            o_hash[i] = e.hash;
            const u64 occ = e.count + e.extra; // the table counts the two strands separately (fh_device.h)
            o_count[i] = occ > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)occ;
            o_extra[i] = e.extra > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)e.extra;
            o_kmer[i] = e.kmer;
            o_pos[i] = e.pos;
        }
        if (tid == 0) {
            ctl->sorted = FIN_OK_RESET;
            s_word[W_FIN] = FIN_OK_RESET;
        }
    }
    // ---- the control block as the host reads it (fh_batch_wait asks it whether the file is taken) ----
    __syncthreads();
    {
        const u32 *src = reinterpret_cast<const u32 *>(ctl);
        u32 *dst = reinterpret_cast<u32 *>(a.h_ctl);
        for (u32 i = tid; i < (u32)(sizeof(Ctl) / 4); i += 1024u) dst[i] = ld32(src + i);
        __threadfence_system();
    }
    __syncthreads();
    // ---- reset: the next batch finds the partition clean ----
    if (s_word[W_FIN] == FIN_OK_RESET) {
        const u32 nd = nd0 + ndrop;
        for (u32 i = tid; i < keep; i += 1024u) clear_entry(&a.table[a.live[i]]);
        for (u32 i = tid; i < nd; i += 1024u) clear_entry(&a.table[a.dead[i]]);
    } else {
        for (u32 i = tid; i < cap; i += 1024u) clear_entry(&a.table[i]);
        if (tid < (u32)N_SHARDS) a.shard_cnt[tid * SHARD_STRIDE] = 0;
    }
    __syncthreads();
    init_ctl_dev(ctl, EMPTY64, 0u, a.size, 0ull, 0u);
    __syncthreads();
    if (tid == 0) ctl->read_first = read_first; // (init_ctl_dev leaves it 0; the batch kernel has no queue reset that would set it)
}

hipError_t launch_batch_epilogue_large(const EpiLargeArgs *args, uint32_t n_files, uint32_t read_first, hipStream_t st) {
    if (n_files == 0) return hipSuccess;
    // (function attributes belong to the current device: once per device, harmless if two worker threads both get here first)
    static std::atomic<bool> done[64];
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !done[dev].load(std::memory_order_acquire)) {
        if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_batch_epilogue_large), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)LG_LDS_BYTES);
            e != hipSuccess)
            return e;
        if (dev >= 0 && dev < 64) done[dev].store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL(k_batch_epilogue_large, dim3(n_files), dim3(1024), LG_LDS_BYTES, st, args, read_first);
    return hipGetLastError();
}

} // namespace fh
