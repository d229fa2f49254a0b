// fh_counts.hip -- the AllCounts sketcher on gfx950 (FH_KIND_ALL_COUNTS; reference: lib/src/sketch_schemes/counts.rs).
//
// A dense histogram of the forward k-mers of the packed stream, 4^k u32 bins (k <= 16), and to_vec as an order-free pass
// over the bins:
//   count   one lane = 32 window starts (48 bytes, fh_counts.h ac_lane_windows); k <= AC_LDS_MAX_K: per-wave copies of the
//           histogram in LDS, flushed once per workgroup with global atomics; larger k: one global atomic per window.
//   fold    bins whose u32 counter wrapped are set to u32::MAX (the saturating add of counts.rs:31)
//   mark    per 4096-bin block: how many bins to_vec emits, and the u64 sum of the saturated counts (num_valid_kmers)
//   scan    one workgroup: exclusive offsets of the blocks
//   compact the emitted rows (ix, c + c[rc] wrapping, c[rc]) in ascending ix
// Counts are integers and order-free: the result is bit-exact whatever the schedule.
//
// Saturation.  A bin's u32 counter wraps like the hardware's add; a bitmap (one bit per bin) remembers that it did.  An add
// of v to a bin whose counter held `old` wrapped iff old + v < old, and the counter then holds the true total mod 2^32 --
// so "wrapped at least once" is exactly "true total >= 2^32", and the fold turns those bins into u32::MAX.  Launches of
// the global form skip the check (a non-returning atomic) while the windows counted since the last fold cannot bring any
// bin to 2^32; the LDS form's per-workgroup counters cannot wrap because the host caps a launch at 2^30 windows.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fh_counts.h"
#include "fh_kernels.h"

namespace fh {

namespace {

constexpr int AC_LDS_THREADS = 512;            // 8 waves
constexpr int AC_GLOBAL_THREADS = 256;
constexpr uint32_t AC_LDS_BYTES = 64u * 1024u; // histogram copies per workgroup: 2 workgroups per CU (160 KiB)
constexpr int AC_BIN_PER_THREAD = 16;
constexpr int AC_FIN_THREADS = 256;
constexpr uint64_t AC_FIN_BINS = (uint64_t)AC_BIN_PER_THREAD * AC_FIN_THREADS; // bins per block of the finishing passes

// copies of the histogram per workgroup: one per wave while they fit in AC_LDS_BYTES (k <= 5), fewer beyond
constexpr int ac_lds_copies(int k) {
    return (int)std::min<uint32_t>(AC_LDS_BYTES / (4u << (2 * k)), (uint32_t)(AC_LDS_THREADS / 64));
}

// 48 bytes from p on; bytes at or behind len read as 0 (a breaker)
__device__ __forceinline__ void ac_load48(const uint8_t *seq, uint64_t len, uint64_t p, bool aligned, u32 *d) {
    if (aligned && p + AC_LANE_BYTES <= len) {
        const uint4 *q = reinterpret_cast<const uint4 *>(seq + p);
        const uint4 a = q[0], b = q[1], c = q[2];
        d[0] = a.x, d[1] = a.y, d[2] = a.z, d[3] = a.w;
        d[4] = b.x, d[5] = b.y, d[6] = b.z, d[7] = b.w;
        d[8] = c.x, d[9] = c.y, d[10] = c.z, d[11] = c.w;
        return;
    }
    for (int w = 0; w < 12; ++w) {
        u32 v = 0;
        for (int i = 0; i < 4; ++i) {
            const uint64_t at = p + 4 * w + i;
            if (at < len) v |= (u32)seq[at] << (8 * i);
        }
        d[w] = v;
    }
}

// v more occurrences of bin ix (global table), the wrap remembered
__device__ __forceinline__ void ac_add_checked(u32 *table, u32 *sat, u32 ix, u32 v) {
    const u32 old = atomicAdd(table + ix, v);
    if (old + v < old) atomicOr(sat + (ix >> 5), 1u << (ix & 31u));
}

template <int K>
__global__ __launch_bounds__(AC_LDS_THREADS) void k_ac_count_lds(AcCountArgs a) {
    constexpr u32 B = 1u << (2 * K);
    constexpr int COPIES = ac_lds_copies(K);
    __shared__ u32 hist[COPIES * B];
    for (u32 i = threadIdx.x; i < COPIES * B; i += AC_LDS_THREADS) hist[i] = 0;
    __syncthreads();
    u32 *mine = hist + (threadIdx.x / 64u) % COPIES * B;
    const bool aligned = (reinterpret_cast<uintptr_t>(a.seq) & 15u) == 0;
    const uint64_t lanes = (uint64_t)gridDim.x * AC_LDS_THREADS;
    for (uint64_t p = a.p_begin + AC_LANE_POS * ((uint64_t)blockIdx.x * AC_LDS_THREADS + threadIdx.x); p < a.p_end; p += AC_LANE_POS * lanes) {
        u32 d[12];
        ac_load48(a.seq, a.len, p, aligned, d);
        const uint64_t left = a.p_end - p;
        ac_lane_windows<K>(d, left < 32 ? (u32)left : 32u, [&](int, u32 ix) { atomicAdd(mine + ix, 1u); });
    }
    __syncthreads();
    for (u32 i = threadIdx.x; i < B; i += AC_LDS_THREADS) {
        u32 v = 0;
        for (int c = 0; c < COPIES; ++c) v += hist[c * B + i];
        if (v) ac_add_checked(a.table, a.sat, i, v);
    }
}

template <int K, bool CHECK>
__global__ __launch_bounds__(AC_GLOBAL_THREADS) void k_ac_count_global(AcCountArgs a) {
    const bool aligned = (reinterpret_cast<uintptr_t>(a.seq) & 15u) == 0;
    const uint64_t lanes = (uint64_t)gridDim.x * AC_GLOBAL_THREADS;
    for (uint64_t p = a.p_begin + AC_LANE_POS * ((uint64_t)blockIdx.x * AC_GLOBAL_THREADS + threadIdx.x); p < a.p_end; p += AC_LANE_POS * lanes) {
        u32 d[12];
        ac_load48(a.seq, a.len, p, aligned, d);
        const uint64_t left = a.p_end - p;
        ac_lane_windows<K>(d, left < 32 ? (u32)left : 32u, [&](int, u32 ix) {
            if (CHECK) ac_add_checked(a.table, a.sat, ix, 1u);
            else atomicAdd(a.table + ix, 1u);
        });
    }
}

__global__ void k_ac_fold(u32 *table, u32 *sat, uint64_t words) {
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (uint64_t)gridDim.x * blockDim.x) {
        u32 bits = sat[w];
        if (!bits) continue;
        sat[w] = 0;
        while (bits) {
            const int b = __builtin_ctz(bits);
            bits &= bits - 1u;
            table[w * 32 + b] = 0xFFFFFFFFu;
        }
    }
}

// the rows to_vec emits from thread t's bins [base, base + 16), and the sum of their forward counts
__device__ __forceinline__ u32 ac_thread_bins(const u32 *table, int k, uint64_t bins, uint64_t base, uint64_t *sum) {
    u32 n = 0;
    uint64_t s = 0;
    for (int i = 0; i < AC_BIN_PER_THREAD; ++i) {
        const uint64_t ix = base + i;
        if (ix >= bins) break;
        const u32 c = table[ix];
        if (!c) continue;
        s += c;
        const u32 rc = ac_revcomp((u32)ix, k);
        n += ac_emit((u32)ix, rc, c, table[rc]) ? 1u : 0u;
    }
    *sum = s;
    return n;
}

// workgroup-wide exclusive scan of one u32 per thread (AC_FIN_THREADS threads); *total = the workgroup's sum
__device__ __forceinline__ u32 ac_block_scan(u32 v, u32 *total) {
    __shared__ u32 sh[AC_FIN_THREADS];
    sh[threadIdx.x] = v;
    __syncthreads();
    for (u32 off = 1; off < AC_FIN_THREADS; off <<= 1) {
        const u32 t = threadIdx.x >= off ? sh[threadIdx.x - off] : 0u;
        __syncthreads();
        sh[threadIdx.x] += t;
        __syncthreads();
    }
    *total = sh[AC_FIN_THREADS - 1];
    const u32 r = sh[threadIdx.x] - v;
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(AC_FIN_THREADS) void k_ac_mark(const u32 *table, int k, uint64_t bins, u32 *blk_cnt, uint64_t *tot) {
    uint64_t s = 0;
    const u32 n = ac_thread_bins(table, k, bins, (uint64_t)blockIdx.x * AC_FIN_BINS + (uint64_t)threadIdx.x * AC_BIN_PER_THREAD, &s);
    u32 total = 0;
    (void)ac_block_scan(n, &total);
    __shared__ uint64_t ssum[AC_FIN_THREADS];
    ssum[threadIdx.x] = s;
    __syncthreads();
    for (u32 off = AC_FIN_THREADS / 2; off; off >>= 1) {
        if (threadIdx.x < off) ssum[threadIdx.x] += ssum[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        blk_cnt[blockIdx.x] = total;
        if (ssum[0]) atomicAdd((unsigned long long *)(tot + 1), (unsigned long long)ssum[0]);
    }
}

// one workgroup: blk_off[i] = the sum of blk_cnt[0, i); tot[0] = the rows of all blocks
__global__ __launch_bounds__(AC_FIN_THREADS) void k_ac_scan(const u32 *blk_cnt, uint64_t nblk, uint64_t *blk_off, uint64_t *tot) {
    const uint64_t per = (nblk + AC_FIN_THREADS - 1) / AC_FIN_THREADS;
    const uint64_t lo = std::min<uint64_t>(threadIdx.x * per, nblk), hi = std::min<uint64_t>(lo + per, nblk);
    uint64_t s = 0;
    for (uint64_t i = lo; i < hi; ++i) s += blk_cnt[i];
    __shared__ uint64_t sh[AC_FIN_THREADS];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (u32 off = 1; off < AC_FIN_THREADS; off <<= 1) {
        const uint64_t t = threadIdx.x >= off ? sh[threadIdx.x - off] : 0ull;
        __syncthreads();
        sh[threadIdx.x] += t;
        __syncthreads();
    }
    uint64_t run = sh[threadIdx.x] - s;
    for (uint64_t i = lo; i < hi; ++i) {
        blk_off[i] = run;
        run += blk_cnt[i];
    }
    if (threadIdx.x == AC_FIN_THREADS - 1) tot[0] = sh[threadIdx.x];
}

__global__ __launch_bounds__(AC_FIN_THREADS) void k_ac_compact(const u32 *table, int k, uint64_t bins, const uint64_t *blk_off,
                                                                uint64_t *o_hash, u32 *o_count, u32 *o_extra) {
    const uint64_t base = (uint64_t)blockIdx.x * AC_FIN_BINS + (uint64_t)threadIdx.x * AC_BIN_PER_THREAD;
    uint64_t s = 0;
    const u32 n = ac_thread_bins(table, k, bins, base, &s);
    u32 total = 0;
    uint64_t o = blk_off[blockIdx.x] + ac_block_scan(n, &total);
    if (!n) return;
    for (int i = 0; i < AC_BIN_PER_THREAD; ++i) {
        const uint64_t ix = base + i;
        if (ix >= bins) break;
        const u32 c = table[ix];
        if (!c) continue;
        const u32 rc = ac_revcomp((u32)ix, k), crc = table[rc];
        if (!ac_emit((u32)ix, rc, c, crc)) continue;
        o_hash[o] = ix;
        o_count[o] = c + crc; // wrapping (counts.rs:52 in a release build)
        o_extra[o] = crc;
        ++o;
    }
}

__global__ void k_ac_add(u32 *dst, const u32 *src, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const u32 a = dst[i], r = a + src[i];
        dst[i] = r < a ? 0xFFFFFFFFu : r;
    }
}

__global__ void k_ac_debug_add(u32 *table, uint64_t n, uint64_t add) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const u32 c = table[i];
        if (!c) continue;
        table[i] = add >= 0xFFFFFFFFull - c ? 0xFFFFFFFFu : (u32)(c + add);
    }
}

// ---- many files per launch (fh_batch_new_counts) ----
// A workgroup takes a contiguous run of the batch's tile space (tiles of TILE_POS window starts, as k2_batch's), file by file:
// its waves deal the file's tiles of the run among themselves, a lane takes the 32 window starts of its group -- in the byte
// form exactly k_ac_count_lds's step, in the two-bit form one u64 of codes and one u32 of base bits plus the group behind
// (the halo; the tile of zeroes behind a file's last tile is the halo of its last lane).  ONE file's histogram is in LDS at a
// time, in k_ac_count_lds's layout; when the run leaves the file its nonzero bins go to the file's table, one atomic each, and
// the LDS copies are cleared.  A window belongs to the lane that owns its start, so it is counted once whatever tile or
// workgroup its last base lies in; bytes and positions at or behind a file's `len` are no bases, so no window spans two files
// and the last K - 1 positions of a file start none.
template <int K>
__global__ __launch_bounds__(AC_LDS_THREADS) void k_ac_batch_count(AcBatchArgs a) {
    constexpr u32 B = 1u << (2 * K);
    constexpr int COPIES = ac_lds_copies(K);
    constexpr u32 WAVES = AC_LDS_THREADS / 64;
    __shared__ u32 hist[COPIES * B];
    for (u32 i = threadIdx.x; i < COPIES * B; i += AC_LDS_THREADS) hist[i] = 0;
    __syncthreads();
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    u32 *mine = hist + wave % COPIES * B;
    const uint64_t t_first = (uint64_t)blockIdx.x * a.tiles_per_group;
    if (t_first >= a.tiles_total) return;
    u32 t = (u32)t_first;
    const u32 t_stop = (u32)std::min<uint64_t>(t_first + a.tiles_per_group, a.tiles_total);
    // the file tile t belongs to: the last one whose first tile is <= t (a file without tiles shares its successor's first tile
    // and is never the last such)
    u32 f = 0;
    {
        u32 lo = 0, hi = a.n_files;
        while (hi - lo > 1u) {
            const u32 mid = (lo + hi) >> 1;
            if (a.files[mid].tile0 <= t) lo = mid;
            else hi = mid;
        }
        f = lo;
    }
    while (t < t_stop) { // (t < tiles_total: some file from f on holds tile t, so f stays below n_files)
        const BatchFile *const fd = a.files + f;
        const u32 f_tile0 = fd->tile0, f_tiles = fd->n_tiles;
        if (f_tiles == 0u || t >= f_tile0 + f_tiles) {
            ++f;
            continue;
        }
        const uint8_t *const seq = fd->seq;
        const uint64_t len = fd->len;
        const u32 run_end = std::min(t_stop, f_tile0 + f_tiles);
        for (u32 tt = t - f_tile0 + wave; tt < run_end - f_tile0; tt += WAVES) {
            const uint64_t p = (uint64_t)tt * TILE_POS + lane * AC_LANE_POS;
            if (p >= len) continue;
            const auto count = [&](int, u32 ix) { atomicAdd(mine + ix, 1u); };
            if (a.two_bit) {
                const uint64_t g = (uint64_t)tt * 64u + lane, g1 = g + 1; // (g1 may be group 0 of the next tile: it exists, fh_pack2.h)
                const uint8_t *const t0 = seq + (g >> 6) * TWO_BIT_TILE_BYTES, *const t1 = seq + (g1 >> 6) * TWO_BIT_TILE_BYTES;
                const uint64_t own = *reinterpret_cast<const uint64_t *>(t0 + 8u * (u32)(g & 63u));
                const u32 g_own = *reinterpret_cast<const u32 *>(t0 + TWO_BIT_CODES_BYTES + 4u * (u32)(g & 63u));
                const uint64_t next = *reinterpret_cast<const uint64_t *>(t1 + 8u * (u32)(g1 & 63u));
                const u32 g_next = *reinterpret_cast<const u32 *>(t1 + TWO_BIT_CODES_BYTES + 4u * (u32)(g1 & 63u));
                ac_group_windows<K>(own, g_own, next, g_next, count);
            } else {
                u32 d[12];
                ac_load48(seq, len, p, true, d); // (a file's stream is 16-byte aligned; bytes behind len read as breakers)
                ac_lane_windows<K>(d, 32u, count);
            }
        }
        __syncthreads();
        u32 *const table = a.tables + (size_t)f * B;
        for (u32 i = threadIdx.x; i < B; i += AC_LDS_THREADS) {
            u32 v = 0;
            for (int c = 0; c < COPIES; ++c) {
                v += hist[c * B + i];
                hist[c * B + i] = 0;
            }
            if (v) atomicAdd(table + i, v); // (no wrap: a file has fewer than 2^32 positions, fh_batch_new_counts)
        }
        __syncthreads();
        t = run_end;
        ++f;
    }
}

// to_vec of one file per workgroup.  The table (at most 16 384 bins) is read into LDS and zeroed behind; bins are looked at in
// rounds of AC_FIN_THREADS consecutive ones (a lane a bin: ascending ix is round by round, wave by wave, lane by lane), so the
// row offset of a bin is (rows of the (round, wave) cells in front of its own) + (emitting lanes below it in its wave).
__global__ __launch_bounds__(AC_FIN_THREADS) void k_ac_batch_epilogue(u32 *tables, int k, u32 *out, u32 out_stride, AcBatchResult *res) {
    constexpr u32 WAVES = AC_FIN_THREADS / 64;
    __shared__ u32 c[1u << (2 * AC_LDS_MAX_K)];
    __shared__ uint64_t ssum[AC_FIN_THREADS];
    const u32 B = 1u << (2 * k), rounds = (B + AC_FIN_THREADS - 1) / AC_FIN_THREADS; // rounds * WAVES <= AC_FIN_THREADS cells
    u32 *const table = tables + (size_t)blockIdx.x * B;
    for (u32 i = threadIdx.x; i < B; i += AC_FIN_THREADS) {
        c[i] = table[i];
        table[i] = 0;
    }
    __syncthreads();
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const auto emits = [&](u32 ix, u32 &cnt, u32 &crc) {
        if (ix >= B) return false;
        cnt = c[ix];
        const u32 rc = ac_revcomp(ix, k);
        crc = c[rc];
        return ac_emit(ix, rc, cnt, crc);
    };
    // pass 1: rows per cell (thread r * WAVES + w keeps cell (r, w)'s), and the sum of the forward counts
    uint64_t s = 0;
    u32 cell_rows = 0;
    for (u32 r = 0; r < rounds; ++r) {
        u32 cnt = 0, crc = 0;
        const bool e = emits(r * AC_FIN_THREADS + threadIdx.x, cnt, crc);
        s += cnt;
        const u32 n = (u32)__popcll(__ballot(e));
        if (lane == 0) ssum[r * WAVES + wave] = n; // (ssum doubles as the hand-over of the cells' rows)
    }
    __syncthreads();
    if (threadIdx.x < rounds * WAVES) cell_rows = (u32)ssum[threadIdx.x];
    __syncthreads();
    u32 n_out = 0;
    const u32 cell_off = ac_block_scan(cell_rows, &n_out);
    ssum[threadIdx.x] = cell_off;
    __syncthreads();
    // pass 2: the rows
    u32 *const o_ix = out + (size_t)blockIdx.x * 3u * out_stride, *const o_count = o_ix + out_stride, *const o_extra = o_count + out_stride;
    for (u32 r = 0; r < rounds; ++r) {
        u32 cnt = 0, crc = 0;
        const u32 ix = r * AC_FIN_THREADS + threadIdx.x;
        const bool e = emits(ix, cnt, crc);
        const uint64_t m = __ballot(e);
        if (e) {
            const u32 o = (u32)ssum[r * WAVES + wave] + (u32)__popcll(m & ((1ull << lane) - 1ull));
            o_ix[o] = ix;
            o_count[o] = cnt + crc; // (cannot wrap: fh_batch_new_counts)
            o_extra[o] = crc;
        }
    }
    __syncthreads();
    ssum[threadIdx.x] = s;
    __syncthreads();
    for (u32 off = AC_FIN_THREADS / 2; off; off >>= 1) {
        if (threadIdx.x < off) ssum[threadIdx.x] += ssum[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) res[blockIdx.x] = AcBatchResult{ssum[0], n_out, 0u};
}

uint32_t grid_cap_of_device() {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
        (void)hipGetLastError();
        cus = 256;
    }
    return (uint32_t)(2 * cus); // two LDS workgroups per CU
}

template <int K>
hipError_t launch_count_k(const AcCountArgs &a, uint32_t grid_cap, hipStream_t st) {
    const uint64_t steps = (a.p_end - a.p_begin + AC_LANE_POS - 1) / AC_LANE_POS;
    if constexpr (K <= AC_LDS_MAX_K) {
        const uint64_t want = std::max<uint64_t>(1, (steps + AC_LDS_THREADS - 1) / AC_LDS_THREADS);
        hipLaunchKernelGGL(k_ac_count_lds<K>, dim3((uint32_t)std::min<uint64_t>(want, grid_cap)),
                           dim3(AC_LDS_THREADS), 0, st, a);
    } else {
        const uint64_t want = std::max<uint64_t>(1, (steps + AC_GLOBAL_THREADS - 1) / AC_GLOBAL_THREADS);
        const dim3 grid((uint32_t)std::min<uint64_t>(want, 8ull * grid_cap));
        if (a.check) hipLaunchKernelGGL((k_ac_count_global<K, true>), grid, dim3(AC_GLOBAL_THREADS), 0, st, a);
        else hipLaunchKernelGGL((k_ac_count_global<K, false>), grid, dim3(AC_GLOBAL_THREADS), 0, st, a);
    }
    return hipGetLastError();
}

} // namespace

uint64_t ac_fin_blocks(int k) { return (ac_bins(k) + AC_FIN_BINS - 1) / AC_FIN_BINS; }

hipError_t launch_ac_count(int k, const AcCountArgs &a, hipStream_t st) {
    if (a.p_end <= a.p_begin) return hipSuccess;
    const uint32_t cap = grid_cap_of_device();
    switch (k) {
#define FH_AC_CASE(K) \
    case K: return launch_count_k<K>(a, cap, st);
        FH_AC_CASE(1) FH_AC_CASE(2) FH_AC_CASE(3) FH_AC_CASE(4) FH_AC_CASE(5) FH_AC_CASE(6) FH_AC_CASE(7) FH_AC_CASE(8)
        FH_AC_CASE(9) FH_AC_CASE(10) FH_AC_CASE(11) FH_AC_CASE(12) FH_AC_CASE(13) FH_AC_CASE(14) FH_AC_CASE(15) FH_AC_CASE(16)
#undef FH_AC_CASE
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_ac_batch_count(int k, const AcBatchArgs &a0, hipStream_t st) {
    if (a0.tiles_total == 0) return hipSuccess;
    AcBatchArgs a = a0;
    // every workgroup a run of at least one tile per wave; no more workgroups than the chip holds at once
    a.tiles_per_group = std::max<uint32_t>(AC_LDS_THREADS / 64, (a.tiles_total + grid_cap_of_device() - 1) / grid_cap_of_device());
    const dim3 grid((a.tiles_total + a.tiles_per_group - 1) / a.tiles_per_group), block(AC_LDS_THREADS);
    switch (k) {
#define FH_AC_CASE(K) \
    case K: hipLaunchKernelGGL(k_ac_batch_count<K>, grid, block, 0, st, a); break;
        FH_AC_CASE(1) FH_AC_CASE(2) FH_AC_CASE(3) FH_AC_CASE(4) FH_AC_CASE(5) FH_AC_CASE(6) FH_AC_CASE(7)
#undef FH_AC_CASE
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_ac_batch_epilogue(uint32_t *tables, int k, uint32_t n_files, uint32_t *out, uint32_t out_stride, AcBatchResult *res,
                                    hipStream_t st) {
    if (k < 1 || k > AC_LDS_MAX_K) return hipErrorInvalidValue;
    if (n_files == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ac_batch_epilogue, dim3(n_files), dim3(AC_FIN_THREADS), 0, st, tables, k, out, out_stride, res);
    return hipGetLastError();
}

hipError_t launch_ac_mark(u32 *table, u32 *sat, int k, u32 *blk_cnt, uint64_t *blk_off, uint64_t *tot, hipStream_t st) {
    const uint64_t bins = ac_bins(k), words = (bins + 31) / 32, nblk = ac_fin_blocks(k);
    hipLaunchKernelGGL(k_ac_fold, dim3((uint32_t)std::min<uint64_t>((words + 255) / 256, 4096)), dim3(256), 0, st, table, sat, words);
    if (hipError_t e = hipMemsetAsync(tot, 0, 2 * sizeof(uint64_t), st)) return e;
    hipLaunchKernelGGL(k_ac_mark, dim3((uint32_t)nblk), dim3(AC_FIN_THREADS), 0, st, table, k, bins, blk_cnt, tot);
    hipLaunchKernelGGL(k_ac_scan, dim3(1), dim3(AC_FIN_THREADS), 0, st, blk_cnt, nblk, blk_off, tot);
    return hipGetLastError();
}

hipError_t launch_ac_compact(const u32 *table, int k, const uint64_t *blk_off, uint64_t *o_hash, u32 *o_count, u32 *o_extra, hipStream_t st) {
    hipLaunchKernelGGL(k_ac_compact, dim3((uint32_t)ac_fin_blocks(k)), dim3(AC_FIN_THREADS), 0, st, table, k, ac_bins(k), blk_off, o_hash,
                       o_count, o_extra);
    return hipGetLastError();
}

hipError_t launch_ac_add(u32 *dst, const u32 *src, uint64_t n, hipStream_t st) {
    hipLaunchKernelGGL(k_ac_add, dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, 8192)), dim3(256), 0, st, dst, src, n);
    return hipGetLastError();
}

hipError_t launch_ac_debug_add(u32 *table, uint64_t n, uint64_t add, hipStream_t st) {
    hipLaunchKernelGGL(k_ac_debug_add, dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, 8192)), dim3(256), 0, st, table, n, add);
    return hipGetLastError();
}

} // namespace fh
