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
