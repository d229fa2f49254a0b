// fh_screen.hip -- THE SCREEN: containment of a library's references in raw reads (finch_index_screen, include/finch_host.h;
// DESIGN.md §3.23), hand-written for gfx950.
//
// A screen does not sketch the sample.  It hashes every k-mer of it and looks each hash up among the library's hashes; per
// reference it reports how many of ITS hashes occur in the sample and how often.  The device side, per call:
//
//   * the table, built from the index's CURRENT postings (sorted by hash, duplicates kept: fh_index.hip): head flags over the
//     keys counted per tile of 2048 (k_screen_heads), the counts scanned by one workgroup (k_screen_scan), the heads written to
//     their places (k_screen_compact) -> dk[nd], the distinct hashes ascending; mult[nd], a zeroed u64 each; dir[2^b + 1],
//     dir[t] = the first distinct hash whose bucket is >= t (k_screen_dir: one bound search per entry).  A hash's bucket is
//     h >> shift with shift = max(0, bits - b), bits = the width of the largest key: the b bits from the highest set bit of the
//     largest key down, not the top bits of the word -- a Scaled library's keys all lie below its max_hash and would share
//     bucket 0 -- and monotone in h, which is what lets dir be a list of bounds;
//   * k_screen<K, SEED0>: persistent waves over the tiles of a staged two-bit piece (fh_pack2.h).  A tile is hashed by the record
//     kernel's unit -- load_tile_two_bit for the tile and its halo, window_valid_mask, Windows, murmur_h1_fast with the murmur3
//     tables in LDS: the tile kernels' arithmetic, not a second statement of it -- eight window starts per lane at a time.  A
//     valid window's hash above the largest key or below the smallest is a miss before any memory access (for a Scaled library
//     that alone rejects all but `scale` of the windows); the others read their bucket's two bounds and search dk between them,
//     and on dk[i] == h add 1 to mult[i] with a 64-bit global atomic.  Valid windows and hits are counted per lane, summed over
//     the wave at its end and added to the call's two counters by one lane;
//   * k_screen_finish: one wave per reference.  Each of its hashes is found in the table (all are there), its multiplicity goes
//     to a scratch array parallel to the library's CSR, shared / sum_mult / the largest multiplicity are reduced over the wave.
//     The lower median of the shared multiplicities is the largest v with |{0 < m < v}| <= (shared - 1) / 2, found bit by bit
//     from the top bit of the largest multiplicity: per bit one pass of wave-wide loads over the reference's scratch.  No sort,
//     no LDS, no bound on a reference's length.
//
// Every window position of a piece belongs to exactly one lane of one tile; what makes pieces tile a sample without a window
// lost or counted twice is the host's packing (fh_host.cpp: ScreenSink).
// Compiled FH_NPARTS times like fh_records.hip (a share of K = 1..32 each); part 0 also holds the table, the finish and the host side.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>

#include "../../include/finch_hip.h"
#include "fh_core.h"
#include "fh_device.h"
#include "fh_kernels.h"
#include "fh_k2_common.h"
#include "fh_internal.h"
#include "fh_pack2.h"
#include "fh_screen.h"

#ifndef FH_PART
#error "compile with -DFH_PART=<0..FH_NPARTS-1>"
#endif

namespace fh {

struct ScreenArgs {
    const uint8_t *region; // the staged piece: n_tiles tiles and the tile of zeroes behind them
    u32 n_tiles, nd;
    u64 seed;
    const u64 *dk;
    const u32 *dir;
    ull *mult;
    u64 kmin, kmax; // dk[0], dk[nd - 1]
    u32 shift, pad;
    ull *counters;  // [0] valid windows, [1] hits
};

constexpr int SCR_WAVES = 4, SCR_THREADS = 64 * SCR_WAVES;
constexpr int SCR_UNIT = 8; // window starts per lane hashed before their lookups are issued
static_assert(fh_pack2::TILE_POS == (uint64_t)TILE_POS && fh_pack2::TILE_BYTES == (uint64_t)TWO_BIT_TILE_BYTES, "fh_pack2.h restates fh_device.h");

// the place of h among the distinct hashes dk[lo0, hi0) of its bucket, or nd: a branch-free bound search (a bucket holds about
// one hash by default; screen_dir_bits makes them long)
__device__ __forceinline__ u32 screen_find(const u64 *dk, const u32 *dir, u32 shift, u32 nd, u64 h) {
    const u32 t = (u32)(h >> shift);
    u32 lo = dir[t];
    u32 n = dir[t + 1u] - lo;
    if (n == 0u) return nd;
    while (n > 1u) {
        const u32 half = n >> 1;
        lo = dk[lo + half] <= h ? lo + half : lo;
        n -= half;
    }
    return dk[lo] == h ? lo : nd;
}

template <int K, bool SEED0>
__global__ __launch_bounds__(SCR_THREADS) void k_screen(const ScreenArgs a) {
    __shared__ Rec4 sA1[has_pair_word(K, false) ? 256 : 1];
    __shared__ Rec4 sA2[has_pair_word(K, true) ? 256 : 1];
    __shared__ Rec2 sB1[has_pair_word(K, false) ? 256 : 1];
    __shared__ Rec2 sB2[has_pair_word(K, true) ? 256 : 1];
    __shared__ Rec2 sP[partial_entries(K)];
    __shared__ __attribute__((aligned(16))) u32 sCodes[SCR_WAVES][256];
    __shared__ __attribute__((aligned(16))) u32 sGood[SCR_WAVES][128];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (has_pair_word(K, false)) {
        for (int q = tid; q < 256; q += SCR_THREADS) {
            sA1[q] = lut_rec_A((u32)q, false);
            sB1[q] = lut_rec_B((u32)q, 4, false);
        }
    }
    if (has_pair_word(K, true)) {
        for (int q = tid; q < 256; q += SCR_THREADS) {
            sA2[q] = lut_rec_A((u32)q, true);
            sB2[q] = lut_rec_B((u32)q, 4, true);
        }
    }
    for (int q = tid; q < partial_entries(K); q += SCR_THREADS) sP[q] = lut_rec_P<K>((u32)q);
    __syncthreads();
    const LutTables LT{sA1, sA2, sB1, sB2, sP, 0u};
    u32 *const codes_ring = sCodes[wave];
    u32 *const good_ring = sGood[wave];
    const uint8_t *const region = a.region;

    u32 nvalid = 0, nhit = 0;
    const u32 n_waves = gridDim.x * (u32)SCR_WAVES;
    for (u32 tile = blockIdx.x * (u32)SCR_WAVES + (u32)wave; tile < a.n_tiles; tile += n_waves) { // (wave-uniform)
        load_tile_two_bit(region, tile, lane, codes_ring, good_ring);
        load_tile_two_bit(region, tile + 1u, lane, codes_ring, good_ring); // (the halo of lane 63; behind the last tile: zeroes)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const u32 par = tile & 1u;
        const uint2 own = *reinterpret_cast<const uint2 *>(&codes_ring[par * 128u + 2u * (u32)lane]);
        const uint2 nbr = *reinterpret_cast<const uint2 *>(&codes_ring[(par * 128u + 2u * (u32)lane + 2u) & 255u]);
        const u32 g_own = good_ring[par * 64u + (u32)lane];
        const u32 g_nbr = good_ring[(par * 64u + (u32)lane + 1u) & 127u];
        const u64 clo = (u64)own.x | ((u64)own.y << 32);
        const u64 chi = (u64)nbr.x | ((u64)nbr.y << 32);
        const u64 g64 = (u64)g_own | ((u64)g_nbr << 32);
        // (positions behind the piece's end are no bases: the host zeroes them, so no window reaches over the end)
        const u32 W = window_valid_mask<K>(g64);
        nvalid += (u32)__popc(W);
        Windows<K> win;
        win.init(clo, chi);
#pragma unroll 1
        for (u32 c = 0; c < (u32)(LANE_POS / SCR_UNIT); ++c) {
            const u32 Wc = (W >> (c * (u32)SCR_UNIT)) & ((1u << SCR_UNIT) - 1u);
            if (__builtin_amdgcn_ballot_w64(Wc != 0u)) { // (wave-uniform: a unit without a valid window is not hashed)
                u64 h[SCR_UNIT];
                bool go[SCR_UNIT];
#pragma unroll
                for (int j = 0; j < SCR_UNIT; ++j) {
                    bool is_rc;
                    const u64 cm = win.canonical(j, is_rc);
                    h[j] = murmur_h1_fast<K, SEED0>(cm, a.seed, LT);
                    go[j] = ((Wc >> j) & 1u) && h[j] >= a.kmin && h[j] <= a.kmax;
                }
#pragma unroll
                for (int j = 0; j < SCR_UNIT; ++j) {
                    if (go[j]) {
                        const u32 i = screen_find(a.dk, a.dir, a.shift, a.nd, h[j]);
                        if (i < a.nd) {
                            atomicAdd(&a.mult[i], 1ull);
                            ++nhit;
                        }
                    }
                }
            }
            win.template advance<SCR_UNIT>();
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier(); // (the next tile overwrites the ring)
    }
    for (int off = 32; off > 0; off >>= 1) {
        nvalid += __shfl_xor(nvalid, off);
        nhit += __shfl_xor(nhit, off);
    }
    if (lane == 0) { // a wave's tiles hold at most 2^30 positions (SCREEN_PIECE_MAX): the sums fit
        if (nvalid) atomicAdd(&a.counters[0], (ull)nvalid);
        if (nhit) atomicAdd(&a.counters[1], (ull)nhit);
    }
}

template <int K>
static hipError_t launch_screen_t(const ScreenArgs &a, uint32_t n_blocks, hipStream_t st) {
    if (a.seed == 0) hipLaunchKernelGGL((k_screen<K, true>), dim3(n_blocks), dim3(SCR_THREADS), 0, st, a);
    else hipLaunchKernelGGL((k_screen<K, false>), dim3(n_blocks), dim3(SCR_THREADS), 0, st, a);
    return hipGetLastError();
}

#ifdef FH_ONLY_K // development builds: one K per translation unit
constexpr int PART_LO = FH_ONLY_K, PART_HI = FH_ONLY_K;
#else
constexpr int PART_LO = FH_PART * (32 / FH_NPARTS) + 1;
constexpr int PART_HI = (FH_PART + 1) * (32 / FH_NPARTS);
#endif

template <int K>
static hipError_t launch_screen_dispatch(int k, const ScreenArgs &a, uint32_t n_blocks, hipStream_t st) {
    if (k == K) return launch_screen_t<K>(a, n_blocks, st);
    if constexpr (K > PART_LO) return launch_screen_dispatch<K - 1>(k, a, n_blocks, st);
    return hipErrorInvalidValue;
}

hipError_t launch_screen_part0(int k, const ScreenArgs &a, uint32_t n_blocks, hipStream_t st);
hipError_t launch_screen_part1(int k, const ScreenArgs &a, uint32_t n_blocks, hipStream_t st);
hipError_t launch_screen_part2(int k, const ScreenArgs &a, uint32_t n_blocks, hipStream_t st);
hipError_t launch_screen_part3(int k, const ScreenArgs &a, uint32_t n_blocks, hipStream_t st);

#define FH_CAT2(a, b) a##b
#define FH_CAT(a, b) FH_CAT2(a, b)
hipError_t FH_CAT(launch_screen_part, FH_PART)(int k, const ScreenArgs &a, uint32_t n_blocks, hipStream_t st) {
    if (k < PART_LO || k > PART_HI) return hipErrorInvalidValue;
    return launch_screen_dispatch<PART_HI>(k, a, n_blocks, st);
}

} // namespace fh

#if FH_PART == 0
// ------------------------------------------------------------------------------------------------------------------------------
// The table, the finish and the host side.
using namespace fh;

namespace {

#define SHIP_TRY(expr)                                                                                    \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess) return api_fail(FH_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

constexpr uint32_t TB_THREADS = 256, TB_ITEMS = 8, TB_TILE = TB_THREADS * TB_ITEMS; // a tile of 2048 postings
constexpr uint32_t SCAN_THREADS = 1024;

// a thread's TB_ITEMS consecutive postings of tile blockIdx.x: how many are heads (the first of a run of equal keys)
__device__ inline uint32_t heads_of(const uint64_t *keys, uint32_t n, uint32_t i0, uint32_t *flags) {
    uint32_t c = 0, f = 0;
    for (uint32_t j = 0; j < TB_ITEMS; ++j) {
        const uint64_t i = (uint64_t)i0 + j;
        if (i < n && (i == 0 || keys[i] != keys[i - 1])) f |= 1u << j, ++c;
    }
    *flags = f;
    return c;
}

__global__ void __launch_bounds__(TB_THREADS) k_screen_heads(const uint64_t *keys, uint32_t n, uint32_t *count) {
    __shared__ uint32_t s_total;
    if (threadIdx.x == 0) s_total = 0;
    __syncthreads();
    uint32_t f;
    const uint64_t i0 = (uint64_t)blockIdx.x * TB_TILE + threadIdx.x * TB_ITEMS;
    uint32_t c = i0 < n ? heads_of(keys, n, (uint32_t)i0, &f) : 0u;
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if ((threadIdx.x & 63u) == 0 && c) atomicAdd(&s_total, c);
    __syncthreads();
    if (threadIdx.x == 0) count[blockIdx.x] = s_total;
}

// count[0 .. n) -> its exclusive prefix sums, *total = the sum; one workgroup, a carry from pass to pass
__global__ void __launch_bounds__(SCAN_THREADS) k_screen_scan(uint32_t *count, uint32_t n, uint32_t *total) {
    __shared__ uint32_t s[SCAN_THREADS];
    __shared__ uint32_t s_carry;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n; base += SCAN_THREADS) { // (uniform)
        const uint32_t i = base + tid;
        const uint32_t v = i < n ? count[i] : 0u;
        s[tid] = v;
        __syncthreads();
        for (uint32_t off = 1; off < SCAN_THREADS; off <<= 1) {
            const uint32_t t = tid >= off ? s[tid - off] : 0u;
            __syncthreads();
            s[tid] += t;
            __syncthreads();
        }
        if (i < n) count[i] = s_carry + s[tid] - v;
        __syncthreads();
        if (tid == SCAN_THREADS - 1) s_carry += s[tid];
        __syncthreads();
    }
    if (tid == 0) *total = s_carry;
}

// the heads of tile blockIdx.x to dk[base[tile] ...], in order; dk has room for every head (nd = the scan's total)
__global__ void __launch_bounds__(TB_THREADS) k_screen_compact(const uint64_t *keys, uint32_t n, const uint32_t *base, uint64_t *dk, uint32_t nd) {
    __shared__ uint32_t s[TB_THREADS];
    const uint32_t tid = threadIdx.x;
    uint32_t f = 0;
    const uint64_t i0 = (uint64_t)blockIdx.x * TB_TILE + tid * TB_ITEMS;
    const uint32_t c = i0 < n ? heads_of(keys, n, (uint32_t)i0, &f) : 0u;
    s[tid] = c;
    __syncthreads();
    for (uint32_t off = 1; off < TB_THREADS; off <<= 1) {
        const uint32_t t = tid >= off ? s[tid - off] : 0u;
        __syncthreads();
        s[tid] += t;
        __syncthreads();
    }
    uint32_t at = base[blockIdx.x] + s[tid] - c;
    for (uint32_t j = 0; j < TB_ITEMS; ++j)
        if ((f >> j) & 1u) {
            if (at < nd) dk[at] = keys[i0 + j];
            ++at;
        }
}

// dir[t] = the first distinct key whose bucket (key >> shift) is >= t, t = 0 .. n_buckets; dir[n_buckets] = nd
__global__ void __launch_bounds__(TB_THREADS) k_screen_dir(const uint64_t *dk, uint32_t nd, uint32_t shift, uint32_t n_buckets, uint32_t *dir) {
    for (uint64_t t = (uint64_t)blockIdx.x * TB_THREADS + threadIdx.x; t <= n_buckets; t += (uint64_t)gridDim.x * TB_THREADS) {
        uint32_t lo = 0, hi = nd;
        if (t == n_buckets) lo = nd;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if ((dk[mid] >> shift) < t) lo = mid + 1;
            else hi = mid;
        }
        dir[t] = lo;
    }
}

struct FinishArgs {
    const uint64_t *rh, *roff;
    uint32_t nr, nd;
    const uint64_t *dk;
    const uint32_t *dir;
    const ull *mult;
    uint32_t shift, pad;
    uint64_t kmax; // dk[nd - 1]: no bucket behind it
    ull *scratch;  // parallel to rh
    uint32_t *o_shared;
    ull *o_sum, *o_median;
};

__device__ inline ull wave_sum(ull v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ void __launch_bounds__(TB_THREADS) k_screen_finish(const FinishArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6, waves = TB_THREADS / 64;
    for (uint64_t r = (uint64_t)blockIdx.x * waves + wave; r < a.nr; r += (uint64_t)gridDim.x * waves) { // (wave-uniform)
        const uint64_t r0 = a.roff[r], r1 = a.roff[r + 1];
        ull shared = 0, sum = 0, mx = 0;
        for (uint64_t t = r0 + lane; t < r1; t += 64) {
            const uint64_t h = a.rh[t]; // (every hash of the library is in the table)
            const uint32_t i = h <= a.kmax ? screen_find(a.dk, a.dir, a.shift, a.nd, h) : a.nd;
            const ull m = i < a.nd ? a.mult[i] : 0ull;
            a.scratch[t] = m; // read back below by this lane alone
            shared += m > 0;
            sum += m;
            mx = m > mx ? m : mx;
        }
        shared = wave_sum(shared);
        sum = wave_sum(sum);
        for (int off = 32; off > 0; off >>= 1) {
            const ull o = __shfl_xor(mx, off);
            mx = o > mx ? o : mx;
        }
        // the lower median m[(shared - 1) / 2] of the shared multiplicities, ascending: the largest v with |{0 < m < v}| <= q
        ull v = 0;
        if (shared) {
            const ull q = (shared - 1) / 2;
            for (int bit = 63 - __clzll((long long)mx); bit >= 0; --bit) {
                const ull cand = v | (1ull << bit);
                ull below = 0;
                for (uint64_t t = r0 + lane; t < r1; t += 64) {
                    const ull m = a.scratch[t];
                    below += m > 0 && m < cand;
                }
                if (wave_sum(below) <= q) v = cand;
            }
        }
        if (lane == 0) {
            a.o_shared[r] = (uint32_t)shared;
            a.o_sum[r] = sum;
            a.o_median[r] = v;
        }
    }
}

hipError_t launch_screen(int k, const ScreenArgs &a, uint32_t n_blocks, hipStream_t st) {
    constexpr int per = 32 / FH_NPARTS;
    switch ((k - 1) / per) {
    case 0: return launch_screen_part0(k, a, n_blocks, st);
    case 1: return launch_screen_part1(k, a, n_blocks, st);
    case 2: return launch_screen_part2(k, a, n_blocks, st);
    case 3: return launch_screen_part3(k, a, n_blocks, st);
    }
    return hipErrorInvalidValue;
}

} // namespace

namespace fh {

struct ScreenDevice {
    ScreenView v;
    uint32_t k = 0;
    uint64_t seed = 0, piece = 0;
    int prev_device = -1;
    uint32_t n_cus = 1;
    hipStream_t stream = nullptr;
    // the table
    uint64_t *dk = nullptr;
    ull *mult = nullptr, *counters = nullptr;
    uint32_t *dir = nullptr;
    uint32_t nd = 0, shift = 0;
    uint64_t kmin = 0, kmax = 0;
    // the slots
    uint8_t *h_stage[2] = {}, *d_stage[2] = {};
    hipEvent_t copied[2] = {}, k0[2] = {}, k1[2] = {}, t0 = nullptr, t1 = nullptr;
    bool timed[2] = {false, false}; // k0 / k1 of the slot hold a launch whose time is not yet in st
    ScreenStats st;
};

void screen_close(ScreenDevice *d) {
    if (!d) return;
    if (hipSetDevice(d->v.device) == hipSuccess) {
        if (d->stream) (void)hipStreamSynchronize(d->stream);
        for (void *p : {(void *)d->dk, (void *)d->mult, (void *)d->counters, (void *)d->dir, (void *)d->d_stage[0], (void *)d->d_stage[1]})
            if (p) (void)hipFree(p);
        for (uint8_t *p : d->h_stage)
            if (p) (void)hipHostFree(p);
        for (hipEvent_t e : {d->copied[0], d->copied[1], d->k0[0], d->k0[1], d->k1[0], d->k1[1], d->t0, d->t1})
            if (e) (void)hipEventDestroy(e);
    }
    if (d->prev_device >= 0) (void)hipSetDevice(d->prev_device);
    (void)hipGetLastError();
    delete d;
}

static int open_into(ScreenDevice *d, int dir_bits) {
    int prev = -1;
    if (hipGetDevice(&prev) == hipSuccess) d->prev_device = prev;
    (void)hipGetLastError();
    SHIP_TRY(hipSetDevice(d->v.device));
    int cus = 0;
    SHIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, d->v.device));
    d->n_cus = (uint32_t)std::max(1, cus);
    d->stream = (hipStream_t)d->v.stream;
    for (hipEvent_t *e : {&d->copied[0], &d->copied[1]}) SHIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    for (hipEvent_t *e : {&d->k0[0], &d->k0[1], &d->k1[0], &d->k1[1], &d->t0, &d->t1}) SHIP_TRY(hipEventCreate(e));

    // --- the distinct keys ---
    const uint32_t n = d->v.n_post;
    const uint32_t n_tiles = (uint32_t)(((uint64_t)n + TB_TILE - 1) / TB_TILE);
    struct Scratch {
        uint32_t *count = nullptr, *total = nullptr;
        ~Scratch() {
            if (count) (void)hipFree(count);
            if (total) (void)hipFree(total);
        }
    } sc;
    SHIP_TRY(api_dev_malloc((void **)&sc.count, (size_t)n_tiles * sizeof(uint32_t)));
    SHIP_TRY(api_dev_malloc((void **)&sc.total, sizeof(uint32_t)));
    SHIP_TRY(hipEventRecord(d->t0, d->stream));
    hipLaunchKernelGGL(k_screen_heads, dim3(n_tiles), dim3(TB_THREADS), 0, d->stream, d->v.keys, n, sc.count);
    SHIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_screen_scan, dim3(1), dim3(SCAN_THREADS), 0, d->stream, sc.count, n_tiles, sc.total);
    SHIP_TRY(hipGetLastError());
    uint32_t nd = 0;
    SHIP_TRY(hipMemcpyAsync(&nd, sc.total, sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
    SHIP_TRY(hipMemcpyAsync(&d->kmin, d->v.keys, sizeof(uint64_t), hipMemcpyDeviceToHost, d->stream));
    SHIP_TRY(hipMemcpyAsync(&d->kmax, d->v.keys + (n - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, d->stream));
    SHIP_TRY(hipStreamSynchronize(d->stream));
    if (nd == 0 || nd > n) return api_fail(FH_ERR_STATE, "screen: %u distinct hashes among %u postings", nd, n);
    d->nd = nd;
    SHIP_TRY(api_dev_malloc((void **)&d->dk, (size_t)nd * sizeof(uint64_t)));
    SHIP_TRY(api_dev_malloc((void **)&d->mult, (size_t)nd * sizeof(ull)));
    SHIP_TRY(api_dev_malloc((void **)&d->counters, 2 * sizeof(ull)));
    hipLaunchKernelGGL(k_screen_compact, dim3(n_tiles), dim3(TB_THREADS), 0, d->stream, d->v.keys, n, (const uint32_t *)sc.count, d->dk, nd);
    SHIP_TRY(hipGetLastError());
    SHIP_TRY(hipMemsetAsync(d->mult, 0, (size_t)nd * sizeof(ull), d->stream));
    SHIP_TRY(hipMemsetAsync(d->counters, 0, 2 * sizeof(ull), d->stream));

    // --- the directory ---
    // (b >= 1: with b = 0 a largest key of 64 bits would make the shift 64, which is no shift at all on the device)
    uint32_t b = 1;
    if (dir_bits >= 0) b = std::min<uint32_t>(std::max<uint32_t>((uint32_t)dir_bits, 1u), SCREEN_DIR_BITS_MAX);
    else
        while (b < SCREEN_DIR_BITS_MAX && (1ull << b) < nd) ++b;
    const uint32_t bits = d->kmax ? 64u - (uint32_t)__builtin_clzll(d->kmax) : 1u; // the width of the largest key
    d->shift = bits > b ? bits - b : 0u; // <= 63
    const uint32_t n_buckets = 1u << b; // (a key's bucket = key >> shift < 2^(bits - shift) <= 2^b)
    SHIP_TRY(api_dev_malloc((void **)&d->dir, ((size_t)n_buckets + 1) * sizeof(uint32_t)));
    hipLaunchKernelGGL(k_screen_dir, dim3(std::min<uint32_t>((n_buckets + TB_THREADS) / TB_THREADS, 1u << 16)), dim3(TB_THREADS), 0, d->stream,
                       (const uint64_t *)d->dk, nd, d->shift, n_buckets, d->dir);
    SHIP_TRY(hipGetLastError());
    SHIP_TRY(hipEventRecord(d->t1, d->stream));

    // --- the slots ---
    const size_t slot_bytes = (size_t)fh_pack2::region_bytes(d->piece);
    for (int s = 0; s < 2; ++s) {
        SHIP_TRY(api_host_malloc((void **)&d->h_stage[s], slot_bytes));
        SHIP_TRY(api_dev_malloc((void **)&d->d_stage[s], slot_bytes));
    }
    SHIP_TRY(hipStreamSynchronize(d->stream));
    float ms = 0.f;
    SHIP_TRY(hipEventElapsedTime(&ms, d->t0, d->t1));
    d->st.table_ms = ms;
    d->st.distinct = nd;
    d->st.table_bytes = (uint64_t)nd * (sizeof(uint64_t) + sizeof(ull)) + ((uint64_t)n_buckets + 1) * sizeof(uint32_t);
    return FH_OK;
}

int screen_open(const ScreenView &v, uint32_t k, uint64_t seed, int dir_bits, uint64_t piece, ScreenDevice **out) {
    if (k < 1 || k > 32 || v.n_post == 0 || v.nr == 0 || piece < SCREEN_PIECE_MIN || piece > SCREEN_PIECE_MAX || piece % fh_pack2::TILE_POS)
        return api_fail(FH_ERR_INVALID, "screen_open: k = %u, %u postings, %u references, pieces of %llu positions", k, v.n_post, v.nr,
                        (unsigned long long)piece);
    ScreenDevice *d = new (std::nothrow) ScreenDevice;
    if (!d) return api_fail(FH_ERR_CAPACITY, "out of host memory");
    d->v = v;
    d->k = k;
    d->seed = seed;
    d->piece = piece;
    if (int rc = open_into(d, dir_bits)) {
        screen_close(d);
        return rc;
    }
    *out = d;
    return FH_OK;
}

uint8_t *screen_slot(ScreenDevice *d, int slot) { return d->h_stage[slot & 1]; }

// the time of the slot's last launch into the figures, once (waits for that launch)
static int settle(ScreenDevice *d, int s) {
    if (!d->timed[s]) return FH_OK;
    SHIP_TRY(hipEventSynchronize(d->k1[s]));
    float ms = 0.f;
    SHIP_TRY(hipEventElapsedTime(&ms, d->k0[s], d->k1[s]));
    d->st.kernel_ms += ms;
    d->timed[s] = false;
    return FH_OK;
}

int screen_launch(ScreenDevice *d, int slot, uint64_t positions) {
    const int s = slot & 1;
    if (positions == 0) return FH_OK;
    if (positions > d->piece) return api_fail(FH_ERR_INVALID, "screen_launch: %llu positions in a piece of %llu", (unsigned long long)positions, (unsigned long long)d->piece);
    SHIP_TRY(hipSetDevice(d->v.device));
    if (int rc = settle(d, s)) return rc; // (the slot's events are reused; its earlier kernel has long read the device twin)
    const uint64_t n_tiles = (positions + fh_pack2::TILE_POS - 1) / fh_pack2::TILE_POS;
    SHIP_TRY(hipMemcpyAsync(d->d_stage[s], d->h_stage[s], (size_t)fh_pack2::region_bytes(positions), hipMemcpyHostToDevice, d->stream));
    SHIP_TRY(hipEventRecord(d->copied[s], d->stream));
    ScreenArgs a{};
    a.region = d->d_stage[s];
    a.n_tiles = (u32)n_tiles; // (<= 2^30 / 2048)
    a.nd = d->nd;
    a.seed = d->seed;
    a.dk = d->dk;
    a.dir = d->dir;
    a.mult = d->mult;
    a.kmin = d->kmin;
    a.kmax = d->kmax;
    a.shift = d->shift;
    a.counters = d->counters;
    // persistent waves: six workgroups of four waves a CU (their LDS: the murmur3 tables and a ring per wave), fewer for a short piece
    const uint32_t n_blocks = (uint32_t)std::min<uint64_t>((n_tiles + SCR_WAVES - 1) / SCR_WAVES, (uint64_t)d->n_cus * 6);
    SHIP_TRY(hipEventRecord(d->k0[s], d->stream));
    SHIP_TRY(launch_screen((int)d->k, a, n_blocks, d->stream));
    SHIP_TRY(hipEventRecord(d->k1[s], d->stream));
    d->timed[s] = true;
    d->st.launches++;
    SHIP_TRY(hipEventSynchronize(d->copied[s])); // the pinned slot may be filled again; the kernel runs on
    return FH_OK;
}

int screen_finish(ScreenDevice *d, uint32_t *shared, uint64_t *sum_mult, uint64_t *median_mult, ScreenStats *st) {
    SHIP_TRY(hipSetDevice(d->v.device));
    for (int s = 0; s < 2; ++s)
        if (int rc = settle(d, s)) return rc;
    const uint32_t nr = d->v.nr;
    struct Out {
        ull *scratch = nullptr, *sum = nullptr, *median = nullptr;
        uint32_t *shared = nullptr;
        ~Out() {
            for (void *p : {(void *)scratch, (void *)sum, (void *)median, (void *)shared})
                if (p) (void)hipFree(p);
        }
    } o;
    SHIP_TRY(api_dev_malloc((void **)&o.scratch, (size_t)d->v.n_post * sizeof(ull)));
    SHIP_TRY(api_dev_malloc((void **)&o.sum, (size_t)nr * sizeof(ull)));
    SHIP_TRY(api_dev_malloc((void **)&o.median, (size_t)nr * sizeof(ull)));
    SHIP_TRY(api_dev_malloc((void **)&o.shared, (size_t)nr * sizeof(uint32_t)));
    FinishArgs f{};
    f.rh = d->v.rh, f.roff = d->v.roff;
    f.nr = nr, f.nd = d->nd;
    f.dk = d->dk, f.dir = d->dir, f.mult = d->mult;
    f.shift = d->shift;
    f.kmax = d->kmax;
    f.scratch = o.scratch;
    f.o_shared = o.shared, f.o_sum = o.sum, f.o_median = o.median;
    SHIP_TRY(hipEventRecord(d->t0, d->stream));
    hipLaunchKernelGGL(k_screen_finish, dim3(std::min<uint32_t>((nr + 3) / 4, 1u << 18)), dim3(TB_THREADS), 0, d->stream, f);
    SHIP_TRY(hipGetLastError());
    SHIP_TRY(hipEventRecord(d->t1, d->stream));
    ull counters[2] = {0, 0};
    SHIP_TRY(hipMemcpyAsync(shared, o.shared, (size_t)nr * sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
    SHIP_TRY(hipMemcpyAsync(sum_mult, o.sum, (size_t)nr * sizeof(ull), hipMemcpyDeviceToHost, d->stream));
    SHIP_TRY(hipMemcpyAsync(median_mult, o.median, (size_t)nr * sizeof(ull), hipMemcpyDeviceToHost, d->stream));
    SHIP_TRY(hipMemcpyAsync(counters, d->counters, sizeof(counters), hipMemcpyDeviceToHost, d->stream));
    SHIP_TRY(hipStreamSynchronize(d->stream));
    float ms = 0.f;
    SHIP_TRY(hipEventElapsedTime(&ms, d->t0, d->t1));
    d->st.kernel_ms += ms;
    d->st.kmers = counters[0];
    d->st.hits = counters[1];
    *st = d->st;
    return FH_OK;
}

} // namespace fh
#endif // FH_PART == 0
