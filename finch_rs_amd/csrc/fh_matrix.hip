// fh_matrix.hip -- minmer_matrix (lib/src/distance.rs:345-364) on the device: one reference sketch of R hashes against many
// sketches, an S x R matrix of i32 whose cell (i, p) is the count sketch i holds for the reference's p-th hash, 0 where it
// does not have it.  DESIGN.md §3.9.
//
// For strictly ascending inputs the reference's two-cursor loop is an order-free predicate per cell, so:
//   * a workgroup takes one sketch (a row) and a block of COLS reference columns; a slice of the sketch's (hash, count)
//     entries sits in LDS;
//   * every lane looks up its CPL reference hashes (columns lane, lane + 256, ...) in the slice with fh_dist.hip's branchless
//     binary search and keeps the cell values in registers;
//   * a sketch longer than a slice is walked slice by slice: the slices hold disjoint value ranges, at most one matches a column;
//   * after the last slice every cell of the block is stored once, a plain dword per lane, consecutive lanes on consecutive
//     columns of the row.  No memset, no scatter, no atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>

#include "../../include/finch_hip.h"
#include "fh_internal.h"
#include "fh_matrix.h"

using namespace fh;

namespace {

#define MHIP_TRY(expr)                                                                                      \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess) return api_fail(FH_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

constexpr uint32_t THREADS = 256;        // four waves
constexpr uint32_t CPL = 4;              // columns per lane
constexpr uint32_t COLS = THREADS * CPL; // columns per workgroup

struct MatrixArgs {
    const uint64_t *ref;  // n_ref
    const uint64_t *soff; // rows + 1
    const uint64_t *sh;
    const uint32_t *sc;
    uint32_t n_ref, slice;
    int32_t *out; // rows x n_ref
};

// #{s[0..n) <= x} over ascending s, n >= 1; top = the largest power of two <= n.  fh_dist.hip's count_below<true>: the same
// number of steps in every lane (the workgroup's n is uniform), no branch; the index is clamped so that no read leaves s[0..n).
__device__ inline uint32_t count_le(const uint64_t *s, uint32_t n, uint32_t top, uint64_t x) {
    uint32_t pos = 0;
    for (uint32_t step = top; step; step >>= 1) {
        const uint32_t p = pos + step;
        const uint64_t v = s[min(p, n) - 1];
        pos = (p <= n && v <= x) ? p : pos;
    }
    return pos;
}

// grid: x = block of COLS columns, y = row; dynamic LDS: a.slice u64 hashes, then a.slice u32 counts
__global__ void __launch_bounds__(THREADS) k_minmer_matrix(MatrixArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t s_h[];
    uint32_t *s_c = (uint32_t *)(s_h + a.slice);
    const uint32_t row = blockIdx.y, c0 = blockIdx.x * COLS + threadIdx.x;
    const uint64_t lo = a.soff[row];
    const uint32_t n = (uint32_t)(a.soff[row + 1] - lo);
    const uint64_t *H = a.sh + lo;
    const uint32_t *C = a.sc + lo;
    uint64_t x[CPL];
    uint32_t val[CPL];
#pragma unroll
    for (uint32_t j = 0; j < CPL; ++j) {
        const uint32_t p = c0 + j * THREADS;
        x[j] = p < a.n_ref ? a.ref[p] : 0; // (a lane past the last column searches like the others and stores nothing)
        val[j] = 0;
    }
    for (uint32_t s0 = 0; s0 < n; s0 += a.slice) {
        const uint32_t ns = min(a.slice, n - s0); // >= 1
        const uint32_t top = 1u << (31 - __clz(ns));
        __syncthreads(); // the previous slice is no longer read
        for (uint32_t i = threadIdx.x; i < ns; i += THREADS) {
            s_h[i] = H[s0 + i];
            s_c[i] = C[s0 + i];
        }
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < CPL; ++j) {
            const uint32_t pos = count_le(s_h, ns, top, x[j]);
            const uint32_t at = pos ? pos - 1 : 0;
            val[j] = (pos && s_h[at] == x[j]) ? s_c[at] : val[j];
        }
    }
    int32_t *o = a.out + (uint64_t)row * a.n_ref;
#pragma unroll
    for (uint32_t j = 0; j < CPL; ++j) {
        const uint32_t p = c0 + j * THREADS;
        if (p < a.n_ref) o[p] = (int32_t)val[j];
    }
}

} // namespace

namespace fh {

struct MatrixDevice {
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t n_ref = 0, max_rows = 0, lds_slice = 0;
    uint64_t max_entries = 0;
    size_t in_bytes = 0;
    uint64_t *ref_d = nullptr;
    struct Buf {
        uint8_t *in_d = nullptr, *in_h = nullptr; // a chunk's input block: offsets | hashes | counts, packed for its rows and entries
        size_t hash_at = 0, count_at = 0;
        uint32_t rows = 0;
        int32_t *out_d = nullptr, *out_h = nullptr;
        hipEvent_t ev0 = nullptr, ev1 = nullptr, done = nullptr;
    } b[2];
};

void matrix_close(MatrixDevice *d) {
    if (!d) return;
    if (hipSetDevice(d->device) == hipSuccess) {
        if (d->stream) (void)hipStreamSynchronize(d->stream);
        if (d->ref_d) (void)hipFree(d->ref_d);
        for (MatrixDevice::Buf &b : d->b) {
            if (b.in_d) (void)hipFree(b.in_d);
            if (b.in_h) (void)hipHostFree(b.in_h);
            if (b.out_d) (void)hipFree(b.out_d);
            if (b.out_h) (void)hipHostFree(b.out_h);
            if (b.ev0) (void)hipEventDestroy(b.ev0);
            if (b.ev1) (void)hipEventDestroy(b.ev1);
            if (b.done) (void)hipEventDestroy(b.done);
        }
        if (d->stream) (void)hipStreamDestroy(d->stream);
    }
    (void)hipGetLastError();
    delete d;
}

static int open_into(MatrixDevice *d, const uint64_t *ref) {
    MHIP_TRY(hipSetDevice(d->device));
    MHIP_TRY(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
    MHIP_TRY(api_dev_malloc((void **)&d->ref_d, (size_t)d->n_ref * sizeof(uint64_t)));
    MHIP_TRY(hipMemcpy(d->ref_d, ref, (size_t)d->n_ref * sizeof(uint64_t), hipMemcpyHostToDevice));
    const size_t out_bytes = (size_t)d->max_rows * d->n_ref * sizeof(int32_t);
    for (MatrixDevice::Buf &b : d->b) {
        MHIP_TRY(api_dev_malloc((void **)&b.in_d, d->in_bytes));
        MHIP_TRY(api_host_malloc((void **)&b.in_h, d->in_bytes));
        MHIP_TRY(api_dev_malloc((void **)&b.out_d, out_bytes));
        MHIP_TRY(api_host_malloc((void **)&b.out_h, out_bytes));
        MHIP_TRY(hipEventCreate(&b.ev0));
        MHIP_TRY(hipEventCreate(&b.ev1));
        MHIP_TRY(hipEventCreateWithFlags(&b.done, hipEventDisableTiming));
    }
    return FH_OK;
}

int matrix_open(int device, const uint64_t *ref, uint32_t n_ref, uint32_t max_rows, uint64_t max_entries, uint32_t longest,
                uint32_t slice, MatrixDevice **out) {
    if (!ref || !n_ref || !max_rows || max_rows > MATRIX_MAX_ROWS || !out)
        return api_fail(FH_ERR_INVALID, "matrix_open: %u reference hashes, %u rows per launch", n_ref, max_rows);
    MatrixDevice *d = new (std::nothrow) MatrixDevice;
    if (!d) return api_fail(FH_ERR_CAPACITY, "out of host memory");
    d->device = device;
    d->n_ref = n_ref;
    d->max_rows = max_rows;
    d->max_entries = max_entries;
    // LDS the launches ask for: no more than the longest sketch needs
    d->lds_slice = std::max(1u, std::min({std::max(slice, 1u), MATRIX_MAX_SLICE, longest}));
    d->in_bytes = ((size_t)max_rows + 1) * sizeof(uint64_t) + (size_t)max_entries * (sizeof(uint64_t) + sizeof(uint32_t)) + 8;
    if (int rc = open_into(d, ref)) {
        matrix_close(d);
        return rc;
    }
    *out = d;
    return FH_OK;
}

int matrix_stage(MatrixDevice *d, int buf, uint32_t rows, uint64_t entries, uint64_t **offsets, uint64_t **hashes, uint32_t **counts) {
    if (!rows || rows > d->max_rows || entries > d->max_entries)
        return api_fail(FH_ERR_INVALID, "matrix_stage: %u rows of %llu entries do not fit the chunk buffer", rows, (unsigned long long)entries);
    MatrixDevice::Buf &b = d->b[buf];
    b.rows = rows;
    b.hash_at = ((size_t)rows + 1) * sizeof(uint64_t);
    b.count_at = b.hash_at + (size_t)entries * sizeof(uint64_t);
    *offsets = (uint64_t *)b.in_h;
    *hashes = (uint64_t *)(b.in_h + b.hash_at);
    *counts = (uint32_t *)(b.in_h + b.count_at);
    return FH_OK;
}

int matrix_launch(MatrixDevice *d, int buf) {
    MatrixDevice::Buf &b = d->b[buf];
    const uint32_t rows = b.rows;
    const uint64_t *off = (const uint64_t *)b.in_h;
    // everything the kernel indexes with: the rows' entries inside what was staged, no row longer than 2^32 - 1
    if (!rows || off[0] != 0 || off[rows] != (b.count_at - b.hash_at) / sizeof(uint64_t))
        return api_fail(FH_ERR_INVALID, "matrix_launch: the offsets do not cover the staged entries");
    for (uint32_t r = 0; r < rows; ++r)
        if (off[r + 1] < off[r] || off[r + 1] - off[r] > UINT32_MAX) return api_fail(FH_ERR_INVALID, "matrix_launch: offsets of row %u", r);
    MHIP_TRY(hipSetDevice(d->device));
    const size_t used = b.count_at + (size_t)off[rows] * sizeof(uint32_t);
    MHIP_TRY(hipMemcpyAsync(b.in_d, b.in_h, used, hipMemcpyHostToDevice, d->stream));
    MatrixArgs a;
    a.ref = d->ref_d;
    a.soff = (const uint64_t *)b.in_d;
    a.sh = (const uint64_t *)(b.in_d + b.hash_at);
    a.sc = (const uint32_t *)(b.in_d + b.count_at);
    a.n_ref = d->n_ref;
    a.slice = d->lds_slice;
    a.out = b.out_d;
    MHIP_TRY(hipEventRecord(b.ev0, d->stream));
    const dim3 grid((d->n_ref + COLS - 1) / COLS, rows);
    hipLaunchKernelGGL(k_minmer_matrix, grid, dim3(THREADS), d->lds_slice * (sizeof(uint64_t) + sizeof(uint32_t)), d->stream, a);
    MHIP_TRY(hipGetLastError());
    MHIP_TRY(hipEventRecord(b.ev1, d->stream));
    MHIP_TRY(hipMemcpyAsync(b.out_h, b.out_d, (size_t)rows * d->n_ref * sizeof(int32_t), hipMemcpyDeviceToHost, d->stream));
    MHIP_TRY(hipEventRecord(b.done, d->stream));
    return FH_OK;
}

int matrix_wait(MatrixDevice *d, int buf, const int32_t **out, double *kernel_ms) {
    MatrixDevice::Buf &b = d->b[buf];
    MHIP_TRY(hipSetDevice(d->device));
    MHIP_TRY(hipEventSynchronize(b.done));
    float ms = 0.f;
    MHIP_TRY(hipEventElapsedTime(&ms, b.ev0, b.ev1));
    *out = b.out_h;
    if (kernel_ms) *kernel_ms = ms;
    return FH_OK;
}

int matrix_current_device() {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return dev;
}

void matrix_restore_device(int device) {
    if (device >= 0 && hipSetDevice(device) != hipSuccess) (void)hipGetLastError();
}

} // namespace fh
