// fh_epilogue_dev.h -- device functions the epilogue kernels of fh_kernels.hip and fh_batch_large.hip share: an entry and a
// control block put back to "never used", and the all-LDS bitonic network.  All are inlined into their callers.
#pragma once
#include <hip/hip_runtime.h>

#include "fh_core.h"
#include "fh_device.h"

namespace fh {

__device__ __forceinline__ void clear_entry(Entry *e) {
    e->hash = EMPTY64;
    e->kmer = EMPTY64;
    e->pos = EMPTY64;
    e->count = 0;
    e->extra = 0;
}

__device__ __forceinline__ void init_ctl_dev(Ctl *ctl, u64 tau0, u32 keep_text_bases, u64 sel_size, u64 tau_floor, u32 hist_on) {
    if (threadIdx.x == 0) {
        ctl->tau = tau0;
        ctl->inserted_total = 0;
        ctl->n_live = 0;
        ctl->overflow = 0;
        ctl->n_coll = 0;
        ctl->need_big = 0;
        ctl->sorted = 1;
        ctl->spec_ok = 0;
        ctl->n_dead = 0;
        ctl->hist_on = hist_on;
        ctl->sel_size = sel_size;
        ctl->tau_floor = tau_floor;
        ctl->next_unit = 0;
        ctl->left_in_pos = 0;
        ctl->n_left_out = 0;
        ctl->stopped = 0;
        ctl->soft_limit = 0xFFFFFFFFu;
        ctl->shard_soft = 0xFFFFFFFFu;
        ctl->read_first = 0;
        ctl->dbg_flush_cycles = ctl->dbg_flush_calls = ctl->dbg_flush_entries = ctl->dbg_wave_cycles = 0;
        ctl->sp_count = 0;
        ctl->sp_extra = 0;
        ctl->sp_pos = EMPTY64;
        ctl->sp_kmer = EMPTY64;
        if (!keep_text_bases) ctl->text_bases = 0;
    }
    for (int i = threadIdx.x; i < 256; i += blockDim.x) {
        ctl->kmer_counts[i] = 0;
        ctl->hist[i] = 0;
    }
}

// The all-LDS bitonic network over N (a power of two, <= SMALL_SORT_MAX) (key, slot) pairs, ascending; the caller has padded
// [n, N) with EMPTY64 keys and put a barrier behind its writes.  Ends on a barrier.
__device__ __forceinline__ void bitonic_lds(u64 *skeys, u32 *sslots, u32 N) {
    const u32 tid = threadIdx.x, nthr = blockDim.x;
    for (u32 kk = 2; kk <= N; kk <<= 1) {
        for (u32 jj = kk >> 1; jj > 0; jj >>= 1) {
            for (u32 i = tid; i < N; i += nthr) {
                const u32 ixj = i ^ jj;
                if (ixj > i) {
                    const bool up = (i & kk) == 0;
                    const u64 a = skeys[i], b = skeys[ixj];
                    if ((a > b) == up) {
                        skeys[i] = b;
                        skeys[ixj] = a;
                        const u32 sa = sslots[i];
                        sslots[i] = sslots[ixj];
                        sslots[ixj] = sa;
                    }
                }
            }
            __syncthreads();
        }
    }
}

} // namespace fh
