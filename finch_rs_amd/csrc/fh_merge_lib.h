// fh_merge_lib.h -- what fh_host.cpp's finch_merge_groups (include/finch_host.h) asks of the device: Sketch.merge
// (merge_sketches, lib/src/python.rs:24-100) folded over many groups of sketches at once, one workgroup per group
// (DESIGN.md §3.12).  Not fh_merge / fh_merge_arrays, the sharded sketcher's union of partial sketches.  Defined in
// fh_merge_lib.hip; no HIP types here, fh_host.cpp is plain C++.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace fh {

// The sketches a handle's groups name, in CSR form: hashes[offsets[s] .. offsets[s + 1]) strictly ascending with their counts
// and extra counts, fewer than 2^32 - 1 entries each.  K-mer text stays on the host.
struct MergeLibInput {
    const uint64_t *hashes;
    const uint32_t *counts, *extras;
    const uint64_t *offsets; // n + 1
    uint32_t n;
};

// One group of a launch: members[mem_begin .. mem_begin + n_members) of the launch's member list (indices into the input), two
// or more, folded in that order.  Its accumulators are records [buf_off, buf_off + cap) of the launch's buffers; cap bounds the
// length after every step of the fold.  has_scale / max_hash: the first member's clip (python.rs:70-89).
struct MergeLibGroup {
    uint64_t buf_off, max_hash;
    uint32_t mem_begin, n_members, cap, has_scale;
};
static_assert(sizeof(MergeLibGroup) == 32, "the device's group descriptor");

// A record of an accumulator: count and extra are the wrapping u32 sums; (slot, pos) says whose k-mer text the record carries:
// entry pos of the group's member slot (the earliest member that held the hash).
struct MergeLibRecord {
    uint64_t hash;
    uint32_t count, extra, slot, pos;
};
static_assert(sizeof(MergeLibRecord) == 24, "the device's record");

// where a group's result lies in the launch's packed record list
struct MergeLibOut {
    uint32_t len, place;
};

constexpr uint32_t MERGE_LIB_MAX_TILE = 4096; // output positions per tile at most (16 per thread)

struct MergeLibDevice;
// checks the input's offsets, uploads it to `device` once (*upload_ms: wall time of that) and allocates two sets of buffers for
// launches of at most max_groups groups, max_members member entries and max_records records (the sum of the groups' caps);
// tile: output positions per tile, 1 .. MERGE_LIB_MAX_TILE; size: NULL is None
int merge_lib_open(int device, const MergeLibInput &in, uint32_t max_groups, uint64_t max_members, uint64_t max_records, uint32_t tile,
                   const uint64_t *size, MergeLibDevice **out, double *upload_ms);
// async on the handle's stream, into buffer set `buf` (0 / 1): the fold of every group.  Everything the kernel indexes with is
// checked here: member indices, the groups' places in the buffers, cap >= the first member's length.
int merge_lib_launch(MergeLibDevice *d, int buf, const MergeLibGroup *groups, uint32_t n_groups, const uint32_t *members, uint64_t n_members);
// waits for buffer set `buf`: outs[g] places group g's result in records[0 .. *n_records) (valid until the set's next launch);
// *kernel_ms: the kernel's time (HIP events), *copy_ms: wall time of the copy back
int merge_lib_wait(MergeLibDevice *d, int buf, const MergeLibOut **outs, const MergeLibRecord **records, uint64_t *n_records,
                   double *kernel_ms, double *copy_ms);
void merge_lib_close(MergeLibDevice *d);

} // namespace fh
