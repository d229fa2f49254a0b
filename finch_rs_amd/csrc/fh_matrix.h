// fh_matrix.h -- what fh_host.cpp's finch_minmer_matrix (include/finch_host.h) asks of the device: the count matrix of
// distance.rs:345-364, rows of many sketches against one reference sketch.  Defined in fh_matrix.hip; no HIP
// types here, fh_host.cpp is plain C++.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace fh {

constexpr uint32_t MATRIX_MAX_SLICE = 4096;  // sketch entries (u64 hash + u32 count) one LDS slice holds at most (48 KiB)
constexpr uint32_t MATRIX_MAX_ROWS = 65535;  // rows of one launch (the grid's y)

struct MatrixDevice;
// uploads the reference's n_ref >= 1 strictly ascending hashes to `device` once and allocates two chunk buffers there, each
// with its pinned twin: the sketches of a chunk (at most max_rows rows of max_entries entries together, none longer than
// `longest`) and its max_rows x n_ref result
int matrix_open(int device, const uint64_t *ref, uint32_t n_ref, uint32_t max_rows, uint64_t max_entries, uint32_t longest,
                uint32_t slice, MatrixDevice **out);
// buffer `buf`'s (0 / 1) pinned input for a chunk of `rows` rows and `entries` entries together, for the caller to fill before
// matrix_launch: offsets[0 .. rows] into hashes / counts (CSR, offsets[0] = 0, offsets[rows] = entries), every row strictly
// ascending
int matrix_stage(MatrixDevice *d, int buf, uint32_t rows, uint64_t entries, uint64_t **offsets, uint64_t **hashes, uint32_t **counts);
// async on the handle's stream: the staged sketches to the device, the kernel, the rows x n_ref result back to the host
int matrix_launch(MatrixDevice *d, int buf);
// waits for buffer `buf`: *out = its rows, row-major (pinned; valid until the buffer's next launch); *kernel_ms = the kernel's
// time (HIP events)
int matrix_wait(MatrixDevice *d, int buf, const int32_t **out, double *kernel_ms);
void matrix_close(MatrixDevice *d);
// the calling thread's current device (-1 if it cannot be told), and back to it
int matrix_current_device();
void matrix_restore_device(int device);

} // namespace fh
