// Step 2d (include/mrk.h): the trainer's matrix taken from device memory - staged column-major, its cells checked, its bins found
// and its bytes written on the device (train_bins.hip), driven by capi_train.cpp (mrk_train_append_device, mrk_train_seal).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

struct mrk_ctx;

namespace mrk {

constexpr int TRAIN_STAGE_TILE = 32;      // the transposing copy moves tiles of 32 rows x 32 columns through LDS
constexpr int TRAIN_MAX_BOUNDS = 254;     // max_bin <= 255: at most max_bin - 1 bounds

// a piece of the caller's row-major matrix into a column-major piece of the staging: stage[c * rows + i] = x[i * cols + c]
void train_launch_stage(mrk_ctx *ctx, hipStream_t s, const double *x, int rows, int cols, double *stage);

// the lowest (column << 32 | row) of every kind of refused cell over the whole set, ~0 where there is none
struct TrainCellFlags {
  unsigned long long infinite;   // +-inf
  unsigned long long narrow;     // f32: finite, +-inf as an f32
  unsigned long long category;   // a categorical column: finite and >= TRAIN_MAX_CATEGORY + 1
};
// one staged piece (rows x cols column-major, its first row is row0 of the set) into *flags by integer atomic min; the caller has set
// *flags to ~0.  is_cat (null: no categorical column): per column
void train_launch_check_cells(mrk_ctx *ctx, hipStream_t s, const double *stage, int rows, int cols, long long row0, bool f32, const int *is_cat,
                              TrainCellFlags *flags);

// the sort keys of a column's cells (sort_device.hpp asc_key of the prepared cell: narrowed when f32, -0.0 as +0.0, NaN last)
void train_launch_keys(mrk_ctx *ctx, hipStream_t s, const double *col, int rows, bool f32, unsigned long long *keys);

// what the device finds for one numeric column
struct TrainColumnCuts {
  long long m;                   // non-NaN cells
  int n_bounds, pad;
  double lo, hi;                 // v[0], v[m - 1] (m > 0)
  double bounds[TRAIN_MAX_BOUNDS];
};
// bytes of scratch train_launch_cuts needs for a column of n cells (beside the keys)
size_t train_cuts_scratch_bytes(long long n);
// keys[0, n) -> *out: the keys are ordered (one workgroup up to 4096, launch_big_sort above), the changes counted, the cuts taken by
// train_cut_at (train_host.hpp).  Enqueued on s; scratch and keys must stay untouched until the launches have run
void train_launch_cuts(mrk_ctx *ctx, hipStream_t s, const unsigned long long *keys, int n, int max_bin, bool f32, void *scratch, TrainColumnCuts *out);

// hist[id] += 1 for every cell of the column with a category (0 <= trunc(x) <= TRAIN_MAX_CATEGORY); the caller zeroes hist
void train_launch_category_counts(mrk_ctx *ctx, hipStream_t s, const double *col, int rows, unsigned *hist);

// train_launch_bin / train_launch_bin_f32 (train.hpp) for a staged piece: the same bins from stage[c * piece_rows + i]
void train_launch_bin_staged(mrk_ctx *ctx, hipStream_t s, const double *stage, int piece_rows, int cols, bool f32, const double *bounds, const int *bound_off,
                             const int *cat_idx, const uint8_t *cat_tables, uint8_t *bins, long long rows, long long row0);

}  // namespace mrk
