// Step 2d of the LambdaMART fit (include/mrk.h): the trainer's matrix comes from DEVICE memory.
//   train_stage            a transposing copy of a row-major piece into a column-major piece of the staging (32 x 32 tiles through LDS)
//   train_check_cells      the refusals of steps 1, 2x and 2c: the lowest offending (column, row) of each kind, integer atomic min
//   train_keys             a column's cells as sort keys: narrowed to f32 for step 2x, -0.0 as +0.0, NaN above everything
//   the order              one workgroup's LDS bitonic network up to 4096 cells, bigsort.hip's sample sort on (key, row) pairs above:
//                          the row is part of the pair, so a column of two values splits into buckets as evenly as any other
//   train_changes          m = the non-NaN cells, the number of positions p with v[p] != v[p - 1], and up to 256 of them in any
//                          order (integer atomics; a list that is read holds ALL changes, and is ranked before use)
//   train_cuts             one workgroup, one lane per cut: train_cut_at (train_host.hpp), the body the host test checks
//   train_category_counts  step 2c's histogram over ids 0 ... 32764, one integer atomic per distinct id of a wavefront
//   train_bin_staged       train_bin / train_bin_f32 (train.hip) reading the column-major staging
// No float atomics, nothing that depends on the order anything runs in.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bitonic_device.hpp"
#include "rank_launch.hpp"
#include "runtime.hpp"
#include "sort_device.hpp"
#include "train.hpp"
#include "train_bins.hpp"
#include "train_host.hpp"

namespace mrk {

namespace {

using u64 = unsigned long long;

constexpr int TB_THREADS = 256;
constexpr int TB_ONE_WG = 4096;          // cells ONE workgroup orders (launch_big_sort takes more than that)
constexpr int TB_LIST = 256;             // change positions kept (>= TRAIN_MAX_BOUNDS)
constexpr int TB_CHANGE_TILE = 2048;     // positions per workgroup of the pass that counts the changes

struct CutCounters {
  u64 m;
  unsigned n_change, pad;
  int list[TB_LIST];
};

__global__ void __launch_bounds__(TB_THREADS)
train_stage_kernel(const double *__restrict__ x, int rows, int cols, double *__restrict__ stage) {
  __shared__ double tile[TRAIN_STAGE_TILE][TRAIN_STAGE_TILE + 1];
  const int r0 = blockIdx.x * TRAIN_STAGE_TILE, c0 = blockIdx.y * TRAIN_STAGE_TILE;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int k = ty; k < TRAIN_STAGE_TILE; k += TB_THREADS / 32) {
    const int r = r0 + k, c = c0 + tx;
    if (r < rows && c < cols) tile[k][tx] = x[(long long)r * cols + c];
  }
  __syncthreads();
  for (int k = ty; k < TRAIN_STAGE_TILE; k += TB_THREADS / 32) {
    const int c = c0 + k, r = r0 + tx;
    if (r < rows && c < cols) stage[(long long)c * rows + r] = tile[tx][k];
  }
}

__global__ void __launch_bounds__(TB_THREADS)
train_check_cells_kernel(const double *__restrict__ stage, int rows, long long row0, int f32, const int *__restrict__ is_cat, TrainCellFlags *flags) {
  const int i = blockIdx.x * TB_THREADS + threadIdx.x, c = blockIdx.y;
  if (i >= rows) return;
  const double x = stage[(long long)c * rows + i];
  const u64 at = ((u64)c << 32) | (u64)(row0 + i);
  if (x != x) return;
  if (isinf(x)) {
    atomicMin(&flags->infinite, at);
    return;
  }
  if (f32 && isinf(__double2float_rn(x))) atomicMin(&flags->narrow, at);
  if (is_cat && is_cat[c] && x >= (double)(TRAIN_MAX_CATEGORY + 1)) atomicMin(&flags->category, at);
}

// the cell as steps 2 / 2x order it
__device__ __forceinline__ double prepared(double x, int f32) {
  if (f32) x = (double)__double2float_rn(x);
  return x == 0.0 ? 0.0 : x;   // -0.0 and +0.0 are one value
}

__global__ void __launch_bounds__(TB_THREADS)
train_keys_kernel(const double *__restrict__ col, int rows, int f32, u64 *__restrict__ keys) {
  const int i = blockIdx.x * TB_THREADS + threadIdx.x;
  if (i < rows) keys[i] = asc_key(prepared(col[i], f32));
}

// n <= TB_ONE_WG keys ordered by one workgroup; sorted[p] = the value of the p-th (NaN for the NaN cells at the end)
__global__ void __launch_bounds__(1024)
train_small_sort_kernel(const u64 *__restrict__ keys, int n, double *__restrict__ sorted) {
  __shared__ u64 s_key[TB_ONE_WG];
  int p2 = 1;
  while (p2 < n) p2 <<= 1;
  for (int i = threadIdx.x; i < p2; i += 1024) s_key[i] = i < n ? keys[i] : ~0ull;
  __syncthreads();
  lds_bitonic<false>(s_key, nullptr, p2);
  for (int i = threadIdx.x; i < n; i += 1024) sorted[i] = asc_value(s_key[i]);
}

__global__ void __launch_bounds__(TB_THREADS)
train_gather_kernel(const u64 *__restrict__ keys, const int *__restrict__ order, int n, double *__restrict__ sorted) {
  const int p = blockIdx.x * TB_THREADS + threadIdx.x;
  if (p < n) sorted[p] = asc_value(keys[order[p]]);
}

// A workgroup takes TB_CHANGE_TILE positions and counts in LDS; two global atomics per workgroup (one per wavefront - 86 000 on two
// addresses for 5.5 M cells - made this pass 2 ms of a column's 3)
__global__ void __launch_bounds__(TB_THREADS)
train_changes_kernel(const double *__restrict__ sorted, int n, CutCounters *ctr) {
  __shared__ unsigned s_values, s_changes, s_base;
  __shared__ int s_list[TB_LIST];
  const int tid = threadIdx.x, lane = threadIdx.x & 63;
  if (tid == 0) s_values = 0u, s_changes = 0u;
  __syncthreads();
  const long long lo = (long long)blockIdx.x * TB_CHANGE_TILE;
  unsigned wave_values = 0;
  for (int k = 0; k < TB_CHANGE_TILE / TB_THREADS; ++k) {   // (uniform: every lane of a wavefront takes part in the ballots)
    const long long p = lo + k * TB_THREADS + tid;
    const double a = p < n ? sorted[p] : __longlong_as_double(0x7ff8000000000000LL);
    const bool value = a == a;
    const bool change = value && p > 0 && a != sorted[p - 1];   // (the NaN cells are last: sorted[p - 1] is a value)
    const u64 values = __ballot(value), changes = __ballot(change);
    wave_values += (unsigned)__popcll(values);
    unsigned base = 0;
    if (lane == 0 && changes) base = atomicAdd(&s_changes, (unsigned)__popcll(changes));
    base = (unsigned)__shfl((int)base, 0, 64);
    const unsigned slot = base + (unsigned)__popcll(changes & ((1ull << lane) - 1ull));
    if (change && slot < (unsigned)TB_LIST) s_list[slot] = (int)p;
  }
  if (lane == 0 && wave_values) atomicAdd(&s_values, wave_values);
  __syncthreads();
  if (tid == 0) {
    if (s_values) atomicAdd(&ctr->m, (u64)s_values);
    s_base = s_changes ? atomicAdd(&ctr->n_change, s_changes) : 0u;
  }
  __syncthreads();
  const unsigned base = s_base, mine = min(s_changes, (unsigned)TB_LIST);
  for (unsigned j = tid; j < mine; j += TB_THREADS)
    if (base + j < (unsigned)TB_LIST) ctr->list[base + j] = s_list[j];
}

__global__ void __launch_bounds__(TB_THREADS)
train_cuts_kernel(const double *__restrict__ sorted, const CutCounters *__restrict__ ctr, int max_bin, int f32, TrainColumnCuts *__restrict__ out) {
  __shared__ long long s_cut[TB_THREADS];
  __shared__ int s_keep[TB_THREADS];
  const int tid = threadIdx.x;
  const long long m = (long long)ctr->m;
  const int n_change = (int)ctr->n_change;
  auto v = [&](long long p) { return sorted[p]; };
  if (tid == 0) {
    out->m = m;
    out->lo = m > 0 ? sorted[0] : 0.0;
    out->hi = m > 0 ? sorted[m - 1] : 0.0;
  }
  if (n_change <= max_bin - 2) {   // every change is a cut; the list holds them all, in any order
    if (tid < n_change) {
      const int p = ctr->list[tid];
      int rank = 0;
      for (int j = 0; j < n_change; ++j) rank += ctr->list[j] < p ? 1 : 0;
      double bound = 0.0;
      (void)train_cut_at(v, m, (long long)p, f32 != 0, &bound);
      out->bounds[rank] = bound;
    }
    if (tid == 0) out->n_bounds = n_change;
    return;
  }
  const int i = tid + 1;
  const bool lane_cut = i <= max_bin - 2;
  double bound = 0.0;
  const long long cut = lane_cut ? train_cut_at(v, m, train_cut_target(m, max_bin, i), f32 != 0, &bound) : m;
  s_cut[tid] = cut;
  __syncthreads();
  // cuts ascend with i: the first i without one ends them, a cut equal to the one before is dropped
  const int keep = lane_cut && cut < m && (tid == 0 || s_cut[tid - 1] != cut) ? 1 : 0;
  s_keep[tid] = keep;
  __syncthreads();
  int slot = 0, total = 0;
  for (int j = 0; j < TB_THREADS; ++j) {
    slot += j < tid ? s_keep[j] : 0;
    total += s_keep[j];
  }
  if (keep) out->bounds[slot] = bound;
  if (tid == 0) out->n_bounds = total;
}

__global__ void __launch_bounds__(TB_THREADS)
train_category_counts_kernel(const double *__restrict__ col, int rows, unsigned *hist) {
  const int i = blockIdx.x * TB_THREADS + threadIdx.x;
  const double x = i < rows ? col[i] : -1.0;
  const int id = x > -1.0 && x < (double)(TRAIN_MAX_CATEGORY + 1) ? (int)x : -1;   // (NaN fails both; -1 < x < 0 truncates to category 0)
  const int lane = threadIdx.x & 63;
  u64 todo = __ballot(id >= 0);
  while (todo) {   // (uniform) one atomic per distinct id of the wavefront
    const int leader = __builtin_ctzll(todo);
    const int of = __shfl(id, leader, 64);
    const u64 same = __ballot(id == of);
    if (lane == leader) atomicAdd(&hist[of], (unsigned)__popcll(same));
    todo &= ~same;
  }
}

template <bool F32>
__global__ void __launch_bounds__(TRAIN_BIN_ROWS)
train_bin_staged_kernel(const double *__restrict__ stage, int piece_rows, const double *__restrict__ bounds, const int *__restrict__ bound_off,
                        const int *__restrict__ cat_idx, const uint8_t *__restrict__ cat_tables, uint8_t *__restrict__ bins, long long rows, long long row0) {
  const int i = blockIdx.x * TRAIN_BIN_ROWS + threadIdx.x, c = blockIdx.y;
  if (i >= piece_rows) return;
  const double x = stage[(long long)c * piece_rows + i];
  uint8_t *out = bins + (long long)c * rows + row0 + i;
  if (!F32 && cat_idx && cat_idx[2 * c] >= 0) {   // (the same for every lane: a categorical column, step 2c)
    *out = (uint8_t)train_category_bin(x, cat_tables + cat_idx[2 * c], cat_idx[2 * c + 1]);
    return;
  }
  int a = bound_off[c], b = bound_off[c + 1];
  const int first = a;
  if (F32) {
    const float v = __double2float_rn(x);
    while (a < b) {   // the number of bounds <= v (a bound is an f32 value: the conversion is exact)
      const int m = (a + b) >> 1;
      if ((float)bounds[m] <= v) a = m + 1;
      else b = m;
    }
  } else {
    while (a < b) {   // the number of bounds < x
      const int m = (a + b) >> 1;
      if (bounds[m] < x) a = m + 1;
      else b = m;
    }
  }
  *out = x != x ? (uint8_t)TRAIN_NAN_BIN : (uint8_t)(a - first);
}

size_t align256(size_t b) { return (b + 255) / 256 * 256; }

}  // namespace

void train_launch_stage(mrk_ctx *ctx, hipStream_t s, const double *x, int rows, int cols, double *stage) {
  ScopedKernelTimer timer(ctx, "train_stage");
  const dim3 grid((unsigned)((rows + TRAIN_STAGE_TILE - 1) / TRAIN_STAGE_TILE), (unsigned)((cols + TRAIN_STAGE_TILE - 1) / TRAIN_STAGE_TILE));
  hipLaunchKernelGGL(train_stage_kernel, grid, dim3(TB_THREADS), 0, s, x, rows, cols, stage);
  MRK_HIP(hipGetLastError());
}

void train_launch_check_cells(mrk_ctx *ctx, hipStream_t s, const double *stage, int rows, int cols, long long row0, bool f32, const int *is_cat,
                              TrainCellFlags *flags) {
  ScopedKernelTimer timer(ctx, "train_check");
  hipLaunchKernelGGL(train_check_cells_kernel, dim3((unsigned)((rows + TB_THREADS - 1) / TB_THREADS), (unsigned)cols), dim3(TB_THREADS), 0, s, stage, rows, row0,
                     f32 ? 1 : 0, is_cat, flags);
  MRK_HIP(hipGetLastError());
}

void train_launch_keys(mrk_ctx *ctx, hipStream_t s, const double *col, int rows, bool f32, unsigned long long *keys) {
  ScopedKernelTimer timer(ctx, "train_keys");
  hipLaunchKernelGGL(train_keys_kernel, dim3((unsigned)((rows + TB_THREADS - 1) / TB_THREADS)), dim3(TB_THREADS), 0, s, col, rows, f32 ? 1 : 0, keys);
  MRK_HIP(hipGetLastError());
}

// [counters][sorted values n x 8][order n x 4][the sample sort's scratch]
size_t train_cuts_scratch_bytes(long long n) {
  const size_t big = n > TB_ONE_WG ? align256((size_t)n * 4) + align256(big_sort_scratch_bytes((int)n)) : 0;
  return align256(sizeof(CutCounters)) + align256((size_t)n * 8) + big;
}

void train_launch_cuts(mrk_ctx *ctx, hipStream_t s, const unsigned long long *keys, int n, int max_bin, bool f32, void *scratch, TrainColumnCuts *out) {
  uint8_t *p = (uint8_t *)scratch;
  CutCounters *ctr = (CutCounters *)p;
  p += align256(sizeof(CutCounters));
  double *sorted = (double *)p;
  p += align256((size_t)n * 8);
  MRK_HIP(hipMemsetAsync(ctr, 0, sizeof(CutCounters), s));
  {
    ScopedKernelTimer timer(ctx, "train_sort");
    if (n <= TB_ONE_WG) {
      hipLaunchKernelGGL(train_small_sort_kernel, dim3(1), dim3(1024), 0, s, keys, n, sorted);
    } else {
      int *order = (int *)p;
      p += align256((size_t)n * 4);
      const SortSrc src{nullptr, keys, 1, 0};
      launch_big_sort(ctx, s, src, n, order, p);
      hipLaunchKernelGGL(train_gather_kernel, dim3((unsigned)((n + TB_THREADS - 1) / TB_THREADS)), dim3(TB_THREADS), 0, s, keys, order, n, sorted);
    }
    MRK_HIP(hipGetLastError());
  }
  ScopedKernelTimer timer(ctx, "train_cuts");
  hipLaunchKernelGGL(train_changes_kernel, dim3((unsigned)((n + TB_CHANGE_TILE - 1) / TB_CHANGE_TILE)), dim3(TB_THREADS), 0, s, sorted, n, ctr);
  hipLaunchKernelGGL(train_cuts_kernel, dim3(1), dim3(TB_THREADS), 0, s, sorted, ctr, max_bin, f32 ? 1 : 0, out);
  MRK_HIP(hipGetLastError());
}

void train_launch_category_counts(mrk_ctx *ctx, hipStream_t s, const double *col, int rows, unsigned *hist) {
  ScopedKernelTimer timer(ctx, "train_cat_counts");
  hipLaunchKernelGGL(train_category_counts_kernel, dim3((unsigned)((rows + TB_THREADS - 1) / TB_THREADS)), dim3(TB_THREADS), 0, s, col, rows, hist);
  MRK_HIP(hipGetLastError());
}

void train_launch_bin_staged(mrk_ctx *ctx, hipStream_t s, const double *stage, int piece_rows, int cols, bool f32, const double *bounds, const int *bound_off,
                             const int *cat_idx, const uint8_t *cat_tables, uint8_t *bins, long long rows, long long row0) {
  ScopedKernelTimer timer(ctx, "train_bin");
  const dim3 grid((unsigned)((piece_rows + TRAIN_BIN_ROWS - 1) / TRAIN_BIN_ROWS), (unsigned)cols);
  if (f32) hipLaunchKernelGGL(train_bin_staged_kernel<true>, grid, dim3(TRAIN_BIN_ROWS), 0, s, stage, piece_rows, bounds, bound_off, cat_idx, cat_tables, bins, rows, row0);
  else hipLaunchKernelGGL(train_bin_staged_kernel<false>, grid, dim3(TRAIN_BIN_ROWS), 0, s, stage, piece_rows, bounds, bound_off, cat_idx, cat_tables, bins, rows, row0);
  MRK_HIP(hipGetLastError());
}

}  // namespace mrk
