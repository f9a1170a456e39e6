// The evaluation that ends a train (LambdaMARTModel.eval, ml/rank/LambdaMARTRanker.scala:406-445) on the device: every group of
// the test split ordered by score and reduced to NDCG@k / MAP@k / MRR.  The formulas are include/mrk.h's (ASSUMPTIONS: ltrlib's
// metric sources are not in the reference tree); what every kernel here computes per group of n items:
//   1. pi, the order of sortBy(-score): ascending (sort_key(score), index) under pair_lt - the order /rank answers in.  Without
//      scores (noopArray: strictly decreasing) pi is the identity and nothing is sorted.
//   2. terms t[i] = gain[pi(i)] / lg[i] - one division per item, all items at once: only the SUM is ordered - and the bit mask
//      rel of "label > 0" in pi order.
//   3. with an NDCG metric, the same terms over the gains sorted descending (ascending sort_key(gain)).
//   4. one lane per asked-for metric adds the first k terms one after the other (NDCG), or walks the set bits of rel (MAP,
//      MRR).  All metrics of a call share steps 1-3.
// log2 and pow are the host's (the lg table, the gains): the kernels divide, add and compare, each correctly rounded and never
// fused.  A group's values go to its own index: nothing depends on which kernel or workgroup took it, and no float atomics.
//   n <= 64                  eval_wave_kernel: one wavefront per group, one lane per item, four groups per workgroup.  No sort
//                            network: a lane's rank is the number of pairs that are pair_lt its own.
//   n <= SORT_MAX_ITEMS      eval_group_kernel: one workgroup per group, the LDS bitonic of bitonic_device.hpp on (key, u16 index),
//                            padded to the next power of two >= n.  44.5 KiB of LDS.
//   beyond                   bigsort.hip's sample sort for both orders, a gather kernel for step 2, one wavefront for step 4.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bitonic_device.hpp"
#include "eval.hpp"
#include "eval_host.hpp"
#include "rank.hpp"
#include "rank_launch.hpp"
#include "runtime.hpp"
#include "sort_device.hpp"
#include "wave_device.hpp"

namespace mrk {

static_assert(EVAL_GROUP_ITEMS == SORT_MAX_ITEMS, "the workgroup kernel takes what one workgroup sorts");
static_assert(EVAL_GROUP_ITEMS <= 65536, "the workgroup kernel keeps indices as u16");

namespace {

typedef unsigned long long u64;

constexpr int EV_WAVES = 4;   // groups per workgroup of the wavefront kernel

__device__ __forceinline__ double as_f64(u64 b) { return __longlong_as_double((long long)b); }
__device__ __forceinline__ u64 as_bits(double v) { return (u64)__double_as_longlong(v); }
__device__ __forceinline__ int cut(int cutoff, int n) { return cutoff == 0 || cutoff > n ? n : cutoff; }

// the first k >= 1 terms added in index order; the first starts the sum
__device__ double sum_terms(const u64 *t, int k) {
  double s = as_f64(t[0]);
  for (int i = 1; i < k; ++i) s = __dadd_rn(s, as_f64(t[i]));
  return s;
}

// rel: bit i of the mask = the item at position i is relevant; bits at n and beyond are 0
__device__ double map_value(const u64 *rel, int n, int k) {
  int R = 0;
  for (int w = 0; w * 64 < n; ++w) R += __popcll(rel[w]);
  if (R == 0) return 0.0;
  int hits = 0;
  double sum = 0.0;
  for (int w = 0; w * 64 < k; ++w) {
    u64 b = rel[w];
    const int left = k - w * 64;
    if (left < 64) b &= (1ull << left) - 1ull;
    while (b) {
      const int i = w * 64 + __ffsll((long long)b) - 1;
      ++hits;
      sum = __dadd_rn(sum, __ddiv_rn((double)hits, (double)(i + 1)));
      b &= b - 1ull;
    }
  }
  return __ddiv_rn(sum, (double)min(R, k));
}

__device__ double mrr_value(const u64 *rel, int n) {
  for (int w = 0; w * 64 < n; ++w) {
    const u64 b = rel[w];
    if (b) return __ddiv_rn(1.0, (double)(w * 64 + __ffsll((long long)b)));
  }
  return 0.0;
}

__device__ __forceinline__ double ndcg_value(double dcg, double idcg, double nolabels) { return idcg == 0.0 ? nolabels : __ddiv_rn(dcg, idcg); }

// step 4 where the terms of both orders are at hand
__device__ double metric_value(int metric, int cutoff, int n, const u64 *t, const u64 *it, const u64 *rel, double nolabels) {
  const int k = cut(cutoff, n);
  if (metric == MRK_METRIC_NDCG) return ndcg_value(sum_terms(t, k), sum_terms(it, k), nolabels);
  if (metric == MRK_METRIC_MAP) return map_value(rel, n, k);
  return mrr_value(rel, n);
}

__global__ void __launch_bounds__(EV_WAVES * 64)
eval_wave_kernel(EvalDev d, const int *__restrict__ groups, int count) {
  __shared__ u64 s_key[EV_WAVES][64];
  __shared__ u64 s_t[EV_WAVES][64], s_it[EV_WAVES][64];
  __shared__ unsigned char s_r[EV_WAVES][64];
  __shared__ u64 s_rel[EV_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int gi = blockIdx.x * EV_WAVES + wave;
  if (gi >= count) return;   // (a whole wavefront: the slices below are its own, ordered by wave_lds_sync)
  const int g = groups[gi];
  const long long base = d.offsets[g];
  const int n = (int)(d.offsets[g + 1] - base);   // 1 ... 64
  const bool mine = lane < n;
  const double gain = mine ? d.gains[base + lane] : 0.0;
  int rank = lane;
  if (d.scores) {
    const u64 key = mine ? sort_key(d.scores[base + lane]) : ~0ull;
    s_key[wave][lane] = key;
    wave_lds_sync();
    rank = 0;
    if (mine)
      for (int j = 0; j < n; ++j) rank += pair_lt(s_key[wave][j], j, key, lane) ? 1 : 0;
    wave_lds_sync();   // (s_key is written again below)
  }
  if (mine) {
    s_t[wave][rank] = as_bits(gain);
    s_r[wave][rank] = d.rel[base + lane];
  }
  wave_lds_sync();
  const u64 relmask = __ballot(mine && s_r[wave][lane] != 0);
  if (lane == 0) s_rel[wave] = relmask;
  if (mine) s_t[wave][lane] = as_bits(__ddiv_rn(as_f64(s_t[wave][lane]), d.lg[lane]));
  if (d.need_ideal) {
    const u64 key = mine ? sort_key(gain) : ~0ull;
    s_key[wave][lane] = key;
    wave_lds_sync();
    int r2 = 0;
    if (mine) {
      for (int j = 0; j < n; ++j) r2 += pair_lt(s_key[wave][j], j, key, lane) ? 1 : 0;
      s_it[wave][r2] = as_bits(gain);
    }
    wave_lds_sync();
    if (mine) s_it[wave][lane] = as_bits(__ddiv_rn(as_f64(s_it[wave][lane]), d.lg[lane]));
  }
  wave_lds_sync();
  for (int m = lane; m < d.n_metrics; m += 64)
    d.out[(long long)m * d.n_groups + g] = metric_value(d.metrics[m], d.cutoffs[m], n, s_t[wave], s_it[wave], &s_rel[wave], d.nolabels);
}

// blockDim.x: a multiple of 64 up to 1024
__global__ void __launch_bounds__(1024)
eval_group_kernel(EvalDev d, const int *__restrict__ groups) {
  __shared__ u64 s_key[EVAL_GROUP_ITEMS];
  __shared__ unsigned short s_idx[EVAL_GROUP_ITEMS];
  __shared__ u64 s_rel[EVAL_GROUP_ITEMS / 64];
  const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63;
  const int g = groups[blockIdx.x];
  const long long base = d.offsets[g];
  const int n = (int)(d.offsets[g + 1] - base);   // 1 ... EVAL_GROUP_ITEMS
  int p2 = 1;
  while (p2 < n) p2 <<= 1;
  const bool sorted = d.scores != nullptr;
  if (sorted) {
    for (int i = tid; i < p2; i += T) {
      s_key[i] = i < n ? sort_key(d.scores[base + i]) : ~0ull;   // (a pad sorts behind every score: NaN's key is 0xfff8...)
      s_idx[i] = (unsigned short)(i < n ? i : 0xffff);
    }
    __syncthreads();
    lds_bitonic<true>(s_key, s_idx, p2);
  }
  // steps 2: thread i owns position i - it reads s_idx[i] and overwrites the dead key beside it
  const int n64 = (n + 63) & ~63;
  for (int i = tid; i < n64; i += T) {   // (whole wavefronts: tid - lane and n64 are multiples of 64)
    const int src = i < n ? (sorted ? (int)s_idx[i] : i) : 0;
    const u64 b = __ballot(i < n && d.rel[base + src] != 0);
    if (lane == 0) s_rel[i >> 6] = b;
    if (i < n) s_key[i] = as_bits(__ddiv_rn(d.gains[base + src], d.lg[i]));
  }
  __syncthreads();
  for (int m = tid; m < d.n_metrics; m += T) {
    const int metric = d.metrics[m], k = cut(d.cutoffs[m], n);
    d.out[(long long)m * d.n_groups + g] = metric == MRK_METRIC_NDCG ? sum_terms(s_key, k) : metric == MRK_METRIC_MAP ? map_value(s_rel, n, k) : mrr_value(s_rel, n);
  }
  if (!d.need_ideal) return;
  __syncthreads();
  for (int i = tid; i < p2; i += T) s_key[i] = i < n ? sort_key(d.gains[base + i]) : ~0ull;
  __syncthreads();
  lds_bitonic<false>(s_key, nullptr, p2);
  for (int i = tid; i < n; i += T) s_key[i] = as_bits(__ddiv_rn(-asc_value(s_key[i]), d.lg[i]));   // sort_key(v) = asc_key(-v)
  __syncthreads();
  for (int m = tid; m < d.n_metrics; m += T)
    if (d.metrics[m] == MRK_METRIC_NDCG) {
      double *o = d.out + (long long)m * d.n_groups + g;   // the DCG this thread left there
      *o = ndcg_value(*o, sum_terms(s_key, cut(d.cutoffs[m], n)), d.nolabels);
    }
}

// step 2 of a group beyond one workgroup: terms[i] = gains[order[i]] / lg[i] and - relwords given - the mask of rel in that order
__global__ void __launch_bounds__(256)
eval_big_gather_kernel(const int *__restrict__ order, const double *__restrict__ gains, const uint8_t *__restrict__ rel, const double *__restrict__ lg,
                       int n, double *__restrict__ terms, u64 *__restrict__ relwords) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;   // (the grid covers n rounded up to whole wavefronts)
  const bool in = i < n;
  const int src = in ? (order ? order[i] : (int)i) : 0;
  if (relwords) {
    const u64 b = __ballot(in && rel[src] != 0);
    if ((threadIdx.x & 63) == 0 && (i >> 6) < ((long long)n + 63) / 64) relwords[i >> 6] = b;
  }
  if (in) terms[i] = __ddiv_rn(gains[src], lg[i]);
}

__global__ void __launch_bounds__(64)
eval_big_walk_kernel(EvalDev d, int g, int n, const u64 *__restrict__ terms, const u64 *__restrict__ iterms, const u64 *__restrict__ relwords) {
  for (int m = threadIdx.x; m < d.n_metrics; m += 64)
    d.out[(long long)m * d.n_groups + g] = metric_value(d.metrics[m], d.cutoffs[m], n, terms, iterms, relwords, d.nolabels);
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

void eval_launch_wave(mrk_ctx *ctx, hipStream_t s, const EvalDev &d, const int *groups, int count) {
  if (count <= 0) return;
  ScopedKernelTimer timer(ctx, "eval_wave");
  hipLaunchKernelGGL(eval_wave_kernel, dim3((unsigned)((count + EV_WAVES - 1) / EV_WAVES)), dim3(EV_WAVES * 64), 0, s, d, groups, count);
  MRK_HIP(hipGetLastError());
}

void eval_launch_group(mrk_ctx *ctx, hipStream_t s, const EvalDev &d, const int *groups, int count, int max_len) {
  if (count <= 0) return;
  ScopedKernelTimer timer(ctx, "eval_group");
  // a bin of short groups (the 65 ... 100 items of a click-through beyond one wavefront) gets workgroups of its size: a stage of the
  // network over 128 pairs keeps 256 lanes busy, not 1 024
  const int threads = max_len <= 512 ? 256 : max_len <= 2048 ? 512 : 1024;
  hipLaunchKernelGGL(eval_group_kernel, dim3((unsigned)count), dim3(threads), 0, s, d, groups);
  MRK_HIP(hipGetLastError());
}

// [sort scratch][order int x n][terms f64 x n][ideal terms f64 x n][rel words]
size_t eval_big_scratch_bytes(int n) {
  return align256(big_sort_scratch_bytes(n)) + align256((size_t)n * 4) + 2 * align256((size_t)n * 8) + align256(((size_t)n + 63) / 64 * 8);
}

void eval_launch_big(mrk_ctx *ctx, hipStream_t s, const EvalDev &d, int group, long long base, int n, void *scratch) {
  ScopedKernelTimer timer(ctx, "eval_big");
  uint8_t *p = (uint8_t *)scratch;
  void *sort_scratch = p;
  p += align256(big_sort_scratch_bytes(n));
  int *order = (int *)p;
  p += align256((size_t)n * 4);
  double *terms = (double *)p;
  p += align256((size_t)n * 8);
  double *iterms = (double *)p;
  p += align256((size_t)n * 8);
  u64 *relwords = (u64 *)p;
  const unsigned grid = (unsigned)(((long long)n + 255) / 256);
  if (d.scores) {
    const SortSrc src{d.scores + base, nullptr, 1, 1};
    launch_big_sort(ctx, s, src, n, order, sort_scratch);
  }
  hipLaunchKernelGGL(eval_big_gather_kernel, dim3(grid), dim3(256), 0, s, d.scores ? order : nullptr, d.gains + base, d.rel + base, d.lg, n, terms, relwords);
  MRK_HIP(hipGetLastError());
  if (d.need_ideal) {
    const SortSrc src{d.gains + base, nullptr, 1, 1};
    launch_big_sort(ctx, s, src, n, order, sort_scratch);
    hipLaunchKernelGGL(eval_big_gather_kernel, dim3(grid), dim3(256), 0, s, order, d.gains + base, d.rel + base, d.lg, n, iterms, (u64 *)nullptr);
    MRK_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(eval_big_walk_kernel, dim3(1), dim3(64), 0, s, d, group, n, (const u64 *)terms, (const u64 *)iterms, (const u64 *)relwords);
  MRK_HIP(hipGetLastError());
}

}  // namespace mrk
