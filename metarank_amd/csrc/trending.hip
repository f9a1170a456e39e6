// The fit of the trending recommender (TrendingPredictor.fit, ml/recommend/TrendingRecommender.scala:39-87) on the device:
// the reference's filter + groupBy + per-item day arrays + decayed sum + sortBy over the whole click-through history.
//
//   1. trending_count_kernel: a grid-stride loop over the staged interactions (u32 item, i32 weight index or -1, i64 ts).
//      An interaction counts for its weight w iff ts > now - window_w (:52-53, strict); its bucket is (now - ts) / 86 400 000
//      (:57) and it adds 1 to the u32 count table[w][day][item] (item-minor: the score kernel's lanes read consecutive
//      words for every day).  Counts are integers, so the table does not depend on arrival order.  A bucket >= days_w is
//      the reference's ArrayIndexOutOfBounds (:58-59): the weight's index + 1 goes to an error word, nothing is clamped.
//      Real histories are Zipf-shaped - today's bucket of a few hot items takes most of the adds -, so lanes of a
//      wavefront that hit the same bin are combined first: the first live lane's bin is broadcast, the lanes that hold it
//      are counted by a ballot, the leader issues ONE atomic of that count, those lanes retire; repeat until none is live.
//      A wavefront of 64 equal bins issues 1 atomic instead of 64; one of 64 different bins loops 64 times over a few ALU
//      instructions and issues the same 64 atomics as before.
//   2. trending_score_kernel: one lane per item, weights in config order; per weight the loop over ALL its days
//      s = s + (double)count[i] * pow[i] (:72-77; separate f64 multiply and add - the JVM never fuses), times the weight
//      (:78); an item without a counted interaction for the weight gets +0.0 instead (:79).  The parts are summed left to
//      right starting from the first (:82).  Weights and pow tables are read at wave-uniform addresses.
//   3. the order of sortBy(-score) (:85): (sort_key(score), item index) pairs - items are numbered in order of first
//      appearance, so the index IS the stable sort's tie-break - by one workgroup for up to SORT_MAX_ITEMS items and by
//      bigsort.hip's sample sort beyond.
// No float atomics anywhere: the result is bit-reproducible.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rank.hpp"
#include "rank_launch.hpp"
#include "runtime.hpp"
#include "sort_device.hpp"
#include "trending.hpp"

namespace mrk {

namespace {

constexpr int TR_THREADS = 256;
constexpr long long TR_DAY_MS = 86400000;
constexpr unsigned long long TR_NO_BIN = ~0ull;

template <int MODE>
__global__ void __launch_bounds__(TR_THREADS)
trending_count_kernel(const uint32_t *__restrict__ item, const int32_t *__restrict__ widx, const long long *__restrict__ ts, long long n,
                      long long now_ms, const TrendingWeightDev *__restrict__ weights, long long items, uint32_t *__restrict__ table,
                      uint32_t *__restrict__ err) {
  const int lane = threadIdx.x & 63;
  const long long stride = (long long)gridDim.x * TR_THREADS;
  // whole wavefronts stay in the loop together (the bound is on the wavefront's first interaction): the ballots below see all 64 lanes
  for (long long i0 = (long long)blockIdx.x * TR_THREADS + (threadIdx.x & ~63); i0 < n; i0 += stride) {
    const long long i = i0 + lane;
    unsigned long long bin = TR_NO_BIN;
    if (i < n) {
      const int w = widx[i];
      if (w >= 0) {
        const TrendingWeightDev W = weights[w];
        const long long t = ts[i];
        const long long threshold = (long long)((unsigned long long)now_ms - (unsigned long long)W.window_ms);  // Timestamp.minus: a Long subtraction
        if (t > threshold) {
          const long long day = (now_ms - t) / TR_DAY_MS;   // now is the maximal ts: never negative
          if (day >= W.days) atomicMax(err, (uint32_t)(w + 1));
          else bin = (unsigned long long)(W.day_off + day) * (unsigned long long)items + item[i];
        }
      }
    }
    if (MODE == TRENDING_COUNT_PLAIN) {
      if (bin != TR_NO_BIN) atomicAdd(&table[bin], 1u);
    } else {
      unsigned long long live = __ballot(bin != TR_NO_BIN);
      while (live) {
        const int leader = __ffsll((long long)live) - 1;
        const unsigned lo = (unsigned)__shfl((int)(unsigned)bin, leader, 64), hi = (unsigned)__shfl((int)(unsigned)(bin >> 32), leader, 64);
        const unsigned long long lb = ((unsigned long long)hi << 32) | lo;
        const unsigned long long same = __ballot(bin == lb);   // (a lane without a bin holds TR_NO_BIN: never a leader's)
        if (lane == leader) atomicAdd(&table[lb], (uint32_t)__popcll(same));
        live &= ~same;
      }
    }
  }
}

__global__ void __launch_bounds__(TR_THREADS)
trending_score_kernel(const uint32_t *__restrict__ table, const TrendingWeightDev *__restrict__ weights, int n_weights,
                      const double *__restrict__ pow_table, long long items, double *__restrict__ score) {
  const long long it = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (it >= items) return;
  double total = 0.0;   // (no weights: 0.0)
  for (int w = 0; w < n_weights; ++w) {
    const TrendingWeightDev W = weights[w];
    const uint32_t *col = table + (unsigned long long)W.day_off * (unsigned long long)items + it;
    const double *pw = pow_table + W.day_off;
    double s = 0.0;
    uint32_t any = 0u;
    for (long long d = 0; d < W.days; ++d) {
      const uint32_t c = col[(unsigned long long)d * (unsigned long long)items];
      any |= c;
      s = __dadd_rn(s, __dmul_rn((double)c, pw[d]));
    }
    const double part = any ? __dmul_rn(s, W.weight) : 0.0;
    total = w == 0 ? part : __dadd_rn(total, part);
  }
  score[it] = total;
}

// n <= SORT_MAX_ITEMS (key, index) pairs ordered by ONE workgroup: a bitonic network in LDS on pair_lt, padded to a power of two
// with pairs that sort last
__global__ void __launch_bounds__(1024)
trending_order_kernel(const double *__restrict__ score, int n, int *__restrict__ order) {
  __shared__ unsigned long long s_key[SORT_MAX_ITEMS];
  __shared__ int s_idx[SORT_MAX_ITEMS];
  const int tid = threadIdx.x;
  int p2 = 1;
  while (p2 < n) p2 <<= 1;
  for (int i = tid; i < p2; i += 1024) {
    s_key[i] = i < n ? sort_key(score[i]) : ~0ull;
    s_idx[i] = i < n ? i : 0x7fffffff;
  }
  __syncthreads();
  for (int k = 2; k <= p2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < p2; i += 1024) {
        const int p = i ^ j;
        if (p > i) {
          const unsigned long long ka = s_key[i], kb = s_key[p];
          const int ia = s_idx[i], ib = s_idx[p];
          const bool up = (i & k) == 0;
          if (up ? pair_lt(kb, ib, ka, ia) : pair_lt(ka, ia, kb, ib)) {
            s_key[i] = kb; s_idx[i] = ib;
            s_key[p] = ka; s_idx[p] = ia;
          }
        }
      }
      __syncthreads();
    }
  for (int i = tid; i < n; i += 1024) order[i] = s_idx[i];
}

}  // namespace

void trending_launch_count(mrk_ctx *ctx, hipStream_t s, int mode, const uint32_t *item, const int32_t *widx, const long long *ts, long long n,
                           long long now_ms, const TrendingWeightDev *weights, long long items, uint32_t *table, uint32_t *err) {
  if (n <= 0) return;
  ScopedKernelTimer timer(ctx, "trending_count");
  const long long want = (n + TR_THREADS - 1) / TR_THREADS;
  const int grid = (int)std::min<long long>(want, (long long)std::max(ctx->n_cus, 1) * 16);
  if (mode == TRENDING_COUNT_PLAIN)
    hipLaunchKernelGGL(trending_count_kernel<TRENDING_COUNT_PLAIN>, dim3(grid), dim3(TR_THREADS), 0, s, item, widx, ts, n, now_ms, weights, items, table, err);
  else
    hipLaunchKernelGGL(trending_count_kernel<TRENDING_COUNT_COMBINE>, dim3(grid), dim3(TR_THREADS), 0, s, item, widx, ts, n, now_ms, weights, items, table, err);
  MRK_HIP(hipGetLastError());
}

void trending_launch_score(mrk_ctx *ctx, hipStream_t s, const uint32_t *table, const TrendingWeightDev *weights, int n_weights, const double *pow,
                           long long items, double *score) {
  if (items <= 0) return;
  ScopedKernelTimer timer(ctx, "trending_score");
  const long long grid = (items + TR_THREADS - 1) / TR_THREADS;
  hipLaunchKernelGGL(trending_score_kernel, dim3((unsigned)grid), dim3(TR_THREADS), 0, s, table, weights, n_weights, pow, items, score);
  MRK_HIP(hipGetLastError());
}

size_t trending_order_scratch_bytes(int n) { return n > SORT_MAX_ITEMS ? big_sort_scratch_bytes(n) : 0; }

void trending_launch_order(mrk_ctx *ctx, hipStream_t s, const double *score, int n, int *order, void *scratch) {
  if (n <= 0) return;
  ScopedKernelTimer timer(ctx, "trending_order");
  if (n <= SORT_MAX_ITEMS) {
    hipLaunchKernelGGL(trending_order_kernel, dim3(1), dim3(1024), 0, s, score, n, order);
    MRK_HIP(hipGetLastError());
  } else {
    const SortSrc src{score, nullptr, 1, 1};
    launch_big_sort(ctx, s, src, n, order, scratch);
  }
}

}  // namespace mrk
