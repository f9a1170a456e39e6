// Device half of the trending recommender's fit (trending.hip), driven by capi_trending.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

struct mrk_ctx;

namespace mrk {

// one InteractionWeight as the kernels read it
struct TrendingWeightDev {
  long long window_ms;   // window.toMillis
  long long days;        // window.toDays: the weight's count array has this many buckets
  long long day_off;     // its first row of the [weight][day][item] count table = its first entry of the pow table
  double weight;
};

// how trending_count_kernel adds to a bin: equal bins of a wavefront combined into one atomic (the default), or one atomic
// per interaction (MRK_TRENDING_COUNT=plain: the A/B of DESIGN 15)
enum TrendingCountMode { TRENDING_COUNT_COMBINE = 0, TRENDING_COUNT_PLAIN = 1 };

// table ([total days][items] u32, zeroed) += the interactions rule 3 counts; *err = max(weight index + 1) of an interaction
// whose day bucket lies outside its weight's array
void trending_launch_count(mrk_ctx *ctx, hipStream_t s, int mode, const uint32_t *item, const int32_t *widx, const long long *ts, long long n,
                           long long now_ms, const TrendingWeightDev *weights, long long items, uint32_t *table, uint32_t *err);
// score[item] by rules 4 and 6
void trending_launch_score(mrk_ctx *ctx, hipStream_t s, const uint32_t *table, const TrendingWeightDev *weights, int n_weights, const double *pow,
                           long long items, double *score);
// order[0, n): the items in the order of sortBy(-score), ties by ascending item index
size_t trending_order_scratch_bytes(int n);
void trending_launch_order(mrk_ctx *ctx, hipStream_t s, const double *score, int n, int *order, void *scratch);

}  // namespace mrk
