// Device half of the ranking evaluation (eval.hip), driven by capi_eval.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

struct mrk_ctx;

namespace mrk {

// what the kernels of one call read and write, all in device memory for the whole call
struct EvalDev {
  const double *scores;        // per row; nullptr: the order of every group is the identity (noopArray, strictly decreasing)
  const double *gains;         // per row: the label, or 2^label - 1 (made on the host)
  const uint8_t *rel;          // per row: label > 0
  const long long *offsets;    // n_groups + 1
  const double *lg;            // lg[i] = log2(i + 2), up to the longest group (made on the host)
  const int *metrics, *cutoffs;
  int n_metrics;
  int need_ideal;              // any metric is NDCG
  double nolabels;
  long long n_groups;
  double *out;                 // [n_metrics][n_groups]: a group's values land at its own index
};

// groups[0, count): groups of <= EVAL_WAVE_ITEMS items, one wavefront each
void eval_launch_wave(mrk_ctx *ctx, hipStream_t s, const EvalDev &d, const int *groups, int count);
// groups[0, count): groups of <= EVAL_GROUP_ITEMS items (the longest has max_len), one workgroup each
void eval_launch_group(mrk_ctx *ctx, hipStream_t s, const EvalDev &d, const int *groups, int count, int max_len);
// one group of n > EVAL_GROUP_ITEMS items starting at row `base`
size_t eval_big_scratch_bytes(int n);
void eval_launch_big(mrk_ctx *ctx, hipStream_t s, const EvalDev &d, int group, long long base, int n, void *scratch);

}  // namespace mrk
