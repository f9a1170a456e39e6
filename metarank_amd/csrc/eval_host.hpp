// Host half of the ranking evaluation (capi_eval.cpp): everything of LambdaMARTModel.eval that is not a sort or an ordered
// sum.  No HIP in here: tests/native/eval_host_test.cpp compiles this file with g++ alone.
// Reference: ml/rank/LambdaMARTRanker.scala:115-123 (the call that ends a train), :406-445 (eval, noopArray, randomArray).
// ltrlib's metric sources are not in the reference tree: the formulas are this project's (include/mrk.h).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "status.hpp"

namespace mrk {

constexpr int EVAL_WAVE_ITEMS = 64;                        // groups of up to this many items: one wavefront each
constexpr int EVAL_GROUP_ITEMS = 4096;                     // ... up to this many (SORT_MAX_ITEMS): one workgroup each; beyond: bigsort.hip
constexpr int64_t EVAL_MAX_GROUP = int64_t(1) << 30;       // items of one group (the sorts index with int)
constexpr int64_t EVAL_MAX_GROUPS = (int64_t(1) << 31) - 1;   // groups of one call (the index lists are int32)
constexpr int64_t EVAL_PIECE_BYTES = int64_t(64) << 20;    // of the feature matrix per upload

// an unknown metric, a negative cutoff, a null array or n_metrics < 1: MRK_ERR_INVALID_ARG
void eval_check_metrics(const int *metrics, const int *cutoffs, int n_metrics);

struct EvalShape {
  int64_t rows = 0;      // group_offsets[n_groups]
  int64_t max_len = 0;   // the longest group
};
// MRK_ERR_INVALID_ARG: null offsets, n_groups < 1, offsets that do not start at 0 or do not strictly increase (an empty group;
// a sequence that wrapped around is one that does not increase); MRK_ERR_UNSUPPORTED: more than EVAL_MAX_GROUPS groups or a
// group of more than EVAL_MAX_GROUP items
EvalShape eval_check_groups(const int64_t *group_offsets, int64_t n_groups);

// gains[i] = labels[i], or pow(2.0, labels[i]) - 1.0 (libm's pow) with relpow; rel[i] = labels[i] > 0.
// A null array or a non-finite label: MRK_ERR_INVALID_ARG with nothing promised about the outputs.
void eval_pack_labels(const double *labels, int64_t rows, bool relpow, double *gains, uint8_t *rel);

// lg[i] = log2(i + 2) (libm's log2), i < n
std::vector<double> eval_lg_table(int64_t n);

// noopArray of every group back to back: out[offsets[g] + i] = (len - i) / (double)len.  Strictly decreasing inside a group, so
// its order is the identity: mrk_model_eval sorts nothing for it.  Here as the definition the tests hold that shortcut against.
void eval_noop_array(const int64_t *group_offsets, int64_t n_groups, double *out);

// the groups by kernel, each list in group order
struct EvalBins {
  std::vector<int32_t> wave, group, big;
  int64_t group_max_len = 0;   // the longest group of `group`
};
// wave_max: the longest group the wavefront kernel takes, clamped to [0, EVAL_WAVE_ITEMS]
EvalBins eval_bins(const int64_t *group_offsets, int64_t n_groups, int wave_max);

// the rows of the feature matrix in upload pieces of at most piece_rows rows (<= 0: what EVAL_PIECE_BYTES hold, at least one row);
// a piece never exceeds INT32_MAX rows (the scorer counts rows with int).  Groups are not looked at: scoring is per row.
struct EvalPiece {
  int64_t row0;
  int32_t rows;
};
std::vector<EvalPiece> eval_pieces(int64_t rows, int cols, int64_t piece_rows);

// the sequential f64 sum of v[0 .. n) in index order, divided by n
double eval_mean(const double *v, int64_t n);

}  // namespace mrk
