// The LambdaMART fit behind mrk_train_fit (include/mrk.h): one boosting loop (train_fit) over one of two growers -
// LeafGrower, LightGBM's leaf-wise tree (per split one histogram launch, one scan, two records read back), and LevelGrower, XGBoost's
// level-wise tree (per level one histogram launch, one scan, the level's records read back once).  The kernels are train.hip, the
// host half train_host.cpp; capi_train.cpp holds the trainer handle, mrk_train_set and the C ABI.
#pragma once
#include <string>
#include <vector>

#include "eval_host.hpp"
#include "runtime.hpp"
#include "train.hpp"
#include "train_host.hpp"

namespace mrk {

static_assert(sizeof(LeafRec) == TRAIN_LEAF_REC_BYTES, "train_fit_bytes (train_host.cpp) counts a LeafRec as TRAIN_LEAF_REC_BYTES");

struct TrainSet {
  bool given = false;
  int64_t rows = 0, n_groups = 0, max_len = 0;
  std::vector<uint8_t> labels;
  std::vector<int64_t> offsets;
  EvalBins by_size;
  DevBuf d_bins, d_labels, d_off, d_wave, d_group, d_score, d_best;   // d_score, d_best: reserved by mrk_train_set, first written by train_fit
  std::vector<double> gains;        // the validation set: what eval.hip reads (eval_pack_labels, relpow)
  std::vector<uint8_t> rel;
  std::vector<double> scores;       // at the best iteration, after the fit
};

// everything of a trainer that the fit reads (what mrk_train_set left) and writes (model ... iterations_run)
struct TrainState {
  mrk_ctx *ctx = nullptr;
  TrainConfig cfg;
  int cols = 0;
  std::vector<std::vector<double>> bounds;
  std::vector<std::string> infos;
  std::vector<std::vector<int32_t>> kept;   // step 2c: per categorical column its kept ids (a numeric column: empty)
  std::vector<int32_t> is_cat;              // per column
  bool any_cat = false;
  DevBuf d_bounds, d_bound_off, d_nbins, d_is_cat, d_cat_idx, d_cat_tables;
  TrainSet set[2];
  int iterations_run = 0;
  std::vector<double> history;
  int best_iteration = 0;
  std::string model;
};

// the tables of step 3 on the device
struct GradTables {
  DevBuf d_lg, d_invlg, d_sigmoid;
  SigmoidTable sig;
  void make(const TrainConfig &cfg, int64_t max_len, hipStream_t st);
  GradDev dev(const TrainConfig &cfg) const;
};
void launch_gradients(mrk_ctx *ctx, hipStream_t st, const GradDev &d, const EvalBins &by_size, const DevBuf &d_wave, const DevBuf &d_group);

// The caller holds nothing of t.ctx: its lock is taken here, per iteration.  t.set[0] is given.
void train_fit(TrainState &t);

}  // namespace mrk
