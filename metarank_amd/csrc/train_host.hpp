// Host half of the LambdaMART fit (train_fit.cpp, capi_train.cpp; the algorithm: include/mrk.h): config, bins, feature
// subsets, the sigmoid table, the quantisation exponents, the memory budget, the tree book-keeping and the model text.  No HIP in here:
// tests/native/train_host_test.cpp compiles this file with g++ alone.
// Reference: LambdaMARTPredictor.makeBooster (ml/rank/LambdaMARTRanker.scala:161-190), LightGBMConfig (config/BoosterConfig.scala:19-28).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "status.hpp"

namespace mrk {

constexpr int TRAIN_SIGMOID_BINS = MRK_TRAIN_SIGMOID_BINS;
constexpr int TRAIN_NAN_BIN = 255;          // the bin of a NaN cell; a column has at most 254 others
constexpr int TRAIN_MAX_GROUP = 4096;       // rows of one group (one workgroup orders it: EVAL_GROUP_ITEMS)
constexpr int TRAIN_MAX_COLS = 65535;
constexpr int TRAIN_MAX_LEAVES = 4096;
constexpr int TRAIN_MAX_LABEL = 30;
constexpr int TRAIN_MAX_CATEGORY = 32764;   // 0x7FFC: the largest id the scorers' categorical cell holds exactly (forest.hpp, QV_CAT)

#ifdef __HIPCC__
#define MRK_TRAIN_HD __host__ __device__
#else
#define MRK_TRAIN_HD
#endif

struct TrainConfig {
  int iterations = 100;
  double learning_rate = 0.1;
  int ndcg_cutoff = 10;
  int max_depth = 8;
  int seed = 0;
  int num_leaves = 16;
  double sampling = 0.8;
  bool debias = false;
  int max_bin = 255;
  int truncation = 30;
  double sigma = 1.0;
  int min_data_in_leaf = 20;
  double min_sum_hessian = 1e-3;
  double lambda_l2 = 0.0;
  int early_stopping = 20;
  std::vector<int32_t> categorical;   // column indices, distinct, >= 0 (below `cols`: judged by mrk_train_set)
  int max_cat_to_onehot = 4;
  int max_cat_threshold = 32;
  double cat_smooth = 10.0;
  double cat_l2 = 10.0;
  int min_data_per_group = 100;
  int backend = 0;                    // "backend": 0 "lightgbm" (steps 2, 5, 6, 7), 1 "xgboost" (steps 2x, 5x, 6x, 7x)
  double lambda = 1.0;                // the three keys of the xgboost backend alone
  double gamma = 0.0;
  double min_child_weight = 1.0;
};
constexpr int TRAIN_BACKEND_LIGHTGBM = 0, TRAIN_BACKEND_XGBOOST = 1;
constexpr int TRAIN_XGB_MAX_DEPTH = 15;     // a node id is a u16: a complete tree of depth 15 has 65535 nodes
// malformed JSON, a value of the wrong type or an unknown key: MRK_ERR_PARSE; a value out of range: MRK_ERR_INVALID_ARG;
// debias = true or numLeaves > TRAIN_MAX_LEAVES: MRK_ERR_UNSUPPORTED.  backend "xgboost": numLeaves, min_data_in_leaf,
// min_sum_hessian, lambda_l2 and the categorical keys but `categorical` are MRK_ERR_INVALID_ARG naming the key, a non-empty
// `categorical` is MRK_ERR_UNSUPPORTED; backend "lightgbm": lambda, gamma and min_child_weight are MRK_ERR_INVALID_ARG
TrainConfig train_parse_config(const char *json, size_t len);

// the upper bounds of the bins of one column but the last (bin(x) = the number of bounds < x), from col[i * stride], i < n.
// An infinite cell: MRK_ERR_INVALID_ARG.  info: LightGBM's feature_infos entry ("none" or "[min:max]").
std::vector<double> train_bin_bounds(const double *col, int64_t n, int64_t stride, int max_bin, std::string *info = nullptr);

// the feature_infos entry of a numeric column with m non-NaN values, the least lo and the greatest hi
std::string train_numeric_info(int64_t m, double lo, double hi);
// %.17g
std::string train_g17(double x);

// step 2x: the bounds of one column for the xgboost backend, f32 values widened to f64: the cells are narrowed to f32 first, the bound
// between neighbours a < b is b (bin(x) = the number of bounds <= (float) x, so x < bound goes left: the model's own test).  A finite
// cell that narrows to +-inf, or an infinite one: MRK_ERR_INVALID_ARG naming `column` and the row.
std::vector<double> train_bin_bounds_f32(const double *col, int64_t n, int64_t stride, int max_bin, int column);
// the cells of another set than the one the bounds came from: the same refusal
void train_check_f32_cells(const double *col, int64_t n, int64_t stride, int column);
// bin(x) of step 2x on the host (the device's is train.hip's): NaN is TRAIN_NAN_BIN
int train_bin_f32(double x, const double *bounds, int n_bounds);

// step 2c: the category ids of a categorical column that get a bin, ascending (the bin of an id is its position): the
// min(distinct, max_bin - 1) most frequent of col[i * stride], i < n, ties to the lower id.  The category of a cell is trunc(x); NaN and
// negative ones have none.  An infinite cell: MRK_ERR_INVALID_ARG; a category beyond TRAIN_MAX_CATEGORY: MRK_ERR_UNSUPPORTED, naming
// `column`, the row and the value.  info: LightGBM's feature_infos entry (the ids joined by ':', or "none").
std::vector<int32_t> train_kept_categories(const double *col, int64_t n, int64_t stride, int max_bin, int column, std::string *info = nullptr);
// the tail of step 2c, from the count of every id 0 ... TRAIN_MAX_CATEGORY (TRAIN_MAX_CATEGORY + 1 counts: the device's histogram too)
std::vector<int32_t> train_kept_from_counts(const std::vector<int64_t> &count, int max_bin, std::string *info = nullptr);
// the cells of a categorical column of another set than the one the ids were kept from: the same two refusals
void train_check_categories(const double *col, int64_t n, int64_t stride, int column);
// id -> bin for ids 0 ... kept.back(), TRAIN_NAN_BIN where the id has none; empty without a kept id
std::vector<uint8_t> train_category_table(const std::vector<int32_t> &kept);
// the bin of a cell of a categorical column under a table of `len` bytes: NaN, a negative category and an id without a bin are
// TRAIN_NAN_BIN (which always goes right: what CategoricalDecision does with them).  The binning kernel calls this too.
MRK_TRAIN_HD inline int train_category_bin(double x, const uint8_t *table, int len) {
  if (!(x > -1.0) || !(x < (double)len)) return TRAIN_NAN_BIN;   // (NaN fails both; -1 < x < 0 truncates to category 0)
  return table[(int)x];
}

// Steps 2 and 2x over values that are ALREADY sorted (step 2d: the device's bin finder, train_bins.hip; tests/native/train_cuts_test.cpp
// holds it against train_bin_bounds on the unsorted cells).  v(p), 0 <= p < m: the sorted non-NaN values as f64 (an f32 value
// widened, f32 = true).  Returns the first position p >= max(t, 1) with v(p) != v(p - 1) - the cut bin_cuts takes for the target t -
// or m when there is none, and writes the bound between v(p - 1) and v(p).  Over a sorted array that position is t itself when
// v(t) != v(t - 1), else the first index that holds a value above v(t): one binary search.
// The targets: with at most max_bin - 2 changes every change is a cut (t = the change itself, or the cut before it + 1); else
// t = train_cut_target(m, max_bin, i) for i = 1 ... max_bin - 2, up to the first i without a cut, a cut equal to the one before dropped.
MRK_TRAIN_HD inline int64_t train_cut_target(int64_t m, int max_bin, int i) { return (int64_t)i * m / (max_bin - 1); }
template <typename V>
MRK_TRAIN_HD inline int64_t train_cut_at(const V &v, int64_t m, int64_t t, bool f32, double *bound) {
  if (t < 1) t = 1;
  if (t >= m) return m;
  int64_t p = t;
  const double x = v(t);
  if (!(v(t - 1) != x)) {
    int64_t lo = t + 1, hi = m;   // the first index in (t, m) whose value is above x, m when none is
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (v(mid) > x) hi = mid;
      else lo = mid + 1;
    }
    if (lo >= m) return m;
    p = lo;
  }
  const double a = v(p - 1), b = v(p);
  double mid = (a + b) / 2.0;
  if (!(mid < b)) mid = a;   // (also a sum that overflowed)
  *bound = f32 ? b : mid;
  return p;
}

// step 7x: is row `row` in the sample of tree `tree`?  The histogram kernels call this too.
MRK_TRAIN_HD inline bool train_row_sampled(double sampling, int seed, int tree, uint64_t row) {
  if (sampling >= 1.0) return true;
  uint64_t z = ((((uint64_t)(uint32_t)seed << 32) | (uint64_t)(uint32_t)tree) ^ (row * 0xD6E8FEB86659FD93ull)) + 0x9E3779B97F4A7C15ull;   // splitmix64's first output
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) * 0x1.0p-53 < sampling;   // (53 bits: the conversion and the product are exact)
}

// the columns of tree `tree`, ascending
std::vector<int32_t> train_feature_subset(int cols, double sampling, int seed, int tree);

constexpr int TRAIN_LEAF_REC_BYTES = 112;   // sizeof(LeafRec) (train.hpp: no HIP in here; train_fit.hpp asserts the two agree)
// backend "xgboost": the most nodes of one level that is scanned (depth < maxDepth; every node holds a sampled row)
int64_t train_level_cap(const TrainConfig &cfg, int64_t rows);
// the device memory a set of that shape holds through the fit (which: 0 training, 1 validation), in bytes: what mrk_train_set asks
// the device for before it uploads anything.  The training set's figure includes the buffers of the backend's grower
double train_fit_bytes(const TrainConfig &cfg, int which, int64_t rows, int cols, int64_t n_groups);

struct SigmoidTable {
  double lo, f;
  std::vector<double> t;
};
SigmoidTable train_sigmoid_table(double sigma);

// 61 - bitlen(rows) - E(vmax), frexp(vmax) = m * 2^E; 0 for vmax == 0
int train_exponent(double vmax, int64_t rows);

// integers 0 ... TRAIN_MAX_LABEL or MRK_ERR_INVALID_ARG
std::vector<uint8_t> train_check_labels(const double *labels, int64_t rows);

struct TrainSums {
  int64_t g = 0, h = 0;
  int64_t c = 0;
};

// one tree in LightGBM's numbering: the s-th split makes internal node s, its left child keeps the leaf index, its right child is leaf s + 1
struct TrainTree {
  std::vector<int32_t> feat, bin, dt, left, right;
  std::vector<double> gain, thr, ivalue, iweight;
  std::vector<int64_t> icount;
  std::vector<int32_t> parent_node, parent_side, depth;   // per leaf
  std::vector<double> value, weight;                      // per leaf
  std::vector<int64_t> count;
  std::vector<int32_t> is_cat;                            // per node
  std::vector<uint32_t> cat_mask;                         // per node 8 words: bit b <=> bin b goes left (zeros for a numeric node)
  TrainTree() : parent_node{-1}, parent_side{0}, depth{0} {}
  int num_leaves() const { return (int)feat.size() + 1; }
  int num_cat() const;
  int split(int leaf, int col, int b, double thr_, bool nan_left, double gain_);   // -> the new leaf
  // a categorical node: threshold = its ordinal among the tree's categorical nodes, decision_type = 9 (categorical, missing type NaN)
  int split_cat(int leaf, int col, const uint32_t *mask8, double gain_);
};

// -G / (H + l2) * lr of quantised sums; *weight: H
double train_leaf_output(const TrainSums &q, int e_g, int e_h, double l2, double lr, double *weight);

// kept: per column the kept ids of step 2c (empty for a numeric column), needed when a tree has a categorical node: its bins go back
// to ids, a node's bitset has max member id / 32 + 1 words.  A tree without one is written as before (num_cat=0, no cat_* lines).
std::string train_write_model(const std::vector<TrainTree> &trees, size_t n_trees, int cols, const std::vector<std::string> &infos, double lr,
                              const std::vector<std::vector<int32_t>> *kept = nullptr);

// one tree of the xgboost backend in XGBoost's breadth-first numbering (step 5x): node 0 is the root, a node that splits gives its
// children the next two free ids.  cond: the bound of a split node, (float)(weight * learningRate) of a leaf.
struct TrainXgbTree {
  std::vector<int32_t> left, right, parent, col, bin, default_left;   // left / right -1 for a leaf; parent 2147483647 for the root
  std::vector<float> cond, base_weight, loss_change, sum_hessian;
  int num_nodes() const { return (int)left.size(); }
  int add(int parent_);                                             // a new leaf -> its id
  void split(int node, int col_, int bin_, float bound, bool nan_left, float gain);   // -> children num_nodes() - 2, num_nodes() - 1
  // weight = -G / (H + lambda) of a node's quantised sums into base_weight / sum_hessian; a leaf's cond = (float)(weight * lr).
  // H + lambda == 0 (no finite weight): MRK_ERR_INVALID_ARG
  void weigh(int node, const TrainSums &q, int e_g, int e_h, double lambda, double lr);
};
// XGBoost's JSON (version [2,1,0], objective rank:ndcg, base_score 5E-1), no whitespace; every f32 as %.9g of its widened value
std::string train_write_xgb_model(const std::vector<TrainXgbTree> &trees, size_t n_trees, int cols);

}  // namespace mrk
