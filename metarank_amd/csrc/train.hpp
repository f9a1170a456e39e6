// Device half of the LambdaMART fit (train.hip), driven by train_fit.cpp (the fit) and capi_train.cpp (binning, mrk_train_gradients).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

struct mrk_ctx;

namespace mrk {

constexpr int TRAIN_BIN_ROWS = 256;     // rows per workgroup of the binning kernel (one lane per row)
constexpr int TRAIN_HIST_ROWS = 2048;   // rows per workgroup of the histogram kernel (256 lanes x 8 rows)
constexpr int TRAIN_HIST_FEATS = 4;     // columns per workgroup of the histogram kernel: 4 LDS histograms of 256 x (i64, i64, u32) = 20 KiB
constexpr int TRAIN_ROW_THREADS = 256;  // lanes per workgroup of the row-parallel kernels (max, quantise, split, apply)

// what the LambdaRank kernels read and write, in device memory for the whole launch
struct GradDev {
  const double *scores;        // per row
  const uint8_t *labels;       // per row: 0 ... 30
  const long long *offsets;    // n_groups + 1
  const double *lg, *invlg;    // log2(i + 2) and 1 / log2(i + 2), up to the longest group (made on the host)
  const double *sigmoid;       // MRK_TRAIN_SIGMOID_BINS entries (made on the host)
  double lo, f;                // the table's index: clamp((delta - lo) * f)
  double sigma, sigma2;
  int truncation;
  double *g, *h;               // per row
};
// groups[0, count): groups of <= 64 rows, one wavefront each
void train_launch_grad_wave(mrk_ctx *ctx, hipStream_t s, const GradDev &d, const int *groups, int count);
// groups[0, count): groups of <= TRAIN_MAX_GROUP rows (the longest has max_len), one workgroup each
void train_launch_grad_group(mrk_ctx *ctx, hipStream_t s, const GradDev &d, const int *groups, int count, int max_len);

// a piece of the row-major matrix into the column-major byte matrix: bins[c * rows + row0 + i] = the number of bounds of column c
// below x[i * cols + c], or 255 for NaN.  bounds of column c: bounds[bound_off[c] ... bound_off[c + 1]).
// cat_idx (null: no categorical column): per column (offset, length) of its id -> bin table in cat_tables, offset < 0 for a numeric
// column; a cell of a categorical column gets train_category_bin under that table
void train_launch_bin(mrk_ctx *ctx, hipStream_t s, const double *x, int piece_rows, int cols, const double *bounds, const int *bound_off, const int *cat_idx,
                      const uint8_t *cat_tables, uint8_t *bins, long long rows, long long row0);

// maxes[0] = max |g| and maxes[1] = max h as bit patterns (both >= 0: the integer order is the order of the values); the caller zeroes them
void train_launch_max(mrk_ctx *ctx, hipStream_t s, const double *g, const double *h, long long rows, unsigned long long *maxes);
// q = (int64) rint(ldexp(v, e)); leaf_of = 0
void train_launch_quantise(mrk_ctx *ctx, hipStream_t s, const double *g, const double *h, long long rows, int e_g, int e_h, long long *qg, long long *qh,
                           uint16_t *leaf_of);

// a (leaf, subset column, bin) histogram: G and H int64, C uint32, each [leaf][n_sub][256]
struct HistDev {
  long long *G, *H;
  unsigned *C;
  int n_sub;
};
// zeroes slot `slot` and adds the rows of `leaf` to it
void train_launch_hist(mrk_ctx *ctx, hipStream_t s, const uint8_t *bins, long long rows, const uint16_t *leaf_of, int leaf, int slot, const long long *qg,
                       const long long *qh, const int *subset, const HistDev &hd);

// the best admitted candidate of a leaf (valid == 0: none) and the leaf's totals
struct LeafRec {
  double gain;
  int valid, col, bin, nan_left;
  long long gl, hl, cl;        // the left side's sums
  long long g, h, c;           // the leaf's
  int is_cat;                  // a categorical candidate: cat_mask bit b <=> bin b goes left (bin, nan_left unused)
  unsigned cat_mask[8];
};
struct ScanParams {
  int e_g, e_h;
  int min_data;
  double min_hess, l2;
  // step 5c
  int max_onehot, max_cat_threshold, min_data_cat;   // min_data_cat = max(min_data_in_leaf, min_data_per_group)
  double cat_smooth, l2_cat;                         // l2_cat = lambda_l2 + cat_l2
  double min_gain;                                   // a numeric candidate is admitted when gain > min_gain: 0 (step 5), gamma (step 5x)
};
// leaf_b < 0: scans leaf_a alone (the root).  Else slot leaf_b holds the histogram of the smaller child of a split and slot leaf_a its
// parent's: first leaves both slots with their own leaf's (sibling = parent - small; leaf_a is the left child), then scans both.
// feat_best: scratch of 2 * n_sub records; out: 2 records (leaf_a, leaf_b).  nbins / is_cat: per column; a categorical column is
// searched by step 5c
void train_launch_scan(mrk_ctx *ctx, hipStream_t s, const HistDev &hd, const int *subset, const int *nbins, const int *is_cat, int leaf_a, int leaf_b,
                       bool small_is_left, const ScanParams &p, LeafRec *feat_best, LeafRec *out);

// rows of `leaf` whose bin of column `col` goes right move to leaf `fresh`
void train_launch_split(mrk_ctx *ctx, hipStream_t s, const uint8_t *col_bins, long long rows, uint16_t *leaf_of, int leaf, int fresh, int bin, int nan_left);
// the same for a categorical node: a bin goes left when it is not 255 and its bit of the mask is set
struct CatMask {
  unsigned w[8];
};
void train_launch_split_cat(mrk_ctx *ctx, hipStream_t s, const uint8_t *col_bins, long long rows, uint16_t *leaf_of, int leaf, int fresh, const CatMask &mask);

// a finished tree on the device: per internal node (column, bin, nan_left, left, right), children as in the model text (~leaf).
// is_cat (null: a tree without a categorical node): per node, and cat_mask 8 words per node
struct TreeDev {
  const int *col, *bin, *nan_left, *left, *right;
  const double *leaf_value;
  const int *is_cat;
  const unsigned *cat_mask;
};
// scores[row] += leaf_value[leaf]: leaf_of given (the training rows) or found by walking the tree over the rows' bins (validation)
void train_launch_apply(mrk_ctx *ctx, hipStream_t s, const TreeDev &t, const uint16_t *leaf_of, const uint8_t *bins, long long rows, double *scores);

// ---- the xgboost backend: a LEVEL-wise grower (include/mrk.h steps 2x, 5x, 6x, 7x) ---------------------------------------------------
// Per level one histogram launch for every node of the level that is built, one scan launch for every node of the level, one routing
// pass.  Per row two u16: node_of, the row's node in XGBoost's breadth-first numbering (the nodes of one depth have consecutive ids, so
// the slot of a node within its level is id - first id of the level), and hist_slot, the index of the row's node among the level's
// BUILT nodes - TRAIN_NO_SLOT when the node is not built (a leaf, the sibling that comes from parent - built child, a node at maxDepth)
// or the row is outside the tree's sample (step 7x): such a row adds nothing to a histogram and is routed all the same.
constexpr int TRAIN_LEVEL_ROWS = 8192;        // rows per workgroup of the level histogram kernel (256 lanes x 32 rows): zeroing and flushing 40 KiB of LDS is paid per tile
constexpr int TRAIN_LEVEL_CHUNK = 8;          // built nodes per workgroup of the level histogram kernel: 8 x 256 x 20 B = 40 KiB of LDS
constexpr int TRAIN_LEVEL_LDS_RECS = 1024;    // split records of a level the routing kernel holds in LDS (12 KiB); more are read from memory
constexpr unsigned TRAIN_NO_SLOT = 0xFFFFu;

// as train_launch_bin for step 2x: the cell is narrowed to f32, its bin is the number of bounds (f32 values widened) <= it
void train_launch_bin_f32(mrk_ctx *ctx, hipStream_t s, const double *x, int piece_rows, int cols, const double *bounds, const int *bound_off, uint8_t *bins,
                          long long rows, long long row0);

// node_of = 0; hist_slot = 0 for a row of tree `tree`'s sample, TRAIN_NO_SLOT for the others
void train_launch_level_begin(mrk_ctx *ctx, hipStream_t s, long long rows, double sampling, int seed, int tree, uint16_t *node_of, uint16_t *hist_slot);

// zeroes nothing: the caller has zeroed the level's slots.  Adds every row with hist_slot = b < n_build to histogram slot build_slot[b]
// of all `hd.n_sub` (= all) columns.  Grid: (row tiles of TRAIN_LEVEL_ROWS, columns, chunks of TRAIN_LEVEL_CHUNK built nodes)
void train_launch_level_hist(mrk_ctx *ctx, hipStream_t s, const uint8_t *bins, long long rows, const uint16_t *hist_slot, const long long *qg, const long long *qh,
                             const int *build_slot, int n_build, const HistDev &hd);

// a node of the level for the scan: its histogram slot; parent_slot >= 0: the slot is first filled with parent - sibling
struct LevelNode {
  int slot, parent_slot, sibling_slot;
};
// per (node, column) scan_column under ScanParams (step 5x: min_data 1, min_hess min_child_weight, l2 lambda, min_gain gamma), then per
// node the best column.  feat_best: scratch of n_nodes * hd.n_sub records; out: n_nodes records
void train_launch_level_scan(mrk_ctx *ctx, hipStream_t s, const HistDev &hd, const int *nbins, const LevelNode *nodes, int n_nodes, const ScanParams &p,
                             LeafRec *feat_best, LeafRec *out);

// what a row needs to leave a node of the level: col < 0 a leaf (the row stays); else bin <= `bin` (NaN when nan_left) goes to node
// `left`, the others to left + 1; slot_l / slot_r: the children's index among the next level's built nodes or TRAIN_NO_SLOT
struct LevelRec {
  int col;
  uint16_t left, slot_l, slot_r;
  uint8_t bin, nan_left;
};
// rows whose node_of is first ... first + n - 1 move to their child.  hist_slot null: routing alone (the validation rows)
void train_launch_level_split(mrk_ctx *ctx, hipStream_t s, const uint8_t *bins, long long rows, uint16_t *node_of, uint16_t *hist_slot, const LevelRec *recs, int first,
                              int n, double sampling, int seed, int tree);

// step 6x: scores[row] = (double) ((float) scores[row] + value[node_of[row]])
void train_launch_level_apply(mrk_ctx *ctx, hipStream_t s, const float *value, const uint16_t *node_of, long long rows, double *scores);
// scores[row] = 0.5 (the base_score)
void train_launch_level_base(mrk_ctx *ctx, hipStream_t s, long long rows, double *scores);

}  // namespace mrk
