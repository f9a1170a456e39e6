// Device half of the xgboost backend's EXACT grower (include/mrk.h steps 2e, 5e; train_exact.hip), driven by
// train_fit.cpp (ExactGrower) and capi_train.cpp (the f32 cells and every column's order at mrk_train_set).
// No bins: the f32 matrix stays resident, column-major, and every column keeps a permutation of the row ids ordered by (node segment,
// value, row), NaN last inside a segment.  A node owns the same positions [start, end) in every column.  Per level: prefix sums of
// (q_g, q_h, sampled) over each column's whole permutation - a node's running sum is the global prefix minus the prefix at its start,
// exact in two's complement -, a candidate wherever the value changes inside a node, one read-back, a routing pass over the rows and a
// stable partition of every column's permutation.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "train.hpp"

struct mrk_ctx;

namespace mrk {

constexpr int TRAIN_EXACT_TILE = 1024;       // positions of a column per workgroup of the scan and partition kernels (256 lanes x 4)
constexpr int TRAIN_EXACT_LDS_ROUTES = 64;   // route records of a level the routing kernel holds in LDS (768 B: staged by a workgroup of 256 rows); more are read from memory

struct ExactSums {
  long long g, h, c;
};
struct ExactSeg {
  int start, end;
};
// the best admitted candidate of one node among some positions of one column (valid == 0: none)
struct ExactCand {
  double gain;
  long long gl, hl, cl;   // the left side's sums (with the node's NaN rows when nan_left)
  unsigned code;          // position * 2 + nan_left: the lower one wins a tie
  float bound;            // the value at position + 1: (float) x < bound goes left
  int valid, pad;
};
// a node's best over all columns, and the node's totals.  valid == EXACT_VALID_CAT: a "c" column won - bound is unused and the 8 words
// of its mask over bins (bit b <=> bin b goes RIGHT) stand behind the level's n records, at ((unsigned *) (recs + n)) + slot * 8
constexpr int EXACT_VALID_CAT = 2;
struct ExactRec {
  double gain;
  long long gl, hl, cl;
  long long g, h, c;
  int valid, col, nan_left;
  float bound;
};
// what a row needs to leave a node of the level: col < 0 a leaf (the row stays); else (float) x < bound (NaN when nan_left) goes to node
// `left`, the others to left + 1.  A categorical node (step 5ec) keeps the 12 bytes, as LevelRec does: col = column | TRAIN_LEVEL_CAT |
// index << TRAIN_LEVEL_MASK_SHIFT, the index of its 8-word mask over bins in the level's mask table; a bin whose bit is set goes RIGHT,
// NaN (bin 255) left when nan_left, every other bin - "other", 254, among them - left
struct ExactRoute {
  int col;
  float bound;
  uint16_t left;
  uint8_t nan_left, pad;
};

// ---- mrk_train_set (step 2e) ----
// a piece of the row-major f64 matrix into the column-major f32 matrix: cells[c * rows + row0 + i] = (float) x[i * cols + c], -0.0f as +0.0f
void train_launch_exact_cells(mrk_ctx *ctx, hipStream_t s, const double *x, int piece_rows, int cols, float *cells, long long rows, long long row0);
// bytes of scratch train_launch_exact_order needs for a column of n cells
size_t train_exact_order_scratch_bytes(long long n);
// order[0, n): the rows of one column by (value, row), NaN last - train_bins.hip's keys (asc_key of the cell) under one workgroup's LDS
// bitonic network up to 4096 cells and launch_big_sort above
void train_launch_exact_order(mrk_ctx *ctx, hipStream_t s, const float *col_cells, int n, void *scratch, int *order);

// ---- one level (step 5e) ----
struct ExactDev {
  const float *cells;          // [cols][rows]
  const int *perm;             // [cols][rows]: the level's order
  const uint16_t *node_of;     // per row
  const long long *qg, *qh;    // per row
  long long rows;
  int cols, n_tiles;
  double sampling;
  int seed, tree;
};
struct ExactLevel {
  int first, n;                // the level's nodes: ids first ... first + n - 1, slot k = id - first, ascending with their segments
  int cap;                     // slots per column of nan / base
  const ExactSeg *seg;         // per slot
  ExactSums *tot;              // per slot: the node's sampled totals (the root's is written by the offsets kernel)
  ExactSums *tile;             // [cols][n_tiles]: a tile's total, then the exclusive prefix over the tiles
  ExactSums *nan;              // [cols][cap]: the sampled NaN rows of (column, node); the caller zeroes [cols][cap]
  ExactSums *base;             // [cols][cap]: the prefix before the node's first position
  ExactCand *feat;             // [cap][cols]: a node that lies inside one tile
  ExactCand *edge;             // [cols][n_tiles][2]: the piece of a node that began before the tile (0) / goes on behind it (1)
  ExactRec *recs;              // per slot
};
// The "c" columns of an enable_categorical fit (steps 2ec, 5ec).  Their cells keep their place in the f32 matrix and
// their permutations - ordered by value, equal categories are contiguous inside a node's segment -; beside them the training set holds
// one byte per cell, the bin of step 2cx.  Per level train_exact_cat_sums turns the runs of equal (node, bin) into the level's
// [n_cat][n][256] sums - one integer atomic triple per piece of a run inside a tile, not one per row - and train_exact_cat_scan judges
// them with step 5cx's own body (train_scan_device.hpp).  n_cat == 0: no kernel reads any of this
struct ExactCat {
  int n_cat, first_q;          // first_q: the first "q" column, -1 when every column is a "c"
  const int *cols;             // [n_cat]: the column of every "c" column, ascending
  const int *cat_of;           // [cols]: a column's index among the "c" columns, -1 for a "q" column
  const int *nbins;            // [cols]: a "c" column's kept categories
  const uint8_t *plane;        // [n_cat][rows]: the training cells' bins (254 "other", 255 NaN)
  ExactSums *hist;             // [n_cat][n][256], n the level's nodes; the caller zeroes it
  unsigned *masks;             // [n][n_cat][8]: the right set of every (node, "c" column) candidate
  const int *cat_idx;          // [cols][2] and cat_tables: the id -> bin tables (train_launch_bin_f32's)
  const uint8_t *cat_tables;
};
// plane[j][row] = train_xgb_category_bin of the f32 cell of "c" column j, every row of the set
void train_launch_exact_cat_bins(mrk_ctx *ctx, hipStream_t s, const float *cells, long long rows, const ExactCat &cat, uint8_t *plane);

// the three launches of a level's search and the pick: tile sums, NaN sums and bases; the prefix over the tiles; the candidates; per node
// the best over columns and tiles.  root: the level is node 0 alone and lv.tot[0] is written first.
// cat.n_cat > 0 (step 5ec): the numeric launches leave the "c" columns' workgroups at once; two more launches - the sums of the runs,
// then per (node, "c" column) step 5cx's scan, which writes lv.feat[slot][column] - come before the pick, which reads a "c" column's
// feat record whatever the node spans and copies the winner's mask behind the records
void train_launch_exact_search(mrk_ctx *ctx, hipStream_t s, const ExactDev &d, const ExactLevel &lv, const ScanParams &p, bool root, const ExactCat &cat);

// rows whose node_of is first ... first + n - 1 move to their child under routes[slot]; cells: the set's own f32 matrix.
// n_masks > 0: the level has categorical routes and `masks` holds n_masks x 8 words - the kernel's categorical form is launched: a row's
// bin is train_xgb_category_bin of its f32 cell under the column's table (exact: the cell is the value the table was counted on), so
// the training and the validation rows take one path and no second plane exists; the numeric form reads none of it
void train_launch_exact_route(mrk_ctx *ctx, hipStream_t s, const float *cells, long long rows, uint16_t *node_of, const ExactRoute *routes, int first, int n,
                              const unsigned *masks = nullptr, int n_masks = 0, const int *cat_idx = nullptr, const uint8_t *cat_tables = nullptr);

// the stable partition of every column's permutation after a routing pass: inside the segment of every node that split, the rows that
// went left in order, then the others in order; everything else stays.  next_first / n_next: the children, in pairs (left, right) in
// ascending parent.  Writes next_seg[0, n_next).  par, tcount ([cols][n_tiles]), lbase, lend ([cols][n_next / 2]): scratch
struct ExactPart {
  const ExactRoute *routes;    // the level that split
  const ExactSeg *seg;
  int first, n, next_first, n_next;
  ExactSeg *par, *next_seg;
  unsigned *tcount, *lbase, *lend;
  int *perm_out;
};
void train_launch_exact_partition(mrk_ctx *ctx, hipStream_t s, const ExactDev &d, const ExactPart &pt);

// seg[0] = {0, rows}
void train_launch_exact_begin(mrk_ctx *ctx, hipStream_t s, long long rows, ExactSeg *seg);

}  // namespace mrk
