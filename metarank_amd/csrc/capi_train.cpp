// C ABI (include/mrk.h) of the LambdaMART fit: LambdaMARTPredictor.makeBooster (ml/rank/LambdaMARTRanker.scala:161-190), both backends.
// Here: the trainer handle, mrk_train_set (argument checks, bins on the host, the tables, the memory budget, the upload in pieces through
// the binning kernel), the second way in - mrk_train_append_device / mrk_train_seal: the matrix staged from DEVICE memory, its cells checked and
// its bins found there (train_bins.hip, step 2d) - and the entry points.  The fit itself - the boosting loop and the two growers - is train_fit.cpp; the kernels are
// train.hip; config, bins, feature subsets, tables, the budget's arithmetic, the tree book-keeping and the model text are train_host.cpp.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <thread>

#include "eval.hpp"
#include "eval_host.hpp"
#include "runtime.hpp"
#include "train.hpp"
#include "train_bins.hpp"
#include "train_fit.hpp"
#include "train_host.hpp"

using namespace mrk;

// rows appended from device memory and not sealed yet (step 2d): column-major pieces, one per mrk_train_append_device
struct StagePiece {
  DevBuf d;                         // [cols][rows] f64
  int64_t row0 = 0;
  int rows = 0;
  const double *column(int c) const { return d.as<double>() + (size_t)c * (size_t)rows; }
};
struct Staging {
  int cols = 0;
  int64_t rows = 0;
  std::vector<StagePiece> pieces;
};

struct mrk_trainer : TrainState {
  std::mutex mu;                    // one set / fit at a time; lock order: mu before ctx->mu
  bool fitted = false;
  Staging stage[2];
};

namespace {

// MRK_TRAIN_PIECE_ROWS: read per call, never on a launch path of the serving side
long long env_int(const char *name, long long dflt) {
  const char *e = getenv(name);
  if (!e || !*e) return dflt;
  char *end = nullptr;
  const long long v = strtoll(e, &end, 10);
  return end && !*end ? v : dflt;
}

// f(c) for every column on up to 8 host threads; the first exception is rethrown
template <typename F>
void for_columns(int cols, F f) {
  const int hw = (int)std::thread::hardware_concurrency();
  const int n = std::max(1, std::min({switches().host_threads > 0 ? switches().host_threads : 8, hw > 0 ? hw : 1, cols}));
  std::atomic<int> next{0};
  std::exception_ptr err;
  std::mutex err_mu;
  auto work = [&] {
    for (int c; (c = next.fetch_add(1)) < cols;) {
      try {
        f(c);
      } catch (...) {
        std::lock_guard<std::mutex> lk(err_mu);
        if (!err) err = std::current_exception();
      }
    }
  };
  std::vector<std::thread> th;
  for (int i = 1; i < n; ++i) th.emplace_back(work);
  work();
  for (auto &t : th) t.join();
  if (err) std::rethrow_exception(err);
}

void check_free(double want, const std::string &what) {
  size_t free_b = 0, total_b = 0;
  MRK_HIP(hipMemGetInfo(&free_b, &total_b));
  if (want > (double)free_b)
    throw StatusError(MRK_ERR_UNSUPPORTED, "train: " + what + " need " + std::to_string((unsigned long long)want) + " bytes on the device, " + std::to_string(free_b) + " are free");
}

// ---- mrk_train_set, one function per step ---------------------------------------------------------------------------------------

EvalShape check_set_args(const mrk_trainer *t, int which, const double *x, int64_t rows, int cols, const int64_t *off, int64_t n_groups) {
  need(which == 0 || which == 1, "train: which is neither 0 (train) nor 1 (validation)");
  need(!t->fitted, "train: the trainer has been fitted");
  need(x != nullptr, "train: null matrix");
  need(rows >= 1 && cols >= 1, "train: rows / cols < 1");
  if (cols > TRAIN_MAX_COLS) throw StatusError(MRK_ERR_UNSUPPORTED, "train: " + std::to_string(cols) + " columns (limit " + std::to_string(TRAIN_MAX_COLS) + ")");
  if (rows >= (int64_t(1) << 31)) throw StatusError(MRK_ERR_UNSUPPORTED, "train: " + std::to_string(rows) + " rows (limit 2^31 - 1)");
  for (int32_t c : t->cfg.categorical)
    if (c >= cols) throw StatusError(MRK_ERR_INVALID_ARG, "train: categorical holds the index " + std::to_string(c) + ", the matrix has " + std::to_string(cols) + " columns");
  const EvalShape sh = eval_check_groups(off, n_groups);
  need(sh.rows == rows, "train: the group offsets do not end at `rows`");
  if (sh.max_len > TRAIN_MAX_GROUP)
    throw StatusError(MRK_ERR_UNSUPPORTED, "train: a group of " + std::to_string(sh.max_len) + " rows (limit " + std::to_string(TRAIN_MAX_GROUP) + ")");
  return sh;
}

// What the backend decides about bins, here and nowhere else in a set: xgboost (step 2x) narrows every cell to f32, finds its bounds
// with train_bin_bounds_f32 and bins with train_launch_bin_f32; lightgbm (steps 2, 2c) finds f64 bounds or, for a categorical column,
// the kept ids, and bins with train_launch_bin.
bool bins_in_f32(const mrk_trainer *t) { return t->cfg.backend == TRAIN_BACKEND_XGBOOST; }

// the training set's column c on the host: its bounds, or its kept category ids
void find_bins(mrk_trainer *t, const double *x, int64_t rows, int c) {
  const size_t k = (size_t)c;
  if (bins_in_f32(t)) t->bounds[k] = train_bin_bounds_f32(x + c, rows, t->cols, t->cfg.max_bin, c);
  else if (t->is_cat[k]) t->kept[k] = train_kept_categories(x + c, rows, t->cols, t->cfg.max_bin, c, &t->infos[k]);
  else t->bounds[k] = train_bin_bounds(x + c, rows, t->cols, t->cfg.max_bin, &t->infos[k]);
}

// the cells of the validation set: what the bin finders refused in the training set is refused here
void check_other_cells(const mrk_trainer *t, const double *x, int64_t rows, int cols) {
  for (int64_t i = 0; i < rows * cols; ++i)
    if (std::isinf(x[i])) throw StatusError(MRK_ERR_INVALID_ARG, "train: cell " + std::to_string(i) + " of the validation matrix is infinite");
  for (int32_t c : t->cfg.categorical) train_check_categories(x + c, rows, cols, c);
  if (bins_in_f32(t)) for_columns(cols, [&](int c) { train_check_f32_cells(x + c, rows, cols, c); });
}

// a piece of the caller's matrix, already in d_x, into the set's column-major bins
void launch_bin_piece(const mrk_trainer *t, hipStream_t st, const double *d_x, const EvalPiece &pc, TrainSet &s) {
  if (bins_in_f32(t)) train_launch_bin_f32(t->ctx, st, d_x, pc.rows, t->cols, t->d_bounds.as<double>(), t->d_bound_off.as<int>(), s.d_bins.as<uint8_t>(), s.rows, pc.row0);
  else
    train_launch_bin(t->ctx, st, d_x, pc.rows, t->cols, t->d_bounds.as<double>(), t->d_bound_off.as<int>(), t->any_cat ? t->d_cat_idx.as<int>() : nullptr,
                     t->any_cat ? t->d_cat_tables.as<uint8_t>() : nullptr, s.d_bins.as<uint8_t>(), s.rows, pc.row0);
}

// a new training set: the trainer's columns start over, the validation set goes
void reset_columns(mrk_trainer *t, int cols) {
  t->set[1] = TrainSet();
  t->cols = cols;
  t->bounds.assign((size_t)cols, {});
  t->infos.assign((size_t)cols, "");
  t->kept.assign((size_t)cols, {});
  t->is_cat.assign((size_t)cols, 0);
  for (int32_t c : t->cfg.categorical) t->is_cat[(size_t)c] = 1;
  t->any_cat = !t->cfg.categorical.empty();
}

void bin_columns_on_host(mrk_trainer *t, const double *x, int64_t rows, int cols) {
  reset_columns(t, cols);
  for_columns(cols, [&](int c) { find_bins(t, x, rows, c); });
}

// bounds, bins per column and the id -> bin tables of the categorical columns, to the device
void upload_tables(mrk_trainer *t, hipStream_t st) {
  const int cols = t->cols;
  std::vector<double> flat;
  std::vector<int> boff((size_t)cols + 1, 0), nbins((size_t)cols);
  for (int c = 0; c < cols; ++c) {
    flat.insert(flat.end(), t->bounds[(size_t)c].begin(), t->bounds[(size_t)c].end());
    boff[(size_t)c + 1] = (int)flat.size();
    nbins[(size_t)c] = t->is_cat[(size_t)c] ? (int)t->kept[(size_t)c].size() : (int)t->bounds[(size_t)c].size() + 1;
  }
  upload(t->d_bounds, flat, st);
  upload(t->d_bound_off, boff, st);
  upload(t->d_nbins, nbins, st);
  upload(t->d_is_cat, t->is_cat, st);
  std::vector<int> cat_idx((size_t)cols * 2, -1);   // per column (offset, length) of its id -> bin table
  std::vector<uint8_t> tables;
  for (int32_t c : t->cfg.categorical) {
    const std::vector<uint8_t> table = train_category_table(t->kept[(size_t)c]);
    cat_idx[(size_t)c * 2] = (int)tables.size(), cat_idx[(size_t)c * 2 + 1] = (int)table.size();
    tables.insert(tables.end(), table.begin(), table.end());
  }
  if (t->any_cat) {
    upload(t->d_cat_idx, cat_idx, st);
    upload(t->d_cat_tables, tables, st);
  }
  MRK_HIP(hipStreamSynchronize(st));   // the vectors are locals
}

// everything the set keeps on the device through the fit (train_fit_bytes), the staging piece and a MiB to spare: there, or refused
void check_budget(const mrk_trainer *t, int which, int64_t rows, int cols, int64_t n_groups, size_t piece_bytes) {
  const bool xgb = t->cfg.backend == TRAIN_BACKEND_XGBOOST;
  const int n_sub = xgb ? cols : (int)train_feature_subset(cols, t->cfg.sampling, 0, 0).size();
  check_free(train_fit_bytes(t->cfg, which, rows, cols, n_groups) + (double)piece_bytes + 1048576.0,
             std::to_string(rows) + " rows x " + std::to_string(cols) + " columns in " + std::to_string(n_groups) + " groups, " +
                 (xgb ? "2 levels x " + std::to_string(train_level_cap(t->cfg, rows)) + " nodes x " : std::to_string(t->cfg.num_leaves) + " leaves x ") + std::to_string(n_sub) +
                 " columns of histograms");
}

void upload_rows_and_groups(TrainSet &s, hipStream_t st);

// the matrix in pieces through the binning kernel, then the labels and the lists of groups
void upload_set(const mrk_trainer *t, TrainSet &s, const double *x, const std::vector<EvalPiece> &pieces, size_t piece_bytes, hipStream_t st) {
  const size_t cols = (size_t)t->cols;
  s.d_bins.reserve((size_t)s.rows * cols);
  DevBuf d_x;
  d_x.reserve(piece_bytes);
  for (const EvalPiece &pc : pieces) {
    MRK_HIP(hipMemcpyAsync(d_x.p, x + (size_t)pc.row0 * cols, (size_t)pc.rows * cols * 8, hipMemcpyHostToDevice, st));
    launch_bin_piece(t, st, d_x.as<double>(), pc, s);
  }
  upload_rows_and_groups(s, st);
  MRK_HIP(hipStreamSynchronize(st));     // the caller's matrix is not kept; d_x goes
}

// the labels and the lists of groups; d_score and d_best are reserved here and first written by the fit
void upload_rows_and_groups(TrainSet &s, hipStream_t st) {
  upload(s.d_labels, s.labels, st);
  upload(s.d_off, s.offsets, st);
  if (!s.by_size.wave.empty()) upload(s.d_wave, s.by_size.wave, st);
  if (!s.by_size.group.empty()) upload(s.d_group, s.by_size.group, st);
  s.d_score.reserve((size_t)s.rows * 8);
  s.d_best.reserve((size_t)s.rows * 8);
}

void set_locked(mrk_trainer *t, int which, const double *x, int64_t rows, int cols, const double *labels, const int64_t *off, int64_t n_groups) {
  const EvalShape sh = check_set_args(t, which, x, rows, cols, off, n_groups);
  t->stage[which] = Staging();   // rows appended from the device and never sealed: gone
  TrainSet &s = t->set[which];
  s = TrainSet();
  s.labels = train_check_labels(labels, rows);
  if (which == 1) {
    need(t->set[0].given, "train: the validation set comes after the training set");
    need(cols == t->cols, "train: the validation set has other columns than the training set");
    s.gains.resize((size_t)rows);
    s.rel.resize((size_t)rows);
    eval_pack_labels(labels, rows, true, s.gains.data(), s.rel.data());
    check_other_cells(t, x, rows, cols);
  } else {
    bin_columns_on_host(t, x, rows, cols);
  }
  s.rows = rows, s.n_groups = n_groups, s.max_len = sh.max_len;
  s.offsets.assign(off, off + n_groups + 1);
  s.by_size = eval_bins(off, n_groups, EVAL_WAVE_ITEMS);

  DeviceLock lk(t->ctx);
  const std::vector<EvalPiece> pieces = eval_pieces(rows, cols, env_int("MRK_TRAIN_PIECE_ROWS", 0));
  const size_t piece_bytes = (size_t)pieces[0].rows * (size_t)cols * 8;
  check_budget(t, which, rows, cols, n_groups, piece_bytes);
  if (which == 0) upload_tables(t, lk.stream);
  upload_set(t, s, x, pieces, piece_bytes, lk.stream);
  drain_profile_events(t->ctx);
  s.given = true;
}

// ---- step 2d: the matrix from device memory (mrk_train_append_device, mrk_train_seal), one function per step ---------------------------

void append_locked(mrk_trainer *t, int which, const double *d_x, int64_t rows, int cols) {
  need(which == 0 || which == 1, "train: which is neither 0 (train) nor 1 (validation)");
  need(!t->fitted, "train: the trainer has been fitted");
  need(d_x != nullptr, "train: null matrix");
  need(rows >= 1 && cols >= 1, "train: rows / cols < 1");
  Staging &sg = t->stage[which];
  need(sg.pieces.empty() || cols == sg.cols, "train: an appended piece has other columns than the pieces before it");
  if (cols > TRAIN_MAX_COLS) throw StatusError(MRK_ERR_UNSUPPORTED, "train: " + std::to_string(cols) + " columns (limit " + std::to_string(TRAIN_MAX_COLS) + ")");
  if (rows >= (int64_t(1) << 31) || sg.rows + rows >= (int64_t(1) << 31))
    throw StatusError(MRK_ERR_UNSUPPORTED, "train: " + std::to_string(sg.rows) + " staged + " + std::to_string(rows) + " appended rows (limit 2^31 - 1)");
  DeviceLock lk(t->ctx);
  const size_t bytes = (size_t)rows * (size_t)cols * 8;
  check_free((double)bytes + 1048576.0, "the staging of " + std::to_string(rows) + " rows x " + std::to_string(cols) + " columns");
  StagePiece pc;
  pc.d.reserve(bytes);
  pc.row0 = sg.rows, pc.rows = (int)rows;
  train_launch_stage(t->ctx, lk.stream, d_x, (int)rows, cols, pc.d.as<double>());
  MRK_HIP(hipStreamSynchronize(lk.stream));   // the caller may rewrite its piece at once
  drain_profile_events(t->ctx);
  sg.cols = cols, sg.rows += rows;
  sg.pieces.push_back(std::move(pc));
}

// the refusals of steps 1, 2x and 2c over the staged cells: the host path's statuses, naming the lowest (column, row) that holds such a cell
void check_staged_cells(const mrk_trainer *t, int which, const Staging &sg, hipStream_t st) {
  std::vector<int> is_cat((size_t)sg.cols, 0);
  for (int32_t c : t->cfg.categorical) is_cat[(size_t)c] = 1;
  DevBuf d_is_cat, d_flags;
  if (!t->cfg.categorical.empty()) upload(d_is_cat, is_cat, st);
  d_flags.reserve(sizeof(TrainCellFlags));
  MRK_HIP(hipMemsetAsync(d_flags.p, 0xFF, sizeof(TrainCellFlags), st));
  for (const StagePiece &pc : sg.pieces)
    train_launch_check_cells(t->ctx, st, pc.d.as<double>(), pc.rows, sg.cols, pc.row0, bins_in_f32(t), t->cfg.categorical.empty() ? nullptr : d_is_cat.as<int>(),
                             d_flags.as<TrainCellFlags>());
  TrainCellFlags f;
  MRK_HIP(hipMemcpyAsync(&f, d_flags.p, sizeof f, hipMemcpyDeviceToHost, st));
  MRK_HIP(hipStreamSynchronize(st));
  auto where = [](unsigned long long at) { return "column " + std::to_string(at >> 32) + ", row " + std::to_string(at & 0xFFFFFFFFull); };
  auto cell = [&](unsigned long long at) {
    const int c = (int)(at >> 32);
    const int64_t r = (int64_t)(at & 0xFFFFFFFFull);
    double v = 0.0;
    for (const StagePiece &pc : sg.pieces)
      if (r >= pc.row0 && r < pc.row0 + pc.rows) MRK_HIP(hipMemcpy(&v, pc.column(c) + (r - pc.row0), 8, hipMemcpyDeviceToHost));
    return train_g17(v);
  };
  const unsigned long long none = ~0ull;
  if (f.infinite != none)
    throw StatusError(MRK_ERR_INVALID_ARG, "train: " + where(f.infinite) + " of the " + (which ? "validation" : "training") + " matrix is infinite");
  if (f.category != none)
    throw StatusError(MRK_ERR_UNSUPPORTED, "train: categorical " + where(f.category) + " holds " + cell(f.category) + " (the largest category is " +
                                               std::to_string(TRAIN_MAX_CATEGORY) + ")");
  if (f.narrow != none) throw StatusError(MRK_ERR_INVALID_ARG, "train: " + where(f.narrow) + " holds " + cell(f.narrow) + ", which is not finite as an f32");
}

// what finding one column's bins needs on the device beside the staging: the keys, the sort's scratch, every column's result, the counts
size_t bin_finder_bytes(const mrk_trainer *t, int64_t rows, int cols) {
  return (size_t)rows * 8 + train_cuts_scratch_bytes(rows) + (size_t)cols * sizeof(TrainColumnCuts) + t->cfg.categorical.size() * (size_t)(TRAIN_MAX_CATEGORY + 1) * 4 + 4096;
}

// steps 2, 2x and 2c of the training set on the device; the few hundred bounds per column (the counts of a categorical one) come back
// for the model writers
void bin_columns_on_device(mrk_trainer *t, const Staging &sg, hipStream_t st) {
  const int cols = sg.cols;
  const int64_t rows = sg.rows;
  const size_t ids = (size_t)TRAIN_MAX_CATEGORY + 1;
  reset_columns(t, cols);
  DevBuf d_keys, d_scratch, d_cuts, d_counts;
  d_keys.reserve((size_t)rows * 8);
  d_scratch.reserve(train_cuts_scratch_bytes(rows));
  d_cuts.reserve((size_t)cols * sizeof(TrainColumnCuts));
  std::vector<int> cat_slot((size_t)cols, -1);
  for (size_t k = 0; k < t->cfg.categorical.size(); ++k) cat_slot[(size_t)t->cfg.categorical[k]] = (int)k;
  if (t->any_cat) {
    d_counts.reserve(t->cfg.categorical.size() * ids * 4);
    MRK_HIP(hipMemsetAsync(d_counts.p, 0, t->cfg.categorical.size() * ids * 4, st));
  }
  for (int c = 0; c < cols; ++c) {
    if (t->is_cat[(size_t)c]) {
      for (const StagePiece &pc : sg.pieces) train_launch_category_counts(t->ctx, st, pc.column(c), pc.rows, d_counts.as<unsigned>() + (size_t)cat_slot[(size_t)c] * ids);
      continue;
    }
    for (const StagePiece &pc : sg.pieces) train_launch_keys(t->ctx, st, pc.column(c), pc.rows, bins_in_f32(t), d_keys.as<unsigned long long>() + pc.row0);
    train_launch_cuts(t->ctx, st, d_keys.as<unsigned long long>(), (int)rows, t->cfg.max_bin, bins_in_f32(t), d_scratch.p, d_cuts.as<TrainColumnCuts>() + c);
  }
  std::vector<TrainColumnCuts> cuts((size_t)cols);
  std::vector<unsigned> counts(t->cfg.categorical.size() * ids);
  MRK_HIP(hipMemcpyAsync(cuts.data(), d_cuts.p, (size_t)cols * sizeof(TrainColumnCuts), hipMemcpyDeviceToHost, st));
  if (t->any_cat) MRK_HIP(hipMemcpyAsync(counts.data(), d_counts.p, counts.size() * 4, hipMemcpyDeviceToHost, st));
  MRK_HIP(hipStreamSynchronize(st));
  for (int c = 0; c < cols; ++c) {
    const size_t k = (size_t)c;
    if (t->is_cat[k]) {
      const unsigned *h = counts.data() + (size_t)cat_slot[k] * ids;
      t->kept[k] = train_kept_from_counts(std::vector<int64_t>(h, h + ids), t->cfg.max_bin, &t->infos[k]);
      continue;
    }
    const TrainColumnCuts &cc = cuts[k];
    if (cc.n_bounds < 0 || cc.n_bounds > TRAIN_MAX_BOUNDS) throw StatusError(MRK_ERR_DEVICE, "train: the bin finder returned " + std::to_string(cc.n_bounds) + " bounds");
    t->bounds[k].assign(cc.bounds, cc.bounds + cc.n_bounds);
    if (!bins_in_f32(t)) t->infos[k] = train_numeric_info(cc.m, cc.lo, cc.hi);
  }
}

void seal_locked(mrk_trainer *t, int which, const double *labels, const int64_t *off, int64_t n_groups) {
  need(which == 0 || which == 1, "train: which is neither 0 (train) nor 1 (validation)");
  need(!t->fitted, "train: the trainer has been fitted");
  need(!t->stage[which].pieces.empty(), "train: nothing was appended to this set");
  // a seal ends the staging whether it succeeds or not: what it refuses, it refuses about these rows
  struct Drop {
    Staging &sg;
    ~Drop() { sg = Staging(); }
  } drop{t->stage[which]};
  const Staging &sg = t->stage[which];
  const int64_t rows = sg.rows;
  const int cols = sg.cols;
  const EvalShape sh = check_set_args(t, which, sg.pieces[0].d.as<double>(), rows, cols, off, n_groups);
  TrainSet &s = t->set[which];
  s = TrainSet();
  s.labels = train_check_labels(labels, rows);
  if (which == 1) {
    need(t->set[0].given, "train: the validation set comes after the training set");
    need(cols == t->cols, "train: the validation set has other columns than the training set");
    s.gains.resize((size_t)rows);
    s.rel.resize((size_t)rows);
    eval_pack_labels(labels, rows, true, s.gains.data(), s.rel.data());
  }
  s.rows = rows, s.n_groups = n_groups, s.max_len = sh.max_len;
  s.offsets.assign(off, off + n_groups + 1);
  s.by_size = eval_bins(off, n_groups, EVAL_WAVE_ITEMS);

  DeviceLock lk(t->ctx);
  hipStream_t st = lk.stream;
  check_budget(t, which, rows, cols, n_groups, which == 0 ? bin_finder_bytes(t, rows, cols) : 4096);
  check_staged_cells(t, which, sg, st);
  if (which == 0) {
    bin_columns_on_device(t, sg, st);
    upload_tables(t, st);
  }
  s.d_bins.reserve((size_t)rows * (size_t)cols);
  for (const StagePiece &pc : sg.pieces)
    train_launch_bin_staged(t->ctx, st, pc.d.as<double>(), pc.rows, cols, bins_in_f32(t), t->d_bounds.as<double>(), t->d_bound_off.as<int>(),
                            t->any_cat ? t->d_cat_idx.as<int>() : nullptr, t->any_cat ? t->d_cat_tables.as<uint8_t>() : nullptr, s.d_bins.as<uint8_t>(), rows, pc.row0);
  upload_rows_and_groups(s, st);
  MRK_HIP(hipStreamSynchronize(st));     // the staging goes
  drain_profile_events(t->ctx);
  s.given = true;
}

void bounds_locked(mrk_trainer *t, int col, double *out, int cap, int *n_bounds) {
  need(t->set[0].given, "train: no training set");
  need(col >= 0 && col < t->cols, "train: no such column");
  need(!t->is_cat[(size_t)col], "train: a categorical column has no bounds");
  const std::vector<double> &b = t->bounds[(size_t)col];
  *n_bounds = (int)b.size();
  if (out && cap >= (int)b.size() && !b.empty()) memcpy(out, b.data(), b.size() * 8);
}

void fit_locked(mrk_trainer *t) {
  need(t->set[0].given, "train: no training set");
  need(!t->fitted, "train: the trainer has been fitted");
  train_fit(*t);
  t->fitted = true;
}

void check_trainer(mrk_trainer *t) { need(t != nullptr, "null trainer"); }

}  // namespace

extern "C" {

int mrk_train_begin(mrk_ctx *ctx, const char *config_json, mrk_trainer **out) {
  return guard([&] {
    need(out != nullptr, "out is null");
    *out = nullptr;
    need(config_json != nullptr, "null config");
    std::unique_ptr<mrk_trainer> t(new mrk_trainer());
    t->cfg = train_parse_config(config_json, strlen(config_json));
    need(ctx != nullptr, "null context");
    ctx_retain(ctx);
    t->ctx = ctx;
    *out = t.release();
  });
}

int mrk_train_set(mrk_trainer *t, int which, const double *rowmajor, int64_t rows, int cols, const double *labels, const int64_t *group_offsets,
                  int64_t n_groups) {
  return guard([&] {
    check_trainer(t);
    std::lock_guard<std::mutex> lk(t->mu);
    set_locked(t, which, rowmajor, rows, cols, labels, group_offsets, n_groups);
  });
}

int mrk_train_append_device(mrk_trainer *t, int which, const double *d_rowmajor, int64_t rows, int cols) {
  return guard([&] {
    need(which == 0 || which == 1, "train: which is neither 0 (train) nor 1 (validation)");   // (judged without a trainer)
    check_trainer(t);
    std::lock_guard<std::mutex> lk(t->mu);
    append_locked(t, which, d_rowmajor, rows, cols);
  });
}

int mrk_train_seal(mrk_trainer *t, int which, const double *labels, const int64_t *group_offsets, int64_t n_groups) {
  return guard([&] {
    need(which == 0 || which == 1, "train: which is neither 0 (train) nor 1 (validation)");
    check_trainer(t);
    std::lock_guard<std::mutex> lk(t->mu);
    seal_locked(t, which, labels, group_offsets, n_groups);
  });
}

int mrk_train_bounds(mrk_trainer *t, int col, double *out_bounds, int cap, int *n_bounds) {
  return guard([&] {
    check_trainer(t);
    need(n_bounds != nullptr, "n_bounds is null");
    std::lock_guard<std::mutex> lk(t->mu);
    bounds_locked(t, col, out_bounds, cap, n_bounds);
  });
}

int mrk_train_fit(mrk_trainer *t) {
  return guard([&] {
    check_trainer(t);
    std::lock_guard<std::mutex> lk(t->mu);
    fit_locked(t);
  });
}

int mrk_train_model(mrk_trainer *t, void *out, size_t cap, size_t *needed) {
  return guard([&] {
    check_trainer(t);
    need(needed != nullptr, "needed is null");
    std::lock_guard<std::mutex> lk(t->mu);
    if (!t->fitted) throw StatusError(MRK_ERR_NOT_FOUND, "train: not fitted yet");
    *needed = t->model.size();
    if (out && cap >= t->model.size()) memcpy(out, t->model.data(), t->model.size());
  });
}

int mrk_train_history(mrk_trainer *t, int *iterations_run, int *best_iteration, double *out_metric, int cap) {
  return guard([&] {
    check_trainer(t);
    std::lock_guard<std::mutex> lk(t->mu);
    if (!t->fitted) throw StatusError(MRK_ERR_NOT_FOUND, "train: not fitted yet");
    if (iterations_run) *iterations_run = t->iterations_run;
    if (best_iteration) *best_iteration = t->best_iteration;
    if (out_metric)
      for (int i = 0; i < cap && i < (int)t->history.size(); ++i) out_metric[i] = t->history[(size_t)i];
  });
}

int mrk_train_scores(mrk_trainer *t, int which, double *out) {
  return guard([&] {
    check_trainer(t);
    need(which == 0 || which == 1, "train: which is neither 0 (train) nor 1 (validation)");
    need(out != nullptr, "out is null");
    std::lock_guard<std::mutex> lk(t->mu);
    if (!t->fitted || !t->set[which].given) throw StatusError(MRK_ERR_NOT_FOUND, "train: no scores of that set");
    memcpy(out, t->set[which].scores.data(), t->set[which].scores.size() * 8);
  });
}

void mrk_train_free(mrk_trainer *t) {
  if (!t) return;
  mrk_ctx *ctx = t->ctx;
  {  // (as mrk_trending_builder_free: the buffers go while nothing of this context runs)
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    delete t;
  }
  ctx_release(ctx);
}

int mrk_train_gradients(mrk_ctx *ctx, const char *config_json, const double *scores, const double *labels, const int64_t *group_offsets, int64_t n_groups,
                        double *out_g, double *out_h) {
  return guard([&] {
    need(config_json != nullptr, "null config");
    const TrainConfig cfg = train_parse_config(config_json, strlen(config_json));
    need(scores != nullptr && out_g != nullptr && out_h != nullptr, "train: null scores / outputs");
    const EvalShape sh = eval_check_groups(group_offsets, n_groups);
    const std::vector<uint8_t> y = train_check_labels(labels, sh.rows);
    for (int64_t i = 0; i < sh.rows; ++i)
      if (!std::isfinite(scores[i])) throw StatusError(MRK_ERR_INVALID_ARG, "train: score " + std::to_string(i) + " is not finite");
    if (sh.max_len > TRAIN_MAX_GROUP)
      throw StatusError(MRK_ERR_UNSUPPORTED, "train: a group of " + std::to_string(sh.max_len) + " rows (limit " + std::to_string(TRAIN_MAX_GROUP) + ")");
    need(ctx != nullptr, "null context");
    const EvalBins by_size = eval_bins(group_offsets, n_groups, EVAL_WAVE_ITEMS);
    DeviceLock lk(ctx);
    hipStream_t st = lk.stream;
    const size_t rows = (size_t)sh.rows;
    check_free(33.0 * (double)rows + 12.0 * (double)n_groups + 16.0 * (double)sh.max_len + 8.0 * TRAIN_SIGMOID_BINS + 65536.0,
               std::to_string(rows) + " rows in " + std::to_string(n_groups) + " groups");
    GradTables tab;
    tab.make(cfg, sh.max_len, st);
    DevBuf d_scores, d_labels, d_off, d_wave, d_group, d_g, d_h;
    d_scores.reserve(rows * 8), d_off.reserve((size_t)(n_groups + 1) * 8), d_g.reserve(rows * 8), d_h.reserve(rows * 8);
    MRK_HIP(hipMemcpyAsync(d_scores.p, scores, rows * 8, hipMemcpyHostToDevice, st));
    MRK_HIP(hipMemcpyAsync(d_off.p, group_offsets, (size_t)(n_groups + 1) * 8, hipMemcpyHostToDevice, st));
    upload(d_labels, y, st);
    if (!by_size.wave.empty()) upload(d_wave, by_size.wave, st);
    if (!by_size.group.empty()) upload(d_group, by_size.group, st);
    GradDev gd = tab.dev(cfg);
    gd.scores = d_scores.as<double>(), gd.labels = d_labels.as<uint8_t>(), gd.offsets = d_off.as<long long>(), gd.g = d_g.as<double>(), gd.h = d_h.as<double>();
    launch_gradients(ctx, st, gd, by_size, d_wave, d_group);
    MRK_HIP(hipMemcpyAsync(out_g, d_g.p, rows * 8, hipMemcpyDeviceToHost, st));
    MRK_HIP(hipMemcpyAsync(out_h, d_h.p, rows * 8, hipMemcpyDeviceToHost, st));
    MRK_HIP(hipStreamSynchronize(st));
    drain_profile_events(ctx);
  });
}

int mrk_train_bins(const char *config_json, const double *column, int64_t n, double *out_bounds, int cap, int *n_bounds) {
  return guard([&] {
    need(config_json != nullptr, "null config");
    const TrainConfig cfg = train_parse_config(config_json, strlen(config_json));
    need(n_bounds != nullptr, "n_bounds is null");
    need(n >= 0 && (column != nullptr || n == 0), "train: null column");
    const std::vector<double> b = cfg.backend == TRAIN_BACKEND_XGBOOST ? train_bin_bounds_f32(column, n, 1, cfg.max_bin, 0) : train_bin_bounds(column, n, 1, cfg.max_bin);
    *n_bounds = (int)b.size();
    if (out_bounds && cap >= (int)b.size() && !b.empty()) memcpy(out_bounds, b.data(), b.size() * 8);
  });
}

int mrk_train_categories(const char *config_json, const double *column, int64_t n, int32_t *out_ids, int cap, int *n_ids) {
  return guard([&] {
    need(config_json != nullptr, "null config");
    const TrainConfig cfg = train_parse_config(config_json, strlen(config_json));
    need(n_ids != nullptr, "n_ids is null");
    need(n >= 0 && (column != nullptr || n == 0), "train: null column");
    const std::vector<int32_t> ids = train_kept_categories(column, n, 1, cfg.max_bin, 0);
    *n_ids = (int)ids.size();
    if (out_ids && cap >= (int)ids.size() && !ids.empty()) memcpy(out_ids, ids.data(), ids.size() * 4);
  });
}

}  // extern "C"
