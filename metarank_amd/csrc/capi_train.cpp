// C ABI (include/mrk.h) of the LambdaMART fit: LambdaMARTPredictor.makeBooster (ml/rank/LambdaMARTRanker.scala:161-190) for the
// LightGBM backend.  Gradients, histograms, split scans and score updates are train.hip; config, bins, feature subsets, tables, the
// tree book-keeping and the model text are train_host.cpp; the validation metric is eval.hip's (the number mrk_eval_scores gives).
// The loop over splits is driven from here: per split one histogram launch, one scan, two records read back.
// backend "xgboost" (steps 2x, 5x, 6x, 7x): the loop is over LEVELS - per level one histogram launch, one scan, the level's records
// read back once - and the model text is XGBoost's JSON.
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
#include "train_host.hpp"

using namespace mrk;

namespace {

struct TrainSet {
  bool given = false;
  int64_t rows = 0, n_groups = 0, max_len = 0;
  std::vector<uint8_t> labels;
  std::vector<int64_t> offsets;
  EvalBins by_size;
  DevBuf d_bins, d_labels, d_off, d_wave, d_group, d_score, d_best;
  std::vector<double> gains;        // the validation set: what eval.hip reads (eval_pack_labels, relpow)
  std::vector<uint8_t> rel;
  std::vector<double> scores;       // at the best iteration, after the fit
};

}  // namespace

struct mrk_trainer {
  mrk_ctx *ctx = nullptr;
  TrainConfig cfg;
  std::mutex mu;                    // one set / fit at a time; lock order: mu before ctx->mu
  int cols = 0;
  std::vector<std::vector<double>> bounds;
  std::vector<std::string> infos;
  std::vector<std::vector<int32_t>> kept;   // step 2c: per categorical column its kept ids (a numeric column: empty)
  std::vector<int32_t> is_cat;              // per column
  bool any_cat = false;
  DevBuf d_bounds, d_bound_off, d_nbins, d_is_cat, d_cat_idx, d_cat_tables;
  TrainSet set[2];
  bool fitted = false;
  std::vector<TrainTree> trees;
  std::vector<TrainXgbTree> xtrees;         // backend "xgboost"
  int iterations_run = 0;
  std::vector<double> history;
  int best_iteration = 0;
  std::string model;
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

// backend "xgboost": the most nodes of one level that is scanned (depth < maxDepth; every node holds a sampled row)
int64_t level_cap(const TrainConfig &cfg, int64_t rows) { return std::max<int64_t>(1, std::min<int64_t>(int64_t(1) << (cfg.max_depth - 1), rows)); }

void check_free(double want, const std::string &what) {
  size_t free_b = 0, total_b = 0;
  MRK_HIP(hipMemGetInfo(&free_b, &total_b));
  if (want > (double)free_b)
    throw StatusError(MRK_ERR_UNSUPPORTED, "train: " + what + " need " + std::to_string((unsigned long long)want) + " bytes on the device, " + std::to_string(free_b) + " are free");
}

void set_locked(mrk_trainer *t, int which, const double *x, int64_t rows, int cols, const double *labels, const int64_t *off, int64_t n_groups) {
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
  TrainSet &s = t->set[which];
  s = TrainSet();
  s.labels = train_check_labels(labels, rows);
  if (which == 1) {
    need(t->set[0].given, "train: the validation set comes after the training set");
    need(cols == t->cols, "train: the validation set has other columns than the training set");
    s.gains.resize((size_t)rows);
    s.rel.resize((size_t)rows);
    eval_pack_labels(labels, rows, true, s.gains.data(), s.rel.data());
    for (int64_t i = 0; i < rows * cols; ++i)
      if (std::isinf(x[i])) throw StatusError(MRK_ERR_INVALID_ARG, "train: cell " + std::to_string(i) + " of the validation matrix is infinite");
    for (int32_t c : t->cfg.categorical) train_check_categories(x + c, rows, cols, c);
    if (t->cfg.backend == TRAIN_BACKEND_XGBOOST) for_columns(cols, [&](int c) { train_check_f32_cells(x + c, rows, cols, c); });
  } else {
    t->set[1] = TrainSet();
    t->cols = cols;
    t->bounds.assign((size_t)cols, {});
    t->infos.assign((size_t)cols, "");
    t->kept.assign((size_t)cols, {});
    t->is_cat.assign((size_t)cols, 0);
    for (int32_t c : t->cfg.categorical) t->is_cat[(size_t)c] = 1;
    t->any_cat = !t->cfg.categorical.empty();
    for_columns(cols, [&](int c) {
      if (t->cfg.backend == TRAIN_BACKEND_XGBOOST) t->bounds[(size_t)c] = train_bin_bounds_f32(x + c, rows, cols, t->cfg.max_bin, c);
      else if (t->is_cat[(size_t)c]) t->kept[(size_t)c] = train_kept_categories(x + c, rows, cols, t->cfg.max_bin, c, &t->infos[(size_t)c]);
      else t->bounds[(size_t)c] = train_bin_bounds(x + c, rows, cols, t->cfg.max_bin, &t->infos[(size_t)c]);
    });
  }
  s.rows = rows, s.n_groups = n_groups, s.max_len = sh.max_len;
  s.offsets.assign(off, off + n_groups + 1);
  s.by_size = eval_bins(off, n_groups, EVAL_WAVE_ITEMS);

  mrk_ctx *ctx = t->ctx;
  DeviceLock lk(ctx);
  hipStream_t st = lk.stream;
  const std::vector<EvalPiece> pieces = eval_pieces(rows, cols, env_int("MRK_TRAIN_PIECE_ROWS", 0));
  const size_t piece_bytes = (size_t)pieces[0].rows * (size_t)cols * 8;
  const bool xgb = t->cfg.backend == TRAIN_BACKEND_XGBOOST;
  const int n_sub = xgb ? cols : (int)train_feature_subset(cols, t->cfg.sampling, 0, 0).size();
  // the histograms: numLeaves slots, or (xgboost) two levels of level_cap slots; per slot and column 256 cells of 20 B and a record
  const double hist_slots = xgb ? 2.0 * (double)level_cap(t->cfg, rows) : (double)t->cfg.num_leaves;
  // resident for the fit: the bins, per row g, h, q_g, q_h, score, best score, leaf and label, the lists of groups, the histograms
  const double fit_bytes = (double)rows * cols + 51.0 * (double)rows + 12.0 * (double)n_groups +
                           (which == 0 ? (20.0 * 256.0 + (xgb ? sizeof(LeafRec) : 0)) * (double)n_sub * hist_slots + 2.0 * sizeof(LeafRec) * (double)n_sub + (xgb ? 2.0 * (double)rows : 0.0)
                                       : 9.0 * (double)rows + 8.0 * (double)n_groups + (xgb ? 2.0 * (double)rows : 0.0));
  check_free(fit_bytes + (double)piece_bytes + 1048576.0, std::to_string(rows) + " rows x " + std::to_string(cols) + " columns in " + std::to_string(n_groups) + " groups, " +
                                                              (xgb ? "2 levels x " + std::to_string(level_cap(t->cfg, rows)) + " nodes x " : std::to_string(t->cfg.num_leaves) + " leaves x ") + std::to_string(n_sub) +
                                                              " columns of histograms");
  if (which == 0) {
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
  s.d_bins.reserve((size_t)rows * (size_t)cols);
  DevBuf d_x;
  d_x.reserve(piece_bytes);
  for (const EvalPiece &pc : pieces) {
    MRK_HIP(hipMemcpyAsync(d_x.p, x + (size_t)pc.row0 * (size_t)cols, (size_t)pc.rows * (size_t)cols * 8, hipMemcpyHostToDevice, st));
    if (xgb) train_launch_bin_f32(ctx, st, d_x.as<double>(), pc.rows, cols, t->d_bounds.as<double>(), t->d_bound_off.as<int>(), s.d_bins.as<uint8_t>(), rows, pc.row0);
    else
      train_launch_bin(ctx, st, d_x.as<double>(), pc.rows, cols, t->d_bounds.as<double>(), t->d_bound_off.as<int>(), t->any_cat ? t->d_cat_idx.as<int>() : nullptr,
                       t->any_cat ? t->d_cat_tables.as<uint8_t>() : nullptr, s.d_bins.as<uint8_t>(), rows, pc.row0);
  }
  upload(s.d_labels, s.labels, st);
  upload(s.d_off, s.offsets, st);
  if (!s.by_size.wave.empty()) upload(s.d_wave, s.by_size.wave, st);
  if (!s.by_size.group.empty()) upload(s.d_group, s.by_size.group, st);
  s.d_score.reserve((size_t)rows * 8);
  s.d_best.reserve((size_t)rows * 8);
  MRK_HIP(hipMemsetAsync(s.d_score.p, 0, (size_t)rows * 8, st));
  MRK_HIP(hipMemsetAsync(s.d_best.p, 0, (size_t)rows * 8, st));
  MRK_HIP(hipStreamSynchronize(st));     // the caller's matrix is not kept
  drain_profile_events(ctx);
  s.given = true;
}

// the tables of step 3 on the device
struct GradTables {
  DevBuf d_lg, d_invlg, d_sigmoid;
  SigmoidTable sig;
  void make(const TrainConfig &cfg, int64_t max_len, hipStream_t st) {
    sig = train_sigmoid_table(cfg.sigma);
    const std::vector<double> lg = eval_lg_table(max_len);
    std::vector<double> invlg(lg.size());
    for (size_t i = 0; i < lg.size(); ++i) invlg[i] = 1.0 / lg[i];
    upload(d_lg, lg, st);
    upload(d_invlg, invlg, st);
    upload(d_sigmoid, sig.t, st);
    MRK_HIP(hipStreamSynchronize(st));   // lg and invlg are locals
  }
  GradDev dev(const TrainConfig &cfg) const {
    GradDev d{};
    d.lg = d_lg.as<double>(), d.invlg = d_invlg.as<double>(), d.sigmoid = d_sigmoid.as<double>();
    d.lo = sig.lo, d.f = sig.f, d.sigma = cfg.sigma, d.sigma2 = cfg.sigma * cfg.sigma, d.truncation = cfg.truncation;
    return d;
  }
};

void launch_gradients(mrk_ctx *ctx, hipStream_t st, const GradDev &d, const EvalBins &by_size, const DevBuf &d_wave, const DevBuf &d_group) {
  train_launch_grad_wave(ctx, st, d, d_wave.as<int>(), (int)by_size.wave.size());
  train_launch_grad_group(ctx, st, d, d_group.as<int>(), (int)by_size.group.size(), (int)by_size.group_max_len);
}

// backend "xgboost": the buffers of the level-wise grower and one tree's growth (step 5x).  Two levels of histograms are resident -
// the level being built and its parents' (sibling = parent - built child) - in slots [buf * cap, buf * cap + cap) of one HistDev.
struct LevelGrower {
  int64_t cap = 0;   // level_cap
  int cols = 0;
  DevBuf d_G, d_H, d_C, d_feat_best, d_recs, d_tables, d_value, d_hist_slot, d_vnode_of;
  PinBuf h_recs, h_tables, h_value;
  // one block per level, host -> device in one copy: the level's split records, the next level's built slots and scan nodes
  size_t off_build = 0, off_nodes = 0, table_bytes = 0;

  void reserve(const TrainConfig &cfg, int64_t rows, int64_t valid_rows, int cols_) {
    cap = level_cap(cfg, rows), cols = cols_;
    const size_t cells = 2 * (size_t)cap * (size_t)cols * 256;
    d_G.reserve(cells * 8), d_H.reserve(cells * 8), d_C.reserve(cells * 4);
    d_feat_best.reserve((size_t)cap * (size_t)cols * sizeof(LeafRec));
    d_recs.reserve((size_t)cap * sizeof(LeafRec)), h_recs.reserve((size_t)cap * sizeof(LeafRec));
    off_build = (size_t)cap * sizeof(LevelRec), off_nodes = off_build + (size_t)cap * 4, table_bytes = off_nodes + (size_t)cap * sizeof(LevelNode);
    d_tables.reserve(table_bytes), h_tables.reserve(table_bytes);
    const size_t max_nodes = std::min<size_t>((size_t(2) << cfg.max_depth), 4 * (size_t)cap + 1);   // (a level has at most twice the nodes of the one above)
    d_value.reserve(max_nodes * 4), h_value.reserve(max_nodes * 4);
    d_hist_slot.reserve((size_t)rows * 2);
    if (valid_rows > 0) d_vnode_of.reserve((size_t)valid_rows * 2);
  }

  // -> false when the root cannot split.  node_of: per training row, 0 on entry (train_launch_quantise); on return every row's node.
  // The stream is waited for once per level that is scanned (the level's records), never per node.
  bool grow(mrk_trainer *t, hipStream_t st, int tree_index, const ScanParams &sp, const long long *qg, const long long *qh, uint16_t *node_of, TrainXgbTree &tree,
            std::vector<TrainSums> &totals) {
    mrk_ctx *ctx = t->ctx;
    const TrainConfig &cfg = t->cfg;
    TrainSet &tr = t->set[0], &va = t->set[1];
    const HistDev hd{d_G.as<long long>(), d_H.as<long long>(), d_C.as<unsigned>(), cols};
    uint16_t *hist_slot = d_hist_slot.as<uint16_t>();
    LevelRec *h_lrec = (LevelRec *)h_tables.as<uint8_t>();
    int *h_build = (int *)(h_tables.as<uint8_t>() + off_build);
    LevelNode *h_nodes = (LevelNode *)(h_tables.as<uint8_t>() + off_nodes);
    const LevelRec *d_lrec = (const LevelRec *)d_tables.as<uint8_t>();
    const int *d_build = (const int *)(d_tables.as<uint8_t>() + off_build);
    const LevelNode *d_nodes = (const LevelNode *)(d_tables.as<uint8_t>() + off_nodes);
    const LeafRec *recs = h_recs.as<LeafRec>();
    auto zero_level = [&](int buf, size_t n) {
      const size_t at = (size_t)buf * (size_t)cap * (size_t)cols * 256, cells = n * (size_t)cols * 256;
      MRK_HIP(hipMemsetAsync(hd.G + at, 0, cells * 8, st));
      MRK_HIP(hipMemsetAsync(hd.H + at, 0, cells * 8, st));
      MRK_HIP(hipMemsetAsync(hd.C + at, 0, cells * 4, st));
    };

    train_launch_level_begin(ctx, st, tr.rows, cfg.sampling, cfg.seed, tree_index, node_of, hist_slot);
    if (va.given) MRK_HIP(hipMemsetAsync(d_vnode_of.p, 0, (size_t)va.rows * 2, st));
    tree = TrainXgbTree();
    tree.add(2147483647);
    totals.assign(1, TrainSums());
    std::vector<int> ids{0};   // the nodes of the level, ascending
    h_build[0] = 0;
    h_nodes[0] = LevelNode{0, -1, -1};
    MRK_HIP(hipMemcpyAsync(d_tables.p, h_tables.p, table_bytes, hipMemcpyHostToDevice, st));
    zero_level(0, 1);
    train_launch_level_hist(ctx, st, tr.d_bins.as<uint8_t>(), tr.rows, hist_slot, qg, qh, d_build, 1, hd);
    for (int d = 0, buf = 0; d < cfg.max_depth; ++d, buf ^= 1) {
      const int n = (int)ids.size();
      train_launch_level_scan(ctx, st, hd, t->d_nbins.as<int>(), d_nodes, n, sp, d_feat_best.as<LeafRec>(), d_recs.as<LeafRec>());
      {
        ScopedKernelTimer timer(ctx, "train_level_readback");
        MRK_HIP(hipMemcpyAsync(h_recs.p, d_recs.p, (size_t)n * sizeof(LeafRec), hipMemcpyDeviceToHost, st));
      }
      MRK_HIP(hipStreamSynchronize(st));   // (h_tables is free again too)
      if (d == 0) totals[0] = TrainSums{recs[0].g, recs[0].h, recs[0].c};
      const bool build_next = d + 1 < cfg.max_depth;
      std::vector<int> next;
      int n_build = 0;
      for (int k = 0; k < n; ++k) {
        const LeafRec &c = recs[k];
        LevelRec &lr = h_lrec[k];
        lr = LevelRec{-1, 0, (uint16_t)TRAIN_NO_SLOT, (uint16_t)TRAIN_NO_SLOT, 0, 0};
        if (!c.valid) continue;
        const int node = ids[(size_t)k];
        const TrainSums whole = totals[(size_t)node];
        tree.split(node, c.col, c.bin, (float)t->bounds[(size_t)c.col][(size_t)c.bin], c.nan_left != 0, (float)c.gain);
        const int l = tree.num_nodes() - 2;
        const TrainSums left{c.gl, c.hl, c.cl}, right{whole.g - c.gl, whole.h - c.hl, whole.c - c.cl};
        totals.push_back(left), totals.push_back(right);
        lr.col = c.col, lr.left = (uint16_t)l, lr.bin = (uint8_t)c.bin, lr.nan_left = (uint8_t)(c.nan_left != 0);
        if (build_next) {   // the child with fewer sampled rows is built (ties: the left), its sibling is parent - built
          const int kl = (int)next.size(), parent_slot = buf * (int)cap + k, slot_l = (buf ^ 1) * (int)cap + kl;
          const bool left_built = left.c <= right.c;
          (left_built ? lr.slot_l : lr.slot_r) = (uint16_t)n_build;
          h_build[n_build++] = left_built ? slot_l : slot_l + 1;
          h_nodes[kl] = left_built ? LevelNode{slot_l, -1, -1} : LevelNode{slot_l, parent_slot, slot_l + 1};
          h_nodes[kl + 1] = left_built ? LevelNode{slot_l + 1, parent_slot, slot_l} : LevelNode{slot_l + 1, -1, -1};
        }
        next.push_back(l), next.push_back(l + 1);
      }
      if (next.empty()) break;
      MRK_HIP(hipMemcpyAsync(d_tables.p, h_tables.p, table_bytes, hipMemcpyHostToDevice, st));
      train_launch_level_split(ctx, st, tr.d_bins.as<uint8_t>(), tr.rows, node_of, hist_slot, d_lrec, ids[0], n, cfg.sampling, cfg.seed, tree_index);
      if (va.given) train_launch_level_split(ctx, st, va.d_bins.as<uint8_t>(), va.rows, d_vnode_of.as<uint16_t>(), nullptr, d_lrec, ids[0], n, cfg.sampling, cfg.seed, tree_index);
      if (build_next) {
        zero_level(buf ^ 1, next.size());
        train_launch_level_hist(ctx, st, tr.d_bins.as<uint8_t>(), tr.rows, hist_slot, qg, qh, d_build, n_build, hd);
      }
      ids.swap(next);
    }
    if (tree.num_nodes() == 1) return false;
    float *value = h_value.as<float>();
    for (int node = 0; node < tree.num_nodes(); ++node) {
      tree.weigh(node, totals[(size_t)node], sp.e_g, sp.e_h, cfg.lambda, cfg.learning_rate);
      value[node] = tree.cond[(size_t)node];   // (read for leaves alone)
    }
    MRK_HIP(hipMemcpyAsync(d_value.p, h_value.p, (size_t)tree.num_nodes() * 4, hipMemcpyHostToDevice, st));
    train_launch_level_apply(ctx, st, d_value.as<float>(), node_of, tr.rows, tr.d_score.as<double>());
    if (va.given) train_launch_level_apply(ctx, st, d_value.as<float>(), d_vnode_of.as<uint16_t>(), va.rows, va.d_score.as<double>());
    return true;
  }
};

void fit_locked(mrk_trainer *t) {
  need(t->set[0].given, "train: no training set");
  need(!t->fitted, "train: the trainer has been fitted");
  mrk_ctx *ctx = t->ctx;
  const TrainConfig &cfg = t->cfg;
  TrainSet &tr = t->set[0], &va = t->set[1];
  const int64_t rows = tr.rows;
  const int cols = t->cols;
  // ctx->mu is held per iteration, not for the fit: every iteration ends with the stream waited for, so other calls on the context
  // (/rank among them) get their turn between two trees
  std::unique_ptr<DeviceLock> lk(new DeviceLock(ctx));
  hipStream_t st = lk->stream;
  // a fit starts from score 0, also after one that a device error ended half-way
  const bool xgb = cfg.backend == TRAIN_BACKEND_XGBOOST;
  for (TrainSet *s : {&tr, &va})
    if (s->given) {
      if (xgb) {   // step 6x: the model's base_score
        train_launch_level_base(ctx, st, s->rows, s->d_score.as<double>());
        train_launch_level_base(ctx, st, s->rows, s->d_best.as<double>());
        continue;
      }
      MRK_HIP(hipMemsetAsync(s->d_score.p, 0, (size_t)s->rows * 8, st));
      MRK_HIP(hipMemsetAsync(s->d_best.p, 0, (size_t)s->rows * 8, st));
    }

  GradTables tab;
  tab.make(cfg, std::max(tr.max_len, va.given ? va.max_len : 0), st);
  const int n_sub_max = xgb ? 0 : (int)train_feature_subset(cols, cfg.sampling, 0, 0).size();   // (the xgboost backend's histograms are the grower's)
  LevelGrower grower;
  if (xgb) grower.reserve(cfg, rows, va.given ? va.rows : 0, cols);
  DevBuf d_g, d_h, d_qg, d_qh, d_leaf_of, d_maxes, d_G, d_H, d_C, d_feat_best, d_recs, d_subset;
  DevBuf d_tcol, d_tbin, d_tnan, d_tleft, d_tright, d_tvalue, d_tis_cat, d_tmask;
  d_g.reserve((size_t)rows * 8), d_h.reserve((size_t)rows * 8), d_qg.reserve((size_t)rows * 8), d_qh.reserve((size_t)rows * 8);
  d_leaf_of.reserve((size_t)rows * 2);
  d_maxes.reserve(16);
  const size_t cells = (size_t)cfg.num_leaves * (size_t)n_sub_max * 256;
  d_G.reserve(cells * 8), d_H.reserve(cells * 8), d_C.reserve(cells * 4);
  d_feat_best.reserve(2 * (size_t)n_sub_max * sizeof(LeafRec));
  d_recs.reserve(2 * sizeof(LeafRec));
  d_subset.reserve((size_t)n_sub_max * 4);
  for (DevBuf *b : {&d_tcol, &d_tbin, &d_tnan, &d_tleft, &d_tright}) b->reserve((size_t)cfg.num_leaves * 4);
  d_tvalue.reserve((size_t)cfg.num_leaves * 8);
  if (t->any_cat) d_tis_cat.reserve((size_t)cfg.num_leaves * 4), d_tmask.reserve((size_t)cfg.num_leaves * 32);
  PinBuf h_back;   // what the host reads per iteration / split: two maxima, two records
  h_back.reserve(16 + 2 * sizeof(LeafRec));
  unsigned long long *h_maxes = h_back.as<unsigned long long>();
  LeafRec *h_recs = (LeafRec *)(h_back.as<uint8_t>() + 16);

  // the validation metric: eval.hip's kernels on the validation scores
  DevBuf d_vgains, d_vrel, d_met, d_cut, d_metric;
  EvalDev ev{};
  std::vector<double> per_group;
  if (va.given) {
    const int metric = MRK_METRIC_NDCG;
    upload(d_vgains, va.gains, st);
    upload(d_vrel, va.rel, st);
    d_met.reserve(4), d_cut.reserve(4), d_metric.reserve((size_t)va.n_groups * 8);
    MRK_HIP(hipMemcpyAsync(d_met.p, &metric, 4, hipMemcpyHostToDevice, st));
    MRK_HIP(hipMemcpyAsync(d_cut.p, &cfg.ndcg_cutoff, 4, hipMemcpyHostToDevice, st));
    MRK_HIP(hipStreamSynchronize(st));
    ev.scores = va.d_score.as<double>(), ev.gains = d_vgains.as<double>(), ev.rel = d_vrel.as<uint8_t>(), ev.offsets = va.d_off.as<long long>();
    ev.lg = tab.d_lg.as<double>(), ev.metrics = d_met.as<int>(), ev.cutoffs = d_cut.as<int>(), ev.n_metrics = 1, ev.need_ideal = 1, ev.nolabels = 1.0;
    ev.n_groups = va.n_groups, ev.out = d_metric.as<double>();
    per_group.resize((size_t)va.n_groups);
  }

  GradDev gd = tab.dev(cfg);
  gd.scores = tr.d_score.as<double>(), gd.labels = tr.d_labels.as<uint8_t>(), gd.offsets = tr.d_off.as<long long>(), gd.g = d_g.as<double>(), gd.h = d_h.as<double>();
  const uint8_t *bins = tr.d_bins.as<uint8_t>();
  uint16_t *leaf_of = d_leaf_of.as<uint16_t>();
  double best_metric = 0.0;
  t->trees.clear(), t->xtrees.clear(), t->history.clear(), t->best_iteration = 0, t->iterations_run = 0;

  for (int it = 0; it < cfg.iterations; ++it) {
    if (it > 0) {
      MRK_HIP(hipStreamSynchronize(st));   // (the copies of a new best iteration)
      lk.reset();
      lk.reset(new DeviceLock(ctx));
    }
    launch_gradients(ctx, st, gd, tr.by_size, tr.d_wave, tr.d_group);
    MRK_HIP(hipMemsetAsync(d_maxes.p, 0, 16, st));
    train_launch_max(ctx, st, gd.g, gd.h, rows, d_maxes.as<unsigned long long>());
    MRK_HIP(hipMemcpyAsync(h_maxes, d_maxes.p, 16, hipMemcpyDeviceToHost, st));
    MRK_HIP(hipStreamSynchronize(st));
    double gmax, hmax;
    memcpy(&gmax, &h_maxes[0], 8), memcpy(&hmax, &h_maxes[1], 8);
    if (gmax == 0.0) break;
    ScanParams sp{train_exponent(gmax, rows), train_exponent(hmax, rows), cfg.min_data_in_leaf, cfg.min_sum_hessian, cfg.lambda_l2,
                  cfg.max_cat_to_onehot, cfg.max_cat_threshold, std::max(cfg.min_data_in_leaf, cfg.min_data_per_group), cfg.cat_smooth, cfg.lambda_l2 + cfg.cat_l2, 0.0};
    if (xgb) sp.min_data = 1, sp.min_hess = cfg.min_child_weight, sp.l2 = cfg.lambda, sp.min_gain = cfg.gamma;   // step 5x's admission rule
    train_launch_quantise(ctx, st, gd.g, gd.h, rows, sp.e_g, sp.e_h, d_qg.as<long long>(), d_qh.as<long long>(), leaf_of);
    TrainXgbTree xtree;
    std::vector<TrainSums> xtotals;
    if (xgb && !grower.grow(t, st, it, sp, d_qg.as<long long>(), d_qh.as<long long>(), leaf_of, xtree, xtotals)) break;
    TrainTree tree;
    if (!xgb) {
    const std::vector<int32_t> subset = train_feature_subset(cols, cfg.sampling, cfg.seed, it);
    MRK_HIP(hipMemcpyAsync(d_subset.p, subset.data(), subset.size() * 4, hipMemcpyHostToDevice, st));   // (waited for with the root's record)
    HistDev hd{d_G.as<long long>(), d_H.as<long long>(), d_C.as<unsigned>(), (int)subset.size()};

    auto scan = [&](int leaf_a, int leaf_b, bool small_is_left) {
      train_launch_scan(ctx, st, hd, d_subset.as<int>(), t->d_nbins.as<int>(), t->d_is_cat.as<int>(), leaf_a, leaf_b, small_is_left, sp, d_feat_best.as<LeafRec>(),
                        d_recs.as<LeafRec>());
      MRK_HIP(hipMemcpyAsync(h_recs, d_recs.p, 2 * sizeof(LeafRec), hipMemcpyDeviceToHost, st));
      MRK_HIP(hipStreamSynchronize(st));
    };
    train_launch_hist(ctx, st, bins, rows, leaf_of, 0, 0, d_qg.as<long long>(), d_qh.as<long long>(), d_subset.as<int>(), hd);
    scan(0, -1, false);
    std::vector<LeafRec> cand{h_recs[0]};
    std::vector<TrainSums> totals{TrainSums{h_recs[0].g, h_recs[0].h, h_recs[0].c}};
    while (tree.num_leaves() < cfg.num_leaves) {
      int leaf = -1;
      for (int l = 0; l < tree.num_leaves(); ++l)
        if (cand[(size_t)l].valid && tree.depth[(size_t)l] < cfg.max_depth && (leaf < 0 || cand[(size_t)l].gain > cand[(size_t)leaf].gain)) leaf = l;
      if (leaf < 0) break;
      const LeafRec c = cand[(size_t)leaf];
      const TrainSums whole = totals[(size_t)leaf];
      double weight = 0.0;
      tree.ivalue.push_back(train_leaf_output(whole, sp.e_g, sp.e_h, cfg.lambda_l2, cfg.learning_rate, &weight));
      tree.iweight.push_back(weight);
      tree.icount.push_back(whole.c);
      int fresh;
      if (c.is_cat) {
        fresh = tree.split_cat(leaf, c.col, c.cat_mask, c.gain);
        CatMask mask;
        memcpy(mask.w, c.cat_mask, sizeof mask.w);
        train_launch_split_cat(ctx, st, bins + (size_t)c.col * (size_t)rows, rows, leaf_of, leaf, fresh, mask);
      } else {
        fresh = tree.split(leaf, c.col, c.bin, t->bounds[(size_t)c.col][(size_t)c.bin], c.nan_left != 0, c.gain);
        train_launch_split(ctx, st, bins + (size_t)c.col * (size_t)rows, rows, leaf_of, leaf, fresh, c.bin, c.nan_left);
      }
      const TrainSums left{c.gl, c.hl, c.cl}, right{whole.g - c.gl, whole.h - c.hl, whole.c - c.cl};
      totals[(size_t)leaf] = left;
      totals.push_back(right);
      cand.resize((size_t)fresh + 1);
      if (tree.num_leaves() >= cfg.num_leaves || tree.depth[(size_t)leaf] >= cfg.max_depth) {   // neither child is split again: no histogram
        cand[(size_t)leaf].valid = cand[(size_t)fresh].valid = 0;
        continue;
      }
      const bool small_is_left = left.c <= right.c;
      train_launch_hist(ctx, st, bins, rows, leaf_of, small_is_left ? leaf : fresh, fresh, d_qg.as<long long>(), d_qh.as<long long>(), d_subset.as<int>(), hd);
      scan(leaf, fresh, small_is_left);
      cand[(size_t)leaf] = h_recs[0];
      cand[(size_t)fresh] = h_recs[1];
    }
    if (tree.num_leaves() == 1) break;
    const int nl = tree.num_leaves();
    tree.value.resize((size_t)nl), tree.weight.resize((size_t)nl), tree.count.resize((size_t)nl);
    for (int l = 0; l < nl; ++l) {
      tree.value[(size_t)l] = train_leaf_output(totals[(size_t)l], sp.e_g, sp.e_h, cfg.lambda_l2, cfg.learning_rate, &tree.weight[(size_t)l]);
      tree.count[(size_t)l] = totals[(size_t)l].c;
    }
    std::vector<int32_t> nan_left((size_t)nl - 1);
    for (int n = 0; n < nl - 1; ++n) nan_left[(size_t)n] = (tree.dt[(size_t)n] & 2) ? 1 : 0;
    MRK_HIP(hipMemcpyAsync(d_tcol.p, tree.feat.data(), (size_t)(nl - 1) * 4, hipMemcpyHostToDevice, st));
    MRK_HIP(hipMemcpyAsync(d_tbin.p, tree.bin.data(), (size_t)(nl - 1) * 4, hipMemcpyHostToDevice, st));
    MRK_HIP(hipMemcpyAsync(d_tnan.p, nan_left.data(), (size_t)(nl - 1) * 4, hipMemcpyHostToDevice, st));
    MRK_HIP(hipMemcpyAsync(d_tleft.p, tree.left.data(), (size_t)(nl - 1) * 4, hipMemcpyHostToDevice, st));
    MRK_HIP(hipMemcpyAsync(d_tright.p, tree.right.data(), (size_t)(nl - 1) * 4, hipMemcpyHostToDevice, st));
    MRK_HIP(hipMemcpyAsync(d_tvalue.p, tree.value.data(), (size_t)nl * 8, hipMemcpyHostToDevice, st));
    const bool cat_tree = tree.num_cat() > 0;   // (the validation walk takes its categorical form only for such a tree)
    if (cat_tree) {
      MRK_HIP(hipMemcpyAsync(d_tis_cat.p, tree.is_cat.data(), (size_t)(nl - 1) * 4, hipMemcpyHostToDevice, st));
      MRK_HIP(hipMemcpyAsync(d_tmask.p, tree.cat_mask.data(), (size_t)(nl - 1) * 32, hipMemcpyHostToDevice, st));
    }
    const TreeDev td{d_tcol.as<int>(), d_tbin.as<int>(), d_tnan.as<int>(), d_tleft.as<int>(), d_tright.as<int>(), d_tvalue.as<double>(),
                     cat_tree ? d_tis_cat.as<int>() : nullptr, cat_tree ? d_tmask.as<unsigned>() : nullptr};
    train_launch_apply(ctx, st, td, leaf_of, nullptr, rows, tr.d_score.as<double>());
    if (va.given) train_launch_apply(ctx, st, td, nullptr, va.d_bins.as<uint8_t>(), va.rows, va.d_score.as<double>());
    }
    if (va.given) {
      {
        ScopedKernelTimer timer(ctx, "train_eval");
        eval_launch_wave(ctx, st, ev, va.d_wave.as<int>(), (int)va.by_size.wave.size());
        eval_launch_group(ctx, st, ev, va.d_group.as<int>(), (int)va.by_size.group.size(), (int)va.by_size.group_max_len);
      }
      MRK_HIP(hipMemcpyAsync(per_group.data(), d_metric.p, per_group.size() * 8, hipMemcpyDeviceToHost, st));
    }
    MRK_HIP(hipStreamSynchronize(st));   // the tree's arrays have left the host; the metric has arrived
    if (xgb) t->xtrees.push_back(std::move(xtree));
    else t->trees.push_back(std::move(tree));
    const int n_trees = t->iterations_run = (int)(xgb ? t->xtrees.size() : t->trees.size());
    if (!va.given) {
      t->best_iteration = n_trees;
      continue;
    }
    const double m = eval_mean(per_group.data(), va.n_groups);
    t->history.push_back(m);
    if (t->best_iteration == 0 || m > best_metric) {
      t->best_iteration = n_trees, best_metric = m;
      MRK_HIP(hipMemcpyAsync(tr.d_best.p, tr.d_score.p, (size_t)rows * 8, hipMemcpyDeviceToDevice, st));
      MRK_HIP(hipMemcpyAsync(va.d_best.p, va.d_score.p, (size_t)va.rows * 8, hipMemcpyDeviceToDevice, st));
    } else if (n_trees - t->best_iteration >= cfg.early_stopping) break;
  }
  for (TrainSet *s : {&tr, &va}) {
    if (!s->given) continue;
    s->scores.resize((size_t)s->rows);
    MRK_HIP(hipMemcpyAsync(s->scores.data(), va.given ? s->d_best.p : s->d_score.p, (size_t)s->rows * 8, hipMemcpyDeviceToHost, st));
  }
  MRK_HIP(hipStreamSynchronize(st));
  drain_profile_events(ctx);
  t->model = xgb ? train_write_xgb_model(t->xtrees, (size_t)t->best_iteration, cols)
                 : train_write_model(t->trees, (size_t)t->best_iteration, cols, t->infos, cfg.learning_rate, &t->kept);
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
