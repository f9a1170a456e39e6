// The boosting loop of the LambdaMART fit and its two growers (train_fit.hpp).  Per iteration the stream is waited for once for the
// maxima, once per split (LeafGrower) or per level (LevelGrower) for the records, and once when the tree is finished.
#include "train_fit.hpp"

#include <algorithm>
#include <cstring>
#include <memory>

#include "eval.hpp"

namespace mrk {

void GradTables::make(const TrainConfig &cfg, int64_t max_len, hipStream_t st) {
  sig = train_sigmoid_table(cfg.sigma);
  const std::vector<double> lg = eval_lg_table(max_len);
  std::vector<double> invlg(lg.size());
  for (size_t i = 0; i < lg.size(); ++i) invlg[i] = 1.0 / lg[i];
  upload(d_lg, lg, st);
  upload(d_invlg, invlg, st);
  upload(d_sigmoid, sig.t, st);
  MRK_HIP(hipStreamSynchronize(st));   // lg and invlg are locals
}

GradDev GradTables::dev(const TrainConfig &cfg) const {
  GradDev d{};
  d.lg = d_lg.as<double>(), d.invlg = d_invlg.as<double>(), d.sigmoid = d_sigmoid.as<double>();
  d.lo = sig.lo, d.f = sig.f, d.sigma = cfg.sigma, d.sigma2 = cfg.sigma * cfg.sigma, d.truncation = cfg.truncation;
  return d;
}

void launch_gradients(mrk_ctx *ctx, hipStream_t st, const GradDev &d, const EvalBins &by_size, const DevBuf &d_wave, const DevBuf &d_group) {
  train_launch_grad_wave(ctx, st, d, d_wave.as<int>(), (int)by_size.wave.size());
  train_launch_grad_group(ctx, st, d, d_group.as<int>(), (int)by_size.group.size(), (int)by_size.group_max_len);
}

namespace {

// backend "lightgbm": the buffers of the leaf-wise grower, one tree's growth (steps 5, 5c, 6) and the forest.  One histogram per leaf
// and subset column is resident: a split builds the smaller child's, the scan turns the parent's into the sibling's.
struct LeafGrower {
  int n_sub_max = 0;   // columns of a tree's subset (the same count for every tree)
  DevBuf d_G, d_H, d_C, d_feat_best, d_recs, d_subset;
  DevBuf d_tcol, d_tbin, d_tnan, d_tleft, d_tright, d_tvalue, d_tis_cat, d_tmask;   // the finished tree (TreeDev)
  PinBuf h_back;                    // the two records of a scan
  std::vector<int32_t> nan_left;    // of the finished tree, per node: alive until its copy has been waited for
  std::vector<TrainTree> trees;

  void reserve(const TrainState &t) {
    const TrainConfig &cfg = t.cfg;
    n_sub_max = (int)train_feature_subset(t.cols, cfg.sampling, 0, 0).size();
    const size_t cells = (size_t)cfg.num_leaves * (size_t)n_sub_max * 256;
    d_G.reserve(cells * 8), d_H.reserve(cells * 8), d_C.reserve(cells * 4);
    d_feat_best.reserve(2 * (size_t)n_sub_max * sizeof(LeafRec));
    d_recs.reserve(2 * sizeof(LeafRec)), h_back.reserve(2 * sizeof(LeafRec));
    d_subset.reserve((size_t)n_sub_max * 4);
    for (DevBuf *b : {&d_tcol, &d_tbin, &d_tnan, &d_tleft, &d_tright}) b->reserve((size_t)cfg.num_leaves * 4);
    d_tvalue.reserve((size_t)cfg.num_leaves * 8);
    if (t.any_cat) d_tis_cat.reserve((size_t)cfg.num_leaves * 4), d_tmask.reserve((size_t)cfg.num_leaves * 32);
  }

  // -> false when the root cannot split.  leaf_of: per training row, 0 on entry (train_launch_quantise); on return every row's leaf.
  // The stream is waited for once per scan (its two records).  The tree joins `trees` before its arrays are copied to the device.
  bool grow(TrainState &t, hipStream_t st, int tree_index, const ScanParams &sp, const long long *qg, const long long *qh, uint16_t *leaf_of) {
    mrk_ctx *ctx = t.ctx;
    const TrainConfig &cfg = t.cfg;
    TrainSet &tr = t.set[0], &va = t.set[1];
    const int64_t rows = tr.rows;
    const uint8_t *bins = tr.d_bins.as<uint8_t>();
    const LeafRec *h_recs = h_back.as<LeafRec>();
    const std::vector<int32_t> subset = train_feature_subset(t.cols, cfg.sampling, cfg.seed, tree_index);
    MRK_HIP(hipMemcpyAsync(d_subset.p, subset.data(), subset.size() * 4, hipMemcpyHostToDevice, st));   // (waited for with the root's record)
    const HistDev hd{d_G.as<long long>(), d_H.as<long long>(), d_C.as<unsigned>(), (int)subset.size()};
    auto scan = [&](int leaf_a, int leaf_b, bool small_is_left) {
      train_launch_scan(ctx, st, hd, d_subset.as<int>(), t.d_nbins.as<int>(), t.d_is_cat.as<int>(), leaf_a, leaf_b, small_is_left, sp, d_feat_best.as<LeafRec>(),
                        d_recs.as<LeafRec>());
      MRK_HIP(hipMemcpyAsync(h_back.p, d_recs.p, 2 * sizeof(LeafRec), hipMemcpyDeviceToHost, st));
      MRK_HIP(hipStreamSynchronize(st));
    };

    train_launch_hist(ctx, st, bins, rows, leaf_of, 0, 0, qg, qh, d_subset.as<int>(), hd);
    scan(0, -1, false);
    trees.emplace_back();
    TrainTree &tree = trees.back();
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
        fresh = tree.split(leaf, c.col, c.bin, t.bounds[(size_t)c.col][(size_t)c.bin], c.nan_left != 0, c.gain);
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
      train_launch_hist(ctx, st, bins, rows, leaf_of, small_is_left ? leaf : fresh, fresh, qg, qh, d_subset.as<int>(), hd);
      scan(leaf, fresh, small_is_left);
      cand[(size_t)leaf] = h_recs[0];
      cand[(size_t)fresh] = h_recs[1];
    }
    if (tree.num_leaves() == 1) {
      trees.pop_back();
      return false;
    }
    const int nl = tree.num_leaves();
    tree.value.resize((size_t)nl), tree.weight.resize((size_t)nl), tree.count.resize((size_t)nl);
    for (int l = 0; l < nl; ++l) {
      tree.value[(size_t)l] = train_leaf_output(totals[(size_t)l], sp.e_g, sp.e_h, cfg.lambda_l2, cfg.learning_rate, &tree.weight[(size_t)l]);
      tree.count[(size_t)l] = totals[(size_t)l].c;
    }
    nan_left.resize((size_t)nl - 1);
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
    return true;
  }

  std::string model(const TrainState &t) const { return train_write_model(trees, (size_t)t.best_iteration, t.cols, t.infos, t.cfg.learning_rate, &t.kept); }
};

// backend "xgboost": the buffers of the level-wise grower, one tree's growth (step 5x) and the forest.  Two levels of histograms are
// resident - the level being built and its parents' (sibling = parent - built child) - in slots [buf * cap, buf * cap + cap) of one HistDev.
struct LevelGrower {
  int64_t cap = 0;   // train_level_cap
  int cols = 0;
  DevBuf d_G, d_H, d_C, d_feat_best, d_recs, d_tables, d_value, d_hist_slot, d_vnode_of;
  PinBuf h_recs, h_tables, h_value;
  // one block per level, host -> device in one copy: the level's split records, the next level's built slots and scan nodes
  size_t off_build = 0, off_nodes = 0, table_bytes = 0;
  std::vector<TrainXgbTree> trees;

  void reserve(const TrainState &t) {
    const TrainConfig &cfg = t.cfg;
    cap = train_level_cap(cfg, t.set[0].rows), cols = t.cols;
    const size_t cells = 2 * (size_t)cap * (size_t)cols * 256;
    d_G.reserve(cells * 8), d_H.reserve(cells * 8), d_C.reserve(cells * 4);
    d_feat_best.reserve((size_t)cap * (size_t)cols * sizeof(LeafRec));
    d_recs.reserve((size_t)cap * sizeof(LeafRec)), h_recs.reserve((size_t)cap * sizeof(LeafRec));
    off_build = (size_t)cap * sizeof(LevelRec), off_nodes = off_build + (size_t)cap * 4, table_bytes = off_nodes + (size_t)cap * sizeof(LevelNode);
    d_tables.reserve(table_bytes), h_tables.reserve(table_bytes);
    const size_t max_nodes = std::min<size_t>((size_t(2) << cfg.max_depth), 4 * (size_t)cap + 1);   // (a level has at most twice the nodes of the one above)
    d_value.reserve(max_nodes * 4), h_value.reserve(max_nodes * 4);
    d_hist_slot.reserve((size_t)t.set[0].rows * 2);
    if (t.set[1].given) d_vnode_of.reserve((size_t)t.set[1].rows * 2);
  }

  // -> false when the root cannot split.  node_of: per training row, 0 on entry (train_launch_quantise); on return every row's node.
  // The stream is waited for once per level that is scanned (the level's records), never per node.
  bool grow(TrainState &t, hipStream_t st, int tree_index, const ScanParams &sp, const long long *qg, const long long *qh, uint16_t *node_of) {
    mrk_ctx *ctx = t.ctx;
    const TrainConfig &cfg = t.cfg;
    TrainSet &tr = t.set[0], &va = t.set[1];
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
    trees.emplace_back();
    TrainXgbTree &tree = trees.back();
    tree.add(2147483647);
    std::vector<TrainSums> totals(1);   // per node
    std::vector<int> ids{0};            // the nodes of the level, ascending
    h_build[0] = 0;
    h_nodes[0] = LevelNode{0, -1, -1};
    MRK_HIP(hipMemcpyAsync(d_tables.p, h_tables.p, table_bytes, hipMemcpyHostToDevice, st));
    zero_level(0, 1);
    train_launch_level_hist(ctx, st, tr.d_bins.as<uint8_t>(), tr.rows, hist_slot, qg, qh, d_build, 1, hd);
    for (int d = 0, buf = 0; d < cfg.max_depth; ++d, buf ^= 1) {
      const int n = (int)ids.size();
      train_launch_level_scan(ctx, st, hd, t.d_nbins.as<int>(), d_nodes, n, sp, d_feat_best.as<LeafRec>(), d_recs.as<LeafRec>());
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
        tree.split(node, c.col, c.bin, (float)t.bounds[(size_t)c.col][(size_t)c.bin], c.nan_left != 0, (float)c.gain);
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
    if (tree.num_nodes() == 1) {
      trees.pop_back();
      return false;
    }
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

  std::string model(const TrainState &t) const { return train_write_xgb_model(trees, (size_t)t.best_iteration, t.cols); }
};

// the validation metric: eval.hip's kernels on the validation scores (the number mrk_eval_scores gives)
struct ValidMetric {
  DevBuf d_vgains, d_vrel, d_met, d_cut, d_metric;
  EvalDev ev{};
  std::vector<double> per_group;

  void make(const TrainConfig &cfg, const TrainSet &va, const double *d_lg, hipStream_t st) {
    const int metric = MRK_METRIC_NDCG;
    upload(d_vgains, va.gains, st);
    upload(d_vrel, va.rel, st);
    d_met.reserve(4), d_cut.reserve(4), d_metric.reserve((size_t)va.n_groups * 8);
    MRK_HIP(hipMemcpyAsync(d_met.p, &metric, 4, hipMemcpyHostToDevice, st));
    MRK_HIP(hipMemcpyAsync(d_cut.p, &cfg.ndcg_cutoff, 4, hipMemcpyHostToDevice, st));
    MRK_HIP(hipStreamSynchronize(st));
    ev.scores = va.d_score.as<double>(), ev.gains = d_vgains.as<double>(), ev.rel = d_vrel.as<uint8_t>(), ev.offsets = va.d_off.as<long long>();
    ev.lg = d_lg, ev.metrics = d_met.as<int>(), ev.cutoffs = d_cut.as<int>(), ev.n_metrics = 1, ev.need_ideal = 1, ev.nolabels = 1.0;
    ev.n_groups = va.n_groups, ev.out = d_metric.as<double>();
    per_group.resize((size_t)va.n_groups);
  }
  // the metric of every group on its way to the host: mean() after the stream has been waited for
  void launch(mrk_ctx *ctx, hipStream_t st, const TrainSet &va) {
    {
      ScopedKernelTimer timer(ctx, "train_eval");
      eval_launch_wave(ctx, st, ev, va.d_wave.as<int>(), (int)va.by_size.wave.size());
      eval_launch_group(ctx, st, ev, va.d_group.as<int>(), (int)va.by_size.group.size(), (int)va.by_size.group_max_len);
    }
    MRK_HIP(hipMemcpyAsync(per_group.data(), d_metric.p, per_group.size() * 8, hipMemcpyDeviceToHost, st));
  }
  double mean() const { return eval_mean(per_group.data(), (int64_t)per_group.size()); }
};

}  // namespace

void train_fit(TrainState &t) {
  mrk_ctx *ctx = t.ctx;
  const TrainConfig &cfg = t.cfg;
  TrainSet &tr = t.set[0], &va = t.set[1];
  const int64_t rows = tr.rows;
  const bool xgb = cfg.backend == TRAIN_BACKEND_XGBOOST;
  // ctx->mu is held per iteration, not for the fit: every iteration ends with the stream waited for, so other calls on the context
  // (/rank among them) get their turn between two trees
  std::unique_ptr<DeviceLock> lk(new DeviceLock(ctx));
  hipStream_t st = lk->stream;
  // a fit starts from score 0 (xgboost, step 6x: the model's base_score), also after one that a device error ended half-way
  for (TrainSet *s : {&tr, &va})
    for (DevBuf *b : {&s->d_score, &s->d_best}) {
      if (!s->given) break;
      if (xgb) train_launch_level_base(ctx, st, s->rows, b->as<double>());
      else MRK_HIP(hipMemsetAsync(b->p, 0, (size_t)s->rows * 8, st));
    }
  GradTables tab;
  tab.make(cfg, std::max(tr.max_len, va.given ? va.max_len : 0), st);
  LeafGrower leaf;     // only the backend's grower holds buffers
  LevelGrower level;
  if (xgb) level.reserve(t);
  else leaf.reserve(t);
  DevBuf d_g, d_h, d_qg, d_qh, d_leaf_of, d_maxes;
  d_g.reserve((size_t)rows * 8), d_h.reserve((size_t)rows * 8), d_qg.reserve((size_t)rows * 8), d_qh.reserve((size_t)rows * 8);
  d_leaf_of.reserve((size_t)rows * 2), d_maxes.reserve(16);
  PinBuf h_back;   // the two maxima of an iteration: train_launch_max leaves the bit patterns of two f64 >= 0
  h_back.reserve(16);
  const double *h_maxes = h_back.as<double>();
  ValidMetric metric;
  if (va.given) metric.make(cfg, va, tab.d_lg.as<double>(), st);
  GradDev gd = tab.dev(cfg);
  gd.scores = tr.d_score.as<double>(), gd.labels = tr.d_labels.as<uint8_t>(), gd.offsets = tr.d_off.as<long long>(), gd.g = d_g.as<double>(), gd.h = d_h.as<double>();
  long long *qg = d_qg.as<long long>(), *qh = d_qh.as<long long>();
  uint16_t *leaf_of = d_leaf_of.as<uint16_t>();   // (xgboost: the row's node)
  double best_metric = 0.0;
  t.history.clear(), t.best_iteration = 0, t.iterations_run = 0;

  for (int it = 0; it < cfg.iterations; ++it) {
    if (it > 0) {
      MRK_HIP(hipStreamSynchronize(st));   // (the copies of a new best iteration)
      lk.reset();
      lk.reset(new DeviceLock(ctx));
    }
    launch_gradients(ctx, st, gd, tr.by_size, tr.d_wave, tr.d_group);
    MRK_HIP(hipMemsetAsync(d_maxes.p, 0, 16, st));
    train_launch_max(ctx, st, gd.g, gd.h, rows, d_maxes.as<unsigned long long>());
    MRK_HIP(hipMemcpyAsync(h_back.p, d_maxes.p, 16, hipMemcpyDeviceToHost, st));
    MRK_HIP(hipStreamSynchronize(st));
    const double gmax = h_maxes[0], hmax = h_maxes[1];
    if (gmax == 0.0) break;
    ScanParams sp{train_exponent(gmax, rows), train_exponent(hmax, rows), cfg.min_data_in_leaf, cfg.min_sum_hessian, cfg.lambda_l2,
                  cfg.max_cat_to_onehot, cfg.max_cat_threshold, std::max(cfg.min_data_in_leaf, cfg.min_data_per_group), cfg.cat_smooth, cfg.lambda_l2 + cfg.cat_l2, 0.0};
    if (xgb) sp.min_data = 1, sp.min_hess = cfg.min_child_weight, sp.l2 = cfg.lambda, sp.min_gain = cfg.gamma;   // step 5x's admission rule
    train_launch_quantise(ctx, st, gd.g, gd.h, rows, sp.e_g, sp.e_h, qg, qh, leaf_of);
    if (!(xgb ? level.grow(t, st, it, sp, qg, qh, leaf_of) : leaf.grow(t, st, it, sp, qg, qh, leaf_of))) break;
    if (va.given) metric.launch(ctx, st, va);
    MRK_HIP(hipStreamSynchronize(st));   // the tree's arrays have left the host; the metric has arrived
    const int n_trees = t.iterations_run = it + 1;   // (every iteration so far has grown a tree)
    if (!va.given) {
      t.best_iteration = n_trees;
      continue;
    }
    const double m = metric.mean();
    t.history.push_back(m);
    if (t.best_iteration == 0 || m > best_metric) {
      t.best_iteration = n_trees, best_metric = m;
      MRK_HIP(hipMemcpyAsync(tr.d_best.p, tr.d_score.p, (size_t)rows * 8, hipMemcpyDeviceToDevice, st));
      MRK_HIP(hipMemcpyAsync(va.d_best.p, va.d_score.p, (size_t)va.rows * 8, hipMemcpyDeviceToDevice, st));
    } else if (n_trees - t.best_iteration >= cfg.early_stopping) break;
  }
  for (TrainSet *s : {&tr, &va}) {
    if (!s->given) continue;
    s->scores.resize((size_t)s->rows);
    MRK_HIP(hipMemcpyAsync(s->scores.data(), va.given ? s->d_best.p : s->d_score.p, (size_t)s->rows * 8, hipMemcpyDeviceToHost, st));
  }
  MRK_HIP(hipStreamSynchronize(st));
  drain_profile_events(ctx);
  t.model = xgb ? level.model(t) : leaf.model(t);
}

}  // namespace mrk
