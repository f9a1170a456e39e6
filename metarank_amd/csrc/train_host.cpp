// Host half of the LambdaMART fit: see train_host.hpp.
#include "train_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "json.hpp"

namespace mrk {

TrainConfig train_parse_config(const char *text, size_t len) {
  auto bad = [](const std::string &m) -> void { throw StatusError(MRK_ERR_PARSE, "train config: " + m); };
  auto range = [](const std::string &m) -> void { throw StatusError(MRK_ERR_INVALID_ARG, "train config: " + m); };
  json::Value root;
  try {
    root = json::parse(text, len);
  } catch (const std::exception &e) {
    bad(e.what());
  }
  if (!root.is_object()) bad("not an object");
  TrainConfig c;
  static const char *known[] = {"iterations", "learningRate", "ndcgCutoff", "maxDepth", "seed", "numLeaves", "sampling", "debias", "max_bin", "truncation",
                                "sigma", "min_data_in_leaf", "min_sum_hessian", "lambda_l2", "early_stopping", "categorical", "max_cat_to_onehot",
                                "max_cat_threshold", "cat_smooth", "cat_l2", "min_data_per_group", "backend", "lambda", "gamma", "min_child_weight"};
  for (auto &kv : root.obj) {
    bool ok = false;
    for (const char *k : known) ok = ok || kv.first == k;
    if (!ok) bad("unknown key '" + kv.first + "'");
  }
  if (const json::Value *v = root.find("backend"))
    if (!v->is_null()) {
      if (v->type != json::Type::String) bad("'backend' is not a string");
      if (v->str == "lightgbm") c.backend = TRAIN_BACKEND_LIGHTGBM;
      else if (v->str == "xgboost") c.backend = TRAIN_BACKEND_XGBOOST;
      else range("backend = '" + v->str + "' (lightgbm or xgboost)");
    }
  {  // a key of the other backend is refused, not ignored: it would be a setting that silently does nothing
    static const char *lgb_only[] = {"numLeaves", "min_data_in_leaf", "min_sum_hessian", "lambda_l2", "max_cat_to_onehot", "max_cat_threshold", "cat_smooth", "cat_l2",
                                     "min_data_per_group"};
    static const char *xgb_only[] = {"lambda", "gamma", "min_child_weight"};
    auto refuse = [&](const char *key, const char *backend) {
      const json::Value *v = root.find(key);
      if (v && !v->is_null()) range(std::string(key) + " is not a key of the " + backend + " backend");
    };
    if (c.backend == TRAIN_BACKEND_XGBOOST)
      for (const char *k : lgb_only) refuse(k, "xgboost");
    else
      for (const char *k : xgb_only) refuse(k, "lightgbm");
  }
  auto integer = [&](const char *key, int &out) {
    const json::Value *v = root.find(key);
    if (!v || v->is_null()) return;   // Option[Int]: the default stays
    if (!v->is_number()) bad(std::string("'") + key + "' is not a number");
    const double d = v->as_double();
    if (!(d == std::floor(d)) || d < -2147483648.0 || d > 2147483647.0) bad(std::string("'") + key + "' is not an Int");
    out = (int)d;
  };
  auto real = [&](const char *key, double &out) {
    const json::Value *v = root.find(key);
    if (!v || v->is_null()) return;
    if (!v->is_number()) bad(std::string("'") + key + "' is not a number");
    out = v->as_double();
  };
  integer("iterations", c.iterations);
  real("learningRate", c.learning_rate);
  integer("ndcgCutoff", c.ndcg_cutoff);
  integer("maxDepth", c.max_depth);
  integer("seed", c.seed);
  integer("numLeaves", c.num_leaves);
  real("sampling", c.sampling);
  if (const json::Value *v = root.find("debias"))
    if (!v->is_null()) {
      if (v->type != json::Type::Bool) bad("'debias' is not a Boolean");
      c.debias = v->b;
    }
  integer("max_bin", c.max_bin);
  integer("truncation", c.truncation);
  real("sigma", c.sigma);
  integer("min_data_in_leaf", c.min_data_in_leaf);
  real("min_sum_hessian", c.min_sum_hessian);
  real("lambda_l2", c.lambda_l2);
  integer("early_stopping", c.early_stopping);
  integer("max_cat_to_onehot", c.max_cat_to_onehot);
  integer("max_cat_threshold", c.max_cat_threshold);
  real("cat_smooth", c.cat_smooth);
  real("cat_l2", c.cat_l2);
  integer("min_data_per_group", c.min_data_per_group);
  real("lambda", c.lambda);
  real("gamma", c.gamma);
  real("min_child_weight", c.min_child_weight);
  if (const json::Value *v = root.find("categorical"))
    if (!v->is_null()) {
      if (!v->is_array()) bad("'categorical' is not an array");
      for (const json::Value &e : v->arr) {
        if (!e.is_number()) bad("'categorical' holds something that is not a number");
        const double d = e.as_double();
        if (!(d == std::floor(d)) || d < -2147483648.0 || d > 2147483647.0) bad("'categorical' holds something that is not an Int");
        if (d < 0.0) range("categorical holds the negative index " + std::to_string((int)d));
        for (int32_t seen : c.categorical)
          if (seen == (int32_t)d) range("categorical holds the index " + std::to_string((int)d) + " twice");
        c.categorical.push_back((int32_t)d);
      }
    }
  auto at_least = [&](const char *key, int v, int lo) {
    if (v < lo) range(std::string(key) + " = " + std::to_string(v) + " (at least " + std::to_string(lo) + ")");
  };
  at_least("iterations", c.iterations, 1);
  at_least("ndcgCutoff", c.ndcg_cutoff, 1);
  at_least("maxDepth", c.max_depth, 1);
  at_least("numLeaves", c.num_leaves, 2);
  at_least("max_bin", c.max_bin, 2);
  if (c.max_bin > 255) range("max_bin = " + std::to_string(c.max_bin) + " (at most 255: a bin is a byte and 255 is NaN's)");
  at_least("truncation", c.truncation, 1);
  at_least("min_data_in_leaf", c.min_data_in_leaf, 1);
  at_least("early_stopping", c.early_stopping, 1);
  at_least("max_cat_to_onehot", c.max_cat_to_onehot, 1);
  at_least("max_cat_threshold", c.max_cat_threshold, 1);
  at_least("min_data_per_group", c.min_data_per_group, 1);
  if (!(c.cat_smooth > 0.0) || !std::isfinite(c.cat_smooth)) range("cat_smooth is not a positive number");
  if (!(c.cat_l2 >= 0.0) || !std::isfinite(c.cat_l2)) range("cat_l2 is negative");
  if (!(c.learning_rate > 0.0) || !std::isfinite(c.learning_rate)) range("learningRate is not a positive number");
  if (!(c.sampling > 0.0 && c.sampling <= 1.0)) range("sampling is not in (0, 1]");
  if (!(c.sigma > 0.0) || !std::isfinite(c.sigma)) range("sigma is not a positive number");
  if (!(c.min_sum_hessian >= 0.0) || !std::isfinite(c.min_sum_hessian)) range("min_sum_hessian is negative");
  if (!(c.lambda_l2 >= 0.0) || !std::isfinite(c.lambda_l2)) range("lambda_l2 is negative");
  if (!(c.lambda >= 0.0) || !std::isfinite(c.lambda)) range("lambda is negative");
  if (!(c.gamma >= 0.0) || !std::isfinite(c.gamma)) range("gamma is negative");
  if (!(c.min_child_weight >= 0.0) || !std::isfinite(c.min_child_weight)) range("min_child_weight is negative");
  if (c.backend == TRAIN_BACKEND_XGBOOST && c.max_depth > TRAIN_XGB_MAX_DEPTH)
    range("maxDepth = " + std::to_string(c.max_depth) + " (at most " + std::to_string(TRAIN_XGB_MAX_DEPTH) + " with the xgboost backend)");
  if (c.backend == TRAIN_BACKEND_XGBOOST && !c.categorical.empty())
    throw StatusError(MRK_ERR_UNSUPPORTED, "train config: categorical columns are not built for the xgboost backend (set-membership splits in XGBoost JSON)");
  if (c.debias) throw StatusError(MRK_ERR_UNSUPPORTED, "train config: debias (position-bias correction) is not built");
  if (c.num_leaves > TRAIN_MAX_LEAVES)
    throw StatusError(MRK_ERR_UNSUPPORTED, "train config: numLeaves = " + std::to_string(c.num_leaves) + " (limit " + std::to_string(TRAIN_MAX_LEAVES) + ")");
  return c;
}

std::string train_g17(double x) {
  char buf[40];
  snprintf(buf, sizeof buf, "%.17g", x);
  return buf;
}

// step 2's choice of positions over the sorted values v: the p with a bound between v[p - 1] and v[p]
template <typename T>
static std::vector<int64_t> bin_cuts(const std::vector<T> &v, int max_bin) {
  const int64_t m = (int64_t)v.size();
  std::vector<int64_t> change;   // p: v[p] != v[p - 1]
  for (int64_t p = 1; p < m; ++p)
    if (v[(size_t)p] != v[(size_t)p - 1]) change.push_back(p);
  if ((int64_t)change.size() + 1 <= max_bin - 1) return change;
  std::vector<int64_t> cuts;
  for (int64_t i = 1; i <= max_bin - 2; ++i) {
    auto it = std::lower_bound(change.begin(), change.end(), i * m / (max_bin - 1));
    if (it == change.end()) break;
    if (cuts.empty() || cuts.back() != *it) cuts.push_back(*it);
  }
  return cuts;
}

std::string train_numeric_info(int64_t m, double lo, double hi) { return m == 0 || lo == hi ? "none" : "[" + train_g17(lo) + ":" + train_g17(hi) + "]"; }

std::vector<double> train_bin_bounds(const double *col, int64_t n, int64_t stride, int max_bin, std::string *info) {
  std::vector<double> v;
  v.reserve((size_t)std::max<int64_t>(n, 0));
  for (int64_t i = 0; i < n; ++i) {
    double x = col[i * stride];
    if (x != x) continue;
    if (std::isinf(x)) throw StatusError(MRK_ERR_INVALID_ARG, "train: cell " + std::to_string(i) + " of a column is infinite");
    if (x == 0.0) x = 0.0;   // -0.0 and +0.0 are one value
    v.push_back(x);
  }
  std::sort(v.begin(), v.end());
  const int64_t m = (int64_t)v.size();
  if (info) *info = train_numeric_info(m, m ? v.front() : 0.0, m ? v.back() : 0.0);
  std::vector<double> out;
  for (int64_t p : bin_cuts(v, max_bin)) {
    const double a = v[(size_t)p - 1], b = v[(size_t)p];
    double mid = (a + b) / 2.0;
    if (!(mid < b)) mid = a;   // (also a sum that overflowed)
    out.push_back(mid);
  }
  return out;
}

// (float) x, or the refusal of step 2x
static float narrowed(double x, int64_t row, int column) {
  const float f = (float)x;   // round to nearest even
  if (std::isinf(f))
    throw StatusError(MRK_ERR_INVALID_ARG, "train: column " + std::to_string(column) + ", row " + std::to_string(row) + " holds " + train_g17(x) + ", which is not finite as an f32");
  return f;
}

std::vector<double> train_bin_bounds_f32(const double *col, int64_t n, int64_t stride, int max_bin, int column) {
  std::vector<float> v;
  v.reserve((size_t)std::max<int64_t>(n, 0));
  for (int64_t i = 0; i < n; ++i) {
    const double x = col[i * stride];
    if (x != x) continue;
    float f = narrowed(x, i, column);
    if (f == 0.0f) f = 0.0f;   // -0.0f and +0.0f are one value
    v.push_back(f);
  }
  std::sort(v.begin(), v.end());
  std::vector<double> out;
  for (int64_t p : bin_cuts(v, max_bin)) out.push_back((double)v[(size_t)p]);
  return out;
}

void train_check_f32_cells(const double *col, int64_t n, int64_t stride, int column) {
  for (int64_t i = 0; i < n; ++i)
    if (col[i * stride] == col[i * stride]) (void)narrowed(col[i * stride], i, column);
}

int train_bin_f32(double x, const double *bounds, int n_bounds) {
  if (x != x) return TRAIN_NAN_BIN;
  const double v = (double)(float)x;
  return (int)(std::upper_bound(bounds, bounds + n_bounds, v) - bounds);   // the number of bounds <= v
}

// the category of a cell or -1; the refusals of step 2c
static int32_t category_of(double x, int64_t row, int column) {
  if (x != x) return -1;
  if (std::isinf(x)) throw StatusError(MRK_ERR_INVALID_ARG, "train: cell " + std::to_string(row) + " of a column is infinite");
  if (x >= (double)(TRAIN_MAX_CATEGORY + 1))
    throw StatusError(MRK_ERR_UNSUPPORTED, "train: categorical column " + std::to_string(column) + ", row " + std::to_string(row) + " holds " + train_g17(x) +
                                               " (the largest category is " + std::to_string(TRAIN_MAX_CATEGORY) + ")");
  return x <= -1.0 ? -1 : (int32_t)x;   // (the conversion truncates: -0.5 is category 0)
}

std::vector<int32_t> train_kept_categories(const double *col, int64_t n, int64_t stride, int max_bin, int column, std::string *info) {
  std::vector<int64_t> count((size_t)TRAIN_MAX_CATEGORY + 1, 0);
  for (int64_t i = 0; i < n; ++i) {
    const int32_t c = category_of(col[i * stride], i, column);
    if (c >= 0) count[(size_t)c] += 1;
  }
  return train_kept_from_counts(count, max_bin, info);
}

std::vector<int32_t> train_kept_from_counts(const std::vector<int64_t> &count, int max_bin, std::string *info) {
  std::vector<int32_t> ids;
  for (int32_t c = 0; c <= TRAIN_MAX_CATEGORY; ++c)
    if (count[(size_t)c] > 0) ids.push_back(c);
  if ((int64_t)ids.size() > max_bin - 1) {
    std::sort(ids.begin(), ids.end(), [&](int32_t a, int32_t b) { return count[(size_t)a] != count[(size_t)b] ? count[(size_t)a] > count[(size_t)b] : a < b; });
    ids.resize((size_t)(max_bin - 1));
    std::sort(ids.begin(), ids.end());
  }
  if (info) {
    *info = ids.empty() ? "none" : "";
    for (size_t k = 0; k < ids.size(); ++k) *info += (k ? ":" : "") + std::to_string(ids[k]);
  }
  return ids;
}

void train_check_categories(const double *col, int64_t n, int64_t stride, int column) {
  for (int64_t i = 0; i < n; ++i) (void)category_of(col[i * stride], i, column);
}

std::vector<uint8_t> train_category_table(const std::vector<int32_t> &kept) {
  std::vector<uint8_t> table(kept.empty() ? 0 : (size_t)kept.back() + 1, (uint8_t)TRAIN_NAN_BIN);
  for (size_t k = 0; k < kept.size(); ++k) table[(size_t)kept[k]] = (uint8_t)k;
  return table;
}

static uint64_t splitmix64(uint64_t &state) {
  state += 0x9E3779B97F4A7C15ull;
  uint64_t z = state;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

std::vector<int32_t> train_feature_subset(int cols, double sampling, int seed, int tree) {
  const int k = std::min(cols, std::max(1, (int)std::floor((double)cols * sampling + 0.5)));
  uint64_t state = ((uint64_t)(uint32_t)seed << 32) | (uint64_t)(uint32_t)tree;
  std::vector<int32_t> idx((size_t)cols);
  for (int i = 0; i < cols; ++i) idx[(size_t)i] = i;
  for (int j = 0; j < k; ++j) {
    const int r = j + (int)(splitmix64(state) % (uint64_t)(cols - j));
    std::swap(idx[(size_t)j], idx[(size_t)r]);
  }
  idx.resize((size_t)k);
  std::sort(idx.begin(), idx.end());
  return idx;
}

SigmoidTable train_sigmoid_table(double sigma) {
  SigmoidTable s;
  s.lo = -25.0 / sigma;
  s.f = (double)TRAIN_SIGMOID_BINS / (50.0 / sigma);
  s.t.resize(TRAIN_SIGMOID_BINS);
  for (int t = 0; t < TRAIN_SIGMOID_BINS; ++t) {
    const double x = s.lo + (double)t / s.f;
    const double z = sigma * x;
    s.t[(size_t)t] = 1.0 / (1.0 + std::exp(z));
  }
  return s;
}

int train_exponent(double vmax, int64_t rows) {
  if (vmax == 0.0) return 0;
  int bitlen = 0;
  for (uint64_t r = (uint64_t)rows; r; r >>= 1) ++bitlen;
  int e = 0;
  std::frexp(vmax, &e);
  return 61 - bitlen - e;
}

int64_t train_level_cap(const TrainConfig &cfg, int64_t rows) { return std::max<int64_t>(1, std::min<int64_t>(int64_t(1) << (cfg.max_depth - 1), rows)); }

double train_fit_bytes(const TrainConfig &cfg, int which, int64_t rows_, int cols, int64_t n_groups_) {
  const bool xgb = cfg.backend == TRAIN_BACKEND_XGBOOST;
  const double rows = (double)rows_, groups = (double)n_groups_, rec = TRAIN_LEAF_REC_BYTES;
  const double n_sub = xgb ? (double)cols : (double)train_feature_subset(cols, cfg.sampling, 0, 0).size();
  const double column_cells = 256.0 * 20.0;   // of one (slot, column) histogram: G and H i64, C u32
  const double bins = rows * cols;
  const double per_row = 51.0 * rows;         // g, h, q_g, q_h, score and best score (8 each), leaf / node (2), label (1)
  const double group_lists = 12.0 * groups;   // the offsets (8) and the by-size lists (4)
  const double row_slots = xgb ? 2.0 * rows : 0.0;   // xgboost, a u16 per row: hist_slot (training), the row's node (validation)
  if (which == 1) return bins + per_row + group_lists + row_slots + (9.0 * rows + 8.0 * groups);   // gains (8), rel (1); the metric per group
  // numLeaves histograms - or two resident levels of train_level_cap nodes, each with a record per (node, column) - and the scan's two
  // rows of records per column (counted for both backends, as it always was: LevelGrower holds one level's records, not two and two rows)
  const double hist = xgb ? (column_cells + rec) * n_sub * 2.0 * (double)train_level_cap(cfg, rows_) : column_cells * n_sub * (double)cfg.num_leaves;
  const double scan_records = 2.0 * rec * n_sub;
  return bins + per_row + group_lists + row_slots + hist + scan_records;
}

std::vector<uint8_t> train_check_labels(const double *labels, int64_t rows) {
  if (!labels) throw StatusError(MRK_ERR_INVALID_ARG, "train: null labels");
  std::vector<uint8_t> out((size_t)rows);
  for (int64_t i = 0; i < rows; ++i) {
    const double y = labels[i];
    if (!(y >= 0.0 && y <= (double)TRAIN_MAX_LABEL) || y != std::floor(y))
      throw StatusError(MRK_ERR_INVALID_ARG, "train: label " + std::to_string(i) + " is " + train_g17(y) + ", not an integer in 0 ... " + std::to_string(TRAIN_MAX_LABEL));
    out[(size_t)i] = (uint8_t)y;
  }
  return out;
}

int TrainTree::split(int leaf, int col, int b, double thr_, bool nan_left, double gain_) {
  const int s = (int)feat.size(), fresh = s + 1;
  feat.push_back(col);
  bin.push_back(b);
  gain.push_back(gain_);
  thr.push_back(thr_);
  dt.push_back(8 | (nan_left ? 2 : 0));
  is_cat.push_back(0);
  cat_mask.resize(cat_mask.size() + 8, 0u);
  left.push_back(~leaf);
  right.push_back(~fresh);
  if (parent_node[(size_t)leaf] >= 0) (parent_side[(size_t)leaf] == 0 ? left : right)[(size_t)parent_node[(size_t)leaf]] = s;
  parent_node[(size_t)leaf] = s;
  parent_side[(size_t)leaf] = 0;
  parent_node.push_back(s);
  parent_side.push_back(1);
  depth[(size_t)leaf] += 1;
  depth.push_back(depth[(size_t)leaf]);
  return fresh;
}

int TrainTree::num_cat() const {
  int n = 0;
  for (int32_t c : is_cat) n += c;
  return n;
}

int TrainTree::split_cat(int leaf, int col, const uint32_t *mask8, double gain_) {
  const int ordinal = num_cat();
  const int fresh = split(leaf, col, 0, (double)ordinal, false, gain_);
  dt.back() = 9;
  is_cat.back() = 1;
  std::copy(mask8, mask8 + 8, cat_mask.end() - 8);
  return fresh;
}

double train_leaf_output(const TrainSums &q, int e_g, int e_h, double l2, double lr, double *weight) {
  const double G = std::ldexp((double)q.g, -e_g), H = std::ldexp((double)q.h, -e_h);
  if (weight) *weight = H;
  const double d = H + l2;
  const double v = -G / d;
  return v * lr;
}

std::string train_write_model(const std::vector<TrainTree> &trees, size_t n_trees, int cols, const std::vector<std::string> &infos, double lr,
                              const std::vector<std::vector<int32_t>> *kept) {
  auto ints = [](std::string &o, const char *key, const auto &a, size_t n) {
    o += key;
    for (size_t i = 0; i < n; ++i) o += (i ? " " : "") + std::to_string((long long)a[i]);
    o += "\n";
  };
  auto f64s = [](std::string &o, const char *key, const std::vector<double> &a, size_t n) {
    o += key;
    for (size_t i = 0; i < n; ++i) o += (i ? " " : "") + train_g17(a[i]);
    o += "\n";
  };
  std::vector<std::string> blocks;
  for (size_t i = 0; i < n_trees; ++i) {
    const TrainTree &t = trees[i];
    const size_t nl = (size_t)t.num_leaves(), nn = nl - 1;
    const int n_cat = t.num_cat();
    std::string b = "Tree=" + std::to_string(i) + "\nnum_leaves=" + std::to_string(nl) + "\nnum_cat=" + std::to_string(n_cat) + "\n";
    ints(b, "split_feature=", t.feat, nn);
    b += "split_gain=";
    for (size_t k = 0; k < nn; ++k) {
      char buf[40];
      snprintf(buf, sizeof buf, "%.9g", (double)(float)t.gain[k]);
      b += (k ? " " : "") + std::string(buf);
    }
    b += "\n";
    f64s(b, "threshold=", t.thr, nn);
    ints(b, "decision_type=", t.dt, nn);
    ints(b, "left_child=", t.left, nn);
    ints(b, "right_child=", t.right, nn);
    f64s(b, "leaf_value=", t.value, nl);
    f64s(b, "leaf_weight=", t.weight, nl);
    ints(b, "leaf_count=", t.count, nl);
    f64s(b, "internal_value=", t.ivalue, nn);
    f64s(b, "internal_weight=", t.iweight, nn);
    ints(b, "internal_count=", t.icount, nn);
    if (n_cat > 0) {   // per categorical node, in node order, a bitset over category IDS
      if (!kept) throw StatusError(MRK_ERR_INVALID_ARG,"train: a categorical node without the tables of kept ids");
      std::vector<int64_t> boundaries{0};
      std::vector<uint32_t> words;
      for (size_t k = 0; k < nn; ++k) {
        if (!t.is_cat[k]) continue;
        const std::vector<int32_t> &ids = (*kept)[(size_t)t.feat[k]];
        const size_t first = words.size();
        for (size_t bin = 0; bin < ids.size(); ++bin) {   // ascending ids: the last member sizes the bitset
          if (!(t.cat_mask[k * 8 + bin / 32] >> (bin % 32) & 1u)) continue;
          const size_t id = (size_t)ids[bin];
          if (words.size() < first + id / 32 + 1) words.resize(first + id / 32 + 1, 0u);
          words[first + id / 32] |= 1u << (id % 32);
        }
        boundaries.push_back((int64_t)words.size());
      }
      ints(b, "cat_boundaries=", boundaries, boundaries.size());
      ints(b, "cat_threshold=", words, words.size());
    }
    b += "is_linear=0\nshrinkage=" + train_g17(lr);
    blocks.push_back(std::move(b));
  }
  std::string o = "tree\nversion=v4\nnum_class=1\nnum_tree_per_iteration=1\nlabel_index=0\nmax_feature_idx=" + std::to_string(cols - 1) + "\nobjective=lambdarank\nfeature_names=";
  for (int c = 0; c < cols; ++c) o += (c ? " Column_" : "Column_") + std::to_string(c);
  o += "\nfeature_infos=";
  for (int c = 0; c < cols; ++c) o += (c ? " " : "") + infos[(size_t)c];
  o += "\ntree_sizes=";
  for (size_t i = 0; i < blocks.size(); ++i) o += (i ? " " : "") + std::to_string(blocks[i].size() + 3);
  o += "\n\n";
  for (auto &b : blocks) o += b + "\n\n\n";
  o += "end of trees\n\nfeature_importances:\n\nparameters:\n[boosting: gbdt]\n[objective: lambdarank]\n\nend of parameters\n\npandas_categorical:null\n";
  return o;
}

int TrainXgbTree::add(int parent_) {
  left.push_back(-1), right.push_back(-1), parent.push_back(parent_), col.push_back(0), bin.push_back(0), default_left.push_back(0);
  cond.push_back(0.0f), base_weight.push_back(0.0f), loss_change.push_back(0.0f), sum_hessian.push_back(0.0f);
  return num_nodes() - 1;
}

void TrainXgbTree::split(int node, int col_, int bin_, float bound, bool nan_left, float gain) {
  const size_t n = (size_t)node;
  col[n] = col_, bin[n] = bin_, default_left[n] = nan_left ? 1 : 0, cond[n] = bound, loss_change[n] = gain;
  const int l = add(node), r = add(node);
  left[n] = l, right[n] = r;
}

void TrainXgbTree::weigh(int node, const TrainSums &q, int e_g, int e_h, double lambda, double lr) {
  const double G = std::ldexp((double)q.g, -e_g), H = std::ldexp((double)q.h, -e_h);
  const double d = H + lambda;
  if (d == 0.0) throw StatusError(MRK_ERR_INVALID_ARG, "train: node " + std::to_string(node) + " has a hessian sum of 0 and lambda is 0: its weight is not finite");
  const double w = -G / d;
  base_weight[(size_t)node] = (float)w;
  sum_hessian[(size_t)node] = (float)H;
  if (left[(size_t)node] < 0) {
    const double v = w * lr;
    cond[(size_t)node] = (float)v;
  }
}

std::string train_write_xgb_model(const std::vector<TrainXgbTree> &trees, size_t n_trees, int cols) {
  auto ints = [](std::string &o, const char *key, const std::vector<int32_t> &a) {
    o += std::string("\"") + key + "\":[";
    for (size_t i = 0; i < a.size(); ++i) o += (i ? "," : "") + std::to_string(a[i]);
    o += "],";
  };
  auto f32s = [](std::string &o, const char *key, const std::vector<float> &a) {
    o += std::string("\"") + key + "\":[";
    for (size_t i = 0; i < a.size(); ++i) {
      char buf[40];
      snprintf(buf, sizeof buf, "%.9g", (double)a[i]);
      o += (i ? "," : "") + std::string(buf);
    }
    o += "],";
  };
  const std::string n = std::to_string(n_trees), nf = std::to_string(cols);
  std::string o = "{\"learner\":{\"attributes\":{},\"feature_names\":[],\"feature_types\":[],\"gradient_booster\":{\"model\":{\"gbtree_model_param\":{\"num_parallel_tree\":\"1\",\"num_trees\":\"" + n + "\"},\"iteration_indptr\":[";
  for (size_t i = 0; i <= n_trees; ++i) o += (i ? "," : "") + std::to_string(i);
  o += "],\"tree_info\":[";
  for (size_t i = 0; i < n_trees; ++i) o += i ? ",0" : "0";
  o += "],\"trees\":[";
  for (size_t i = 0; i < n_trees; ++i) {
    const TrainXgbTree &t = trees[i];
    const std::vector<int32_t> zeros((size_t)t.num_nodes(), 0);
    o += i ? ",{" : "{";
    f32s(o, "base_weights", t.base_weight);
    o += "\"categories\":[],\"categories_nodes\":[],\"categories_segments\":[],\"categories_sizes\":[],";
    ints(o, "default_left", t.default_left);
    o += "\"id\":" + std::to_string(i) + ",";
    ints(o, "left_children", t.left);
    f32s(o, "loss_changes", t.loss_change);
    ints(o, "parents", t.parent);
    ints(o, "right_children", t.right);
    f32s(o, "split_conditions", t.cond);
    ints(o, "split_indices", t.col);
    ints(o, "split_type", zeros);
    f32s(o, "sum_hessian", t.sum_hessian);
    o += "\"tree_param\":{\"num_deleted\":\"0\",\"num_feature\":\"" + nf + "\",\"num_nodes\":\"" + std::to_string(t.num_nodes()) + "\",\"size_leaf_vector\":\"1\"}}";
  }
  o += "]},\"name\":\"gbtree\"},\"learner_model_param\":{\"base_score\":\"5E-1\",\"boost_from_average\":\"1\",\"num_class\":\"0\",\"num_feature\":\"" + nf +
       "\",\"num_target\":\"1\"},\"objective\":{\"name\":\"rank:ndcg\",\"lambdarank_param\":{}}},\"version\":[2,1,0]}";
  return o;
}

}  // namespace mrk
