// Host half of the ranking evaluation: see eval_host.hpp.
#include "eval_host.hpp"

#include <algorithm>
#include <cmath>

namespace mrk {

void eval_check_metrics(const int *metrics, const int *cutoffs, int n_metrics) {
  if (!metrics || !cutoffs) throw StatusError(MRK_ERR_INVALID_ARG, "eval: null metrics / cutoffs");
  if (n_metrics < 1) throw StatusError(MRK_ERR_INVALID_ARG, "eval: no metric asked for");
  for (int m = 0; m < n_metrics; ++m) {
    if (metrics[m] < MRK_METRIC_NDCG || metrics[m] > MRK_METRIC_MRR) throw StatusError(MRK_ERR_INVALID_ARG, "eval: unknown metric " + std::to_string(metrics[m]));
    if (cutoffs[m] < 0) throw StatusError(MRK_ERR_INVALID_ARG, "eval: negative cutoff " + std::to_string(cutoffs[m]));
  }
}

EvalShape eval_check_groups(const int64_t *off, int64_t n_groups) {
  if (!off) throw StatusError(MRK_ERR_INVALID_ARG, "eval: null group offsets");
  if (n_groups < 1) throw StatusError(MRK_ERR_INVALID_ARG, "eval: no groups");
  if (n_groups > EVAL_MAX_GROUPS) throw StatusError(MRK_ERR_UNSUPPORTED, "eval: more than " + std::to_string(EVAL_MAX_GROUPS) + " groups in one call");
  if (off[0] != 0) throw StatusError(MRK_ERR_INVALID_ARG, "eval: group offsets do not start at 0");
  EvalShape sh;
  for (int64_t g = 0; g < n_groups; ++g) {
    if (off[g + 1] <= off[g]) throw StatusError(MRK_ERR_INVALID_ARG, "eval: group " + std::to_string(g) + " is empty or its offsets decrease");
    const int64_t len = off[g + 1] - off[g];   // (both in [0, INT64_MAX] and ordered: no overflow)
    if (len > EVAL_MAX_GROUP) throw StatusError(MRK_ERR_UNSUPPORTED, "eval: group " + std::to_string(g) + " has " + std::to_string(len) + " items (limit " + std::to_string(EVAL_MAX_GROUP) + ")");
    sh.max_len = std::max(sh.max_len, len);
  }
  sh.rows = off[n_groups];
  return sh;
}

void eval_pack_labels(const double *labels, int64_t rows, bool relpow, double *gains, uint8_t *rel) {
  if (!labels) throw StatusError(MRK_ERR_INVALID_ARG, "eval: null labels");
  for (int64_t i = 0; i < rows; ++i) {
    const double y = labels[i];
    if (!std::isfinite(y)) throw StatusError(MRK_ERR_INVALID_ARG, "eval: label " + std::to_string(i) + " is not finite");
    gains[i] = relpow ? std::pow(2.0, y) - 1.0 : y;
    rel[i] = y > 0.0 ? 1 : 0;
  }
}

std::vector<double> eval_lg_table(int64_t n) {
  std::vector<double> lg((size_t)std::max<int64_t>(n, 0));
  for (int64_t i = 0; i < n; ++i) lg[(size_t)i] = std::log2((double)(i + 2));
  return lg;
}

void eval_noop_array(const int64_t *off, int64_t n_groups, double *out) {
  for (int64_t g = 0; g < n_groups; ++g) {
    const int64_t len = off[g + 1] - off[g];
    for (int64_t i = 0; i < len; ++i) out[off[g] + i] = (double)(len - i) / (double)len;
  }
}

EvalBins eval_bins(const int64_t *off, int64_t n_groups, int wave_max) {
  wave_max = std::min(std::max(wave_max, 0), EVAL_WAVE_ITEMS);
  EvalBins b;
  for (int64_t g = 0; g < n_groups; ++g) {
    const int64_t len = off[g + 1] - off[g];
    if (len <= wave_max) b.wave.push_back((int32_t)g);
    else if (len <= EVAL_GROUP_ITEMS) {
      b.group.push_back((int32_t)g);
      b.group_max_len = std::max(b.group_max_len, len);
    } else b.big.push_back((int32_t)g);
  }
  return b;
}

std::vector<EvalPiece> eval_pieces(int64_t rows, int cols, int64_t piece_rows) {
  if (piece_rows <= 0) piece_rows = std::max<int64_t>(1, EVAL_PIECE_BYTES / (8 * (int64_t)std::max(cols, 1)));
  piece_rows = std::min<int64_t>(piece_rows, INT32_MAX);
  std::vector<EvalPiece> out;
  for (int64_t r = 0; r < rows; r += piece_rows) out.push_back(EvalPiece{r, (int32_t)std::min(piece_rows, rows - r)});
  return out;
}

double eval_mean(const double *v, int64_t n) {
  double s = v[0];
  for (int64_t i = 1; i < n; ++i) s = s + v[i];
  return s / (double)n;
}

}  // namespace mrk
