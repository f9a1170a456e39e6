// Host half of the similar-items index: see index_host.hpp.
#include "index_host.hpp"

#include <algorithm>
#include <cstring>

namespace mrk {

std::string knn_check_shape(int64_t rows, int cols) {
  if (cols < 1 || cols > KNN_MAX_COLS) return "index: cols = " + std::to_string(cols) + " is outside the limit 1 <= cols <= " + std::to_string(KNN_MAX_COLS);
  if (rows < 0) return "index: negative row count";
  if (rows > KNN_MAX_ROWS) return "index: rows = " + std::to_string(rows) + " is outside the limit rows < 2^31";
  return "";
}

std::string knn_check_n(int n, int n_items) {
  if (n < 0 || n_items < 0) return "index: negative count";
  if ((int64_t)n + n_items > KNN_MAX_N)
    return "index: n + n_items = " + std::to_string((int64_t)n + n_items) + " is outside the limit n + n_items <= " + std::to_string(KNN_MAX_N);
  return "";
}

bool knn_f32_lossless(const double *values, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    const double back = (double)(float)values[i];
    if (memcmp(&back, &values[i], sizeof(double)) != 0) return false;
  }
  return true;
}

std::string KnnIds::build(const char *const *names, int64_t rows) {
  ids.clear();
  row_of.clear();
  ids.reserve((size_t)rows);
  row_of.reserve((size_t)rows);
  for (int64_t r = 0; r < rows; ++r) {
    if (!names[r]) return "index: id of row " + std::to_string(r) + " is null";
    ids.emplace_back(names[r]);
    if (!row_of.emplace(ids.back(), r).second) return "index: id '" + ids.back() + "' is stored twice (row " + std::to_string(r) + ")";
  }
  return "";
}

int64_t KnnIds::row(const char *id) const {
  if (!id) return -1;
  auto it = row_of.find(id);
  return it == row_of.end() ? -1 : it->second;
}

std::vector<int64_t> knn_known_rows(const KnnIds &ids, const char *const *item_ids, int n_items) {
  std::vector<int64_t> out;
  for (int i = 0; i < n_items; ++i) {
    const int64_t r = ids.row(item_ids[i]);
    if (r >= 0) out.push_back(r);
  }
  return out;
}

void knn_centroid(const double *vectors, int n, int cols, double *out) {
  for (int i = 0; i < cols; ++i) {
    double sum = 0.0;
    for (int k = 0; k < n; ++k) sum += vectors[(size_t)k * cols + i];
    out[i] = sum / n;
  }
}

namespace {
// java.lang.Double.compare's order as an unsigned key (sort_device.hpp asc_key, on the host)
uint64_t asc_key_host(double v) {
  uint64_t bits;
  memcpy(&bits, &v, 8);
  if (v != v) bits = 0x7ff8000000000000ULL;
  return (bits & 0x8000000000000000ULL) ? ~bits : (bits | 0x8000000000000000ULL);
}
}  // namespace

int knn_recommend_order(int32_t *rows, double *score, int n_found, const std::vector<int64_t> &request_rows, int count) {
  std::vector<std::pair<uint64_t, int>> kept;   // (key of -score, position among the kept)
  std::vector<int32_t> r;
  std::vector<double> s;
  for (int i = 0; i < n_found && (int)r.size() < count; ++i) {
    if (std::find(request_rows.begin(), request_rows.end(), (int64_t)rows[i]) != request_rows.end()) continue;
    kept.emplace_back(asc_key_host(-score[i]), (int)r.size());
    r.push_back(rows[i]);
    s.push_back(score[i]);
  }
  std::stable_sort(kept.begin(), kept.end(), [](const std::pair<uint64_t, int> &a, const std::pair<uint64_t, int> &b) { return a.first < b.first; });
  for (size_t i = 0; i < kept.size(); ++i) {
    rows[i] = r[(size_t)kept[i].second];
    score[i] = s[(size_t)kept[i].second];
  }
  return (int)kept.size();
}

void knn_plan_pieces(const int32_t *lens, int64_t n, int64_t max_tokens, int max_rows, std::vector<int64_t> &starts) {
  starts.clear();
  int64_t count = 0, tokens = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (count == 0 || !knn_piece_takes(count, tokens, lens[i], max_tokens, max_rows)) {
      starts.push_back(i);
      count = 0;
      tokens = 0;
    }
    ++count;
    tokens += lens[i];
  }
  starts.push_back(n);
}

}  // namespace mrk
