// Host half of the similar-items fit.  See als_host.hpp.
#include "als_host.hpp"

#include <algorithm>
#include <cmath>
#include <numeric>

#include "json.hpp"

namespace mrk {

AlsConfig als_parse_config(const char *json, size_t len) {
  auto bad = [](const std::string &m) -> void { throw StatusError(MRK_ERR_PARSE, "als config: " + m); };
  json::Value root;
  try {
    root = json::parse(json, len);
  } catch (const std::exception &e) {
    bad(e.what());
  }
  if (!root.is_object()) bad("not an object");
  AlsConfig cfg;
  auto integer = [&](const char *key, int &out) {
    const json::Value *v = root.find(key);
    if (!v || v->is_null()) return;   // Option[Int]: the default stays
    if (!v->is_number()) bad(std::string("'") + key + "' is not a number");
    const double d = v->as_double();
    if (!(d == std::floor(d)) || d < -2147483648.0 || d > 2147483647.0) bad(std::string("'") + key + "' is not an Int");
    out = (int)d;
  };
  auto real = [&](const char *key, float &out) {
    const json::Value *v = root.find(key);
    if (!v || v->is_null()) return;   // Option[Float]
    if (!v->is_number()) bad(std::string("'") + key + "' is not a number");
    out = v->as_float();              // decimal -> float in one rounding, as the JVM's Float parser
  };
  integer("iterations", cfg.iterations);
  integer("factors", cfg.factors);
  real("userReg", cfg.user_reg);
  real("itemRef", cfg.item_reg);      // (sic: ALSRecImpl.scala:66)
  if (const json::Value *ints = root.find("interactions"))
    if (!ints->is_null()) {
      if (!ints->is_array()) bad("'interactions' is not a list");
      for (auto &s : ints->arr)
        if (!s.is_string()) bad("'interactions' holds something that is not a string");
    }
  if (cfg.factors < 1) throw StatusError(MRK_ERR_INVALID_ARG, "als config: factors = " + std::to_string(cfg.factors) + " (at least 1)");
  if (cfg.iterations < 1) throw StatusError(MRK_ERR_INVALID_ARG, "als config: iterations = " + std::to_string(cfg.iterations) + " (at least 1)");
  return cfg;
}

void AlsStream::add(const char *const *user_ids, const char *const *item_ids, int64_t n) {
  if (n < 0) throw StatusError(MRK_ERR_INVALID_ARG, "als: negative pair count");
  if (n == 0) return;
  if (!user_ids || !item_ids) throw StatusError(MRK_ERR_INVALID_ARG, "null user_ids / item_ids");
  for (int64_t i = 0; i < n; ++i)
    if (!user_ids[i] || !item_ids[i])
      throw StatusError(MRK_ERR_INVALID_ARG, std::string("null ") + (user_ids[i] ? "item" : "user") + " id at pair " + std::to_string(i));
  if (n > ALS_MAX_PAIRS - (int64_t)pairs.size()) throw StatusError(MRK_ERR_UNSUPPORTED, "als: more than 2^31 - 1 pairs in one fit");
  auto intern = [](std::vector<std::string> &ids, std::unordered_map<std::string, uint32_t> &index_of, const char *id) {
    auto it = index_of.find(id);
    if (it != index_of.end()) return it->second;
    const uint32_t k = (uint32_t)ids.size();
    ids.emplace_back(id);
    index_of.emplace(ids.back(), k);
    return k;
  };
  pairs.reserve(pairs.size() + (size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const uint64_t u = intern(users, user_of, user_ids[i]), it = intern(items, item_of, item_ids[i]);
    pairs.push_back(u << 32 | it);
  }
}

int64_t AlsStream::distinct_pairs() const {
  std::vector<uint64_t> p(pairs);
  std::sort(p.begin(), p.end());
  return (int64_t)(std::unique(p.begin(), p.end()) - p.begin());
}

namespace {

// rows by descending length, ties by ascending index
std::vector<int32_t> by_length(const std::vector<int32_t> &off) {
  std::vector<int32_t> order(off.size() - 1);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return off[(size_t)a + 1] - off[(size_t)a] > off[(size_t)b + 1] - off[(size_t)b]; });
  return order;
}

}  // namespace

AlsProblem als_build_problem(const AlsStream &st) {
  AlsProblem pr;
  pr.users = (int64_t)st.users.size();
  pr.items = (int64_t)st.items.size();
  std::vector<uint64_t> p(st.pairs);
  std::sort(p.begin(), p.end());   // by (user, item): the CSR order
  p.erase(std::unique(p.begin(), p.end()), p.end());
  pr.nnz = (int64_t)p.size();
  pr.u_off.assign((size_t)pr.users + 1, 0);
  pr.i_off.assign((size_t)pr.items + 1, 0);
  pr.u_idx.resize(p.size());
  pr.i_idx.resize(p.size());
  for (size_t k = 0; k < p.size(); ++k) {
    pr.u_off[(size_t)(p[k] >> 32) + 1] += 1;
    pr.i_off[(size_t)(uint32_t)p[k] + 1] += 1;
    pr.u_idx[k] = (int32_t)(uint32_t)p[k];
  }
  for (size_t u = 0; u < (size_t)pr.users; ++u) pr.u_off[u + 1] += pr.u_off[u];
  for (size_t i = 0; i < (size_t)pr.items; ++i) pr.i_off[i + 1] += pr.i_off[i];
  std::vector<int32_t> at(pr.i_off.begin(), pr.i_off.end() - 1);
  for (size_t k = 0; k < p.size(); ++k) pr.i_idx[(size_t)at[(size_t)(uint32_t)p[k]]++] = (int32_t)(p[k] >> 32);   // users ascending: p is sorted by user
  // c_i = w0 * p_i^alpha / Z, Z = the sum of p_j^alpha in item order
  pr.conf.resize((size_t)pr.items);
  double z = 0.0;
  for (size_t i = 0; i < (size_t)pr.items; ++i) {
    const double pi = (double)(pr.i_off[i + 1] - pr.i_off[i]) / (double)pr.nnz;
    pr.conf[i] = std::pow(pi, ALS_ALPHA);
    z = z + pr.conf[i];
  }
  for (size_t i = 0; i < (size_t)pr.items; ++i) pr.conf[i] = ALS_W0 * pr.conf[i] / z;
  pr.u_order = by_length(pr.u_off);
  pr.i_order = by_length(pr.i_off);
  return pr;
}

namespace {

inline uint64_t mix(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}
constexpr uint64_t GOLDEN = 0x9E3779B97F4A7C15ull;

}  // namespace

double als_init_value(uint64_t seed, int matrix, uint64_t row, uint64_t col) {
  const uint64_t h = mix(mix(mix(seed + GOLDEN * (uint64_t)(matrix + 1)) + row) + col);
  const uint64_t a = mix(h + GOLDEN), b = mix(h + 2 * GOLDEN);
  const double u1 = (double)((a >> 11) + 1) * 0x1p-53, u2 = (double)(b >> 11) * 0x1p-53;
  const double radius = std::sqrt(-2.0 * std::log(u1));
  const double z = radius * std::cos(6.283185307179586 * u2);
  return ALS_INIT_STD * z;
}

void als_init_matrix(uint64_t seed, int matrix, int64_t rows, int cols, double *out) {
  for (int64_t r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) out[(size_t)r * cols + c] = als_init_value(seed, matrix, (uint64_t)r, (uint64_t)c);
}

}  // namespace mrk
