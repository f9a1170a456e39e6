// Host half of the similar-items fit (capi_als.cpp): everything of MFPredictor.fit / ALSRecImpl.train that is not the ALS
// iterations.  No HIP in here: tests/native/als_host_test.cpp compiles this file with g++ alone.
// Reference: ml/recommend/MFRecommender.scala:44-63 (the UIRT lines), ml/recommend/mf/ALSRecImpl.scala:18-41 (the fixed
// settings), :46-81 (ALSConfig and its decoder).  The algorithm is eALS (He, Zhang, Kan, Chua, SIGIR 2016).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "status.hpp"

namespace mrk {

constexpr int ALS_MAX_FACTORS = 256;                        // K: what a sweep's workgroup keeps of its own row in LDS beside the staged rows
constexpr int64_t ALS_MAX_PAIRS = (int64_t(1) << 31) - 1;   // pairs of one fit (CSR offsets are int32 on the device)
constexpr double ALS_W0 = 128.0;                            // rec.eals.overall, ALSRecImpl.scala:27
constexpr double ALS_ALPHA = 0.4;                           // rec.eals.ratio, :28
constexpr double ALS_INIT_STD = 0.01;

// ALSConfig(interactions = Nil, iterations = 100, factors = 100, userReg = 0.01f, itemReg = 0.01f, store, selector)
struct AlsConfig {
  int iterations = 100, factors = 100;
  float user_reg = 0.01f, item_reg = 0.01f;
  double lambda_user() const { return (double)user_reg; }   // a Java float in f64 arithmetic: (double)(float)x
  double lambda_item() const { return (double)item_reg; }
};

// ALSConfig's decoder, ALSRecImpl.scala:60-81.  The item regulariser is read from the key "itemRef" (:66) - a key "itemReg" is
// ignored, as there; reproduced, not corrected.  `interactions` (a list of strings), `store` and `selector` are the host's: it
// filters before it hands pairs over.  MRK_ERR_PARSE: malformed JSON, not an object, a field of the wrong type (iterations /
// factors that are no integers, regularisers that are no numbers, interactions that is no list of strings);
// MRK_ERR_INVALID_ARG: factors or iterations < 1.  (factors above ALS_MAX_FACTORS is judged at fit.)
AlsConfig als_parse_config(const char *json, size_t len);

// The pairs of a fit as the host sees them: user and item ids interned in order of first appearance over all adds, every
// (user, item) as one 64-bit key (user << 32 | item) in arrival order.
struct AlsStream {
  std::vector<std::string> users, items;
  std::unordered_map<std::string, uint32_t> user_of, item_of;
  std::vector<uint64_t> pairs;
  // appends n pairs; a null id, a null array with n > 0, n < 0 (MRK_ERR_INVALID_ARG) or more than ALS_MAX_PAIRS pairs
  // (MRK_ERR_UNSUPPORTED) fail the call with nothing appended
  void add(const char *const *user_ids, const char *const *item_ids, int64_t n);
  int64_t distinct_pairs() const;
};

// R_u as CSR and R_i as CSC over the distinct pairs, the confidences, and the order the sweeps walk their rows in
struct AlsProblem {
  int64_t users = 0, items = 0, nnz = 0;
  std::vector<int32_t> u_off, u_idx;      // users + 1 offsets; per user its items ascending
  std::vector<int32_t> i_off, i_idx;      // items + 1 offsets; per item its users ascending
  std::vector<double> conf;               // c_i = w0 * p_i^alpha / sum_j p_j^alpha, p_i = n_i / nnz; the sum in item order, pow is libm's
  std::vector<int32_t> u_order, i_order;  // rows by descending length, ties by ascending index: a sweep starts its longest rows first
};
AlsProblem als_build_problem(const AlsStream &st);

// The documented counter-based generator of the initial factors.  value(seed, matrix, row, col), matrix 0 = users, 1 = items:
//   mix(x): x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31     (all mod 2^64)
//   h  = mix(mix(mix(seed + 0x9E3779B97F4A7C15 * (matrix + 1)) + row) + col)
//   a  = mix(h + 0x9E3779B97F4A7C15), b = mix(h + 2 * 0x9E3779B97F4A7C15)
//   u1 = ((a >> 11) + 1) * 2^-53  in (0, 1],  u2 = (b >> 11) * 2^-53  in [0, 1)
//   value = 0.01 * (sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2))                               (Box-Muller; libm's log / cos)
double als_init_value(uint64_t seed, int matrix, uint64_t row, uint64_t col);
void als_init_matrix(uint64_t seed, int matrix, int64_t rows, int cols, double *out);   // rows x cols, row-major

}  // namespace mrk
