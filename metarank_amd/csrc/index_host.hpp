// Host half of the similar-items index (capi_index.cpp): everything of /recommend that is not the table scan.  No HIP
// in here: tests/native/index_host_test.cpp compiles this file with g++ alone.
// Reference: ml/recommend/embedding/HnswJavaIndex.scala:23-59 (lookup, centroid), ml/recommend/MFRecommender.scala:66-80
// (predict: filter + take), ml/Recommender.scala:36-44 (sortBy(-score)).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

namespace mrk {

constexpr int KNN_MAX_N = 2048;      // n + n_items of one lookup: what a workgroup of the selection kernel keeps in LDS
constexpr int KNN_MAX_COLS = 4096;
constexpr int64_t KNN_MAX_ROWS = (int64_t(1) << 31) - 1;

// "" when the shape is inside the limits, else the message of the MRK_ERR_INVALID_ARG that names the limit
std::string knn_check_shape(int64_t rows, int cols);
std::string knn_check_n(int n, int n_items);

// true when every value survives double -> float -> double with the same bits (-0.0 stays -0.0; a float denormal does, 1e-40
// as a double does not; a NaN does when its payload fits a float's)
bool knn_f32_lossless(const double *values, size_t n);

// item id -> row.  An id may be stored once.
struct KnnIds {
  std::vector<std::string> ids;
  std::unordered_map<std::string, int64_t> row_of;
  // "" or the message of the error (a duplicate id)
  std::string build(const char *const *names, int64_t rows);
  int64_t row(const char *id) const;   // -1: unknown
};

// HnswIndexReader.lookup's choice of rows: unknown ids dropped, duplicates kept, request order
std::vector<int64_t> knn_known_rows(const KnnIds &ids, const char *const *item_ids, int n_items);

// HnswIndexReader.centroid: per dimension the sequential sum over `vectors` (n x cols, request order) divided by n
void knn_centroid(const double *vectors, int n, int cols, double *out);

// EmbeddingSimilarityModel.predict after the lookup + Recommender.recommend's ordering: drops the results whose row is one of
// `request_rows`, keeps the first `count`, then orders them by stable sortBy(-score) under java.lang.Double.compare -
// farthest first among the nearest, NaN scores last.  Returns how many are left (rows / score are rewritten in place).
int knn_recommend_order(int32_t *rows, double *score, int n_found, const std::vector<int64_t> &request_rows, int count);

// ---- mrk_index_build_texts: how a catalogue's sequences are cut into forward passes ("pieces")
// Most sequences of one piece: the packed attention launch of the encoder puts the sequence in grid.z (encoder.hip,
// forward_impl), which HIP limits to 65 535.
constexpr int KNN_PIECE_MAX_ROWS = 65535;
// The rule, one sequence at a time: a piece that holds `count` sequences of `tokens` tokens takes one more of `len` tokens when
// it is empty (a piece always holds at least one sequence, however small the budget) or when both limits still hold.
inline bool knn_piece_takes(int64_t count, int64_t tokens, int32_t len, int64_t max_tokens, int max_rows) {
  return count == 0 || (count < max_rows && tokens + len <= max_tokens);
}
// Cuts sequences 0 .. n-1 of `lens` tokens, in order, into pieces: every piece is the longest run the rule above allows.
// starts = the first sequence of every piece, then n (pieces + 1 entries; {0} for n == 0).
void knn_plan_pieces(const int32_t *lens, int64_t n, int64_t max_tokens, int max_rows, std::vector<int64_t> &starts);

}  // namespace mrk
