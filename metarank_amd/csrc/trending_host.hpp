// Host half of the trending recommender (capi_trending.cpp): everything of TrendingPredictor / TrendingModel that is not the
// aggregate over the click-through history.  No HIP in here: tests/native/trending_host_test.cpp compiles this file with g++
// alone.
// Reference: ml/recommend/TrendingRecommender.scala:21-26 (InteractionWeight), :137-152 (its decoder), :39-47 (now, items),
// :89-111 (load), :115-133 (predict, save), model/Timestamp.scala:11-24, util/DurationJson.scala:9-13.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "status.hpp"

namespace mrk {

constexpr int64_t TRENDING_DAY_MS = 86400000;
constexpr int64_t TRENDING_MAX_INTERACTIONS = (int64_t(1) << 31) - 1;

// InteractionWeight(interaction, weight = 1.0, decay = 1.0, window = 30.days)
struct TrendingWeight {
  std::string interaction;
  double weight = 1.0, decay = 1.0;
  int64_t window_ms = 30 * TRENDING_DAY_MS;   // window.toMillis
  int64_t days = 30;                          // window.toDays (truncating): the length of the per-item count array
};

struct TrendingConfig {
  std::vector<TrendingWeight> weights;
  int64_t total_days() const;
  // the weight an interaction type counts for, -1: none
  int weight_of(const char *type) const;
};

// {"weights":[{"interaction":"click","weight":1.0,"decay":0.5,"window":"30d"}, ...]} - TrendingRecommender.scala:137-164.
// MRK_ERR_PARSE: malformed JSON, no weights list, a weight without interaction, a weight / decay that is not a number, a
// window that is not ([0-9]+)([smhd]); MRK_ERR_UNSUPPORTED: two weights naming one interaction (the reference's .toMap
// would let the last one's counts feed both).  A `selector` key is ignored: the host applies it before it hands
// interactions over.
TrendingConfig trending_parse_config(const char *json, size_t len);

// pow[i] = Math.pow(decay, i) for i = 0 .. days - 1, by libm's pow(decay, (double)i)
std::vector<double> trending_pow_table(double decay, int64_t days);

// The stream of a fit as the host sees it: item ids interned in order of first appearance (`ints.map(_.item).distinct`,
// :47 - the interned index is also the tie-break index of the final sortBy), the running `now` (:45: the maximal ts of ALL
// interactions) and the number of interactions.
struct TrendingStream {
  std::vector<std::string> ids;
  std::unordered_map<std::string, uint32_t> index_of;
  int64_t now_ms = 0;
  int64_t interactions = 0;
  uint32_t intern(const char *id);
  void saw(int64_t ts_ms) {
    if (interactions == 0 || ts_ms > now_ms) now_ms = ts_ms;
    ++interactions;
  }
};

// What one mrk_trending_add call must satisfy BEFORE anything of it is appended (MRK_ERR_INVALID_ARG otherwise; more than
// 2^31 - 1 interactions in one fit: MRK_ERR_UNSUPPORTED), and the weight index of each of the call's type names.
std::vector<int32_t> trending_check_call(const TrendingConfig &cfg, const TrendingStream &st, const char *const *item_ids,
                                         const char *const *type_names, int n_types, const int32_t *type_idx,
                                         const int64_t *ts_ms, int64_t n);

// TrendingModel: items in model order
struct TrendingModel {
  std::vector<std::string> ids;
  std::vector<double> scores;
  int64_t interactions = -1, now_ms = -1;   // of the fit; -1 for a loaded model
};

// TrendingModel.save (:123-133): big-endian i32 1, i32 size, per item writeUTF(id) + f64 score.  Ids are written as the
// bytes they were handed over with (the modified-UTF-8 convention of codec.cpp's readUTF); one of more than 65 535 bytes
// is what writeUTF throws on: MRK_ERR_UNSUPPORTED.
std::vector<uint8_t> trending_save(const TrendingModel &m);
// TrendingPredictor.loadSync (:90-110).  Another version: MRK_ERR_UNSUPPORTED; size <= 0, truncation, trailing bytes: MRK_ERR_PARSE.
TrendingModel trending_load(const uint8_t *bytes, size_t len);
// TrendingModel.predict (:116-121): how many of the leading items a request for `count` gets; count <= 0: MRK_ERR_INVALID_ARG
int trending_predict_n(const TrendingModel &m, int count);

}  // namespace mrk
