// util/DurationJson.scala:9-13: ([0-9]+)([smhd]) -> milliseconds.  Shared by the feature registry (features.cpp) and the
// trending recommender's config (trending_host.cpp); no dependencies, so the HIP-free host halves can include it.
#pragma once
#include <cstdint>
#include <string>

namespace mrk {

inline bool parse_duration_ms(const std::string &s, int64_t &out) {
  if (s.size() < 2) return false;
  int64_t n = 0;
  for (size_t i = 0; i + 1 < s.size(); ++i) {
    if (s[i] < '0' || s[i] > '9') return false;
    n = n * 10 + (s[i] - '0');
    if (n > 100000000000LL) return false;  // (FiniteDuration is bounded too: ~292 years; 1e11 days is far outside)
  }
  switch (s.back()) {
    case 's': out = n * 1000; return true;
    case 'm': out = n * 60 * 1000; return true;
    case 'h': out = n * 3600 * 1000; return true;
    case 'd': out = n * 86400 * 1000; return true;
    default: return false;
  }
}

}  // namespace mrk
