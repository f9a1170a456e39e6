// Host half of the device-matched field_match columns.  See match_host.hpp.
#include "match_host.hpp"

#include <algorithm>
#include <cmath>
#include <exception>
#include <utility>

#include "json.hpp"

namespace mrk {

namespace {

// the UTF-16 code units of a UTF-8 string, one at a time (lenient like String.hashCode's reader in features.cpp: a
// truncated or stray byte still yields a deterministic unit)
struct Utf16Reader {
  const unsigned char *p, *e;
  uint32_t low = 0;   // pending low surrogate
  explicit Utf16Reader(std::string_view s) : p((const unsigned char *)s.data()), e((const unsigned char *)s.data() + s.size()) {}
  bool next(uint32_t &unit) {
    if (low) { unit = low; low = 0; return true; }
    if (p == e) return false;
    const unsigned char c = *p;
    uint32_t cp;
    int n;
    if (c < 0x80) { cp = c; n = 1; }
    else if ((c >> 5) == 6) { cp = c & 31; n = 2; }
    else if ((c >> 4) == 14) { cp = c & 15; n = 3; }
    else { cp = c & 7; n = 4; }
    ++p;
    for (int k = 1; k < n && p != e; ++k, ++p) cp = (cp << 6) | (*p & 63);
    if (cp >= 0x10000) {
      cp -= 0x10000;
      unit = 0xD800 + ((cp >> 10) & 0x3ff);
      low = 0xDC00 + (cp & 0x3ff);
    } else {
      unit = cp;
    }
    return true;
  }
};

}  // namespace

int utf16_compare(std::string_view a, std::string_view b) {
  Utf16Reader ra(a), rb(b);
  for (;;) {
    uint32_t ua = 0, ub = 0;
    const bool ha = ra.next(ua), hb = rb.next(ub);
    if (!ha || !hb) return ha ? 1 : (hb ? -1 : 0);   // a prefix sorts first
    if (ua != ub) return ua < ub ? -1 : 1;
  }
}

bool utf16_strictly_ascending(const std::string_view *tokens, int n) {
  for (int i = 1; i < n; ++i)
    if (utf16_compare(tokens[i - 1], tokens[i]) >= 0) return false;
  return true;
}

std::string termfreq_parse(const char *json_bytes, size_t len, TermFreqDic &out) {
  if (!json_bytes || len == 0) return "term-frequency dictionary: empty input";
  try {
    const json::Value root = json::parse(json_bytes, len);
    if (!root.is_object()) return "term-frequency dictionary: a JSON object is expected";
    for (const char *key : {"language", "fields", "docs", "avgdl", "termfreq"}) {
      const json::Value *v = root.find(key);
      if (!v || v->is_null()) return std::string("term-frequency dictionary: missing '") + key + "'";
    }
    TermFreqDic d;
    if (!root.at("language").is_string()) return "term-frequency dictionary: 'language' must be a string";
    d.language = root.at("language").as_string();
    if (!root.at("fields").is_array()) return "term-frequency dictionary: 'fields' must be a list";
    const json::Value &docs = root.at("docs"), &avgdl = root.at("avgdl"), &tf = root.at("termfreq");
    if (!docs.is_number() || !avgdl.is_number()) return "term-frequency dictionary: 'docs' and 'avgdl' must be numbers";
    const double nd = docs.as_double();
    if (!(nd >= 0.0) || nd > 2147483647.0 || nd != std::floor(nd)) return "term-frequency dictionary: 'docs' must be an Int >= 0";
    d.docs = (int32_t)nd;
    d.avgdl = avgdl.as_double();
    if (!std::isfinite(d.avgdl) || !(d.avgdl > 0.0)) return "term-frequency dictionary: 'avgdl' must be finite and positive";
    if (!tf.is_object()) return "term-frequency dictionary: 'termfreq' must be an object";
    d.termfreq.reserve(tf.obj.size());
    for (const auto &kv : tf.obj) {
      if (!kv.second.is_number()) return "term-frequency dictionary: the frequency of '" + kv.first + "' is not a number";
      const double f = kv.second.as_double();
      if (!(f >= 0.0) || f > 2147483647.0 || f != std::floor(f)) return "term-frequency dictionary: the frequency of '" + kv.first + "' must be an Int >= 0";
      d.termfreq[kv.first] = (int32_t)f;   // a repeated key: the last one wins, as in a Map built from pairs
    }
    out = std::move(d);
    return "";
  } catch (const std::exception &e) {
    return std::string("term-frequency dictionary: ") + e.what();
  }
}

double bm25_idf_w(const TermFreqDic &dic, std::string_view term) {
  const double K1 = 1.2;
  thread_local std::string key;   // the map is keyed by std::string: one buffer per thread, reused, instead of one per token
  key.assign(term.data(), term.size());
  const auto it = dic.termfreq.find(key);
  const int32_t gtf = it == dic.termfreq.end() ? 0 : it->second;
  // volatile: every operation is rounded to f64 on its own whatever the compiler's contraction setting
  volatile double num = (double)(dic.docs - gtf) + 0.5;   // (freq.docs - globalTermFreq) is an Int subtraction
  volatile double den = (double)gtf + 0.5;
  volatile double q = num / den;
  volatile double arg = 1.0 + q;
  volatile double idf = std::log(arg);
  volatile double w = 1.0 * (K1 + 1.0);
  volatile double r = idf * w;
  return r;
}

MatchPack match_pack_ids(int method, const TermFreqDic *dic, const std::string_view *tokens, int n, const uint32_t *ids, double *cs) {
  const bool bm25 = method == MATCH_BM25;
  const int cap = bm25 ? MATCH_MAX_QUERY_BM25 : MATCH_MAX_QUERY;
  const int total = match_const_count(method);
  cs[0] = -1.0;
  cs[1] = 0.0;
  for (int k = 2; k < total; ++k) cs[k] = MATCH_PAD;
  if (bm25) {
    cs[MATCH_BM25_AVGDL] = dic ? dic->avgdl : 1.0;
    for (int k = 0; k < MATCH_MAX_QUERY_BM25; ++k) cs[MATCH_BM25_W + k] = 0.0;
  }
  if (!tokens || n <= 0) return MATCH_PACK_OK;
  if (n > cap) return MATCH_PACK_TOO_MANY;
  if (!utf16_strictly_ascending(tokens, n)) return MATCH_PACK_NOT_ASCENDING;
  double keys[MATCH_MAX_QUERY];
  int known = 0;
  for (int i = 0; i < n; ++i) {
    const uint32_t id = ids[i];
    if (id != 0) keys[known++] = bm25 ? (double)id * 64.0 + (double)i : (double)id;   // distinct strings have distinct ids
    if (bm25 && dic) cs[MATCH_BM25_W + i] = bm25_idf_w(*dic, tokens[i]);
  }
  std::sort(keys, keys + known);
  double *dst = cs + (bm25 ? MATCH_BM25_IDS : MATCH_TERM_IDS);
  for (int k = 0; k < known; ++k) dst[k] = keys[k];
  cs[0] = (double)known;
  cs[1] = (double)n;
  return MATCH_PACK_OK;
}

}  // namespace mrk
