// Host half of the device-matched field_match columns (method term | ngram | bm25): string order, the term-frequency
// dictionary, the per-token weights and the packing of a request's query into the feature's const block.  No HIP in
// here: tests/native/match_host_test.cpp compiles this file with g++ alone.
// Reference: feature/matcher/FieldMatcher.scala:15-65 (merge walk, unique), feature/matcher/BM25Matcher.scala:20-45.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <string_view>
#include <unordered_map>

#include "rank.hpp"   // the const-block layout the device reads (MATCH_*): plain integers, no HIP

namespace mrk {

// String.compareTo over UTF-8 input: the order of the UTF-16 code units (then of the lengths).  It differs from byte
// order only where a supplementary character (surrogates D800..DFFF in UTF-16) meets U+E000..U+FFFF.  < 0, 0, > 0.
int utf16_compare(std::string_view a, std::string_view b);
// what TermMatcher / NgramMatcher.tokenize emit (FieldMatcher.unique): every token above its predecessor
bool utf16_strictly_ascending(const std::string_view *tokens, int n);

// BM25Matcher.TermFreqDic (BM25Matcher.scala:45)
struct TermFreqDic {
  std::string language;
  int32_t docs = 0;
  double avgdl = 0;
  std::unordered_map<std::string, int32_t> termfreq;
};
// "" or the message of the error: malformed JSON, a missing key, docs < 0 or past Int, avgdl not finite or not positive, a
// term frequency that is negative or past Int
std::string termfreq_parse(const char *json_bytes, size_t len, TermFreqDic &out);
// termIDF * (1 * (K1 + 1.0)) of one query token, each operation rounded on its own (BM25Matcher.scala:31-33)
double bm25_idf_w(const TermFreqDic &dic, std::string_view term);

enum MatchPack : int { MATCH_PACK_OK = 0, MATCH_PACK_TOO_MANY = 1, MATCH_PACK_NOT_ASCENDING = 2 };
// Fills the const block `cs` (match_const_count(method) doubles) of one request.  tokens == nullptr: the request has no
// query field.  ids[i]: interned id of tokens[i], 0 when the store never saw it.  `dic` is read for bm25 only.
MatchPack match_pack_ids(int method, const TermFreqDic *dic, const std::string_view *tokens, int n, const uint32_t *ids, double *cs);
// ... with the ids looked up by find_token(string_view) -> uint32_t (never inserts); a direct call, nothing on the heap
template <class Find>
MatchPack match_pack_query(int method, const TermFreqDic *dic, const std::string_view *tokens, int n, Find &&find_token, double *cs) {
  uint32_t ids[MATCH_MAX_QUERY];
  const int m = tokens && n > 0 && n <= MATCH_MAX_QUERY ? n : 0;   // past the limit match_pack_ids refuses before it reads an id
  for (int i = 0; i < m; ++i) ids[i] = find_token(tokens[i]);
  return match_pack_ids(method, dic, tokens, n, ids, cs);
}

}  // namespace mrk
