// Host half of the device-matched field_match columns (csrc/match_host.cpp), built with g++ -fsanitize=address,undefined by
// tests/test_fieldmatch_cpu.py.  Prints "idfw <term> <f64 bits>" lines the Python test compares with its own reference.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "match_host.hpp"

using namespace mrk;

static int failures = 0;
#define CHECK(cond)                                                            \
  do {                                                                         \
    if (!(cond)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

static bool asc(std::vector<std::string_view> v) { return utf16_strictly_ascending(v.data(), (int)v.size()); }

static const char *kDic =
    "{\"language\": \"en\", \"fields\": [\"title\"], \"docs\": 1000, \"avgdl\": 7.25, "
    "\"termfreq\": {\"common\": 900, \"rare\": 3, \"mid\": 120, \"over\": 1500, \"zero\": 0, \"caf\\u00e9\": 17}}";

int main() {
  // ---- String.compareTo order
  CHECK(utf16_compare("a", "b") < 0 && utf16_compare("b", "a") > 0 && utf16_compare("abc", "abc") == 0);
  CHECK(utf16_compare("ab", "abc") < 0 && utf16_compare("", "a") < 0 && utf16_compare("", "") == 0);
  CHECK(utf16_compare("z", "\xc3\xa9") < 0);                        // U+00E9 above ASCII
  CHECK(utf16_compare("\xc3\xa9", "\xe4\xb8\xad") < 0);              // U+00E9 < U+4E2D
  // U+FFFD (EF BF BD) against U+1F600 (F0 9F 98 80): bytes say FFFD < 1F600, UTF-16 says D83D DE00 < FFFD
  CHECK(strcmp("\xef\xbf\xbd", "\xf0\x9f\x98\x80") < 0);
  CHECK(utf16_compare("\xef\xbf\xbd", "\xf0\x9f\x98\x80") > 0);
  CHECK(utf16_compare("\xee\x80\x80", "\xf0\x90\x80\x80") > 0);      // U+E000 > U+10000 (D800 DC00)
  CHECK(utf16_compare("\xed\x9f\xbf", "\xf0\x90\x80\x80") < 0);      // U+D7FF < U+10000
  CHECK(utf16_compare("\xf0\x90\x80\x80", "\xf0\x9f\x98\x80") < 0);  // two supplementary characters: code point order
  CHECK(utf16_compare("a\xf0\x9f\x98\x80", "a\xef\xbf\xbd") < 0 && utf16_compare("\xf0\x9f\x98\x80", "\xf0\x9f\x98\x80x") < 0);
  // ---- strictly ascending
  CHECK(asc({}) && asc({"x"}) && asc({"a", "b", "c"}));
  CHECK(!asc({"a", "a"}) && !asc({"b", "a"}) && !asc({"a", "c", "b"}));
  CHECK(asc({"\xf0\x9f\x98\x80", "\xef\xbf\xbd"}) && !asc({"\xef\xbf\xbd", "\xf0\x9f\x98\x80"}));
  // ---- dictionary
  TermFreqDic dic;
  CHECK(termfreq_parse(kDic, strlen(kDic), dic).empty());
  CHECK(dic.docs == 1000 && dic.avgdl == 7.25 && dic.termfreq.size() == 6 && dic.termfreq.at("rare") == 3 && dic.termfreq.at("caf\xc3\xa9") == 17);
  auto refused = [](const std::string &text) {
    TermFreqDic d;
    d.docs = -7;
    const std::string err = termfreq_parse(text.data(), text.size(), d);
    return !err.empty() && d.docs == -7;   // an error leaves the output alone
  };
  const std::string head = "{\"language\": \"en\", \"fields\": [], ";
  CHECK(refused("{\"language\": \"en\", ") && refused("") && refused("[1, 2]") && refused("nonsense"));
  CHECK(refused(head + "\"avgdl\": 3.0, \"termfreq\": {}}"));                                   // no docs
  CHECK(refused(head + "\"docs\": 3, \"termfreq\": {}}"));                                      // no avgdl
  CHECK(refused(head + "\"docs\": 3, \"avgdl\": 3.0}"));                                        // no termfreq
  CHECK(refused("{\"fields\": [], \"docs\": 3, \"avgdl\": 3.0, \"termfreq\": {}}"));            // no language
  CHECK(refused(head + "\"docs\": 3, \"avgdl\": null, \"termfreq\": {}}"));                     // Json.fromDoubleOrNull(NaN)
  CHECK(refused(head + "\"docs\": 3, \"avgdl\": NaN, \"termfreq\": {}}"));
  CHECK(refused(head + "\"docs\": 3, \"avgdl\": 0, \"termfreq\": {}}"));
  CHECK(refused(head + "\"docs\": 3, \"avgdl\": 0.0, \"termfreq\": {}}"));
  CHECK(refused(head + "\"docs\": 3, \"avgdl\": -2.5, \"termfreq\": {}}"));
  CHECK(refused(head + "\"docs\": 3, \"avgdl\": 1e999, \"termfreq\": {}}"));
  CHECK(refused(head + "\"docs\": -1, \"avgdl\": 3.0, \"termfreq\": {}}"));
  CHECK(refused(head + "\"docs\": 4294967296, \"avgdl\": 3.0, \"termfreq\": {}}"));
  CHECK(refused(head + "\"docs\": 3, \"avgdl\": 3.0, \"termfreq\": {\"a\": -1}}"));
  CHECK(refused(head + "\"docs\": 3, \"avgdl\": 3.0, \"termfreq\": {\"a\": \"x\"}}"));
  CHECK(refused(head + "\"docs\": 3, \"avgdl\": 3.0, \"termfreq\": [1]}"));
  TermFreqDic empty;
  const std::string e = head + "\"docs\": 0, \"avgdl\": 3.0, \"termfreq\": {}}";
  CHECK(termfreq_parse(e.data(), e.size(), empty).empty() && empty.termfreq.empty() && empty.docs == 0);
  CHECK(bm25_idf_w(empty, "x") == std::log(1.0 + 0.5 / 0.5) * (1.0 * (1.2 + 1.0)));
  // ---- idf * w: printed for the Python reference (bit equality is asserted there)
  for (const char *t : {"common", "rare", "mid", "over", "zero", "caf\xc3\xa9", "absent"}) {
    const double v = bm25_idf_w(dic, t);
    unsigned long long bits;
    memcpy(&bits, &v, 8);
    printf("idfw %s %016llx\n", t, bits);
  }
  CHECK(bm25_idf_w(dic, "over") < 0.0);   // gtf > docs: a negative idf, finite
  CHECK(std::isfinite(bm25_idf_w(dic, "over")));
  // ---- const-block packing
  std::map<std::string, uint32_t> ids = {{"a", 50}, {"b", 7}, {"c", 4000000000u}, {"e", 9}};
  auto find = [&](std::string_view s) -> uint32_t { auto it = ids.find(std::string(s)); return it == ids.end() ? 0u : it->second; };
  std::vector<double> cs((size_t)match_const_count(MATCH_TERM), -5.0);
  CHECK(match_const_count(MATCH_TERM) == 130 && match_const_count(MATCH_NGRAM) == 130 && match_const_count(MATCH_BM25) == 131);
  {  // no query field, and an empty one
    CHECK(match_pack_query(MATCH_TERM, nullptr, nullptr, 0, find, cs.data()) == MATCH_PACK_OK && cs[0] == -1.0 && cs[1] == 0.0 && cs[2] == MATCH_PAD && cs[129] == MATCH_PAD);
    std::string_view none[1];
    CHECK(match_pack_query(MATCH_NGRAM, nullptr, none, 0, find, cs.data()) == MATCH_PACK_OK && cs[0] == -1.0);
  }
  {  // a, b, c, d (unknown), e -> ids ascending: 7, 9, 50, 4e9; |Q| counts d
    std::string_view q[5] = {"a", "b", "c", "d", "e"};
    CHECK(match_pack_query(MATCH_TERM, nullptr, q, 5, find, cs.data()) == MATCH_PACK_OK);
    CHECK(cs[0] == 4.0 && cs[1] == 5.0 && cs[2] == 7.0 && cs[3] == 9.0 && cs[4] == 50.0 && cs[5] == 4000000000.0 && cs[6] == MATCH_PAD);
    std::string_view only_unknown[2] = {"x", "y"};
    CHECK(match_pack_query(MATCH_TERM, nullptr, only_unknown, 2, find, cs.data()) == MATCH_PACK_OK && cs[0] == 0.0 && cs[1] == 2.0 && cs[2] == MATCH_PAD);
    std::string_view desc[2] = {"b", "a"}, dup[2] = {"a", "a"};
    CHECK(match_pack_query(MATCH_TERM, nullptr, desc, 2, find, cs.data()) == MATCH_PACK_NOT_ASCENDING);
    CHECK(match_pack_query(MATCH_TERM, nullptr, dup, 2, find, cs.data()) == MATCH_PACK_NOT_ASCENDING);
  }
  {  // bm25: id * 64 + position, weights by position
    std::vector<double> bs((size_t)match_const_count(MATCH_BM25), -5.0);
    TermFreqDic d2 = dic;
    std::string_view q[4] = {"a", "b", "common", "e"};
    ids["common"] = 8;
    CHECK(match_pack_query(MATCH_BM25, &d2, q, 4, find, bs.data()) == MATCH_PACK_OK);
    CHECK(bs[0] == 4.0 && bs[1] == 4.0 && bs[MATCH_BM25_AVGDL] == 7.25);
    CHECK(bs[3] == 7.0 * 64 + 1 && bs[4] == 8.0 * 64 + 2 && bs[5] == 9.0 * 64 + 3 && bs[6] == 50.0 * 64 + 0 && bs[7] == MATCH_PAD && bs[66] == MATCH_PAD);
    CHECK(bs[MATCH_BM25_W + 0] == bm25_idf_w(dic, "a") && bs[MATCH_BM25_W + 2] == bm25_idf_w(dic, "common") && bs[MATCH_BM25_W + 4] == 0.0 && bs[MATCH_BM25_W + 63] == 0.0);
    CHECK(4000000000.0 * 64 + 63 < MATCH_PAD);
  }
  {  // the limits: 128 / 64 pass, 129 / 65 do not
    std::vector<std::string> names;
    char buf[16];
    for (int i = 0; i < 130; ++i) { snprintf(buf, sizeof buf, "t%04d", i); names.push_back(buf); }
    std::vector<std::string_view> q(names.begin(), names.end());
    auto all = [&](std::string_view s) -> uint32_t { return (uint32_t)atoi(std::string(s.substr(1)).c_str()) + 1u; };
    CHECK(match_pack_query(MATCH_TERM, nullptr, q.data(), 128, all, cs.data()) == MATCH_PACK_OK && cs[0] == 128.0 && cs[2] == 1.0 && cs[129] == 128.0);
    CHECK(match_pack_query(MATCH_TERM, nullptr, q.data(), 129, all, cs.data()) == MATCH_PACK_TOO_MANY);
    std::vector<double> bs((size_t)match_const_count(MATCH_BM25));
    CHECK(match_pack_query(MATCH_BM25, &dic, q.data(), 64, all, bs.data()) == MATCH_PACK_OK && bs[0] == 64.0 && bs[66] == 64.0 * 64 + 63);
    CHECK(match_pack_query(MATCH_BM25, &dic, q.data(), 65, all, bs.data()) == MATCH_PACK_TOO_MANY);
  }
  if (failures == 0) printf("ALL OK\n");
  return failures == 0 ? 0 : 1;
}
