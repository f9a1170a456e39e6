// Host half of the trending recommender (csrc/trending_host.cpp) without HIP: config decoding and its refusals, interning in
// order of first appearance, the running `now`, the pow tables, the argument checks of one add call, predict, and the
// bitstream under mutation (every truncation of a small model is refused, never read past its end).  Built with ASan + UBSan
// by tests/test_trending_cpu.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/mrk.h"
#include "trending_host.hpp"

using namespace mrk;

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);               \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

static uint64_t bits(double v) {
  uint64_t b;
  memcpy(&b, &v, 8);
  return b;
}

template <typename F>
static int status_of(F &&f) {
  try {
    f();
    return MRK_OK;
  } catch (const StatusError &e) {
    return e.status;
  }
}

static TrendingConfig parse(const std::string &s) { return trending_parse_config(s.c_str(), s.size()); }

int main() {
  {  // the decoder: defaults 1.0 / 1.0 / 30 days (TrendingRecommender.scala:21-26), toDays truncates
    const TrendingConfig c = parse(R"({"weights":[{"interaction":"click"},{"interaction":"buy","weight":5,"decay":0.5,"window":"36h"},
                                     {"interaction":"view","weight":null,"decay":null,"window":null},{"interaction":"x","window":"90m"}],"selector":{"accept":true}})");
    CHECK(c.weights.size() == 4);
    CHECK(c.weights[0].weight == 1.0 && c.weights[0].decay == 1.0 && c.weights[0].window_ms == 30 * TRENDING_DAY_MS && c.weights[0].days == 30);
    CHECK(c.weights[1].weight == 5.0 && c.weights[1].decay == 0.5 && c.weights[1].window_ms == 36LL * 3600 * 1000 && c.weights[1].days == 1);
    CHECK(c.weights[2].weight == 1.0 && c.weights[2].days == 30);
    CHECK(c.weights[3].window_ms == 90LL * 60 * 1000 && c.weights[3].days == 0);
    CHECK(c.total_days() == 61);
    CHECK(c.weight_of("buy") == 1 && c.weight_of("nope") == -1);
    CHECK(parse(R"({"weights":[]})").weights.empty());
  }
  {  // refusals
    CHECK(status_of([] { parse(R"({"weights":[{"interaction":"a"},{"interaction":"b"},{"interaction":"a"}]})"); }) == MRK_ERR_UNSUPPORTED);
    CHECK(status_of([] { parse(R"({"weights":[{"interaction":"a")"); }) == MRK_ERR_PARSE);
    CHECK(status_of([] { parse("[]"); }) == MRK_ERR_PARSE);
    CHECK(status_of([] { parse("{}"); }) == MRK_ERR_PARSE);
    CHECK(status_of([] { parse(R"({"weights":[{"weight":1}]})"); }) == MRK_ERR_PARSE);
    CHECK(status_of([] { parse(R"({"weights":[{"interaction":"a","window":"3w"}]})"); }) == MRK_ERR_PARSE);
    CHECK(status_of([] { parse(R"({"weights":[{"interaction":"a","window":"d"}]})"); }) == MRK_ERR_PARSE);
    CHECK(status_of([] { parse(R"({"weights":[{"interaction":"a","window":30}]})"); }) == MRK_ERR_PARSE);
    CHECK(status_of([] { parse(R"({"weights":[{"interaction":"a","decay":"x"}]})"); }) == MRK_ERR_PARSE);
  }
  {  // pow tables: libm's pow(decay, i); pow(0, 0) = 1; overflow to Infinity
    const std::vector<double> p = trending_pow_table(0.5, 4);
    CHECK(p.size() == 4 && p[0] == 1.0 && p[1] == 0.5 && p[2] == 0.25 && p[3] == 0.125);
    const std::vector<double> z = trending_pow_table(0.0, 3);
    CHECK(z[0] == 1.0 && z[1] == 0.0 && z[2] == 0.0);
    const std::vector<double> big = trending_pow_table(1e200, 3);
    CHECK(big[0] == 1.0 && big[1] == 1e200 && std::isinf(big[2]));
    const std::vector<double> d = trending_pow_table(0.9, 30);
    for (int i = 0; i < 30; ++i) CHECK(bits(d[(size_t)i]) == bits(std::pow(0.9, (double)i)));
    CHECK(trending_pow_table(0.5, 0).empty());
  }
  {  // interning in order of first appearance; now = the maximal ts of everything seen, negative values included
    TrendingStream st;
    const char *ids[] = {"p3", "p1", "p3", "p2", "p1", ""};
    const int64_t ts[] = {-50, -70, -10, -30, -20, -40};
    std::vector<uint32_t> got;
    for (int i = 0; i < 6; ++i) {
      got.push_back(st.intern(ids[i]));
      st.saw(ts[i]);
    }
    CHECK((got == std::vector<uint32_t>{0, 1, 0, 2, 1, 3}));
    CHECK((st.ids == std::vector<std::string>{"p3", "p1", "p2", ""}));
    CHECK(st.now_ms == -10 && st.interactions == 6);
    printf("interned: %s,%s,%s now=%lld\n", st.ids[0].c_str(), st.ids[1].c_str(), st.ids[2].c_str(), (long long)st.now_ms);
  }
  {  // one add call: the weight of each type name; an index outside the call's table, a null id, null arrays
    const TrendingConfig c = parse(R"({"weights":[{"interaction":"buy"},{"interaction":"click"}]})");
    TrendingStream st;
    const char *ids[] = {"a", "b"};
    const char *names[] = {"click", "view", "buy"};
    const int32_t idx[] = {2, 1};
    const int64_t ts[] = {1, 2};
    const std::vector<int32_t> w = trending_check_call(c, st, ids, names, 3, idx, ts, 2);
    CHECK((w == std::vector<int32_t>{1, -1, 0}));
    const int32_t over[] = {0, 3}, under[] = {-1, 0};
    CHECK(status_of([&] { trending_check_call(c, st, ids, names, 3, over, ts, 2); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([&] { trending_check_call(c, st, ids, names, 3, under, ts, 2); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([&] { trending_check_call(c, st, ids, names, 0, idx, ts, 2); }) == MRK_ERR_INVALID_ARG);
    const char *hole[] = {"a", nullptr};
    CHECK(status_of([&] { trending_check_call(c, st, hole, names, 3, idx, ts, 2); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([&] { trending_check_call(c, st, nullptr, names, 3, idx, ts, 2); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([&] { trending_check_call(c, st, ids, names, 3, idx, ts, -1); }) == MRK_ERR_INVALID_ARG);
    CHECK(trending_check_call(c, st, nullptr, nullptr, 0, nullptr, nullptr, 0).empty());
    st.interactions = TRENDING_MAX_INTERACTIONS - 1;
    CHECK(status_of([&] { trending_check_call(c, st, ids, names, 3, idx, ts, 2); }) == MRK_ERR_UNSUPPORTED);
  }
  {  // the bitstream: round trip, layout, and every mutation
    TrendingModel m;
    m.ids = {"p2", "", "caf\xc3\xa9"};
    m.scores = {3.0, -0.0, std::numeric_limits<double>::quiet_NaN()};
    const std::vector<uint8_t> b = trending_save(m);
    const uint8_t head[] = {0, 0, 0, 1, 0, 0, 0, 3, 0, 2, 'p', '2', 0x40, 0x08, 0, 0, 0, 0, 0, 0, 0, 0, 0x80};
    CHECK(b.size() == 8 + (2 + 2 + 8) + (2 + 0 + 8) + (2 + 5 + 8));
    CHECK(memcmp(b.data(), head, sizeof head) == 0);
    const TrendingModel r = trending_load(b.data(), b.size());
    CHECK(r.ids == m.ids && r.interactions == -1 && r.now_ms == -1);
    for (size_t i = 0; i < 3; ++i) CHECK(bits(r.scores[i]) == bits(m.scores[i]));
    CHECK(trending_save(r) == b);
    int refused = 0;
    for (size_t cut = 0; cut < b.size(); ++cut) {   // an exact-size heap copy: ASan sees any read past the cut
      std::vector<uint8_t> t(b.begin(), b.begin() + (long)cut);
      refused += status_of([&] { trending_load(t.data(), t.size()); }) == MRK_ERR_PARSE;
    }
    CHECK(refused == (int)b.size());
    printf("truncations refused: %d of %zu\n", refused, b.size());
    std::vector<uint8_t> t = b;
    t.push_back(0);
    CHECK(status_of([&] { trending_load(t.data(), t.size()); }) == MRK_ERR_PARSE);            // trailing garbage
    t = b; t[3] = 2;
    CHECK(status_of([&] { trending_load(t.data(), t.size()); }) == MRK_ERR_UNSUPPORTED);      // another version
    t = b; t[0] = 0xff;
    CHECK(status_of([&] { trending_load(t.data(), t.size()); }) == MRK_ERR_UNSUPPORTED);
    t = b; t[7] = 0;
    CHECK(status_of([&] { trending_load(t.data(), t.size()); }) == MRK_ERR_PARSE);            // size 0
    t = b; t[4] = 0x80;
    CHECK(status_of([&] { trending_load(t.data(), t.size()); }) == MRK_ERR_PARSE);            // size < 0
    t = b; t[4] = 0x7f; t[5] = t[6] = t[7] = 0xff;
    CHECK(status_of([&] { trending_load(t.data(), t.size()); }) == MRK_ERR_PARSE);            // a size that must not be allocated
    t = b; t[7] = 4;
    CHECK(status_of([&] { trending_load(t.data(), t.size()); }) == MRK_ERR_PARSE);            // one item more than there is
    t = b; t[7] = 2;
    CHECK(status_of([&] { trending_load(t.data(), t.size()); }) == MRK_ERR_PARSE);            // one fewer: the last is trailing
    t = b; t[8] = 0xff; t[9] = 0xff;
    CHECK(status_of([&] { trending_load(t.data(), t.size()); }) == MRK_ERR_PARSE);            // an id length past the end
    CHECK(status_of([&] { trending_load(nullptr, 0); }) == MRK_ERR_PARSE);
    // writeUTF's limit
    TrendingModel big;
    big.ids = {std::string(65535, 'a')};
    big.scores = {1.0};
    CHECK(trending_load(trending_save(big).data(), 8 + 2 + 65535 + 8).ids[0].size() == 65535);
    big.ids[0].push_back('a');
    CHECK(status_of([&] { trending_save(big); }) == MRK_ERR_UNSUPPORTED);
    // predict
    CHECK(trending_predict_n(m, 2) == 2 && trending_predict_n(m, 3) == 3 && trending_predict_n(m, 100) == 3);
    CHECK(status_of([&] { trending_predict_n(m, 0); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([&] { trending_predict_n(m, -4); }) == MRK_ERR_INVALID_ARG);
  }
  if (failures) {
    printf("%d FAILURES\n", failures);
    return 1;
  }
  printf("ALL OK\n");
  return 0;
}
