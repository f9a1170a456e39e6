// CPU unit test of the per-column distinct-token tracker (csrc/store.hpp Column::distinct), the bound features.cpp sizes the
// pre-pass hash tables by: after puts through every entry point that can write a string cell - put_string and
// put_string_list in their C-string and their KeyRef forms, the binary loader (codec.cpp load_feature_values, scalar kinds
// 0 and 3) - after lists are overwritten, erased or replaced by numbers, and after clone_items, the count of every column
// is >= the number of distinct tokens the column holds NOW and == the number it ever held (it never goes down).
// store.cpp, features.cpp and codec.cpp are compiled into the binary (ASan + UBSan); the rest is libmrk_hip.so; no device.
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "features.hpp"
#include "store.hpp"

namespace mrk { int load_feature_values(Store &store, const uint8_t *bytes, size_t len, int64_t now_ms); }
using namespace mrk;

static unsigned long long rng_state = 0x2545f4914f6cdd1dull;
static unsigned long long rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

// one pre-ttl ScalarValue record of the FeatureValue wire format: [0][scope 1 = item][utf id][utf feature][varlong ts][scalar]
static void utf(std::vector<uint8_t> &o, const std::string &s) {
  o.push_back((uint8_t)(s.size() >> 8));
  o.push_back((uint8_t)s.size());
  o.insert(o.end(), s.begin(), s.end());
}
static std::vector<uint8_t> record(const std::string &item, const std::string &col, const std::vector<std::string> &v, bool as_list) {
  std::vector<uint8_t> o{0, 1};
  utf(o, item);
  utf(o, col);
  o.push_back(5);  // timestamp
  if (as_list) {
    o.push_back(3);
    o.push_back((uint8_t)v.size());  // (< 128: one varint byte)
    for (auto &s : v) utf(o, s);
  } else {
    o.push_back(0);
    utf(o, v[0]);
  }
  return o;
}

int main() {
  const char *cfg = R"({"features": [
    {"name": "genre", "type": "string", "scope": "item", "source": "item.genre", "values": ["a", "b", "c"], "encode": "index"},
    {"name": "div", "type": "diversity", "source": "item.tags"},
    {"name": "pop", "type": "number", "scope": "item", "source": "item.pop"},
    {"name": "profile", "type": "interacted_with", "scope": "session", "interaction": "click", "field": ["item.genres", "item.actors"]}],
    "models": {"m": {"type": "lambdamart", "features": ["genre", "div", "pop", "profile"]}}})";
  Store st;
  std::unique_ptr<Registry> reg = load_config(cfg, strlen(cfg), st, false);
  const char *cols[] = {"genre", "div", "profile_genres", "profile_actors"};
  const int vocab[] = {3, 40, 500, 5000};   // a tiny, a small, a medium and a large vocabulary
  std::map<std::string, std::set<std::string>> ever;                        // column -> every token ever stored
  std::map<std::string, std::map<std::string, std::vector<std::string>>> live;   // column -> item -> its value now
  int bad = 0, checks = 0;
  auto distinct_of = [&](const char *col) { const Table &t = st.tables[SC_ITEM]; return (size_t)t.cols[(size_t)t.col_of.at(col)].distinct; };
  auto check = [&](const char *when) {
    for (const char *col : cols) {
      std::set<std::string> now;
      for (auto &kv : live[col]) now.insert(kv.second.begin(), kv.second.end());
      const size_t d = distinct_of(col);
      ++checks;
      if (d < now.size() || d != ever[col].size()) { printf("%s: column %s distinct %zu, live %zu, ever %zu\n", when, col, d, now.size(), ever[col].size()); ++bad; }
    }
  };
  check("empty store");
  auto churn = [&](int rounds, int n_items, const char *suffix) {
    for (int round = 0; round < rounds; ++round) {
      const int ci = (int)(rnd() % 4);
      const char *col = cols[ci];
      const std::string item = std::to_string(rnd() % (unsigned)n_items) + suffix, key = "item=" + item + "/" + col;
      auto token = [&] { return std::string(col) + "_" + std::to_string(rnd() % (unsigned)vocab[ci]); };
      const int n = rnd() % 6 == 0 ? (int)(rnd() % 41) : (int)(rnd() % 6);   // (longer lists leave the inline heap for the pool)
      std::vector<std::string> v;
      for (int i = 0; i < n; ++i) v.push_back(token());
      std::vector<const char *> p;
      std::vector<std::string_view> sv;
      for (auto &s : v) { p.push_back(s.c_str()); sv.push_back(s); }
      const KeyRef kr{SC_ITEM, item, col};
      switch (rnd() % 8) {
        case 0: st.put_string_list(key.c_str(), p.data(), n); break;
        case 1: st.put_string_list(kr, sv.data(), n); break;
        case 2: { const auto b = record(item, col, v, true); load_feature_values(st, b.data(), b.size(), -1); break; }
        case 3: v.assign(1, token()); st.put_string(key.c_str(), v[0].c_str()); break;
        case 4: v.assign(1, token()); st.put_string(kr, std::string_view(v[0])); break;
        case 5: { v.assign(1, token()); const auto b = record(item, col, v, false); load_feature_values(st, b.data(), b.size(), -1); break; }
        case 6: v.clear(); st.put_double(key.c_str(), 2.5); break;    // a number over a string cell
        default: v.clear(); st.erase(key.c_str()); break;
      }
      ever[col].insert(v.begin(), v.end());
      live[col][item] = v;
      if (round % 997 == 0) check("churn");
    }
  };
  churn(20000, 300, "");
  check("after puts and overwrites");
  // clones copy records: every token of a clone was counted when its original was put
  const size_t before[4] = {distinct_of(cols[0]), distinct_of(cols[1]), distinct_of(cols[2]), distinct_of(cols[3])};
  st.clone_items(2);
  for (const char *col : cols) {
    std::map<std::string, std::vector<std::string>> add;
    for (auto &kv : live[col])
      for (int k = 1; k <= 2; ++k) add[kv.first + "#" + std::to_string(k)] = kv.second;
    live[col].insert(add.begin(), add.end());
  }
  for (int c = 0; c < 4; ++c)
    if (distinct_of(cols[c]) != before[c]) { printf("clone_items moved the count of %s\n", cols[c]); ++bad; }
  check("after clones");
  churn(5000, 300, "#2");   // puts over the clones
  check("after puts over clones");
  // the tiny vocabulary was exhausted, the large one was not: the count is the vocabulary, not the number of insertions
  if (distinct_of("genre") != 3) { printf("genre: %zu distinct\n", distinct_of("genre")); ++bad; }
  if (distinct_of("profile_actors") <= 500 || distinct_of("profile_actors") > 5000) { printf("actors: %zu distinct\n", distinct_of("profile_actors")); ++bad; }
  printf("distinct: genre %zu div %zu genres %zu actors %zu; %d checks, %d bad\n", distinct_of("genre"), distinct_of("div"), distinct_of("profile_genres"),
         distinct_of("profile_actors"), checks, bad);
  return bad == 0 ? 0 : 1;
}
