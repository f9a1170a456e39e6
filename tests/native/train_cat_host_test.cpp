// Categorical columns in the host half of the LambdaMART fit (csrc/train_host.cpp, include/mrk.h steps 2c and 5c) without HIP: the new
// config keys, the kept-id table (frequency order, ties to the lower id, max_bin - 1 of them, the refusals), the dense id -> bin table
// and the bin of a cell at its edges, a categorical node's numbering, and the cat_* lines of the model text on a hand-made tree whose
// members sit on both sides of every word boundary.  Built with ASan + UBSan by tests/test_train_cat_cpu.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/mrk.h"
#include "train_host.hpp"

using namespace mrk;

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);               \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

template <typename F>
static int status_of(F &&f, std::string *msg = nullptr) {
  try {
    f();
    return MRK_OK;
  } catch (const StatusError &e) {
    if (msg) *msg = e.what();
    return e.status;
  }
}

static TrainConfig parse(const std::string &s) { return train_parse_config(s.c_str(), s.size()); }

static std::vector<int32_t> kept_of(const std::vector<double> &v, int max_bin = 255, std::string *info = nullptr) {
  return train_kept_categories(v.data(), (int64_t)v.size(), 1, max_bin, 7, info);
}

static std::string line_of(const std::string &text, const std::string &key) {
  const size_t at = text.find("\n" + key + "=");
  if (at == std::string::npos) return "<none>";
  const size_t from = at + key.size() + 2;
  return text.substr(from, text.find('\n', from) - from);
}

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  {  // the decoder
    const TrainConfig d = parse("{}");
    CHECK(d.categorical.empty() && d.max_cat_to_onehot == 4 && d.max_cat_threshold == 32 && d.cat_smooth == 10.0 && d.cat_l2 == 10.0 && d.min_data_per_group == 100);
    const TrainConfig c = parse(R"({"categorical":[3,0,9],"max_cat_to_onehot":1,"max_cat_threshold":2,"cat_smooth":0.5,"cat_l2":0,"min_data_per_group":1})");
    CHECK((c.categorical == std::vector<int32_t>{3, 0, 9}) && c.max_cat_to_onehot == 1 && c.max_cat_threshold == 2 && c.cat_smooth == 0.5 && c.cat_l2 == 0.0 && c.min_data_per_group == 1);
    CHECK(parse(R"({"categorical":null,"cat_l2":null})").categorical.empty());
    CHECK(status_of([] { parse(R"({"categorical":3})"); }) == MRK_ERR_PARSE);
    CHECK(status_of([] { parse(R"({"categorical":[1.5]})"); }) == MRK_ERR_PARSE);
    CHECK(status_of([] { parse(R"({"categorical":["1"]})"); }) == MRK_ERR_PARSE);
    CHECK(status_of([] { parse(R"({"categorical":[2,2]})"); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([] { parse(R"({"categorical":[-1]})"); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([] { parse(R"({"max_cat_to_onehot":0})"); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([] { parse(R"({"max_cat_threshold":0})"); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([] { parse(R"({"cat_smooth":0})"); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([] { parse(R"({"cat_l2":-1})"); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([] { parse(R"({"min_data_per_group":0})"); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([] { parse(R"({"cat_smooth":"x"})"); }) == MRK_ERR_PARSE);
  }
  {  // the kept ids
    std::string info;
    CHECK(kept_of({}, 255, &info).empty() && info == "none");
    CHECK(kept_of({nan, nan, -1.0, -7.5}, 255, &info).empty() && info == "none");
    CHECK((kept_of({5.0, 2.9, nan, -0.5, 5.0, -3.0, 2.0}, 255, &info) == std::vector<int32_t>{0, 2, 5}) && info == "0:2:5");   // 2.9 -> 2, -0.5 -> 0
    CHECK((kept_of({32764.0, 0.0}) == std::vector<int32_t>{0, 32764}));
    std::string msg;
    CHECK(status_of([] { kept_of({1.0, 32765.0}); }, &msg) == MRK_ERR_UNSUPPORTED && msg.find("32765") != std::string::npos && msg.find("column 7") != std::string::npos &&
          msg.find("row 1") != std::string::npos);
    CHECK(status_of([&] { kept_of({1.0, inf}); }) == MRK_ERR_INVALID_ARG && status_of([&] { kept_of({-inf}); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([] { kept_of({1e300}); }) == MRK_ERR_UNSUPPORTED);
    // the most frequent max_bin - 1; among equal counts the lower id
    std::vector<double> v;
    for (int id = 0; id < 10; ++id)
      for (int k = 0; k < (id == 6 ? 5 : 2); ++k) v.push_back(id);
    CHECK((kept_of(v, 4) == std::vector<int32_t>{0, 1, 6}));
    CHECK(kept_of(v, 255).size() == 10 && kept_of(v, 2).size() == 1 && kept_of(v, 2)[0] == 6);
    std::vector<double> d300;
    for (int id = 0; id < 300; ++id) d300.push_back(id);
    CHECK(kept_of(d300).size() == 254 && kept_of(d300).back() == 253);
    const double strided[] = {1.0, 9.0, 2.0, 9.0, 1.0, 9.0};
    CHECK((train_kept_categories(strided, 3, 2, 255, 0) == std::vector<int32_t>{1, 2}));
    train_check_categories(strided, 3, 2, 0);
    const double far[] = {0.0, 40000.0};
    CHECK(status_of([&] { train_check_categories(far, 2, 1, 3); }, &msg) == MRK_ERR_UNSUPPORTED && msg.find("column 3") != std::string::npos);
  }
  {  // id -> bin and the bin of a cell
    CHECK(train_category_table({}).empty());
    const std::vector<int32_t> kept{0, 31, 32, 63, 64, 32764};
    const std::vector<uint8_t> tab = train_category_table(kept);
    CHECK(tab.size() == 32765);
    size_t with_bin = 0;
    for (uint8_t b : tab) with_bin += b != TRAIN_NAN_BIN;
    CHECK(with_bin == kept.size());
    const int len = (int)tab.size();
    for (size_t k = 0; k < kept.size(); ++k) CHECK(train_category_bin((double)kept[k], tab.data(), len) == (int)k);
    CHECK(train_category_bin(0.999, tab.data(), len) == 0 && train_category_bin(-0.5, tab.data(), len) == 0 && train_category_bin(-0.0, tab.data(), len) == 0);
    CHECK(train_category_bin(31.5, tab.data(), len) == 1 && train_category_bin(32764.9, tab.data(), len) == 5);
    for (double x : {nan, -1.0, -1e300, 1.0, 30.0, 33.0, 32763.0, 32765.0, 1e300, 4294967296.0, 9.3e18})
      CHECK(train_category_bin(x, tab.data(), len) == TRAIN_NAN_BIN);
    CHECK(train_category_bin(0.0, nullptr, 0) == TRAIN_NAN_BIN);   // a column with no kept category
    const std::vector<uint8_t> small = train_category_table({2});
    CHECK(small.size() == 3 && small[0] == 255 && small[1] == 255 && small[2] == 0 && train_category_bin(3.0, small.data(), 3) == TRAIN_NAN_BIN);
  }
  {  // numbering and the text: node 0 numeric, nodes 1 and 2 categorical
    const std::vector<std::vector<int32_t>> kept{{}, {0, 31, 32, 63, 64, 32764}, {3, 5}};
    TrainTree t;
    CHECK(t.split(0, 0, 1, 0.5, false, 2.0) == 1);
    uint32_t all[8] = {0x3f, 0, 0, 0, 0, 0, 0, 0}, one[8] = {0x2, 0, 0, 0, 0, 0, 0, 0};
    CHECK(t.split_cat(1, 1, all, 1.0) == 2);
    CHECK(t.split_cat(0, 2, one, 0.5) == 3);
    CHECK((t.dt == std::vector<int32_t>{8, 9, 9}) && (t.thr == std::vector<double>{0.5, 0.0, 1.0}) && (t.is_cat == std::vector<int32_t>{0, 1, 1}));
    CHECK(t.cat_mask.size() == 24 && t.cat_mask[8] == 0x3f && t.cat_mask[16] == 0x2 && t.cat_mask[0] == 0);
    CHECK((t.left == std::vector<int32_t>{2, ~1, ~0}) && (t.right == std::vector<int32_t>{1, ~2, ~3}));
    t.value = {0.1, -0.2, 0.3, 0.0}, t.weight = {1, 2, 3, 4}, t.count = {5, 6, 7, 8};
    t.ivalue = {0, 0, 0}, t.iweight = {10, 5, 5}, t.icount = {26, 13, 13};
    const std::string m = train_write_model({t}, 1, 3, {"[0:1]", "0:31:32:63:64:32764", "3:5"}, 0.1, &kept);
    CHECK(line_of(m, "num_cat") == "2" && line_of(m, "decision_type") == "8 9 9" && line_of(m, "threshold") == "0.5 0 1");
    CHECK(line_of(m, "cat_boundaries") == "0 1024 1025");
    CHECK(line_of(m, "feature_infos") == "[0:1] 0:31:32:63:64:32764 3:5");
    const std::string words = line_of(m, "cat_threshold");
    std::vector<unsigned long> w;
    for (size_t at = 0; at < words.size();) {
      w.push_back(strtoul(words.c_str() + at, nullptr, 10));
      at = words.find(' ', at);
      at = at == std::string::npos ? words.size() : at + 1;
    }
    CHECK(w.size() == 1025);
    if (w.size() == 1025) {
      CHECK(w[0] == 0x80000001ul && w[1] == 0x80000001ul && w[2] == 0x1ul && w[1023] == (1ul << (32764 % 32)) && w[1024] == (1ul << 5));
      for (size_t i = 3; i < 1023; ++i) CHECK(w[i] == 0);
    }
    CHECK(m.find("\ninternal_count=26 13 13\ncat_boundaries=") != std::string::npos && m.find("\nis_linear=0\n") != std::string::npos);
    // a tree without a categorical node: no cat_* lines, with or without the table
    TrainTree n;
    n.split(0, 0, 1, 0.5, false, 2.0);
    n.value = {0.1, -0.2}, n.weight = {1, 2}, n.count = {5, 6}, n.ivalue = {0}, n.iweight = {3}, n.icount = {11};
    const std::string a = train_write_model({n}, 1, 3, {"[0:1]", "none", "none"}, 0.1, &kept), b = train_write_model({n}, 1, 3, {"[0:1]", "none", "none"}, 0.1);
    CHECK(a == b && a.find("cat_") == std::string::npos && line_of(a, "num_cat") == "0");
  }
  if (failures) {
    printf("%d FAILURES\n", failures);
    return 1;
  }
  printf("ALL OK\n");
  return 0;
}
