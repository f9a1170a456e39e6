// Host half of the LambdaMART fit (csrc/train_host.cpp) without HIP: the config decoder and its refusals, the bins on the edge columns
// (none, constant, all NaN, neighbours one ulp apart, +-0.0, more distinct values than bins, a sum that overflows, an infinite cell),
// the feature subsets, the sigmoid table, the exponents, the label check, the tree numbering and the model text.  Built with
// ASan + UBSan by tests/test_train_cpu.py; the numbers are compared with tests/train_reference.py there.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <utility>
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
static int status_of(F &&f) {
  try {
    f();
    return MRK_OK;
  } catch (const StatusError &e) {
    return e.status;
  }
}

static TrainConfig parse(const std::string &s) { return train_parse_config(s.c_str(), s.size()); }

static std::vector<double> bounds_of(const std::vector<double> &v, int max_bin = 255, std::string *info = nullptr) {
  return train_bin_bounds(v.data(), (int64_t)v.size(), 1, max_bin, info);
}

int main() {
  {  // the decoder
    const TrainConfig d = parse("{}");
    CHECK(d.iterations == 100 && d.learning_rate == 0.1 && d.ndcg_cutoff == 10 && d.max_depth == 8 && d.seed == 0 && d.num_leaves == 16 && d.sampling == 0.8);
    CHECK(d.max_bin == 255 && d.truncation == 30 && d.sigma == 1.0 && d.min_data_in_leaf == 20 && d.min_sum_hessian == 1e-3 && d.lambda_l2 == 0.0 && d.early_stopping == 20);
    const TrainConfig c = parse(R"({"iterations":7,"learningRate":0.3,"numLeaves":31,"seed":-5,"debias":false,"lambda_l2":1,"sampling":null})");
    CHECK(c.iterations == 7 && c.learning_rate == 0.3 && c.num_leaves == 31 && c.seed == -5 && c.lambda_l2 == 1.0 && c.sampling == 0.8);
    CHECK(status_of([] { parse("{"); }) == MRK_ERR_PARSE);
    CHECK(status_of([] { parse("[]"); }) == MRK_ERR_PARSE);
    CHECK(status_of([] { parse(R"({"num_leaves":3})"); }) == MRK_ERR_PARSE);   // an unknown key
    CHECK(status_of([] { parse(R"({"iterations":"3"})"); }) == MRK_ERR_PARSE);
    CHECK(status_of([] { parse(R"({"iterations":1.5})"); }) == MRK_ERR_PARSE);
    CHECK(status_of([] { parse(R"({"debias":1})"); }) == MRK_ERR_PARSE);
    CHECK(status_of([] { parse(R"({"iterations":0})"); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([] { parse(R"({"max_bin":256})"); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([] { parse(R"({"sampling":0})"); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([] { parse(R"({"debias":true})"); }) == MRK_ERR_UNSUPPORTED);
    CHECK(status_of([] { parse(R"({"numLeaves":4097})"); }) == MRK_ERR_UNSUPPORTED);
    CHECK(status_of([] { parse(R"({"numLeaves":4096})"); }) == MRK_OK);
  }
  {  // bins
    std::string info;
    CHECK(bounds_of({}, 255, &info).empty() && info == "none");
    CHECK(bounds_of({2.0, 2.0, 2.0}, 255, &info).empty() && info == "none");
    const double nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(bounds_of({nan, nan}, 255, &info).empty() && info == "none");
    const std::vector<double> b3 = bounds_of({3.0, 1.0, nan, 2.0, 1.0}, 255, &info);
    CHECK(b3.size() == 2 && b3[0] == 1.5 && b3[1] == 2.5 && info == "[1:3]");
    const double x = 1.0, nx = std::nextafter(1.0, 2.0);
    const std::vector<double> bn = bounds_of({nx, x});
    CHECK(bn.size() == 1 && bn[0] == x);                       // the midpoint rounds to the upper neighbour: the lower one is the bound
    const std::vector<double> bz = bounds_of({-0.0, 0.0, 1.0});
    CHECK(bz.size() == 1 && bz[0] == 0.5);                     // -0.0 and +0.0 are one value
    const double big = std::numeric_limits<double>::max();
    const std::vector<double> bo = bounds_of({big, big / 2 * 1.5});
    CHECK(bo.size() == 1 && std::isfinite(bo[0]) && bo[0] < big);   // the sum overflows: the lower value is the bound
    std::vector<double> many;
    for (int i = 0; i < 1000; ++i) many.push_back((double)(i % 500));
    const std::vector<double> bm = bounds_of(many);
    CHECK(!bm.empty() && bm.size() <= 253);
    for (size_t i = 1; i < bm.size(); ++i) CHECK(bm[i - 1] < bm[i]);
    CHECK(bounds_of(many, 2).empty());                         // max_bin = 2: one value bin and NaN's
    std::vector<double> d254, d255;
    for (int i = 0; i < 254; ++i) d254.push_back(i);
    for (int i = 0; i < 255; ++i) d255.push_back(i);
    CHECK(bounds_of(d254).size() == 253 && bounds_of(d255).size() <= 253);
    CHECK(status_of([] { bounds_of({1.0, std::numeric_limits<double>::infinity()}); }) == MRK_ERR_INVALID_ARG);
    const double strided[] = {1.0, 9.0, 2.0, 9.0, 3.0, 9.0};
    CHECK(train_bin_bounds(strided, 3, 2, 255).size() == 2);
  }
  {  // subsets: ascending, distinct, the size rounds half up, a function of (seed, tree)
    for (int cols : {1, 2, 8, 24, 1000})
      for (int tree = 0; tree < 3; ++tree) {
        const std::vector<int32_t> s = train_feature_subset(cols, 0.8, 7, tree);
        CHECK((int)s.size() == std::max(1, (int)std::floor(cols * 0.8 + 0.5)));
        for (size_t i = 0; i < s.size(); ++i) CHECK(s[i] >= 0 && s[i] < cols && (i == 0 || s[i - 1] < s[i]));
        CHECK(s == train_feature_subset(cols, 0.8, 7, tree));
      }
    CHECK(train_feature_subset(24, 0.5, 1, 0) != train_feature_subset(24, 0.5, 1, 1));
    CHECK(train_feature_subset(24, 0.5, 1, 0) != train_feature_subset(24, 0.5, 2, 0));
    CHECK(train_feature_subset(8, 1.0, -3, 5).size() == 8 && train_feature_subset(8, 0.01, 0, 0).size() == 1);
    // what tests/test_train_cpu.py compares with the restatement: three seeds (one negative: its 32 bits count) x trees x shapes
    for (int seed : {0, 12345, -7})
      for (int tree : {0, 1, 2, 99})
        for (auto shape : {std::make_pair(24, 0.8), std::make_pair(24, 0.5), std::make_pair(7, 0.3), std::make_pair(300, 0.9)}) {
          printf("subset cols=%d sampling=%.17g seed=%d tree=%d:", shape.first, shape.second, seed, tree);
          for (int32_t c : train_feature_subset(shape.first, shape.second, seed, tree)) printf(" %d", c);
          printf("\n");
        }
  }
  {  // tables and exponents
    const SigmoidTable s = train_sigmoid_table(1.0);
    CHECK(s.t.size() == MRK_TRAIN_SIGMOID_BINS && s.lo == -25.0 && s.f == 65536.0 / 50.0);
    CHECK(s.t[0] < 1.0 && s.t[0] > 0.999 && s.t.back() > 0.0 && s.t.back() < 1e-10 && std::fabs(s.t[32768] - 0.5) < 1e-12);
    for (size_t i = 1; i < s.t.size(); ++i) CHECK(s.t[i - 1] >= s.t[i]);
    CHECK(train_exponent(0.0, 100) == 0);
    CHECK(train_exponent(1.0, 1) == 61 - 1 - 1 && train_exponent(0.75, 255) == 61 - 8 - 0 && train_exponent(3.0, 256) == 61 - 9 - 2);
    const double g = 0.7499;   // |g| <= gmax: the quantised value of every row stays below 2^(61 - bitlen(rows))
    CHECK(std::fabs(std::nearbyint(std::ldexp(g, train_exponent(0.75, 255)))) < std::ldexp(1.0, 61 - 8));
  }
  {  // labels
    const double ok[] = {0.0, 30.0, 4.0}, half[] = {0.5}, big[] = {31.0}, neg[] = {-1.0}, nn[] = {std::nan("")};
    CHECK(train_check_labels(ok, 3) == (std::vector<uint8_t>{0, 30, 4}));
    for (const double *bad : {half, big, neg, nn}) CHECK(status_of([&] { train_check_labels(bad, 1); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([] { train_check_labels(nullptr, 0); }) == MRK_ERR_INVALID_ARG);
  }
  {  // the memory budget of mrk_train_set, every figure worked out by hand from the terms in train_fit_bytes' comments
    const TrainConfig lgb = parse("{}"), xgb = parse(R"({"backend":"xgboost"})");   // 16 leaves, sampling 0.8: 8 of 10 columns; maxDepth 8
    CHECK(train_level_cap(xgb, 1000) == 128 && train_level_cap(xgb, 50) == 50 && train_level_cap(xgb, 0) == 1);
    CHECK(train_fit_bytes(lgb, 0, 1000, 10, 50) == 718752.0);     // 10 000 + 51 000 + 600 + 5 120 x 8 x 16 + 224 x 8
    CHECK(train_fit_bytes(lgb, 1, 1000, 10, 50) == 71000.0);      // 61 600 + 9 000 + 400
    CHECK(train_fit_bytes(xgb, 0, 1000, 10, 50) == 13459760.0);   // 61 600 + 2 000 + 5 232 x 10 x 2 x 128 + 224 x 10
    CHECK(train_fit_bytes(xgb, 1, 1000, 10, 50) == 73000.0);      // 61 600 + 2 000 + 9 000 + 400
    CHECK(train_fit_bytes(xgb, 0, 50, 3, 5) == 1573132.0);        // rows < 2^7, 50 nodes a level: 2 760 + 100 + 5 232 x 3 x 100 + 224 x 3
  }
  {  // numbering and the text
    TrainTree t;
    CHECK(t.split(0, 3, 1, 0.5, false, 2.0) == 1);   // node 0: leaves 0 | 1
    CHECK(t.split(1, 2, 0, 1.5, true, 1.0) == 2);    // node 1 under node 0's right: leaves 1 | 2
    CHECK(t.split(0, 3, 0, 0.25, false, 0.5) == 3);  // node 2 under node 0's left: leaves 0 | 3
    CHECK((t.left == std::vector<int32_t>{2, ~1, ~0}) && (t.right == std::vector<int32_t>{1, ~2, ~3}));
    CHECK((t.dt == std::vector<int32_t>{8, 10, 8}) && (t.depth == std::vector<int32_t>{2, 2, 2, 2}));
    t.value = {0.1, -0.2, 0.3, 0.0}, t.weight = {1, 2, 3, 4}, t.count = {5, 6, 7, 8};
    t.ivalue = {0, 0, 0}, t.iweight = {10, 5, 5}, t.icount = {26, 13, 13};
    const std::string m = train_write_model({t}, 1, 4, {"none", "[0:1]", "[0:1]", "[0:1]"}, 0.1);
    CHECK(m.rfind("tree\nversion=v4\nnum_class=1\nnum_tree_per_iteration=1\nlabel_index=0\nmax_feature_idx=3\nobjective=lambdarank\n", 0) == 0);
    CHECK(m.find("feature_names=Column_0 Column_1 Column_2 Column_3\n") != std::string::npos);
    CHECK(m.find("\nleft_child=2 -2 -1\nright_child=1 -3 -4\nleaf_value=0.10000000000000001 -0.20000000000000001 0.29999999999999999 0\n") != std::string::npos);
    CHECK(m.find("\nsplit_gain=2 1 0.5\nthreshold=0.5 1.5 0.25\ndecision_type=8 10 8\n") != std::string::npos);
    CHECK(train_write_model({t}, 0, 4, {"none", "none", "none", "none"}, 0.1).find("Tree=") == std::string::npos);
    double w = 0.0;
    CHECK(train_leaf_output(TrainSums{-8, 16, 3}, 3, 2, 0.0, 0.5, &w) == 0.125 && w == 4.0);   // -(-1) / 4 * 0.5
  }
  if (failures) {
    printf("%d FAILURES\n", failures);
    return 1;
  }
  printf("ALL OK\n");
  return 0;
}
