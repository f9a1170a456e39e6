// The xgboost backend in the host half of the LambdaMART fit (csrc/train_host.cpp, include/mrk.h steps 2x, 5x, 7x) without HIP: the
// config keys and which backend owns which, the f32 bin finder (the bound AT the upper neighbour, cells that share an f32, +-0, NaN,
// the refusal of a cell that is not finite as an f32), the bin of a cell at a bound and one f32 ulp beside it, the row sample, the
// breadth-first numbering, the refusal of a node without a finite weight and the JSON text on a one-split tree and a depth-15 chain.
// Built with ASan + UBSan by tests/test_train_xgb_cpu.py.
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

static std::vector<double> bounds_of(const std::vector<double> &v, int max_bin = 255) { return train_bin_bounds_f32(v.data(), (int64_t)v.size(), 1, max_bin, 3); }

static size_t count_of(const std::string &text, const std::string &what) {
  size_t n = 0;
  for (size_t at = text.find(what); at != std::string::npos; at = text.find(what, at + 1)) ++n;
  return n;
}

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  {  // the decoder
    const TrainConfig d = parse(R"({"backend":"xgboost"})");
    CHECK(d.backend == TRAIN_BACKEND_XGBOOST && d.lambda == 1.0 && d.gamma == 0.0 && d.min_child_weight == 1.0 && d.max_depth == 8 && d.sampling == 0.8);
    CHECK(parse("{}").backend == TRAIN_BACKEND_LIGHTGBM && parse(R"({"backend":"lightgbm","numLeaves":31})").num_leaves == 31 && parse(R"({"backend":null})").backend == 0);
    const TrainConfig c = parse(R"({"backend":"xgboost","lambda":0,"gamma":0.5,"min_child_weight":0.001,"maxDepth":15,"sampling":1})");
    CHECK(c.lambda == 0.0 && c.gamma == 0.5 && c.min_child_weight == 0.001 && c.max_depth == 15 && c.sampling == 1.0);
    std::string msg;
    for (const char *key : {"numLeaves", "min_data_in_leaf", "min_sum_hessian", "lambda_l2", "max_cat_to_onehot", "max_cat_threshold", "cat_smooth", "cat_l2", "min_data_per_group"}) {
      CHECK(status_of([&] { parse(std::string(R"({"backend":"xgboost",")") + key + "\":5}"); }, &msg) == MRK_ERR_INVALID_ARG && msg.find(key) != std::string::npos);
      CHECK(parse(std::string(R"({"backend":"xgboost",")") + key + "\":null}").backend == TRAIN_BACKEND_XGBOOST);
    }
    for (const char *key : {"lambda", "gamma", "min_child_weight"}) {
      CHECK(status_of([&] { parse(std::string("{\"") + key + "\":1}"); }, &msg) == MRK_ERR_INVALID_ARG && msg.find(key) != std::string::npos);
      CHECK(status_of([&] { parse(std::string(R"({"backend":"xgboost",")") + key + "\":-1}"); }, &msg) == MRK_ERR_INVALID_ARG && msg.find(key) != std::string::npos);
      CHECK(status_of([&] { parse(std::string(R"({"backend":"xgboost",")") + key + "\":\"x\"}"); }) == MRK_ERR_PARSE);
    }
    CHECK(status_of([] { parse(R"({"backend":"catboost"})"); }) == MRK_ERR_INVALID_ARG && status_of([] { parse(R"({"backend":1})"); }) == MRK_ERR_PARSE);
    CHECK(status_of([] { parse(R"({"backend":"xgboost","categorical":[1]})"); }) == MRK_ERR_UNSUPPORTED && parse(R"({"backend":"xgboost","categorical":[]})").categorical.empty());
    CHECK(status_of([] { parse(R"({"backend":"xgboost","debias":true})"); }) == MRK_ERR_UNSUPPORTED);
    CHECK(status_of([] { parse(R"({"backend":"xgboost","maxDepth":16})"); }) == MRK_ERR_INVALID_ARG && parse(R"({"maxDepth":16})").max_depth == 16);
    CHECK(status_of([] { parse(R"({"backend":"xgboost","colsample_bytree":1})"); }) == MRK_ERR_PARSE);
  }
  {  // step 2x
    const float one = 1.0f, below = std::nextafterf(one, 0.0f), above = std::nextafterf(one, 2.0f);
    const std::vector<double> b = bounds_of({2.0, (double)below, 1.0, (double)above, 1.0 + 1e-12, 1.0 - 1e-12, nan});
    CHECK((b == std::vector<double>{1.0, (double)above, 2.0}));   // 1 +- 1e-12 are 1.0f: four values, the bound IS the upper neighbour
    CHECK(train_bin_f32((double)below, b.data(), 3) == 0 && train_bin_f32(1.0 - 1e-12, b.data(), 3) == 1 && train_bin_f32(1.0, b.data(), 3) == 1);
    CHECK(train_bin_f32(1.0 + 1e-12, b.data(), 3) == 1 && train_bin_f32((double)above, b.data(), 3) == 2 && train_bin_f32(2.0, b.data(), 3) == 3 && train_bin_f32(1e30, b.data(), 3) == 3);
    CHECK(train_bin_f32(nan, b.data(), 3) == TRAIN_NAN_BIN && train_bin_f32(-5.0, b.data(), 3) == 0);
    for (double x : {(double)below, 1.0 - 1e-12, 1.0, 1.0 + 1e-12, (double)above, 1.5, 2.0})   // candidate c sends left exactly (float) x < bound[c]
      for (int c = 0; c < 3; ++c) CHECK((train_bin_f32(x, b.data(), 3) <= c) == ((float)x < (float)b[(size_t)c]));
    CHECK((bounds_of({-0.0, 0.0, nan, 0.0}).empty()) && (bounds_of({-0.0, 1.0}) == std::vector<double>{1.0}) && bounds_of({nan, nan}).empty() && bounds_of({}).empty());
    std::vector<double> many;   // pairwise distinct f64 cells on 10 shared f32 values
    for (int i = 0; i < 1000; ++i) many.push_back((double)(i % 10 + 1) + (double)(i / 10) * 1e-13);
    CHECK(bounds_of(many).size() == 9);
    many.clear();
    for (int i = 0; i < 1000; ++i) many.push_back((double)i * 0.37);
    const std::vector<double> q = bounds_of(many);   // the quantile walk: at most max_bin - 2 bounds, ascending, every one an f32 cell of the column
    CHECK(q.size() == 253);
    for (size_t i = 0; i < q.size(); ++i) CHECK((double)(float)q[i] == q[i] && (i == 0 || q[i - 1] < q[i]));
    CHECK(bounds_of(many, 4).size() == 2);
    std::string msg;
    CHECK(status_of([&] { bounds_of({1.0, 1e39}); }, &msg) == MRK_ERR_INVALID_ARG && msg.find("column 3") != std::string::npos && msg.find("row 1") != std::string::npos);
    CHECK(status_of([&] { bounds_of({-1e39}); }) == MRK_ERR_INVALID_ARG && status_of([&] { bounds_of({inf}); }) == MRK_ERR_INVALID_ARG);
    CHECK(bounds_of({3.4028234e38, 0.0}).size() == 1);   // FLT_MAX stays finite
    const std::vector<double> cells{nan, 1.0, 1e39};
    CHECK(status_of([&] { train_check_f32_cells(cells.data(), 3, 1, 5); }, &msg) == MRK_ERR_INVALID_ARG && msg.find("column 5") != std::string::npos && msg.find("row 2") != std::string::npos);
    CHECK(status_of([&] { train_check_f32_cells(cells.data(), 2, 1, 5); }) == MRK_OK);
  }
  {  // step 7x
    int in = 0;
    for (uint64_t r = 0; r < 10000; ++r) in += train_row_sampled(0.5, 3, 7, r) ? 1 : 0;
    CHECK(in > 4700 && in < 5300);
    CHECK(train_row_sampled(1.0, 3, 7, 12345) && train_row_sampled(0.5, 3, 7, 42) == train_row_sampled(0.5, 3, 7, 42));
    int differ = 0;
    for (uint64_t r = 0; r < 1000; ++r) differ += train_row_sampled(0.5, 3, 7, r) != train_row_sampled(0.5, 3, 8, r) ? 1 : 0;
    CHECK(differ > 300);
  }
  {  // a one-split tree, a refusal, the text
    TrainXgbTree t;
    CHECK(t.add(2147483647) == 0 && t.num_nodes() == 1);
    t.split(0, 4, 7, 1.5f, true, 0.25f);
    CHECK(t.num_nodes() == 3 && t.left[0] == 1 && t.right[0] == 2 && t.parent[1] == 0 && t.parent[2] == 0 && t.default_left[0] == 1);
    t.weigh(0, TrainSums{-8, 16, 10}, 2, 3, 1.0, 0.1);
    t.weigh(1, TrainSums{-4, 8, 5}, 2, 3, 1.0, 0.1);
    t.weigh(2, TrainSums{-4, 8, 5}, 2, 3, 1.0, 0.1);
    CHECK(t.base_weight[0] == (float)(2.0 / 3.0) && t.sum_hessian[0] == 2.0f && t.cond[0] == 1.5f);   // -(-2) / (2 + 1); a split node keeps its bound
    CHECK(t.base_weight[1] == 0.5f && t.cond[1] == (float)(0.5 * 0.1) && t.sum_hessian[2] == 1.0f);
    std::string msg;
    CHECK(status_of([&] { t.weigh(2, TrainSums{-4, 0, 5}, 2, 3, 0.0, 0.1); }, &msg) == MRK_ERR_INVALID_ARG && msg.find("node 2") != std::string::npos);
    const std::string text = train_write_xgb_model({t}, 1, 6);
    CHECK(text.find(R"("split_conditions":[1.5,0.0500000007,0.0500000007],)") != std::string::npos);
    CHECK(text.find(R"("parents":[2147483647,0,0],)") != std::string::npos && text.find(R"("left_children":[1,-1,-1],)") != std::string::npos);
    CHECK(text.find(R"("loss_changes":[0.25,0,0],)") != std::string::npos && text.find(R"("split_indices":[4,0,0],"split_type":[0,0,0],)") != std::string::npos);
    CHECK(text.find(R"("base_score":"5E-1")") != std::string::npos && text.find(R"("num_feature":"6")") != std::string::npos && text.find(R"("num_trees":"1")") != std::string::npos);
    CHECK(text.find(R"("iteration_indptr":[0,1],"tree_info":[0],)") != std::string::npos && text.find(' ') == std::string::npos && text.find('\n') == std::string::npos);
    CHECK(text.substr(text.size() - 20) == R"(},"version":[2,1,0]})");
    const std::string none = train_write_xgb_model({t}, 0, 6);   // a fit without a tree
    CHECK(none.find(R"("num_trees":"0"},"iteration_indptr":[0],"tree_info":[],"trees":[]})") != std::string::npos);
  }
  {  // a chain of depth 15: the right child splits again, ids in breadth-first order
    TrainXgbTree t;
    t.add(2147483647);
    int node = 0;
    for (int d = 0; d < TRAIN_XGB_MAX_DEPTH; ++d) {
      t.split(node, d % 3, d, (float)d, false, 1.0f);
      CHECK(t.left[(size_t)node] == 2 * d + 1 && t.right[(size_t)node] == 2 * d + 2);
      node = t.right[(size_t)node];
    }
    CHECK(t.num_nodes() == 31);
    for (int n = 0; n < t.num_nodes(); ++n) t.weigh(n, TrainSums{n - 15, 4, 1}, 0, 0, 1.0, 1.0);
    const std::string text = train_write_xgb_model({t, t}, 2, 3);
    CHECK(count_of(text, "\"tree_param\"") == 2 && count_of(text, "\"num_nodes\":\"31\"") == 2 && text.find("\"id\":1,") != std::string::npos);
    CHECK(text.find("\"parents\":[2147483647,0,0,2,2,4,4,") != std::string::npos);
  }
  if (failures) {
    printf("%d FAILURES\n", failures);
    return 1;
  }
  printf("ALL OK\n");
  return 0;
}
