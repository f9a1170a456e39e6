// Host half of the similar-items index (csrc/index_host.cpp) without HIP: the reference's known answer for
// EmbeddingSimilarityModel.predict (EmbeddingSimilarityModelTest.scala:15-33), recommend's ordering, the centroid, the
// id table, the f32-lossless check and the limits.  Built with ASan + UBSan by tests/test_index_cpu.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "index_host.hpp"

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

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  {  // EmbeddingSimilarityModelTest.scala:15-33: lookup answers p1..p5, all 1.0; count = 3, items = [p2, p4] -> p1, p3, p5
    const char *names[] = {"p1", "p2", "p3", "p4", "p5"};
    KnnIds ids;
    CHECK(ids.build(names, 5).empty());
    const char *req[] = {"p2", "p4"};
    int32_t rows[] = {0, 1, 2, 3, 4};
    double score[] = {1.0, 1.0, 1.0, 1.0, 1.0};
    const int left = knn_recommend_order(rows, score, 5, knn_known_rows(ids, req, 2), 3);
    CHECK(left == 3);
    std::string got;
    for (int i = 0; i < left; ++i) got += ids.ids[(size_t)rows[i]] + (i + 1 < left ? "," : "");
    printf("known answer: %s\n", got.c_str());
    CHECK(got == "p1,p3,p5");
  }
  {  // farthest first among the nearest `count`; equal scores keep lookup order; -0.0 after 0.0 (key of -score); NaN last
    int32_t rows[] = {10, 11, 12, 13, 14, 15, 16, 17};
    double score[] = {-0.0, 0.0, 0.25, 0.25, 0.5, nan, nan, 0.75};
    const int left = knn_recommend_order(rows, score, 8, {12}, 6);   // kept: 10 11 13 14 15 16
    CHECK(left == 6);
    // sortBy(-score): keys -0.5 < -0.25 < -0.0 (from 0.0) < 0.0 (from -0.0) < NaN, NaN in lookup order
    const int32_t want[] = {14, 13, 11, 10, 15, 16};
    for (int i = 0; i < 6; ++i) CHECK(rows[i] == want[i]);
    CHECK(score[0] == 0.5 && score[1] == 0.25 && bits(score[2]) == bits(0.0) && bits(score[3]) == bits(-0.0) && std::isnan(score[4]) && std::isnan(score[5]));
    int32_t r2[] = {1, 2};
    double s2[] = {0.1, 0.2};
    CHECK(knn_recommend_order(r2, s2, 2, {1, 2}, 5) == 0);      // nothing left after the filter
    int32_t r3[] = {1, 2, 3};
    double s3[] = {0.1, 0.2, 0.3};
    CHECK(knn_recommend_order(r3, s3, 3, {}, 10) == 3 && r3[0] == 3 && r3[2] == 1);   // count larger than what is left
    int32_t r4[] = {1, 2, 3};
    double s4[] = {0.1, 0.2, 0.3};
    CHECK(knn_recommend_order(r4, s4, 3, {}, 0) == 0);
  }
  {  // id table and HnswIndexReader.lookup's choice of rows: unknown dropped, duplicates kept, request order
    const char *names[] = {"a", "b", "c", ""};
    KnnIds ids;
    CHECK(ids.build(names, 4).empty());
    CHECK(ids.row("a") == 0 && ids.row("c") == 2 && ids.row("") == 3 && ids.row("zz") == -1 && ids.row(nullptr) == -1);
    const char *req[] = {"c", "nope", "a", "c", "?"};
    const std::vector<int64_t> rows = knn_known_rows(ids, req, 5);
    CHECK(rows.size() == 3 && rows[0] == 2 && rows[1] == 0 && rows[2] == 2);
    const char *none[] = {"x", "y"};
    CHECK(knn_known_rows(ids, none, 2).empty());
    const char *dup[] = {"a", "b", "a"};
    KnnIds bad;
    CHECK(bad.build(dup, 3).find("stored twice") != std::string::npos);
    const char *nul[] = {"a", nullptr};
    CHECK(!bad.build(nul, 2).empty());
  }
  {  // centroid: sequential sum in request order, divided by the number kept (duplicates count twice)
    const double v[] = {1e16, 1.0, /**/ 1.0, 2.0, /**/ -1e16, 4.0, /**/ 1.0, 2.0};
    double c[2];
    knn_centroid(v, 4, 2, c);
    // ((1e16 + 1) + -1e16) + 1 = 1 in f64 (the first 1 is absorbed), a pairwise or sorted sum would give 2
    CHECK(bits(c[0]) == bits((((1e16 + 1.0) + -1e16) + 1.0) / 4) && c[0] == 0.25);
    CHECK(bits(c[1]) == bits(9.0 / 4));
    double one[2];
    knn_centroid(v, 1, 2, one);
    CHECK(bits(one[0]) == bits(1e16) && bits(one[1]) == bits(1.0));
  }
  {  // the f32-lossless check
    const double ok[] = {0.0, -0.0, 1.0, -2.5, (double)1e-40f, (double)std::numeric_limits<float>::denorm_min(), (double)std::numeric_limits<float>::max(),
                         (double)0.1f, std::numeric_limits<double>::infinity(), nan};
    CHECK(knn_f32_lossless(ok, sizeof(ok) / sizeof(ok[0])));
    CHECK(knn_f32_lossless(ok, 0));
    const double bad[] = {0.1, 1e-40, 1e-160, 1e150, 4.9e-324, 1.0 + 1e-12, 16777217.0};
    for (double b : bad) {
      const double two[] = {1.0, b};
      CHECK(!knn_f32_lossless(two, 2));
    }
  }
  {  // limits, each named in its message
    CHECK(knn_check_n(2048, 0).empty() && knn_check_n(2000, 48).empty() && knn_check_n(0, 0).empty());
    CHECK(knn_check_n(2049, 0).find("n + n_items <= 2048") != std::string::npos);
    CHECK(knn_check_n(2048, 1).find("n + n_items <= 2048") != std::string::npos);
    CHECK(knn_check_n(2147483647, 2147483647).find("2048") != std::string::npos);
    CHECK(!knn_check_n(-1, 0).empty());
    CHECK(knn_check_shape(1, 1).empty() && knn_check_shape(2147483647LL, 4096).empty() && knn_check_shape(0, 4).empty());
    CHECK(knn_check_shape(10, 0).find("1 <= cols <= 4096") != std::string::npos);
    CHECK(knn_check_shape(10, 4097).find("1 <= cols <= 4096") != std::string::npos);
    CHECK(knn_check_shape(2147483648LL, 4).find("rows < 2^31") != std::string::npos);
    CHECK(!knn_check_shape(-1, 4).empty());
  }
  if (failures) {
    printf("%d FAILED\n", failures);
    return 1;
  }
  printf("ALL OK\n");
  return 0;
}
