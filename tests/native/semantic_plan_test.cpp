// The piece planner of the semantic fit (csrc/index_host.cpp knn_plan_pieces, mrk_index_build_texts) without HIP: hand-written
// cases and a few thousand random ones against the rule's properties.  Built with ASan + UBSan by tests/test_semantic_cpu.py.
#include <cstdio>
#include <cstdint>
#include <random>
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

static std::vector<int64_t> plan(const std::vector<int32_t> &lens, int64_t budget, int max_rows) {
  std::vector<int64_t> starts{-7, -7};   // (whatever was in there is gone)
  knn_plan_pieces(lens.data(), (int64_t)lens.size(), budget, max_rows, starts);
  return starts;
}

// the properties every plan has; returns the number of pieces
static size_t check_properties(const std::vector<int32_t> &lens, int64_t budget, int max_rows) {
  const std::vector<int64_t> s = plan(lens, budget, max_rows);
  const int64_t n = (int64_t)lens.size();
  CHECK(!s.empty() && s.front() == 0 && s.back() == n);   // consecutive pieces that cover [0, n) exactly once
  if (n == 0) CHECK(s.size() == 1);
  for (size_t k = 0; k + 1 < s.size(); ++k) {
    const int64_t lo = s[k], hi = s[k + 1];
    CHECK(hi > lo);                      // at least one sequence
    CHECK(hi - lo <= max_rows);
    int64_t sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += lens[(size_t)i];
    if (hi - lo > 1) CHECK(sum <= budget);
    if (hi < n) CHECK(hi - lo == max_rows || sum + lens[(size_t)hi] > budget);   // it could not have taken the next one
  }
  return s.size() - 1;
}

int main() {
  using V = std::vector<int64_t>;
  CHECK(KNN_PIECE_MAX_ROWS == 65535);
  // an exact fit: 3 + 4 + 3 = 10, then 10 alone, then 5 + 5
  CHECK((plan({3, 4, 3, 10, 5, 5}, 10, 100) == V{0, 3, 4, 6}));
  CHECK((plan({3, 4, 3, 10, 5, 5}, 9, 100) == V{0, 2, 3, 4, 5, 6}));
  // a budget of 1, and a budget below every length: one sequence per piece, not an error
  CHECK((plan({2, 2, 2}, 1, 100) == V{0, 1, 2, 3}));
  CHECK((plan({1, 1, 1}, 1, 100) == V{0, 1, 2, 3}));
  CHECK((plan({7, 9, 24}, 5, 100) == V{0, 1, 2, 3}));
  CHECK((plan({7, 9, 24}, 0, 100) == V{0, 1, 2, 3}));
  // a long sequence between short ones keeps its place
  CHECK((plan({2, 2, 30, 2, 2}, 8, 100) == V{0, 2, 3, 5}));
  // the row cap binds before the budget: 70 000 sequences of 2 tokens, a large budget
  {
    const std::vector<int32_t> lens(70000, 2);
    const V s = plan(lens, int64_t(1) << 40, KNN_PIECE_MAX_ROWS);
    CHECK((s == V{0, 65535, 70000}));
    CHECK(check_properties(lens, int64_t(1) << 40, KNN_PIECE_MAX_ROWS) == 2);
    CHECK(check_properties(lens, 2 * 65535 - 1, KNN_PIECE_MAX_ROWS) == 2);   // ... and one token short of it: 65 534 per piece
    CHECK((plan(lens, 2 * 65535 - 1, KNN_PIECE_MAX_ROWS)[1] == 65534));
  }
  CHECK((plan({2, 2, 2, 2, 2}, 100, 2) == V{0, 2, 4, 5}));
  CHECK((plan({2, 2, 2, 2}, 100, 1) == V{0, 1, 2, 3, 4}));
  // n = 0
  CHECK((plan({}, 10, 100) == V{0}));
  {
    std::vector<int64_t> s{5};
    knn_plan_pieces(nullptr, 0, 10, 100, s);
    CHECK((s == V{0}));
  }
  // the one-step rule the fit's loop shares with the planner
  CHECK(knn_piece_takes(0, 0, 1000, 1, 1));
  CHECK(knn_piece_takes(1, 4, 6, 10, 2) && !knn_piece_takes(1, 4, 7, 10, 2) && !knn_piece_takes(2, 4, 1, 10, 2));

  // random cases
  std::mt19937_64 rng(20240613);
  size_t pieces = 0;
  for (int round = 0; round < 4000; ++round) {
    const int n = (int)(rng() % 200);
    const int top = 1 + (int)(rng() % (round % 3 == 0 ? 4 : 40));
    std::vector<int32_t> lens((size_t)n);
    for (auto &l : lens) l = 1 + (int32_t)(rng() % (uint64_t)top);
    const int64_t budget = (int64_t)(rng() % (round % 5 == 0 ? 2000 : 120));
    const int max_rows = 1 + (int)(rng() % (round % 2 ? 300 : 12));
    pieces += check_properties(lens, budget, max_rows);
  }
  CHECK(pieces > 4000);
  if (failures) {
    printf("%d FAILURES\n", failures);
    return 1;
  }
  printf("ALL OK (%zu pieces planned)\n", pieces);
  return 0;
}
