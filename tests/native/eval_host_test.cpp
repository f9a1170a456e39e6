// Native driver of csrc/eval_host.cpp (no HIP): built with g++ -fsanitize=address,undefined by tests/test_eval_cpu.py.
// Binning at the kernel thresholds, piece planning with a group straddling pieces, refused offsets and metrics, and the lg table,
// the gains and noopArray against constants.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "../../include/mrk.h"
#include "eval_host.hpp"

using namespace mrk;

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
      exit(1);                                                    \
    }                                                             \
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

static std::vector<int64_t> offsets_of(const std::vector<int64_t> &lens) {
  std::vector<int64_t> off{0};
  for (int64_t n : lens) off.push_back(off.back() + n);
  return off;
}

int main() {
  // binning at 64 / 65 and 4096 / 4097, each list in group order
  {
    const std::vector<int64_t> off = offsets_of({1, 64, 65, 4096, 4097, 63, 8200, 100});
    const EvalShape sh = eval_check_groups(off.data(), 8);
    CHECK(sh.rows == 1 + 64 + 65 + 4096 + 4097 + 63 + 8200 + 100 && sh.max_len == 8200);
    EvalBins b = eval_bins(off.data(), 8, 64);
    CHECK((b.wave == std::vector<int32_t>{0, 1, 5}));
    CHECK((b.group == std::vector<int32_t>{2, 3, 7}) && b.group_max_len == 4096);
    CHECK((b.big == std::vector<int32_t>{4, 6}));
    b = eval_bins(off.data(), 8, 0);   // MRK_EVAL_WAVE_MAX=0: everything one workgroup sorts goes to the workgroup kernel
    CHECK(b.wave.empty() && (b.group == std::vector<int32_t>{0, 1, 2, 3, 5, 7}) && (b.big == std::vector<int32_t>{4, 6}));
    b = eval_bins(off.data(), 8, 1000);   // clamped to one wavefront
    CHECK((b.wave == std::vector<int32_t>{0, 1, 5}));
    b = eval_bins(off.data(), 8, -3);
    CHECK(b.wave.empty());
    b = eval_bins(off.data(), 8, 63);
    CHECK((b.wave == std::vector<int32_t>{0, 5}) && b.group.front() == 1);
  }
  // refused offsets
  {
    const int64_t ok[] = {0, 3, 5}, late[] = {1, 3, 5}, empty[] = {0, 3, 3}, down[] = {0, 3, 2}, neg[] = {0, -1, 5};
    const int64_t wrapped[] = {0, std::numeric_limits<int64_t>::max(), std::numeric_limits<int64_t>::min()};   // a sum that overflowed
    const int64_t huge[] = {0, EVAL_MAX_GROUP + 1}, most[] = {0, EVAL_MAX_GROUP};
    CHECK(status_of([&] { eval_check_groups(ok, 2); }) == MRK_OK);
    CHECK(status_of([&] { eval_check_groups(nullptr, 2); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([&] { eval_check_groups(ok, 0); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([&] { eval_check_groups(ok, -1); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([&] { eval_check_groups(late, 2); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([&] { eval_check_groups(empty, 2); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([&] { eval_check_groups(down, 2); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([&] { eval_check_groups(neg, 2); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([&] { eval_check_groups(wrapped, 2); }) != MRK_OK);
    CHECK(status_of([&] { eval_check_groups(huge, 1); }) == MRK_ERR_UNSUPPORTED);
    CHECK(status_of([&] { eval_check_groups(most, 1); }) == MRK_OK);
    CHECK(status_of([&] { eval_check_groups(ok, EVAL_MAX_GROUPS + 1); }) == MRK_ERR_UNSUPPORTED);   // judged before an offset is read
  }
  // metrics and cutoffs
  {
    const int good[] = {MRK_METRIC_NDCG, MRK_METRIC_MAP, MRK_METRIC_MRR}, cut[] = {10, 0, 5}, bad[] = {0, 3, 1}, low[] = {-1, 0, 0}, negcut[] = {10, -1, 5};
    CHECK(status_of([&] { eval_check_metrics(good, cut, 3); }) == MRK_OK);
    CHECK(status_of([&] { eval_check_metrics(bad, cut, 3); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([&] { eval_check_metrics(low, cut, 3); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([&] { eval_check_metrics(good, negcut, 3); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([&] { eval_check_metrics(good, cut, 0); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([&] { eval_check_metrics(nullptr, cut, 3); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([&] { eval_check_metrics(good, nullptr, 3); }) == MRK_ERR_INVALID_ARG);
  }
  // piece planning: 10 rows in groups of {4, 6}, pieces of 3 rows - the cuts at 3, 6, 9 fall inside both groups
  {
    std::vector<EvalPiece> p = eval_pieces(10, 24, 3);
    CHECK(p.size() == 4);
    int64_t at = 0;
    for (const EvalPiece &pc : p) {
      CHECK(pc.row0 == at && pc.rows >= 1 && pc.rows <= 3);
      at += pc.rows;
    }
    CHECK(at == 10 && p[3].rows == 1);
    p = eval_pieces(10, 24, 10);
    CHECK(p.size() == 1 && p[0].row0 == 0 && p[0].rows == 10);
    p = eval_pieces(10, 24, 0);   // the default: 64 MiB of 24 f64 columns
    CHECK(p.size() == 1);
    const int64_t per = EVAL_PIECE_BYTES / (8 * 24);
    p = eval_pieces(2 * per + 1, 24, 0);
    CHECK(p.size() == 3 && p[0].rows == per && p[1].row0 == per && p[2].row0 == 2 * per && p[2].rows == 1);
    p = eval_pieces(5, 0, 0);     // no columns: still finite pieces
    CHECK(p.size() == 1 && p[0].rows == 5);
    p = eval_pieces(int64_t(5) << 31, 1, int64_t(1) << 40);   // a piece never exceeds what the scorer counts with int
    CHECK(p.size() == 6 && p[0].rows == INT32_MAX);
    CHECK(eval_pieces(0, 3, 0).empty());
  }
  // lg, gains, noopArray, mean against constants
  {
    const std::vector<double> lg = eval_lg_table(7);
    CHECK(lg.size() == 7 && lg[0] == 1.0 && lg[2] == 2.0 && lg[6] == 3.0);
    CHECK(lg[1] == std::log2(3.0) && std::fabs(lg[1] - 1.584962500721156) < 1e-15);
    CHECK(eval_lg_table(0).empty());
    const double y[] = {0.0, 1.0, 2.0, 3.0, 4.0, -1.0, 0.5};
    double g[7];
    uint8_t r[7];
    eval_pack_labels(y, 7, true, g, r);
    CHECK(g[0] == 0.0 && g[1] == 1.0 && g[2] == 3.0 && g[3] == 7.0 && g[4] == 15.0 && g[5] == -0.5 && g[6] == std::pow(2.0, 0.5) - 1.0);
    CHECK(r[0] == 0 && r[1] == 1 && r[4] == 1 && r[5] == 0 && r[6] == 1);
    eval_pack_labels(y, 7, false, g, r);
    for (int i = 0; i < 7; ++i) CHECK(g[i] == y[i]);
    const double tiny[] = {1e-300};   // relevant, though its gain rounds to 0
    eval_pack_labels(tiny, 1, true, g, r);
    CHECK(g[0] == 0.0 && r[0] == 1);
    const double nan[] = {1.0, std::nan("")}, inf[] = {std::numeric_limits<double>::infinity()};
    CHECK(status_of([&] { eval_pack_labels(nan, 2, false, g, r); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([&] { eval_pack_labels(inf, 1, true, g, r); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([&] { eval_pack_labels(nullptr, 1, true, g, r); }) == MRK_ERR_INVALID_ARG);
    const int64_t off[] = {0, 4, 5, 8};
    double noop[8];
    eval_noop_array(off, 3, noop);
    const double want[] = {1.0, 0.75, 0.5, 0.25, 1.0, 1.0, 2.0 / 3.0, 1.0 / 3.0};
    for (int i = 0; i < 8; ++i) CHECK(noop[i] == want[i]);
    const double v[] = {0.1, 0.2, 0.3};
    CHECK(eval_mean(v, 3) == (0.1 + 0.2 + 0.3) / 3.0 && eval_mean(v, 1) == 0.1);
  }
  printf("ALL OK\n");
  return 0;
}
