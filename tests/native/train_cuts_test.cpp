// Step 2d's cut rule without HIP (csrc/train_host.hpp train_cut_at / train_cut_target: the body the device's train_cuts_kernel calls)
// against steps 2 and 2x themselves (train_bin_bounds, train_bin_bounds_f32 on the UNSORTED cells): the cells are prepared and sorted
// the way the device does it - NaN dropped, -0.0 as +0.0, narrowed to f32 for 2x - and the cuts are taken lane by lane from the sorted
// array, as the kernel takes them: with at most max_bin - 2 changes every change (given as its own target, and again by the chain
// "the cut before + 1"), else one target per i with the first missing cut ending them and a repeated cut dropped.  Every comparison
// is by bit pattern.  Built with ASan + UBSan by tests/test_train_device_cpu.py.
#include <algorithm>
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
static int cases = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);               \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

static std::vector<double> sorted_cells(const std::vector<double> &cells, bool f32) {
  std::vector<double> v;
  for (double x : cells) {
    if (x != x) continue;
    if (f32) x = (double)(float)x;
    if (x == 0.0) x = 0.0;
    v.push_back(x);
  }
  std::sort(v.begin(), v.end());
  return v;
}

// what train_cuts_kernel does, one loop iteration per lane; chain: the few-changes branch by "the cut before + 1" instead of the list
static std::vector<double> cuts_of_sorted(const std::vector<double> &v, int max_bin, bool f32, bool chain, bool *quantile_branch = nullptr) {
  const int64_t m = (int64_t)v.size();
  auto at = [&](int64_t p) {
    if (p < 0 || p >= m) {   // the function never reads outside [0, m)
      printf("FAIL read at %lld of %lld\n", (long long)p, (long long)m);
      ++failures;
      return 0.0;
    }
    return v[(size_t)p];
  };
  std::vector<int64_t> change;
  for (int64_t p = 1; p < m; ++p)
    if (v[(size_t)p] != v[(size_t)p - 1]) change.push_back(p);
  std::vector<double> out;
  if (quantile_branch) *quantile_branch = (int64_t)change.size() > max_bin - 2;
  if ((int64_t)change.size() <= max_bin - 2) {
    int64_t prev = 0;
    for (size_t k = 0; k < change.size(); ++k) {
      double b = 0.0;
      const int64_t p = train_cut_at(at, m, chain ? prev + 1 : change[k], f32, &b);
      CHECK(p == change[k]);
      out.push_back(b);
      prev = p;
    }
    if (chain) {
      double b = 0.0;
      CHECK(train_cut_at(at, m, prev + 1, f32, &b) == m);   // after the last change: none
    }
    return out;
  }
  std::vector<int64_t> cut((size_t)max_bin, m);
  std::vector<double> bound((size_t)max_bin, 0.0);
  for (int i = 1; i <= max_bin - 2; ++i) cut[(size_t)i] = train_cut_at(at, m, train_cut_target(m, max_bin, i), f32, &bound[(size_t)i]);
  for (int i = 1; i <= max_bin - 2; ++i) {
    if (i > 1) CHECK(cut[(size_t)i] >= cut[(size_t)i - 1]);   // what lets a lane look at its neighbour alone
    if (cut[(size_t)i] < m && (i == 1 || cut[(size_t)i - 1] != cut[(size_t)i])) out.push_back(bound[(size_t)i]);
  }
  return out;
}

static bool same_bits(const std::vector<double> &a, const std::vector<double> &b) {
  return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * 8) == 0);
}

// both backends, both forms of the few-changes branch; -> did the f64 case take the quantile branch
static bool check_column(const char *name, const std::vector<double> &cells, int max_bin) {
  bool quantile = false;
  for (int f32 = 0; f32 < 2; ++f32) {
    bool finite = true;
    for (double x : cells) finite = finite && !(f32 && x == x && std::isinf((float)x));
    if (!finite) continue;   // (1.7e308 is no f32: step 2x refuses the column)
    const std::vector<double> want = f32 ? train_bin_bounds_f32(cells.data(), (int64_t)cells.size(), 1, max_bin, 0) : train_bin_bounds(cells.data(), (int64_t)cells.size(), 1, max_bin);
    const std::vector<double> v = sorted_cells(cells, f32 != 0);
    for (int chain = 0; chain < 2; ++chain) {
      bool q = false;
      const std::vector<double> got = cuts_of_sorted(v, max_bin, f32 != 0, chain != 0, &q);
      if (!f32) quantile = q;
      ++cases;
      if (!same_bits(got, want)) {
        printf("FAIL %s max_bin=%d f32=%d chain=%d: %zu bounds, want %zu\n", name, max_bin, f32, chain, got.size(), want.size());
        ++failures;
      }
    }
  }
  return quantile;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}
static void shuffle(std::vector<double> &v) {
  for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[(size_t)(next_u64() % i)]);
}

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const int max_bins[] = {2, 3, 4, 16, 255};
  for (int max_bin : max_bins) {
    // m = 0, 1, 2
    check_column("empty", {}, max_bin);
    check_column("all NaN", {nan, nan, nan}, max_bin);
    check_column("one cell", {2.5}, max_bin);
    check_column("one cell and NaN", {nan, 2.5, nan}, max_bin);
    check_column("two equal", {2.5, 2.5}, max_bin);
    check_column("two cells", {2.5, -1.0}, max_bin);
    {  // exactly max_bin - 1 distinct values: every change is a cut; exactly max_bin: the quantile rule
      std::vector<double> a, b;
      for (int k = 0; k < max_bin - 1; ++k)
        for (int r = 0; r < 3; ++r) a.push_back((double)k * 0.5);
      for (int k = 0; k < max_bin; ++k)
        for (int r = 0; r < 3; ++r) b.push_back((double)k * 0.5);
      shuffle(a), shuffle(b);
      CHECK(!check_column("max_bin - 1 distinct", a, max_bin));
      CHECK(check_column("max_bin distinct", b, max_bin));
    }
    {  // a run of equal values across several quantile positions: the cuts repeat and are dropped
      std::vector<double> c;
      for (int k = 0; k < 300; ++k) c.push_back((double)k);
      for (int k = 0; k < 2000; ++k) c.push_back(150.0);
      shuffle(c);
      CHECK(check_column("a run across quantile positions", c, max_bin));
    }
    {  // the last run reaches the end: the targets inside it have no cut (bin_cuts' `it == end` break)
      std::vector<double> c;
      for (int k = 0; k < 300; ++k) c.push_back((double)k);
      for (int k = 0; k < 3000; ++k) c.push_back(1e6);
      shuffle(c);
      CHECK(check_column("a last run to the end", c, max_bin));
      std::vector<double> d;   // and a first run from the start
      for (int k = 0; k < 300; ++k) d.push_back((double)k);
      for (int k = 0; k < 3000; ++k) d.push_back(-1e6);
      shuffle(d);
      CHECK(check_column("a first run from the start", d, max_bin));
    }
    {  // neighbours one ulp apart: the midpoint is no value below b, the bound falls back to a
      const double x = 0.3;
      check_column("one ulp apart", {x, std::nextafter(x, 1.0), x, std::nextafter(x, 1.0), std::nextafter(x, 0.0)}, max_bin);
      std::vector<double> c;
      double y = 1.0;
      for (int k = 0; k < 600; ++k, y = std::nextafter(y, 2.0)) c.push_back(y);
      shuffle(c);
      CHECK(check_column("600 neighbours", c, max_bin));
    }
    {  // two values near 1.7e308: a + b overflows
      check_column("overflowing sum", {1.7e308, 1.6e308, 1.7e308, -1.7e308, -1.6e308}, max_bin);
      std::vector<double> c;
      for (int k = 0; k < 400; ++k) c.push_back(1.7e308 - (double)k * 4e292), c.push_back(-1.7e308 + (double)k * 4e292);
      shuffle(c);
      CHECK(check_column("400 overflowing sums", c, max_bin));
    }
    // -0.0 beside +0.0: one value
    check_column("zeros", {-0.0, 0.0, -0.0, 1.0, -1.0, 0.0}, max_bin);
    check_column("zeros alone", {-0.0, 0.0, -0.0}, max_bin);
    {  // cells that share an f32 but not an f64, NaN among them
      std::vector<double> c;
      for (int k = 0; k < 1000; ++k) c.push_back(k % 7 == 0 ? nan : 1.0 + (double)(next_u64() % 4096) * 0x1.0p-40);
      check_column("f32 neighbours", c, max_bin);
    }
    {  // plain random columns, a few sizes
      for (int n : {255, 256, 257, 4097}) {
        std::vector<double> c;
        for (int k = 0; k < n; ++k) c.push_back((double)(int64_t)(next_u64() % 2000001) * 1e-3 - 1000.0);
        check_column("random", c, max_bin);
        std::vector<double> d;
        for (int k = 0; k < n; ++k) d.push_back((double)(next_u64() % 10));
        check_column("ten values", d, max_bin);
        std::vector<double> e;
        for (int k = 0; k < n; ++k) e.push_back((double)(next_u64() % 2));
        check_column("two values", e, max_bin);
      }
    }
  }
  printf("%d comparisons\n", cases);
  if (failures) {
    printf("%d FAILURES\n", failures);
    return 1;
  }
  printf("ALL OK\n");
  return 0;
}
