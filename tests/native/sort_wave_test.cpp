// CPU: the lane rule of the wavefront-per-request ordering (csrc/sort_device.hpp sort_wave_step; rank.hip sort_wave_kernel) compiled
// for the HOST.  64 simulated lanes hold the keys of candidates l and l + 64 (pads ~0); candidate j's key is "broadcast" from its
// owner lane, four keys a round with the bounds rounded up to whole rounds as the kernel does, and every lane adds the rule's
// increments.  The counts must be the positions of std::stable_sort on (sort_key, index): a permutation, bit for bit.
//   sizes     n = 0, 1, 2, 63, 64, 65, 100, 127, 128
//   patterns  all equal; strictly descending; strictly ascending; NaNs of both signs (and payloads); +-0; +-inf; runs of ties that
//             straddle lanes 63 / 64; random draws from a few values
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#define MRK_SORT_HOST 1
#define __host__
#define __device__
#define __forceinline__ inline
static inline long long __double_as_longlong(double d) { long long v; memcpy(&v, &d, 8); return v; }
static inline double __longlong_as_double(long long v) { double d; memcpy(&d, &v, 8); return d; }
#include "sort_device.hpp"

typedef unsigned long long u64;
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static long long g_bad = 0, g_checks = 0;
#define EXPECT(cond, ...) do { ++g_checks; if (!(cond)) { if (++g_bad < 20) { printf(__VA_ARGS__); printf("\n"); } } } while (0)

static double bits(u64 b) { return __longlong_as_double((long long)b); }

// the kernel's walk over one request, on 64 host lanes
static void wave_order(const std::vector<double> &scores, std::vector<int> &order) {
  const int n = (int)scores.size();
  u64 mine0[64], mine1[64];
  int before0[64] = {0}, before1[64] = {0};
  for (int l = 0; l < 64; ++l) {
    mine0[l] = l < n ? mrk::sort_key(scores[(size_t)l]) : ~0ull;
    mine1[l] = l + 64 < n ? mrk::sort_key(scores[(size_t)l + 64]) : ~0ull;
  }
  const int n4 = (n + 3) & ~3, n_lo = n4 < 64 ? n4 : 64;
  for (int j = 0; j < n_lo; ++j)
    for (int l = 0; l < 64; ++l) {
      const mrk::SortWaveStep s = mrk::sort_wave_step(mine0[l], l, mine1[l], l + 64, mine0[j], j);
      before0[l] += s.lo;
      before1[l] += s.hi;
    }
  for (int j = 64; j < n4; ++j)
    for (int l = 0; l < 64; ++l) {
      const mrk::SortWaveStep s = mrk::sort_wave_step(mine0[l], l, mine1[l], l + 64, mine1[j - 64], j);
      before0[l] += s.lo;
      before1[l] += s.hi;
    }
  order.assign((size_t)n, -1);
  for (int l = 0; l < 64; ++l) {
    if (l < n) {
      EXPECT(before0[l] >= 0 && before0[l] < n, "n %d lane %d: position %d out of range", n, l, before0[l]);
      if (before0[l] >= 0 && before0[l] < n) order[(size_t)before0[l]] = l;
    }
    if (l + 64 < n) {
      EXPECT(before1[l] >= 0 && before1[l] < n, "n %d lane %d (+64): position %d out of range", n, l, before1[l]);
      if (before1[l] >= 0 && before1[l] < n) order[(size_t)before1[l]] = l + 64;
    }
  }
}

static void check(const char *what, const std::vector<double> &scores) {
  const int n = (int)scores.size();
  std::vector<int> got;
  wave_order(scores, got);
  std::vector<std::pair<u64, int>> ref((size_t)n);
  for (int i = 0; i < n; ++i) ref[(size_t)i] = {mrk::sort_key(scores[(size_t)i]), i};
  std::stable_sort(ref.begin(), ref.end());
  for (int p = 0; p < n; ++p) EXPECT(got[(size_t)p] == ref[(size_t)p].second, "%s n %d: place %d holds %d, expected %d", what, n, p, got[(size_t)p], ref[(size_t)p].second);
}

int main() {
  const double inf = std::numeric_limits<double>::infinity();
  const double nan_p = bits(0x7ff8000000000000ull), nan_n = bits(0xfff8000000000000ull), nan_payload = bits(0x7ff0000000000123ull), nan_np = bits(0xfff4000000000001ull);
  const int sizes[] = {0, 1, 2, 63, 64, 65, 100, 127, 128};
  static_assert(mrk::SORT_WAVE_MAX == 128, "the sizes below end at the kernel's largest request");
  for (int n : sizes) {
    std::vector<double> v((size_t)n);
    for (int i = 0; i < n; ++i) v[(size_t)i] = 1.5;
    check("all equal", v);
    for (int i = 0; i < n; ++i) v[(size_t)i] = (double)(n - i);
    check("descending", v);
    for (int i = 0; i < n; ++i) v[(size_t)i] = (double)i * 0.25 - 7.0;
    check("ascending", v);
    const double special[] = {nan_p, nan_n, nan_payload, nan_np, 0.0, -0.0, inf, -inf, 1.0, -1.0, 5e-324, -5e-324};
    for (int i = 0; i < n; ++i) v[(size_t)i] = special[i % 12];
    check("specials in turn", v);
    for (int rep = 0; rep < 20; ++rep) {
      for (int i = 0; i < n; ++i) v[(size_t)i] = special[rnd() % 12];
      check("specials at random", v);
    }
    for (int i = 0; i < n; ++i) v[(size_t)i] = (i & 1) ? 0.0 : -0.0;
    check("+-0", v);
    for (int i = 0; i < n; ++i) v[(size_t)i] = (i % 3 == 0) ? nan_n : (i % 3 == 1 ? nan_p : nan_payload);
    check("all NaN", v);
    // runs of ties that straddle lanes 63 / 64: one value over [lo, hi) around 64, other values on both sides
    for (int lo : {0, 50, 60, 62, 63}) for (int hi : {64, 65, 66, 70, 128}) {
      for (int i = 0; i < n; ++i) v[(size_t)i] = (i >= lo && i < hi) ? 3.0 : (double)(rnd() % 7);
      check("tie run across 63 / 64", v);
    }
    for (int rep = 0; rep < 50; ++rep) {
      for (int i = 0; i < n; ++i) v[(size_t)i] = (double)(rnd() % 5) - 2.0;
      check("few values", v);
      for (int i = 0; i < n; ++i) v[(size_t)i] = bits(rnd());
      check("random bits", v);
    }
  }
  printf("sort wave rule: %lld checks, %lld bad\n", g_checks, g_bad);
  return g_bad ? 1 : 0;
}
