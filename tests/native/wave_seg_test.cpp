// CPU: the lane mapping of the all-lanes pre-pass (csrc/wave_device.hpp: wave_nth_set, wave_seg_source, wave_seg_median_of,
// iw_task_rounds, iw_task_of).  The first two and the last two are pure functions of the lane number and of wave-uniform values, so a
// loop over the 64 lanes stands in for the wavefront; the segmented median runs on 64 host threads as tests/native/wave_test.cpp's
// (the ballot and the LDS ordering point are barriers).
//  * wave_seg_median_of against the existing wave_median_of run on each segment's values alone, bit for bit: segment widths 1, 3,
//    20, 21, 32, 64, segments filling the wavefront and not, n = 0, 1, 2, 19, 20, odd and even per segment, NaNs, all NaN, +-0,
//    duplicates, infinities.
//  * wave_seg_source against a per-segment SERIAL prefix count: lane j of a segment must get exactly the candidate whose
//    exclusive prefix count in the segment's flags is j, while j < min(limit, flags set), and nobody else may get a candidate;
//    segment widths 1, 3, 20, 21, 32, 64, segments that fill the wavefront and that do not, flags all set / none / alternating /
//    random, limits 0 .. width.
//  * the task dealing: every (k, u) with k < len and u < n is visited exactly once whatever way the rounds are claimed - one
//    wavefront taking them all, two or three taking turns by a stride, and two claimers drawing from one counter in every
//    interleaving (all schedules for short lists, random ones for long lists) - and no lane outside the tasks is valid.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include <pthread.h>
static pthread_barrier_t g_bar;
static thread_local struct { unsigned x; } threadIdx;
static unsigned char g_pred[64];
static unsigned long long ballot_impl(bool p) {
  g_pred[threadIdx.x & 63] = p ? 1 : 0;
  pthread_barrier_wait(&g_bar);
  unsigned long long m = 0;
  for (int i = 0; i < 64; ++i) m |= (unsigned long long)g_pred[i] << i;
  pthread_barrier_wait(&g_bar);   // nobody overwrites its predicate before everyone has read
  return m;
}
#define __device__
#define __forceinline__ inline
#define __ballot(p) ballot_impl(p)
#define __popcll(x) __builtin_popcountll(x)
#define __builtin_amdgcn_fence(order, scope) ((void)0)
#define __builtin_amdgcn_wave_barrier() pthread_barrier_wait(&g_bar)
static inline double __longlong_as_double(long long v) { double d; memcpy(&d, &v, 8); return d; }
static inline double __dadd_rn(double a, double b) { return a + b; }
static inline double __dsub_rn(double a, double b) { return a - b; }
static inline double __dmul_rn(double a, double b) { return a * b; }
#include <cmath>
using std::floor;
#include "wave_device.hpp"

static uint64_t rng_state = 0x243f6a8885a308d3ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static long long g_bad = 0, g_checks = 0;
#define EXPECT(cond, ...) do { ++g_checks; if (!(cond)) { if (++g_bad < 20) { printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void test_nth_set() {
  std::vector<uint64_t> masks = {1ull, 1ull << 63, ~0ull, 0x5555555555555555ull, 0xaaaaaaaaaaaaaaaaull, 0xffffffff00000000ull, 0x00000000ffffffffull, 0x8000000000000001ull};
  for (int i = 0; i < 200; ++i) masks.push_back(rnd() & rnd());
  for (int i = 0; i < 200; ++i) masks.push_back(rnd() | rnd());
  for (uint64_t m : masks) {
    int j = 0;
    for (int pos = 0; pos < 64; ++pos)
      if (m >> pos & 1) {
        const int got = mrk::wave_nth_set(m, j);
        EXPECT(got == pos, "nth_set(%016llx, %d) = %d, expected %d", (unsigned long long)m, j, got, pos);
        ++j;
      }
  }
}

static void seg_case(const std::vector<uint64_t> &balls, int width, int segs, int limit) {
  // serial restatement: per segment, walk the 64 candidates with a running prefix count
  int expect[64];
  for (int l = 0; l < 64; ++l) expect[l] = -1;
  for (int s = 0; s < segs; ++s) {
    int run = 0;
    for (int cand = 0; cand < 64; ++cand) {
      if (!(balls[(size_t)s] >> cand & 1)) continue;
      if (run < limit && run < width) expect[s * width + run] = cand;
      ++run;
    }
  }
  for (int lane = 0; lane < 64; ++lane) {
    const int seg = lane / width;
    const uint64_t mine = seg < segs ? balls[(size_t)seg] : ~0ull;   // (a lane of no segment may hold anything)
    const int got = mrk::wave_seg_source(mine, lane, width, segs, limit);
    EXPECT(got == expect[lane], "seg_source width %d segs %d limit %d lane %d: %d expected %d", width, segs, limit, lane, got, expect[lane]);
  }
}

static void test_seg_source() {
  const int widths[] = {1, 3, 20, 21, 32, 64};
  for (int width : widths) {
    const int fit = 64 / width;   // P x width equal to 64 (widths 1, 32, 64) or below it (3, 20, 21), and fewer segments than fit
    std::vector<int> seg_counts = {fit};
    if (fit > 1) seg_counts.push_back(1);
    if (fit > 2) seg_counts.push_back(fit / 2);
    for (int segs : seg_counts)
      for (int kind = 0; kind < 8; ++kind) {
        std::vector<uint64_t> balls;
        for (int s = 0; s < segs; ++s)
          balls.push_back(kind == 0 ? ~0ull : kind == 1 ? 0ull : kind == 2 ? 0x5555555555555555ull : kind == 3 ? 0xaaaaaaaaaaaaaaaaull
                          : kind == 4 ? ~0ull << (s % 64) : kind == 5 ? (rnd() & rnd() & rnd()) : rnd());
        for (int limit : {0, 1, width / 2, width - 1, width, width + 5})   // (a limit past the segment: the segment's width bounds it)
          if (limit >= 0) seg_case(balls, width, segs, limit);
      }
  }
}

// rounds handed out by `claim(who)`; every claimer runs prepass_interacted_tasks' loop for one list
static void check_cover(const std::vector<std::vector<uint32_t>> &rounds_of, uint32_t len, uint32_t n, const char *what) {
  std::vector<int> seen((size_t)len * n, 0);
  for (size_t w = 0; w < rounds_of.size(); ++w)
    for (uint32_t rd : rounds_of[w])
      for (uint32_t lane = 0; lane < 64; ++lane) {
        uint32_t k = 99999, u = 99999;
        const bool valid = mrk::iw_task_of(rd, lane, len, n, k, u);
        if (valid) {
          EXPECT(k < len && u < n, "%s len %u n %u round %u lane %u: task (%u, %u) out of range", what, len, n, rd, lane, k, u);
          if (k < len && u < n) ++seen[(size_t)u * len + k];
        } else {
          EXPECT(k == 0 && u == 0, "%s len %u n %u round %u lane %u: a lane without a task must name (0, 0)", what, len, n, rd, lane);
        }
      }
  for (uint32_t u = 0; u < n; ++u)
    for (uint32_t k = 0; k < len; ++k)
      EXPECT(seen[(size_t)u * len + k] == 1, "%s len %u n %u: task (%u, %u) visited %d times", what, len, n, k, u, seen[(size_t)u * len + k]);
}

static void test_tasks() {
  const uint32_t lens[] = {0, 1, 15, 16, 17, 63, 64, 65, 100};
  for (uint32_t len : lens)
    for (uint32_t n = 1; n <= 4; ++n) {
      const uint32_t rounds = mrk::iw_task_rounds(len, n);
      EXPECT(rounds * 64u >= len * n && (rounds == 0 || (rounds - 1) * 64u < len * n), "rounds(%u, %u) = %u", len, n, rounds);
      // 64 lanes: one wavefront takes every round; 128 / 192 lanes without a counter: rounds by stride
      for (uint32_t waves = 1; waves <= 3; ++waves) {
        std::vector<std::vector<uint32_t>> by(waves);
        for (uint32_t w = 0; w < waves; ++w)
          for (uint32_t rd = w; rd < rounds; rd += waves) by[w].push_back(rd);
        check_cover(by, len, n, "stride");
      }
      // two claimers on one counter: a schedule says who claims next; a claimer stops at its first claim past the last round,
      // so the schedule runs until both have stopped
      const uint32_t total = rounds + 2;   // claims made in all
      const uint64_t n_sched = total <= 12 ? 1ull << total : 3000;
      for (uint64_t sc = 0; sc < n_sched; ++sc) {
        const uint64_t bits = total <= 12 ? sc : rnd();
        std::vector<std::vector<uint32_t>> by(2);
        bool live[2] = {true, true};
        uint32_t counter = 0;
        for (uint32_t step = 0; live[0] || live[1]; ++step) {
          int who = (int)(bits >> (step % 64) & 1);
          if (!live[who]) who ^= 1;
          const uint32_t mine = counter++;   // wave_claim
          if (mine < rounds) by[(size_t)who].push_back(mine);
          else live[who] = false;
        }
        EXPECT(counter == total, "two claimers made %u claims, expected %u", counter, total);
        check_cover(by, len, n, "claims");
      }
    }
}

// ---- the segmented median on 64 threads
struct MedCase { int width, segs; std::vector<std::vector<double>> vals; };   // vals[s]: the values of segment s (<= width)
static std::vector<MedCase> g_med;
static double g_one[64], g_xch[64];
static double g_seg_got[64], g_ref[64];   // per lane: the segmented result; per segment: wave_median_of on that segment alone

static void *lane_main(void *arg) {
  threadIdx.x = (unsigned)(uintptr_t)arg;
  const int lane = (int)threadIdx.x;
  for (size_t c = 0; c < g_med.size(); ++c) {
    const MedCase &mc = g_med[c];
    for (int s = 0; s < mc.segs; ++s) {   // the reference: every segment by itself through the existing function
      const int n = (int)mc.vals[(size_t)s].size();
      if (lane < n) g_one[lane] = mc.vals[(size_t)s][(size_t)lane];
      pthread_barrier_wait(&g_bar);
      const double m = mrk::wave_median_of(g_one, n);
      if (lane == 0) g_ref[s] = m;
      pthread_barrier_wait(&g_bar);
    }
    const int seg = lane / mc.width, j = lane - seg * mc.width;
    const int n_mine = seg < mc.segs ? (int)mc.vals[(size_t)seg].size() : 0;
    const double held = j < n_mine ? mc.vals[(size_t)seg][(size_t)j] : -777.0;   // (a lane past its segment's values holds anything)
    // the cross-lane read: everybody publishes, everybody reads (all 64 lanes call it together, as on the device)
    const auto read_lane = [lane](double x, int src) {
      g_xch[lane] = x;
      pthread_barrier_wait(&g_bar);
      const double got = g_xch[src];
      pthread_barrier_wait(&g_bar);
      return got;
    };
    g_seg_got[lane] = mrk::wave_seg_median_of(held, n_mine, mc.width, mc.segs, read_lane);
    pthread_barrier_wait(&g_bar);
    if (lane == 0)
      for (int l = 0; l < 64; ++l) {
        const int sg = l / mc.width;
        if (sg >= mc.segs) continue;
        const bool both_nan = g_seg_got[l] != g_seg_got[l] && g_ref[sg] != g_ref[sg];
        EXPECT(both_nan || memcmp(&g_seg_got[l], &g_ref[sg], 8) == 0, "median case %zu width %d segs %d lane %d (n %zu): %.17g expected %.17g", c, mc.width,
               mc.segs, l, mc.vals[(size_t)sg].size(), g_seg_got[l], g_ref[sg]);
      }
    pthread_barrier_wait(&g_bar);
  }
  return nullptr;
}

static void test_seg_median() {
  const int widths[] = {1, 3, 20, 21, 32, 64};
  for (int width : widths) {
    const int fit = 64 / width;
    for (int segs : {fit, 1, (fit + 1) / 2})
      for (int rep = 0; rep < 14; ++rep) {
        MedCase mc{width, segs, {}};
        for (int s = 0; s < segs; ++s) {
          const int wanted[] = {0, 1, 2, 19, 20, 7, 12, width, width - 1};
          int n = rep < 9 ? wanted[(rep + s) % 9] : (int)(rnd() % (uint64_t)(width + 1));
          if (n > width) n = width;
          if (n < 0) n = 0;
          std::vector<double> v;
          for (int i = 0; i < n; ++i) {
            const uint64_t r = rnd();
            double x = (double)(int64_t)(r % 2001) / 8.0 - 125.0;            // plenty of ties
            if (rep % 3 == 1 && r % 7 == 0) x = std::nan("");
            if (rep % 4 == 2 && r % 5 == 0) x = (r & 64) ? 0.0 : -0.0;
            if (rep == 11 || (rep == 12 && s % 2)) x = std::nan("");          // nothing but NaN (in every / every other segment)
            if (rep == 10) x = 3.25;                                           // all equal
            if (rep == 13 && r % 3 == 0) x = (r & 1) ? INFINITY : -INFINITY;
            v.push_back(x);
          }
          mc.vals.push_back(v);
        }
        g_med.push_back(mc);
      }
  }
  pthread_barrier_init(&g_bar, nullptr, 64);
  pthread_t th[64];
  for (uintptr_t l = 0; l < 64; ++l) pthread_create(&th[l], nullptr, lane_main, (void *)l);
  for (int l = 0; l < 64; ++l) pthread_join(th[l], nullptr);
}

int main() {
  threadIdx.x = 0;
  test_nth_set();
  test_seg_source();
  test_tasks();
  test_seg_median();
  printf("wave segments and tasks: %lld checks, %lld bad\n", g_checks, g_bad);
  return g_bad ? 1 : 0;
}
