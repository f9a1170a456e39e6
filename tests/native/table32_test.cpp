// CPU: the COMPACT token -> count hash tables (csrc/table32_device.hpp: 4-byte entries - 20 bits of token id, the walked-past
// mark, 11 bits of count) with the ONE-LANE stand-in for the wavefront primitives of table_test.cpp, against a std::map AND against
// the 8-byte tables of table_device.hpp entry by entry: same keys in the same entries, the same inserts refused, the same
// counts, the same walked-past marks.  Insert, lookup and the list forms; several host threads inserting into one table; a key
// counted exactly 2 047 times; token ids 1 and 2^20 - 1; a table at its load bound and past it (walked-past marks occur); a table
// that starts at an 8- but not 16-byte aligned address.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <thread>
#include <vector>

#define __device__
#define __forceinline__ inline
static inline unsigned long long __builtin_amdgcn_ballot_w64(bool p) { return p ? 1ull : 0ull; }
static inline uint32_t __umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
template <typename T> static inline T atomicAdd(T *p, T v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
template <typename T> static inline T atomicOr(T *p, T v) { return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }
template <typename T> static inline T atomicCAS(T *p, T c, T v) {
  __atomic_compare_exchange_n(p, &c, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST);
  return c;   // the value found there (== the expected one on success), like the device's atomicCAS
}
using std::min;

#include "table_device.hpp"
#include "table32_device.hpp"

using namespace mrk;

static long long checks = 0, bad = 0;
#define CHECK(cond, ...) do { ++checks; if (!(cond)) { ++bad; if (bad < 30) { printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint64_t rng_state = 0x243f6a8885a308d3ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

// a compact table of `cap` entries that starts 8 (odd = true) or 16 bytes into a 16-byte aligned block, with guard words around it
struct Tab32 {
  std::vector<uint64_t> store;   // (8-byte elements: the block is 8-byte aligned at least; the start is fixed up below)
  uint32_t *t;
  uint32_t cap;
  Tab32(uint32_t cap_, bool odd) : store(cap_ / 2 + 8, 0xa5a5a5a5a5a5a5a5ull), cap(cap_) {
    uintptr_t p = (uintptr_t)store.data();
    p = (p + 15) & ~(uintptr_t)15;
    p += odd ? 8 : 16;
    t = (uint32_t *)p;
    for (uint32_t i = 0; i < cap; ++i) t[i] = 0u;
  }
  bool guards_intact() const {
    const uint32_t *lo = (const uint32_t *)store.data(), *hi = lo + store.size() * 2;
    for (const uint32_t *q = lo; q < t; ++q) if (*q != 0xa5a5a5a5u) return false;
    for (const uint32_t *q = t + cap; q < hi; ++q) if (*q != 0xa5a5a5a5u) return false;
    return true;
  }
};

// every entry of the compact table is the entry of the wide one, narrower
static void same_tables(const Tab32 &c, const std::vector<unsigned long long> &w, const char *what) {
  for (uint32_t i = 0; i < c.cap; ++i) {
    const uint32_t e = c.t[i];
    const unsigned long long x = w[i];
    const bool ok = (e >> T32_KEY_SHIFT) == (uint32_t)x && (e & T32_COUNT_MASK) == ((uint32_t)(x >> 32) & 0x7fffffffu) &&
                    ((e & T32_WALKED) != 0u) == ((x & TABLE_WALKED) != 0ull);
    CHECK(ok, "%s: cap %u entry %u: compact %08x, wide %016llx", what, c.cap, i, e, x);
  }
}

static void against_map_and_wide() {
  const uint32_t caps[] = {8, 10, 12, 16, 38, 64, 100, 258, 1000, 2730};   // even, >= 8: what the host hands out
  long long marks = 0;
  for (uint32_t cap : caps) {
    const uint32_t usable = cap / MRK_PROBE_W * MRK_PROBE_W;
    for (int fill_pct : {0, 10, 50, 75, 90, 100, 130}) {   // 75: the load bound the host sizes for; beyond: refusals
      for (int rep = 0; rep < 6; ++rep) {
        Tab32 tab(cap, rep % 2 == 0);
        std::vector<unsigned long long> wide(cap, 0ull);
        std::map<uint32_t, uint32_t> ref;
        const uint32_t distinct = std::max<uint32_t>(fill_pct ? 1u : 0u, (uint32_t)((uint64_t)cap * fill_pct / 100));
        std::vector<uint32_t> universe;   // neighbouring ids, or ids from the whole 20-bit range with both ends in it
        for (uint32_t i = 0; i < distinct; ++i) universe.push_back(rep % 3 == 1 ? 1u + i : 1u + (uint32_t)(rnd() % T32_MAX_TOKEN));
        if (distinct >= 2 && rep % 3 != 1) { universe[0] = 1u; universe[1] = T32_MAX_TOKEN; }
        const uint32_t n_ins = std::min<uint32_t>(distinct * 3, 2047u);   // the host's rule: at most 2 047 insertions into a compact table
        for (uint32_t i = 0; i < n_ins; ++i) {
          const uint32_t tok = universe[rnd() % universe.size()];
          const bool list = i % 5 == 4;
          const bool ok = list ? table_add_list(&tok, tab.t, cap, 1u) == 0u : table_add(tab.t, cap, tok, true);
          const bool okw = list ? table_add_list(&tok, wide.data(), cap, 1u) == 0u : table_add(wide.data(), cap, tok, true);
          if (ok) ref[tok] += 1;
          CHECK(ok == okw, "cap %u: insert of %u: compact %d, wide %d", cap, tok, (int)ok, (int)okw);
          CHECK(ok || ref.size() >= usable, "table_add refused with room left: cap %u keys %zu", cap, ref.size());
          CHECK(ok || !ref.count(tok), "table_add refused a key it holds");
        }
        (void)table_add(tab.t, cap, 12345u, false);   // a lane that rides along inserts nothing
        (void)table_add(wide.data(), cap, 12345u, false);
        same_tables(tab, wide, "sequential");
        CHECK(tab.guards_intact(), "cap %u: a word outside the table was written", cap);
        size_t used = 0;
        for (uint32_t i = 0; i < cap; ++i) {
          const uint32_t e = tab.t[i];
          if (e & T32_WALKED) ++marks;
          if (!e) continue;
          ++used;
          CHECK(ref.count(e >> T32_KEY_SHIFT) && ref[e >> T32_KEY_SHIFT] == (e & T32_COUNT_MASK), "cap %u: entry %08x is not a key of the map with its count", cap, e);
        }
        CHECK(used == ref.size(), "cap %u: %zu entries for %zu keys", cap, used, ref.size());
        std::vector<uint32_t> q;   // lookups: present keys, absent keys (both ends of the id range among them), riding lanes
        for (auto &kv : ref) q.push_back(kv.first);
        for (int i = 0; i < 64; ++i) q.push_back(1u + (uint32_t)(rnd() % T32_MAX_TOKEN));
        q.push_back(1u);
        q.push_back(T32_MAX_TOKEN);
        for (uint32_t tok : q) {
          const uint32_t exp = ref.count(tok) ? ref[tok] : 0u;
          const uint32_t a = table_get(tab.t, cap, tok, true), ride = table_get(tab.t, cap, tok, false);
          CHECK(a == exp && ride == 0u, "cap %u fill %d: tok %u expected %u got %u (riding %u)", cap, fill_pct, tok, exp, a, ride);
          CHECK(a == table_get(wide.data(), cap, tok, true), "cap %u: lookup of %u differs from the wide table's", cap, tok);
        }
        std::vector<uint32_t> list;   // the list forms: sums in list order (integers: exact)
        for (int i = 0; i < 21; ++i) list.push_back(q[rnd() % q.size()]);
        for (uint32_t len : {0u, 1u, 7u, 8u, 9u, 21u}) {
          double exp = 0.5;
          for (uint32_t i = 0; i < len; ++i) exp += ref.count(list[i]) ? ref[list[i]] : 0u;
          const double s0 = table_sum_list(list.data(), tab.t, cap, len, 0.5);
          CHECK(s0 == exp, "sum_list len %u: %g expected %g", len, s0, exp);
          uint32_t head[TOK_BATCH];
          for (int t = 0; t < TOK_BATCH; ++t) head[t] = (uint32_t)t < len ? list[t] : 0u;
          double exp8 = 0.25;
          for (uint32_t i = 0; i < std::min<uint32_t>(len, TOK_BATCH); ++i) exp8 += ref.count(list[i]) ? ref[list[i]] : 0u;
          CHECK(table_sum_tokens<TOK_BATCH>(tab.t, cap, head, len, 0.25) == exp8, "sum_tokens len %u", len);
        }
      }
    }
  }
  printf("walked-past marks seen: %lld\n", marks);
  CHECK(marks > 0, "no table ever had a bucket walked past: the load-bound cases do not reach the mark");
}

// the count field's last value: one key inserted exactly 2 047 times between two neighbours in its bucket
static void count_limit() {
  for (bool odd : {false, true}) {
    Tab32 tab(8, odd);
    for (uint32_t tok : {T32_MAX_TOKEN, 1u, 77u}) {
      for (uint32_t i = 0; i < (tok == 1u ? 2047u : 3u); ++i) CHECK(table_add(tab.t, 8, tok, true), "insert refused");
    }
    CHECK(table_get(tab.t, 8, 1u, true) == 2047u, "2 047 inserts counted %u", table_get(tab.t, 8, 1u, true));
    CHECK(table_get(tab.t, 8, T32_MAX_TOKEN, true) == 3u && table_get(tab.t, 8, 77u, true) == 3u, "the neighbours of the full counter changed");
    CHECK(table_get(tab.t, 8, 2u, true) == 0u && table_get(tab.t, 8, T32_MAX_TOKEN - 1u, true) == 0u, "an absent neighbour id was found");
    uint32_t used = 0;
    for (uint32_t i = 0; i < 8; ++i) used += tab.t[i] ? 1u : 0u;
    CHECK(used == 3u && tab.guards_intact(), "entries %u", used);
  }
}

// Several host threads - each a one-lane wavefront - inserting into ONE table at the same time (table_test.cpp's hammer)
static void hammer() {
  int twice = 0;
  for (int round = 0; round < 300; ++round) {
    const uint32_t cap = (uint32_t[]){16, 24, 40, 64, 130}[round % 5];
    const int n_thr = 6, per = (int)(cap * 3 / 4 / n_thr) * 4;
    const uint32_t universe = std::max(2u, cap * 3 / 4 - 2);
    Tab32 tab(cap, round % 2 == 0);
    std::vector<std::vector<uint32_t>> toks(n_thr);
    std::vector<int> refused(n_thr, 0);
    const uint32_t base = round % 3 == 0 ? T32_MAX_TOKEN - universe : 1000u;   // (the top of the id range too)
    for (int t = 0; t < n_thr; ++t)
      for (int i = 0; i < per; ++i) toks[t].push_back(base + 1u + (uint32_t)(rnd() % universe));
    std::vector<std::thread> th;
    int go = 0;
    for (int t = 0; t < n_thr; ++t)
      th.emplace_back([&, t] {
        while (!__atomic_load_n(&go, __ATOMIC_ACQUIRE)) {}
        for (uint32_t tok : toks[t]) if (!table_add(tab.t, cap, tok, true)) refused[t] += 1;
      });
    __atomic_store_n(&go, 1, __ATOMIC_RELEASE);
    for (auto &x : th) x.join();
    std::map<uint32_t, uint32_t> ref;
    for (auto &v : toks) for (uint32_t tok : v) ref[tok] += 1;
    size_t used = 0;
    for (uint32_t i = 0; i < cap; ++i) used += tab.t[i] ? 1 : 0;
    if (used > ref.size()) ++twice;
    for (int t = 0; t < n_thr; ++t) CHECK(!refused[t], "concurrent insert refused (cap %u, %zu keys)", cap, ref.size());
    for (auto &kv : ref) {
      const uint32_t got = table_get(tab.t, cap, kv.first, true);
      CHECK(got == kv.second, "concurrent inserts of %u: count %u, expected %u (cap %u)", kv.first, got, kv.second, cap);
    }
    CHECK(tab.guards_intact(), "cap %u: a word outside the table was written", cap);
  }
  CHECK(twice == 0, "%d concurrent rounds left a key in two entries", twice);
}

int main() {
  static_assert(T32_MAX_TOKEN == (1u << 20) - 1u && T32_COUNT_MASK == 2047u, "the entry format of DESIGN.md §2");
  hammer();
  count_limit();
  against_map_and_wide();
  printf("compact tables, PROBE_W %d: %lld checks, %lld bad\n", (int)MRK_PROBE_W, checks, bad);
  return bad ? 1 : 0;
}
