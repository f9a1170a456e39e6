// Host test of the serving queue's synchronisation pieces (csrc/serve_sync.hpp): the reader gate that lets mrk_serve_stop free a
// server under mrk_rank's lock-free readers, the slot pool, the overflow window.  Includes serve_sync.hpp alone and builds with g++
// without a HIP include path.  Built and run by tests/test_serve_sync_cpu.py twice: under ASan + UBSan and under TSan.
#include "serve_sync.hpp"

#include <cstdio>
#include <thread>

using namespace mrk;

static int failures = 0;
#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      ++failures;                                                    \
    }                                                                \
  } while (0)

// 4 readers enter, dereference what the pointer publishes, leave; the stopper withdraws the pointer, turns the epoch, waits and frees
// the object.  A reader that could still hold the withdrawn pointer keeps the stopper waiting: no use-after-free, no race.
static void test_gate() {
  struct Obj { std::atomic<long> hits{0}; int tag; };
  ReaderGate gate;
  std::atomic<Obj *> hot{nullptr};
  std::atomic<bool> done{false};
  std::atomic<long> seen{0}, wrong{0};
  std::vector<std::thread> readers;
  for (int t = 0; t < 4; ++t)
    readers.emplace_back([&] {
      while (!done.load()) {
        const int cell = gate.enter();
        if (Obj *o = hot.load(std::memory_order_seq_cst)) {
          o->hits.fetch_add(1, std::memory_order_relaxed);
          if (o->tag != 42) wrong.fetch_add(1);
          seen.fetch_add(1, std::memory_order_relaxed);
        }
        gate.leave(cell);
      }
    });
  const int rounds = 4000;
  for (int r = 0; r < rounds; ++r) {
    Obj *o = new Obj();
    o->tag = 42;
    hot.store(o, std::memory_order_seq_cst);
    if ((r & 7) == 0) std::this_thread::yield();   // (some rounds give the readers time to find it)
    hot.store(nullptr, std::memory_order_seq_cst);
    gate.turn_and_wait([] { std::this_thread::yield(); });
    o->tag = 0;   // nobody reads it any more: a plain write, then the free
    delete o;
  }
  done.store(true);
  for (auto &t : readers) t.join();
  CHECK(wrong.load() == 0);
  CHECK(gate.readers[0].load() == 0 && gate.readers[1].load() == 0);
  CHECK(gate.epoch.load() == (std::uint32_t)rounds);
  std::printf("gate: %d rounds, %ld reads of a live object\n", rounds, seen.load());
}

static void test_pool() {
  bool retired[3] = {false, false, false};
  int busy_calls = 0;
  auto is_retired = [&](int s) { return retired[s]; };
  auto busy = [&] { ++busy_calls; };
  {
    SlotPool p;
    p.fill(3);
    CHECK(p.all_back());
    CHECK(p.take(is_retired, busy) == 0 && p.take(is_retired, busy) == 1 && p.take(is_retired, busy) == 2);
    CHECK(!p.all_back() && busy_calls == 0);
    CHECK(p.take(is_retired, busy) == -1 && busy_calls == 1);   // every slot busy: the caller is told, under the mutex
    p.give_back(1, is_retired);
    p.give_back(2, is_retired);
    CHECK(p.take(is_retired, busy) == 2);                        // a given-back slot is on top
    p.give_back(2, is_retired);
    p.give_back(0, is_retired);
    CHECK(p.all_back() && p.dead_slots == 0);
    // a slot whose gang is retired is skipped and counted dead on take ...
    retired[0] = true;
    CHECK(p.take(is_retired, busy) == 2 && p.dead_slots == 1 && p.free_slots.size() == 1);
    // ... and on give-back
    retired[2] = true;
    p.give_back(2, is_retired);
    CHECK(p.dead_slots == 2 && p.free_slots.size() == 1 && p.all_back());
    CHECK(p.take(is_retired, busy) == 1);
    CHECK(p.take(is_retired, busy) == -1 && busy_calls == 2);
    p.give_back(1, is_retired);
    p.close_and_wait();   // everything is back (one free, two dead): returns at once
    CHECK(p.closing && p.take(is_retired, busy) == -1 && busy_calls == 2);   // closing: nothing is handed out, and nobody is told "busy"
  }
  {
    // "all back" becomes true exactly when free + dead == slots, and wakes the waiter
    SlotPool p;
    p.fill(3);
    retired[0] = retired[1] = retired[2] = false;
    for (int i = 0; i < 3; ++i) CHECK(p.take(is_retired, busy) == i);
    std::atomic<bool> woke{false};
    std::thread stopper([&] { p.close_and_wait(); woke.store(true); });
    p.give_back(0, is_retired);
    CHECK(!p.all_back() && !woke.load());
    retired[1] = true;
    p.give_back(1, is_retired);
    CHECK(!p.all_back() && !woke.load() && p.dead_slots == 1);
    p.give_back(2, is_retired);
    CHECK(p.all_back());
    stopper.join();
    CHECK(woke.load() && p.free_slots.size() + p.dead_slots == 3);
  }
}

static void test_overflow_window() {
  const std::int64_t ms = 1000000;
  OverflowWindow w;
  w.threshold = 96;
  w.front_ns = 50 * ms;
  std::int64_t now = 1000 * ms;
  // threshold - 1 overflows inside 10 ms do not trip it (the first opens the window and counts 1)
  for (int i = 0; i < w.threshold - 1; ++i) w.note_overflow(now + i * 1000);
  CHECK(w.front_until() == 0 && w.count.load() == w.threshold - 1);
  // the threshold-th does
  const std::int64_t at = now + 9 * ms;
  w.note_overflow(at);
  CHECK(w.front_until() == at + w.front_ns && w.count.load() == 0);
  // a gap of more than 10 ms restarts the count at 1
  w.front_until_ns.store(0);
  for (int i = 0; i < 50; ++i) w.note_overflow(at + i);
  CHECK(w.count.load() == 50);
  now = w.window_ns.load() + 10 * ms + 1;
  w.note_overflow(now);
  CHECK(w.count.load() == 1 && w.window_ns.load() == now && w.front_until() == 0);
  // exactly 10 ms is still the same window
  w.note_overflow(now + 10 * ms);
  CHECK(w.count.load() == 2 && w.window_ns.load() == now);
}

int main() {
  test_gate();
  test_pool();
  test_overflow_window();
  if (failures) return 1;
  std::printf("ALL OK\n");
  return 0;
}
