// The synchronisation pieces of the serving queue (capi_serve.cpp) that are host logic alone: no HIP, no other header of the
// library - tests/native/serve_sync_test.cpp drives them under ASan + UBSan and under TSan.
#pragma once
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <vector>

namespace mrk {

// Lets readers use a pointer somebody else may withdraw and free, without a lock.  Readers count themselves into the current
// epoch's cell BEFORE they load the pointer; the stop side withdraws the pointer, turns the epoch and waits for the old cell to
// drain - whoever could still hold the withdrawn pointer is in it.
struct ReaderGate {
  std::atomic<std::uint32_t> epoch{0};
  std::atomic<int> readers[2] = {{0}, {0}};
  std::mutex stop_mu;
  int enter() {   // the cell to leave()
    for (;;) {
      const std::uint32_t e = epoch.load(std::memory_order_seq_cst);
      readers[e & 1].fetch_add(1, std::memory_order_seq_cst);
      if (epoch.load(std::memory_order_seq_cst) == e) return (int)(e & 1);
      readers[e & 1].fetch_sub(1, std::memory_order_seq_cst);
    }
  }
  void leave(int cell) { readers[cell].fetch_sub(1, std::memory_order_seq_cst); }
  // (the pointer is withdrawn) returns when no reader that entered before the turn is left; `pause` between looks
  template <typename Pause>
  void turn_and_wait(Pause pause) {
    std::lock_guard<std::mutex> lk(stop_mu);
    const std::uint32_t e = epoch.fetch_add(1, std::memory_order_seq_cst);
    while (readers[e & 1].load(std::memory_order_seq_cst) != 0) pause();
  }
};

// The free slots of a queue.  A stack: the most recently used slot is the one whose workgroup is still resident.  A slot whose
// gang was retired (`retired(slot)`, asked under the pool's mutex) is never handed out again: it is counted dead where it is met.
struct SlotPool {
  std::mutex mu;
  std::condition_variable cv;
  std::vector<int> free_slots;
  std::size_t n_slots = 0, dead_slots = 0;
  bool closing = false;
  void fill(int n) {
    n_slots = (std::size_t)n;
    for (int i = 0; i < n; ++i) free_slots.push_back(n - 1 - i);  // slot 0 on top
  }
  // a free slot, or -1: the pool is closing, or every slot is busy - then `every_slot_busy()` has been called, under the mutex
  template <typename Retired, typename Busy>
  int take(Retired retired, Busy every_slot_busy) {
    std::lock_guard<std::mutex> lk(mu);
    if (closing) return -1;
    while (!free_slots.empty()) {
      const int c = free_slots.back();
      free_slots.pop_back();
      if (retired(c)) { dead_slots += 1; continue; }   // retired with its gang
      return c;
    }
    every_slot_busy();
    return -1;
  }
  template <typename Retired>
  void give_back(int slot, Retired retired) {
    std::lock_guard<std::mutex> lk(mu);
    if (retired(slot)) dead_slots += 1;
    else free_slots.push_back(slot);
    cv.notify_one();   // under the mutex: mrk_serve_stop deletes the server as soon as it sees the last slot back
  }
  bool all_back() {
    std::lock_guard<std::mutex> lk(mu);
    return free_slots.size() + dead_slots == n_slots;
  }
  // nothing is handed out any more; returns when every slot is back or dead
  void close_and_wait() {
    std::unique_lock<std::mutex> lk(mu);
    closing = true;
    cv.wait(lk, [&] { return free_slots.size() + dead_slots == n_slots; });  // requests in flight finish first
  }
};

// Overload guard (a process with fewer CPUs than the queue has slots): overflowing callers in numbers mean the CPUs are gone -
// everybody goes through the front, whose waiters sleep, for `front_ns`; then the queue is tried again
struct OverflowWindow {
  int threshold = 0;
  std::int64_t front_ns = 0;
  std::atomic<std::int64_t> front_until_ns{0}, window_ns{0};
  std::atomic<int> count{0};
  std::int64_t front_until() const { return front_until_ns.load(std::memory_order_relaxed); }
  void note_overflow(std::int64_t now_ns) {   // a caller found every slot busy
    const std::int64_t w = window_ns.load(std::memory_order_relaxed);
    if (now_ns - w > 10000000) {   // 10 ms windows
      window_ns.store(now_ns, std::memory_order_relaxed);
      count.store(1, std::memory_order_relaxed);
      return;
    }
    if (count.fetch_add(1, std::memory_order_relaxed) + 1 >= threshold) {
      count.store(0, std::memory_order_relaxed);
      front_until_ns.store(now_ns + front_ns, std::memory_order_relaxed);
    }
  }
};

}  // namespace mrk
