// The serving queue of the C ABI (include/mrk.h mrk_serve_*).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <thread>

#include <sched.h>
#include <sys/prctl.h>
#include <time.h>

#include "rank_host.hpp"

using namespace mrk;

// ---------------------------------------------------------------- the serving queue
// main/command/Serve.scala:130-150 (warm-up, then the port opens) and api/routes/RankApi.scala:25-41 (one rerank per
// request thread): mrk_serve_start compiles what the model needs and prepares `n_slots` slots, each a persistent workgroup
// (rank_device.hpp rank_serve_body; launched in gangs of SERVE_GANG per kernel and stream) with its request / result blocks in
// pinned memory; mrk_serve_rank is then the whole
// request path: resolve the request on the calling thread, write it into a free slot, publish, spin on the acknowledgement -
// no HIP call, no launch, no copy command.  Whatever the one-workgroup path does not cover (more than 128 candidates,
// per-item overrides, tables beyond the slot's LDS, explain) goes through mrk_rank.

namespace {

struct ServeSlot {
  int gang = 0;                 // index into mrk_server::gangs; this slot is workgroup `index - gang.first` of the gang's kernel
  void *pinned = nullptr;       // [ServeCtl 128 B][output block][input block], coherent host memory
  ServeCtl *ctl = nullptr;
  uint8_t *h_out = nullptr, *h_in = nullptr;
  DevBuf d_in;
  HostBatch hb;
  uint32_t seq = 0;
};

// One kernel launch = one gang of up to SERVE_GANG slots on one stream.  `mu` orders launches and stops of the gang; `launch_id`
// names the launch whose workgroups are (or were last) resident - a slot whose `ctl->exited` equals it has been left.
//
// The states of a gang, as the host knows them (running / counted / dead / stuck; every move is made under `mu`):
//   never launched       - / - / - / -, launch_id 0.  The first request in one of its slots launches it (revive_gang -> launch_gang).
//   resident             R / C / - / -: a kernel was launched and has not been waited for.  Its workgroups may have left on their own
//                        (idle or life time); the host learns that only by waiting.  drain_gang moves it to "left" - asked by revive_gang
//                        (a request found its workgroup gone), quiesce_servers (a store flush) and mrk_serve_stop - or, when the kernel is
//                        still there at the deadline, retires it; serve_fast retires it when a workgroup does not answer for 5 s.
//   left                 - / - / - / -, launch_id != 0: waited for, nothing of it touches the device.  The next request launches it again.
//   retired and resident R / C / D / -: none of its slots is handed out again (serve_sync.hpp SlotPool counts them dead).  The next
//                        flush (quiesce_servers) waits up to 2 s for it: gone -> - / - / D / -, which mrk_serve_stop frees like a gang
//                        that left; still there -> stuck, and the flush is refused.
//   retired and stuck    R / C / D / S: every later flush asks once, without waiting, and is refused while the kernel stays; when it
//                        is found gone: - / - / D / -.
//   retired and leaked   mrk_serve_stop met it retired and resident (stuck or not): leak_resident_gang.  It stays counted in
//                        resident_gangs() for the life of the process.
// `running` and `counted` change together, in resident() and left(), and nowhere else.
struct ServeGang {
  hipStream_t stream = nullptr;
  int first = 0, n = 0;
  DevBuf d_slots, d_clock;      // ServeSlotDev[n]; the gang's last-activity word
  std::mutex mu;
  std::atomic<uint32_t> launch_id{0};
  bool running = false;         // (mu) a kernel was launched and has not been waited for
  bool counted = false;         // (mu) ... and is counted in resident_gangs() (runtime.hpp: memory is not given back meanwhile)
  std::atomic<bool> dead{false};   // a workgroup of it did not answer in time: none of its slots is handed out again (a late answer would land in the next request's buffers)
  bool stuck = false;           // ... and was still resident after a flush waited 2 s for it: later flushes ask once, without waiting again
  // (mu) a kernel of it has been launched
  void resident() {
    running = true;
    if (!counted) { counted = true; resident_gangs().fetch_add(1, std::memory_order_acq_rel); }
  }
  // (mu) it left (or its launch failed): nothing of this gang touches the device any more
  void left() {
    running = false;
    if (counted) { counted = false; resident_gangs().fetch_sub(1, std::memory_order_acq_rel); }
  }
};

constexpr size_t SERVE_OUT_BYTES = 2048;          // scores 128 x 8 | order 128 x 4 | status 2 x 4
constexpr size_t SERVE_IN_CAP = 64 * 1024;
constexpr int SERVE_THREADS = 512;                // 128 item lanes x op split 4; 8 wavefronts split the trees
constexpr size_t SERVE_LDS = 128 * 1024;

}  // namespace

struct mrk_server {
  mrk_ctx *ctx = nullptr;
  mrk_model *model = nullptr;
  std::string model_name;
  const Program *prog = nullptr;
  bool f64 = true;
  bool walk = false;            // the model is scored by the tree walk (rank_serve_walk_body)
  void *jit_fn = nullptr;
  uint64_t idle_ticks = 0, life_ticks = 0;
  std::vector<std::unique_ptr<ServeSlot>> slots;
  std::vector<std::unique_ptr<ServeGang>> gangs;
  std::atomic<int> users{0};   // callers of mrk_rank that are inside serve_fast through the context's server list
  std::atomic<int> waiting{0};          // callers between publish and acknowledgement
  bool guard = false;          // the overload guard is on (a process with fewer CPUs than the queue has slots)
  OverflowWindow overflow;
  std::atomic<uint64_t> est_dev_ns{0};  // what a request takes on the device (input copy + ranking + write-back), smoothed
  SlotPool pool;
  bool slot_retired(int slot) const { return gangs[(size_t)slots[(size_t)slot]->gang]->dead.load(); }
  std::atomic<uint64_t> n_queue{0}, n_fallback{0}, n_launches{0};
  std::atomic<uint64_t> dev_ticks[4] = {{0}, {0}, {0}, {0}};   // device-side 100 MHz ticks: input copy, ranking, result write-back; [3]: shader cycles of the ranking
  std::atomic<uint64_t> host_ns[3] = {{0}, {0}, {0}};     // host-side ns: resolve + pack, publish -> acknowledgement, copy-out
};

namespace {

void tell_gang(mrk_server &srv, ServeGang &g, uint32_t v) {
  for (int i = g.first; i < g.first + g.n; ++i) __atomic_store_n(&srv.slots[(size_t)i]->ctl->stop, v, __ATOMIC_SEQ_CST);
}

// Waits until the stream is idle or the deadline has passed (false).  PauseSpin: a request is waiting for the answer - look as often
// as the runtime allows, and at the clock every 256 looks; SleepMs: a flush - look once a millisecond.
enum class Pace { PauseSpin, SleepMs };
bool idle_by(hipStream_t stream, std::chrono::steady_clock::time_point deadline, Pace pace) {
  hipError_t q = hipStreamQuery(stream);
  for (uint32_t spin = 1; q == hipErrorNotReady; ++spin) {
    if ((pace == Pace::SleepMs || (spin & 0xffu) == 0u) && std::chrono::steady_clock::now() >= deadline) break;
    if (pace == Pace::SleepMs) std::this_thread::sleep_for(std::chrono::milliseconds(1));
    else __builtin_ia32_pause();
    q = hipStreamQuery(stream);
  }
  return q != hipErrorNotReady;
}

// (g.mu held) waits until every workgroup of the gang has left: they serve what is published in their slots first.  Bounded: a
// gang that is still resident after `seconds` is retired (false).
bool drain_gang(mrk_server &srv, ServeGang &g, int seconds) {
  if (!g.running) return true;
  tell_gang(srv, g, 1u);
  if (!idle_by(g.stream, std::chrono::steady_clock::now() + std::chrono::seconds(seconds), Pace::PauseSpin)) {
    g.dead.store(true);
    return false;
  }
  tell_gang(srv, g, 0u);
  g.left();
  return true;
}

// (g.mu held; the caller holds the store shared: the device views are current)
void launch_gang(mrk_server &srv, ServeGang &g) {
  mrk_ctx *ctx = srv.ctx;
  ServeGangDev d;
  d.slots = g.d_slots.as<ServeSlotDev>();
  d.clock = g.d_clock.as<unsigned long long>();
  d.launch_id = g.launch_id.load() + 1;
  d.pad = 0;
  d.idle_ticks = srv.idle_ticks;
  d.life_ticks = srv.life_ticks;
  if (srv.walk)
    launch_rank_serve_walk(ctx, g.stream, ctx->store->device_view(), srv.prog->device_view(), walk_device_view(srv.model, srv.prog->dim), d,
                           g.n, SERVE_THREADS, SERVE_LDS, srv.f64, srv.jit_fn);
  else
    launch_rank_serve(ctx, g.stream, ctx->store->device_view(), srv.prog->device_view(), qs_device_view(srv.model), qs_forest_view(srv.model), d,
                      g.n, SERVE_THREADS, SERVE_LDS, srv.f64, srv.jit_fn);
  g.launch_id.store(d.launch_id);
  g.resident();
  srv.n_launches.fetch_add(1);
}

// The caller has published a request in a slot of `g` and saw (or assumes) that no workgroup of launch `seen` will serve it:
// the gang is drained and launched again as a whole, unless somebody else did meanwhile.  Returns the launch now resident.
uint32_t revive_gang(mrk_server &srv, ServeGang &g, uint32_t seen) {
  std::lock_guard<std::mutex> lk(g.mu);
  if (g.dead.load()) throw StatusError(MRK_ERR_DEVICE, "the slot's serving gang was retired");
  if (g.running && g.launch_id.load() != seen) return g.launch_id.load();
  if (!drain_gang(srv, g, 5)) throw StatusError(MRK_ERR_DEVICE, "a serving gang did not leave within 5 s (its slots are retired)");
  launch_gang(srv, g);
  return g.launch_id.load();
}

// (g.mu held) mrk_serve_stop met a retired gang whose kernel was never seen to leave.  Its workgroups may still be resident, polling
// their slots' pinned blocks: stream, blocks and device buffers are leaked on purpose (a hipFree would wait for the resident
// kernel - for ever, if it hangs).  The gang stays `running` and counted.
void leak_resident_gang(mrk_server &srv, ServeGang &g) {
  g.d_slots.p = nullptr; g.d_slots.cap = 0;
  g.d_clock.p = nullptr; g.d_clock.cap = 0;
  for (int i = g.first; i < g.first + g.n; ++i) { srv.slots[(size_t)i]->d_in.p = nullptr; srv.slots[(size_t)i]->d_in.cap = 0; }
}

// The CPUs this process may use: its affinity mask, cut by the cgroup's quota (v2 cpu.max, v1 cfs_quota_us / cfs_period_us).
int cpu_budget() {
  static const int budget = [] {
    cpu_set_t set;
    int n = sched_getaffinity(0, sizeof set, &set) == 0 ? CPU_COUNT(&set) : (int)std::thread::hardware_concurrency();
    if (n < 1) n = 1;
    long long quota = -1, period = 0;
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
      char q[32] = {0};
      if (fscanf(f, "%31s %lld", q, &period) == 2 && strcmp(q, "max") != 0) quota = atoll(q);
      fclose(f);
    } else if (FILE *g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
      if (fscanf(g, "%lld", &quota) != 1) quota = -1;
      fclose(g);
      if (FILE *h = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
        if (fscanf(h, "%lld", &period) != 1) period = 0;
        fclose(h);
      }
    }
    if (quota > 0 && period > 0) n = std::min<long long>(n, std::max<long long>(1, (quota + period - 1) / period));
    return n;
  }();
  return budget;
}

int64_t ns_of(std::chrono::steady_clock::duration d) { return std::chrono::duration_cast<std::chrono::nanoseconds>(d).count(); }

// true: ranked through the queue (status = the request's device status word); false: not a request the queue takes
bool serve_fast(mrk_server &srv, const mrk_request *req, double *out_scores, int32_t *out_order, int &status) {
  mrk_ctx *ctx = srv.ctx;
  if (!switches().rank_serve || req->n_items > QS_TILE_ROWS) return false;
  const auto h0 = std::chrono::steady_clock::now();
  const int64_t now_ns = ns_of(h0.time_since_epoch());
  if (srv.guard && now_ns < srv.overflow.front_until()) return false;   // overloaded a moment ago: the front
  // (every slot busy: the batching front of mrk_rank combines the overflow)
  const int si = srv.pool.take([&](int c) { return srv.slot_retired(c); }, [&] { if (srv.guard) srv.overflow.note_overflow(now_ns); });
  if (si < 0) return false;
  struct Release {
    mrk_server &s;
    int i;
    bool dead = false;
    ~Release() { s.pool.give_back(i, [&](int c) { return dead || s.slot_retired(c); }); }
  } release{srv, si};
  ServeSlot &sl = *srv.slots[(size_t)si];
  const Program &prog = locked_program(ctx, srv.model_name.c_str());
  if (&prog != srv.prog || program_mutates_store(prog) || prog.normalises()) return false;
  StoreAccess access(ctx);
  MRK_HIP(hipSetDevice(ctx->device));
  check_model_fits(srv.model, prog);
  HostBatch &hb = sl.hb;
  resolve_requests(prog, *ctx->store, req, 1, nullptr, hb);
  const int T = hb.total_items;
  const int vals = median_vals_cap(hb.max_doubles);
  if (!one_workgroup_takes(shape_of(srv.model), srv.walk, prog.dim, (int)prog.prep.size(), hb.max_items, !hb.overrides.empty(), hb.max_req_entries, vals,
                           SERVE_THREADS, SERVE_LDS))
    return false;
  // the request's input block: build_batch's arrays, 16-byte aligned
  const InputLayout in(hb, 16);
  if (in.bytes > SERVE_IN_CAP) return false;
  in.fill(sl.h_in, hb);
  ServeCtl &ctl = *sl.ctl;
  ctl.in_bytes = (uint32_t)in.bytes;
  ctl.o_reqs = (uint32_t)in.o_reqs; ctl.o_consts = (uint32_t)in.o_consts; ctl.o_irf = (uint32_t)in.o_irf;
  ctl.o_prep = (uint32_t)in.o_prep; ctl.o_slot = (uint32_t)in.o_slot; ctl.o_ireq = (uint32_t)in.o_ireq;
  ctl.total_items = (uint32_t)T; ctl.tab_entries = table_entries(hb.max_req_entries); ctl.vals_cap = (uint32_t)vals; ctl.mode = 4;
  const uint32_t seq = ++sl.seq;
  if (seq == 0xffffffffu) sl.seq = 0;  // (never: 4 G requests through one slot)
  const auto h1 = std::chrono::steady_clock::now();
  __atomic_store_n(&ctl.seq, seq, __ATOMIC_SEQ_CST);  // publishes the block and the header
  ServeGang &g = *srv.gangs[(size_t)sl.gang];
  uint32_t seen = g.launch_id.load();   // (0: never launched - no slot's `exited` word holds it)
  auto gone = [&] { return seen == 0u || __atomic_load_n(&ctl.exited, __ATOMIC_SEQ_CST) == seen; };
  auto acked = [&] { return __atomic_load_n(&ctl.ack, __ATOMIC_ACQUIRE) == seq; };
  if (gone()) seen = revive_gang(srv, g, seen);
  // Waiting: the first few callers spin on the acknowledgement (nothing is faster); the callers beyond them sleep through
  // the time the device is known to need and spin for the rest.  64 callers spinning for 0.1 ms each are 64 busy CPUs: on a
  // host whose CPU quota is smaller (the measurement boxes: profiles/r06_ad) the scheduler parks them for whole periods -
  // p50 0.15 ms, maximum 77 ... 400 ms, and the closed-loop rate FELL from 32 to 64 callers.
  struct Waiting {
    std::atomic<int> &n;
    int mine;
    explicit Waiting(std::atomic<int> &c) : n(c), mine(c.fetch_add(1) + 1) {}
    ~Waiting() { n.fetch_sub(1); }
  } waiting(srv.waiting);
  const bool sleeper = waiting.mine > switches().serve_spin_callers;
  if (sleeper) {
    static thread_local bool slack_set = false;
    if (!slack_set) { (void)prctl(PR_SET_TIMERSLACK, 1000ul, 0ul, 0ul, 0ul); slack_set = true; }   // this thread's timers: 1 us instead of 50
    // (publish -> acknowledgement is the device's total + 15 ... 20 us of PCIe round trips: profiles/r06_ad, 96 against 77 us)
    const uint64_t est = srv.est_dev_ns.load(std::memory_order_relaxed);
    if (est > 20000 && !acked()) {
      struct timespec ts = {0, (long)std::min<uint64_t>(est + (uint64_t)switches().serve_sleep_extra_us * 1000, 2000000)};
      (void)nanosleep(&ts, nullptr);
    }
  }
  // ... and a sleeper does not spin for the rest either: it looks every few microseconds (`serve_poll_us`; 0 = spin).  Spinning
  // tails kept 64 callers just inside a 16-CPU quota and 80 callers outside it: the whole process was throttled for 100 - 200 ms
  // at a time and the rate fell from 360 k to 180 k requests/s (profiles/r06_aj).
  const long poll_ns = sleeper ? (long)switches().serve_poll_us * 1000 : 0;
  const auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(5);
  for (uint32_t spin = 1; !acked(); ++spin) {
    if (poll_ns > 0 || (spin & 31u) == 0u) {
      if (gone()) {  // the workgroup left (idle / old / told to stop) - possibly after serving this request
        if (acked()) break;
        seen = revive_gang(srv, g, seen);
      } else if ((spin & (poll_ns > 0 ? 0xffu : 0xffffu)) == 0u && std::chrono::steady_clock::now() > deadline) {
        tell_gang(srv, g, 1u);  // should they still be alive: leave
        g.dead.store(true);
        release.dead = true;
        char why[256];
        snprintf(why, sizeof why, "the serving workgroup did not answer within 5 s (its gang is retired; slot %d: seq %u ack %u exited %u stop %u, gang launch %u seen %u)",
                 si, __atomic_load_n(&ctl.seq, __ATOMIC_SEQ_CST), __atomic_load_n(&ctl.ack, __ATOMIC_SEQ_CST), __atomic_load_n(&ctl.exited, __ATOMIC_SEQ_CST),
                 __atomic_load_n(&ctl.stop, __ATOMIC_SEQ_CST), g.launch_id.load(), seen);
        throw StatusError(MRK_ERR_DEVICE, why);
      }
    }
    if (poll_ns > 0) {
      struct timespec ts = {0, poll_ns};
      (void)nanosleep(&ts, nullptr);
    } else {
      __builtin_ia32_pause();
    }
  }
  const auto h2 = std::chrono::steady_clock::now();
  if (out_scores && T) memcpy(out_scores, sl.h_out, (size_t)T * 8);
  if (out_order && T) memcpy(out_order, sl.h_out + 1024, (size_t)T * 4);
  const int32_t *hs = (const int32_t *)(sl.h_out + 1536);
  status = hs[0] | hs[1];
  const unsigned long long *clk = (const unsigned long long *)(hs + 16);
  for (int k = 0; k < 4; ++k) srv.dev_ticks[k].fetch_add(clk[k]);
  {
    const uint64_t sample = (clk[0] + clk[1] + clk[2]) * 10, old = srv.est_dev_ns.load(std::memory_order_relaxed);   // 100 MHz ticks -> ns
    if (sample < 10000000) srv.est_dev_ns.store(old ? (old * 7 + sample) / 8 : sample, std::memory_order_relaxed);
  }
  const auto h3 = std::chrono::steady_clock::now();
  srv.host_ns[0].fetch_add((uint64_t)ns_of(h1 - h0));
  srv.host_ns[1].fetch_add((uint64_t)ns_of(h2 - h1));
  srv.host_ns[2].fetch_add((uint64_t)ns_of(h3 - h2));
  srv.n_queue.fetch_add(1);
  return true;
}

}  // namespace

void mrk::quiesce_servers(mrk_ctx *ctx) {  // the caller holds the store exclusively: no request is in flight in any slot
  std::lock_guard<std::mutex> lk(ctx->servers_mu);
  for (mrk_server *srv : ctx->servers) {
    for (auto &g : srv->gangs) {   // tell all of them first: they leave side by side
      std::lock_guard<std::mutex> gl(g->mu);
      if (g->running && !g->dead.load()) tell_gang(*srv, *g, 1u);
    }
    for (auto &g : srv->gangs) {
      std::lock_guard<std::mutex> gl(g->mu);
      if (!g->running) continue;
      if (!g->dead.load()) {
        if (drain_gang(*srv, *g, 5)) continue;
      }
      // A retired gang (a workgroup of it missed the 5 s deadline) was told to stop when it was retired.  Slow is not hung: if
      // its kernel is still on the device it still reads the store views it was launched with, and the caller is about to
      // reallocate them - wait for it a while, and refuse the flush rather than free memory under a live kernel.
      // (the 2 s are spent ONCE per stuck gang: while it stays resident every later flush fails at once instead of holding
      //  the store exclusively for another 2 s per request - one stuck workgroup is an error state, not a stall of the service)
      if (!idle_by(g->stream, std::chrono::steady_clock::now() + (g->stuck ? std::chrono::seconds(0) : std::chrono::seconds(2)), Pace::SleepMs)) {
        g->stuck = true;
        throw StatusError(MRK_ERR_DEVICE, "a retired serving workgroup is still resident: the store is not reallocated under it");
      }
      g->stuck = false;
      g->left();
    }
  }
  if (resident_gangs().load(std::memory_order_acquire) == 0) flush_deferred_releases();
}

extern "C" {

int mrk_serve_start(mrk_ctx *ctx, mrk_model *model, const char *model_name, int n_slots, mrk_server **out) {
  return guard([&] {
    if (!out) throw StatusError(MRK_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    if (!ctx || !model || !model_name || n_slots < 1 || n_slots > 64) throw StatusError(MRK_ERR_INVALID_ARG, "bad arguments (1..64 slots)");
    if (model->ctx != ctx) throw StatusError(MRK_ERR_INVALID_ARG, "model belongs to another context");
    const Program &prog = locked_program(ctx, model_name);
    // a forest of larger trees is walked in the request's workgroup (rank_serve_walk_body) when its matrix, its largest chunk and
    // the chunk's leaf values fit the workgroup's LDS next to each other; MRK_RANK_ONE_WALK=0: refused, as before that kernel
    const ModelShape ms = shape_of(model);
    const bool walk = walk_one_model(ms, switches());
    if (!model->qs.ok && !walk) throw StatusError(MRK_ERR_UNSUPPORTED, "the serving queue scores with the bit-vector scorer (trees of <= 16 leaves); use mrk_rank for this model");
    check_model_fits(model, prog);
    if (walk) {
      const bool wf64 = ms.f64;
      const int lt = walk_leaf_trees(ms.max_chunk_trees);
      const size_t need = rank_one_walk_lds_bytes(prog.dim, wf64, ms.max_chunk_bytes, ms.max_chunk_trees, lt, 0);   // (the forest alone: a request's tables come on top)
      if (need > SERVE_LDS) {
        if (model->qs.ok) throw StatusError(MRK_ERR_UNSUPPORTED, "MRK_SCORER=walk: this model's matrix and chunk do not fit the serving workgroup's LDS");
        throw StatusError(MRK_ERR_UNSUPPORTED, "the serving queue walks this forest in one workgroup's LDS (" + std::to_string(SERVE_LDS) + " bytes) and it does not fit: matrix " +
                                                   std::to_string(prog.dim) + " columns x 128 rows x " + std::to_string(wf64 ? 8 : 4) + " bytes = " +
                                                   std::to_string(rank_one_walk_matrix_bytes(prog.dim, wf64)) + ", largest chunk " + std::to_string(model->packed.max_chunk_bytes) +
                                                   " bytes + leaf values of " + std::to_string(lt) + " trees = " +
                                                   std::to_string(rank_one_walk_scoring_bytes(wf64, model->packed.max_chunk_bytes, (int)model->packed.max_chunk_trees, lt)) +
                                                   "; use mrk_rank for this model");
      }
    }
    MRK_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<mrk_server> srv(new mrk_server());
    srv->ctx = ctx;
    srv->model = model;
    srv->model_name = model_name;
    srv->prog = &prog;
    srv->f64 = ms.f64;
    srv->idle_ticks = (uint64_t)std::max(1, switches().serve_idle_us) * 100ull;  // wall_clock64: 100 MHz
    srv->life_ticks = (uint64_t)std::max(1, switches().serve_life_us) * 100ull;
    srv->walk = walk;
    // warm-up: the compile happens here, not under the first request
    srv->jit_fn = jit_function(prog, walk ? JIT_SERVE_WALK : JIT_SERVE, srv->f64, !walk && switches().thr_stage ? &model->qs_sig : nullptr);
    srv->overflow.front_ns = (int64_t)switches().serve_overload_ms * 1000000;
    // A resident kernel holds its stream's hardware queue for as long as it stays, and streams that share a hardware queue wait
    // for each other: round 5's "collapse at 32 callers" (p99 76 ms) was a slot whose stream had landed behind another slot's
    // resident kernel (ROCm maps a process's streams onto GPU_MAX_HW_QUEUES = 4 hardware queues by default; mrk_init asks for
    // 24, hw_queue_budget in capi.cpp).  One kernel per slot (round 6's first form) therefore capped the slots at the queues, and
    // the callers beyond them - sent through mrk_rank's front, whose lanes share the same queues - still met 150 ... 230 ms stalls.
    // Slots are launched in GANGS instead: SERVE_GANG workgroups per kernel, one stream per gang - 64 slots on 8 streams.
    const int n_gangs = std::min((n_slots + SERVE_GANG - 1) / SERVE_GANG, std::max(1, hw_queue_budget() - 4));   // 4: the context stream, the lanes of mrk_rank's front, a batch
    n_slots = std::min(n_slots, n_gangs * SERVE_GANG);
    for (int i = 0; i < n_slots; ++i) {
      std::unique_ptr<ServeSlot> sl(new ServeSlot());
      sl->gang = i / SERVE_GANG;
      MRK_HIP(hipHostMalloc(&sl->pinned, 128 + SERVE_OUT_BYTES + SERVE_IN_CAP, hipHostMallocCoherent | hipHostMallocMapped));
      memset(sl->pinned, 0, 128 + SERVE_OUT_BYTES + SERVE_IN_CAP);
      static_assert(sizeof(ServeCtl) == 128, "ServeCtl is one 128-byte line");
      sl->ctl = (ServeCtl *)sl->pinned;
      sl->h_out = (uint8_t *)sl->pinned + 128;
      sl->h_in = sl->h_out + SERVE_OUT_BYTES;
      sl->d_in.reserve(SERVE_IN_CAP);
      srv->slots.push_back(std::move(sl));
    }
    srv->pool.fill(n_slots);
    for (int k = 0; k < n_gangs; ++k) {
      std::unique_ptr<ServeGang> g(new ServeGang());
      g->first = k * SERVE_GANG;
      g->n = std::min(SERVE_GANG, n_slots - g->first);
      MRK_HIP(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
      std::vector<ServeSlotDev> view((size_t)g->n);
      for (int i = 0; i < g->n; ++i) {
        ServeSlot &sl = *srv->slots[(size_t)(g->first + i)];
        view[(size_t)i].ctl = sl.ctl;
        view[(size_t)i].in_host = sl.h_in;
        view[(size_t)i].in_dev = sl.d_in.as<uint8_t>();
        view[(size_t)i].out = OneOut{(double *)sl.h_out, (int32_t *)(sl.h_out + 1024), (int32_t *)(sl.h_out + 1536), nullptr, 1};
      }
      g->d_slots.reserve(view.size() * sizeof(ServeSlotDev));
      g->d_clock.reserve(8);
      MRK_HIP(hipMemcpy(g->d_slots.p, view.data(), view.size() * sizeof(ServeSlotDev), hipMemcpyHostToDevice));
      MRK_HIP(hipMemset(g->d_clock.p, 0, 8));
      srv->gangs.push_back(std::move(g));
    }
    srv->guard = srv->overflow.front_ns > 0 && cpu_budget() < n_slots;   // fewer CPUs than slots: callers in overflow are CPUs that are not there
    srv->overflow.threshold = std::max(3 * n_slots, 96);
    mrk_model_retain(model);
    ctx_retain(ctx);
    {
      std::lock_guard<std::mutex> lk(ctx->servers_mu);
      ctx->servers.push_back(srv.get());
      ctx->n_servers.store((int)ctx->servers.size(), std::memory_order_release);
      ctx->hot_server.store(srv.get(), std::memory_order_seq_cst);
    }
    *out = srv.release();
  });
}

}  // extern "C"

static int serve_one(mrk_server *srv, const mrk_request *req, double *out_scores, int32_t *out_order, bool &done) {
  int status = 0;
  done = false;
  const int rc = guard([&] { done = serve_fast(*srv, req, out_scores, out_order, status); });
  if (rc != MRK_OK || !done) return rc;
  std::string msg;
  const int code = status_to_code(status, msg);
  if (code != MRK_OK) set_last_error(msg);
  return code;
}

extern "C" int mrk_serve_rank(mrk_server *srv, const mrk_request *req, double *out_scores, int32_t *out_order) {
  if (!srv || !req) { set_last_error("null argument"); return MRK_ERR_INVALID_ARG; }
  bool done = false;
  const int rc = serve_one(srv, req, out_scores, out_order, done);
  if (done || rc != MRK_OK) return rc;
  srv->n_fallback.fetch_add(1);
  return rank_front(srv->ctx, srv->model, srv->model_name.c_str(), req, out_scores, out_order, nullptr);
}

// mrk_rank's way into the queue: the context's server for (model, model_name), if one was started.  `users` keeps
// mrk_serve_stop from freeing it between the lookup and the slot.
int mrk::rank_through_server(mrk_ctx *ctx, mrk_model *model, const char *model_name, const mrk_request *req, double *out_scores,
                             int32_t *out_order, bool &done) {
  done = false;
  if (req->n_items > QS_TILE_ROWS) return MRK_OK;
  // The context's most recently started queue, without a lock (64 callers a few hundred thousand times a second on one mutex
  // are a queue of their own, and a holder the scheduler parks stops them all).  Readers count themselves into the current
  // epoch's cell BEFORE they load the pointer; mrk_serve_stop withdraws the pointer, turns the epoch and waits for the old
  // cell to drain - whoever could still hold the withdrawn pointer is in it.
  {
    const int cell = ctx->hot_gate.enter();
    mrk_server *hot = ctx->hot_server.load(std::memory_order_seq_cst);
    int rc = MRK_OK;
    const bool mine = hot && hot->model == model && hot->model_name == model_name;
    if (mine) {
      rc = serve_one(hot, req, out_scores, out_order, done);
      if (!done && rc == MRK_OK) hot->n_fallback.fetch_add(1);
    }
    ctx->hot_gate.leave(cell);
    if (mine) return rc;
  }
  mrk_server *srv = nullptr;
  {
    std::lock_guard<std::mutex> lk(ctx->servers_mu);
    for (mrk_server *c : ctx->servers) {
      if (c->model == model && c->model_name == model_name) { srv = c; break; }
    }
    if (srv) srv->users.fetch_add(1);
  }
  if (!srv) return MRK_OK;
  const int rc = serve_one(srv, req, out_scores, out_order, done);
  if (!done && rc == MRK_OK) srv->n_fallback.fetch_add(1);
  srv->users.fetch_sub(1);
  return rc;
}

extern "C" {

int mrk_serve_stats(mrk_server *srv, int64_t *out, int n_out) {
  if (!srv || !out || n_out < 0) return MRK_ERR_INVALID_ARG;
  int64_t v[MRK_SERVE_STATS] = {};
  v[0] = (int64_t)srv->n_queue.load();
  v[1] = (int64_t)srv->n_fallback.load();
  v[2] = (int64_t)srv->n_launches.load();
  for (int k = 0; k < 3; ++k) {
    v[3 + k] = (int64_t)srv->host_ns[k].load();
    v[6 + k] = (int64_t)(srv->dev_ticks[k].load() * 10);   // 100 MHz ticks -> ns
  }
  v[9] = (int64_t)srv->dev_ticks[3].load();
  for (int k = 0; k < n_out && k < MRK_SERVE_STATS; ++k) out[k] = v[k];   // never past the caller's buffer, whatever ABI it was built for
  return MRK_OK;
}

void mrk_serve_stop(mrk_server *srv) {
  if (!srv) return;
  mrk_ctx *ctx = srv->ctx;
  srv->pool.close_and_wait();
  {
    std::lock_guard<std::mutex> lk(ctx->servers_mu);
    ctx->servers.erase(std::remove(ctx->servers.begin(), ctx->servers.end(), srv), ctx->servers.end());
    ctx->n_servers.store((int)ctx->servers.size(), std::memory_order_release);
    if (ctx->hot_server.load() == srv) ctx->hot_server.store(ctx->servers.empty() ? nullptr : ctx->servers.back(), std::memory_order_seq_cst);
  }
  ctx->hot_gate.turn_and_wait([] { std::this_thread::yield(); });   // mrk_rank's lock-free readers that may still hold the withdrawn pointer (rank_through_server)
  while (srv->users.load() != 0) std::this_thread::yield();   // callers of mrk_rank that found this server before it left the list
  (void)hipSetDevice(ctx->device);
  for (auto &g : srv->gangs) {
    std::lock_guard<std::mutex> gl(g->mu);
    if (!g->dead.load()) (void)drain_gang(*srv, *g, 5);
    if (g->dead.load() && g->running) {
      leak_resident_gang(*srv, *g);
      continue;
    }
    if (g->stream) (void)hipStreamDestroy(g->stream);
    for (int i = g->first; i < g->first + g->n; ++i) {
      ServeSlot &sl = *srv->slots[(size_t)i];
      if (sl.pinned) (void)hipHostFree(sl.pinned);
    }
  }
  mrk_model_free(srv->model);
  delete srv;
  if (resident_gangs().load(std::memory_order_acquire) == 0) flush_deferred_releases();
  ctx_release(ctx);
}

}  // extern "C"
