// Host runtime shared by the C-ABI translation units: context, model handle, HIP helpers.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mrk.h"
#include "forest.hpp"
#include "serve_sync.hpp"
#include "status.hpp"
#include "switches.hpp"

namespace mrk {

#define MRK_HIP(expr)                                                                         \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess)                                                                     \
      throw ::mrk::StatusError(MRK_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

// hipFree / hipHostFree wait for EVERY resident kernel of the device.  While gangs of the serving queue are resident (capi_serve.cpp:
// they stay up to MRK_SERVE_LIFE_US and are relaunched at once under traffic, so with 8 of them the device is hardly ever idle) a
// buffer that regrows - the scratch batches of mrk_rank's front finding their sizes - stalled its caller for 70 ... 190 ms
// (profiles/r06_al_front_trace.txt: the `build` phase of a combined batch).  So while any gang is resident, memory is not given
// back at once: release_device / release_pinned put it on a list that is emptied when the last gang has been waited for.
std::atomic<int> &resident_gangs();           // capi.cpp
void release_device(void *p);                 // hipFree now, or later
void release_pinned(void *p);                 // hipHostFree now, or later
void flush_deferred_releases();               // (no gang resident: give everything back)

// RAII device buffer (hipMalloc / hipFree), grow-only reserve.
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
    return *this;
  }
  ~DevBuf() { release(); }
  void release() {
    if (p) release_device(p);
    p = nullptr;
    cap = 0;
  }
  // The first allocation is exact; a buffer that has to GROW is one whose size follows the traffic (the scratch batches of
  // mrk_rank's front: the combined batch is whatever was queued), and every regrowth is a hipFree - a device-wide
  // synchronisation - plus a hipMalloc: milliseconds, seen as 40-90 ms p99 by 64 callers while eight lanes found their sizes
  // (profiles/r06_c).  So regrowth at least doubles (x 1.25 beyond 256 MB).
  void reserve(size_t bytes) {
    if (bytes <= cap) return;
    const size_t grown = cap >= (256u << 20) ? cap + cap / 4 : cap * 2;
    release();
    size_t want = bytes < 256 ? 256 : bytes;
    if (grown > want) want = grown;
    MRK_HIP(hipMalloc(&p, want));
    cap = want;
  }
  template <typename T>
  T *as() const { return (T *)p; }
};

// pinned host staging buffer
struct PinBuf {
  void *p = nullptr;
  size_t cap = 0;
  PinBuf() = default;
  PinBuf(const PinBuf &) = delete;
  PinBuf &operator=(const PinBuf &) = delete;
  ~PinBuf() { if (p) release_pinned(p); }
  void reserve(size_t bytes) {  // (regrowth doubles, like DevBuf's)
    if (bytes <= cap) return;
    const size_t grown = cap >= (256u << 20) ? cap + cap / 4 : cap * 2;
    if (p) release_pinned(p);
    p = nullptr;
    cap = 0;
    size_t want = bytes < 4096 ? 4096 : bytes;
    if (grown > want) want = grown;
    MRK_HIP(hipHostMalloc(&p, want, hipHostMallocDefault));
    cap = want;
  }
  template <typename T>
  T *as() const { return (T *)p; }
};

struct KernelTimer {
  double total_ms = 0.0;
  int64_t launches = 0;
};

struct Store;     // store.hpp
struct Registry;  // features.hpp
struct RankTicket;  // rank_front.cpp

}  // namespace mrk

struct mrk_batch;   // rank_host.hpp
struct mrk_server;  // capi_serve.cpp

struct mrk_ctx {
  // owner reference (dropped by mrk_shutdown) + one per live model / batch: the context outlives its handles
  std::atomic<int> refs{1};
  bool closed = false;
  int device = 0;
  hipStream_t stream = nullptr;
  // the stream kernel launches and their HIP-event timers go to: the context stream, or - while a batch with
  // its own stream runs (ctx->mu held) - that batch's stream
  hipStream_t launch = nullptr;
  int n_cus = 0;
  size_t lds_per_block = 0;
  std::mutex mu;  // serialises kernel launches (ctx->launch routing, timers) + the context's scratch buffers
  // The feature store: puts / flushes take it exclusively, everything that reads the host mirror or launches kernels
  // that read the device tables takes it shared (a flush may reallocate the tables; it waits for the device first).
  // Lock order: store_mu before mu.
  std::shared_mutex store_mu;
  // libstdc++'s shared_mutex prefers readers; since round 6 several leaders of mrk_rank's front hold the store shared at
  // overlapping times, so a put could wait for ever.  Writers announce themselves (StoreWriteLock) and new readers
  // (StoreAccess, rank_host.hpp) let them pass first.
  std::atomic<int> store_writers{0};
  // scratch for predict_f64
  mrk::DevBuf d_x, d_out, d_flag;
  mrk::DevBuf d_cells;  // binned tile of the bit-vector scorer (score_qs.hip), grow-only
  mrk::PinBuf h_flag;
  // profiling
  bool profile = false;
  std::map<std::string, mrk::KernelTimer> timers;
  std::vector<std::tuple<std::string, hipEvent_t, hipEvent_t>> pending_events;
  // feature side (created by mrk_config_load_json)
  mrk::Registry *registry = nullptr;  // owned; freed by mrk::free_rank_state
  mrk::Store *store = nullptr;
  // mrk_rank's scratch batches ("lanes": grow-only mrk_batch objects, lane 0 on the context stream, the others on streams of
  // their own; owned, freed by mrk::free_rank_state).  A lane is held by one leader of the batching front at a time (qmu).
  static constexpr int RANK_LANES_MAX = 8;
  mrk_batch *rank_lane[RANK_LANES_MAX] = {};
  bool lane_busy[RANK_LANES_MAX] = {};
  // mrk_values' scratch batch (a grow-only mrk_batch on a stream of its own; owned, freed by mrk::free_rank_state): one caller at a time
  mrk_batch *values_lane = nullptr;
  std::mutex values_mu;               // lock order: values_mu before store_mu
  // multi-GPU (comm.cpp): the RCCL communicator this context's device belongs to (ncclComm_t), nullptr = a world of one
  void *comm = nullptr;
  int comm_rank = 0, comm_world = 1;
  mrk::DevBuf d_comm;                 // scratch of the host-value collectives
  // EVERY collective on `comm` is issued under this lock (RCCL does not allow concurrent calls on one communicator).  The
  // host must also issue collectives in the same order on every rank (mrk.h): the lock makes a mistake a wait, not a race.
  std::mutex comm_mu;
  std::mutex servers_mu;              // the serving queues of this context (capi_serve.cpp mrk_serve_*): a store flush stops their workgroups
  std::vector<mrk_server *> servers;
  std::atomic<int> n_servers{0};      // its size, for mrk_rank's lock-free "is there a queue at all"
  std::atomic<mrk_server *> hot_server{nullptr};   // the most recently started one: mrk_rank's way in without the mutex ...
  mrk::ReaderGate hot_gate;                        // ... guarded by reader counts per epoch parity (capi_serve.cpp rank_through_server)
  // batching front of mrk_rank: concurrent callers are combined into device batches by whichever waiting caller finds a
  // free lane (rank_front.cpp); several batches are in flight at once - one per lane
  std::mutex qmu;
  std::condition_variable qcv;
  std::vector<mrk::RankTicket *> rank_queue;
  mrk_ctx();
  ~mrk_ctx();
};

// exclusive access to a context's feature store, with precedence over readers that have not started yet
struct StoreWriteLock {
  mrk_ctx *ctx;
  std::unique_lock<std::shared_mutex> lk;
  explicit StoreWriteLock(mrk_ctx *c) : ctx(c) {
    ctx->store_writers.fetch_add(1);
    lk = std::unique_lock<std::shared_mutex>(ctx->store_mu);
    ctx->store_writers.fetch_sub(1);
  }
};

struct mrk_model {
  mrk_ctx *ctx = nullptr;
  std::atomic<int> refs{1};
  mrk::Forest forest;
  mrk::PackedForest packed;
  std::vector<std::string> container_features;
  int n_warmup = 0;                    // container v3: RankingEventFormat records kept for mrk_model_warmup
  std::vector<uint8_t> warmup_bytes;
  mrk::DevBuf d_image, d_trees, d_chunks, d_cat;
  // bit-vector image (forests of <= 16-leaf trees); qs.ok == false => tree-walk kernel only
  mrk::PackedForestQS qs;
  mrk::QsSignature qs_sig;             // the image's view signature (forest.hpp): part of the key of the specialised assembly kernels
  mrk::DevBuf d_qs_bnodes;             // byte-mode node image (qs.byte_ok)
  mrk::DevBuf d_qs_nodes, d_qs_leaves, d_qs_thr, d_qs_feats, d_qs_views, d_qs_catnodes, d_qs_cat;
};

namespace mrk {

// The way into a context for an entry that works on its device: holds ctx->mu (kernel launches, the scratch buffers), refuses
// a context that mrk_shutdown has closed, and selects the context's device for the calling thread - in that order.
struct DeviceLock {
  std::lock_guard<std::mutex> lk;
  hipStream_t stream;
  explicit DeviceLock(mrk_ctx *ctx) : lk(ctx->mu), stream(ctx->stream) {
    if (ctx->closed) throw StatusError(MRK_ERR_INVALID_ARG, "context is shut down");
    MRK_HIP(hipSetDevice(ctx->device));
  }
};

// a host vector into a device buffer on `s` (the caller keeps `h` until the stream has been waited for); never a null pointer
template <typename T>
void upload(DevBuf &d, const std::vector<T> &h, hipStream_t s) {
  d.reserve(std::max<size_t>(h.size() * sizeof(T), 16));
  if (!h.empty()) MRK_HIP(hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s));
}

// capi.cpp: a serialised booster by its backend tag (MRK_BACKEND_*); an unknown tag is MRK_ERR_INVALID_ARG
Forest parse_booster(int backend, const uint8_t *bytes, size_t len);

// Times a kernel with HIP events on ctx->stream when profiling is enabled.
struct ScopedKernelTimer {
  mrk_ctx *ctx;
  const char *name;
  hipEvent_t a = nullptr, b = nullptr;
  ScopedKernelTimer(mrk_ctx *c, const char *n);
  ~ScopedKernelTimer();
};
void drain_profile_events(mrk_ctx *ctx);

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of a function ON A DEVICE: a process that drives several devices
// (mrk_init with n contexts) has to opt in once per (device, function), whichever thread launches first.  Cheap on the
// launch path: a thread-local memo of the last pair in front of a mutex-protected set.
void lds_optin(mrk_ctx *ctx, const void *fn, int bytes = 160 * 1024);

// Hardware queues the HIP runtime may spread this process's streams over (GPU_MAX_HW_QUEUES; ROCm's default is 4).  The first
// mrk_* call that touches HIP sets it to 24 unless the host has set it; returns what is in force as far as the library can tell.
int hw_queue_budget();

void ctx_retain(mrk_ctx *ctx);
void ctx_release(mrk_ctx *ctx);

// capi_rank.cpp: releases ctx->registry / ctx->store
void free_rank_state(mrk_ctx *ctx);
// comm.cpp
void comm_destroy(mrk_ctx *ctx);
void comm_allgather_f64_inplace(mrk_ctx *ctx, double *buf, size_t chunk, hipStream_t stream);
void comm_allgather_f64(mrk_ctx *ctx, const double *send, double *recv, size_t count, hipStream_t stream);
void comm_allgather_i32(mrk_ctx *ctx, const int32_t *send, int32_t *recv, size_t count, hipStream_t stream);
// features.cpp: drops the encoder references mrk_config_bind_encoder took
void unbind_encoders(mrk_ctx *ctx);
// features.cpp: mrk_config_bind_termfreq (parses BM25Matcher.TermFreqDic JSON, binds it to a device-matched bm25 field_match)
void bind_termfreq(mrk_ctx *ctx, const char *feature, const char *json_bytes, size_t len);

// capi.cpp: a null / closed model, a negative shape, a null matrix / output, fewer columns than the forest splits on (MRK_ERR_DIM_MISMATCH)
void check_predict_args(mrk_model *model, const void *x, int rows, int cols, const void *out);

// score.hip
void launch_score(mrk_ctx *ctx, mrk_model *m, const double *d_x, int rows, int cols, double *d_out,
                  int *d_flag);
uint32_t score_chunk_budget();
// score_qs.hip: false => not applicable, use the tree-walk kernel
bool launch_score_qs(mrk_ctx *ctx, mrk_model *m, const double *d_x, int rows, int cols, double *d_out, int *d_flag,
                     const uint32_t *d_row_req);
void launch_score_qs_cells(mrk_ctx *ctx, mrk_model *m, const uint16_t *d_cells, int rows, double *d_out);

}  // namespace mrk
