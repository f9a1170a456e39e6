// What the rank side's translation units share (capi_rank.cpp: the batch pipeline, mrk_values*, mrk_batch_*; capi_store.cpp:
// config, store and mrk_debug_* entry points; rank_front.cpp: the batching front of mrk_rank; capi_serve.cpp: the serving queue).
#pragma once
#include <algorithm>
#include <chrono>
#include <cstring>
#include <thread>

#include "features.hpp"
#include "qs_device.hpp"
#include "rank.hpp"
#include "rank_launch.hpp"
#include "rank_plan.hpp"
#include "runtime.hpp"

struct mrk_batch {
  mrk_ctx *ctx = nullptr;
  const mrk::Program *prog = nullptr;
  int n_req = 0, total_items = 0;
  std::mutex bmu;            // a batch is driven by one thread at a time; this makes a mistake a wait instead of a race
  mrk::DevBuf d_in, d_prep_out, d_arena, d_matrix;
  hipStream_t stream = nullptr;   // batches made by mrk_batch_prepare / _create own a stream: several can be in flight on one device
  hipStream_t s() const { return stream ? stream : ctx->stream; }
  mrk::DevBuf d_out;              // [scores: (T + shard padding) f64][order: T i32][status: n_req i32][load status: n_req i32], fetched with ONE copy
                             // (load status: what the id-resolution kernel found at load time - ST_BAD_IDS; status is zeroed by every run)
  size_t out_order_off = 0, out_status_off = 0, out_bytes = 0;
  mrk::PinBuf h_out;
  bool fetch_enqueued = false;          // the download of d_out into h_out is on the stream behind the last run
  mrk::DevBuf d_cells;            // the scorer's binned tile (bit-vector models), grow-only
  mrk::DevBuf d_sort;                        // scratch of the multi-workgroup sort (bigsort.hip)
  mrk::DevBuf d_norm_order;                  // norm: position over a request of more than SORT_MAX_ITEMS candidates: its column's order
  mrk::DevBuf d_gather;                      // mrk_batch_gather_scores: the scores of every rank
  mrk::DevBuf d_gather_status;               // item-sharded runs: the status words of every rank ([world][n_req]) before they are OR-ed
  struct BigReq { int r, n_items, item_begin; };
  std::vector<BigReq> big;              // requests with n_items > SORT_MAX_ITEMS
  mrk::PinBuf h_in;
  mrk::HostBatch hb;              // host half of the last load (grow-only scratch)
  mrk::DevBuf d_ids;              // flat item ids of the batch: [offsets: (T + 1) u32][bytes]
  mrk::PinBuf h_ids;              // their staging copy when the caller's memory is not pinned
  mrk::BatchDev view{};
  std::vector<int32_t> h_status;
  std::vector<int32_t> codes;           // mrk_status per request (mrk_batch_host_outputs)
  mrk::BatchShape sh;             // what the plans read of the load (rank_plan.hpp; want_matrix is filled in per run)
  // the f64 matrix is materialised only on demand (explain / parity / models without a bit-vector image)
  bool want_matrix = false;
  // training rows (mrk_values, mrk_batch_load_values): mrk_batch_run(batch, NULL) assembles the rows of the loaded values program
  bool values = false;
  mrk::PinBuf h_vals;                        // [rows: T x dim f64][status: n_req i32][load status: n_req i32]
  size_t vals_status_off = 0;
  // what the last run left behind (reset by every run and every load)
  struct Ran {
    bool direct_out = false;            // the one-launch kernel: scores / order / status were written into h_out by the device
    bool matrix_valid = false;
    bool values = false;                // a values run: scores are 0.0 and the order is the request's own (NoopRanker.scala:22-26), filled by the host
    bool values_direct = false;         // ... by the one-launch values kernel: the device wrote rows and status words into h_vals itself
    // the fused cells launch (mrk_debug_batch_launch): bytes of a table entry in the kernel that ran (0: no such launch), which kernel
    // (0 interpreting, 1 mrk_jit_rank_cells, 2 mrk_jit_rank_cells_split), its dynamic LDS and what the LDS was sized from
    int entry_bytes = 0, kernel = 0;
    bool split_sized = false;
    size_t lds = 0, rt_bytes = 0;
    uint32_t thr_cap = 0;
  } ran;
};

namespace mrk {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

void quiesce_servers(mrk_ctx *ctx);   // capi_serve.cpp

// Access to the feature store for the duration of a call.  Readers (resolving a batch, launching kernels that gather from
// the device tables) share it; whatever is dirty is flushed first, exclusively.  `exclusive`: the call mutates host-side
// store state itself (lazily tokenised cross-encoder texts).
struct StoreAccess {
  mrk_ctx *ctx;
  std::shared_lock<std::shared_mutex> shared;
  std::unique_lock<std::shared_mutex> unique;
  StoreAccess(mrk_ctx *c, bool exclusive = false, bool flush = true) : ctx(c) {
    if (!ctx->store) throw StatusError(MRK_ERR_INVALID_ARG, "mrk_config_load_json must be called first");
    if (exclusive) {
      ctx->store_writers.fetch_add(1);
      unique = std::unique_lock<std::shared_mutex>(ctx->store_mu);
      ctx->store_writers.fetch_sub(1);
      if (flush) do_flush();
      return;
    }
    lock_shared();
    while (flush && ctx->store->dirty()) {
      shared.unlock();
      {
        StoreWriteLock x(ctx);
        do_flush();
      }
      lock_shared();
    }
  }
  // readers that have not started wait for announced writers (puts from the feedback stream must not starve behind the
  // overlapping leaders of mrk_rank's front); a reader never holds anything while it waits here
  void lock_shared() {
    if (ctx->store_writers.load(std::memory_order_acquire) > 0) {
      // ... for at most a millisecond: a stream of puts that never pauses must not starve the readers either
      const auto until = std::chrono::steady_clock::now() + std::chrono::milliseconds(1);
      while (ctx->store_writers.load(std::memory_order_acquire) > 0 && std::chrono::steady_clock::now() < until) std::this_thread::yield();
    }
    shared = std::shared_lock<std::shared_mutex>(ctx->store_mu);
  }
  // the device work is enqueued: what follows (waiting for it, copying results) needs no store - a flush synchronises the device itself
  void release() {
    if (shared.owns_lock()) shared.unlock();
    if (unique.owns_lock()) unique.unlock();
  }
  void do_flush() {
    MRK_HIP(hipSetDevice(ctx->device));
    quiesce_servers(ctx);  // persistent workgroups hold the device views they were launched with: they leave, and come back with the next request
    ctx->store->flush(ctx->stream);
  }
};

// One block for a load's inputs - the arrays BatchDev points into, each at a multiple of `align`: 256 for a batch's device block,
// 16 for a serving slot's, whose offsets travel in ServeCtl.  An array without elements (no overrides) takes no room.
struct InputLayout {
  size_t o_reqs, o_consts, o_irf, o_ov, o_prep, o_slot, o_ireq;
  size_t host_bytes;   // everything the host always fills; the per-item arrays follow
  size_t bytes;
  InputLayout(const HostBatch &hb, size_t align) {
    size_t off = 0;
    auto place = [&](size_t n) { size_t o = off; off = align_up(off + n, align); return o; };
    o_reqs = place(hb.reqs.size() * sizeof(ReqDev));
    o_consts = place(hb.consts.size() * 8);
    o_irf = place(hb.irf.size() * 4);
    o_ov = place(hb.overrides.size() * sizeof(Override));
    o_prep = place(hb.prep_out.size() * sizeof(PrepOut));
    host_bytes = std::max(off, align);
    o_slot = place((size_t)hb.total_items * 4);
    o_ireq = place((size_t)hb.total_items * 4);
    bytes = std::max(off, align);
  }
  // device-resolved ids: item_slot / item_req are written by a kernel
  size_t filled(const HostBatch &hb) const { return hb.device_ids ? host_bytes : bytes; }
  void fill(uint8_t *h, const HostBatch &hb) const {
    auto put = [&](size_t o, const void *src, size_t n) { if (n) memcpy(h + o, src, n); };
    put(o_reqs, hb.reqs.data(), hb.reqs.size() * sizeof(ReqDev));
    put(o_consts, hb.consts.data(), hb.consts.size() * 8);
    put(o_irf, hb.irf.data(), hb.irf.size() * 4);
    put(o_ov, hb.overrides.data(), hb.overrides.size() * sizeof(Override));
    put(o_prep, hb.prep_out.data(), hb.prep_out.size() * sizeof(PrepOut));
    if (hb.device_ids) return;
    put(o_slot, hb.item_slot.data(), (size_t)hb.total_items * 4);
    put(o_ireq, hb.item_req.data(), (size_t)hb.total_items * 4);
  }
};

// capi_rank.cpp: the batch pipeline
int status_to_code(int st, std::string &msg);
bool program_mutates_store(const Program &prog);
void build_batch(mrk_ctx *ctx, const Program &prog, const mrk_request *reqs, int n_req, const mrk_item_ids *ids, mrk_batch &b);
ModelShape shape_of(const mrk_model *m);
void check_model_fits(mrk_model *model, const Program &prog);
WalkDev walk_device_view(const mrk_model *m, int cols);
void run_batch(mrk_batch &b, mrk_model *model, int lo, int hi, bool sort, bool direct = false);
void run_values(mrk_batch &b);
void enqueue_fetch(mrk_batch &b, bool scores, bool order);
void fetch_batch(mrk_batch &b, double *scores, int32_t *order, double *matrix);
// capi_store.cpp: the program of a configured model (program_of: the caller holds the store)
const Program &program_of(mrk_ctx *ctx, const char *model_name);
const Program &locked_program(mrk_ctx *ctx, const char *model_name);
// rank_front.cpp / capi_serve.cpp: the two ways of a single request
int rank_front(mrk_ctx *ctx, mrk_model *model, const char *model_name, const mrk_request *req, double *out_scores,
               int32_t *out_order, double *out_matrix);
int rank_through_server(mrk_ctx *ctx, mrk_model *model, const char *model_name, const mrk_request *req, double *out_scores,
                        int32_t *out_order, bool &done);
// codec.cpp
int load_feature_values(Store &store, const uint8_t *bytes, size_t len, int64_t now_ms);

}  // namespace mrk
