// The batch pipeline of the C ABI (include/mrk.h): build, run and fetch of a device batch; mrk_values*, mrk_batch_*.
#include <algorithm>
#include <cstring>

#include "rank_host.hpp"

namespace mrk {

int status_to_code(int st, std::string &msg) {
  if (st & ST_ARITHMETIC) { msg = "java.lang.ArithmeticException: / by zero (normalised rate: global `top` counter is 0)"; return MRK_ERR_ARITHMETIC; }
  if (st & ST_DIM) { msg = "dim mismatch: item embedding is shorter than the query embedding"; return MRK_ERR_DIM_MISMATCH; }
  if (st & ST_ILLEGAL_ARG) { msg = "requirement failed: Duration is limited to +-(2^63-1)ns (ca. 292 years)"; return MRK_ERR_INVALID_ARG; }
  if (st & 32) { msg = "Input data contains `inf` or a value too large, while `missing` is not set to `inf`"; return MRK_ERR_INVALID_ARG; }
  if (st & ST_BAD_IDS) { msg = "item id offsets descend or pass bytes_len (mrk_item_ids)"; return MRK_ERR_INVALID_ARG; }
  if (st & ST_TOO_MANY) { msg = "diversity over more values than the device pre-pass supports: set `top`"; return MRK_ERR_UNSUPPORTED; }
  if (st & ST_TABLE_FULL) { msg = "internal: pre-pass hash table under-sized (store changed between prepare and run?)"; return MRK_ERR_DEVICE; }
  return MRK_OK;
}

void free_rank_state(mrk_ctx *ctx) {
  for (int i = 0; i <= mrk_ctx::RANK_LANES_MAX; ++i) {   // (the last round: mrk_values' scratch batch)
    mrk_batch *&lane = i < mrk_ctx::RANK_LANES_MAX ? ctx->rank_lane[i] : ctx->values_lane;
    mrk_batch *b = lane;
    if (!b) continue;
    (void)hipSetDevice(ctx->device);
    if (b->stream) {
      (void)hipStreamSynchronize(b->stream);
      (void)hipStreamDestroy(b->stream);
    }
    delete b;
    lane = nullptr;
  }
  delete ctx->registry;
  delete ctx->store;
  ctx->registry = nullptr;
  ctx->store = nullptr;
}

bool program_mutates_store(const Program &prog) {
  for (const HostOp &ho : prog.host_ops)
    if (ho.def->cross && ho.def->encoder) return true;
  return false;
}

static bool is_pinned_host(const void *p) {
  if (!p) return false;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // plain malloc memory: not an error worth keeping
    return false;
  }
  return a.type == hipMemoryTypeHost;
}

// (re)builds the device-resident batch (inputs uploaded, outputs allocated, id resolution enqueued); the caller holds
// the store (StoreAccess) and the batch
void build_batch(mrk_ctx *ctx, const Program &prog, const mrk_request *reqs, int n_req, const mrk_item_ids *ids, mrk_batch &b) {
  Store &store = *ctx->store;
  MRK_HIP(hipSetDevice(ctx->device));
  HostBatch &hb = b.hb;
  resolve_requests(prog, store, reqs, n_req, ids, hb);
  b.ctx = ctx;
  b.prog = &prog;
  b.n_req = n_req;
  b.total_items = hb.total_items;
  const int T = hb.total_items;
  const InputLayout in(hb, 256);
  const size_t up_bytes = in.filled(hb);
  b.h_in.reserve(up_bytes);
  b.d_in.reserve(in.bytes);
  in.fill(b.h_in.as<uint8_t>(), hb);
  MRK_HIP(hipMemcpyAsync(b.d_in.p, b.h_in.p, up_bytes, hipMemcpyHostToDevice, b.s()));
  uint8_t *d = b.d_in.as<uint8_t>();
  // outputs in one allocation: one device-to-host copy per fetch (single-request latency)
  const size_t score_slots = (size_t)T + 256 * QS_TILE_ROWS;  // room for the padded chunks of an item-sharded all-gather
  b.out_order_off = align_up(score_slots * 8, 256);
  b.out_status_off = align_up(b.out_order_off + std::max<size_t>(T, 1) * 4, 256);
  b.out_bytes = b.out_status_off + 2 * std::max<size_t>(n_req, 1) * 4;
  b.d_out.reserve(b.out_bytes);
  int32_t *d_load_status = (int32_t *)(b.d_out.as<uint8_t>() + b.out_status_off) + std::max(n_req, 1);
  MRK_HIP(hipMemsetAsync(d_load_status, 0, std::max<size_t>(n_req, 1) * 4, b.s()));
  if (hb.device_ids && T > 0) {
    // the ids as they arrived: [offsets][bytes] in one device buffer; pinned caller memory is read by the copy engine
    // directly, anything else goes through the batch's pinned staging buffer
    const size_t off_bytes = ((size_t)T + 1) * 4;
    const size_t id_bytes = ids->offsets[T];
    if (id_bytes > ids->bytes_len || ids->bytes_len > 0xffffffffull)
      throw StatusError(MRK_ERR_INVALID_ARG, "mrk_item_ids: the last offset passes bytes_len (or bytes_len >= 4 GiB)");
    const size_t o_bytes = align_up(off_bytes, 256);
    b.d_ids.reserve(o_bytes + std::max<size_t>(id_bytes, 1));
    const void *src_off = ids->offsets, *src_bytes = ids->bytes;
    const bool own_staging = (const void *)ids->offsets == (const void *)b.h_ids.p;   // mrk_rank's front flattens straight into this batch's pinned staging
    if (!own_staging && (!is_pinned_host(ids->offsets) || !is_pinned_host(ids->bytes))) {
      b.h_ids.reserve(o_bytes + std::max<size_t>(id_bytes, 1));
      memcpy(b.h_ids.p, ids->offsets, off_bytes);
      memcpy(b.h_ids.as<uint8_t>() + o_bytes, ids->bytes, id_bytes);
      src_off = b.h_ids.p;
      src_bytes = b.h_ids.as<uint8_t>() + o_bytes;
    }
    MRK_HIP(hipMemcpyAsync(b.d_ids.p, src_off, off_bytes, hipMemcpyHostToDevice, b.s()));
    if (id_bytes) MRK_HIP(hipMemcpyAsync(b.d_ids.as<uint8_t>() + o_bytes, src_bytes, id_bytes, hipMemcpyHostToDevice, b.s()));
    launch_resolve_ids(b.s(), store.tables[SC_ITEM].id_table_view(), b.d_ids.as<uint8_t>() + o_bytes, b.d_ids.as<uint32_t>(), (uint32_t)id_bytes,
                       (const ReqDev *)(d + in.o_reqs), n_req, T, (int32_t *)(d + in.o_slot), (uint32_t *)(d + in.o_ireq), d_load_status);
  }
  b.d_arena.reserve(std::max<size_t>(hb.arena_entries, 1) * 8);
  b.d_matrix.reserve(std::max<size_t>((size_t)T * prog.dim, 1) * 8);
  BatchDev &v = b.view;
  v.reqs = (const ReqDev *)(d + in.o_reqs);
  v.n_req = n_req;
  v.total_items = T;
  v.item_lo = 0;
  v.item_hi = T;
  v.item_slot = (const int32_t *)(d + in.o_slot);
  v.item_req = (const uint32_t *)(d + in.o_ireq);
  v.consts = (const double *)(d + in.o_consts);
  v.irf = (const int32_t *)(d + in.o_irf);
  v.overrides = (const Override *)(d + in.o_ov);
  v.n_overrides = (int)hb.overrides.size();
  v.prep_out = (PrepOut *)(d + in.o_prep);
  v.arena = (unsigned long long *)b.d_arena.p;
  v.status = (int32_t *)(b.d_out.as<uint8_t>() + b.out_status_off);
  v.matrix = (double *)b.d_matrix.p;
  v.scores = (double *)b.d_out.p;
  v.order = (int32_t *)(b.d_out.as<uint8_t>() + b.out_order_off);
  b.h_status.assign(n_req, 0);
  b.ran = {};
  b.fetch_enqueued = false;
  b.big.clear();
  size_t big_bytes = 0;
  for (int r = 0; r < n_req; ++r)
    if (hb.reqs[r].n_items > SORT_MAX_ITEMS) {
      b.big.push_back({r, hb.reqs[r].n_items, (int)hb.reqs[r].item_begin});
      big_bytes = std::max(big_bytes, big_sort_scratch_bytes(hb.reqs[r].n_items));
    }
  if (big_bytes) b.d_sort.reserve(big_bytes);  // one scratch: the big requests of a batch are sorted one after the other on its stream
  b.sh = BatchShape{};
  b.sh.n_req = n_req;
  b.sh.total_items = T;
  b.sh.max_items = hb.max_items;
  b.sh.compact_tables = hb.compact_tables;
  b.sh.overrides = !hb.overrides.empty();
  b.sh.normalises = prog.normalises();
  b.sh.n_prep = (int)prog.prep.size();
  b.sh.dim = prog.dim;
  fused_batch_shape(b.sh, hb.max_req_entries, hb.max_doubles, switches());
}

static BatchShape shape_of(const mrk_batch &b) {
  BatchShape sh = b.sh;
  sh.want_matrix = b.want_matrix;
  return sh;
}

ModelShape shape_of(const mrk_model *m) {
  ModelShape s;
  if (!m) return s;
  s.present = true;
  s.qs_ok = m->qs.ok;
  s.f64 = m->forest.backend == Backend::LightGBM;
  if (s.qs_ok) {
    const QsDev q = qs_device_view(m);
    s.thr_cap = q.thr_cap;
    s.rt_doubles = q.rt_doubles;
    s.n_views = q.n_views;
  }
  s.max_chunk_bytes = m->packed.max_chunk_bytes;
  s.max_chunk_trees = (int)m->packed.max_chunk_trees;
  return s;
}

void check_model_fits(mrk_model *model, const Program &prog) {
  if (!model) return;
  if (model->refs.load() <= 0) throw StatusError(MRK_ERR_INVALID_ARG, "model is closed");
  int used = 0;
  for (auto &t : model->forest.trees)
    for (auto f : t.feat) used = std::max(used, f + 1);
  if (used > prog.dim)
    throw StatusError(MRK_ERR_DIM_MISMATCH, "booster splits on feature " + std::to_string(used - 1) + " but model '" + prog.model +
                                                "' has " + std::to_string(prog.dim) + " columns");
}

// pre-pass + assembly into the row-major f64 matrix (ClickthroughQuery's layout); inside a LaunchOn
static void assemble_matrix(mrk_batch &b, const StoreDev &st, const ProgramDev &pd, void *jit_matrix_fn = nullptr) {
  mrk_ctx *ctx = b.ctx;
  if (b.sh.fused_ok) {
    launch_rank_fused(ctx, st, pd, b.view, b.sh.fused_entries, b.sh.fused_vals, b.sh.fused_threads, b.sh.fused_split, jit_matrix_fn ? 1 : b.sh.fused_slices, nullptr, nullptr, true, jit_matrix_fn);
  } else {
    launch_prepass(ctx, st, pd, b.view, b.sh.fused_entries, nullptr);
    launch_assemble(ctx, st, pd, b.view);
  }
  for (const Program::NormCol &nc : b.prog->norm_cols)  // schema.norm.scale over the request's column (Normalize.scala:13-45)
    if (!nc.cross || nc.cross->encoder) {
      launch_normalize(ctx, b.view, pd.dim, nc.col, nc.mode);
      if (nc.mode == NORM_POSITION)  // requests too large for one workgroup: ordered by the multi-workgroup sort
        for (auto &br : b.big) {
          b.d_norm_order.reserve((size_t)br.n_items * 4);
          launch_normalize_big(ctx, b.view, pd.dim, nc.col, br.item_begin, br.n_items, b.d_norm_order.as<int>(), b.d_sort.p);
        }
    }
  b.ran.matrix_valid = true;
}

// items per shard of an item-sharded run: ceil(total / count) rounded up to whole scorer tiles
static_assert(MRK_SHARD_TILE == QS_TILE_ROWS, "a shard is a whole number of scorer tiles");
static int shard_chunk(const mrk_batch &b, int count) { return (int)mrk_shard_chunk(b.total_items, count); }

static void sort_batch(mrk_batch &b) {
  mrk_ctx *ctx = b.ctx;
  launch_sort(ctx, b.view, b.hb.max_items);
  if (b.big.empty()) return;
  ScopedKernelTimer timer(ctx, "sort");
  for (auto &br : b.big) {
    const SortSrc src{b.view.scores + br.item_begin, nullptr, 1, 1};
    launch_big_sort(ctx, ctx->launch, src, br.n_items, b.view.order + br.item_begin, b.d_sort.p);
  }
}

// routes kernel launches (and their timers) to a batch's stream; holds ctx->mu for as long as it lives
struct LaunchOn {
  mrk_ctx *ctx;
  std::lock_guard<std::mutex> lk;
  LaunchOn(mrk_ctx *c, hipStream_t s) : ctx(c), lk(c->mu) { ctx->launch = s; }
  ~LaunchOn() { ctx->launch = ctx->stream; }
};

// ---- forests the bit-vector scorer does not take (trees of more than 16 leaves), and any forest under MRK_SCORER=walk: the
// one-request kernels that walk the trees in the request's workgroup (rank_device.hpp rank_one_walk_body)
WalkDev walk_device_view(const mrk_model *m, int cols) {
  WalkDev w;
  w.image = m->d_image.as<uint8_t>();
  w.trees = m->d_trees.as<TreeRef>();
  w.chunks = m->d_chunks.as<ChunkRef>();
  w.cat_bits = m->d_cat.as<uint32_t>();
  w.n_chunks = (int32_t)m->packed.chunks.size();
  w.cols = cols;
  w.chunk_cap = (m->packed.max_chunk_bytes + 15u) & ~15u;
  w.ref_cap = ((uint32_t)m->packed.max_chunk_trees * (uint32_t)sizeof(TreeRef) + 15u) & ~15u;
  w.leaf_trees = walk_leaf_trees((int)m->packed.max_chunk_trees);
  w.pad = 0;
  w.base = m->forest.base_score;
  return w;
}
static_assert(sizeof(TreeRef) == 12 && WALK_TILE_ROWS == QS_TILE_ROWS, "launch_shape.hpp sizes the TreeRef rows and the matrix of rank_one_walk_body");

// enqueue the pipeline on the batch's stream for batch items [lo, hi); the caller holds the store (StoreAccess).  Which pipeline:
// rank_plan.hpp plan_rank, asked once.
void run_batch(mrk_batch &b, mrk_model *model, int lo, int hi, bool sort, bool direct) {
  mrk_ctx *ctx = b.ctx;
  MRK_HIP(hipSetDevice(ctx->device));
  check_model_fits(model, *b.prog);
  const BatchShape &sh = b.sh;
  const ModelShape ms = shape_of(model);
  const RankPlan plan = plan_rank(shape_of(b), ms, switches(), lo, hi, sort, direct);
  const int rows = hi - lo;
  const bool f64 = ms.present && ms.f64;
  // the kernels specialised for this model (hiprtc, ~7 s the first time): compiled before the launch lock is taken.  nullptr (specialisation
  // off, a background compile pending): the interpreting kernel of the same path
  const QsSignature *sig = plan.keyed ? &model->qs_sig : nullptr;
  void *jit_fn = jit_function(*b.prog, plan.kernel, f64, sig);
  void *jit_rt_fn = jit_function(*b.prog, plan.items_rt ? JIT_ITEMS_RT : JIT_NONE, f64, sig);
  void *jit_prep_fn = jit_function(*b.prog, plan.prepass ? JIT_PREPASS : JIT_NONE, f64, sig);
  LaunchOn on(ctx, b.s());
  const StoreDev st = ctx->store->device_view();
  const ProgramDev pd = b.prog->device_view();
  b.fetch_enqueued = false;
  b.ran = {};
  b.view.item_lo = plan.whole_matrix ? 0 : lo;
  b.view.item_hi = plan.whole_matrix ? b.total_items : hi;
  switch (plan.path) {
    case RankPath::One:
    case RankPath::OneWalk: {   // (the whole batch; the kernel writes the status words itself, and orders)
      b.h_out.reserve(b.out_bytes);
      uint8_t *h = b.h_out.as<uint8_t>();
      const OneOut out{(double *)h, (int32_t *)(h + b.out_order_off), (int32_t *)(h + b.out_status_off),
                       (const int32_t *)(b.d_out.as<uint8_t>() + b.out_status_off) + std::max(b.n_req, 1), std::max(b.n_req, 1)};
      if (plan.path == RankPath::OneWalk)
        launch_rank_one_walk(ctx, st, pd, b.view, sh.fused_entries, sh.fused_vals, sh.fused_threads, sh.fused_split, walk_device_view(model, pd.dim), out, f64,
                             one_request_lds_bytes(ms, true, pd.dim, sh.fused_entries, sh.fused_vals, sh.fused_threads), jit_fn);
      else launch_rank_one(ctx, st, pd, b.view, sh.fused_entries, sh.fused_vals, sh.fused_threads, sh.fused_split, qs_device_view(model), qs_forest_view(model), out, f64, jit_fn);
      b.ran.direct_out = true;
      return;
    }
    case RankPath::FusedCells:
    case RankPath::ItemCells: {
      // hot path: the assembled values go straight into the scorer's binned tile; no f64 matrix
      MRK_HIP(hipMemsetAsync(b.view.status, 0, std::max<size_t>(b.n_req, 1) * 4, b.s()));
      const QsDev q = qs_device_view(model);
      const size_t tile_bytes = (size_t)q.n_views * QS_TILE_ROWS * 2;
      const size_t n_tiles = ((size_t)b.total_items + QS_TILE_ROWS - 1) / QS_TILE_ROWS;
      b.d_cells.reserve(std::max<size_t>(n_tiles * tile_bytes, 16));
      if (hi % QS_TILE_ROWS && tile_bytes)  // rows past the last item of the last tile of this range
        MRK_HIP(hipMemsetAsync(b.d_cells.as<uint8_t>() + (size_t)(hi / QS_TILE_ROWS) * tile_bytes, 0, tile_bytes, b.s()));
      if (plan.path == RankPath::FusedCells) {
        // (jit_fn == nullptr: the interpreting kernel - 8-byte entries, sized as a split kernel only when it splits)
        const bool split_kernel = jit_fn && plan.split_kernel;
        b.ran.kernel = !jit_fn ? 0 : split_kernel ? 2 : 1;
        b.ran.entry_bytes = jit_fn ? plan.entry_bytes : 8;
        b.ran.split_sized = sh.fused_split > 1 || sh.fused_slices > 1 || split_kernel;
        b.ran.rt_bytes = sig && sig->ok ? (size_t)sig->rt_total * 8 : 0;
        b.ran.thr_cap = q.thr_cap;
        b.ran.lds = launch_rank_fused(ctx, st, pd, b.view, sh.fused_entries, sh.fused_vals, sh.fused_threads, sh.fused_split, sh.fused_slices, &q, b.d_cells.as<uint16_t>(), f64, jit_fn,
                                      b.ran.rt_bytes, b.ran.entry_bytes, split_kernel);
      } else {
        launch_prepass(ctx, st, pd, b.view, sh.fused_entries, jit_prep_fn);
        launch_assemble_cells(ctx, st, pd, b.view, q, b.d_cells.as<uint16_t>(), f64, jit_fn, sh.fused_entries, jit_rt_fn, jit_rt_fn ? model->qs_sig.rt_total : 0u);
      }
      // lo is a multiple of the tile size: the scorer sees rows [lo, hi) as its rows [0, hi - lo)
      launch_score_qs_cells(ctx, model, b.d_cells.as<uint16_t>() + (size_t)(lo / QS_TILE_ROWS) * (tile_bytes / 2), rows, b.view.scores + lo);
      break;
    }
    case RankPath::Matrix:
      MRK_HIP(hipMemsetAsync(b.view.status, 0, std::max<size_t>(b.n_req, 1) * 4, b.s()));
      assemble_matrix(b, st, pd, jit_fn);
      b.ran.matrix_valid = plan.whole_matrix || (lo == 0 && hi == b.total_items);
      if (model && rows > 0) {
        launch_score_batch(ctx, model, b.view.matrix + (size_t)lo * pd.dim, rows, pd.dim, b.view.scores + lo, b.view.status, b.view.item_req + lo);
      } else if (rows > 0) {
        // NoopModel (ml/rank/NoopRanker.scala:22-26): every score is 0.0
        MRK_HIP(hipMemsetAsync(b.view.scores + lo, 0, (size_t)rows * 8, b.s()));
      }
      break;
  }
  b.view.item_lo = 0;
  b.view.item_hi = b.total_items;
  if (sort) sort_batch(b);
}

static void run_batch(mrk_batch &b, mrk_model *model) { run_batch(b, model, 0, b.total_items, true); }

// The training rows of a batch (TrainBuffer.handleRanking: ItemValue.fromState over the loaded values program) on the batch's
// stream; the caller holds the store (StoreAccess).  One launch into the batch's pinned block - no forest, no ordering, no copy
// command - or the matrix path's assembly, fetched by a copy: rank_plan.hpp plan_values.  The specialised kernel is used with or
// without a model.
void run_values(mrk_batch &b) {
  mrk_ctx *ctx = b.ctx;
  MRK_HIP(hipSetDevice(ctx->device));
  const BatchShape &sh = b.sh;
  const ValuesPlan plan = plan_values(shape_of(b), switches());
  const size_t T = (size_t)b.total_items, R = (size_t)std::max(b.n_req, 1);
  void *jit_fn = jit_function(*b.prog, plan.kernel, true, nullptr);   // (before LaunchOn: a first use may compile)
  LaunchOn on(ctx, b.s());
  const StoreDev st = ctx->store->device_view();
  const ProgramDev pd = b.prog->device_view();
  b.fetch_enqueued = false;
  b.ran = {};
  b.ran.values = true;
  b.view.item_lo = 0;
  b.view.item_hi = b.total_items;
  if (plan.one) {
    b.vals_status_off = align_up(T * (size_t)pd.dim * 8, 256);
    b.h_vals.reserve(b.vals_status_off + 2 * R * 4);
    uint8_t *h = b.h_vals.as<uint8_t>();
    const ValuesOut out{(double *)h, (int32_t *)(h + b.vals_status_off), (const int32_t *)(b.d_out.as<uint8_t>() + b.out_status_off) + R, (int32_t)R};
    launch_rank_values(ctx, st, pd, b.view, sh.fused_entries, sh.fused_vals, sh.fused_threads, sh.fused_split, out, jit_fn);
    b.ran.values_direct = true;
    return;
  }
  MRK_HIP(hipMemsetAsync(b.view.status, 0, R * 4, b.s()));
  assemble_matrix(b, st, pd, jit_fn);
}

// NoopRanker's answer (ml/rank/NoopRanker.scala:22-26) for a values run: every score 0.0, every request in its own order
static void fill_noop_outputs(const mrk_batch &b, double *scores, int32_t *order) {
  if (scores) std::fill(scores, scores + b.total_items, 0.0);
  if (order)
    for (const ReqDev &rq : b.hb.reqs)
      for (int i = 0; i < rq.n_items; ++i) order[rq.item_begin + i] = i;
}

// scores + order + status -> the batch's pinned result buffer, one copy (a copy into pageable caller memory is staged by
// the runtime anyway, and three small copies cost three round trips); asynchronous
void enqueue_fetch(mrk_batch &b, bool scores, bool order) {
  if (b.ran.direct_out || b.ran.values_direct) return;  // the device wrote h_out / h_vals itself
  const size_t T = (size_t)b.total_items;
  b.h_out.reserve(b.out_bytes);
  uint8_t *h = b.h_out.as<uint8_t>();
  const uint8_t *d = b.d_out.as<uint8_t>();
  if (T * 8 <= 64 * 1024) {  // small batch: the whole blob
    MRK_HIP(hipMemcpyAsync(h, d, b.out_bytes, hipMemcpyDeviceToHost, b.s()));
  } else {                   // else the used ranges
    if (scores && T) MRK_HIP(hipMemcpyAsync(h, d, T * 8, hipMemcpyDeviceToHost, b.s()));
    if (order && T) MRK_HIP(hipMemcpyAsync(h + b.out_order_off, d + b.out_order_off, T * 4, hipMemcpyDeviceToHost, b.s()));
    MRK_HIP(hipMemcpyAsync(h + b.out_status_off, d + b.out_status_off, 2 * std::max<size_t>(b.n_req, 1) * 4, hipMemcpyDeviceToHost, b.s()));  // status + load status
  }
}

// the caller holds the store when `matrix` may have to be assembled (StoreAccess), and the batch
void fetch_batch(mrk_batch &b, double *scores, int32_t *order, double *matrix) {
  mrk_ctx *ctx = b.ctx;
  MRK_HIP(hipSetDevice(ctx->device));
  const size_t T = (size_t)b.total_items;
  const int32_t *hs;   // [status of the run: max(n_req, 1)][load status], in pinned memory
  if (b.ran.values_direct) {   // the one-launch values kernel: rows and status words are in the batch's pinned block once the stream is idle
    MRK_HIP(hipStreamSynchronize(b.s()));
    const uint8_t *h = b.h_vals.as<uint8_t>();
    if (matrix && T && b.prog->dim) memcpy(matrix, h, T * b.prog->dim * 8);
    hs = (const int32_t *)(h + b.vals_status_off);
  } else {
    if (matrix && T && b.prog->dim && !b.ran.matrix_valid) {
      // the last run assembled straight into the scorer's tile: materialise the f64 matrix now
      LaunchOn on(ctx, b.s());
      assemble_matrix(b, ctx->store->device_view(), b.prog->device_view());
    }
    if (!b.fetch_enqueued) enqueue_fetch(b, scores != nullptr, order != nullptr);
    b.fetch_enqueued = false;
    if (matrix && T && b.prog->dim) MRK_HIP(hipMemcpyAsync(matrix, b.d_matrix.p, T * b.prog->dim * 8, hipMemcpyDeviceToHost, b.s()));
    // (Measured and removed, round 6: a leader of mrk_rank's front sleeping on a hipEventBlockingSync event instead of this polling
    // wait when several lanes are in flight - 183 k vs 183 k requests/s at 64 callers, 289 k vs 301 k at 128, profiles/r06_e_callers.txt.)
    MRK_HIP(hipStreamSynchronize(b.s()));
    const uint8_t *h = b.h_out.as<uint8_t>();
    if (scores && T) memcpy(scores, h, T * 8);
    if (order && T) memcpy(order, h + b.out_order_off, T * 4);
    hs = (const int32_t *)(h + b.out_status_off);
  }
  if (b.ran.values) fill_noop_outputs(b, scores, order);   // (a values run launches neither scorer nor sort)
  const int32_t *hl = hs + std::max(b.n_req, 1);
  for (int r = 0; r < b.n_req; ++r) b.h_status[(size_t)r] = hs[r] | hl[r];
  if (ctx->profile) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    drain_profile_events(ctx);
  }
}

}  // namespace mrk

using namespace mrk;

extern "C" {

// ---- training rows: what TrainBuffer.handleRanking asks ItemValue.fromState for (flow/TrainBuffer.scala:51-71)
static const Program &values_program_in(const Registry &reg, const char *model_name, int mode) {
  if (mode != MODE_ONLINE && mode != MODE_OFFLINE) throw StatusError(MRK_ERR_INVALID_ARG, "mode must be 0 (online) or 1 (offline)");
  const Program *p = reg.values_program(model_name, mode);
  if (!p) throw StatusError(MRK_ERR_NOT_FOUND, std::string("model ") + (model_name ? model_name : "<mapping>") + " is not configured");
  return *p;
}

static const Program &locked_values_program(mrk_ctx *ctx, const char *model_name, int mode) {
  if (!ctx) throw StatusError(MRK_ERR_INVALID_ARG, "null argument");
  std::shared_lock<std::shared_mutex> sl(ctx->store_mu);
  if (!ctx->registry) throw StatusError(MRK_ERR_INVALID_ARG, "mrk_config_load_json must be called first");
  const Program &p = values_program_in(*ctx->registry, model_name, mode);
  if (!p.d_ops.p)
    throw StatusError(MRK_ERR_UNSUPPORTED, "the mapping needs " + std::to_string(p.prep.size()) + " per-request reductions (interacted_with fields + diversity features); 32 are supported");
  return p;
}

int mrk_values(mrk_ctx *ctx, const char *model_name, int mode, const mrk_request *req, double *out_matrix) {
  return guard([&] {
    if (!ctx || !req || !out_matrix) throw StatusError(MRK_ERR_INVALID_ARG, "null argument");
    const Program &prog = locked_values_program(ctx, model_name, mode);
    std::lock_guard<std::mutex> vl(ctx->values_mu);
    MRK_HIP(hipSetDevice(ctx->device));
    if (!ctx->values_lane) {
      std::unique_ptr<mrk_batch> nb(new mrk_batch());
      MRK_HIP(hipStreamCreateWithFlags(&nb->stream, hipStreamNonBlocking));
      ctx->values_lane = nb.release();
    }
    mrk_batch &b = *ctx->values_lane;
    StoreAccess access(ctx, program_mutates_store(prog));
    if (b.ctx) MRK_HIP(hipStreamSynchronize(b.s()));  // a previous call that failed before its fetch may have left an upload from h_in in flight
    build_batch(ctx, prog, req, 1, nullptr, b);
    b.values = true;
    b.want_matrix = false;
    run_values(b);
    if (!b.ran.values_direct) {
      enqueue_fetch(b, false, false);
      b.fetch_enqueued = true;
    }
    access.release();   // (the rows are assembled: what follows needs no store)
    fetch_batch(b, nullptr, nullptr, out_matrix);
    std::string msg;
    const int code = status_to_code(b.h_status[0], msg);
    if (code != MRK_OK) throw StatusError(code, msg);
  });
}

int mrk_values_binary(mrk_ctx *ctx, const char *model_name, int mode, const uint8_t *event, size_t len, int *out_n_items, double *out_matrix, int capacity) {
  DecodedRequest dr;
  int rc = guard([&] {
    if (out_n_items) *out_n_items = 0;
    if (!event) throw StatusError(MRK_ERR_INVALID_ARG, "null event");
    dr.decode(event, len);
    if (out_n_items) *out_n_items = dr.req.n_items;
    if (dr.req.n_items > capacity) throw StatusError(MRK_ERR_INVALID_ARG, "the event has more items than the output buffer holds");
  });
  if (rc != MRK_OK) return rc;
  return mrk_values(ctx, model_name, mode, &dr.req, out_matrix);
}

int mrk_values_dim(mrk_ctx *ctx, const char *model_name) {
  int dim = -1;
  int rc = guard([&] {
    if (!ctx) throw StatusError(MRK_ERR_INVALID_ARG, "null argument");
    std::shared_lock<std::shared_mutex> lk(ctx->store_mu);
    if (!ctx->registry) throw StatusError(MRK_ERR_INVALID_ARG, "mrk_config_load_json must be called first");
    dim = values_program_in(*ctx->registry, model_name, MODE_OFFLINE).dim;
  });
  return rc == MRK_OK ? dim : rc;
}

// "<name>\t<first column>\t<dim>\t<single|vector|category>\n" per feature of a values program, in column order
static std::string values_columns_text(const Program &prog) {
  std::string text;
  for (const HostOp &ho : prog.host_ops) {
    const FeatureDef &f = *ho.def;
    // the MValue the reference's feature emits (feature/*.scala): CategoryValue for string encode: index and referer,
    // VectorValue for the list-valued features whatever their dim, SingleValue for the rest
    const bool category = f.category || (f.type == FType::String && f.index_encode);
    const bool vector = f.type == FType::Vector || (f.type == FType::String && !f.index_encode) || f.type == FType::WindowCount || f.type == FType::Rate ||
                        f.type == FType::InteractedWith || (f.type == FType::ExternalRanking && !f.category) || (f.type == FType::ExternalItem && f.dim > 1);
    text += f.name + "\t" + std::to_string(ho.dst) + "\t" + std::to_string(f.dim) + "\t" + (category ? "category" : vector ? "vector" : "single") + "\n";
  }
  return text;
}

static void copy_text(const std::string &text, char *out, size_t cap, size_t *needed) {
  *needed = text.size() + 1;
  if (!out || cap < text.size() + 1) throw StatusError(MRK_ERR_INVALID_ARG, "output buffer too small (see *needed)");
  memcpy(out, text.c_str(), text.size() + 1);
}

int mrk_values_columns(mrk_ctx *ctx, const char *model_name, char *out, size_t cap, size_t *needed) {
  return guard([&] {
    if (!ctx || !needed) throw StatusError(MRK_ERR_INVALID_ARG, "null argument");
    std::string text;
    {
      std::shared_lock<std::shared_mutex> lk(ctx->store_mu);
      if (!ctx->registry) throw StatusError(MRK_ERR_INVALID_ARG, "mrk_config_load_json must be called first");
      text = values_columns_text(values_program_in(*ctx->registry, model_name, MODE_OFFLINE));
    }
    copy_text(text, out, cap, needed);
  });
}

int mrk_config_values_columns(const char *json, size_t len, const char *model_name, char *out, size_t cap, size_t *needed) {
  return guard([&] {
    if (!json || !needed) throw StatusError(MRK_ERR_INVALID_ARG, "null argument");
    Store st;
    std::unique_ptr<Registry> reg = load_config(json, len, st, /*upload=*/false);
    copy_text(values_columns_text(values_program_in(*reg, model_name, MODE_OFFLINE)), out, cap, needed);
  });
}

int mrk_batch_create(mrk_ctx *ctx, mrk_batch **out) {
  return guard([&] {
    if (!out) throw StatusError(MRK_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    if (!ctx) throw StatusError(MRK_ERR_INVALID_ARG, "null context");
    { DeviceLock open(ctx); }   // (not held while the stream is made; the device stays selected for this thread)
    std::unique_ptr<mrk_batch> b(new mrk_batch());
    b->ctx = ctx;
    MRK_HIP(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    ctx_retain(ctx);
    *out = b.release();
  });
}

int mrk_batch_load(mrk_batch *batch, const char *model_name, const mrk_request *reqs, int n_req, const mrk_item_ids *ids) {
  return guard([&] {
    if (!batch || !batch->ctx || n_req < 0 || (n_req > 0 && !reqs)) throw StatusError(MRK_ERR_INVALID_ARG, "bad arguments");
    mrk_ctx *ctx = batch->ctx;
    const Program &prog = locked_program(ctx, model_name);
    std::lock_guard<std::mutex> bl(batch->bmu);
    MRK_HIP(hipSetDevice(ctx->device));
    MRK_HIP(hipStreamSynchronize(batch->s()));  // the previous run may still read the staging buffers
    StoreAccess access(ctx, program_mutates_store(prog));
    build_batch(ctx, prog, reqs, n_req, ids, *batch);
    batch->values = false;
  });
}

int mrk_batch_load_values(mrk_batch *batch, const char *model_name, int mode, const mrk_request *reqs, int n_req, const mrk_item_ids *ids) {
  return guard([&] {
    if (!batch || !batch->ctx || n_req < 0 || (n_req > 0 && !reqs)) throw StatusError(MRK_ERR_INVALID_ARG, "bad arguments");
    mrk_ctx *ctx = batch->ctx;
    const Program &prog = locked_values_program(ctx, model_name, mode);
    std::lock_guard<std::mutex> bl(batch->bmu);
    MRK_HIP(hipSetDevice(ctx->device));
    MRK_HIP(hipStreamSynchronize(batch->s()));  // the previous run may still read the staging buffers
    StoreAccess access(ctx, program_mutates_store(prog));
    build_batch(ctx, prog, reqs, n_req, ids, *batch);
    batch->values = true;
  });
}

int mrk_batch_prepare(mrk_ctx *ctx, const char *model_name, const mrk_request *reqs, int n_req, mrk_batch **out) {
  if (!out) { set_last_error("out is null"); return MRK_ERR_INVALID_ARG; }
  *out = nullptr;
  mrk_batch *b = nullptr;
  int rc = mrk_batch_create(ctx, &b);
  if (rc != MRK_OK) return rc;
  rc = mrk_batch_load(b, model_name, reqs, n_req, nullptr);
  if (rc == MRK_OK) rc = guard([&] { MRK_HIP(hipStreamSynchronize(b->s())); });
  if (rc != MRK_OK) {
    const std::string msg = mrk_last_error();
    mrk_batch_free(b);
    set_last_error(msg);
    return rc;
  }
  *out = b;
  return MRK_OK;
}

int mrk_batch_total_items(mrk_batch *batch) { return batch ? batch->total_items : MRK_ERR_INVALID_ARG; }

static void check_batch(mrk_batch *batch, mrk_model *model) {
  if (!batch || !batch->ctx) throw StatusError(MRK_ERR_INVALID_ARG, "null batch");
  if (!batch->prog) throw StatusError(MRK_ERR_INVALID_ARG, "the batch has not been loaded");
  if (model && model->ctx != batch->ctx) throw StatusError(MRK_ERR_INVALID_ARG, "model belongs to another context");
}

int mrk_batch_run(mrk_batch *batch, mrk_model *model) {
  return guard([&] {
    check_batch(batch, model);
    std::lock_guard<std::mutex> bl(batch->bmu);
    StoreAccess access(batch->ctx, false, /*flush=*/false);  // what the batch resolved against stays what it reads
    if (batch->values && !model) { run_values(*batch); return; }   // loaded by mrk_batch_load_values: the training rows
    run_batch(*batch, model);
  });
}

int mrk_batch_shard_chunk(mrk_batch *batch, int shard_count) {
  if (!batch || shard_count < 1) return MRK_ERR_INVALID_ARG;
  return shard_chunk(*batch, shard_count);
}

int mrk_batch_run_shard(mrk_batch *batch, mrk_model *model, int shard_index, int shard_count) {
  return guard([&] {
    check_batch(batch, model);
    if (shard_count < 1 || shard_count > 256 || shard_index < 0 || shard_index >= shard_count)
      throw StatusError(MRK_ERR_INVALID_ARG, "bad shard index / count (1..256 shards)");
    std::lock_guard<std::mutex> bl(batch->bmu);
    StoreAccess access(batch->ctx, false, false);
    int64_t lo = 0, hi = 0;
    if (mrk_shard_range(batch->total_items, shard_index, shard_count, &lo, &hi) != MRK_OK) throw StatusError(MRK_ERR_INVALID_ARG, "bad shard");
    run_batch(*batch, model, (int)lo, (int)hi, false);
  });
}

int mrk_batch_allgather_scores(mrk_batch *batch) {
  return guard([&] {
    check_batch(batch, nullptr);
    std::lock_guard<std::mutex> bl(batch->bmu);
    mrk_ctx *ctx = batch->ctx;
    if (!ctx->comm) return;  // no communicator: a world of one, nothing to merge
    MRK_HIP(hipSetDevice(ctx->device));
    // the score buffer has room for the padded chunks of up to 256 shards (build_batch)
    comm_allgather_f64_inplace(ctx, batch->view.scores, (size_t)shard_chunk(*batch, ctx->comm_world), batch->s());
    // the status words too: an item that fails its request lies in ONE rank's slice, every rank must report it
    if (batch->n_req > 0) {
      batch->d_gather_status.reserve((size_t)ctx->comm_world * batch->n_req * 4);
      comm_allgather_i32(ctx, batch->view.status, batch->d_gather_status.as<int32_t>(), (size_t)batch->n_req, batch->s());
      launch_status_or(batch->s(), batch->d_gather_status.as<int32_t>(), ctx->comm_world, batch->n_req, batch->view.status);
    }
    batch->fetch_enqueued = false;
  });
}

int mrk_batch_run_sharded(mrk_batch *batch, mrk_model *model) {
  if (!batch || !batch->ctx) { set_last_error("null batch"); return MRK_ERR_INVALID_ARG; }
  mrk_ctx *ctx = batch->ctx;
  if (!ctx->comm) return mrk_batch_run(batch, model);
  int rc = mrk_batch_run_shard(batch, model, ctx->comm_rank, ctx->comm_world);
  if (rc == MRK_OK) rc = mrk_batch_allgather_scores(batch);
  if (rc == MRK_OK) rc = mrk_batch_sort(batch);
  return rc;
}

int mrk_batch_gather_scores(mrk_batch *batch, double **d_all_scores) {
  return guard([&] {
    check_batch(batch, nullptr);
    if (!d_all_scores) throw StatusError(MRK_ERR_INVALID_ARG, "null output");
    std::lock_guard<std::mutex> bl(batch->bmu);
    mrk_ctx *ctx = batch->ctx;
    const size_t T = (size_t)batch->total_items;
    MRK_HIP(hipSetDevice(ctx->device));
    if (!ctx->comm) { *d_all_scores = batch->view.scores; return; }
    batch->d_gather.reserve(std::max<size_t>(T * (size_t)ctx->comm_world, 1) * 8);
    comm_allgather_f64(ctx, batch->view.scores, batch->d_gather.as<double>(), T, batch->s());
    *d_all_scores = batch->d_gather.as<double>();
  });
}

int mrk_batch_sort(mrk_batch *batch) {
  return guard([&] {
    check_batch(batch, nullptr);
    std::lock_guard<std::mutex> bl(batch->bmu);
    MRK_HIP(hipSetDevice(batch->ctx->device));
    LaunchOn on(batch->ctx, batch->s());
    batch->fetch_enqueued = false;
    sort_batch(*batch);
  });
}

void *mrk_batch_stream(mrk_batch *batch) { return batch ? (void *)batch->s() : nullptr; }

int mrk_batch_sync(mrk_batch *batch) {
  return guard([&] {
    if (!batch) throw StatusError(MRK_ERR_INVALID_ARG, "null batch");
    MRK_HIP(hipSetDevice(batch->ctx->device));
    MRK_HIP(hipStreamSynchronize(batch->s()));
    if (batch->ctx->profile) {
      std::lock_guard<std::mutex> lk(batch->ctx->mu);
      drain_profile_events(batch->ctx);
    }
  });
}

int mrk_batch_device_outputs(mrk_batch *batch, double **d_scores, int32_t **d_order, double **d_matrix) {
  return guard([&] {
    check_batch(batch, nullptr);
    std::lock_guard<std::mutex> bl(batch->bmu);
    if (d_scores) *d_scores = batch->view.scores;
    if (d_order) *d_order = batch->view.order;
    if (d_matrix) {  // from now on every run materialises the f64 matrix
      batch->want_matrix = true;
      *d_matrix = batch->view.matrix;
    }
  });
}

int mrk_batch_fetch(mrk_batch *batch, double *out_scores, int32_t *out_order, double *out_matrix) {
  return guard([&] {
    check_batch(batch, nullptr);
    std::lock_guard<std::mutex> bl(batch->bmu);
    StoreAccess access(batch->ctx, false, false);
    fetch_batch(*batch, out_scores, out_order, out_matrix);
  });
}

int mrk_batch_enqueue_fetch(mrk_batch *batch) {
  return guard([&] {
    check_batch(batch, nullptr);
    std::lock_guard<std::mutex> bl(batch->bmu);
    MRK_HIP(hipSetDevice(batch->ctx->device));
    enqueue_fetch(*batch, true, true);
    batch->fetch_enqueued = true;
  });
}

int mrk_batch_host_outputs(mrk_batch *batch, const double **scores, const int32_t **order, const int32_t **status) {
  return guard([&] {
    check_batch(batch, nullptr);
    std::lock_guard<std::mutex> bl(batch->bmu);
    MRK_HIP(hipSetDevice(batch->ctx->device));
    if (!batch->fetch_enqueued) {  // mrk_batch_enqueue_fetch was not called behind the run: ask for everything now
      enqueue_fetch(*batch, true, true);
      batch->fetch_enqueued = true;
    }
    fetch_batch(*batch, nullptr, nullptr, nullptr);  // waits for the batch; status words -> h_status
    if (batch->ran.values) {   // (a values run launches neither scorer nor sort)
      batch->h_out.reserve(batch->out_bytes);
      fill_noop_outputs(*batch, batch->h_out.as<double>(), (int32_t *)(batch->h_out.as<uint8_t>() + batch->out_order_off));
    }
    const uint8_t *h = batch->h_out.as<uint8_t>();
    if (scores) *scores = (const double *)h;
    if (order) *order = (const int32_t *)(h + batch->out_order_off);
    if (status) {
      batch->codes.resize((size_t)std::max(batch->n_req, 1));
      std::string msg;
      for (int r = 0; r < batch->n_req; ++r) batch->codes[(size_t)r] = status_to_code(batch->h_status[(size_t)r], msg);
      *status = batch->codes.data();
    }
  });
}

void *mrk_host_alloc(size_t bytes) {
  void *p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return p;
}

void mrk_host_free(void *p) {
  if (p) (void)hipHostFree(p);
}

int mrk_batch_status(mrk_batch *batch, int32_t *out_status) {
  return guard([&] {
    check_batch(batch, nullptr);
    if (!out_status) throw StatusError(MRK_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> bl(batch->bmu);
    fetch_batch(*batch, nullptr, nullptr, nullptr);
    for (int r = 0; r < batch->n_req; ++r) {
      std::string msg;
      out_status[r] = status_to_code(batch->h_status[r], msg);
    }
  });
}

void mrk_batch_free(mrk_batch *batch) {
  if (!batch) return;
  mrk_ctx *ctx = batch->ctx;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(batch->s());
    if (batch->stream) (void)hipStreamDestroy(batch->stream);
    delete batch;
    ctx_release(ctx);
  } else {
    delete batch;
  }
}

}  // extern "C"
