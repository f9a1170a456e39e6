// Config, feature store and mrk_debug_* entry points of the C ABI (include/mrk.h).
#include <cstring>

#include "rank_host.hpp"

namespace mrk {

static Store &store_of(mrk_ctx *ctx) {
  if (!ctx) throw StatusError(MRK_ERR_INVALID_ARG, "null context");
  if (!ctx->store) throw StatusError(MRK_ERR_INVALID_ARG, "mrk_config_load_json must be called first");
  return *ctx->store;
}

const Program &program_of(mrk_ctx *ctx, const char *model_name) {
  if (!ctx || !model_name) throw StatusError(MRK_ERR_INVALID_ARG, "null argument");
  if (!ctx->registry) throw StatusError(MRK_ERR_INVALID_ARG, "mrk_config_load_json must be called first");
  const Program *p = ctx->registry->program(model_name);
  if (!p) throw StatusError(MRK_ERR_NOT_FOUND, std::string("model ") + model_name + " is not configured");
  return *p;
}

const Program &locked_program(mrk_ctx *ctx, const char *model_name) {
  std::shared_lock<std::shared_mutex> sl(ctx->store_mu);
  return program_of(ctx, model_name);
}

}  // namespace mrk

using namespace mrk;

extern "C" {

int mrk_config_load_json(mrk_ctx *ctx, const char *json, size_t len) {
  return guard([&] {
    if (!ctx || !json) throw StatusError(MRK_ERR_INVALID_ARG, "null argument");
    StoreWriteLock sl(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->registry) throw StatusError(MRK_ERR_INVALID_ARG, "this context already has a configuration");
    MRK_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<Store> st(new Store());
    std::unique_ptr<Registry> reg = load_config(json, len, *st);
    ctx->store = st.release();
    ctx->registry = reg.release();
  });
}

int mrk_config_specialize(const char *json, size_t len, const char *model_name, int f64, int what, uint8_t *out, size_t cap, size_t *needed) {
  return guard([&] {
    const int kernel = (what >> 8) - 1;  // what = (1 + kernel) << 8 | form: one kernel's translation unit; high byte 0: all kernels
    what &= 0xff;
    if (!json || !model_name || !needed || (what != 0 && what != 1) || kernel < JIT_ALL || kernel > JIT_ITEMS_RT || kernel == JIT_UNUSED)  // (the two kernels of forests scored by the tree walk: JIT_ALL shows them, mrk_config_precompile builds them)
      throw StatusError(MRK_ERR_INVALID_ARG, "null argument / unknown `what`");
    Store st;
    std::unique_ptr<Registry> reg = load_config(json, len, st, /*upload=*/false);
    const Program *p = reg->program(model_name);
    if (!p) throw StatusError(MRK_ERR_NOT_FOUND, std::string("model ") + model_name + " is not configured");
    const std::string src = jit_source(*p, f64 != 0, kernel);
    std::vector<char> code;
    if (what == 1 && out) {  // sizing calls (out == NULL) do not compile
      std::string log;
      code = jit_compile(src, log);
    }
    const char *data = what == 0 ? src.data() : code.data();
    const size_t n = what == 0 ? src.size() : code.size();
    *needed = what == 1 && !out ? (size_t)1 << 22 : n;  // code objects: an upper bound for the sizing call
    if (cap < n || !out) throw StatusError(MRK_ERR_INVALID_ARG, "output buffer too small (see *needed)");
    memcpy(out, data, n);
  });
}

int mrk_config_specialize_values(const char *json, size_t len, const char *model_name, int mode, int what, uint8_t *out, size_t cap, size_t *needed) {
  return guard([&] {
    const int kernel = (what >> 8) - 1;  // as mrk_config_specialize; the values kernel (1 + JIT_VALUES) included
    what &= 0xff;
    if (!json || !needed || (what != 0 && what != 1) || kernel < JIT_ALL || kernel > JIT_VALUES || kernel == JIT_UNUSED) throw StatusError(MRK_ERR_INVALID_ARG, "null argument / unknown `what`");
    if (mode != MODE_ONLINE && mode != MODE_OFFLINE) throw StatusError(MRK_ERR_INVALID_ARG, "mode must be 0 (online) or 1 (offline)");
    Store st;
    std::unique_ptr<Registry> reg = load_config(json, len, st, /*upload=*/false);
    const Program *p = reg->values_program(model_name, mode);
    if (!p) throw StatusError(MRK_ERR_NOT_FOUND, std::string("model ") + (model_name ? model_name : "<mapping>") + " is not configured");
    const std::string src = jit_source(*p, true, kernel);
    std::vector<char> code;
    if (what == 1 && out) {  // sizing calls (out == NULL) do not compile
      std::string log;
      code = jit_compile(src, log);
    }
    const char *data = what == 0 ? src.data() : code.data();
    const size_t n = what == 0 ? src.size() : code.size();
    *needed = what == 1 && !out ? (size_t)1 << 22 : n;
    if (cap < n || !out) throw StatusError(MRK_ERR_INVALID_ARG, "output buffer too small (see *needed)");
    memcpy(out, data, n);
  });
}

// host only: the view signature of a serialised booster (what mrk_model_load would key this model's kernels by)
static QsSignature signature_of_bytes(int backend, const uint8_t *bytes, size_t len, bool &f64) {
  if (!bytes || !len) throw StatusError(MRK_ERR_INVALID_ARG, "null model bytes");
  const Forest f = parse_booster(backend, bytes, len);
  f64 = f.backend == Backend::LightGBM;
  const PackedForestQS qs = pack_forest_qs(f, f.n_features);
  return qs.ok ? qs_signature(qs, qs_stage_cap(qs)) : QsSignature{};
}

int mrk_config_specialize_for_model(const char *json, size_t len, const char *model_name, int backend, const uint8_t *model_bytes, size_t model_len,
                                    int what, uint8_t *out, size_t cap, size_t *needed) {
  return guard([&] {
    const int kernel = (what >> 8) - 1;
    what &= 0xff;
    if (!json || !model_name || !needed || (what != 0 && what != 1) || kernel < JIT_ALL || kernel > JIT_ITEMS_RT || kernel == JIT_UNUSED)  // (the two kernels of forests scored by the tree walk: JIT_ALL shows them, mrk_config_precompile builds them)
      throw StatusError(MRK_ERR_INVALID_ARG, "null argument / unknown `what`");
    bool f64 = true;
    const QsSignature sig = signature_of_bytes(backend, model_bytes, model_len, f64);
    Store st;
    std::unique_ptr<Registry> reg = load_config(json, len, st, /*upload=*/false);
    const Program *p = reg->program(model_name);
    if (!p) throw StatusError(MRK_ERR_NOT_FOUND, std::string("model ") + model_name + " is not configured");
    const std::string src = jit_source(*p, f64, kernel, switches().jit_sig ? &sig : nullptr);
    std::vector<char> code;
    if (what == 1 && out) {
      std::string log;
      code = jit_compile(src, log);
    }
    const char *data = what == 0 ? src.data() : code.data();
    const size_t n = what == 0 ? src.size() : code.size();
    *needed = what == 1 && !out ? (size_t)1 << 22 : n;
    if (cap < n || !out) throw StatusError(MRK_ERR_INVALID_ARG, "output buffer too small (see *needed)");
    memcpy(out, data, n);
  });
}

int mrk_config_precompile_for_model(const char *json, size_t len, const char *model_name, int backend, const uint8_t *model_bytes, size_t model_len,
                                    unsigned kernel_mask, const char *dir, int *out_compiled) {
  return guard([&] {
    if (out_compiled) *out_compiled = 0;
    if (!json || !model_name || !dir) throw StatusError(MRK_ERR_INVALID_ARG, "null argument");
    bool f64 = true;
    const QsSignature sig = signature_of_bytes(backend, model_bytes, model_len, f64);
    Store st;
    std::unique_ptr<Registry> reg = load_config(json, len, st, /*upload=*/false);
    const Program *p = reg->program(model_name);
    if (!p) throw StatusError(MRK_ERR_NOT_FOUND, std::string("model ") + model_name + " is not configured");
    const int n = jit_precompile(*p, f64, kernel_mask, dir, &sig);
    if (out_compiled) *out_compiled = n;
  });
}

int mrk_config_precompile(const char *json, size_t len, const char *model_name, int f64, unsigned kernel_mask, const char *dir, int *out_compiled) {
  return guard([&] {
    if (out_compiled) *out_compiled = 0;
    if (!json || !model_name || !dir) throw StatusError(MRK_ERR_INVALID_ARG, "null argument");
    Store st;
    std::unique_ptr<Registry> reg = load_config(json, len, st, /*upload=*/false);
    const Program *p = reg->program(model_name);
    if (!p) throw StatusError(MRK_ERR_NOT_FOUND, std::string("model ") + model_name + " is not configured");
    const int n = jit_precompile(*p, f64 != 0, kernel_mask, dir);
    if (out_compiled) *out_compiled = n;
  });
}

int mrk_config_warmup(mrk_ctx *ctx, const char *model_name) {
  return guard([&] {
    if (!ctx || !model_name) throw StatusError(MRK_ERR_INVALID_ARG, "null argument");
    const Program *p;
    {
      std::shared_lock<std::shared_mutex> sl(ctx->store_mu);
      p = &program_of(ctx, model_name);
    }
    jit_wait(*p);
  });
}

int mrk_config_kernel_keys(mrk_ctx *ctx, const char *model_name, char *out, size_t cap, size_t *needed) {
  return guard([&] {
    if (!ctx || !model_name || !needed) throw StatusError(MRK_ERR_INVALID_ARG, "null argument");
    const Program *p;
    {
      std::shared_lock<std::shared_mutex> sl(ctx->store_mu);
      p = &program_of(ctx, model_name);
    }
    const std::string keys = jit_loaded_keys(*p);
    *needed = keys.size() + 1;
    if (!out || cap < keys.size() + 1) throw StatusError(MRK_ERR_INVALID_ARG, "output buffer too small (see *needed)");
    memcpy(out, keys.c_str(), keys.size() + 1);
  });
}

#ifdef MRK_PHASE_CLOCKS
extern "C" int mrk_debug_phase_clocks(const mrk::Program *prog, unsigned long long *out64);
// measurement builds only (not part of include/mrk.h): read-and-reset the per-phase cycle sums of the specialised kernel
int mrk_debug_phase(mrk_ctx *ctx, const char *model_name, unsigned long long *out64) {
  if (!ctx || !ctx->registry) return -1;
  std::lock_guard<std::mutex> lk(ctx->mu);
  (void)hipDeviceSynchronize();
  return mrk_debug_phase_clocks(ctx->registry->program(model_name), out64);
}
#endif

int mrk_model_dim(mrk_ctx *ctx, const char *model_name) {
  int dim = -1;
  int rc = guard([&] {
    if (!ctx || !model_name) throw StatusError(MRK_ERR_INVALID_ARG, "null argument");
    std::shared_lock<std::shared_mutex> lk(ctx->store_mu);
    if (!ctx->registry) throw StatusError(MRK_ERR_INVALID_ARG, "mrk_config_load_json must be called first");
    const Program *p = ctx->registry->program(model_name);
    if (!p) throw StatusError(MRK_ERR_NOT_FOUND, std::string("model ") + model_name + " is not configured");
    dim = p->dim;
  });
  return rc == MRK_OK ? dim : rc;
}

int mrk_config_bind_termfreq(mrk_ctx *ctx, const char *feature, const char *json_bytes, size_t len) {
  return guard([&] {
    if (!ctx || !feature || !json_bytes) throw StatusError(MRK_ERR_INVALID_ARG, "mrk_config_bind_termfreq: null argument");
    bind_termfreq(ctx, feature, json_bytes, len);
  });
}

#define STORE_PUT(call)                                   \
  return guard([&] {                                      \
    if (!key) throw StatusError(MRK_ERR_INVALID_ARG, "null key"); \
    Store &st = store_of(ctx);                            \
    StoreWriteLock lk(ctx); \
    (void)st.call;                                        \
  })

int mrk_store_put_double(mrk_ctx *ctx, const char *key, double v) { STORE_PUT(put_double(key, v)); }
int mrk_store_put_bool(mrk_ctx *ctx, const char *key, int v) { STORE_PUT(put_bool(key, v != 0)); }
int mrk_store_put_string(mrk_ctx *ctx, const char *key, const char *v) { STORE_PUT(put_string(key, v)); }
int mrk_store_put_string_list(mrk_ctx *ctx, const char *key, const char *const *v, int n) { STORE_PUT(put_string_list(key, v, n)); }
int mrk_store_put_double_list(mrk_ctx *ctx, const char *key, const double *v, int n) { STORE_PUT(put_double_list(key, v, n)); }
int mrk_store_put_counter(mrk_ctx *ctx, const char *key, int64_t v) { STORE_PUT(put_counter(key, v)); }
int mrk_store_put_periodic(mrk_ctx *ctx, const char *key, const int64_t *v, int n) { STORE_PUT(put_periodic(key, v, n)); }
int mrk_store_put_bounded_list(mrk_ctx *ctx, const char *key, const char *const *v, int n) { STORE_PUT(put_bounded_list(key, v, n)); }
int mrk_store_delete(mrk_ctx *ctx, const char *key) { STORE_PUT(erase(key)); }
int mrk_store_increment_periodic(mrk_ctx *ctx, const char *key, int64_t ts_ms, int64_t inc) { STORE_PUT(increment_periodic(key, ts_ms, inc)); }
static int put_binary(mrk_ctx *ctx, const uint8_t *bytes, size_t len, int64_t now_ms, int *out_records) {
  return guard([&] {
    if (out_records) *out_records = 0;
    if (!bytes && len) throw StatusError(MRK_ERR_INVALID_ARG, "null blob");
    Store &st = store_of(ctx);
    StoreWriteLock lk(ctx);
    const int n = load_feature_values(st, bytes, len, now_ms);
    if (out_records) *out_records = n;
  });
}

int mrk_store_put_binary(mrk_ctx *ctx, const uint8_t *bytes, size_t len, int *out_records) { return put_binary(ctx, bytes, len, -1, out_records); }

int mrk_store_put_binary_at(mrk_ctx *ctx, const uint8_t *bytes, size_t len, int64_t now_ms, int *out_records) {
  if (now_ms < 0) { set_last_error("mrk_store_put_binary_at: negative clock"); return MRK_ERR_INVALID_ARG; }
  return put_binary(ctx, bytes, len, now_ms, out_records);
}

int mrk_store_expire(mrk_ctx *ctx, int64_t now_ms, int64_t *out_expired) {
  return guard([&] {
    if (out_expired) *out_expired = 0;
    Store &st = store_of(ctx);
    StoreWriteLock lk(ctx);
    const int64_t n = st.ttl_expire(now_ms);
    if (out_expired) *out_expired = n;
  });
}

int mrk_store_increment_periodic_batch(mrk_ctx *ctx, const char *const *keys, const int64_t *ts_ms, const int64_t *inc, int n) {
  return guard([&] {
    if (n < 0 || (n > 0 && (!keys || !ts_ms || !inc))) throw StatusError(MRK_ERR_INVALID_ARG, "bad increment batch");
    Store &st = store_of(ctx);
    StoreWriteLock lk(ctx);
    for (int i = 0; i < n; ++i) {
      if (!keys[i]) throw StatusError(MRK_ERR_INVALID_ARG, "null key");
      (void)st.increment_periodic(keys[i], ts_ms[i], inc[i]);
    }
  });
}
int mrk_store_increment(mrk_ctx *ctx, const char *key, int64_t inc) { STORE_PUT(increment(key, inc)); }
int mrk_store_append(mrk_ctx *ctx, const char *key, const char *value, int64_t ts_ms) { STORE_PUT(append(key, value, ts_ms)); }

/* not part of include/mrk.h (measurement aid, Store::clone_items): grows the ITEM table to (copies + 1) x its size */
// launch_shape.hpp through the C ABI, for tests without a device: out = {lanes per workgroup, op split, slices}
int mrk_debug_fused_shape(int n_req, int max_items, int *out3) {
  const mrk::FusedShape s = mrk::fused_launch_shape(n_req, max_items);
  out3[0] = s.threads();
  out3[1] = s.split;
  out3[2] = s.slices;
  return MRK_OK;
}
// rank_plan.hpp through the C ABI, for tests without a device, under the DEFAULT switches but for the three the table varies.
// in[24] = {n_req, candidates per request, the largest request's table entries, its median values, compact_tables, overrides,
// want_matrix, normalises, n_prep, dim | model: present, bit-vector image, f64, thr_cap, n_views, rt_doubles, max_chunk_bytes,
// max_chunk_trees | lo, hi (-1: every item), sort, direct | MRK_RANK_ONE_WALK (-1 unset), MRK_SCORER=walk};
// out8 = {path (RankPath), kernel (JIT_*, -2 none), items_rt, prepass, keyed, whole_matrix, entry_bytes, split_kernel};
// values != 0: plan_values instead - out8 = {one launch, kernel}
int mrk_debug_rank_plan(const int64_t *in, int values, int64_t *out8) {
  mrk::Switches sw;
  sw.rank_one_walk = (int)in[22];
  sw.scorer_walk = in[23] != 0;
  mrk::BatchShape b;
  b.n_req = (int)in[0]; b.max_items = (int)in[1]; b.total_items = b.n_req * b.max_items;
  b.compact_tables = in[4] != 0; b.overrides = in[5] != 0; b.want_matrix = in[6] != 0; b.normalises = in[7] != 0;
  b.n_prep = (int)in[8]; b.dim = (int)in[9];
  mrk::fused_batch_shape(b, (uint64_t)in[2], (int)in[3], sw);
  mrk::ModelShape m;
  m.present = in[10] != 0; m.qs_ok = in[11] != 0; m.f64 = in[12] != 0;
  m.thr_cap = (uint32_t)in[13]; m.n_views = (int)in[14]; m.rt_doubles = (uint32_t)in[15];
  m.max_chunk_bytes = (size_t)in[16]; m.max_chunk_trees = (int)in[17];
  for (int i = 0; i < 8; ++i) out8[i] = 0;
  if (values) {
    const mrk::ValuesPlan v = mrk::plan_values(b, sw);
    out8[0] = v.one; out8[1] = v.kernel;
    return MRK_OK;
  }
  const mrk::RankPlan p = mrk::plan_rank(b, m, sw, (int)in[18], in[19] < 0 ? b.total_items : (int)in[19], in[20] != 0, in[21] != 0);
  out8[0] = (int64_t)p.path; out8[1] = p.kernel; out8[2] = p.items_rt; out8[3] = p.prepass; out8[4] = p.keyed; out8[5] = p.whole_matrix;
  out8[6] = p.entry_bytes; out8[7] = p.split_kernel;
  return MRK_OK;
}
int mrk_debug_scorer_split(int rows, int views, int f64, int n_cus) {
  return mrk::scorer_waves_per_tile(((long long)rows + mrk::QS_TILE_ROWS - 1) / mrk::QS_TILE_ROWS, views, f64 != 0, n_cus, mrk::QS_LEAVES, mrk::QS_TILE_ROWS);
}

// launch_shape.hpp rank_one_walk_lds_bytes with the trees per round the library would choose (walk_leaf_trees) (*out_leaf_trees)
int64_t mrk_debug_walk_lds(int cols, int f64, int64_t chunk_bytes, int chunk_trees, int64_t assembly_bytes, int *out_leaf_trees) {
  const int lt = mrk::walk_leaf_trees(chunk_trees);
  if (out_leaf_trees) *out_leaf_trees = lt;
  return (int64_t)mrk::rank_one_walk_lds_bytes(cols, f64 != 0, (size_t)chunk_bytes, chunk_trees, lt, (size_t)assembly_bytes);
}

int mrk_debug_clone_items(mrk_ctx *ctx, int copies, int64_t *out_items) {
  return guard([&] {
    Store &st = store_of(ctx);
    StoreWriteLock lk(ctx);
    const uint32_t n = st.clone_items(copies);
    if (out_items) *out_items = n;
  });
}

/* not part of include/mrk.h: layout of one scope's table - out[0..5] = slots, record stride, first byte of the inline heap,
 * heap bytes, token pool entries, f64 pool entries (benchmarks report bytes per record from it) */
int mrk_debug_store_info(mrk_ctx *ctx, int scope, int64_t *out) {
  return guard([&] {
    Store &st = store_of(ctx);
    if (scope < 0 || scope >= SC_COUNT || !out) throw StatusError(MRK_ERR_INVALID_ARG, "bad scope");
    std::shared_lock<std::shared_mutex> lk(ctx->store_mu);
    const Table &t = st.tables[scope];
    out[0] = t.n_slots; out[1] = t.stride; out[2] = t.heap_off; out[3] = t.heap_cap;
    out[4] = (int64_t)st.tok_pool.host.size(); out[5] = (int64_t)st.f64_pool.host.size();
  });
}

/* not part of include/mrk.h: the pre-pass hash tables of a loaded batch as the host sized them - out3 = {fused_entries (the
 * largest request's table entries: what the fused launch's LDS is sized by), requests, tables per request}; caps (n_caps >=
 * requests x tables, or NULL) receives every request's per-table capacity in entries, request-major (tests, measurement notes) */
int mrk_debug_batch_tables(mrk_batch *b, int64_t *out3, uint32_t *caps, int64_t n_caps) {
  return guard([&] {
    if (!b || !b->prog || !out3) throw StatusError(MRK_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(b->bmu);
    const size_t n_prep = b->prog->prep.size(), n = (size_t)b->n_req * n_prep;
    out3[0] = b->sh.fused_entries; out3[1] = b->n_req; out3[2] = (int64_t)n_prep;
    if (!caps) return;
    if (n_caps < (int64_t)n || b->hb.prep_out.size() < n) throw StatusError(MRK_ERR_INVALID_ARG, "caps is too short");
    for (size_t i = 0; i < n; ++i) caps[i] = b->hb.prep_out[i].tab_cap;
  });
}

/* not part of include/mrk.h: the fused cells launch of a batch's last run - out10 = {bytes of a table entry in the kernel that ran
 * (4: the compact form, 8: the wide one, 0: the run had no such launch), the launch's dynamic LDS bytes, the kernel (0 the
 * interpreting one, 1 mrk_jit_rank_cells, 2 mrk_jit_rank_cells_split), 1 if every table of the batch fits the compact entry,
 * then what the LDS was sized from: table entries, median values, threads, threshold staging doubles, resident threshold bytes,
 * 1 if sized for the split kernel}.  The launch's own figures ([0] - [2], [7] - [9]) are what that launch recorded: all 0 after a run
 * without a fused cells launch (one launch, item-parallel, matrix) - [7] - [9] used to keep an earlier launch's values or, for [9], the batch's shape */
int mrk_debug_batch_launch(mrk_batch *b, int64_t *out10) {
  return guard([&] {
    if (!b || !out10) throw StatusError(MRK_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(b->bmu);
    out10[0] = b->ran.entry_bytes; out10[1] = (int64_t)b->ran.lds; out10[2] = b->ran.kernel; out10[3] = b->sh.compact_tables ? 1 : 0;
    out10[4] = b->sh.fused_entries; out10[5] = b->sh.fused_vals; out10[6] = b->sh.fused_threads; out10[7] = b->ran.thr_cap; out10[8] = (int64_t)b->ran.rt_bytes;
    out10[9] = b->ran.split_sized ? 1 : 0;
  });
}

/* not part of include/mrk.h, host only: the arithmetic of the two rules above - out2 = {1 if a table with `insertions` inserted
 * tokens over a column whose largest token id is `max_token` fits the compact entry (features.hpp compact_table_ok), the dynamic
 * LDS bytes of a fused launch (launch_shape.hpp fused_lds_bytes)} */
int mrk_debug_fused_lds(int64_t insertions, int64_t max_token, int64_t tab_entries, int64_t vals_cap, int64_t threads, int64_t thr_cap, int64_t rt_bytes,
                        int split, int entry_bytes, int64_t *out2) {
  return guard([&] {
    if (!out2 || insertions < 0 || max_token < 0 || (entry_bytes != 4 && entry_bytes != 8)) throw StatusError(MRK_ERR_INVALID_ARG, "bad argument");
    out2[0] = compact_table_ok((uint64_t)insertions, (uint32_t)std::min<int64_t>(max_token, 0xffffffffll)) ? 1 : 0;
    out2[1] = (int64_t)fused_lds_bytes((uint32_t)tab_entries, (int)vals_cap, (int)threads, (uint32_t)thr_cap, (size_t)rt_bytes, split != 0, entry_bytes);
  });
}

/* not part of include/mrk.h: the distinct tokens ever stored in one ITEM-scope column (Column::distinct: the bound of
 * features.cpp table_capacity), -1 = no such column */
int mrk_debug_column_distinct(mrk_ctx *ctx, const char *column, int64_t *out) {
  return guard([&] {
    Store &st = store_of(ctx);
    if (!column || !out) throw StatusError(MRK_ERR_INVALID_ARG, "null argument");
    std::shared_lock<std::shared_mutex> lk(ctx->store_mu);
    const Table &t = st.tables[SC_ITEM];
    auto it = t.col_of.find(column);
    *out = it == t.col_of.end() ? -1 : (int64_t)t.cols[(size_t)it->second].distinct;
  });
}

int mrk_store_flush(mrk_ctx *ctx) {
  return guard([&] {
    Store &st = store_of(ctx);
    StoreWriteLock lk(ctx);
    MRK_HIP(hipSetDevice(ctx->device));
    st.flush(ctx->stream);
  });
}

}  // extern "C"
