// C ABI (include/mrk.h) of the trending recommender: POST /recommend's TrendingPredictor.fit / load and TrendingModel.predict /
// save (ml/recommend/TrendingRecommender.scala:39-133).  The aggregate over the history is trending.hip; config, interning,
// `now`, pow tables and the bitstream are trending_host.cpp.  A finished model is a host object.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "runtime.hpp"
#include "trending.hpp"
#include "trending_host.hpp"

using namespace mrk;

struct mrk_trending_builder {
  mrk_ctx *ctx = nullptr;
  TrendingConfig cfg;
  TrendingStream st;
  std::mutex mu;              // one add / fit at a time; lock order: mu before ctx->mu
  bool broken = false;        // an add failed half-way: the staged arrays and the id table no longer agree
  // staged interactions on the device, SoA, `cap` entries each
  DevBuf d_item, d_widx, d_ts;
  int64_t cap = 0;
  PinBuf pin;
};

struct mrk_trending {
  TrendingModel m;
};

namespace {

constexpr int64_t PIECE = int64_t(1) << 20;   // interactions per pinned piece of an upload (16 MiB)

// room for `total` staged interactions; what is staged already moves over.  Caller holds ctx->mu.
void grow(mrk_trending_builder *b, int64_t total) {
  if (total <= b->cap) return;
  const int64_t cap = std::min<int64_t>(TRENDING_MAX_INTERACTIONS, std::max<int64_t>({total, b->cap * 2, int64_t(1) << 16}));
  DevBuf item, widx, ts;
  item.reserve((size_t)cap * 4);
  widx.reserve((size_t)cap * 4);
  ts.reserve((size_t)cap * 8);
  const size_t have = (size_t)b->st.interactions;
  if (have) {
    hipStream_t s = b->ctx->stream;
    MRK_HIP(hipMemcpyAsync(item.p, b->d_item.p, have * 4, hipMemcpyDeviceToDevice, s));
    MRK_HIP(hipMemcpyAsync(widx.p, b->d_widx.p, have * 4, hipMemcpyDeviceToDevice, s));
    MRK_HIP(hipMemcpyAsync(ts.p, b->d_ts.p, have * 8, hipMemcpyDeviceToDevice, s));
    MRK_HIP(hipStreamSynchronize(s));
  }
  b->d_item = std::move(item);
  b->d_widx = std::move(widx);
  b->d_ts = std::move(ts);
  b->cap = cap;
}

int count_mode() {
  const char *e = getenv("MRK_TRENDING_COUNT");   // read per fit, never on a launch path of the serving side
  return e && !strcmp(e, "plain") ? TRENDING_COUNT_PLAIN : TRENDING_COUNT_COMBINE;
}

void fit_locked(mrk_trending_builder *b, TrendingModel &out) {
  mrk_ctx *ctx = b->ctx;
  const TrendingConfig &cfg = b->cfg;
  const int64_t n = b->st.interactions, items = (int64_t)b->st.ids.size();
  const int64_t total_days = cfg.total_days();
  const int n_weights = (int)cfg.weights.size();
  DeviceLock lk(ctx);
  hipStream_t s = lk.stream;
  // limits: the count table must fit what is free beside the staged interactions (no chunked fit)
  const size_t order_scratch = trending_order_scratch_bytes((int)items);
  const double table_bytes = 4.0 * (double)items * (double)total_days;
  const double other_bytes = 12.0 * (double)items + (double)order_scratch + 8.0 * (double)total_days + 64.0 * (n_weights + 1) + 4096;
  size_t free_b = 0, total_b = 0;
  MRK_HIP(hipMemGetInfo(&free_b, &total_b));
  if (table_bytes + other_bytes > (double)free_b)
    throw StatusError(MRK_ERR_UNSUPPORTED, "trending: the count table of " + std::to_string(items) + " items x " + std::to_string(total_days) + " days (" +
                                               std::to_string((unsigned long long)table_bytes) + " bytes) does not fit the " + std::to_string(free_b) +
                                               " bytes free on the device beside " + std::to_string((unsigned long long)n * 16) + " bytes of staged interactions");
  std::vector<TrendingWeightDev> wdev((size_t)n_weights);
  std::vector<double> pow_table;
  pow_table.reserve((size_t)total_days);
  long long off = 0;
  for (int w = 0; w < n_weights; ++w) {
    const TrendingWeight &cw = cfg.weights[(size_t)w];
    wdev[(size_t)w] = TrendingWeightDev{cw.window_ms, cw.days, off, cw.weight};
    const std::vector<double> p = trending_pow_table(cw.decay, cw.days);
    pow_table.insert(pow_table.end(), p.begin(), p.end());
    off += cw.days;
  }
  DevBuf d_table, d_w, d_pow, d_score, d_order, d_scratch, d_err;
  const size_t table_sz = (size_t)items * (size_t)total_days * 4;
  d_table.reserve(table_sz);
  upload(d_w, wdev, s);
  upload(d_pow, pow_table, s);
  d_score.reserve((size_t)items * 8);
  d_order.reserve((size_t)items * 4);
  d_scratch.reserve(order_scratch);
  d_err.reserve(4);
  if (table_sz) MRK_HIP(hipMemsetAsync(d_table.p, 0, table_sz, s));
  MRK_HIP(hipMemsetAsync(d_err.p, 0, 4, s));
  trending_launch_count(ctx, s, count_mode(), b->d_item.as<uint32_t>(), b->d_widx.as<int32_t>(), b->d_ts.as<long long>(), n, b->st.now_ms,
                        d_w.as<TrendingWeightDev>(), items, d_table.as<uint32_t>(), d_err.as<uint32_t>());
  trending_launch_score(ctx, s, d_table.as<uint32_t>(), d_w.as<TrendingWeightDev>(), n_weights, d_pow.as<double>(), items, d_score.as<double>());
  trending_launch_order(ctx, s, d_score.as<double>(), (int)items, d_order.as<int>(), d_scratch.p);
  std::vector<int32_t> order((size_t)items);
  std::vector<double> score((size_t)items);
  uint32_t err = 0;
  MRK_HIP(hipMemcpyAsync(order.data(), d_order.p, (size_t)items * 4, hipMemcpyDeviceToHost, s));
  MRK_HIP(hipMemcpyAsync(score.data(), d_score.p, (size_t)items * 8, hipMemcpyDeviceToHost, s));
  MRK_HIP(hipMemcpyAsync(&err, d_err.p, 4, hipMemcpyDeviceToHost, s));
  MRK_HIP(hipStreamSynchronize(s));
  drain_profile_events(ctx);
  if (err) {
    const TrendingWeight &cw = cfg.weights[(size_t)err - 1];
    throw StatusError(MRK_ERR_DIM_MISMATCH, "trending: an interaction of weight '" + cw.interaction + "' inside its window of " + std::to_string(cw.window_ms) +
                                                " ms falls into day bucket >= " + std::to_string(cw.days) + " (the window is not a whole number of days: the JVM would throw ArrayIndexOutOfBounds)");
  }
  out.ids.resize((size_t)items);
  out.scores.resize((size_t)items);
  for (size_t i = 0; i < (size_t)items; ++i) {
    const int32_t k = order[i];
    if (k < 0 || k >= items) throw StatusError(MRK_ERR_DEVICE, "trending: the device returned an order outside the items");
    out.ids[i] = b->st.ids[(size_t)k];
    out.scores[i] = score[(size_t)k];
  }
  out.interactions = n;
  out.now_ms = b->st.now_ms;
}

}  // namespace

extern "C" {

// == TrendingConfig's decoder, TrendingRecommender.scala:137-164 + the start of TrendingPredictor.fit
int mrk_trending_begin(mrk_ctx *ctx, const char *config_json, mrk_trending_builder **out) {
  return guard([&] {
    need(out != nullptr, "out is null");
    *out = nullptr;
    need(config_json != nullptr, "null config");
    std::unique_ptr<mrk_trending_builder> b(new mrk_trending_builder());
    b->cfg = trending_parse_config(config_json, strlen(config_json));   // (before the context: a config is judged without a device)
    need(ctx != nullptr, "null context");
    b->ctx = ctx;
    ctx_retain(ctx);
    *out = b.release();
  });
}

// == the flatMap of TrendingPredictor.fit (:40-44): ItemInteraction(ti.item, ti.tpe, ct.ct.ts), appended in stream order
int mrk_trending_add(mrk_trending_builder *b, const char *const *item_ids, const char *const *type_names, int n_types, const int32_t *type_idx,
                     const int64_t *ts_ms, int64_t n) {
  return guard([&] {
    need(b != nullptr, "null builder");
    std::lock_guard<std::mutex> bl(b->mu);
    need(!b->broken, "trending: an earlier add failed on the device; start a new builder");
    const std::vector<int32_t> weight_of = trending_check_call(b->cfg, b->st, item_ids, type_names, n_types, type_idx, ts_ms, n);
    if (n == 0) return;
    mrk_ctx *ctx = b->ctx;
    DeviceLock lk(ctx);
    grow(b, b->st.interactions + n);
    b->pin.reserve((size_t)std::min(n, PIECE) * 16);
    b->broken = true;   // until the call has gone through
    for (int64_t i0 = 0; i0 < n; i0 += PIECE) {
      const int64_t m = std::min(PIECE, n - i0);
      long long *p_ts = b->pin.as<long long>();               // [ts i64 x m][item u32 x m][weight i32 x m]
      uint32_t *p_item = (uint32_t *)(p_ts + m);
      int32_t *p_w = (int32_t *)(p_item + m);
      const int64_t at = b->st.interactions;
      for (int64_t i = 0; i < m; ++i) {
        p_item[i] = b->st.intern(item_ids[i0 + i]);
        p_w[i] = weight_of[(size_t)type_idx[i0 + i]];
        p_ts[i] = ts_ms[i0 + i];
        b->st.saw(ts_ms[i0 + i]);
      }
      MRK_HIP(hipMemcpyAsync(b->d_ts.as<long long>() + at, p_ts, (size_t)m * 8, hipMemcpyHostToDevice, ctx->stream));
      MRK_HIP(hipMemcpyAsync(b->d_item.as<uint32_t>() + at, p_item, (size_t)m * 4, hipMemcpyHostToDevice, ctx->stream));
      MRK_HIP(hipMemcpyAsync(b->d_widx.as<int32_t>() + at, p_w, (size_t)m * 4, hipMemcpyHostToDevice, ctx->stream));
      MRK_HIP(hipStreamSynchronize(ctx->stream));   // the pinned piece is reused
    }
    b->broken = false;
  });
}

// == the rest of TrendingPredictor.fit (:45-86)
int mrk_trending_fit(mrk_trending_builder *b, mrk_trending **out) {
  return guard([&] {
    need(out != nullptr, "out is null");
    *out = nullptr;
    need(b != nullptr, "null builder");
    std::lock_guard<std::mutex> bl(b->mu);
    need(!b->broken, "trending: an earlier add failed on the device; start a new builder");
    if (b->st.interactions == 0) throw StatusError(MRK_ERR_NOT_FOUND, "no interactions found");
    std::unique_ptr<mrk_trending> t(new mrk_trending());
    fit_locked(b, t->m);
    *out = t.release();
  });
}

void mrk_trending_builder_free(mrk_trending_builder *b) {
  if (!b) return;
  mrk_ctx *ctx = b->ctx;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    delete b;
  }
  ctx_release(ctx);
}

// == TrendingPredictor.loadSync, :90-110
int mrk_trending_load(mrk_ctx *ctx, const uint8_t *bytes, size_t len, mrk_trending **out) {
  (void)ctx;   // a model is a host object: no device, and no context, is needed
  return guard([&] {
    need(out != nullptr, "out is null");
    *out = nullptr;
    need(bytes != nullptr || len == 0, "null bytes");
    std::unique_ptr<mrk_trending> t(new mrk_trending());
    t->m = trending_load(bytes, len);
    *out = t.release();
  });
}

// == TrendingModel.save, :123-133
int mrk_trending_save(mrk_trending *t, uint8_t *out, size_t cap, size_t *needed) {
  return guard([&] {
    need(t != nullptr, "null trending model");
    const std::vector<uint8_t> bytes = trending_save(t->m);
    if (needed) *needed = bytes.size();
    need(out != nullptr && cap >= bytes.size(), "trending: output buffer too small (see *needed)");
    memcpy(out, bytes.data(), bytes.size());
  });
}

int mrk_trending_info(mrk_trending *t, int64_t *items, int64_t *interactions, int64_t *now_ms) {
  return guard([&] {
    need(t != nullptr, "null trending model");
    if (items) *items = (int64_t)t->m.ids.size();
    if (interactions) *interactions = t->m.interactions;
    if (now_ms) *now_ms = t->m.now_ms;
  });
}

const char *mrk_trending_id(mrk_trending *t, int64_t rank) {
  if (!t || rank < 0 || rank >= (int64_t)t->m.ids.size()) return nullptr;
  return t->m.ids[(size_t)rank].c_str();
}

// == TrendingModel.predict, :116-121
int mrk_trending_predict(mrk_trending *t, int count, double *out_scores, int32_t *out_n) {
  return guard([&] {
    need(out_n != nullptr, "out_n is null");
    *out_n = 0;
    need(t != nullptr, "null trending model");
    const int n = trending_predict_n(t->m, count);
    need(out_scores != nullptr, "null output");
    memcpy(out_scores, t->m.scores.data(), (size_t)n * 8);
    *out_n = n;
  });
}

void mrk_trending_free(mrk_trending *t) { delete t; }

}  // extern "C"
