// C ABI (include/mrk.h) of the similar-items fit: POST /recommend's MFPredictor.fit with ALSRecImpl.train
// (ml/recommend/MFRecommender.scala:26-63, ml/recommend/mf/ALSRecImpl.scala:18-81).  The iterations are als.hip; config, interning,
// CSR / CSC, confidences and the generator are als_host.cpp; the result is an ordinary mrk_index (capi_index.cpp).
#include <chrono>
#include <cstring>
#include <memory>

#include "als.hpp"
#include "als_host.hpp"
#include "index_host.hpp"
#include "knn.hpp"
#include "runtime.hpp"

using namespace mrk;

struct mrk_als_builder {
  mrk_ctx *ctx = nullptr;   // null: a host-only builder (mrk_als_begin_host)
  AlsConfig cfg;
  AlsStream st;
  std::mutex mu;            // one add / fit at a time; lock order: mu before ctx->mu
};

namespace {

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

mrk_index *fit_locked(mrk_als_builder *b, uint64_t seed, const double *init_users, const double *init_items, double *out_user_factors) {
  mrk_ctx *ctx = b->ctx;
  const int K = b->cfg.factors;
  auto t0 = std::chrono::steady_clock::now();
  const AlsProblem pr = als_build_problem(b->st);
  const double problem_ms = ms_since(t0);
  if (pr.items > KNN_MAX_ROWS)
    throw StatusError(MRK_ERR_UNSUPPORTED, "als: " + std::to_string(pr.items) + " items are more than an index's " + std::to_string(KNN_MAX_ROWS) + " rows");
  t0 = std::chrono::steady_clock::now();
  std::vector<double> P((size_t)pr.users * K), Q((size_t)pr.items * K);
  if (init_users) {
    memcpy(P.data(), init_users, P.size() * 8);
    memcpy(Q.data(), init_items, Q.size() * 8);
  } else {
    als_init_matrix(seed, 0, pr.users, K, P.data());
    als_init_matrix(seed, 1, pr.items, K, Q.data());
  }
  const double init_ms = ms_since(t0);
  std::vector<double> entry_wc((size_t)pr.nnz);   // w - c_i per entry of R_u, w = 1
  for (size_t k = 0; k < entry_wc.size(); ++k) entry_wc[k] = 1.0 - pr.conf[(size_t)pr.u_idx[k]];
  std::vector<const char *> ids((size_t)pr.items);
  for (size_t i = 0; i < ids.size(); ++i) ids[i] = b->st.items[i].c_str();

  DeviceLock lk(ctx);
  hipStream_t s = lk.stream;
  // limit: everything of a fit is resident at once (no chunked fit): both factor matrices, the entries twice (R_u, R_i), r and
  // w - c per entry, the chunk partials of the larger product, and the index table the item factors end in
  const size_t partial_bytes = als_gram_scratch_bytes(std::max(pr.users, pr.items), K);
  const double work = 8.0 * K * ((double)pr.users + 2.0 * ((double)pr.items + 64)) + 24.0 * (double)pr.nnz + 16.0 * K * K + (double)partial_bytes +
                      8.0 * ((double)pr.users + (double)pr.items) + 16.0 * ((double)pr.items + 64) + 65536;
  size_t free_b = 0, total_b = 0;
  MRK_HIP(hipMemGetInfo(&free_b, &total_b));
  if (work > (double)free_b)
    throw StatusError(MRK_ERR_UNSUPPORTED, "als: a fit of " + std::to_string(pr.users) + " users x " + std::to_string(pr.items) + " items x " +
                                               std::to_string(K) + " factors over " + std::to_string(pr.nnz) + " distinct pairs needs " +
                                               std::to_string((unsigned long long)work) + " bytes of device memory, " + std::to_string(free_b) + " are free");
  DevBuf d_P, d_Q, d_Sq, d_Sp, d_partial, d_rhat, d_wc, d_conf, d_uoff, d_uidx, d_uord, d_ioff, d_iidx, d_iord;
  upload(d_P, P, s);
  upload(d_Q, Q, s);
  upload(d_wc, entry_wc, s);
  upload(d_conf, pr.conf, s);
  upload(d_uoff, pr.u_off, s);
  upload(d_uidx, pr.u_idx, s);
  upload(d_uord, pr.u_order, s);
  upload(d_ioff, pr.i_off, s);
  upload(d_iidx, pr.i_idx, s);
  upload(d_iord, pr.i_order, s);
  d_Sq.reserve((size_t)K * K * 8);
  d_Sp.reserve((size_t)K * K * 8);
  d_partial.reserve(partial_bytes);
  d_rhat.reserve(std::max<size_t>((size_t)pr.nnz * 8, 16));
  MRK_HIP(hipStreamSynchronize(s));   // the host vectors go out of use
  AlsSide users, items;
  users.d_off = d_uoff.as<int32_t>(), users.d_idx = d_uidx.as<int32_t>(), users.d_order = d_uord.as<int32_t>();
  users.d_entry_wc = d_wc.as<double>(), users.rows = pr.users;
  items.d_off = d_ioff.as<int32_t>(), items.d_idx = d_iidx.as<int32_t>(), items.d_order = d_iord.as<int32_t>();
  items.rows = pr.items;
  for (int it = 0; it < b->cfg.iterations; ++it) {
    als_launch_gram(ctx, s, "als_gram_items", d_Q.as<double>(), d_conf.as<double>(), pr.items, K, d_partial.as<double>(), d_Sq.as<double>());
    als_launch_sweep(ctx, s, false, users, d_P.as<double>(), d_Q.as<double>(), d_Sq.as<double>(), d_conf.as<double>(), b->cfg.lambda_user(), K, d_rhat.as<double>());
    als_launch_gram(ctx, s, "als_gram_users", d_P.as<double>(), nullptr, pr.users, K, d_partial.as<double>(), d_Sp.as<double>());
    als_launch_sweep(ctx, s, true, items, d_Q.as<double>(), d_P.as<double>(), d_Sp.as<double>(), d_conf.as<double>(), b->cfg.lambda_item(), K, d_rhat.as<double>());
  }
  if (out_user_factors) MRK_HIP(hipMemcpyAsync(out_user_factors, d_P.p, P.size() * 8, hipMemcpyDeviceToHost, s));
  mrk_index *ix = nullptr;
  {
    ScopedKernelTimer t(ctx, "als_pack");
    ix = index_from_device_f64(ctx, ids.data(), d_Q.as<double>(), pr.items, K);   // (ends in a synchronise of the stream)
  }
  drain_profile_events(ctx);
  if (ctx->profile) {
    for (auto &e : {std::make_pair("als_host_problem", problem_ms), std::make_pair("als_host_init", init_ms)}) {
      auto &tm = ctx->timers[e.first];
      tm.total_ms += e.second;
      tm.launches += 1;
    }
  }
  return ix;
}

void check_builder(mrk_als_builder *b) { need(b != nullptr, "null builder"); }

// what both begin entries do: clears *out, a builder with the parsed config and no context
std::unique_ptr<mrk_als_builder> begin_host(const char *config_json, mrk_als_builder **out) {
  need(out != nullptr, "out is null");
  *out = nullptr;
  need(config_json != nullptr, "null config");
  std::unique_ptr<mrk_als_builder> b(new mrk_als_builder());
  b->cfg = als_parse_config(config_json, strlen(config_json));
  return b;
}

}  // namespace

extern "C" {

// == ALSConfig's decoder, ALSRecImpl.scala:60-81
int mrk_als_begin(mrk_ctx *ctx, const char *config_json, mrk_als_builder **out) {
  return guard([&] {
    std::unique_ptr<mrk_als_builder> b = begin_host(config_json, out);   // (before the context: a config is judged without a device)
    need(ctx != nullptr, "null context");
    b->ctx = ctx;
    ctx_retain(ctx);
    *out = b.release();
  });
}

int mrk_als_begin_host(const char *config_json, mrk_als_builder **out) {
  return guard([&] {
    std::unique_ptr<mrk_als_builder> b = begin_host(config_json, out);
    *out = b.release();
  });
}

// == the lines of MFPredictor.uirt (MFRecommender.scala:54-59): user, item, rating 1
int mrk_als_add(mrk_als_builder *b, const char *const *user_ids, const char *const *item_ids, int64_t n) {
  return guard([&] {
    check_builder(b);
    std::lock_guard<std::mutex> bl(b->mu);
    b->st.add(user_ids, item_ids, n);
  });
}

// == ALSRecImpl.train (ALSRecImpl.scala:19-41) + KnnIndex.write (MFRecommender.scala:32)
int mrk_als_fit(mrk_als_builder *b, uint64_t seed, const double *init_users, const double *init_items, double *out_user_factors, mrk_index **out) {
  return guard([&] {
    need(out != nullptr, "out is null");
    *out = nullptr;
    check_builder(b);
    need((init_users == nullptr) == (init_items == nullptr), "als: initial factors must be given for both matrices or for neither");
    std::lock_guard<std::mutex> bl(b->mu);
    need(b->ctx != nullptr, "als: a host-only builder cannot fit");
    if (b->st.pairs.empty()) throw StatusError(MRK_ERR_NOT_FOUND, "no interactions found");
    if (b->cfg.factors > ALS_MAX_FACTORS)
      throw StatusError(MRK_ERR_UNSUPPORTED, "als: factors = " + std::to_string(b->cfg.factors) + " is above the limit of " + std::to_string(ALS_MAX_FACTORS));
    *out = fit_locked(b, seed, init_users, init_items, out_user_factors);
  });
}

int mrk_als_info(mrk_als_builder *b, int64_t *users, int64_t *items, int64_t *pairs, int64_t *distinct_pairs) {
  return guard([&] {
    check_builder(b);
    std::lock_guard<std::mutex> bl(b->mu);
    if (users) *users = (int64_t)b->st.users.size();
    if (items) *items = (int64_t)b->st.items.size();
    if (pairs) *pairs = (int64_t)b->st.pairs.size();
    if (distinct_pairs) *distinct_pairs = b->st.distinct_pairs();
  });
}

int mrk_als_config(mrk_als_builder *b, int *iterations, int *factors, double *lambda_user, double *lambda_item) {
  return guard([&] {
    check_builder(b);
    if (iterations) *iterations = b->cfg.iterations;
    if (factors) *factors = b->cfg.factors;
    if (lambda_user) *lambda_user = b->cfg.lambda_user();
    if (lambda_item) *lambda_item = b->cfg.lambda_item();
  });
}

const char *mrk_als_id(mrk_als_builder *b, int matrix, int64_t index) {
  if (!b || (matrix != 0 && matrix != 1)) return nullptr;
  std::lock_guard<std::mutex> bl(b->mu);
  const std::vector<std::string> &ids = matrix == 0 ? b->st.users : b->st.items;
  return index < 0 || index >= (int64_t)ids.size() ? nullptr : ids[(size_t)index].c_str();
}

int mrk_als_problem(mrk_als_builder *b, int32_t *user_offsets, int32_t *user_items, int32_t *item_offsets, int32_t *item_users, double *confidence) {
  return guard([&] {
    check_builder(b);
    std::lock_guard<std::mutex> bl(b->mu);
    if (b->st.pairs.empty()) throw StatusError(MRK_ERR_NOT_FOUND, "no interactions found");
    const AlsProblem pr = als_build_problem(b->st);
    if (user_offsets) memcpy(user_offsets, pr.u_off.data(), pr.u_off.size() * 4);
    if (user_items) memcpy(user_items, pr.u_idx.data(), pr.u_idx.size() * 4);
    if (item_offsets) memcpy(item_offsets, pr.i_off.data(), pr.i_off.size() * 4);
    if (item_users) memcpy(item_users, pr.i_idx.data(), pr.i_idx.size() * 4);
    if (confidence) memcpy(confidence, pr.conf.data(), pr.conf.size() * 8);
  });
}

int mrk_als_init_matrix(uint64_t seed, int matrix, int64_t rows, int cols, double *out) {
  return guard([&] {
    need(matrix == 0 || matrix == 1, "als: matrix is 0 (users) or 1 (items)");
    need(rows >= 0 && cols >= 0, "als: negative shape");
    need(rows == 0 || cols == 0 || out, "null output");
    als_init_matrix(seed, matrix, rows, cols, out);
  });
}

void mrk_als_builder_free(mrk_als_builder *b) {
  if (!b) return;
  mrk_ctx *ctx = b->ctx;
  delete b;   // (a builder holds no device memory between calls)
  if (ctx) ctx_release(ctx);
}

}  // extern "C"
