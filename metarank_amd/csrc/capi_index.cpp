// C ABI (include/mrk.h) of the similar-items index: POST /recommend's KnnIndexWriter.write / KnnIndexReader.lookup
// (ml/recommend/embedding/HnswJavaIndex.scala) and EmbeddingSimilarityModel.predict (ml/recommend/MFRecommender.scala:66-80).
// The table scan and the selection are knn.hip; the request logic is index_host.cpp.
#include <algorithm>
#include <cstring>
#include <memory>

#include "index_host.hpp"
#include "knn.hpp"
#include "runtime.hpp"

using namespace mrk;

struct mrk_index {
  mrk_ctx *ctx = nullptr;
  KnnTable table;
  KnnIds ids;
  // scratch of a search (under ctx->mu), grow-only
  KnnScratch scratch;
  DevBuf d_q, d_out_rows, d_out_dist, d_fetch_rows, d_fetch;
};

namespace {

template <typename F>
int guard(F &&f) {
  try {
    f();
    return MRK_OK;
  } catch (const StatusError &e) {
    set_last_error(e.what());
    return e.status;
  } catch (const std::bad_alloc &) {
    set_last_error("out of host memory");
    return MRK_ERR_DEVICE;
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return MRK_ERR_PARSE;
  }
}

void need(bool ok, const char *what) {
  if (!ok) throw StatusError(MRK_ERR_INVALID_ARG, what);
}
void need_ok(const std::string &err) {
  if (!err.empty()) throw StatusError(MRK_ERR_INVALID_ARG, err);
}

// the min(n, rows) nearest rows of each query into out_rows / out_dist (n_queries x n, the first out_n[q] of a row filled);
// caller holds ctx->mu.  More queries than one launch takes: chunks.
void search_locked(mrk_index *ix, const double *queries, int nq, int n, int32_t *out_rows, double *out_dist, int32_t *out_n) {
  mrk_ctx *ctx = ix->ctx;
  const KnnTable &t = ix->table;
  const int k = (int)std::min<int64_t>(n, t.rows);
  for (int q = 0; q < nq; ++q) out_n[q] = k;
  if (k == 0 || nq == 0) return;
  MRK_HIP(hipSetDevice(ctx->device));
  const int chunk = knn_query_chunk(t.rows);
  std::vector<int32_t> h_rows((size_t)std::min(nq, chunk) * k);
  std::vector<double> h_dist(h_rows.size());
  for (int q0 = 0; q0 < nq; q0 += chunk) {
    const int m = std::min(chunk, nq - q0);
    ix->d_q.reserve((size_t)m * t.cols * 8);
    ix->d_out_rows.reserve((size_t)m * k * 4);
    ix->d_out_dist.reserve((size_t)m * k * 8);
    MRK_HIP(hipMemcpyAsync(ix->d_q.p, queries + (size_t)q0 * t.cols, (size_t)m * t.cols * 8, hipMemcpyHostToDevice, ctx->stream));
    knn_search(ctx, t, ix->scratch, ix->d_q.as<double>(), m, k, ix->d_out_rows.as<int32_t>(), ix->d_out_dist.as<double>());
    MRK_HIP(hipMemcpyAsync(h_rows.data(), ix->d_out_rows.p, (size_t)m * k * 4, hipMemcpyDeviceToHost, ctx->stream));
    MRK_HIP(hipMemcpyAsync(h_dist.data(), ix->d_out_dist.p, (size_t)m * k * 8, hipMemcpyDeviceToHost, ctx->stream));
    MRK_HIP(hipStreamSynchronize(ctx->stream));
    drain_profile_events(ctx);
    for (int q = 0; q < m; ++q) {
      memcpy(out_rows + (size_t)(q0 + q) * n, h_rows.data() + (size_t)q * k, (size_t)k * 4);
      memcpy(out_dist + (size_t)(q0 + q) * n, h_dist.data() + (size_t)q * k, (size_t)k * 8);
    }
  }
}

// HnswIndexReader.lookup: the query is the stored vector of the one known item, or the centroid of the known ones; the few
// rows it needs are fetched from the device (the table has no host mirror).  Returns how many results were written.
int lookup_locked(mrk_index *ix, const char *const *item_ids, int n_items, int n, int32_t *out_rows, double *out_dist) {
  const std::vector<int64_t> rows = knn_known_rows(ix->ids, item_ids, n_items);
  if (rows.empty() || n == 0) return 0;   // (several ids, none known: the reference would search for a NaN centroid)
  mrk_ctx *ctx = ix->ctx;
  const KnnTable &t = ix->table;
  MRK_HIP(hipSetDevice(ctx->device));
  const int m = (int)rows.size();
  ix->d_fetch_rows.reserve((size_t)m * 8);
  ix->d_fetch.reserve((size_t)m * t.cols * 8);
  std::vector<double> vectors((size_t)m * t.cols), query((size_t)t.cols);
  MRK_HIP(hipMemcpyAsync(ix->d_fetch_rows.p, rows.data(), (size_t)m * 8, hipMemcpyHostToDevice, ctx->stream));
  knn_fetch_rows(t, ix->d_fetch_rows.as<int64_t>(), m, ix->d_fetch.as<double>(), ctx->stream);
  MRK_HIP(hipMemcpyAsync(vectors.data(), ix->d_fetch.p, vectors.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  MRK_HIP(hipStreamSynchronize(ctx->stream));
  if (n_items == 1) query = vectors;
  else knn_centroid(vectors.data(), m, t.cols, query.data());
  int32_t found = 0;
  search_locked(ix, query.data(), 1, n, out_rows, out_dist, &found);
  return found;
}

void check_index(mrk_index *ix) {
  need(ix != nullptr, "null index");
  need(ix->ctx != nullptr, "index is closed");
}

}  // namespace

extern "C" {

// == KnnIndexWriter.write(EmbeddingMap), HnswJavaIndex.scala:68-87
int mrk_index_build(mrk_ctx *ctx, const char *const *ids, const void *values, int elem_bytes, int64_t rows, int cols, mrk_index **out) {
  return guard([&] {
    need(out != nullptr, "out is null");
    *out = nullptr;
    need(ctx != nullptr, "null context");
    need(elem_bytes == 4 || elem_bytes == 8, "index: elem_bytes must be 4 (float) or 8 (double)");
    need_ok(knn_check_shape(rows, cols));
    need(rows == 0 || (ids && values), "null ids / values");
    std::unique_ptr<mrk_index> ix(new mrk_index());
    need_ok(ix->ids.build(ids, rows));
    const int stored = elem_bytes == 4 || knn_f32_lossless((const double *)values, (size_t)rows * cols) ? 4 : 8;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->closed) throw StatusError(MRK_ERR_INVALID_ARG, "context is shut down");
    MRK_HIP(hipSetDevice(ctx->device));
    KnnTable &t = ix->table;
    knn_table_alloc(t, rows, cols, stored, ctx->stream);
    // the caller's rows go up in pieces of about 64 MiB and are cut into the table's blocks on the device
    const int64_t piece = std::max<int64_t>(64, (int64_t(64) << 20) / ((int64_t)cols * elem_bytes) / 64 * 64);
    DevBuf staging;
    for (int64_t r0 = 0; r0 < rows; r0 += piece) {
      const int64_t m = std::min(piece, rows - r0);
      const size_t bytes = (size_t)m * cols * elem_bytes;
      staging.reserve(bytes);
      MRK_HIP(hipMemcpyAsync(staging.p, (const char *)values + (size_t)r0 * cols * elem_bytes, bytes, hipMemcpyHostToDevice, ctx->stream));
      knn_pack(t, staging.p, elem_bytes, r0, m, ctx->stream);
      MRK_HIP(hipStreamSynchronize(ctx->stream));
    }
    knn_norms(t, ctx->stream);
    MRK_HIP(hipStreamSynchronize(ctx->stream));
    ix->ctx = ctx;
    ctx_retain(ctx);
    *out = ix.release();
  });
}

int mrk_index_info(mrk_index *ix, int64_t *rows, int *cols, int *stored_elem_bytes, int64_t *device_bytes) {
  return guard([&] {
    check_index(ix);
    if (rows) *rows = ix->table.rows;
    if (cols) *cols = ix->table.cols;
    if (stored_elem_bytes) *stored_elem_bytes = ix->table.elem_bytes;
    if (device_bytes) *device_bytes = (int64_t)(ix->table.vals_bytes() + (size_t)ix->table.n_blocks * 64 * sizeof(double));
  });
}

const char *mrk_index_id(mrk_index *ix, int64_t row) {
  if (!ix || row < 0 || row >= (int64_t)ix->ids.ids.size()) return nullptr;
  return ix->ids.ids[(size_t)row].c_str();
}

int64_t mrk_index_row(mrk_index *ix, const char *id) { return ix ? ix->ids.row(id) : -1; }

// == HnswIndexReader.lookupOne (index.findNearest(vector, n)), HnswJavaIndex.scala:56-59, for a batch of vectors
int mrk_index_search(mrk_index *ix, const double *queries, int n_queries, int n, int32_t *out_rows, double *out_dist, int32_t *out_n) {
  return guard([&] {
    check_index(ix);
    need(n_queries >= 0, "index: negative query count");
    need_ok(knn_check_n(n, 0));
    need(n_queries == 0 || (queries && out_n), "null queries / out_n");
    need(n_queries == 0 || n == 0 || (out_rows && out_dist), "null output");
    std::lock_guard<std::mutex> lk(ix->ctx->mu);
    search_locked(ix, queries, n_queries, n, out_rows, out_dist, out_n);
  });
}

// == HnswIndexReader.lookup(items, n), HnswJavaIndex.scala:25-38
int mrk_index_lookup(mrk_index *ix, const char *const *item_ids, int n_items, int n, int32_t *out_rows, double *out_dist, int32_t *out_n) {
  return guard([&] {
    check_index(ix);
    need(out_n != nullptr, "out_n is null");
    *out_n = 0;
    need_ok(knn_check_n(n, n_items));
    need(n_items == 0 || item_ids, "null item ids");
    need(n == 0 || (out_rows && out_dist), "null output");
    std::lock_guard<std::mutex> lk(ix->ctx->mu);
    *out_n = lookup_locked(ix, item_ids, n_items, n, out_rows, out_dist);
  });
}

// == EmbeddingSimilarityModel.predict (MFRecommender.scala:66-77) + the ordering of Recommender.recommend (Recommender.scala:42)
int mrk_index_recommend(mrk_index *ix, const char *const *item_ids, int n_items, int count, int32_t *out_rows, double *out_score, int32_t *out_n) {
  return guard([&] {
    check_index(ix);
    need(out_n != nullptr, "out_n is null");
    *out_n = 0;
    need(n_items > 0 && item_ids, "similar items recommender requires request.items to be non-empty");
    need_ok(knn_check_n(count, n_items));
    need(count == 0 || (out_rows && out_score), "null output");
    const int n = count + n_items;
    std::vector<int32_t> rows((size_t)n);
    std::vector<double> score((size_t)n);
    int found;
    {
      std::lock_guard<std::mutex> lk(ix->ctx->mu);
      found = lookup_locked(ix, item_ids, n_items, n, rows.data(), score.data());
    }
    const int left = knn_recommend_order(rows.data(), score.data(), found, knn_known_rows(ix->ids, item_ids, n_items), count);
    if (left == 0) throw StatusError(MRK_ERR_NOT_FOUND, "empty response from the recommender");
    memcpy(out_rows, rows.data(), (size_t)left * 4);
    memcpy(out_score, score.data(), (size_t)left * 8);
    *out_n = left;
  });
}

void mrk_index_free(mrk_index *ix) {
  if (!ix) return;
  mrk_ctx *ctx = ix->ctx;
  if (!ctx) {
    delete ix;
    return;
  }
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    delete ix;
  }
  ctx_release(ctx);
}

}  // extern "C"
