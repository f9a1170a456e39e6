// C ABI (include/mrk.h) of the similar-items index: POST /recommend's KnnIndexWriter.write / KnnIndexReader.lookup
// (ml/recommend/embedding/HnswJavaIndex.scala) and EmbeddingSimilarityModel.predict (ml/recommend/MFRecommender.scala:66-80).
// The table scan and the selection are knn.hip; the request logic is index_host.cpp.
#include <algorithm>
#include <cstring>
#include <memory>
#include <numeric>
#include <thread>
#include <tuple>

#include "encoder.hpp"
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

// ---- mrk_index_build_texts

// Tokens of one forward pass when the caller passes max_tokens = 0.  From the sweep of tools/semantic_fit_bench.py over {8 192,
// 32 768, 65 536, 131 072} on one MI355X (LOG.md round 13: 150.9 k / 179.4 k / 182.3 k / 186.2 k items/s, run-to-run spread
// 0.5 % at the most): every step still gains more than the spread, so the largest budget measured.  At 131 072 the activations of
// a MiniLM-L6-shaped encoder (H = 384, I = 1 536, f32: H * 10 + 4 * H * 4 + I * 4 = 16 128 B per token) are 2.11 GB.
constexpr int64_t SEMANTIC_DEFAULT_MAX_TOKENS = 131072;
constexpr int64_t SEMANTIC_MAX_TOKENS_CAP = int64_t(1) << 24;   // a larger budget is taken as this one (token offsets are int32 on the device)

struct HipEvent {
  hipEvent_t ev = nullptr;
  explicit HipEvent(unsigned flags = hipEventDisableTiming) { MRK_HIP(hipEventCreateWithFlags(&ev, flags)); }
  HipEvent(const HipEvent &) = delete;
  HipEvent &operator=(const HipEvent &) = delete;
  ~HipEvent() { if (ev) (void)hipEventDestroy(ev); }
};

// Token ids of texts [from, from + m) appended to `out` (Tokenizer::encode: one sequence, truncated, with specials, no padding);
// a window of many texts is shared among the library's host threads (MRK_HOST_THREADS, at most 16).
void tokenize_texts(const Tokenizer &tok, const char *const *texts, int64_t from, int64_t m, std::vector<std::vector<int32_t>> &out) {
  const size_t base = out.size();
  out.resize(base + (size_t)m);
  auto run = [&](int64_t lo, int64_t hi) {
    for (int64_t i = lo; i < hi; ++i) out[base + (size_t)i] = std::move(tok.encode(texts[from + i], nullptr).ids);
  };
  int workers = switches().host_threads > 0 ? switches().host_threads : (int)std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
  workers = (int)std::min<int64_t>(std::min(workers, 16), m / 256);
  if (workers <= 1) return run(0, m);
  std::vector<std::thread> pool;
  std::vector<std::exception_ptr> failed((size_t)workers);
  const int64_t per = (m + workers - 1) / workers;
  for (int w = 0; w < workers; ++w)
    pool.emplace_back([&, w] {
      try {
        run(std::min(m, w * per), std::min(m, (w + 1) * per));
      } catch (...) {
        failed[(size_t)w] = std::current_exception();
      }
    });
  for (auto &t : pool) t.join();
  for (auto &f : failed)
    if (f) std::rethrow_exception(f);
}

// The fit proper.  `ix` has its ids; on return its table holds every row and its norms.  Streams: the forward passes and the
// pool-and-pack launches go to the encoder's stream under enc->mu, one piece at a time; the table's allocation, zero fill and
// norms go to the context's stream under ctx->mu; two events order the streams (table ready -> first pack, last pack -> norms).
void fit_texts(mrk_ctx *ctx, mrk_encoder *enc, mrk_index *ix, const char *const *texts, int64_t rows, int64_t max_tokens) {
  const EncoderShape &sh = enc->dev.shape;
  KnnTable &t = ix->table;
  MRK_HIP(hipSetDevice(ctx->device));
  HipEvent table_ready, packs_done;
  const bool profile = ctx->profile;
  {
    DeviceLock lk(ctx);   // (selects the device a second time: the events above are made before the lock is taken)
    knn_table_alloc(t, rows, sh.hidden, 4, ctx->stream);
    MRK_HIP(hipEventRecord(table_ready.ev, ctx->stream));
  }
  // (declared outside the try block below: on an error they must outlive the wait for the encoder's stream)
  PinBuf pin[2];
  HipEvent free_ev[2];
  std::vector<std::tuple<const char *, hipEvent_t, hipEvent_t>> timed;   // (timer, begin, end) of every piece, when profiling
  auto finish = [&](bool ok) {
    // nothing of this call is left on the encoder's stream when it returns: the pinned buffers and a partial table die with it
    const hipError_t rc = hipStreamSynchronize(enc->stream);
    std::lock_guard<std::mutex> lk(ctx->mu);
    for (auto &e : timed) {
      float ms = 0.f;
      if (ok && rc == hipSuccess && hipEventElapsedTime(&ms, std::get<1>(e), std::get<2>(e)) == hipSuccess) {
        auto &tm = ctx->timers[std::get<0>(e)];
        tm.total_ms += ms;
        tm.launches += 1;
      }
    }
    for (auto &e : timed)
      if (std::get<0>(e)[0] == 'e') { (void)hipEventDestroy(std::get<1>(e)); (void)hipEventDestroy(std::get<2>(e)); }
      else (void)hipEventDestroy(std::get<2>(e));   // (a piece's "encoder" end is its "knn_pool_pack" begin)
    timed.clear();
    if (ok) MRK_HIP(rc);
  };
  try {
    // Two pinned id buffers in run_encoder's packed layout, [ids | type_ids | position ids] x M then cu x (n + 1), then - 8-byte
    // aligned - the sequences' destination rows: the host tokenises and fills one while the device works through the other.
    // free_ev[b] says that buffer b's words have left the host.
    bool used[2] = {false, false};
    int next_buf = 0;
    const int window = switches().semantic_window;
    const int64_t window_tokens = max_tokens * std::max(window, 1);
    std::vector<std::vector<int32_t>> pending;   // tokenised, not yet sent: input rows [sent, sent + pending.size())
    std::vector<int32_t> lens;
    std::vector<int64_t> order, starts;
    int64_t sent = 0, taken = 0, pending_tokens = 0;
    bool first_piece = true, reserved = false;
    size_t M_res = 0, words_res = 0;
    auto id_words = [](size_t M, size_t n) { return (3 * M + n + 1 + 1) / 2 * 2 + 2 * n; };

    auto send_piece = [&](const int64_t *seq, int64_t n) {   // seq: positions in `pending` (input row = sent + position)
      size_t M = 0;
      int max_len = 0;
      for (int64_t k = 0; k < n; ++k) {
        M += pending[(size_t)seq[k]].size();
        max_len = std::max(max_len, (int)pending[(size_t)seq[k]].size());
      }
      if (max_len > sh.max_pos)
        throw StatusError(MRK_ERR_INVALID_ARG, "encoder: sequence length " + std::to_string(max_len) + " exceeds the model's " + std::to_string(sh.max_pos) + " positions");
      const size_t words = id_words(M, (size_t)n);
      const int b = next_buf;
      next_buf ^= 1;
      if (used[b]) MRK_HIP(hipEventSynchronize(free_ev[b].ev));
      pin[b].reserve(std::max(words, words_res) * 4);
      int32_t *h = pin[b].as<int32_t>(), *cu = h + 3 * M;
      const size_t dst_at = (3 * M + (size_t)n + 1 + 1) / 2 * 2;
      int64_t *dst = (int64_t *)(h + dst_at);
      size_t at = 0;
      for (int64_t k = 0; k < n; ++k) {
        const std::vector<int32_t> &ids = pending[(size_t)seq[k]];
        cu[k] = (int32_t)at;
        memcpy(h + at, ids.data(), ids.size() * 4);
        memset(h + M + at, 0, ids.size() * 4);   // one sequence: every token is of type 0
        std::iota(h + 2 * M + at, h + 2 * M + at + ids.size(), 0);
        dst[k] = sent + seq[k];
        at += ids.size();
      }
      cu[n] = (int32_t)at;
      if (dst_at > 3 * M + (size_t)n + 1) h[dst_at - 1] = 0;
      EncoderMarks marks;
      marks.uploaded = free_ev[b].ev;
      if (profile) {
        MRK_HIP(hipEventCreate(&marks.begin));
        if (hipEventCreate(&marks.end) != hipSuccess) { (void)hipEventDestroy(marks.begin); throw StatusError(MRK_ERR_DEVICE, "hipEventCreate failed"); }
        if (hipEventCreate(&marks.packed) != hipSuccess) { (void)hipEventDestroy(marks.begin); (void)hipEventDestroy(marks.end); throw StatusError(MRK_ERR_DEVICE, "hipEventCreate failed"); }
        timed.emplace_back("encoder", marks.begin, marks.end);
        timed.emplace_back("knn_pool_pack", marks.end, marks.packed);
      }
      std::lock_guard<std::mutex> lk(enc->mu);   // per piece: a query embedding from the same handle waits for one piece
      enc->dev.f32 = encoder_calls_in_f32(*enc) && !enc->dev.layers32.empty();
      encoder_reserve_call(*enc, std::max(M, M_res), std::max(words, words_res));
      if (first_piece) MRK_HIP(hipStreamWaitEvent(enc->stream, table_ready.ev, 0));
      first_piece = false;
      EncoderDest to;
      to.table = &t;
      to.d_dst_row = (const int64_t *)(enc->scratch.ids.as<int32_t>() + dst_at);
      used[b] = true;
      encoder_enqueue(*enc, h, words, (int)n, max_len, (int)M, MODE_POOL, to, marks);
    };

    while (sent < rows) {
      // tokenise until the pending sequences certainly hold a whole piece more than the window (or the catalogue ends)
      // (two sequences at least: one that is longer than the budget is a piece of its own and says nothing about the next)
      while (taken < rows && (pending.size() < 2 || (pending_tokens <= window_tokens && (int64_t)pending.size() <= (int64_t)KNN_PIECE_MAX_ROWS * std::max(window, 1)))) {
        const int64_t m = std::min<int64_t>(rows - taken, std::max<int64_t>(64, std::min<int64_t>(4096, (window_tokens - pending_tokens) / 16)));
        const size_t base = pending.size();
        tokenize_texts(enc->tok, texts, taken, m, pending);
        for (size_t i = base; i < pending.size(); ++i) pending_tokens += (int64_t)pending[i].size();
        taken += m;
      }
      const bool last = taken == rows;
      if (!reserved) {
        // the scratch is sized ONCE, before the first piece: for min(max_tokens, total tokens) - the total is known when the
        // whole catalogue fits the first window - or for the longest sequence there can be where that is longer
        size_t longest = (size_t)std::min(enc->tok.max_length(), sh.max_pos);
        if (last) {
          longest = 1;
          for (auto &ids : pending) longest = std::max(longest, ids.size());
        }
        M_res = std::max<size_t>((size_t)std::min<int64_t>(max_tokens, last ? pending_tokens : max_tokens), longest);
        words_res = id_words(M_res, std::min<size_t>(M_res, (size_t)KNN_PIECE_MAX_ROWS));
        reserved = true;
      }
      const int64_t np = (int64_t)pending.size();
      order.resize((size_t)np);
      std::iota(order.begin(), order.end(), 0);
      // length order inside the window: a piece's attention grid is sized by its longest sequence.  (Not for a catalogue that is
      // one piece anyway: there the order changes nothing, and the launches stay those of one mrk_encoder_embed call.)
      if (window > 0 && !(last && sent == 0 && pending_tokens <= max_tokens && np <= KNN_PIECE_MAX_ROWS))
        std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return pending[(size_t)a].size() < pending[(size_t)b].size(); });
      lens.resize((size_t)np);
      for (int64_t k = 0; k < np; ++k) lens[(size_t)k] = (int32_t)pending[(size_t)order[(size_t)k]].size();
      knn_plan_pieces(lens.data(), np, max_tokens, KNN_PIECE_MAX_ROWS, starts);
      // In input order the last planned piece may still grow with texts not tokenised yet: it waits for the next round, so the
      // pieces are those of one knn_plan_pieces over the whole catalogue.  A length-ordered window is sent whole.
      const size_t n_send = last || window > 0 ? starts.size() - 1 : starts.size() - 2;
      if (n_send == 0) throw StatusError(MRK_ERR_DEVICE, "index: the piece planner made no progress");   // (cannot happen: see the loop above)
      for (size_t k = 0; k < n_send; ++k) send_piece(order.data() + starts[k], starts[k + 1] - starts[k]);
      const int64_t done = starts[n_send];
      for (int64_t k = 0; k < done; ++k) pending_tokens -= (int64_t)pending[(size_t)k].size();
      pending.erase(pending.begin(), pending.begin() + done);
      sent += done;
    }
    if (!first_piece) MRK_HIP(hipEventRecord(packs_done.ev, enc->stream));
    finish(true);
  } catch (...) {
    finish(false);
    throw;
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rows > 0) MRK_HIP(hipStreamWaitEvent(ctx->stream, packs_done.ev, 0));
  {
    ScopedKernelTimer timer(ctx, "knn_norms");
    knn_norms(t, ctx->stream);
  }
  MRK_HIP(hipStreamSynchronize(ctx->stream));
  drain_profile_events(ctx);
}

}  // namespace

namespace mrk {

mrk_index *index_from_device_f64(mrk_ctx *ctx, const char *const *ids, const double *d_values, int64_t rows, int cols) {
  need_ok(knn_check_shape(rows, cols));
  std::unique_ptr<mrk_index> ix(new mrk_index());
  need_ok(ix->ids.build(ids, rows));
  MRK_HIP(hipSetDevice(ctx->device));
  KnnTable &t = ix->table;
  knn_table_alloc(t, rows, cols, 8, ctx->stream);
  knn_pack(t, d_values, 8, 0, rows, ctx->stream);
  knn_norms(t, ctx->stream);
  MRK_HIP(hipStreamSynchronize(ctx->stream));
  ix->ctx = ctx;
  ctx_retain(ctx);
  return ix.release();
}

}  // namespace mrk

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
    DeviceLock lk(ctx);
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

// == BertSemanticPredictor.fit (embed every item's text) + KnnIndexWriter.write, ml/recommend/BertSemanticRecommender.scala:25-79
int mrk_index_build_texts(mrk_ctx *ctx, mrk_encoder *enc, const char *const *ids, const char *const *texts, int64_t rows, int64_t max_tokens,
                          mrk_index **out) {
  return guard([&] {
    need(out != nullptr, "out is null");
    *out = nullptr;
    need(ctx != nullptr, "null context");
    need(enc != nullptr, "null encoder");
    need(enc->ctx == ctx, "index: the encoder belongs to another context");
    need(max_tokens >= 0, "index: max_tokens is negative");
    need_ok(knn_check_shape(rows, enc->dev.shape.hidden));
    need(rows == 0 || (ids && texts), "null ids / texts");
    for (int64_t r = 0; r < rows; ++r)
      if (!texts[r]) throw StatusError(MRK_ERR_INVALID_ARG, "index: text of row " + std::to_string(r) + " is null");
    std::unique_ptr<mrk_index> ix(new mrk_index());
    need_ok(ix->ids.build(ids, rows));
    encoder_retain(enc);   // (a concurrent mrk_encoder_free must not take the handle away under the fit)
    try {
      fit_texts(ctx, enc, ix.get(), texts, rows, max_tokens == 0 ? SEMANTIC_DEFAULT_MAX_TOKENS : std::min(max_tokens, SEMANTIC_MAX_TOKENS_CAP));
    } catch (...) {
      {
        std::lock_guard<std::mutex> lk(ctx->mu);
        (void)hipStreamSynchronize(ctx->stream);
        ix.reset();   // the partial table
      }
      encoder_release(enc);
      throw;
    }
    encoder_release(enc);
    ix->ctx = ctx;
    ctx_retain(ctx);
    *out = ix.release();
  });
}

// == index.get(id).vector (HnswJavaIndex.scala:29-31) for n rows
int mrk_index_vectors(mrk_index *ix, const int64_t *rows, int n, double *out) {
  return guard([&] {
    check_index(ix);
    need(n >= 0, "index: negative row count");
    need(n == 0 || (rows && out), "null rows / out");
    const KnnTable &t = ix->table;
    for (int i = 0; i < n; ++i)
      if (rows[i] < 0 || rows[i] >= t.rows)
        throw StatusError(MRK_ERR_INVALID_ARG, "index: row " + std::to_string(rows[i]) + " is outside 0 <= row < " + std::to_string(t.rows));
    if (n == 0) return;
    mrk_ctx *ctx = ix->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    MRK_HIP(hipSetDevice(ctx->device));
    const int chunk = (int)std::max<int64_t>(1, (int64_t(32) << 20) / ((int64_t)t.cols * 8));   // about 32 MiB of doubles at a time
    for (int r0 = 0; r0 < n; r0 += chunk) {
      const int m = std::min(chunk, n - r0);
      ix->d_fetch_rows.reserve((size_t)m * 8);
      ix->d_fetch.reserve((size_t)m * t.cols * 8);
      MRK_HIP(hipMemcpyAsync(ix->d_fetch_rows.p, rows + r0, (size_t)m * 8, hipMemcpyHostToDevice, ctx->stream));
      knn_fetch_rows(t, ix->d_fetch_rows.as<int64_t>(), m, ix->d_fetch.as<double>(), ctx->stream);
      MRK_HIP(hipMemcpyAsync(out + (size_t)r0 * t.cols, ix->d_fetch.p, (size_t)m * t.cols * 8, hipMemcpyDeviceToHost, ctx->stream));
      MRK_HIP(hipStreamSynchronize(ctx->stream));
    }
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
