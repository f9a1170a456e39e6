// C ABI (include/mrk.h) of the ranking evaluation: LambdaMARTModel.eval (ml/rank/LambdaMARTRanker.scala:406-445), the step that
// ends every train (:115-123).  Sorting and the ordered sums are eval.hip; validation, gains, the lg table, binning, piece
// planning and the mean are eval_host.cpp.  Every argument is judged before the device is touched.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "eval.hpp"
#include "eval_host.hpp"
#include "runtime.hpp"

using namespace mrk;

namespace {

// MRK_EVAL_WAVE_MAX / MRK_EVAL_PIECE_ROWS: read per call, never on a launch path of the serving side
long long env_int(const char *name, long long dflt) {
  const char *e = getenv(name);
  if (!e || !*e) return dflt;
  char *end = nullptr;
  const long long v = strtoll(e, &end, 10);
  return end && !*end ? v : dflt;
}

// what both entries judge and prepare on the host before any device work
struct Checked {
  EvalShape sh;
  std::vector<double> gains;
  std::vector<uint8_t> rel;
  bool need_ideal = false;
};

Checked check_common(const int *metrics, const int *cutoffs, int n_metrics, int flags, const double *labels, const int64_t *group_offsets, int64_t n_groups) {
  eval_check_metrics(metrics, cutoffs, n_metrics);
  need((flags & ~MRK_EVAL_RELPOW) == 0, "eval: unknown flags");
  Checked c;
  c.sh = eval_check_groups(group_offsets, n_groups);
  need(labels != nullptr, "eval: null labels");
  c.gains.resize((size_t)c.sh.rows);
  c.rel.resize((size_t)c.sh.rows);
  eval_pack_labels(labels, c.sh.rows, (flags & MRK_EVAL_RELPOW) != 0, c.gains.data(), c.rel.data());
  for (int m = 0; m < n_metrics; ++m) c.need_ideal |= metrics[m] == MRK_METRIC_NDCG;
  return c;
}

// the device side of one call; the caller holds ctx->mu
struct EvalRun {
  mrk_ctx *ctx;
  hipStream_t s;
  int64_t n_groups;
  int n_metrics, n_sets;
  EvalBins bins;
  EvalDev dev{};
  const int64_t *offsets;
  DevBuf d_gains, d_rel, d_off, d_lg, d_met, d_cut, d_wave, d_group, d_out, d_scratch;

  EvalRun(mrk_ctx *c, const Checked &ck, const int *metrics, const int *cutoffs, int nm, double nolabels, const int64_t *group_offsets, int64_t ng, int sets,
          size_t other_bytes)
      : ctx(c), s(c->stream), n_groups(ng), n_metrics(nm), n_sets(sets), offsets(group_offsets) {
    const size_t rows = (size_t)ck.sh.rows;
    bins = eval_bins(group_offsets, ng, (int)std::min<long long>(std::max<long long>(env_int("MRK_EVAL_WAVE_MAX", EVAL_WAVE_ITEMS), 0), EVAL_WAVE_ITEMS));
    size_t scratch = 0;
    for (int32_t g : bins.big) scratch = std::max(scratch, eval_big_scratch_bytes((int)(group_offsets[g + 1] - group_offsets[g])));
    const std::vector<double> lg = eval_lg_table(ck.sh.max_len);
    const double want = 9.0 * (double)rows + 16.0 * (double)ng + 8.0 * (double)lg.size() + 8.0 * (double)sets * nm * (double)ng + (double)scratch + (double)other_bytes + 65536.0;
    size_t free_b = 0, total_b = 0;
    MRK_HIP(hipMemGetInfo(&free_b, &total_b));
    if (want > (double)free_b)
      throw StatusError(MRK_ERR_UNSUPPORTED, "eval: " + std::to_string(rows) + " rows in " + std::to_string(ng) + " groups need " + std::to_string((unsigned long long)want) +
                                                 " bytes on the device, " + std::to_string(free_b) + " are free");
    upload(d_gains, ck.gains, s);
    upload(d_rel, ck.rel, s);
    upload(d_lg, lg, s);
    if (!bins.wave.empty()) upload(d_wave, bins.wave, s);
    if (!bins.group.empty()) upload(d_group, bins.group, s);
    // (the caller's arrays are no vectors)
    d_off.reserve((size_t)(ng + 1) * 8);
    d_met.reserve((size_t)nm * 4);
    d_cut.reserve((size_t)nm * 4);
    d_out.reserve((size_t)sets * nm * (size_t)ng * 8);
    MRK_HIP(hipMemcpyAsync(d_off.p, group_offsets, (size_t)(ng + 1) * 8, hipMemcpyHostToDevice, s));
    MRK_HIP(hipMemcpyAsync(d_met.p, metrics, (size_t)nm * 4, hipMemcpyHostToDevice, s));
    MRK_HIP(hipMemcpyAsync(d_cut.p, cutoffs, (size_t)nm * 4, hipMemcpyHostToDevice, s));
    if (scratch) d_scratch.reserve(scratch);
    MRK_HIP(hipStreamSynchronize(s));   // lg is a local; the uploads have left the host
    dev.gains = d_gains.as<double>();
    dev.rel = d_rel.as<uint8_t>();
    dev.offsets = d_off.as<long long>();
    dev.lg = d_lg.as<double>();
    dev.metrics = d_met.as<int>();
    dev.cutoffs = d_cut.as<int>();
    dev.n_metrics = nm;
    dev.need_ideal = ck.need_ideal ? 1 : 0;
    dev.nolabels = nolabels;
    dev.n_groups = ng;
  }

  // every metric of every group for one array of scores (nullptr: the identity order) into set `set` of d_out
  void eval_set(const double *d_scores, int set) {
    EvalDev d = dev;
    d.scores = d_scores;
    d.out = d_out.as<double>() + (size_t)set * n_metrics * (size_t)n_groups;
    eval_launch_wave(ctx, s, d, d_wave.as<int>(), (int)bins.wave.size());
    eval_launch_group(ctx, s, d, d_group.as<int>(), (int)bins.group.size(), (int)bins.group_max_len);
    for (int32_t g : bins.big) eval_launch_big(ctx, s, d, g, offsets[g], (int)(offsets[g + 1] - offsets[g]), d_scratch.p);
  }

  // waits for the device; per_group: [set][metric][group]
  void fetch(std::vector<double> &per_group) {
    per_group.resize((size_t)n_sets * n_metrics * (size_t)n_groups);
    MRK_HIP(hipMemcpyAsync(per_group.data(), d_out.p, per_group.size() * 8, hipMemcpyDeviceToHost, s));
    MRK_HIP(hipStreamSynchronize(s));
    drain_profile_events(ctx);
  }
};

}  // namespace

extern "C" {

int mrk_eval_scores(mrk_ctx *ctx, int metric, int cutoff, int flags, double nolabels, const double *scores, const double *labels,
                    const int64_t *group_offsets, int64_t n_groups, double *out_value, double *out_per_group) {
  return guard([&] {
    need(out_value != nullptr, "eval: out_value is null");
    const Checked ck = check_common(&metric, &cutoff, 1, flags, labels, group_offsets, n_groups);
    need(scores != nullptr, "eval: null scores");
    need(ctx != nullptr, "null context");
    DeviceLock lk(ctx);
    const size_t rows = (size_t)ck.sh.rows;
    EvalRun run(ctx, ck, &metric, &cutoff, 1, nolabels, group_offsets, n_groups, 1, rows * 8);
    DevBuf d_scores;
    d_scores.reserve(rows * 8);
    MRK_HIP(hipMemcpyAsync(d_scores.p, scores, rows * 8, hipMemcpyHostToDevice, run.s));
    run.eval_set(d_scores.as<double>(), 0);
    std::vector<double> per_group;
    run.fetch(per_group);
    *out_value = eval_mean(per_group.data(), n_groups);
    if (out_per_group) memcpy(out_per_group, per_group.data(), (size_t)n_groups * 8);
  });
}

int mrk_model_eval(mrk_model *model, const int *metrics, const int *cutoffs, int n_metrics, int flags, double nolabels, const double *rowmajor, int cols,
                   const double *labels, const int64_t *group_offsets, int64_t n_groups, const double *random_scores, double *out, double *out_scores) {
  return guard([&] {
    need(out != nullptr, "eval: out is null");
    const Checked ck = check_common(metrics, cutoffs, n_metrics, flags, labels, group_offsets, n_groups);
    need(rowmajor != nullptr, "eval: null matrix");
    need(cols >= 0, "negative matrix shape");
    const std::vector<EvalPiece> pieces = eval_pieces(ck.sh.rows, cols, env_int("MRK_EVAL_PIECE_ROWS", 0));
    check_predict_args(model, rowmajor, pieces.empty() ? 0 : pieces[0].rows, cols, out);   // null / closed model, MRK_ERR_DIM_MISMATCH as predictMat gives
    mrk_ctx *ctx = model->ctx;
    DeviceLock lk(ctx);
    const size_t rows = (size_t)ck.sh.rows;
    const size_t piece_bytes = (size_t)pieces[0].rows * (size_t)std::max(cols, 1) * 8;
    const int n_sets = 3;   // predicted, noop, random
    EvalRun run(ctx, ck, metrics, cutoffs, n_metrics, nolabels, group_offsets, n_groups, n_sets, rows * 8 * (random_scores ? 2 : 1) + piece_bytes);
    hipStream_t s = run.s;
    // one predictMat over all rows, a piece of the matrix at a time: scoring is per row, so a group may straddle pieces
    DevBuf d_x, d_scores, d_random;
    d_x.reserve(piece_bytes);
    d_scores.reserve(rows * 8);
    MRK_HIP(hipMemsetAsync(ctx->d_flag.p, 0, sizeof(int), s));
    for (const EvalPiece &pc : pieces) {
      MRK_HIP(hipMemcpyAsync(d_x.p, rowmajor + (size_t)pc.row0 * (size_t)cols, (size_t)pc.rows * (size_t)cols * 8, hipMemcpyHostToDevice, s));
      ScopedKernelTimer timer(ctx, "eval_score");
      launch_score(ctx, model, d_x.as<double>(), pc.rows, cols, d_scores.as<double>() + pc.row0, ctx->d_flag.as<int>());
    }
    MRK_HIP(hipMemcpyAsync(ctx->h_flag.p, ctx->d_flag.p, sizeof(int), hipMemcpyDeviceToHost, s));
    run.eval_set(d_scores.as<double>(), 0);
    run.eval_set(nullptr, 1);
    if (random_scores) {
      d_random.reserve(rows * 8);
      MRK_HIP(hipMemcpyAsync(d_random.p, random_scores, rows * 8, hipMemcpyHostToDevice, s));
      run.eval_set(d_random.as<double>(), 2);
    }
    if (out_scores) MRK_HIP(hipMemcpyAsync(out_scores, d_scores.p, rows * 8, hipMemcpyDeviceToHost, s));
    std::vector<double> per_group;
    run.fetch(per_group);
    if (*ctx->h_flag.as<int>() & 1)
      throw StatusError(MRK_ERR_INVALID_ARG, "Input data contains `inf` or a value too large, while `missing` is not set to `inf`");
    for (int m = 0; m < n_metrics; ++m)
      for (int set = 0; set < n_sets; ++set)
        out[m * 3 + set] = set == 2 && !random_scores ? std::numeric_limits<double>::quiet_NaN()
                                                      : eval_mean(per_group.data() + ((size_t)set * n_metrics + m) * (size_t)n_groups, n_groups);
  });
}

}  // extern "C"
