// The LambdaMART fit on the device (LambdaMARTPredictor.makeBooster, ml/rank/LambdaMARTRanker.scala:161-190, for the LightGBM
// backend).  The algorithm is include/mrk.h's: LightGBM's lambdarank objective and leaf-wise histogram learner where
// the rules are public, and two departures that make every result independent of the order anything arrives in:
//   - whatever is summed across rows is an int64 sum of quantised gradients (LDS and global INTEGER atomics, parent - sibling);
//     no float atomics anywhere;
//   - exp and log2 are the host's (the sigmoid table, lg): the kernels add, multiply, divide and compare, each correctly rounded
//     and never fused.
// Kernels, in the order of one iteration:
//   train_grad_wave / train_grad_group   a group ordered by score (sort_key / pair_lt: the order /rank and eval.hip answer in), then
//                                        one lane per item adds its pairs in ascending partner rank.  n <= 64: one wavefront per
//                                        group, ranks by counting; n <= 4096: one workgroup, the LDS bitonic.  44.1 KiB of LDS.
//   train_grad_wave_bias / _group_bias   the same with step 3b (position_bias): every pair divided by t_plus[pos(hi)] *
//                                        t_minus[pos(lo)], and the pair costs cp, cm per item.  Then train_pos_sum: cp / cm quantised
//                                        and added per position, int64 LDS histograms flushed with global integer atomics
//   train_max, train_quantise            max |g|, max h as integer maxima of bit patterns; q = (int64) rint(ldexp(v, e))
//   train_hist                           per (TRAIN_HIST_ROWS rows, TRAIN_HIST_FEATS columns): LDS histograms of the rows of one
//                                        leaf, non-empty bins flushed with global integer atomics
//   train_scan, train_pick               sibling = parent - small; per (leaf, column) a prefix scan over the bins and the best
//                                        admitted candidate - a categorical column (step 5c): a sort-and-scan over its bins,
//                                        scan_cat_column -; per leaf the best column
//   train_split, train_split_cat         rows of the split leaf that go right get the new leaf (by bin <= b; by a mask over bins)
//   train_apply                          score += leaf value (training rows by leaf_of, validation rows by walking the tree)
// train_bin (once per fit) turns the f64 matrix into column-major bytes (a categorical column through its id -> bin table, step 2c).
// backend "xgboost" (steps 2x, 5x, 6x, 7x) grows LEVEL-wise with the same gradients, quantisation and scan body:
//   train_bin_f32                        the cell narrowed to f32, bin = the number of f32 bounds <= it; a "c" column (step 2cx)
//                                        through its id -> bin byte table, "other" 254, NaN 255
//   train_level_begin                    per tree: node_of = 0, hist_slot = 0 for a sampled row, 0xFFFF for the others
//   train_level_hist                     one launch per level, per (row tile, column, chunk of built nodes): LDS histograms of the rows
//                                        whose hist_slot lies in the chunk, non-empty bins flushed with global integer atomics
//   train_level_scan (+ train_pick)      per (node of the level, column): sibling = parent - built child, then scan_column under step
//                                        5x's admission rule - a "c" column (step 5cx): scan_cat_column_xgb, a counting rank and one
//                                        scan over its bins -; per node the best column; the level's records are read back once
//   train_level_split                    one row pass per level: the level's records in LDS, a row moves to its child and gets the
//                                        child's built slot (0xFFFF when the child is not built or the row is outside the sample);
//                                        <true>: a level with a categorical node, its masks over bins in LDS beside the records
//   train_level_apply, train_level_base  score = (double) ((float) score + leaf[node_of]); score = 0.5, the base_score
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "bitonic_device.hpp"
#include "runtime.hpp"
#include "sort_device.hpp"
#include "train.hpp"
#include "train_host.hpp"
#include "train_scan_device.hpp"
#include "wave_device.hpp"

namespace mrk {

static_assert(TRAIN_MAX_GROUP <= 65536, "the group kernel keeps indices as u16");
static_assert(TRAIN_HIST_ROWS % TRAIN_ROW_THREADS == 0 && TRAIN_LEVEL_ROWS % TRAIN_ROW_THREADS == 0, "a histogram workgroup takes whole rounds of rows");

namespace {

typedef unsigned long long u64;

constexpr int TG_WAVES = 4;   // groups per workgroup of the wavefront kernel

__device__ __forceinline__ double gain_of(int y) { return (double)((1u << y) - 1u); }   // 2^y - 1, y <= 30: exact

// s_cnt: how many items carry each label.  inv = 1 / maxDCG@k over the gains sorted descending, 0 when that is 0; one lane
__device__ double inv_max_dcg(const int *s_cnt, const double *__restrict__ lg, int k) {
  double acc = 0.0;
  int i = 0;
  for (int y = TRAIN_MAX_LABEL; y >= 0 && i < k; --y) {
    const double gn = gain_of(y);
    for (int c = s_cnt[y]; c > 0 && i < k; --c, ++i) acc = __dadd_rn(acc, __ddiv_rn(gn, lg[i]));
  }
  return acc == 0.0 ? 0.0 : __ddiv_rn(1.0, acc);
}

// Step 3b: where a kernel finds the position of a rank and the factors.  NoBias is the plain kernels': item_pairs<NoBias> holds no line
// of step 3b, a template parameter and not a branch in the pair loop.
struct NoBias {};
// the wavefront kernel: the clamped position of every rank and every factor the group can reach sit in the wavefront's LDS slice
struct WaveBias {
  const unsigned char *s_pos;
  const double *s_tp, *s_tm, *cost;
  __device__ __forceinline__ int pos(int q) const { return s_pos[q]; }
  __device__ __forceinline__ double tp(int i) const { return s_tp[i]; }
  __device__ __forceinline__ double tm(int i) const { return s_tm[i]; }
};
// the workgroup kernel: s_idx already holds the rank's place in the list; the first TRAIN_BIAS_LDS_POS factors per side are in LDS
struct GroupBias {
  const unsigned short *s_idx;
  const double *s_tp, *s_tm, *g_tp, *g_tm, *cost;
  int last;   // positions - 1
  __device__ __forceinline__ int pos(int q) const { return min((int)s_idx[q], last); }
  __device__ __forceinline__ double tp(int i) const { return i < TRAIN_BIAS_LDS_POS ? s_tp[i] : g_tp[i]; }
  __device__ __forceinline__ double tm(int i) const { return i < TRAIN_BIAS_LDS_POS ? s_tm[i] : g_tm[i]; }
};

// the pairs of the item at rank r: s_key / s_lab in rank order; (g, h) of that item and, under step 3b, its (cp, cm)
template <typename B>
__device__ __forceinline__ void item_pairs(const GradDev &d, const B &b, const u64 *s_key, const unsigned char *s_lab, int n, int k, int r, double inv,
                                           double &g_out, double &h_out, double &cp_out, double &cm_out) {
  constexpr bool BIAS = !std::is_same<B, NoBias>::value;
  const int y = s_lab[r];
  const double sr = -asc_value(s_key[r]);   // sort_key(s) = asc_key(-s)
  const double gr = gain_of(y), ilr = d.invlg[r];
  const int qn = r < k ? n : k;             // a pair counts when min(r, q) < k
  double g = 0.0, h = 0.0;
  double cp = 0.0, cm = 0.0, own_p = 1.0, own_m = 1.0;   // 3b: this item's t_plus and t_minus, read once
  if constexpr (BIAS) {
    const int pr = b.pos(r);
    own_p = b.tp(pr), own_m = b.tm(pr);
  }
  for (int q = 0; q < qn; ++q) {
    const int yq = s_lab[q];
    if (yq == y) continue;                  // (q == r too)
    const double sq = -asc_value(s_key[q]);
    const double gq = gain_of(yq), ilq = d.invlg[q];
    const bool hi = y > yq;
    const double delta = hi ? __dsub_rn(sr, sq) : __dsub_rn(sq, sr);
    const double t = fmin(fmax(__dmul_rn(__dsub_rn(delta, d.lo), d.f), 0.0), (double)(TRAIN_SIGMOID_BINS - 1));
    const double rho = d.sigmoid[(int)t];
    // 3b: both table reads go out with one index before anything waits for either; the partner's factor comes from LDS meanwhile
    double L = 0.0, x = 1.0;
    if constexpr (BIAS) {
      L = b.cost[(int)t];
      const int pq = b.pos(q);
      x = hi ? b.tm(pq) : b.tp(pq);   // the partner's side of c = t_plus[pos(hi)] * t_minus[pos(lo)]
    }
    const double dg = hi ? __dsub_rn(gr, gq) : __dsub_rn(gq, gr);
    const double dl = fabs(hi ? __dsub_rn(ilr, ilq) : __dsub_rn(ilq, ilr));
    const double w = __dmul_rn(__dmul_rn(dg, dl), inv);
    double lam = __dmul_rn(__dmul_rn(d.sigma, rho), w);
    double eta = __dmul_rn(__dmul_rn(__dmul_rn(d.sigma2, rho), __dsub_rn(1.0, rho)), w);
    if constexpr (BIAS) {   // three divisions that do not depend on each other: their refinement steps interleave
      const double c = __dmul_rn(hi ? own_p : own_m, x);
      lam = __ddiv_rn(lam, c);
      eta = __ddiv_rn(eta, c);
      const double share = __ddiv_rn(__dmul_rn(L, w), x);   // cost / t_minus[j] for the clicked side, cost / t_plus[i] for the other
      cp = hi ? __dadd_rn(cp, share) : cp;
      cm = hi ? cm : __dadd_rn(cm, share);
    }
    g = hi ? __dsub_rn(g, lam) : __dadd_rn(g, lam);
    h = __dadd_rn(h, eta);
  }
  g_out = g;
  h_out = h;
  cp_out = cp;
  cm_out = cm;
}

__global__ void __launch_bounds__(TG_WAVES * 64)
train_grad_wave_kernel(GradDev d, const int *__restrict__ groups, int count) {
  __shared__ u64 s_tmp[TG_WAVES][64], s_key[TG_WAVES][64];
  __shared__ unsigned char s_lab[TG_WAVES][64];
  __shared__ int s_cnt[TG_WAVES][32];
  __shared__ double s_inv[TG_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int gi = blockIdx.x * TG_WAVES + wave;
  if (gi >= count) return;   // (a whole wavefront: the slices below are its own, ordered by wave_lds_sync)
  const int g = groups[gi];
  const long long base = d.offsets[g];
  const int n = (int)(d.offsets[g + 1] - base);   // 1 ... 64
  const bool mine = lane < n;
  const int k = min(d.truncation, n);
  const u64 key = mine ? sort_key(d.scores[base + lane]) : ~0ull;
  const int y = mine ? d.labels[base + lane] : 0;
  s_tmp[wave][lane] = key;
  if (lane < 32) s_cnt[wave][lane] = 0;
  wave_lds_sync();
  int rank = 0;
  if (mine) {
    for (int j = 0; j < n; ++j) rank += pair_lt(s_tmp[wave][j], j, key, lane) ? 1 : 0;
    s_key[wave][rank] = key;
    s_lab[wave][rank] = (unsigned char)y;
    atomicAdd(&s_cnt[wave][y], 1);
  }
  wave_lds_sync();
  if (lane == 0) s_inv[wave] = inv_max_dcg(s_cnt[wave], d.lg, k);
  wave_lds_sync();
  if (mine) {
    double gg, hh, cp, cm;
    item_pairs(d, NoBias{}, s_key[wave], s_lab[wave], n, k, rank, s_inv[wave], gg, hh, cp, cm);
    d.g[base + lane] = gg;
    d.h[base + lane] = hh;
  }
}

// blockDim.x: a multiple of 64 up to 1024
__global__ void __launch_bounds__(1024)
train_grad_group_kernel(GradDev d, const int *__restrict__ groups) {
  __shared__ u64 s_key[TRAIN_MAX_GROUP];
  __shared__ unsigned short s_idx[TRAIN_MAX_GROUP];
  __shared__ unsigned char s_lab[TRAIN_MAX_GROUP];
  __shared__ int s_cnt[32];
  __shared__ double s_inv;
  const int tid = threadIdx.x, T = blockDim.x;
  const int g = groups[blockIdx.x];
  const long long base = d.offsets[g];
  const int n = (int)(d.offsets[g + 1] - base);   // 1 ... TRAIN_MAX_GROUP
  const int k = min(d.truncation, n);
  int p2 = 1;
  while (p2 < n) p2 <<= 1;
  for (int i = tid; i < p2; i += T) {
    s_key[i] = i < n ? sort_key(d.scores[base + i]) : ~0ull;   // (a pad sorts behind every score)
    s_idx[i] = (unsigned short)(i < n ? i : 0xffff);
  }
  if (tid < 32) s_cnt[tid] = 0;
  __syncthreads();
  lds_bitonic<true>(s_key, s_idx, p2);
  for (int r = tid; r < n; r += T) {
    const int y = d.labels[base + s_idx[r]];
    s_lab[r] = (unsigned char)y;
    atomicAdd(&s_cnt[y], 1);
  }
  __syncthreads();
  if (tid == 0) s_inv = inv_max_dcg(s_cnt, d.lg, k);
  __syncthreads();
  const double inv = s_inv;
  for (int r = tid; r < n; r += T) {
    double gg, hh, cp, cm;
    item_pairs(d, NoBias{}, s_key, s_lab, n, k, r, inv, gg, hh, cp, cm);
    d.g[base + s_idx[r]] = gg;
    d.h[base + s_idx[r]] = hh;
  }
}

// Step 3b's variants of the two kernels above: the same steps, item_pairs under WaveBias / GroupBias, and 3b's staging.  They are kernels
// of their own and not one templated body behind both pairs: a body behind a function call makes the plain kernels load their arguments
// in one piece and changes their machine code.
// One wavefront per group of <= 64 rows: the lane index before ranking is the item's place in the list; it goes to LDS beside the key
// and the label of its rank, with the min(positions, n) factors per side the group can reach.
__global__ void __launch_bounds__(TG_WAVES * 64)
train_grad_wave_bias_kernel(GradDev d, BiasDev b, const int *__restrict__ groups, int count) {
  __shared__ u64 s_tmp[TG_WAVES][64], s_key[TG_WAVES][64];
  __shared__ unsigned char s_lab[TG_WAVES][64], s_pos[TG_WAVES][64];
  __shared__ int s_cnt[TG_WAVES][32];
  __shared__ double s_inv[TG_WAVES], s_tp[TG_WAVES][64], s_tm[TG_WAVES][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int gi = blockIdx.x * TG_WAVES + wave;
  if (gi >= count) return;   // (a whole wavefront, as above)
  const int g = groups[gi];
  const long long base = d.offsets[g];
  const int n = (int)(d.offsets[g + 1] - base);   // 1 ... 64
  const bool mine = lane < n;
  const int k = min(d.truncation, n);
  const u64 key = mine ? sort_key(d.scores[base + lane]) : ~0ull;
  const int y = mine ? d.labels[base + lane] : 0;
  s_tmp[wave][lane] = key;
  if (lane < 32) s_cnt[wave][lane] = 0;
  if (lane < min(b.positions, n)) {
    s_tp[wave][lane] = b.t_plus[lane];
    s_tm[wave][lane] = b.t_minus[lane];
  }
  wave_lds_sync();
  int rank = 0;
  if (mine) {
    for (int j = 0; j < n; ++j) rank += pair_lt(s_tmp[wave][j], j, key, lane) ? 1 : 0;
    s_key[wave][rank] = key;
    s_lab[wave][rank] = (unsigned char)y;
    s_pos[wave][rank] = (unsigned char)min(lane, b.positions - 1);
    atomicAdd(&s_cnt[wave][y], 1);
  }
  wave_lds_sync();
  if (lane == 0) s_inv[wave] = inv_max_dcg(s_cnt[wave], d.lg, k);
  wave_lds_sync();
  if (mine) {
    double gg, hh, cp, cm;
    item_pairs(d, WaveBias{s_pos[wave], s_tp[wave], s_tm[wave], b.cost}, s_key[wave], s_lab[wave], n, k, rank, s_inv[wave], gg, hh, cp, cm);
    d.g[base + lane] = gg;
    d.h[base + lane] = hh;
    b.cp[base + lane] = cp;
    b.cm[base + lane] = cm;
  }
}

// One workgroup per group; blockDim.x: a multiple of 64 up to 1024.  s_idx is the position before clamping; the first min(positions, n,
// TRAIN_BIAS_LDS_POS) factors per side are staged in LDS (60.1 KiB with them), a longer list reads the rest from memory.
__global__ void __launch_bounds__(1024)
train_grad_group_bias_kernel(GradDev d, BiasDev b, const int *__restrict__ groups) {
  __shared__ u64 s_key[TRAIN_MAX_GROUP];
  __shared__ unsigned short s_idx[TRAIN_MAX_GROUP];
  __shared__ unsigned char s_lab[TRAIN_MAX_GROUP];
  __shared__ int s_cnt[32];
  __shared__ double s_inv, s_tp[TRAIN_BIAS_LDS_POS], s_tm[TRAIN_BIAS_LDS_POS];
  const int tid = threadIdx.x, T = blockDim.x;
  const int g = groups[blockIdx.x];
  const long long base = d.offsets[g];
  const int n = (int)(d.offsets[g + 1] - base);   // 1 ... TRAIN_MAX_GROUP
  const int k = min(d.truncation, n);
  int p2 = 1;
  while (p2 < n) p2 <<= 1;
  for (int i = tid; i < p2; i += T) {
    s_key[i] = i < n ? sort_key(d.scores[base + i]) : ~0ull;   // (a pad sorts behind every score)
    s_idx[i] = (unsigned short)(i < n ? i : 0xffff);
  }
  if (tid < 32) s_cnt[tid] = 0;
  for (int i = tid; i < min(min(b.positions, n), TRAIN_BIAS_LDS_POS); i += T) {
    s_tp[i] = b.t_plus[i];
    s_tm[i] = b.t_minus[i];
  }
  __syncthreads();
  lds_bitonic<true>(s_key, s_idx, p2);
  for (int r = tid; r < n; r += T) {
    const int y = d.labels[base + s_idx[r]];
    s_lab[r] = (unsigned char)y;
    atomicAdd(&s_cnt[y], 1);
  }
  __syncthreads();
  if (tid == 0) s_inv = inv_max_dcg(s_cnt, d.lg, k);
  __syncthreads();
  const double inv = s_inv;
  const GroupBias gb{s_idx, s_tp, s_tm, b.t_plus, b.t_minus, b.cost, b.positions - 1};
  for (int r = tid; r < n; r += T) {
    double gg, hh, cp, cm;
    item_pairs(d, gb, s_key, s_lab, n, k, r, inv, gg, hh, cp, cm);
    d.g[base + s_idx[r]] = gg;
    d.h[base + s_idx[r]] = hh;
    b.cp[base + s_idx[r]] = cp;
    b.cm[base + s_idx[r]] = cm;
  }
}

// Step 3b's position sums.  A workgroup takes `run` consecutive groups, a wavefront one group at a time, a lane the rows 64 apart: the
// row's place in its list is then the loop counter.  cp / cm are quantised on the way (train_quantise's rounding) into an int64 LDS
// histogram per side; a lane keeps what falls on the clamped last position in registers - with few positions that is most rows, and
// they would queue on one LDS address - and adds it once.  Non-zero bins are flushed with global integer atomics (train_hist's pattern).
__global__ void __launch_bounds__(TRAIN_ROW_THREADS)
train_pos_sum_kernel(const double *__restrict__ cp, const double *__restrict__ cm, const long long *__restrict__ offsets, long long n_groups, int run,
                     int positions, int e_p, int e_m, u64 *__restrict__ Qp, u64 *__restrict__ Qm) {
  __shared__ u64 s_p[TRAIN_POS_LDS_BINS], s_m[TRAIN_POS_LDS_BINS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int last = positions - 1, lds_n = min(positions, TRAIN_POS_LDS_BINS);
  for (int i = tid; i < lds_n; i += TRAIN_ROW_THREADS) {
    s_p[i] = 0;
    s_m[i] = 0;
  }
  __syncthreads();
  const long long g0 = (long long)blockIdx.x * run, g1 = min(g0 + run, n_groups);
  u64 tail_p = 0, tail_m = 0;   // (two's complement: the unsigned sum is the signed one)
  for (long long g = g0 + wave; g < g1; g += TRAIN_ROW_THREADS / 64) {
    const long long base = offsets[g];
    const int n = (int)(offsets[g + 1] - base);
    for (int i = lane; i < n; i += 64) {
      const u64 qp = (u64)(long long)rint(ldexp(cp[base + i], e_p)), qm = (u64)(long long)rint(ldexp(cm[base + i], e_m));
      if (i >= last) {
        tail_p += qp;
        tail_m += qm;
      } else if (i < TRAIN_POS_LDS_BINS) {
        if (qp) atomicAdd(&s_p[i], qp);
        if (qm) atomicAdd(&s_m[i], qm);
      } else {
        if (qp) atomicAdd(&Qp[i], qp);
        if (qm) atomicAdd(&Qm[i], qm);
      }
    }
  }
  if (last < TRAIN_POS_LDS_BINS) {
    if (tail_p) atomicAdd(&s_p[last], tail_p);
    if (tail_m) atomicAdd(&s_m[last], tail_m);
  } else {
    if (tail_p) atomicAdd(&Qp[last], tail_p);
    if (tail_m) atomicAdd(&Qm[last], tail_m);
  }
  __syncthreads();
  for (int i = tid; i < lds_n; i += TRAIN_ROW_THREADS) {
    if (s_p[i]) atomicAdd(&Qp[i], s_p[i]);
    if (s_m[i]) atomicAdd(&Qm[i], s_m[i]);
  }
}

__global__ void __launch_bounds__(TRAIN_BIN_ROWS)
train_bin_kernel(const double *__restrict__ x, int piece_rows, int cols, const double *__restrict__ bounds, const int *__restrict__ bound_off,
                 const int *__restrict__ cat_idx, const uint8_t *__restrict__ cat_tables, uint8_t *__restrict__ bins, long long rows, long long row0) {
  const int i = blockIdx.x * TRAIN_BIN_ROWS + threadIdx.x;
  if (i >= piece_rows) return;
  const double *row = x + (long long)i * cols;
  for (int c = 0; c < cols; ++c) {
    const double v = row[c];
    if (cat_idx && cat_idx[2 * c] >= 0) {   // (the same for every lane: a categorical column, step 2c)
      bins[(long long)c * rows + row0 + i] = (uint8_t)train_category_bin(v, cat_tables + cat_idx[2 * c], cat_idx[2 * c + 1]);
      continue;
    }
    int a = bound_off[c], b = bound_off[c + 1];
    const int first = a;
    while (a < b) {   // the number of bounds < v
      const int m = (a + b) >> 1;
      if (bounds[m] < v) a = m + 1;
      else b = m;
    }
    bins[(long long)c * rows + row0 + i] = v != v ? (uint8_t)TRAIN_NAN_BIN : (uint8_t)(a - first);
  }
}

__global__ void __launch_bounds__(TRAIN_ROW_THREADS)
train_max_kernel(const double *__restrict__ g, const double *__restrict__ h, long long rows, u64 *__restrict__ maxes) {
  __shared__ u64 s_max[2];
  if (threadIdx.x < 2) s_max[threadIdx.x] = 0;
  __syncthreads();
  u64 mg = 0, mh = 0;
  for (long long i = (long long)blockIdx.x * TRAIN_ROW_THREADS + threadIdx.x; i < rows; i += (long long)gridDim.x * TRAIN_ROW_THREADS) {
    mg = max(mg, (u64)__double_as_longlong(fabs(g[i])));
    mh = max(mh, (u64)__double_as_longlong(fabs(h[i])));
  }
  atomicMax(&s_max[0], mg);
  atomicMax(&s_max[1], mh);
  __syncthreads();
  if (threadIdx.x < 2) atomicMax(&maxes[threadIdx.x], s_max[threadIdx.x]);
}

__global__ void __launch_bounds__(TRAIN_ROW_THREADS)
train_quantise_kernel(const double *__restrict__ g, const double *__restrict__ h, long long rows, int e_g, int e_h, long long *__restrict__ qg,
                      long long *__restrict__ qh, uint16_t *__restrict__ leaf_of) {
  const long long i = (long long)blockIdx.x * TRAIN_ROW_THREADS + threadIdx.x;
  if (i >= rows) return;
  qg[i] = (long long)rint(ldexp(g[i], e_g));
  qh[i] = (long long)rint(ldexp(h[i], e_h));
  leaf_of[i] = 0;
}

__global__ void __launch_bounds__(TRAIN_ROW_THREADS)
train_hist_kernel(const uint8_t *__restrict__ bins, long long rows, const uint16_t *__restrict__ leaf_of, int leaf, int slot, const long long *__restrict__ qg,
                  const long long *__restrict__ qh, const int *__restrict__ subset, HistDev hd) {
  __shared__ u64 s_g[TRAIN_HIST_FEATS][256], s_h[TRAIN_HIST_FEATS][256];
  __shared__ unsigned s_c[TRAIN_HIST_FEATS][256];
  const int tid = threadIdx.x;
  const int j0 = blockIdx.y * TRAIN_HIST_FEATS;
  const int nf = min(TRAIN_HIST_FEATS, hd.n_sub - j0);
  for (int f = 0; f < nf; ++f) {
    s_g[f][tid] = 0;
    s_h[f][tid] = 0;
    s_c[f][tid] = 0;
  }
  const uint8_t *col[TRAIN_HIST_FEATS];
  for (int f = 0; f < TRAIN_HIST_FEATS; ++f) col[f] = bins + (long long)subset[j0 + min(f, nf - 1)] * rows;
  __syncthreads();
  const long long tile0 = (long long)blockIdx.x * TRAIN_HIST_ROWS;
  for (int step = 0; step < TRAIN_HIST_ROWS / TRAIN_ROW_THREADS; ++step) {
    const long long row = tile0 + step * TRAIN_ROW_THREADS + tid;
    if (row < rows && leaf_of[row] == leaf) {
      const u64 vg = (u64)qg[row], vh = (u64)qh[row];   // (two's complement: the unsigned sum is the signed one)
      for (int f = 0; f < nf; ++f) {
        const int b = col[f][row];
        atomicAdd(&s_g[f][b], vg);
        atomicAdd(&s_h[f][b], vh);
        atomicAdd(&s_c[f][b], 1u);
      }
    }
  }
  __syncthreads();
  for (int f = 0; f < nf; ++f) {
    const unsigned c = s_c[f][tid];
    if (c == 0) continue;
    const size_t at = ((size_t)slot * hd.n_sub + (size_t)(j0 + f)) * 256 + tid;
    atomicAdd((u64 *)&hd.G[at], s_g[f][tid]);
    atomicAdd((u64 *)&hd.H[at], s_h[f][tid]);
    atomicAdd(&hd.C[at], c);
  }
}

// lane b holds bin b of one (leaf, column); the best admitted candidate of the column into *out
__device__ void scan_column(long long g, long long h, long long c, int nb, int col, const ScanParams &p, LeafRec *out, long long (*s_buf)[3][256],
                            double *s_gain, int *s_code, long long *s_nan) {
  const int tid = threadIdx.x;
  if (tid == TRAIN_NAN_BIN) {
    s_nan[0] = g, s_nan[1] = h, s_nan[2] = c;
    g = 0, h = 0, c = 0;
  }
  long long pg = g, ph = h, pc = c;
  block_scan(pg, ph, pc, s_buf);          // (its first barrier publishes s_nan)
  const long long ng = s_nan[0], nh = s_nan[1], nc = s_nan[2];
  if (tid == 255) s_nan[3] = pg + ng, s_nan[4] = ph + nh, s_nan[5] = pc + nc;   // (lane 255 added nothing of its own: the sum of the other bins)
  __syncthreads();
  const long long Tg = s_nan[3], Th = s_nan[4], Tc = s_nan[5];
  double best = 0.0;
  int code = -1;
  long long bl_g = 0, bl_h = 0, bl_c = 0;
  if (tid <= nb - 2) {
    const double parent = side_term(Tg, Th, p);
    for (int nl = 0; nl <= (nc > 0 ? 1 : 0); ++nl) {
      const long long lg_ = pg + (nl ? ng : 0), lh = ph + (nl ? nh : 0), lc = pc + (nl ? nc : 0);
      const long long rg = Tg - lg_, rh = Th - lh, rc = Tc - lc;
      const double HL = real_of(lh, p.e_h), HR = real_of(rh, p.e_h);
      const double gain = __dsub_rn(__dadd_rn(side_term(lg_, lh, p), side_term(rg, rh, p)), parent);
      const bool ok = lc >= p.min_data && rc >= p.min_data && HL >= p.min_hess && HR >= p.min_hess && gain > p.min_gain;
      if (ok && (code < 0 || gain > best)) {   // (NaN to the right wins a tie)
        best = gain;
        code = tid * 2 + nl;
        bl_g = lg_, bl_h = lh, bl_c = lc;
      }
    }
  }
  const int win = block_best(best, code, s_gain, s_code);
  if (win < 0 ? tid == 0 : tid == (win >> 1)) {
    LeafRec r;
    r.gain = win < 0 ? 0.0 : best;
    r.valid = win < 0 ? 0 : 1;
    r.col = col;
    r.bin = win < 0 ? 0 : tid;
    r.nan_left = win < 0 ? 0 : (win & 1);
    r.gl = bl_g, r.hl = bl_h, r.cl = bl_c;
    r.g = Tg, r.h = Th, r.c = Tc;
    r.is_cat = 0;
    for (int w = 0; w < 8; ++w) r.cat_mask[w] = 0;
    *out = r;
  }
  __syncthreads();   // (s_gain, s_code, s_nan are written again by the next call)
}

// Step 5c: lane b holds bin b of one (leaf, CATEGORICAL column) - b < nb a kept category, 255 everything without one, which always goes
// right.  A candidate is a set of bins < nb that goes left.  nb <= max_onehot: one bin against the rest, lane b judges {b}.  Else the
// bins with count >= cat_smooth, ordered ascending by (G / (H + cat_smooth), bin): lane i judges the first i + 1 of them and the last
// i + 1, i < min(max_cat_threshold, (m + 1) / 2), each on its own.  The order is a counting rank: every lane compares its key with
// all nb keys, read as LDS broadcasts (one address per instruction: no bank conflict) behind ONE barrier; a bitonic network would
// take 36 barrier-separated stages for 256 keys and padding keys for the bins that are not eligible.  The bins that are not
// eligible are put behind the eligible ones, so one block_scan gives the prefix sums, the eligible total (position m - 1) and the
// leaf's total (position 255).
__device__ void scan_cat_column(long long g, long long h, long long c, int nb, int col, const ScanParams &p, LeafRec *out, long long (*s_buf)[3][256],
                                double *s_gain, int *s_code, long long *s_nan, u64 *s_mask) {
  const int tid = threadIdx.x;
  const bool onehot = nb <= p.max_onehot;
  bool elig = false;
  int pos = tid, m = 0;   // pos: where this lane's bin stands in the order; m: eligible bins
  if (!onehot) {
    elig = tid < nb && (double)c >= p.cat_smooth;
    const double key = elig ? __ddiv_rn(real_of(g, p.e_g), __dadd_rn(real_of(h, p.e_h), p.cat_smooth)) : 0.0;   // finite, never -0.0
    s_gain[tid] = key;
    s_code[tid] = elig ? 1 : 0;
    __syncthreads();
    int below = 0, before = 0;   // eligible bins that stand before this one in the order; eligible bins of a lower index
    for (int j = 0; j < nb; ++j) {
      const double kj = s_gain[j];
      const int ej = s_code[j];
      m += ej;
      before += (ej && j < tid) ? 1 : 0;
      below += (ej && (kj < key || (kj == key && j < tid))) ? 1 : 0;
    }
    pos = elig ? below : m + (tid - before);   // (a permutation of 0 ... 255)
    s_buf[0][0][pos] = g;
    s_buf[0][1][pos] = h;
    s_buf[0][2][pos] = c;
    __syncthreads();
    g = s_buf[0][0][tid];
    h = s_buf[0][1][tid];
    c = s_buf[0][2][tid];
  }
  long long pg = g, ph = h, pc = c;
  block_scan(pg, ph, pc, s_buf);   // (its first barrier: every lane has read its position)
  s_buf[0][0][tid] = pg;
  s_buf[0][1][tid] = ph;
  s_buf[0][2][tid] = pc;
  __syncthreads();
  const long long Tg = s_buf[0][0][255], Th = s_buf[0][1][255], Tc = s_buf[0][2][255];
  const double l2s = onehot ? p.l2 : p.l2_cat;
  const long long min_count = onehot ? p.min_data : p.min_data_cat;
  const int n_cand = onehot ? nb : min(p.max_cat_threshold, (m + 1) / 2);
  double best = 0.0;
  int code = -1;
  long long bl_g = 0, bl_h = 0, bl_c = 0;
  if (tid < n_cand) {
    const double parent = side_term(Tg, Th, p);   // (the parent's term keeps lambda_l2 alone)
    for (int dir = 0; dir <= (onehot ? 0 : 1); ++dir) {
      long long lg_, lh, lc;
      if (onehot) lg_ = g, lh = h, lc = c;
      else if (dir == 0) lg_ = pg, lh = ph, lc = pc;
      else {   // the last tid + 1 of the m eligible bins: their total minus the first m - 1 - tid
        const int k = m - 2 - tid;
        lg_ = s_buf[0][0][m - 1] - (k >= 0 ? s_buf[0][0][k] : 0);
        lh = s_buf[0][1][m - 1] - (k >= 0 ? s_buf[0][1][k] : 0);
        lc = s_buf[0][2][m - 1] - (k >= 0 ? s_buf[0][2][k] : 0);
      }
      const long long rg = Tg - lg_, rh = Th - lh, rc = Tc - lc;
      const double HL = real_of(lh, p.e_h), HR = real_of(rh, p.e_h);
      const double gain = __dsub_rn(__dadd_rn(side_term_l2(lg_, lh, p, l2s), side_term_l2(rg, rh, p, l2s)), parent);
      const bool ok = lc >= min_count && rc >= min_count && HL >= p.min_hess && HR >= p.min_hess && gain > 0.0;
      if (ok && (code < 0 || gain > best)) {   // (direction 0 wins a tie)
        best = gain;
        code = dir * 256 + tid;
        bl_g = lg_, bl_h = lh, bl_c = lc;
      }
    }
  }
  const int win = block_best(best, code, s_gain, s_code);
  const int wdir = win >> 8, wi = win & 255;
  if (win >= 0 && tid == wi) s_nan[0] = bl_g, s_nan[1] = bl_h, s_nan[2] = bl_c;
  // the winner's left set as a mask over BINS: lane b knows where bin b stands
  const bool member = win >= 0 && (onehot ? tid == wi : (elig && (wdir == 0 ? pos <= wi : pos >= m - 1 - wi)));
  const u64 wave_mask = __ballot(member);
  if ((tid & 63) == 0) s_mask[tid >> 6] = wave_mask;
  __syncthreads();
  if (tid == 0) {
    LeafRec r;
    r.gain = win < 0 ? 0.0 : s_gain[0];
    r.valid = win < 0 ? 0 : 1;
    r.col = col;
    r.bin = 0;
    r.nan_left = 0;
    r.gl = win < 0 ? 0 : s_nan[0], r.hl = win < 0 ? 0 : s_nan[1], r.cl = win < 0 ? 0 : s_nan[2];
    r.g = Tg, r.h = Th, r.c = Tc;
    r.is_cat = 1;
    for (int w = 0; w < 4; ++w) {
      r.cat_mask[2 * w] = (unsigned)s_mask[w];
      r.cat_mask[2 * w + 1] = (unsigned)(s_mask[w] >> 32);
    }
    *out = r;
  }
  __syncthreads();   // (everything in LDS is written again by the next call)
}

// one workgroup per subset column j, lane b = bin b
__global__ void __launch_bounds__(256)
train_scan_kernel(HistDev hd, const int *__restrict__ subset, const int *__restrict__ nbins, const int *__restrict__ is_cat, int leaf_a, int leaf_b,
                  int small_is_left, ScanParams p, LeafRec *__restrict__ feat_best) {
  __shared__ long long s_buf[2][3][256];
  __shared__ double s_gain[256];
  __shared__ int s_code[256];
  __shared__ long long s_nan[6];   // the NaN bin's sums, the leaf's totals
  __shared__ u64 s_mask[4];        // a categorical winner's left bins: one ballot per wavefront
  const int tid = threadIdx.x, j = blockIdx.x;
  const int col = subset[j], nb = nbins[col];
  const bool cat = is_cat[col] != 0;   // (the same for the whole workgroup)
  const size_t ia = ((size_t)leaf_a * hd.n_sub + j) * 256 + tid;
  long long ag = hd.G[ia], ah = hd.H[ia], ac = hd.C[ia];
  long long bg = 0, bh = 0, bc = 0;
  if (leaf_b >= 0) {
    // slot b: the smaller child's histogram; slot a: the parent's.  Afterwards each slot holds its own leaf's.
    const size_t ib = ((size_t)leaf_b * hd.n_sub + j) * 256 + tid;
    const long long sg = hd.G[ib], sh = hd.H[ib], sc = hd.C[ib];
    if (small_is_left) {
      bg = ag - sg, bh = ah - sh, bc = ac - sc;
      ag = sg, ah = sh, ac = sc;
    } else {
      ag -= sg, ah -= sh, ac -= sc;
      bg = sg, bh = sh, bc = sc;
    }
    hd.G[ia] = ag, hd.H[ia] = ah, hd.C[ia] = (unsigned)ac;
    hd.G[ib] = bg, hd.H[ib] = bh, hd.C[ib] = (unsigned)bc;
  }
  if (cat) {
    scan_cat_column(ag, ah, ac, nb, col, p, &feat_best[j], s_buf, s_gain, s_code, s_nan, s_mask);
    if (leaf_b >= 0) scan_cat_column(bg, bh, bc, nb, col, p, &feat_best[hd.n_sub + j], s_buf, s_gain, s_code, s_nan, s_mask);
    return;
  }
  scan_column(ag, ah, ac, nb, col, p, &feat_best[j], s_buf, s_gain, s_code, s_nan);
  if (leaf_b >= 0) scan_column(bg, bh, bc, nb, col, p, &feat_best[hd.n_sub + j], s_buf, s_gain, s_code, s_nan);
}

// one wavefront per leaf: the best column (the highest gain, then the lowest: the subset ascends)
__global__ void __launch_bounds__(64)
train_pick_kernel(const LeafRec *__restrict__ feat_best, int n_sub, LeafRec *__restrict__ out) {
  __shared__ double s_gain[64];
  __shared__ int s_j[64];
  const int lane = threadIdx.x;
  const LeafRec *fb = feat_best + (size_t)blockIdx.x * n_sub;
  double best = 0.0;
  int bj = -1;
  for (int j = lane; j < n_sub; j += 64)
    if (fb[j].valid && (bj < 0 || fb[j].gain > best)) {
      best = fb[j].gain;
      bj = j;
    }
  s_gain[lane] = best;
  s_j[lane] = bj;
  wave_lds_sync();
  if (lane == 0) {
    for (int l = 1; l < 64; ++l)
      if (s_j[l] >= 0 && (bj < 0 || s_gain[l] > best || (s_gain[l] == best && s_j[l] < bj))) {
        best = s_gain[l];
        bj = s_j[l];
      }
    out[blockIdx.x] = fb[bj < 0 ? 0 : bj];
  }
}

__global__ void __launch_bounds__(TRAIN_ROW_THREADS)
train_split_kernel(const uint8_t *__restrict__ col_bins, long long rows, uint16_t *__restrict__ leaf_of, int leaf, int fresh, int bin, int nan_left) {
  const long long i = (long long)blockIdx.x * TRAIN_ROW_THREADS + threadIdx.x;
  if (i >= rows || leaf_of[i] != leaf) return;
  const int b = col_bins[i];
  const bool left = b <= bin || (b == TRAIN_NAN_BIN && nan_left);
  if (!left) leaf_of[i] = (uint16_t)fresh;
}

// the categorical form: the mask comes as kernel arguments; its word is picked by selects (a lane-indexed argument would go to scratch)
__global__ void __launch_bounds__(TRAIN_ROW_THREADS)
train_split_cat_kernel(const uint8_t *__restrict__ col_bins, long long rows, uint16_t *__restrict__ leaf_of, int leaf, int fresh, CatMask mask) {
  const long long i = (long long)blockIdx.x * TRAIN_ROW_THREADS + threadIdx.x;
  if (i >= rows || leaf_of[i] != leaf) return;
  const int b = col_bins[i];
  unsigned word = 0;
#pragma unroll
  for (int w = 0; w < 8; ++w) word = (b >> 5) == w ? mask.w[w] : word;
  const bool left = b != TRAIN_NAN_BIN && ((word >> (b & 31)) & 1u);
  if (!left) leaf_of[i] = (uint16_t)fresh;
}

// CAT: the tree has a categorical node (the host picks the form; the numeric one reads neither is_cat nor cat_mask)
template <bool CAT>
__global__ void __launch_bounds__(TRAIN_ROW_THREADS)
train_apply_kernel(TreeDev t, const uint16_t *__restrict__ leaf_of, const uint8_t *__restrict__ bins, long long rows, double *__restrict__ scores) {
  const long long i = (long long)blockIdx.x * TRAIN_ROW_THREADS + threadIdx.x;
  if (i >= rows) return;
  int leaf;
  if (leaf_of) leaf = leaf_of[i];
  else {
    int n = 0;
    while (n >= 0) {
      const int b = bins[(long long)t.col[n] * rows + i];
      bool left;
      if (CAT && t.is_cat[n]) left = b != TRAIN_NAN_BIN && ((t.cat_mask[n * 8 + (b >> 5)] >> (b & 31)) & 1u);
      else left = b <= t.bin[n] || (b == TRAIN_NAN_BIN && t.nan_left[n]);
      n = left ? t.left[n] : t.right[n];
    }
    leaf = ~n;
  }
  scores[i] = __dadd_rn(scores[i], t.leaf_value[leaf]);
}

// ---- the xgboost backend (train.hpp: the level-wise grower) ----

// step 2x: the cell narrowed to f32 (round to nearest even), its bin the number of bounds <= it
__global__ void __launch_bounds__(TRAIN_BIN_ROWS)
train_bin_f32_kernel(const double *__restrict__ x, int piece_rows, int cols, const double *__restrict__ bounds, const int *__restrict__ bound_off,
                     const int *__restrict__ cat_idx, const uint8_t *__restrict__ cat_tables, uint8_t *__restrict__ bins, long long rows, long long row0) {
  const int i = blockIdx.x * TRAIN_BIN_ROWS + threadIdx.x;
  if (i >= piece_rows) return;
  const double *row = x + (long long)i * cols;
  for (int c = 0; c < cols; ++c) {
    if (cat_idx && cat_idx[2 * c] >= 0) {   // (the same for every lane: a "c" column, step 2cx)
      bins[(long long)c * rows + row0 + i] = (uint8_t)train_xgb_category_bin(row[c], cat_tables + cat_idx[2 * c], cat_idx[2 * c + 1]);
      continue;
    }
    const float v = __double2float_rn(row[c]);
    int a = bound_off[c], b = bound_off[c + 1];
    const int first = a;
    while (a < b) {   // the number of bounds <= v (a bound is an f32 value: the conversion is exact)
      const int m = (a + b) >> 1;
      if ((float)bounds[m] <= v) a = m + 1;
      else b = m;
    }
    bins[(long long)c * rows + row0 + i] = v != v ? (uint8_t)TRAIN_NAN_BIN : (uint8_t)(a - first);
  }
}

__global__ void __launch_bounds__(TRAIN_ROW_THREADS)
train_level_begin_kernel(long long rows, double sampling, int seed, int tree, uint16_t *__restrict__ node_of, uint16_t *__restrict__ hist_slot) {
  const long long i = (long long)blockIdx.x * TRAIN_ROW_THREADS + threadIdx.x;
  if (i >= rows) return;
  node_of[i] = 0;
  hist_slot[i] = train_row_sampled(sampling, seed, tree, (u64)i) ? (uint16_t)0 : (uint16_t)TRAIN_NO_SLOT;
}

// blockIdx: (row tile, column, chunk of built nodes).  A row whose hist_slot lies in the chunk adds (q_g, q_h, 1) to its node's LDS
// histogram of this column; non-empty bins go to memory with integer atomics: every arrangement of tiles gives the same sums
__global__ void __launch_bounds__(TRAIN_ROW_THREADS)
train_level_hist_kernel(const uint8_t *__restrict__ bins, long long rows, const uint16_t *__restrict__ hist_slot, const long long *__restrict__ qg,
                        const long long *__restrict__ qh, const int *__restrict__ build_slot, int n_build, HistDev hd) {
  __shared__ u64 s_g[TRAIN_LEVEL_CHUNK][256], s_h[TRAIN_LEVEL_CHUNK][256];
  __shared__ unsigned s_c[TRAIN_LEVEL_CHUNK][256];
  const int tid = threadIdx.x;
  const int j = blockIdx.y;
  const unsigned chunk = blockIdx.z;
  const int nn = min(TRAIN_LEVEL_CHUNK, n_build - (int)chunk * TRAIN_LEVEL_CHUNK);
  for (int f = 0; f < nn; ++f) {
    s_g[f][tid] = 0;
    s_h[f][tid] = 0;
    s_c[f][tid] = 0;
  }
  const uint8_t *col = bins + (long long)j * rows;
  __syncthreads();
  const long long tile0 = (long long)blockIdx.x * TRAIN_LEVEL_ROWS;
  for (int step = 0; step < TRAIN_LEVEL_ROWS / TRAIN_ROW_THREADS; ++step) {
    const long long row = tile0 + step * TRAIN_ROW_THREADS + tid;
    if (row >= rows) continue;
    const unsigned bs = hist_slot[row];
    if (bs / TRAIN_LEVEL_CHUNK != chunk) continue;   // (TRAIN_NO_SLOT lies in no chunk: n_build <= 32768)
    const int f = (int)(bs % TRAIN_LEVEL_CHUNK);     // (< nn: a slot is below n_build)
    const int b = col[row];
    atomicAdd(&s_g[f][b], (u64)qg[row]);             // (two's complement: the unsigned sum is the signed one)
    atomicAdd(&s_h[f][b], (u64)qh[row]);
    atomicAdd(&s_c[f][b], 1u);
  }
  __syncthreads();
  for (int f = 0; f < nn; ++f) {
    const unsigned c = s_c[f][tid];
    if (c == 0) continue;
    const size_t at = ((size_t)build_slot[chunk * TRAIN_LEVEL_CHUNK + f] * hd.n_sub + (size_t)j) * 256 + tid;
    atomicAdd((u64 *)&hd.G[at], s_g[f][tid]);
    atomicAdd((u64 *)&hd.H[at], s_h[f][tid]);
    atomicAdd(&hd.C[at], c);
  }
}

// blockIdx: (node of the level, column); lane b = bin b.  A node that was not built gets parent - sibling first (its sibling's
// workgroups only read the sibling's slot), then step 5's candidate loop under the caller's admission rule
__global__ void __launch_bounds__(256)
train_level_scan_kernel(HistDev hd, const int *__restrict__ nbins, const int *__restrict__ is_cat, const LevelNode *__restrict__ nodes, ScanParams p,
                        LeafRec *__restrict__ feat_best) {
  __shared__ long long s_buf[2][3][256];
  __shared__ double s_gain[256];
  __shared__ int s_code[256];
  __shared__ long long s_nan[6];   // the NaN bin's sums and the node's totals; step 5cx: the NaN bin's and the "other" bin's
  __shared__ u64 s_mask[4];        // a categorical winner's right bins: one ballot per wavefront
  const int tid = threadIdx.x, j = blockIdx.y;
  const LevelNode nd = nodes[blockIdx.x];
  const size_t at = ((size_t)nd.slot * hd.n_sub + j) * 256 + tid;
  long long g, h, c;
  if (nd.parent_slot >= 0) {
    const size_t ip = ((size_t)nd.parent_slot * hd.n_sub + j) * 256 + tid, is = ((size_t)nd.sibling_slot * hd.n_sub + j) * 256 + tid;
    g = hd.G[ip] - hd.G[is], h = hd.H[ip] - hd.H[is], c = (long long)hd.C[ip] - (long long)hd.C[is];
    hd.G[at] = g, hd.H[at] = h, hd.C[at] = (unsigned)c;
  } else {
    g = hd.G[at], h = hd.H[at], c = hd.C[at];
  }
  LeafRec *out = &feat_best[(size_t)blockIdx.x * hd.n_sub + j];
  if (is_cat[j]) scan_cat_column_xgb(g, h, c, nbins[j], j, p, out, s_buf, s_gain, s_code, s_nan, s_mask);   // (the same for the whole workgroup)
  else scan_column(g, h, c, nbins[j], j, p, out, s_buf, s_gain, s_code, s_nan);
}

// CAT: the level has a categorical record (the host picks the form; the numeric one has no line of step 5cx and reads no mask).  The
// masks of the level's categorical nodes are staged in LDS beside the records when at most TRAIN_LEVEL_LDS_MASKS of them exist - a
// row's word is then one ds_read at (index * 8 + bin / 32) - and read from memory otherwise
template <bool CAT>
__global__ void __launch_bounds__(TRAIN_ROW_THREADS)
train_level_split_kernel(const uint8_t *__restrict__ bins, long long rows, uint16_t *__restrict__ node_of, uint16_t *__restrict__ hist_slot,
                         const LevelRec *__restrict__ recs, int first, int n, double sampling, int seed, int tree, const unsigned *__restrict__ masks,
                         int n_masks) {
  __shared__ LevelRec s_recs[TRAIN_LEVEL_LDS_RECS];
  __shared__ unsigned s_masks[CAT ? TRAIN_LEVEL_LDS_MASKS * 8 : 1];
  const bool in_lds = n <= TRAIN_LEVEL_LDS_RECS;   // (the same for every lane)
  const bool masks_in_lds = CAT && n_masks <= TRAIN_LEVEL_LDS_MASKS;
  if constexpr (CAT) {
    if (masks_in_lds)
      for (int k = threadIdx.x; k < n_masks * 8; k += TRAIN_ROW_THREADS) s_masks[k] = masks[k];
    if (masks_in_lds && !in_lds) __syncthreads();
  }
  if (in_lds) {
    for (int k = threadIdx.x; k < n; k += TRAIN_ROW_THREADS) s_recs[k] = recs[k];
    __syncthreads();
  }
  const long long i = (long long)blockIdx.x * TRAIN_ROW_THREADS + threadIdx.x;
  if (i >= rows) return;
  const unsigned s = (unsigned)node_of[i] - (unsigned)first;
  if (s >= (unsigned)n) return;                    // a row of a finished leaf: its hist_slot is TRAIN_NO_SLOT already
  const LevelRec r = in_lds ? s_recs[s] : recs[s];
  if (r.col < 0) {
    if (hist_slot) hist_slot[i] = (uint16_t)TRAIN_NO_SLOT;
    return;
  }
  bool left;
  if (CAT && (r.col & TRAIN_LEVEL_CAT)) {
    const int b = bins[(long long)(r.col & 0xFFFF) * rows + i];
    const int at = (r.col >> TRAIN_LEVEL_MASK_SHIFT) * 8 + (b >> 5);   // (below n_masks * 8: the host numbered the masks)
    const unsigned word = masks_in_lds ? s_masks[at] : masks[at];
    left = b == TRAIN_NAN_BIN ? r.nan_left != 0 : !((word >> (b & 31)) & 1u);   // (bit 255 is never set; "other", 254, neither: left)
  } else {
    const int b = bins[(long long)r.col * rows + i];
    left = b <= r.bin || (b == TRAIN_NAN_BIN && r.nan_left);
  }
  node_of[i] = (uint16_t)(r.left + (left ? 0 : 1));
  if (hist_slot) {
    const unsigned to = left ? r.slot_l : r.slot_r;
    hist_slot[i] = to != TRAIN_NO_SLOT && train_row_sampled(sampling, seed, tree, (u64)i) ? (uint16_t)to : (uint16_t)TRAIN_NO_SLOT;
  }
}

__global__ void __launch_bounds__(TRAIN_ROW_THREADS)
train_level_apply_kernel(const float *__restrict__ value, const uint16_t *__restrict__ node_of, long long rows, double *__restrict__ scores) {
  const long long i = (long long)blockIdx.x * TRAIN_ROW_THREADS + threadIdx.x;
  if (i >= rows) return;
  scores[i] = (double)__fadd_rn(__double2float_rn(scores[i]), value[node_of[i]]);   // (the score is an f32 value: the narrowing is exact)
}

__global__ void __launch_bounds__(TRAIN_ROW_THREADS)
train_level_base_kernel(long long rows, double *__restrict__ scores) {
  const long long i = (long long)blockIdx.x * TRAIN_ROW_THREADS + threadIdx.x;
  if (i < rows) scores[i] = 0.5;
}

unsigned row_grid(long long rows) { return (unsigned)((rows + TRAIN_ROW_THREADS - 1) / TRAIN_ROW_THREADS); }

}  // namespace

void train_launch_grad_wave(mrk_ctx *ctx, hipStream_t s, const GradDev &d, const int *groups, int count) {
  if (count <= 0) return;
  ScopedKernelTimer timer(ctx, "train_grad");
  hipLaunchKernelGGL(train_grad_wave_kernel, dim3((unsigned)((count + TG_WAVES - 1) / TG_WAVES)), dim3(TG_WAVES * 64), 0, s, d, groups, count);
  MRK_HIP(hipGetLastError());
}

void train_launch_grad_group(mrk_ctx *ctx, hipStream_t s, const GradDev &d, const int *groups, int count, int max_len) {
  if (count <= 0) return;
  ScopedKernelTimer timer(ctx, "train_grad");
  const int threads = max_len <= 512 ? 256 : max_len <= 2048 ? 512 : 1024;   // (eval_launch_group's sizes: a sort stage over 128 pairs keeps 256 lanes busy)
  hipLaunchKernelGGL(train_grad_group_kernel, dim3((unsigned)count), dim3(threads), 0, s, d, groups);
  MRK_HIP(hipGetLastError());
}

void train_launch_grad_wave_bias(mrk_ctx *ctx, hipStream_t s, const GradDev &d, const BiasDev &b, const int *groups, int count) {
  if (count <= 0) return;
  ScopedKernelTimer timer(ctx, "train_grad_bias");
  hipLaunchKernelGGL(train_grad_wave_bias_kernel, dim3((unsigned)((count + TG_WAVES - 1) / TG_WAVES)), dim3(TG_WAVES * 64), 0, s, d, b, groups, count);
  MRK_HIP(hipGetLastError());
}

void train_launch_grad_group_bias(mrk_ctx *ctx, hipStream_t s, const GradDev &d, const BiasDev &b, const int *groups, int count, int max_len) {
  if (count <= 0) return;
  ScopedKernelTimer timer(ctx, "train_grad_bias");
  const int threads = max_len <= 512 ? 256 : max_len <= 2048 ? 512 : 1024;   // (train_launch_grad_group's sizes)
  hipLaunchKernelGGL(train_grad_group_bias_kernel, dim3((unsigned)count), dim3(threads), 0, s, d, b, groups);
  MRK_HIP(hipGetLastError());
}

void train_launch_pos_sum(mrk_ctx *ctx, hipStream_t s, const double *cp, const double *cm, const long long *offsets, long long n_groups, int positions, int e_p,
                          int e_m, long long *Qp, long long *Qm) {
  if (n_groups <= 0) return;
  ScopedKernelTimer timer(ctx, "train_pos_sum");
  // at most 1024 workgroups flush into the same bins; a small set still spreads over several (a run is at least 4 groups, one per wavefront)
  const int run = (int)std::max<long long>(4, (n_groups + 1023) / 1024);
  hipLaunchKernelGGL(train_pos_sum_kernel, dim3((unsigned)((n_groups + run - 1) / run)), dim3(TRAIN_ROW_THREADS), 0, s, cp, cm, offsets, n_groups, run, positions, e_p,
                     e_m, (u64 *)Qp, (u64 *)Qm);
  MRK_HIP(hipGetLastError());
}

void train_launch_bin(mrk_ctx *ctx, hipStream_t s, const double *x, int piece_rows, int cols, const double *bounds, const int *bound_off, const int *cat_idx,
                      const uint8_t *cat_tables, uint8_t *bins, long long rows, long long row0) {
  if (piece_rows <= 0 || cols <= 0) return;
  ScopedKernelTimer timer(ctx, "train_bin");
  hipLaunchKernelGGL(train_bin_kernel, dim3((unsigned)((piece_rows + TRAIN_BIN_ROWS - 1) / TRAIN_BIN_ROWS)), dim3(TRAIN_BIN_ROWS), 0, s, x, piece_rows, cols, bounds,
                     bound_off, cat_idx, cat_tables, bins, rows, row0);
  MRK_HIP(hipGetLastError());
}

void train_launch_max(mrk_ctx *ctx, hipStream_t s, const double *g, const double *h, long long rows, unsigned long long *maxes) {
  ScopedKernelTimer timer(ctx, "train_grad");
  hipLaunchKernelGGL(train_max_kernel, dim3(std::min(row_grid(rows), 1024u)), dim3(TRAIN_ROW_THREADS), 0, s, g, h, rows, maxes);
  MRK_HIP(hipGetLastError());
}

void train_launch_quantise(mrk_ctx *ctx, hipStream_t s, const double *g, const double *h, long long rows, int e_g, int e_h, long long *qg, long long *qh,
                           uint16_t *leaf_of) {
  ScopedKernelTimer timer(ctx, "train_grad");
  hipLaunchKernelGGL(train_quantise_kernel, dim3(row_grid(rows)), dim3(TRAIN_ROW_THREADS), 0, s, g, h, rows, e_g, e_h, qg, qh, leaf_of);
  MRK_HIP(hipGetLastError());
}

void train_launch_hist(mrk_ctx *ctx, hipStream_t s, const uint8_t *bins, long long rows, const uint16_t *leaf_of, int leaf, int slot, const long long *qg,
                       const long long *qh, const int *subset, const HistDev &hd) {
  ScopedKernelTimer timer(ctx, "train_hist");
  const size_t at = (size_t)slot * hd.n_sub * 256;
  MRK_HIP(hipMemsetAsync(hd.G + at, 0, (size_t)hd.n_sub * 256 * 8, s));
  MRK_HIP(hipMemsetAsync(hd.H + at, 0, (size_t)hd.n_sub * 256 * 8, s));
  MRK_HIP(hipMemsetAsync(hd.C + at, 0, (size_t)hd.n_sub * 256 * 4, s));
  const dim3 grid((unsigned)((rows + TRAIN_HIST_ROWS - 1) / TRAIN_HIST_ROWS), (unsigned)((hd.n_sub + TRAIN_HIST_FEATS - 1) / TRAIN_HIST_FEATS));
  hipLaunchKernelGGL(train_hist_kernel, grid, dim3(TRAIN_ROW_THREADS), 0, s, bins, rows, leaf_of, leaf, slot, qg, qh, subset, hd);
  MRK_HIP(hipGetLastError());
}

void train_launch_scan(mrk_ctx *ctx, hipStream_t s, const HistDev &hd, const int *subset, const int *nbins, const int *is_cat, int leaf_a, int leaf_b,
                       bool small_is_left, const ScanParams &p, LeafRec *feat_best, LeafRec *out) {
  ScopedKernelTimer timer(ctx, "train_scan");
  hipLaunchKernelGGL(train_scan_kernel, dim3((unsigned)hd.n_sub), dim3(256), 0, s, hd, subset, nbins, is_cat, leaf_a, leaf_b, small_is_left ? 1 : 0, p, feat_best);
  MRK_HIP(hipGetLastError());
  hipLaunchKernelGGL(train_pick_kernel, dim3(leaf_b >= 0 ? 2u : 1u), dim3(64), 0, s, (const LeafRec *)feat_best, hd.n_sub, out);
  MRK_HIP(hipGetLastError());
}

void train_launch_split(mrk_ctx *ctx, hipStream_t s, const uint8_t *col_bins, long long rows, uint16_t *leaf_of, int leaf, int fresh, int bin, int nan_left) {
  ScopedKernelTimer timer(ctx, "train_apply");
  hipLaunchKernelGGL(train_split_kernel, dim3(row_grid(rows)), dim3(TRAIN_ROW_THREADS), 0, s, col_bins, rows, leaf_of, leaf, fresh, bin, nan_left);
  MRK_HIP(hipGetLastError());
}

void train_launch_split_cat(mrk_ctx *ctx, hipStream_t s, const uint8_t *col_bins, long long rows, uint16_t *leaf_of, int leaf, int fresh, const CatMask &mask) {
  ScopedKernelTimer timer(ctx, "train_apply");
  hipLaunchKernelGGL(train_split_cat_kernel, dim3(row_grid(rows)), dim3(TRAIN_ROW_THREADS), 0, s, col_bins, rows, leaf_of, leaf, fresh, mask);
  MRK_HIP(hipGetLastError());
}

void train_launch_apply(mrk_ctx *ctx, hipStream_t s, const TreeDev &t, const uint16_t *leaf_of, const uint8_t *bins, long long rows, double *scores) {
  if (rows <= 0) return;
  ScopedKernelTimer timer(ctx, "train_apply");
  if (t.is_cat) hipLaunchKernelGGL(train_apply_kernel<true>, dim3(row_grid(rows)), dim3(TRAIN_ROW_THREADS), 0, s, t, leaf_of, bins, rows, scores);
  else hipLaunchKernelGGL(train_apply_kernel<false>, dim3(row_grid(rows)), dim3(TRAIN_ROW_THREADS), 0, s, t, leaf_of, bins, rows, scores);
  MRK_HIP(hipGetLastError());
}

void train_launch_bin_f32(mrk_ctx *ctx, hipStream_t s, const double *x, int piece_rows, int cols, const double *bounds, const int *bound_off, const int *cat_idx,
                          const uint8_t *cat_tables, uint8_t *bins, long long rows, long long row0) {
  if (piece_rows <= 0 || cols <= 0) return;
  ScopedKernelTimer timer(ctx, "train_bin");
  hipLaunchKernelGGL(train_bin_f32_kernel, dim3((unsigned)((piece_rows + TRAIN_BIN_ROWS - 1) / TRAIN_BIN_ROWS)), dim3(TRAIN_BIN_ROWS), 0, s, x, piece_rows, cols, bounds,
                     bound_off, cat_idx, cat_tables, bins, rows, row0);
  MRK_HIP(hipGetLastError());
}

void train_launch_level_begin(mrk_ctx *ctx, hipStream_t s, long long rows, double sampling, int seed, int tree, uint16_t *node_of, uint16_t *hist_slot) {
  ScopedKernelTimer timer(ctx, "train_level_split");
  hipLaunchKernelGGL(train_level_begin_kernel, dim3(row_grid(rows)), dim3(TRAIN_ROW_THREADS), 0, s, rows, sampling, seed, tree, node_of, hist_slot);
  MRK_HIP(hipGetLastError());
}

void train_launch_level_hist(mrk_ctx *ctx, hipStream_t s, const uint8_t *bins, long long rows, const uint16_t *hist_slot, const long long *qg, const long long *qh,
                             const int *build_slot, int n_build, const HistDev &hd) {
  if (n_build <= 0) return;
  ScopedKernelTimer timer(ctx, "train_level_hist");
  const dim3 grid((unsigned)((rows + TRAIN_LEVEL_ROWS - 1) / TRAIN_LEVEL_ROWS), (unsigned)hd.n_sub, (unsigned)((n_build + TRAIN_LEVEL_CHUNK - 1) / TRAIN_LEVEL_CHUNK));
  hipLaunchKernelGGL(train_level_hist_kernel, grid, dim3(TRAIN_ROW_THREADS), 0, s, bins, rows, hist_slot, qg, qh, build_slot, n_build, hd);
  MRK_HIP(hipGetLastError());
}

void train_launch_level_scan(mrk_ctx *ctx, hipStream_t s, const HistDev &hd, const int *nbins, const int *is_cat, const LevelNode *nodes, int n_nodes,
                             const ScanParams &p, LeafRec *feat_best, LeafRec *out) {
  ScopedKernelTimer timer(ctx, "train_level_scan");
  hipLaunchKernelGGL(train_level_scan_kernel, dim3((unsigned)n_nodes, (unsigned)hd.n_sub), dim3(256), 0, s, hd, nbins, is_cat, nodes, p, feat_best);
  MRK_HIP(hipGetLastError());
  hipLaunchKernelGGL(train_pick_kernel, dim3((unsigned)n_nodes), dim3(64), 0, s, (const LeafRec *)feat_best, hd.n_sub, out);
  MRK_HIP(hipGetLastError());
}

void train_launch_level_split(mrk_ctx *ctx, hipStream_t s, const uint8_t *bins, long long rows, uint16_t *node_of, uint16_t *hist_slot, const LevelRec *recs, int first,
                              int n, double sampling, int seed, int tree, const unsigned *masks, int n_masks) {
  if (rows <= 0) return;
  ScopedKernelTimer timer(ctx, "train_level_split");
  if (n_masks > 0)
    hipLaunchKernelGGL(train_level_split_kernel<true>, dim3(row_grid(rows)), dim3(TRAIN_ROW_THREADS), 0, s, bins, rows, node_of, hist_slot, recs, first, n, sampling, seed,
                       tree, masks, n_masks);
  else
    hipLaunchKernelGGL(train_level_split_kernel<false>, dim3(row_grid(rows)), dim3(TRAIN_ROW_THREADS), 0, s, bins, rows, node_of, hist_slot, recs, first, n, sampling, seed,
                       tree, masks, n_masks);
  MRK_HIP(hipGetLastError());
}

void train_launch_level_apply(mrk_ctx *ctx, hipStream_t s, const float *value, const uint16_t *node_of, long long rows, double *scores) {
  if (rows <= 0) return;
  ScopedKernelTimer timer(ctx, "train_apply");
  hipLaunchKernelGGL(train_level_apply_kernel, dim3(row_grid(rows)), dim3(TRAIN_ROW_THREADS), 0, s, value, node_of, rows, scores);
  MRK_HIP(hipGetLastError());
}

void train_launch_level_base(mrk_ctx *ctx, hipStream_t s, long long rows, double *scores) {
  if (rows <= 0) return;
  ScopedKernelTimer timer(ctx, "train_apply");
  hipLaunchKernelGGL(train_level_base_kernel, dim3(row_grid(rows)), dim3(TRAIN_ROW_THREADS), 0, s, rows, scores);
  MRK_HIP(hipGetLastError());
}

}  // namespace mrk
