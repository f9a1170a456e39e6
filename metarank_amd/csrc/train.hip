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
//   train_bin_f32                        the cell narrowed to f32, bin = the number of f32 bounds <= it
//   train_level_begin                    per tree: node_of = 0, hist_slot = 0 for a sampled row, 0xFFFF for the others
//   train_level_hist                     one launch per level, per (row tile, column, chunk of built nodes): LDS histograms of the rows
//                                        whose hist_slot lies in the chunk, non-empty bins flushed with global integer atomics
//   train_level_scan (+ train_pick)      per (node of the level, column): sibling = parent - built child, then scan_column under step
//                                        5x's admission rule; per node the best column; the level's records are read back once
//   train_level_split                    one row pass per level: the level's records in LDS, a row moves to its child and gets the
//                                        child's built slot (0xFFFF when the child is not built or the row is outside the sample)
//   train_level_apply, train_level_base  score = (double) ((float) score + leaf[node_of]); score = 0.5, the base_score
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bitonic_device.hpp"
#include "runtime.hpp"
#include "sort_device.hpp"
#include "train.hpp"
#include "train_host.hpp"
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

// the pairs of the item at rank r: s_key / s_lab in rank order; (g, h) of that item
__device__ __forceinline__ void item_pairs(const GradDev &d, const u64 *s_key, const unsigned char *s_lab, int n, int k, int r, double inv, double &g_out,
                                           double &h_out) {
  const int y = s_lab[r];
  const double sr = -asc_value(s_key[r]);   // sort_key(s) = asc_key(-s)
  const double gr = gain_of(y), ilr = d.invlg[r];
  const int qn = r < k ? n : k;             // a pair counts when min(r, q) < k
  double g = 0.0, h = 0.0;
  for (int q = 0; q < qn; ++q) {
    const int yq = s_lab[q];
    if (yq == y) continue;                  // (q == r too)
    const double sq = -asc_value(s_key[q]);
    const double gq = gain_of(yq), ilq = d.invlg[q];
    const bool hi = y > yq;
    const double delta = hi ? __dsub_rn(sr, sq) : __dsub_rn(sq, sr);
    const double t = fmin(fmax(__dmul_rn(__dsub_rn(delta, d.lo), d.f), 0.0), (double)(TRAIN_SIGMOID_BINS - 1));
    const double rho = d.sigmoid[(int)t];
    const double dg = hi ? __dsub_rn(gr, gq) : __dsub_rn(gq, gr);
    const double dl = fabs(hi ? __dsub_rn(ilr, ilq) : __dsub_rn(ilq, ilr));
    const double w = __dmul_rn(__dmul_rn(dg, dl), inv);
    const double lam = __dmul_rn(__dmul_rn(d.sigma, rho), w);
    const double eta = __dmul_rn(__dmul_rn(__dmul_rn(d.sigma2, rho), __dsub_rn(1.0, rho)), w);
    g = hi ? __dsub_rn(g, lam) : __dadd_rn(g, lam);
    h = __dadd_rn(h, eta);
  }
  g_out = g;
  h_out = h;
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
    double gg, hh;
    item_pairs(d, s_key[wave], s_lab[wave], n, k, rank, s_inv[wave], gg, hh);
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
    double gg, hh;
    item_pairs(d, s_key, s_lab, n, k, r, inv, gg, hh);
    d.g[base + s_idx[r]] = gg;
    d.h[base + s_idx[r]] = hh;
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

// inclusive prefix sums over the 256 lanes' (g, h, c); every lane calls it
__device__ void block_scan(long long &g, long long &h, long long &c, long long (*s_buf)[3][256]) {
  const int tid = threadIdx.x;
  int cur = 0;
  s_buf[0][0][tid] = g;
  s_buf[0][1][tid] = h;
  s_buf[0][2][tid] = c;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    for (int v = 0; v < 3; ++v) s_buf[cur ^ 1][v][tid] = s_buf[cur][v][tid] + (tid >= d ? s_buf[cur][v][tid - d] : 0);
    cur ^= 1;
    __syncthreads();
  }
  g = s_buf[cur][0][tid];
  h = s_buf[cur][1][tid];
  c = s_buf[cur][2][tid];
  __syncthreads();   // (the buffers are written again by the next call)
}

__device__ __forceinline__ double real_of(long long q, int e) { return ldexp((double)q, -e); }   // (the conversion rounds to nearest even)

__device__ __forceinline__ double side_term_l2(long long qg, long long qh, const ScanParams &p, double l2) {
  const double G = real_of(qg, p.e_g), H = real_of(qh, p.e_h);
  return __ddiv_rn(__dmul_rn(G, G), __dadd_rn(H, l2));
}

__device__ __forceinline__ double side_term(long long qg, long long qh, const ScanParams &p) { return side_term_l2(qg, qh, p, p.l2); }

// every lane brings its best candidate (code < 0: none): the code of the workgroup's best - the highest gain, then the lowest code -
// or -1; its gain is left in s_gain[0]
__device__ int block_best(double best, int code, double *s_gain, int *s_code) {
  const int tid = threadIdx.x;
  s_gain[tid] = best;
  s_code[tid] = code;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (tid < d) {
      const double ga = s_gain[tid], gb = s_gain[tid + d];
      const int ca = s_code[tid], cb = s_code[tid + d];
      if (cb >= 0 && (ca < 0 || gb > ga || (gb == ga && cb < ca))) {
        s_gain[tid] = gb;
        s_code[tid] = cb;
      }
    }
    __syncthreads();
  }
  return s_code[0];
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
                     uint8_t *__restrict__ bins, long long rows, long long row0) {
  const int i = blockIdx.x * TRAIN_BIN_ROWS + threadIdx.x;
  if (i >= piece_rows) return;
  const double *row = x + (long long)i * cols;
  for (int c = 0; c < cols; ++c) {
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
train_level_scan_kernel(HistDev hd, const int *__restrict__ nbins, const LevelNode *__restrict__ nodes, ScanParams p, LeafRec *__restrict__ feat_best) {
  __shared__ long long s_buf[2][3][256];
  __shared__ double s_gain[256];
  __shared__ int s_code[256];
  __shared__ long long s_nan[6];
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
  scan_column(g, h, c, nbins[j], j, p, &feat_best[(size_t)blockIdx.x * hd.n_sub + j], s_buf, s_gain, s_code, s_nan);
}

__global__ void __launch_bounds__(TRAIN_ROW_THREADS)
train_level_split_kernel(const uint8_t *__restrict__ bins, long long rows, uint16_t *__restrict__ node_of, uint16_t *__restrict__ hist_slot,
                         const LevelRec *__restrict__ recs, int first, int n, double sampling, int seed, int tree) {
  __shared__ LevelRec s_recs[TRAIN_LEVEL_LDS_RECS];
  const bool in_lds = n <= TRAIN_LEVEL_LDS_RECS;   // (the same for every lane)
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
  const int b = bins[(long long)r.col * rows + i];
  const bool left = b <= r.bin || (b == TRAIN_NAN_BIN && r.nan_left);
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

void train_launch_bin_f32(mrk_ctx *ctx, hipStream_t s, const double *x, int piece_rows, int cols, const double *bounds, const int *bound_off, uint8_t *bins,
                          long long rows, long long row0) {
  if (piece_rows <= 0 || cols <= 0) return;
  ScopedKernelTimer timer(ctx, "train_bin");
  hipLaunchKernelGGL(train_bin_f32_kernel, dim3((unsigned)((piece_rows + TRAIN_BIN_ROWS - 1) / TRAIN_BIN_ROWS)), dim3(TRAIN_BIN_ROWS), 0, s, x, piece_rows, cols, bounds,
                     bound_off, bins, rows, row0);
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

void train_launch_level_scan(mrk_ctx *ctx, hipStream_t s, const HistDev &hd, const int *nbins, const LevelNode *nodes, int n_nodes, const ScanParams &p,
                             LeafRec *feat_best, LeafRec *out) {
  ScopedKernelTimer timer(ctx, "train_level_scan");
  hipLaunchKernelGGL(train_level_scan_kernel, dim3((unsigned)n_nodes, (unsigned)hd.n_sub), dim3(256), 0, s, hd, nbins, nodes, p, feat_best);
  MRK_HIP(hipGetLastError());
  hipLaunchKernelGGL(train_pick_kernel, dim3((unsigned)n_nodes), dim3(64), 0, s, (const LeafRec *)feat_best, hd.n_sub, out);
  MRK_HIP(hipGetLastError());
}

void train_launch_level_split(mrk_ctx *ctx, hipStream_t s, const uint8_t *bins, long long rows, uint16_t *node_of, uint16_t *hist_slot, const LevelRec *recs, int first,
                              int n, double sampling, int seed, int tree) {
  if (rows <= 0) return;
  ScopedKernelTimer timer(ctx, "train_level_split");
  hipLaunchKernelGGL(train_level_split_kernel, dim3(row_grid(rows)), dim3(TRAIN_ROW_THREADS), 0, s, bins, rows, node_of, hist_slot, recs, first, n, sampling, seed, tree);
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
