// Device code that train.hip (the histogram growers' scans) and train_exact.hip (the exact grower's categorical scan, step 5ec) both
// compile: the 256-lane prefix scan over bins, the gain's side term, the workgroup's best candidate and step 5cx's candidate loop over
// the bins of one (node, "c" column).  One text, so that a "c" column is judged by the same instructions under either tree_method.
// Every function expects a workgroup of 256 lanes, lane b holding bin b.
#pragma once
#include <hip/hip_runtime.h>

#include "train.hpp"
#include "train_host.hpp"

namespace mrk {

namespace {

typedef unsigned long long u64;

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

// Step 5cx (backend "xgboost"): lane b holds bin b of one (node, "c" column) - b < nb a kept category, 254 "other", which ALWAYS goes
// left, 255 NaN, which is tried on either side.  A candidate is a set R of kept bins that goes RIGHT (the model's set-membership test:
// member -> right).  nb < TRAIN_XGB_MAX_CAT_TO_ONEHOT: lane b judges R = {b}.  Else the bins with a sampled row and H + lambda > 0,
// ordered ascending by (G / (H + lambda), bin): lane i judges the first i + 1 of them (direction 0) and the last i + 1 (direction 1),
// i < min(TRAIN_XGB_MAX_CAT_THRESHOLD, m), each on its own, under both NaN placements - four candidates a lane.
// Data movement, scan_cat_column's: the order is a counting rank - every lane compares its key with all nb keys, read as LDS
// broadcasts (one address per instruction: no bank conflict) behind ONE barrier; the bins that are not eligible are parked behind the
// eligible ones, and lanes 254 / 255 hand their sums over through s_nan and carry zeros, so ONE block_scan yields every prefix, the
// eligible total (position m - 1) and the kept bins' total (position 255).  The node's total is that plus "other" plus NaN; "other"
// is on the left of every candidate because left = total - right.  The winner's R leaves as four ballots over BINS.
// Ties: the highest gain, then direction 0, then the smaller i (one-vs-rest: the lower bin), then NaN right.
__device__ void scan_cat_column_xgb(long long g, long long h, long long c, int nb, int col, const ScanParams &p, LeafRec *out, long long (*s_buf)[3][256],
                                    double *s_gain, int *s_code, long long *s_nan, u64 *s_mask) {
  const int tid = threadIdx.x;
  const bool onehot = nb < TRAIN_XGB_MAX_CAT_TO_ONEHOT;
  if (tid >= TRAIN_OTHER_BIN) {   // (nb <= 253: neither lane holds a kept bin)
    long long *to = s_nan + (tid == TRAIN_NAN_BIN ? 0 : 3);
    to[0] = g, to[1] = h, to[2] = c;
    g = 0, h = 0, c = 0;
  }
  const long long own_g = g, own_h = h, own_c = c;   // bin b's sums: one-vs-rest's right side
  bool elig = false;
  int pos = tid, m = 0;   // pos: where this lane's bin stands in the order; m: eligible bins
  if (!onehot) {
    const double den = __dadd_rn(real_of(h, p.e_h), p.l2);
    elig = tid < nb && c > 0 && den > 0.0;
    const double key = elig ? __ddiv_rn(real_of(g, p.e_g), den) : 0.0;   // finite, never -0.0
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
  block_scan(pg, ph, pc, s_buf);   // (its first barrier: every lane has read its position; s_nan is published)
  s_buf[0][0][tid] = pg;
  s_buf[0][1][tid] = ph;
  s_buf[0][2][tid] = pc;
  __syncthreads();
  const long long ng = s_nan[0], nh = s_nan[1], nc = s_nan[2];
  const long long Tg = s_buf[0][0][255] + s_nan[3] + ng, Th = s_buf[0][1][255] + s_nan[4] + nh, Tc = s_buf[0][2][255] + s_nan[5] + nc;
  const int n_cand = onehot ? nb : min(TRAIN_XGB_MAX_CAT_THRESHOLD, m);
  double best = 0.0;
  int code = -1;
  long long bl_g = 0, bl_h = 0, bl_c = 0;
  if (tid < n_cand) {
    const double parent = side_term(Tg, Th, p);
    for (int dir = 0; dir <= (onehot ? 0 : 1); ++dir) {
      long long sg, sh, sc;   // R's sums
      if (onehot) sg = own_g, sh = own_h, sc = own_c;
      else if (dir == 0) sg = pg, sh = ph, sc = pc;
      else {   // the last tid + 1 of the m eligible bins: their total minus the first m - 1 - tid
        const int k = m - 2 - tid;
        sg = s_buf[0][0][m - 1] - (k >= 0 ? s_buf[0][0][k] : 0);
        sh = s_buf[0][1][m - 1] - (k >= 0 ? s_buf[0][1][k] : 0);
        sc = s_buf[0][2][m - 1] - (k >= 0 ? s_buf[0][2][k] : 0);
      }
      for (int nl = 0; nl <= (nc > 0 ? 1 : 0); ++nl) {   // NaN right first: it wins a tie
        const long long rg = sg + (nl ? 0 : ng), rh = sh + (nl ? 0 : nh), rc = sc + (nl ? 0 : nc);
        const long long lg_ = Tg - rg, lh = Th - rh, lc = Tc - rc;
        const double HL = real_of(lh, p.e_h), HR = real_of(rh, p.e_h);
        const double gain = __dsub_rn(__dadd_rn(side_term(lg_, lh, p), side_term(rg, rh, p)), parent);
        const bool ok = lc >= p.min_data && rc >= p.min_data && HL >= p.min_hess && HR >= p.min_hess && gain > p.min_gain;
        if (ok && (code < 0 || gain > best)) {   // (the earlier of a lane's four wins a tie: direction 0, then NaN right)
          best = gain;
          code = dir * 512 + tid * 2 + nl;
          bl_g = lg_, bl_h = lh, bl_c = lc;
        }
      }
    }
  }
  const int win = block_best(best, code, s_gain, s_code);   // (the lowest code of the highest gain: direction, then i, then NaN right)
  const int wdir = win >> 9, wi = (win >> 1) & 255;
  if (win >= 0 && tid == wi) s_nan[0] = bl_g, s_nan[1] = bl_h, s_nan[2] = bl_c;   // (every lane read s_nan before block_best's barriers)
  // the winner's right set as a mask over BINS: lane b knows where bin b stands
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
    r.nan_left = win < 0 ? 0 : (win & 1);
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

}  // namespace

}  // namespace mrk
