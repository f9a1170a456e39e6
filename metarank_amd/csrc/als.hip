// The eALS iterations of the similar-items fit (mrk_als_fit): the two sweeps and the two K x K products.  DESIGN.md section 17.
// Algorithm: He, Zhang, Kan, Chua, "Fast Matrix Factorization for Online Recommendation with Implicit Feedback", SIGIR 2016,
// Algorithm 1 / Eq. 12-13 - what the reference runs through librec's EALSRecommender
// (ml/recommend/mf/ALSRecImpl.scala:18-41).  All arithmetic is f64, every * + / one IEEE operation (the library is built with
// -ffp-contract=off), no float atomics: tests/als_reference.py restates every sum in the order written here and the factors are
// compared bit for bit.
//
// Order of summation (a function of each sum's length alone):
//   wave sum   - a sum over the L terms of a row (its entries; the K terms over k): 64 partials, partial l = the terms l, l + 64,
//                l + 128, ... added in that order to +0.0; then the fold s = 32, 16, 8, 4, 2, 1: partial[l] = partial[l] +
//                partial[l + s] for l < s; the sum is partial[0].  (Done as a butterfly: every lane adds its partner's value,
//                addition commutes, so all 64 lanes end with partial[0]'s bits.)  The excluded term k = f of the k-sum is +0.0.
//   dot        - r_ui = p_u . q_i: k = 0 .. K-1 in order, added to +0.0.
//   product    - S[f][k]: rows in chunks of ALS_GRAM_CHUNK consecutive rows; a chunk's terms added in row order to +0.0; the chunk
//                sums added in chunk order to +0.0.
#include <algorithm>

#include "als.hpp"

namespace mrk {

namespace {

constexpr int ALS_WAVE = 64;
constexpr int ALS_GRAM_THREADS = 256;
constexpr size_t ALS_STAGE_BYTES = 16 * 1024;      // default LDS budget of a row's staged factor rows
constexpr size_t ALS_SWEEP_LDS_MAX = 60 * 1024;    // ... and what the switch may raise it to
constexpr size_t ALS_GRAM_LDS = 48 * 1024;

inline int padded(int K) { return K | 1; }   // an odd row stride in doubles: lanes reading one column of consecutive staged rows hit 64 banks
inline size_t sweep_lds_bytes(int K, int stage) { return ((size_t)padded(K) + (size_t)stage * (padded(K) + 2)) * sizeof(double); }

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_xor(v, s, ALS_WAVE);
  return v;
}

// One row, one wavefront.  Lane l owns the row's entries l, l + 64, ... (their r and w - c slots are only ever touched by that
// lane) and the factors k = l, l + 64, ... of the row's own vector in LDS.  STAGED: the entries' factor rows, r and w - c live in
// LDS (n <= stage); else the factor rows are gathered from `other` at every step and r lives in d_rhat.
template <bool ITEM, bool STAGED>
__device__ void als_row(int lane, int n, const int32_t *__restrict__ idx, const double *__restrict__ entry_wc, double row_c, double *__restrict__ self_row,
                        const double *__restrict__ other, const double *__restrict__ S, double lambda, int K, int Kp, double *l_own, double *l_q,
                        double *l_r, double *l_w, double *__restrict__ g_r) {
  for (int k = lane; k < K; k += ALS_WAVE) l_own[k] = self_row[k];
  if (STAGED) {
    for (int j = 0; j < n; ++j) {
      const double *src = other + (size_t)idx[j] * K;
      for (int k = lane; k < K; k += ALS_WAVE) l_q[j * Kp + k] = src[k];
    }
    if (!ITEM)
      for (int j = lane; j < n; j += ALS_WAVE) l_w[j] = entry_wc[j];
  }
  __syncthreads();   // (the workgroup is this one wavefront)
  double *r = STAGED ? l_r : g_r;
  for (int j = lane; j < n; j += ALS_WAVE) {
    const double *q = STAGED ? l_q + j * Kp : other + (size_t)idx[j] * K;
    double acc = 0.0;
    for (int k = 0; k < K; ++k) acc = acc + l_own[k] * q[k];
    r[j] = acc;
  }
  const double row_wc = 1.0 - row_c;
  for (int f = 0; f < K; ++f) {
    const double pf = l_own[f];
    const double *Sf = S + (size_t)f * K;
    double num = 0.0, den = 0.0, ks = 0.0;
    for (int j = lane; j < n; j += ALS_WAVE) {
      const double q = STAGED ? l_q[j * Kp + f] : other[(size_t)idx[j] * K + f];
      const double wc = ITEM ? row_wc : (STAGED ? l_w[j] : entry_wc[j]);
      const double rf = r[j] - pf * q;
      r[j] = rf;
      num = num + (1.0 - wc * rf) * q;
      den = den + wc * (q * q);
    }
    for (int k = lane; k < K; k += ALS_WAVE) ks = ks + (k == f ? 0.0 : l_own[k] * Sf[k]);
    num = wave_sum(num);
    den = wave_sum(den);
    ks = wave_sum(ks);
    const double sff = Sf[f];
    const double pnew = ITEM ? (num - row_c * ks) / ((den + row_c * sff) + lambda) : (num - ks) / ((den + sff) + lambda);
    for (int j = lane; j < n; j += ALS_WAVE) {
      const double q = STAGED ? l_q[j * Kp + f] : other[(size_t)idx[j] * K + f];
      r[j] = r[j] + pnew * q;
    }
    if (lane == (f & (ALS_WAVE - 1))) l_own[f] = pnew;   // the lane that reads l_own[f] in the k-sums
  }
  for (int k = lane; k < K; k += ALS_WAVE) self_row[k] = l_own[k];
}

// grid.x = rows, one wavefront each, the longest rows first (d_order): the rows that take longest are under way before the
// many short ones fill the rest of the device
template <bool ITEM>
__global__ __launch_bounds__(ALS_WAVE) void als_sweep_kernel(const int32_t *__restrict__ off, const int32_t *__restrict__ idx_all,
                                                             const int32_t *__restrict__ order, const double *__restrict__ entry_wc_all,
                                                             const double *__restrict__ conf, int64_t rows, double *__restrict__ self,
                                                             const double *__restrict__ other, const double *__restrict__ S, double lambda, int K,
                                                             int stage, double *__restrict__ rhat) {
  extern __shared__ double als_lds[];
  const int Kp = K | 1;
  double *l_own = als_lds, *l_q = l_own + Kp, *l_r = l_q + (size_t)stage * Kp, *l_w = l_r + stage;
  const int64_t b = blockIdx.x;
  if (b >= rows) return;
  const int64_t row = order[b];
  if (row < 0 || row >= rows) return;
  const int lo = off[row], n = off[row + 1] - lo;
  if (n <= 0) return;
  const int lane = threadIdx.x;
  const double row_c = ITEM ? conf[row] : 0.0;
  const double *wc = ITEM ? nullptr : entry_wc_all + lo;
  if (n <= stage) als_row<ITEM, true>(lane, n, idx_all + lo, wc, row_c, self + (size_t)row * K, other, S, lambda, K, Kp, l_own, l_q, l_r, l_w, rhat + lo);
  else als_row<ITEM, false>(lane, n, idx_all + lo, wc, row_c, self + (size_t)row * K, other, S, lambda, K, Kp, l_own, l_q, l_r, l_w, rhat + lo);
}

// One chunk of ALS_GRAM_CHUNK rows per workgroup: the chunk's rows pass through LDS in tiles; a thread owns the outputs
// o = tid, tid + 256, ... (f = o / K, k = o % K: a wavefront reads consecutive k of one or two f) and carries each output's
// running sum from tile to tile in its slot of the chunk's partial.
template <bool WEIGHTED>
__global__ __launch_bounds__(ALS_GRAM_THREADS) void als_gram_chunk_kernel(const double *__restrict__ M, const double *__restrict__ conf, int64_t rows,
                                                                          int K, int tile_rows, double *__restrict__ partial) {
  extern __shared__ double als_lds[];
  double *l_m = als_lds, *l_c = l_m + (size_t)tile_rows * K;
  const int64_t r0 = (int64_t)blockIdx.x * ALS_GRAM_CHUNK, r1 = min(rows, r0 + ALS_GRAM_CHUNK);
  double *out = partial + (size_t)blockIdx.x * K * K;
  const int tid = threadIdx.x;
  for (int64_t t0 = r0; t0 < r1; t0 += tile_rows) {
    const int nt = (int)min((int64_t)tile_rows, r1 - t0);
    __syncthreads();
    for (int e = tid; e < nt * K; e += ALS_GRAM_THREADS) l_m[e] = M[(size_t)t0 * K + e];
    if (WEIGHTED)
      for (int r = tid; r < nt; r += ALS_GRAM_THREADS) l_c[r] = conf[t0 + r];
    __syncthreads();
    for (int o = tid; o < K * K; o += ALS_GRAM_THREADS) {
      const int f = o / K, k = o - f * K;
      double acc = t0 == r0 ? 0.0 : out[o];
      for (int r = 0; r < nt; ++r) {
        const double prod = l_m[r * K + f] * l_m[r * K + k];
        acc = acc + (WEIGHTED ? l_c[r] * prod : prod);
      }
      out[o] = acc;
    }
  }
}

__global__ __launch_bounds__(ALS_GRAM_THREADS) void als_gram_reduce_kernel(const double *__restrict__ partial, int chunks, int KK, double *__restrict__ S) {
  const int o = blockIdx.x * ALS_GRAM_THREADS + threadIdx.x;
  if (o >= KK) return;
  double acc = 0.0;
  for (int c = 0; c < chunks; ++c) acc = acc + partial[(size_t)c * KK + o];
  S[o] = acc;
}

}  // namespace

int als_stage_rows(int K) {
  const size_t per_row = ((size_t)padded(K) + 2) * sizeof(double);
  const int most = (int)((ALS_SWEEP_LDS_MAX - (size_t)padded(K) * sizeof(double)) / per_row);
  const int want = switches().als_stage_max > 0 ? switches().als_stage_max : (int)(ALS_STAGE_BYTES / per_row);
  return std::max(1, std::min(want, most));
}

size_t als_gram_scratch_bytes(int64_t rows, int K) {
  return (size_t)std::max<int64_t>(1, (rows + ALS_GRAM_CHUNK - 1) / ALS_GRAM_CHUNK) * K * K * sizeof(double);
}

void als_launch_gram(mrk_ctx *ctx, hipStream_t s, const char *timer, const double *d_M, const double *d_conf, int64_t rows, int K, double *d_partial,
                     double *d_S) {
  ScopedKernelTimer t(ctx, timer);
  const int chunks = (int)((rows + ALS_GRAM_CHUNK - 1) / ALS_GRAM_CHUNK);
  const int tile_rows = (int)std::min<size_t>(ALS_GRAM_CHUNK, ALS_GRAM_LDS / (((size_t)K + 1) * sizeof(double)));
  const size_t lds = (size_t)tile_rows * (K + 1) * sizeof(double);
  if (chunks > 0) {
    if (d_conf) hipLaunchKernelGGL(als_gram_chunk_kernel<true>, dim3((unsigned)chunks), dim3(ALS_GRAM_THREADS), lds, s, d_M, d_conf, rows, K, tile_rows, d_partial);
    else hipLaunchKernelGGL(als_gram_chunk_kernel<false>, dim3((unsigned)chunks), dim3(ALS_GRAM_THREADS), lds, s, d_M, d_conf, rows, K, tile_rows, d_partial);
    MRK_HIP(hipGetLastError());
  }
  const int KK = K * K;
  hipLaunchKernelGGL(als_gram_reduce_kernel, dim3((unsigned)((KK + ALS_GRAM_THREADS - 1) / ALS_GRAM_THREADS)), dim3(ALS_GRAM_THREADS), 0, s, d_partial, chunks, KK, d_S);
  MRK_HIP(hipGetLastError());
}

void als_launch_sweep(mrk_ctx *ctx, hipStream_t s, bool item_side, const AlsSide &side, double *d_self, const double *d_other, const double *d_S,
                      const double *d_conf, double lambda, int K, double *d_rhat) {
  if (side.rows <= 0) return;
  ScopedKernelTimer t(ctx, item_side ? "als_sweep_items" : "als_sweep_users");
  const int stage = als_stage_rows(K);
  const size_t lds = sweep_lds_bytes(K, stage);
  const dim3 grid((unsigned)side.rows), block(ALS_WAVE);
  if (item_side)
    hipLaunchKernelGGL(als_sweep_kernel<true>, grid, block, lds, s, side.d_off, side.d_idx, side.d_order, side.d_entry_wc, d_conf, side.rows, d_self, d_other, d_S,
                       lambda, K, stage, d_rhat);
  else
    hipLaunchKernelGGL(als_sweep_kernel<false>, grid, block, lds, s, side.d_off, side.d_idx, side.d_order, side.d_entry_wc, d_conf, side.rows, d_self, d_other, d_S,
                       lambda, K, stage, d_rhat);
  MRK_HIP(hipGetLastError());
}

}  // namespace mrk
