// Exact similar-items search: POST /recommend's KnnIndexReader.lookup (ml/recommend/embedding/HnswJavaIndex.scala:23-59) as a
// brute-force scan of the embedding table.  The distance is hnswlib-core's DOUBLE_COSINE_DISTANCE,
//   dot = nru = nrv = 0.0;  for i in 0 .. D-1: dot += u[i]*v[i]; nru += u[i]*u[i]; nrv += v[i]*v[i]
//   distance = 1.0 - dot / (sqrt(nru) * sqrt(nrv))
// in f64 with separate multiplies and adds: one lane owns one (query, row) pair and walks i in order, so the bits are the
// JVM's.  No matrix instruction (its accumulation order is not this one).  DESIGN.md section 12.
#include <algorithm>

#include "index_host.hpp"
#include "knn.hpp"
#include "sort_device.hpp"

namespace mrk {

namespace {

constexpr int KNN_THREADS = 256;                       // every kernel here: 4 wavefronts
constexpr int KNN_WAVES = KNN_THREADS / 64;
constexpr unsigned long long KNN_SENT_KEY = ~0ULL;     // above every asc_key (the largest real key is the canonical NaN's)
constexpr int KNN_SENT_ROW = 0x7fffffff;

template <typename T> struct KnnVec;
template <> struct KnnVec<float> { using type = float4; };
template <> struct KnnVec<double> { using type = double2; };
template <typename T> __device__ __forceinline__ double knn_lane(const typename KnnVec<T>::type &v, int k);
template <> __device__ __forceinline__ double knn_lane<float>(const float4 &v, int k) {
  return (double)(k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w);   // widening is exact: both widths give the same bits
}
template <> __device__ __forceinline__ double knn_lane<double>(const double2 &v, int k) { return k == 0 ? v.x : v.y; }

__host__ __device__ __forceinline__ size_t knn_offset(int64_t r, int d, int groups, int G) {
  return ((size_t)(r >> 6) * groups + d / G) * 64 * G + (size_t)(r & 63) * G + d % G;
}

// ---- build

template <typename S, typename T>
__global__ __launch_bounds__(KNN_THREADS) void knn_pack_kernel(const S *__restrict__ src, T *__restrict__ vals, int64_t row0, int64_t n,
                                                                int cols, int groups) {
  const int64_t i = (int64_t)blockIdx.x * KNN_THREADS + threadIdx.x;
  if (i >= n * cols) return;
  const int64_t r = i / cols;
  const int d = (int)(i - r * cols);
  vals[knn_offset(row0 + r, d, groups, 16 / (int)sizeof(T))] = (T)src[i];
}

// The semantic fit (mrk_index_build_texts): mean pooling of the encoder's packed hidden states x [M, H], written as table rows.
// A lane owns one (sequence, group of 4 dimensions): four f64 sums over the sequence's tokens in token order - meanpool_kernel's
// arithmetic (encoder.hip), so a row has the bits mrk_encoder_embed gives - with one 16-byte load per token, and ONE 16-byte
// store, which is exactly one (row, group) element of the blocked layout.  Consecutive lanes are consecutive groups of one
// sequence (a token's H floats are read as consecutive bytes), consecutive sequences are neighbours in the grid, so the 64
// stores that make up a group's 1 KiB line meet in L2.  H is a multiple of 64 (capi_encoder.cpp build_encoder): no tail group.
__global__ __launch_bounds__(KNN_THREADS) void knn_pool_pack_kernel(const float *__restrict__ x, const int32_t *__restrict__ cu,
                                                                     const int64_t *__restrict__ dst_row, int64_t row0, int n, int64_t rows, int H,
                                                                     int groups, float *__restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * KNN_THREADS + threadIdx.x;
  if (i >= (int64_t)n * groups) return;
  const int b = (int)(i / groups), g = (int)(i - (int64_t)b * groups);
  const int64_t r = dst_row ? dst_row[b] : row0 + b;
  if (r < 0 || r >= rows) return;
  const int first = cu[b], cnt = cu[b + 1] - first;
  const float4 *p = (const float4 *)(x + (size_t)first * H) + g;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int j = 0; j < cnt; ++j) {
    const float4 v = p[(size_t)j * groups];
    a0 += (double)v.x;
    a1 += (double)v.y;
    a2 += (double)v.z;
    a3 += (double)v.w;
  }
  const double c = (double)cnt;
  const float4 out = make_float4((float)(a0 / c), (float)(a1 / c), (float)(a2 / c), (float)(a3 / c));
  *(float4 *)(vals + knn_offset(r, g * 4, groups, 4)) = out;
}

// sqrt(nrv) of every row, the sum walked in the order of the spec
template <typename T>
__global__ __launch_bounds__(KNN_THREADS) void knn_norms_kernel(const T *__restrict__ vals, double *__restrict__ snv, int64_t rows, int cols,
                                                                 int groups) {
  constexpr int G = 16 / (int)sizeof(T);
  using Vec = typename KnnVec<T>::type;
  const int64_t r = (int64_t)blockIdx.x * KNN_THREADS + threadIdx.x;
  if (r >= rows) return;
  const Vec *p = (const Vec *)vals + (size_t)(r >> 6) * groups * 64 + (r & 63);
  double nrv = 0.0;
  for (int g = 0; g < groups; ++g) {
    const Vec v = p[(size_t)g * 64];
#pragma unroll
    for (int k = 0; k < G; ++k)
      if (g * G + k < cols) {
        const double x = knn_lane<T>(v, k);
        nrv = __dadd_rn(nrv, __dmul_rn(x, x));
      }
  }
  snv[r] = sqrt(nrv);
}

template <typename T>
__global__ __launch_bounds__(KNN_THREADS) void knn_fetch_kernel(const T *__restrict__ vals, const int64_t *__restrict__ rows, int cols, int groups,
                                                                 double *__restrict__ out) {
  const int64_t r = rows[blockIdx.x];
  for (int d = threadIdx.x; d < cols; d += KNN_THREADS) out[(size_t)blockIdx.x * cols + d] = (double)vals[knn_offset(r, d, groups, 16 / (int)sizeof(T))];
}

// ---- search

// sqrt(nru) of every query
__global__ __launch_bounds__(64) void knn_query_norms_kernel(const double *__restrict__ q, int nq, int cols, double *__restrict__ snu) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= nq) return;
  double nru = 0.0;
  for (int d = 0; d < cols; ++d) {
    const double u = q[(size_t)j * cols + d];
    nru = __dadd_rn(nru, __dmul_rn(u, u));
  }
  snu[j] = sqrt(nru);
}

// One wavefront per block of 64 rows, one lane per row, QT queries per lane: a 16-byte load of the row's next G dimensions
// feeds QT running sums, so QT queries share every byte read from the table.  The queries' values are the same for all lanes:
// they are read through the scalar unit (uniform address, read-only memory).  Each sum is strictly d = 0, 1, ... cols-1 with a
// multiply and an add that are never fused, whatever QT is: a query's bits do not depend on its batch.
// Workgroups of one row range and different query tiles are neighbours in the grid, so they meet in L2.
template <typename T, int QT>
__global__ __launch_bounds__(KNN_THREADS) void knn_scan_kernel(const T *__restrict__ vals, const double *__restrict__ snv, const double *__restrict__ q,
                                                                const double *__restrict__ snu, int nq, int n_tiles, int64_t rows, int cols,
                                                                int groups, int64_t n_blocks, unsigned long long *__restrict__ keys) {
  constexpr int G = 16 / (int)sizeof(T);
  using Vec = typename KnnVec<T>::type;
  const int tile = (int)(blockIdx.x % (unsigned)n_tiles);
  const int64_t b = (int64_t)(blockIdx.x / (unsigned)n_tiles) * KNN_WAVES + (threadIdx.x >> 6);
  if (b >= n_blocks) return;
  const int lane = threadIdx.x & 63;
  const int q0 = tile * QT;
  const Vec *p = (const Vec *)vals + (size_t)b * groups * 64 + lane;
  const double *qp[QT];
  double acc[QT];
#pragma unroll
  for (int j = 0; j < QT; ++j) {
    qp[j] = q + (size_t)min(q0 + j, nq - 1) * cols;   // a tile's unused slots repeat the last query; their sums are dropped
    acc[j] = 0.0;
  }
  const int full = cols / G;
#pragma unroll 4
  for (int g = 0; g < full; ++g) {
    const Vec v = p[(size_t)g * 64];
#pragma unroll
    for (int k = 0; k < G; ++k) {
      const double x = knn_lane<T>(v, k);
#pragma unroll
      for (int j = 0; j < QT; ++j) acc[j] = __dadd_rn(acc[j], __dmul_rn(qp[j][g * G + k], x));
    }
  }
  if (full * G < cols) {   // the last, partly filled group: its padding takes no part (0.0 + -0.0 would already differ)
    const Vec v = p[(size_t)full * 64];
#pragma unroll
    for (int k = 0; k < G - 1; ++k)
      if (full * G + k < cols) {
        const double x = knn_lane<T>(v, k);
#pragma unroll
        for (int j = 0; j < QT; ++j) acc[j] = __dadd_rn(acc[j], __dmul_rn(qp[j][full * G + k], x));
      }
  }
  const int64_t r = b * 64 + lane;
  if (r >= rows) return;
  const double sv = snv[r];
#pragma unroll
  for (int j = 0; j < QT; ++j)
    if (q0 + j < nq) {
      const double dist = 1.0 - acc[j] / __dmul_rn(snu[q0 + j], sv);
      keys[(size_t)(q0 + j) * rows + r] = asc_key(dist);
    }
}

// ---- selection: the n smallest (key, row) pairs

__device__ __forceinline__ void knn_cmpx(unsigned long long *k, int *r, int a, int b, bool asc) {
  const unsigned long long ka = k[a], kb = k[b];
  const int ra = r[a], rb = r[b];
  if (pair_lt(kb, rb, ka, ra) == asc) {
    k[a] = kb; r[a] = rb;
    k[b] = ka; r[b] = ra;
  }
}
// sorts a bitonic sequence of nb pairs ascending (nb a power of two); every thread of the workgroup calls it
__device__ void knn_bitonic_merge(unsigned long long *k, int *r, int nb) {
  for (int j = nb >> 1; j > 0; j >>= 1) {
    for (int t = threadIdx.x; t < (nb >> 1); t += KNN_THREADS) {
      const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
      knn_cmpx(k, r, lo, lo + j, true);
    }
    __syncthreads();
  }
}
__device__ void knn_bitonic_sort(unsigned long long *k, int *r, int nb) {
  for (int size = 2; size <= nb; size <<= 1)
    for (int j = size >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (nb >> 1); t += KNN_THREADS) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        knn_cmpx(k, r, lo, lo + j, (lo & size) == 0);
      }
      __syncthreads();
    }
}

// A workgroup keeps the nb >= n smallest pairs of its segment sorted in LDS (`best`).  An element enters the staging list only
// when it is below the current n-th smallest; when the list is nearly full it is sorted and merged into `best` (bitonic, the
// order rule is sort_device.hpp's pair_lt: key, then row - so ties come out by ascending row) and the bound tightens.  On
// unsorted data a handful of merges serve a whole segment.  The pairs are distinct, so the result does not depend on the
// order the lanes reached the list in.
// in_rows == nullptr: the element's row is its index (first pass over the keys of the scan); else candidates of a first pass.
// out_dist != nullptr: the last pass - writes distances instead of keys.
__global__ __launch_bounds__(KNN_THREADS) void knn_select_kernel(const unsigned long long *__restrict__ in_keys, const int *__restrict__ in_rows,
                                                                  int64_t per_query, int64_t seg, int n, int nb, unsigned long long *__restrict__ out_keys,
                                                                  int *__restrict__ out_rows, double *__restrict__ out_dist) {
  extern __shared__ unsigned long long knn_lds[];
  unsigned long long *bk = knn_lds, *sk = knn_lds + nb;
  int *br = (int *)(knn_lds + 2 * nb), *sr = br + nb;
  __shared__ int cnt;
  __shared__ unsigned long long thr_k;
  __shared__ int thr_r;
  const int tid = threadIdx.x;
  const int64_t lo = (int64_t)blockIdx.x * seg, hi = min(per_query, lo + seg);
  const size_t qbase = (size_t)blockIdx.y * per_query;
  for (int i = tid; i < nb; i += KNN_THREADS) { bk[i] = KNN_SENT_KEY; br[i] = KNN_SENT_ROW; }
  if (tid == 0) { cnt = 0; thr_k = KNN_SENT_KEY; thr_r = KNN_SENT_ROW; }
  __syncthreads();
  for (int64_t base = lo; base < hi; base += KNN_THREADS) {
    const int64_t i = base + tid;
    if (i < hi) {
      const unsigned long long k = in_keys[qbase + i];
      const int r = in_rows ? in_rows[qbase + i] : (int)i;
      if (pair_lt(k, r, thr_k, thr_r)) {
        const int pos = atomicAdd(&cnt, 1);   // < nb: the list is emptied while it still has room for a whole round
        sk[pos] = k;
        sr[pos] = r;
      }
    }
    __syncthreads();
    const int c = cnt;
    __syncthreads();
    if (c > nb - KNN_THREADS || (base + KNN_THREADS >= hi && c > 0)) {
      for (int t = c + tid; t < nb; t += KNN_THREADS) { sk[t] = KNN_SENT_KEY; sr[t] = KNN_SENT_ROW; }
      __syncthreads();
      knn_bitonic_sort(sk, sr, nb);
      for (int t = tid; t < nb; t += KNN_THREADS)   // the nb smallest of both lists, as a bitonic sequence
        if (pair_lt(sk[nb - 1 - t], sr[nb - 1 - t], bk[t], br[t])) { bk[t] = sk[nb - 1 - t]; br[t] = sr[nb - 1 - t]; }
      __syncthreads();
      knn_bitonic_merge(bk, br, nb);
      if (tid == 0) { cnt = 0; thr_k = bk[n - 1]; thr_r = br[n - 1]; }
      __syncthreads();
    }
  }
  const size_t obase = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * n;
  for (int i = tid; i < n; i += KNN_THREADS) {
    out_rows[obase + i] = br[i];
    if (out_dist) out_dist[obase + i] = asc_value(bk[i]);
    else out_keys[obase + i] = bk[i];
  }
}

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace

void knn_table_alloc(KnnTable &t, int64_t rows, int cols, int elem_bytes, hipStream_t stream) {
  const int G = 16 / elem_bytes;
  t.rows = rows;
  t.cols = cols;
  t.elem_bytes = elem_bytes;
  t.n_blocks = ceil_div(rows, 64);
  t.groups = (cols + G - 1) / G;
  t.d_vals.reserve(std::max<size_t>(t.vals_bytes(), 16));
  t.d_snv.reserve(std::max<size_t>((size_t)t.n_blocks * 64 * sizeof(double), 16));
  if (t.vals_bytes()) MRK_HIP(hipMemsetAsync(t.d_vals.p, 0, t.vals_bytes(), stream));
}

void knn_pack(KnnTable &t, const void *d_src, int src_elem_bytes, int64_t row0, int64_t n, hipStream_t stream) {
  if (n <= 0) return;
  const dim3 grid((unsigned)ceil_div(n * t.cols, KNN_THREADS)), block(KNN_THREADS);
  if (t.elem_bytes == 4 && src_elem_bytes == 4)
    hipLaunchKernelGGL((knn_pack_kernel<float, float>), grid, block, 0, stream, (const float *)d_src, t.d_vals.as<float>(), row0, n, t.cols, t.groups);
  else if (t.elem_bytes == 4)
    hipLaunchKernelGGL((knn_pack_kernel<double, float>), grid, block, 0, stream, (const double *)d_src, t.d_vals.as<float>(), row0, n, t.cols, t.groups);
  else
    hipLaunchKernelGGL((knn_pack_kernel<double, double>), grid, block, 0, stream, (const double *)d_src, t.d_vals.as<double>(), row0, n, t.cols, t.groups);
  MRK_HIP(hipGetLastError());
}

void knn_pool_pack(KnnTable &t, const float *d_x, const int32_t *d_cu, const int64_t *d_dst_row, int64_t row0, int n, hipStream_t stream) {
  if (n <= 0) return;
  if (t.elem_bytes != 4 || t.cols % 4 != 0 || (!d_dst_row && (row0 < 0 || row0 + n > t.rows)))
    throw StatusError(MRK_ERR_INVALID_ARG, "knn_pool_pack: launch outside its limits");
  const dim3 grid((unsigned)ceil_div((int64_t)n * t.groups, KNN_THREADS)), block(KNN_THREADS);
  hipLaunchKernelGGL(knn_pool_pack_kernel, grid, block, 0, stream, d_x, d_cu, d_dst_row, row0, n, t.rows, t.cols, t.groups, t.d_vals.as<float>());
  MRK_HIP(hipGetLastError());
}

void knn_norms(KnnTable &t, hipStream_t stream) {
  if (t.rows <= 0) return;
  const dim3 grid((unsigned)ceil_div(t.rows, KNN_THREADS)), block(KNN_THREADS);
  if (t.elem_bytes == 4) hipLaunchKernelGGL(knn_norms_kernel<float>, grid, block, 0, stream, t.d_vals.as<float>(), t.d_snv.as<double>(), t.rows, t.cols, t.groups);
  else hipLaunchKernelGGL(knn_norms_kernel<double>, grid, block, 0, stream, t.d_vals.as<double>(), t.d_snv.as<double>(), t.rows, t.cols, t.groups);
  MRK_HIP(hipGetLastError());
}

void knn_fetch_rows(const KnnTable &t, const int64_t *d_rows, int n, double *d_out, hipStream_t stream) {
  if (n <= 0) return;
  if (t.elem_bytes == 4) hipLaunchKernelGGL(knn_fetch_kernel<float>, dim3(n), dim3(KNN_THREADS), 0, stream, t.d_vals.as<float>(), d_rows, t.cols, t.groups, d_out);
  else hipLaunchKernelGGL(knn_fetch_kernel<double>, dim3(n), dim3(KNN_THREADS), 0, stream, t.d_vals.as<double>(), d_rows, t.cols, t.groups, d_out);
  MRK_HIP(hipGetLastError());
}

int knn_query_chunk(int64_t rows) {
  const int64_t fit = (int64_t(256) << 20) / (std::max<int64_t>(rows, 1) * 8);
  if (fit >= 64) return 64;
  if (fit >= 8) return (int)(fit / 8 * 8);   // whole tiles of 8 queries
  return (int)std::max<int64_t>(fit, 1);
}

template <typename T, int QT>
static void launch_scan(mrk_ctx *ctx, const KnnTable &t, const double *d_q, const double *d_snu, int nq, unsigned long long *d_keys) {
  const int n_tiles = (nq + QT - 1) / QT;
  const int64_t grid = ceil_div(t.n_blocks, KNN_WAVES) * n_tiles;
  hipLaunchKernelGGL((knn_scan_kernel<T, QT>), dim3((unsigned)grid), dim3(KNN_THREADS), 0, ctx->launch, t.d_vals.as<T>(), t.d_snv.as<double>(), d_q, d_snu,
                     nq, n_tiles, t.rows, t.cols, t.groups, t.n_blocks, d_keys);
  MRK_HIP(hipGetLastError());
}

template <typename T>
static void launch_scan_t(mrk_ctx *ctx, const KnnTable &t, const double *d_q, const double *d_snu, int nq, unsigned long long *d_keys) {
  if (nq == 1) launch_scan<T, 1>(ctx, t, d_q, d_snu, nq, d_keys);
  else if (nq <= 4) launch_scan<T, 4>(ctx, t, d_q, d_snu, nq, d_keys);
  else launch_scan<T, 8>(ctx, t, d_q, d_snu, nq, d_keys);
}

void knn_search(mrk_ctx *ctx, const KnnTable &t, KnnScratch &s, const double *d_queries, int nq, int n, int32_t *d_out_rows, double *d_out_dist) {
  if (nq <= 0 || n <= 0 || t.rows <= 0) return;
  if (nq > knn_query_chunk(t.rows) || n > KNN_MAX_N || n > t.rows) throw StatusError(MRK_ERR_INVALID_ARG, "knn_search: launch outside its limits");
  s.keys.reserve((size_t)nq * t.rows * 8);
  s.snu.reserve((size_t)nq * 8);
  hipLaunchKernelGGL(knn_query_norms_kernel, dim3((nq + 63) / 64), dim3(64), 0, ctx->launch, d_queries, nq, t.cols, s.snu.as<double>());
  MRK_HIP(hipGetLastError());
  {
    ScopedKernelTimer timer(ctx, "knn_scan");
    if (t.elem_bytes == 4) launch_scan_t<float>(ctx, t, d_queries, s.snu.as<double>(), nq, s.keys.as<unsigned long long>());
    else launch_scan_t<double>(ctx, t, d_queries, s.snu.as<double>(), nq, s.keys.as<unsigned long long>());
  }
  // selection: up to 256 segments per query, each at least 4 096 rows and 4 x its list, then one workgroup per query over the segments' n best
  int nb = 512;
  while (nb < n) nb <<= 1;
  const int64_t seg = std::max<int64_t>(std::max<int64_t>(4096, 4 * nb), ceil_div(ceil_div(t.rows, 256), KNN_THREADS) * KNN_THREADS);
  const int n_seg = (int)ceil_div(t.rows, seg);
  const size_t lds = (size_t)nb * 2 * (8 + 4);
  ScopedKernelTimer timer(ctx, "knn_select");
  if (n_seg == 1) {
    hipLaunchKernelGGL(knn_select_kernel, dim3(1, nq), dim3(KNN_THREADS), lds, ctx->launch, s.keys.as<unsigned long long>(), (const int *)nullptr, t.rows, seg, n,
                       nb, (unsigned long long *)nullptr, d_out_rows, d_out_dist);
    MRK_HIP(hipGetLastError());
    return;
  }
  const size_t cand = (size_t)nq * n_seg * n;
  s.cand_keys.reserve(cand * 8);
  s.cand_rows.reserve(cand * 4);
  hipLaunchKernelGGL(knn_select_kernel, dim3(n_seg, nq), dim3(KNN_THREADS), lds, ctx->launch, s.keys.as<unsigned long long>(), (const int *)nullptr, t.rows, seg, n,
                     nb, s.cand_keys.as<unsigned long long>(), s.cand_rows.as<int>(), (double *)nullptr);
  MRK_HIP(hipGetLastError());
  const int64_t per_query = (int64_t)n_seg * n;
  hipLaunchKernelGGL(knn_select_kernel, dim3(1, nq), dim3(KNN_THREADS), lds, ctx->launch, s.cand_keys.as<unsigned long long>(), s.cand_rows.as<int>(), per_query,
                     per_query, n, nb, (unsigned long long *)nullptr, d_out_rows, d_out_dist);
  MRK_HIP(hipGetLastError());
}

}  // namespace mrk
