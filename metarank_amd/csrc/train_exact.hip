// The xgboost backend's EXACT grower on the device (include/mrk.h steps 2e, 5e): split enumeration over sorted columns.
// A workgroup takes TRAIN_EXACT_TILE consecutive positions of ONE column's permutation, a lane four consecutive ones: the lane adds
// its four triples in registers, the wavefront scans the lane sums with shuffles, LDS carries four wavefront totals.  The values and
// node slots of the tile (and of the one position behind it) sit in LDS for the neighbour test.
//   train_exact_cells / _keys / _small_sort   step 2e, once per set: the f32 matrix, a column's sort keys, its order (launch_big_sort above 4096)
//   train_exact_scan<false>   per (tile, column): the tile's total of (q_g, q_h, sampled), the sampled NaN rows per node (an LDS table over
//                             the nodes the tile touches - they are consecutive slots -, flushed with integer atomics) and, where a node
//                             starts inside the tile, the tile-local prefix before it
//   train_exact_offsets       per column: the exclusive prefix over the tile totals; every node's base = its tile's prefix + the local one
//   train_exact_scan<true>    the same tile again: running sum = tile prefix + local prefix - base; a position whose successor is in the
//                             same node, is not NaN and holds another value judges NaN right and - with sampled NaN rows - NaN left.
//                             Per node of the tile: LDS integer max over the gains' bit patterns, then min over the codes of the lanes
//                             that hold that gain, then that one lane writes the record - of the node when it lies inside the tile, of
//                             the tile's edge when it goes on before or behind it
//   train_exact_pick          per node: the best over columns and the tiles it spans (gain, then column, then position, then NaN right)
//   train_exact_route<CAT>    a row pass: (float) x < bound, NaN by nan_left; <true>: a level with a categorical route, its masks over bins in LDS
//   train_exact_cat_bins / _cat_sums / _cat_scan   "c" columns (enable_categorical; steps 2ec, 5ec): a byte per training cell;
//                             per level the sums per (node, bin) from the RUNS of equal categories in the column's order - one atomic triple
//                             per piece of a run inside a tile -, then step 5cx's scan over them (train_scan_device.hpp: train.hip's text)
//   train_exact_parents / _count / _count_offsets / _scatter   the stable partition: per column a prefix count of the rows that went
//                             left, the same prefix-minus-base trick; the left ROW count of a node fixes its children's segments
// Integer sums only, nothing depends on the order anything runs in; every gain is f64, correctly rounded, never fused.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bitonic_device.hpp"
#include "rank_launch.hpp"
#include "runtime.hpp"
#include "sort_device.hpp"
#include "train_exact.hpp"
#include "train_host.hpp"
#include "train_scan_device.hpp"

namespace mrk {

namespace {

typedef unsigned long long u64;

constexpr int EX_THREADS = 256, EX_PER = 4, EX_TILE = TRAIN_EXACT_TILE;
constexpr int EX_ONE_WG = 4096;   // cells ONE workgroup orders (launch_big_sort takes more than that)
static_assert(EX_THREADS * EX_PER == EX_TILE, "a lane takes four consecutive positions of the tile");

__global__ void __launch_bounds__(TRAIN_BIN_ROWS)
train_exact_cells_kernel(const double *__restrict__ x, int piece_rows, int cols, float *__restrict__ cells, long long rows, long long row0) {
  const int i = blockIdx.x * TRAIN_BIN_ROWS + threadIdx.x;
  if (i >= piece_rows) return;
  const double *row = x + (long long)i * cols;
  for (int c = 0; c < cols; ++c) {
    const float v = __double2float_rn(row[c]);
    cells[(long long)c * rows + row0 + i] = v == 0.0f ? 0.0f : v;   // -0.0f and +0.0f are one value
  }
}

__global__ void __launch_bounds__(EX_THREADS)
train_exact_keys_kernel(const float *__restrict__ cells, int n, u64 *__restrict__ keys) {
  const int i = blockIdx.x * EX_THREADS + threadIdx.x;
  if (i < n) keys[i] = asc_key((double)cells[i]);   // (NaN above everything)
}

// n <= EX_ONE_WG (key, row) pairs ordered by one workgroup
__global__ void __launch_bounds__(1024)
train_exact_small_sort_kernel(const u64 *__restrict__ keys, int n, int *__restrict__ order) {
  __shared__ u64 s_key[EX_ONE_WG];
  __shared__ unsigned short s_idx[EX_ONE_WG];
  int p2 = 1;
  while (p2 < n) p2 <<= 1;
  for (int i = threadIdx.x; i < p2; i += 1024) {
    s_key[i] = i < n ? keys[i] : ~0ull;   // (a pad sorts behind every cell: no key is ~0)
    s_idx[i] = (unsigned short)(i < n ? i : 0xffff);
  }
  __syncthreads();
  lds_bitonic<true>(s_key, s_idx, p2);
  for (int i = threadIdx.x; i < n; i += 1024) order[i] = s_idx[i];
}

// (real_of and side_term: train_scan_device.hpp)

// plane[j][row]: the bin of step 2cx of the f32 cell.  blockIdx: (256 rows, "c" column)
__global__ void __launch_bounds__(TRAIN_BIN_ROWS)
train_exact_cat_bins_kernel(const float *__restrict__ cells, long long rows, ExactCat cat, uint8_t *__restrict__ plane) {
  const long long i = (long long)blockIdx.x * TRAIN_BIN_ROWS + threadIdx.x;
  if (i >= rows) return;
  const int j = blockIdx.y, col = cat.cols[j];
  plane[(long long)j * rows + i] = (uint8_t)train_xgb_category_bin((double)cells[(long long)col * rows + i], cat.cat_tables + cat.cat_idx[2 * col], cat.cat_idx[2 * col + 1]);
}

// every lane brings the sum of its own positions and leaves with the sum of the lanes before it; tot: the workgroup's.  One barrier
__device__ __forceinline__ void block_excl_scan3(long long &g, long long &h, long long &c, long long (*s_w)[EX_THREADS / 64], long long *tot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long og = g, oh = h, oc = c;
  for (int d = 1; d < 64; d <<= 1) {
    const long long tg = __shfl_up(g, d, 64), th = __shfl_up(h, d, 64), tc = __shfl_up(c, d, 64);
    if (lane >= d) g += tg, h += th, c += tc;
  }
  if (lane == 63) s_w[0][wave] = g, s_w[1][wave] = h, s_w[2][wave] = c;
  __syncthreads();
  long long bg = 0, bh = 0, bc = 0;
  tot[0] = tot[1] = tot[2] = 0;
  for (int w = 0; w < EX_THREADS / 64; ++w) {
    const long long wg = s_w[0][w], wh = s_w[1][w], wc = s_w[2][w];
    if (w < wave) bg += wg, bh += wh, bc += wc;
    tot[0] += wg, tot[1] += wh, tot[2] += wc;
  }
  g = g - og + bg, h = h - oh + bh, c = c - oc + bc;
}

__device__ __forceinline__ unsigned block_excl_scan1(unsigned v, unsigned *s_w, unsigned *tot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned x = v;
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned t = (unsigned)__shfl_up((int)x, d, 64);
    if (lane >= d) x += t;
  }
  if (lane == 63) s_w[wave] = x;
  __syncthreads();
  unsigned before = 0, all = 0;
  for (int w = 0; w < EX_THREADS / 64; ++w) {
    before += w < wave ? s_w[w] : 0u;
    all += s_w[w];
  }
  *tot = all;
  return x - v + before;
}

// blockIdx: (tile, column).  CAND false: the first pass of a level; true: its candidates.  CATS: the fit has "c" columns (the host picks
// the form: without one the kernels hold no line of step 5ec and are the instructions they were before it)
template <bool CAND, bool CATS>
__global__ void __launch_bounds__(EX_THREADS)
train_exact_scan_kernel(ExactDev d, ExactLevel lv, ScanParams sp, const int *__restrict__ cat_of) {
  if constexpr (CATS)
    if (cat_of[blockIdx.y] >= 0) return;   // a "c" column (the same for the whole workgroup): step 5ec searches it
  __shared__ float s_val[EX_TILE + 1];
  __shared__ int s_k[EX_TILE + 1];          // a position's node slot, -1: none (a finished leaf, or behind the last row)
  __shared__ long long s_w[3][EX_THREADS / 64];
  __shared__ int s_klo, s_any;
  __shared__ u64 s_a[EX_TILE], s_b[EX_TILE];   // per node of the tile, from slot s_klo.  First pass: the NaN rows' q_g and q_h; candidates: s_a the best gain's bits
  __shared__ unsigned s_c[EX_TILE];            // first pass: the NaN rows' count; candidates: the lowest code that holds the best gain
  const int tid = threadIdx.x, tile = blockIdx.x, col = blockIdx.y;
  const long long tile0 = (long long)tile * EX_TILE;
  const float *cells = d.cells + (long long)col * d.rows;
  const int *perm = d.perm + (long long)col * d.rows;
  if (tid == 0) s_klo = 0x7fffffff, s_any = 0;
  for (int j = 0; j < EX_PER; ++j) {
    s_a[tid * EX_PER + j] = 0;
    s_b[tid * EX_PER + j] = 0;
    s_c[tid * EX_PER + j] = CAND ? 0xFFFFFFFFu : 0u;
  }
  __syncthreads();
  long long g[EX_PER], h[EX_PER], c[EX_PER];   // the lane's own triples, then their running sums
  int k[EX_PER];
  float v[EX_PER];
#pragma unroll
  for (int j = 0; j < EX_PER; ++j) {
    const int i = tid * EX_PER + j;
    const long long p = tile0 + i;
    g[j] = 0, h[j] = 0, c[j] = 0, k[j] = -1, v[j] = 0.0f;
    if (p < d.rows) {
      const int row = min(max(perm[p], 0), (int)d.rows - 1);   // (a permutation: the clamp changes nothing and keeps every gather inside)
      const unsigned s = (unsigned)d.node_of[row] - (unsigned)lv.first;
      v[j] = cells[row];
      if (s < (unsigned)lv.n) {
        k[j] = (int)s;
        if (train_row_sampled(d.sampling, d.seed, d.tree, (u64)row)) g[j] = d.qg[row], h[j] = d.qh[row], c[j] = 1;
      }
    }
    s_val[i] = v[j];
    s_k[i] = k[j];
    if (k[j] >= 0) atomicMin(&s_klo, k[j]);
  }
  if (tid == 0) {   // the position behind the tile: the last position's neighbour
    const long long p = tile0 + EX_TILE;
    int nk = -1;
    float nv = 0.0f;
    if (p < d.rows) {
      const int row = min(max(perm[p], 0), (int)d.rows - 1);   // (a permutation: the clamp changes nothing and keeps every gather inside)
      const unsigned s = (unsigned)d.node_of[row] - (unsigned)lv.first;
      nk = s < (unsigned)lv.n ? (int)s : -1;
      nv = cells[row];
    }
    s_val[EX_TILE] = nv;
    s_k[EX_TILE] = nk;
  }
#pragma unroll
  for (int j = 1; j < EX_PER; ++j) g[j] += g[j - 1], h[j] += h[j - 1], c[j] += c[j - 1];
  long long eg = g[EX_PER - 1], eh = h[EX_PER - 1], ec = c[EX_PER - 1], tot[3];
  block_excl_scan3(eg, eh, ec, s_w, tot);   // (its barrier publishes s_klo, s_val and s_k)
  const int klo = s_klo;
  const size_t tile_at = (size_t)col * (size_t)d.n_tiles + (size_t)tile;

  if constexpr (!CAND) {
    if (tid == 0) lv.tile[tile_at] = ExactSums{tot[0], tot[1], tot[2]};
#pragma unroll
    for (int j = 0; j < EX_PER; ++j) {
      if (k[j] < 0) continue;
      const size_t at = (size_t)col * (size_t)lv.cap + (size_t)k[j];
      const long long pg = j ? g[j - 1] : 0, ph = j ? h[j - 1] : 0, pc = j ? c[j - 1] : 0;
      if (tile0 + tid * EX_PER + j == (long long)lv.seg[k[j]].start) lv.base[at] = ExactSums{eg + pg, eh + ph, ec + pc};
      const unsigned kk = (unsigned)(k[j] - klo);
      if (v[j] != v[j] && c[j] != pc && kk < (unsigned)EX_TILE) {   // a sampled NaN row
        atomicAdd(&s_a[kk], (u64)(g[j] - pg));                      // (two's complement: the unsigned sum is the signed one)
        atomicAdd(&s_b[kk], (u64)(h[j] - ph));
        atomicAdd(&s_c[kk], 1u);
        s_any = 1;
      }
    }
    __syncthreads();
    if (!s_any) return;   // (the same for the whole workgroup)
    for (int j = 0; j < EX_PER; ++j) {
      const int i = tid * EX_PER + j;
      const unsigned n_nan = s_c[i];
      if (n_nan == 0 || klo + i >= lv.n) continue;
      ExactSums *to = lv.nan + (size_t)col * (size_t)lv.cap + (size_t)(klo + i);
      atomicAdd((u64 *)&to->g, s_a[i]);
      atomicAdd((u64 *)&to->h, s_b[i]);
      atomicAdd((u64 *)&to->c, (u64)n_nan);
    }
  } else {
    const ExactSums tp = lv.tile[tile_at];   // the sum of the tiles before this one
    double best[EX_PER];
    unsigned code[EX_PER];
    long long bl_g[EX_PER], bl_h[EX_PER], bl_c[EX_PER];
    float bound[EX_PER];
    bool has[EX_PER];
#pragma unroll
    for (int j = 0; j < EX_PER; ++j) {
      has[j] = false, best[j] = 0.0, code[j] = 0u, bl_g[j] = 0, bl_h[j] = 0, bl_c[j] = 0, bound[j] = 0.0f;
      const int i = tid * EX_PER + j;
      const unsigned kk = (unsigned)(k[j] - klo);
      if (k[j] < 0 || v[j] != v[j] || kk >= (unsigned)EX_TILE) continue;
      const float nv = s_val[i + 1];
      if (s_k[i + 1] != k[j] || nv != nv || nv == v[j]) continue;   // the value changes inside the node, between two values
      const size_t at = (size_t)col * (size_t)lv.cap + (size_t)k[j];
      const ExactSums b = lv.base[at], T = lv.tot[k[j]], N = lv.nan[at];
      const long long pg = tp.g + eg + g[j] - b.g, ph = tp.h + eh + h[j] - b.h, pc = tp.c + ec + c[j] - b.c;   // the node's rows up to here
      const double parent = side_term(T.g, T.h, sp);
      for (int nl = 0; nl <= (N.c > 0 ? 1 : 0); ++nl) {
        const long long lg_ = pg + (nl ? N.g : 0), lh = ph + (nl ? N.h : 0), lc = pc + (nl ? N.c : 0);
        const long long rg = T.g - lg_, rh = T.h - lh, rc = T.c - lc;
        const double HL = real_of(lh, sp.e_h), HR = real_of(rh, sp.e_h);
        const double gain = __dsub_rn(__dadd_rn(side_term(lg_, lh, sp), side_term(rg, rh, sp)), parent);
        const bool ok = lc >= sp.min_data && rc >= sp.min_data && HL >= sp.min_hess && HR >= sp.min_hess && gain > sp.min_gain && gain > 0.0;
        if (ok && (!has[j] || gain > best[j])) {   // (NaN to the right wins a tie)
          has[j] = true, best[j] = gain;
          code[j] = (unsigned)((tile0 + i) * 2 + nl);
          bl_g[j] = lg_, bl_h[j] = lh, bl_c[j] = lc;
          bound[j] = nv;
        }
      }
      if (has[j]) atomicMax(&s_a[kk], (u64)__double_as_longlong(best[j]));   // (a gain above 0: the integer order is the order of the values)
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < EX_PER; ++j)
      if (has[j] && s_a[k[j] - klo] == (u64)__double_as_longlong(best[j])) atomicMin(&s_c[k[j] - klo], code[j]);
    __syncthreads();
    const long long tile_end = tile0 + EX_TILE;
#pragma unroll
    for (int j = 0; j < EX_PER; ++j) {
      const int i = tid * EX_PER + j;
      const unsigned kk = (unsigned)(k[j] - klo);
      if (k[j] < 0 || kk >= (unsigned)EX_TILE) continue;
      const bool first_of_piece = i == 0 || s_k[i - 1] != k[j];
      const bool none = s_a[kk] == 0;
      const bool winner = has[j] && s_a[kk] == (u64)__double_as_longlong(best[j]) && s_c[kk] == code[j];
      if (!(winner || (none && first_of_piece))) continue;   // one lane per node piece of the tile writes
      const ExactSeg sg = lv.seg[k[j]];
      ExactCand *to = sg.start < tile0 ? &lv.edge[tile_at * 2] : sg.end > tile_end ? &lv.edge[tile_at * 2 + 1] : &lv.feat[(size_t)k[j] * (size_t)d.cols + (size_t)col];
      *to = ExactCand{best[j], bl_g[j], bl_h[j], bl_c[j], code[j], bound[j], winner ? 1 : 0, 0};
    }
  }
}

// one workgroup per column: vals[0, n) become their exclusive prefix sums; -> the total (every lane)
__device__ __forceinline__ void column_excl_scan3(ExactSums *vals, int n, long long (*s_w)[EX_THREADS / 64], long long *tot) {
  const int tid = threadIdx.x;
  const int chunk = (n + EX_THREADS - 1) / EX_THREADS;
  const int lo = min(tid * chunk, n), hi = min(lo + chunk, n);
  long long g = 0, h = 0, c = 0;
  for (int i = lo; i < hi; ++i) g += vals[i].g, h += vals[i].h, c += vals[i].c;
  block_excl_scan3(g, h, c, s_w, tot);
  for (int i = lo; i < hi; ++i) {
    const ExactSums own = vals[i];
    vals[i] = ExactSums{g, h, c};
    g += own.g, h += own.h, c += own.c;
  }
}

// root: 0, or 1 + the column whose total becomes the root's (the first "q" column)
template <bool CATS>
__global__ void __launch_bounds__(EX_THREADS)
train_exact_offsets_kernel(ExactLevel lv, int n_tiles, int root, const int *__restrict__ cat_of) {
  __shared__ long long s_w[3][EX_THREADS / 64];
  const int col = blockIdx.x;
  if constexpr (CATS)
    if (cat_of[col] >= 0) return;   // (the first pass wrote nothing for a "c" column)
  ExactSums *tile = lv.tile + (size_t)col * (size_t)n_tiles;
  long long tot[3];
  column_excl_scan3(tile, n_tiles, s_w, tot);
  if (col == root - 1 && threadIdx.x == 0) lv.tot[0] = ExactSums{tot[0], tot[1], tot[2]};
  __syncthreads();   // (the prefixes were written by other lanes of this workgroup)
  for (int k = threadIdx.x; k < lv.n; k += EX_THREADS) {
    const ExactSums tp = tile[lv.seg[k].start / EX_TILE];
    ExactSums *b = lv.base + (size_t)col * (size_t)lv.cap + (size_t)k;
    b->g += tp.g, b->h += tp.h, b->c += tp.c;
  }
}

// Step 5ec's sums.  blockIdx: (tile, "c" column).  Ordered by value, the rows of one category are a RUN inside a node's segment, so the
// level's sums per (node, bin) come from the tile's prefix sums and not from the rows one by one: a PIECE is a maximal stretch of equal
// (slot, bin) inside the tile; the lane that holds a piece's last position adds incl[last] - excl[first] to hist[column][slot][bin]
// with three 64-bit integer atomics, where the pieces of a run that straddles tiles meet.  A row outside the tree's sample stays inside
// its piece and adds nothing - it would otherwise cut a run in two wherever it stands -; a piece without a sampled row adds nothing; a
// row of a finished leaf belongs to no piece.  Where a piece began: a max-scan over "my own index where a piece starts here, else -1" -
// lane-local over four positions, shuffles inside the wavefront, four wavefront carries through LDS.  The inclusive prefixes go through
// LDS (3 x 8 B x 1024 = 24 KiB) for the one read at first - 1.  Integer sums: nothing depends on the order the workgroups run in.
__global__ void __launch_bounds__(EX_THREADS)
train_exact_cat_sums_kernel(ExactDev d, ExactLevel lv, ExactCat cat) {
  __shared__ long long s_incl[3][EX_TILE];
  __shared__ int s_key[EX_TILE];               // slot * 256 + bin, -1: no piece
  __shared__ long long s_w[3][EX_THREADS / 64];
  __shared__ int s_first[EX_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x, j = blockIdx.y;
  const long long tile0 = (long long)tile * EX_TILE;
  const int *perm = d.perm + (long long)cat.cols[j] * d.rows;
  const uint8_t *plane = cat.plane + (long long)j * d.rows;
  long long g[EX_PER], h[EX_PER], c[EX_PER];   // the lane's own triples, then their running sums
  int key[EX_PER];
#pragma unroll
  for (int q = 0; q < EX_PER; ++q) {
    const int i = tid * EX_PER + q;
    const long long p = tile0 + i;
    g[q] = 0, h[q] = 0, c[q] = 0, key[q] = -1;
    if (p < d.rows) {
      const int row = min(max(perm[p], 0), (int)d.rows - 1);   // (a permutation: the clamp changes nothing and keeps every gather inside)
      const unsigned s = (unsigned)d.node_of[row] - (unsigned)lv.first;
      if (s < (unsigned)lv.n) {
        key[q] = (int)s * 256 + plane[row];
        if (train_row_sampled(d.sampling, d.seed, d.tree, (u64)row)) g[q] = d.qg[row], h[q] = d.qh[row], c[q] = 1;
      }
    }
    s_key[i] = key[q];
  }
#pragma unroll
  for (int q = 1; q < EX_PER; ++q) g[q] += g[q - 1], h[q] += h[q - 1], c[q] += c[q - 1];
  long long eg = g[EX_PER - 1], eh = h[EX_PER - 1], ec = c[EX_PER - 1], tot[3];
  block_excl_scan3(eg, eh, ec, s_w, tot);   // (its barrier publishes s_key)
  int first[EX_PER], run = -1;               // the latest piece start among the lane's positions up to q, -1: none yet
#pragma unroll
  for (int q = 0; q < EX_PER; ++q) {
    const int i = tid * EX_PER + q;
    s_incl[0][i] = eg + g[q], s_incl[1][i] = eh + h[q], s_incl[2][i] = ec + c[q];
    const int prev = q ? key[q - 1] : tid ? s_key[i - 1] : -2;   // (-2: no key - position 0 starts a piece)
    if (key[q] != prev) run = i;
    first[q] = run;
  }
  int m = run;
  for (int dd = 1; dd < 64; dd <<= 1) {
    const int t = __shfl_up(m, dd, 64);
    if (lane >= dd) m = max(m, t);
  }
  if (lane == 63) s_first[wave] = m;
  int before = __shfl_up(m, 1, 64);   // the latest start among the positions of the lanes before this one
  if (lane == 0) before = -1;
  __syncthreads();   // s_incl, s_first
  for (int w = 0; w < wave; ++w) before = max(before, s_first[w]);
#pragma unroll
  for (int q = 0; q < EX_PER; ++q) {
    const int i = tid * EX_PER + q;
    const int next = q + 1 < EX_PER ? key[q + 1] : i + 1 < EX_TILE ? s_key[i + 1] : -2;
    if (key[q] < 0 || key[q] == next) continue;   // not a piece's last position
    const int f = max(first[q], before);          // (0 <= f <= i: position 0 starts a piece)
    const long long sg = s_incl[0][i] - (f > 0 ? s_incl[0][f - 1] : 0), sh = s_incl[1][i] - (f > 0 ? s_incl[1][f - 1] : 0),
                    sc = s_incl[2][i] - (f > 0 ? s_incl[2][f - 1] : 0);
    if (sc == 0) continue;
    ExactSums *to = cat.hist + ((size_t)j * (size_t)lv.cap + (size_t)(key[q] >> 8)) * 256 + (size_t)(key[q] & 255);
    atomicAdd((u64 *)&to->g, (u64)sg);   // (two's complement: the unsigned sum is the signed one)
    atomicAdd((u64 *)&to->h, (u64)sh);
    atomicAdd((u64 *)&to->c, (u64)sc);
  }
}

// Step 5ec's search.  blockIdx: (slot, "c" column); lane b loads bin b of the level's sums and runs step 5cx's body - the text the
// histogram grower compiles (train_scan_device.hpp) - into a record in LDS; the candidate then goes where the pick reads a column's,
// lv.feat[slot][column] (code: nan_left), its right set into the side table.  root_tot: no "q" column exists - the root's total is this
// scan's (of "c" column 0)
__global__ void __launch_bounds__(256)
train_exact_cat_scan_kernel(ExactLevel lv, ExactCat cat, ScanParams sp, int cols, int root_tot) {
  __shared__ long long s_buf[2][3][256];
  __shared__ double s_gain[256];
  __shared__ int s_code[256];
  __shared__ long long s_nan[6];
  __shared__ u64 s_mask[4];
  __shared__ LeafRec s_rec;
  const int tid = threadIdx.x, k = blockIdx.x, j = blockIdx.y, col = cat.cols[j];
  const ExactSums b = cat.hist[((size_t)j * (size_t)lv.cap + (size_t)k) * 256 + (size_t)tid];
  scan_cat_column_xgb(b.g, b.h, b.c, cat.nbins[col], col, sp, &s_rec, s_buf, s_gain, s_code, s_nan, s_mask);   // (its last barrier publishes s_rec)
  if (tid == 0) {
    lv.feat[(size_t)k * (size_t)cols + (size_t)col] = ExactCand{s_rec.gain, s_rec.gl, s_rec.hl, s_rec.cl, (unsigned)s_rec.nan_left, 0.0f, s_rec.valid, 0};
    if (root_tot && j == 0) lv.tot[0] = ExactSums{s_rec.g, s_rec.h, s_rec.c};
  }
  if (tid < 8) cat.masks[((size_t)k * (size_t)cat.n_cat + (size_t)j) * 8 + (size_t)tid] = s_rec.cat_mask[tid];
}

// one workgroup per node: the best record over the columns and - for a node that spans tiles - over their edge records.
// CATS false: cat_of, masks, n_cat unread
template <bool CATS>
__global__ void __launch_bounds__(EX_THREADS)
train_exact_pick_kernel(ExactLevel lv, int cols, int n_tiles, const int *__restrict__ cat_of, const unsigned *__restrict__ masks, int n_cat) {
  __shared__ double s_gain[EX_THREADS];
  __shared__ int s_col[EX_THREADS];
  __shared__ unsigned s_code[EX_THREADS];
  __shared__ const ExactCand *s_at[EX_THREADS];
  const int tid = threadIdx.x, k = blockIdx.x;
  const ExactSeg sg = lv.seg[k];
  const int t0 = sg.start / EX_TILE, t1 = (sg.end - 1) / EX_TILE, span = t1 - t0 + 1;
  double best = 0.0;
  int bcol = -1;
  unsigned bcode = 0;
  const ExactCand *bat = nullptr;
  for (long long it = tid; it < (long long)cols * span; it += EX_THREADS) {
    const int c = (int)(it / span), t = t0 + (int)(it % span);
    const bool by_runs = CATS && cat_of[c] >= 0;   // a "c" column: ONE record whatever the node spans, never an edge record
    if (by_runs && t != t0) continue;
    const ExactCand *r = span == 1 || by_runs ? &lv.feat[(size_t)k * (size_t)cols + (size_t)c]
                                   : &lv.edge[((size_t)c * (size_t)n_tiles + (size_t)t) * 2 + ((long long)sg.start < (long long)t * EX_TILE ? 0 : 1)];
    if (!r->valid) continue;
    const double gn = r->gain;
    const unsigned cd = r->code;
    if (bcol < 0 || gn > best || (gn == best && (c < bcol || (c == bcol && cd < bcode)))) best = gn, bcol = c, bcode = cd, bat = r;
  }
  s_gain[tid] = best, s_col[tid] = bcol, s_code[tid] = bcode, s_at[tid] = bat;
  __syncthreads();
  if (tid != 0) return;
  for (int l = 1; l < EX_THREADS; ++l) {
    const double gn = s_gain[l];
    const int c = s_col[l];
    if (c >= 0 && (bcol < 0 || gn > best || (gn == best && (c < bcol || (c == bcol && s_code[l] < bcode))))) best = gn, bcol = c, bcode = s_code[l], bat = s_at[l];
  }
  const ExactSums T = lv.tot[k];
  ExactRec out{0.0, 0, 0, 0, T.g, T.h, T.c, 0, 0, 0, 0.0f};
  if (bcol >= 0) out = ExactRec{best, bat->gl, bat->hl, bat->cl, T.g, T.h, T.c, 1, bcol, (int)(bcode & 1u), bat->bound};
  if (CATS && bcol >= 0 && cat_of[bcol] >= 0) {   // the winner's right set rides behind the level's records: still one read-back
    out.valid = EXACT_VALID_CAT;
    const unsigned *from = masks + ((size_t)k * (size_t)n_cat + (size_t)cat_of[bcol]) * 8;
    unsigned *to = (unsigned *)(lv.recs + lv.n) + (size_t)k * 8;
    for (int w = 0; w < 8; ++w) to[w] = from[w];
  }
  lv.recs[k] = out;
}

// CAT: the level has a categorical route (the host picks the form; the numeric one has no line of step 5ec and reads no mask).  As
// train_level_split_kernel: the masks are staged in LDS when at most TRAIN_LEVEL_LDS_MASKS exist - a row's word is one ds_read - and
// read from memory otherwise.  A row's bin comes from its f32 cell and the column's id -> bin table
template <bool CAT>
__global__ void __launch_bounds__(TRAIN_ROW_THREADS)
train_exact_route_kernel(const float *__restrict__ cells, long long rows, uint16_t *__restrict__ node_of, const ExactRoute *__restrict__ routes, int first, int n,
                         const unsigned *__restrict__ masks, int n_masks, const int *__restrict__ cat_idx, const uint8_t *__restrict__ cat_tables) {
  __shared__ ExactRoute s_routes[TRAIN_EXACT_LDS_ROUTES];
  __shared__ unsigned s_masks[CAT ? TRAIN_LEVEL_LDS_MASKS * 8 : 1];
  const bool in_lds = n <= TRAIN_EXACT_LDS_ROUTES;   // (the same for every lane)
  const bool masks_in_lds = CAT && n_masks <= TRAIN_LEVEL_LDS_MASKS;
  if constexpr (CAT) {
    if (masks_in_lds)
      for (int k = threadIdx.x; k < n_masks * 8; k += TRAIN_ROW_THREADS) s_masks[k] = masks[k];
    if (masks_in_lds && !in_lds) __syncthreads();
  }
  if (in_lds) {
    for (int k = threadIdx.x; k < n; k += TRAIN_ROW_THREADS) s_routes[k] = routes[k];
    __syncthreads();
  }
  const long long i = (long long)blockIdx.x * TRAIN_ROW_THREADS + threadIdx.x;
  if (i >= rows) return;
  const unsigned s = (unsigned)node_of[i] - (unsigned)first;
  if (s >= (unsigned)n) return;   // a row of a finished leaf
  const ExactRoute r = in_lds ? s_routes[s] : routes[s];
  if (r.col < 0) return;
  bool left;
  if (CAT && (r.col & TRAIN_LEVEL_CAT)) {
    const int col = r.col & 0xFFFF;
    const int b = train_xgb_category_bin((double)cells[(long long)col * rows + i], cat_tables + cat_idx[2 * col], cat_idx[2 * col + 1]);
    const int at = (r.col >> TRAIN_LEVEL_MASK_SHIFT) * 8 + (b >> 5);   // (below n_masks * 8: the host numbered the masks)
    const unsigned word = masks_in_lds ? s_masks[at] : masks[at];
    left = b == TRAIN_NAN_BIN ? r.nan_left != 0 : !((word >> (b & 31)) & 1u);   // (bit 255 is never set; "other", 254, neither: left)
  } else {
    const float x = cells[(long long)r.col * rows + i];
    left = x != x ? r.nan_left != 0 : x < r.bound;
  }
  node_of[i] = (uint16_t)(r.left + (left ? 0 : 1));
}

// the segment of every node that split, by the index of its pair of children
__global__ void __launch_bounds__(EX_THREADS)
train_exact_parents_kernel(ExactPart pt) {
  const int k = blockIdx.x * EX_THREADS + threadIdx.x;
  if (k >= pt.n || pt.routes[k].col < 0) return;
  const int j = ((int)pt.routes[k].left - pt.next_first) >> 1;
  if (j >= 0 && j < pt.n_next / 2) pt.par[j] = pt.seg[k];
}

// blockIdx: (tile, column).  SCATTER false: the tile's count of rows that went left, the local counts at a parent's first and last
// position; true: every position's place in the next level's order
template <bool SCATTER>
__global__ void __launch_bounds__(EX_THREADS)
train_exact_part_kernel(ExactDev d, ExactPart pt) {
  __shared__ unsigned s_w[EX_THREADS / 64];
  const int tid = threadIdx.x, tile = blockIdx.x, col = blockIdx.y;
  const long long tile0 = (long long)tile * EX_TILE;
  const int *perm = d.perm + (long long)col * d.rows;
  const int half = pt.n_next / 2;
  int row[EX_PER], kc[EX_PER];
  unsigned before[EX_PER], mine = 0;   // rows that went left among the lane's earlier positions
#pragma unroll
  for (int j = 0; j < EX_PER; ++j) {
    const long long p = tile0 + tid * EX_PER + j;
    row[j] = 0, kc[j] = -1, before[j] = mine;
    if (p < d.rows) {
      row[j] = min(max(perm[p], 0), (int)d.rows - 1);
      const unsigned s = (unsigned)d.node_of[row[j]] - (unsigned)pt.next_first;
      if (s < (unsigned)pt.n_next) kc[j] = (int)s;   // the row's node split: an even child slot is the left one
    }
    mine += kc[j] >= 0 && !(kc[j] & 1) ? 1u : 0u;
  }
  unsigned total;
  const unsigned excl = block_excl_scan1(mine, s_w, &total);
  const size_t tile_at = (size_t)col * (size_t)d.n_tiles + (size_t)tile;
  if constexpr (!SCATTER) {
    if (tid == 0) pt.tcount[tile_at] = total;
#pragma unroll
    for (int j = 0; j < EX_PER; ++j) {
      if (kc[j] < 0) continue;
      const long long p = tile0 + tid * EX_PER + j;
      const int jj = kc[j] >> 1;
      const ExactSeg sg = pt.par[jj];
      const unsigned here = excl + before[j];
      if (p == sg.start) pt.lbase[(size_t)col * half + jj] = here;
      if (p == sg.end - 1) pt.lend[(size_t)col * half + jj] = here + (kc[j] & 1 ? 0u : 1u);
    }
  } else {
    const unsigned tp = pt.tcount[tile_at];
    int *out = pt.perm_out + (long long)col * d.rows;
#pragma unroll
    for (int j = 0; j < EX_PER; ++j) {
      const long long p = tile0 + tid * EX_PER + j;
      if (p >= d.rows) continue;
      long long dst = p;
      if (kc[j] >= 0) {
        const int jj = kc[j] >> 1;
        const ExactSeg sg = pt.par[jj];
        const long long in_left = (long long)(tp + excl + before[j]) - (long long)pt.lbase[(size_t)col * half + jj];   // rows of the segment before p that went left
        const long long n_left = pt.lend[(size_t)col * half + jj];
        dst = kc[j] & 1 ? sg.start + n_left + (p - sg.start - in_left) : sg.start + in_left;
        if (dst < sg.start || dst >= sg.end) dst = p;   // (never: a place outside the segment is not written)
      }
      out[dst] = row[j];
    }
  }
}

__global__ void __launch_bounds__(EX_THREADS)
train_exact_count_offsets_kernel(ExactPart pt, int n_tiles) {
  __shared__ unsigned s_w[EX_THREADS / 64];
  const int tid = threadIdx.x, col = blockIdx.x;
  unsigned *tc = pt.tcount + (size_t)col * (size_t)n_tiles;
  const int chunk = (n_tiles + EX_THREADS - 1) / EX_THREADS;
  const int lo = min(tid * chunk, n_tiles), hi = min(lo + chunk, n_tiles);
  unsigned sum = 0, total;
  for (int i = lo; i < hi; ++i) sum += tc[i];
  unsigned run = block_excl_scan1(sum, s_w, &total);
  for (int i = lo; i < hi; ++i) {
    const unsigned own = tc[i];
    tc[i] = run;
    run += own;
  }
  __syncthreads();   // (the prefixes were written by other lanes of this workgroup)
  const int half = pt.n_next / 2;
  for (int jj = tid; jj < half; jj += EX_THREADS) {
    const ExactSeg sg = pt.par[jj];
    const unsigned b = tc[sg.start / EX_TILE] + pt.lbase[(size_t)col * half + jj];
    const unsigned e = tc[(sg.end - 1) / EX_TILE] + pt.lend[(size_t)col * half + jj];
    pt.lbase[(size_t)col * half + jj] = b;
    pt.lend[(size_t)col * half + jj] = e - b;   // the node's left ROW count: the same in every column
    if (col == 0) {
      pt.next_seg[2 * jj] = ExactSeg{sg.start, sg.start + (int)(e - b)};
      pt.next_seg[2 * jj + 1] = ExactSeg{sg.start + (int)(e - b), sg.end};
    }
  }
}

__global__ void train_exact_begin_kernel(long long rows, ExactSeg *seg) { seg[0] = ExactSeg{0, (int)rows}; }

size_t align256(size_t b) { return (b + 255) / 256 * 256; }

}  // namespace

void train_launch_exact_cells(mrk_ctx *ctx, hipStream_t s, const double *x, int piece_rows, int cols, float *cells, long long rows, long long row0) {
  if (piece_rows <= 0 || cols <= 0) return;
  ScopedKernelTimer timer(ctx, "train_bin");
  hipLaunchKernelGGL(train_exact_cells_kernel, dim3((unsigned)((piece_rows + TRAIN_BIN_ROWS - 1) / TRAIN_BIN_ROWS)), dim3(TRAIN_BIN_ROWS), 0, s, x, piece_rows, cols, cells,
                     rows, row0);
  MRK_HIP(hipGetLastError());
}

// [keys n x 8][the sample sort's scratch]
size_t train_exact_order_scratch_bytes(long long n) { return align256((size_t)n * 8) + (n > EX_ONE_WG ? align256(big_sort_scratch_bytes((int)n)) : 0); }

void train_launch_exact_order(mrk_ctx *ctx, hipStream_t s, const float *col_cells, int n, void *scratch, int *order) {
  ScopedKernelTimer timer(ctx, "train_sort");
  u64 *keys = (u64 *)scratch;
  hipLaunchKernelGGL(train_exact_keys_kernel, dim3((unsigned)((n + EX_THREADS - 1) / EX_THREADS)), dim3(EX_THREADS), 0, s, col_cells, n, keys);
  if (n <= EX_ONE_WG) {
    hipLaunchKernelGGL(train_exact_small_sort_kernel, dim3(1), dim3(1024), 0, s, (const u64 *)keys, n, order);
  } else {
    const SortSrc src{nullptr, keys, 1, 0};
    launch_big_sort(ctx, s, src, n, order, (uint8_t *)scratch + align256((size_t)n * 8));
  }
  MRK_HIP(hipGetLastError());
}

void train_launch_exact_cat_bins(mrk_ctx *ctx, hipStream_t s, const float *cells, long long rows, const ExactCat &cat, uint8_t *plane) {
  if (rows <= 0 || cat.n_cat <= 0) return;
  ScopedKernelTimer timer(ctx, "train_bin");
  hipLaunchKernelGGL(train_exact_cat_bins_kernel, dim3((unsigned)((rows + TRAIN_BIN_ROWS - 1) / TRAIN_BIN_ROWS), (unsigned)cat.n_cat), dim3(TRAIN_BIN_ROWS), 0, s, cells, rows,
                     cat, plane);
  MRK_HIP(hipGetLastError());
}

void train_launch_exact_search(mrk_ctx *ctx, hipStream_t s, const ExactDev &d, const ExactLevel &lv, const ScanParams &p, bool root, const ExactCat &cat) {
  const dim3 grid((unsigned)d.n_tiles, (unsigned)d.cols);
  const int *cat_of = cat.cat_of;
  const bool cats = cat.n_cat > 0;
  const bool numeric = cat.n_cat < d.cols;   // (a fit of "c" columns alone launches no numeric search: the root's total is the categorical scan's)
  if (numeric) {
    ScopedKernelTimer timer(ctx, "train_exact_sums");
    hipLaunchKernelGGL((cats ? train_exact_scan_kernel<false, true> : train_exact_scan_kernel<false, false>), grid, dim3(EX_THREADS), 0, s, d, lv, p, cat_of);
    hipLaunchKernelGGL((cats ? train_exact_offsets_kernel<true> : train_exact_offsets_kernel<false>), dim3((unsigned)d.cols), dim3(EX_THREADS), 0, s, lv, d.n_tiles,
                       root ? 1 + (cats ? cat.first_q : 0) : 0, cat_of);
    MRK_HIP(hipGetLastError());
  }
  if (cats) {
    ScopedKernelTimer timer(ctx, "train_exact_cat_sums");
    hipLaunchKernelGGL(train_exact_cat_sums_kernel, dim3((unsigned)d.n_tiles, (unsigned)cat.n_cat), dim3(EX_THREADS), 0, s, d, lv, cat);
    MRK_HIP(hipGetLastError());
  }
  if (cats) {
    ScopedKernelTimer timer(ctx, "train_exact_cat_scan");
    hipLaunchKernelGGL(train_exact_cat_scan_kernel, dim3((unsigned)lv.n, (unsigned)cat.n_cat), dim3(256), 0, s, lv, cat, p, d.cols, root && !numeric ? 1 : 0);
    MRK_HIP(hipGetLastError());
  }
  ScopedKernelTimer timer(ctx, "train_exact_candidates");
  if (numeric) hipLaunchKernelGGL((cats ? train_exact_scan_kernel<true, true> : train_exact_scan_kernel<true, false>), grid, dim3(EX_THREADS), 0, s, d, lv, p, cat_of);
  hipLaunchKernelGGL((cats ? train_exact_pick_kernel<true> : train_exact_pick_kernel<false>), dim3((unsigned)lv.n), dim3(EX_THREADS), 0, s, lv, d.cols, d.n_tiles, cat_of,
                     (const unsigned *)cat.masks, cat.n_cat);
  MRK_HIP(hipGetLastError());
}

void train_launch_exact_route(mrk_ctx *ctx, hipStream_t s, const float *cells, long long rows, uint16_t *node_of, const ExactRoute *routes, int first, int n,
                              const unsigned *masks, int n_masks, const int *cat_idx, const uint8_t *cat_tables) {
  if (rows <= 0) return;
  ScopedKernelTimer timer(ctx, "train_exact_route");
  const dim3 grid((unsigned)((rows + TRAIN_ROW_THREADS - 1) / TRAIN_ROW_THREADS));
  if (n_masks > 0)
    hipLaunchKernelGGL(train_exact_route_kernel<true>, grid, dim3(TRAIN_ROW_THREADS), 0, s, cells, rows, node_of, routes, first, n, masks, n_masks, cat_idx, cat_tables);
  else
    hipLaunchKernelGGL(train_exact_route_kernel<false>, grid, dim3(TRAIN_ROW_THREADS), 0, s, cells, rows, node_of, routes, first, n, masks, n_masks, cat_idx, cat_tables);
  MRK_HIP(hipGetLastError());
}

void train_launch_exact_partition(mrk_ctx *ctx, hipStream_t s, const ExactDev &d, const ExactPart &pt) {
  ScopedKernelTimer timer(ctx, "train_exact_partition");
  const dim3 grid((unsigned)d.n_tiles, (unsigned)d.cols);
  hipLaunchKernelGGL(train_exact_parents_kernel, dim3((unsigned)((pt.n + EX_THREADS - 1) / EX_THREADS)), dim3(EX_THREADS), 0, s, pt);
  hipLaunchKernelGGL(train_exact_part_kernel<false>, grid, dim3(EX_THREADS), 0, s, d, pt);
  hipLaunchKernelGGL(train_exact_count_offsets_kernel, dim3((unsigned)d.cols), dim3(EX_THREADS), 0, s, pt, d.n_tiles);
  hipLaunchKernelGGL(train_exact_part_kernel<true>, grid, dim3(EX_THREADS), 0, s, d, pt);
  MRK_HIP(hipGetLastError());
}

void train_launch_exact_begin(mrk_ctx *ctx, hipStream_t s, long long rows, ExactSeg *seg) {
  ScopedKernelTimer timer(ctx, "train_exact_route");
  hipLaunchKernelGGL(train_exact_begin_kernel, dim3(1), dim3(1), 0, s, rows, seg);
  MRK_HIP(hipGetLastError());
}

}  // namespace mrk
