// The dense products of an encoder loaded with MRK_ENCODER_SPLIT, on gfx950's bf16 matrix instruction - and, under
// MRK_ENCODER_SPLIT_ATTENTION=1, its attention (attention_split_kernel, further down).
//
// Arithmetic: an f32 operand is a sum of bf16 terms (split_bf16, encoder.hpp: x1 = bf16_rne(x), x2 = bf16_rne(x - x1), ...),
// a product the sum of the leading term products, every one of them v_mfma_f32_32x32x16_bf16 with f32 accumulation:
//     SPLIT_PRODUCTS = 3:  a1 w1  +  (a1 w2 + a2 w1)                      two planes per operand
//     SPLIT_PRODUCTS = 6:  ... + (a2 w2 + a1 w3 + a3 w1)                   three planes
// The weights' planes are made once at load (capi_encoder.cpp), the activations' on the way from global memory (f32) into LDS -
// once per tile and k block, not per MFMA.
//
// THE CANONICAL ORDER.  An output element owns two f32 accumulators that start at 0: C0 takes the first-order product, C1
// every smaller one.  k is walked in ascending steps of 16 (one MFMA's depth); step s adds, in this order,
//     C0 += a1 w1 [16 s .. 16 s + 15];   C1 += a1 w2 [same k];   C1 += a2 w1;   (six products: C1 += a2 w2; += a1 w3; += a3 w1)
// and after the last step the element is (C0 + C1), then bias, then GELU / residual.  The weight rows are the instruction's A
// operand, the token rows its B operand, in every launch.  The tile kernel has ONE body; its launch shapes differ in how
// many 32 x 32 blocks a wavefront owns and in how many wavefronts share the staging, never in an element's chain, and the
// one-request kernel (gemm_split_skinny_kernel) hands the same two accumulators from wavefront to wavefront - so a token's bits
// depend on neither the kernel, nor the tile it fell into, nor the batch it travelled in (tests/test_encoder_split_gpu.py,
// tests/test_encoder_split_skinny_gpu.py).
//
// Tile and LDS: a workgroup of WR x WC wavefronts computes a (32 WR TM) x (32 WC TN) tile.  Per 32-wide k block it stages the
// bf16 planes of its A rows and W rows in LDS as [plane][row][32 + 8]: the 80-byte row stride keeps every 16-byte fragment read
// aligned and spreads eight consecutive rows over distinct banks.  A fragment is 8 consecutive k of one row - lane l reads row
// l & 31 at k = 16 s + 8 (l >> 5) - which is exactly the operand layout of the instruction (encoder.hip's header), so no
// shuffling anywhere.  The next k block's global loads (A as f32, W as bf16 planes, 16 bytes per lane each) are in flight during
// the MFMAs, as in gemm_f32_mfma32_kernel; the split of A happens between the two barriers, from registers.
// The products are computed transposed, as in the f32 kernels: a lane ends up with 4 consecutive output columns of one token.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "encoder.hpp"
#include "launch_shape.hpp"
#include "switches.hpp"

namespace mrk {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef uint32_t uintx2 __attribute__((ext_vector_type(2)));
typedef uint32_t uintx4 __attribute__((ext_vector_type(4)));

constexpr int NP = SPLIT_PLANES;
constexpr int SBK = 32, SLD = SBK + 8;   // k block; LDS row stride in bf16 elements (80 bytes)

// bias, then GELU (libm erf) / residual, of the 4 consecutive columns n4 .. n4 + 3 of row m: what the f32 path fuses
template <int EPI>
__device__ __forceinline__ void store_split_quad(const floatx4 &acc, int m, int n4, int M, int N, const float *__restrict__ bias,
                                                 const float *__restrict__ res, float *__restrict__ out) {
  if (m >= M) return;
  const floatx4 bv = *(const floatx4 *)(bias + n4);
  floatx4 rv = {0.f, 0.f, 0.f, 0.f};
  if (EPI == DENSE_RES) rv = *(const floatx4 *)(res + (size_t)m * N + n4);
  floatx4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float v = acc[e] + bv[e];
    if (EPI == DENSE_GELU) v = 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));
    if (EPI == DENSE_RES) v += rv[e];
    o[e] = v;
  }
  *(floatx4 *)(out + (size_t)m * N + n4) = o;
}

// FOLD: the grid is 8 x (row tiles per XCD) x (column tiles) and one XCD's workgroups walk the column tiles of the same rows of A
// back to back (gemm_f32_mfma_kernel's fold); else blockIdx.x is the column tile of the only row tile.
template <int WR, int WC, int TM, int TN, bool FOLD, int EPI>
__global__ __launch_bounds__(64 * WR * WC, 2) void gemm_split_kernel(const float *__restrict__ A, const uint16_t *__restrict__ W, const float *__restrict__ bias,
                                                                 const float *__restrict__ res, float *__restrict__ out, int M, int N, int K) {
  constexpr int NT = 64 * WR * WC, BM = 32 * WR * TM, BN = 32 * WC * TN;
  constexpr int A_PER = BM * 8 / NT, A_ROWS = NT / 8;   // a k block of A: 8 pieces of 4 floats per row
  constexpr int W_PER = BN * 4 / NT, W_ROWS = NT / 4;   // ... of a W plane: 4 pieces of 8 bf16 per row
  static_assert(BM * 8 % NT == 0 && BN * 4 % NT == 0, "every lane stages whole pieces");
  __shared__ __align__(16) uint16_t As[NP][BM][SLD];
  __shared__ __align__(16) uint16_t Ws[NP][BN][SLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave / WC, wc = wave % WC;
  int m0 = 0, n0 = blockIdx.x * BN;
  if (FOLD) {
    const int n_tiles = N / BN, m_tiles = (M + BM - 1) / BM, per_xcd = (m_tiles + 7) / 8;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int m_tile = xcd * per_xcd + slot / n_tiles;
    if (m_tile >= m_tiles) return;
    m0 = m_tile * BM;
    n0 = (slot % n_tiles) * BN;
  }
  const size_t plane = (size_t)N * K;
  const int ar = tid >> 3, ac = (tid & 7) * 4;   // staging of A: row within a slab of A_ROWS, first of 4 floats
  const int sr = tid >> 2, sc = (tid & 3) * 8;   // staging of W: row within a slab of W_ROWS, first of 8 bf16

  floatx4 ra[A_PER];
  uintx4 rw[NP][W_PER];
  auto load_tiles = [&](int k0) {
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
      int m = m0 + i * A_ROWS + ar;
      m = m < M ? m : M - 1;   // rows past M repeat the last one and are never stored
      ra[i] = *(const floatx4 *)(A + (size_t)m * K + k0 + ac);
    }
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int j = 0; j < W_PER; ++j) rw[p][j] = *(const uintx4 *)(W + p * plane + (size_t)(n0 + j * W_ROWS + sr) * K + k0 + sc);
  };
  auto store_tiles = [&]() {
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
      uint16_t t[4][NP];
#pragma unroll
      for (int e = 0; e < 4; ++e) split_bf16(ra[i][e], t[e]);
#pragma unroll
      for (int p = 0; p < NP; ++p)
        *(uintx2 *)&As[p][i * A_ROWS + ar][ac] = uintx2{(uint32_t)t[0][p] | ((uint32_t)t[1][p] << 16), (uint32_t)t[2][p] | ((uint32_t)t[3][p] << 16)};
    }
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int j = 0; j < W_PER; ++j) *(uintx4 *)&Ws[p][j * W_ROWS + sr][sc] = rw[p][j];
  };

  floatx16 c0[TN][TM], c1[TN][TM];
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) c0[j][i][r] = c1[j][i][r] = 0.f;

  // one term product of the step over the wavefront's blocks: consecutive MFMAs write different accumulators
  auto product = [&](floatx16 (&c)[TN][TM], const bf16x8 (&fw)[TN], const bf16x8 (&fa)[TM]) {
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int i = 0; i < TM; ++i) c[j][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw[j], fa[i], c[j][i], 0, 0, 0);
  };

  const int KT = K / SBK;
  load_tiles(0);
  store_tiles();
  __syncthreads();
  const int fr = lane & 31, fk = (lane >> 5) * 8, fg = (lane >> 5) * 4;
  for (int kt = 0; kt < KT; ++kt) {
    if (kt + 1 < KT) load_tiles((kt + 1) * SBK);
#pragma unroll
    for (int s = 0; s < SBK / 16; ++s) {
      bf16x8 fa[NP][TM], fw[NP][TN];
#pragma unroll
      for (int p = 0; p < NP; ++p) {
#pragma unroll
        for (int i = 0; i < TM; ++i) fa[p][i] = *(const bf16x8 *)&As[p][(wr * TM + i) * 32 + fr][16 * s + fk];
#pragma unroll
        for (int j = 0; j < TN; ++j) fw[p][j] = *(const bf16x8 *)&Ws[p][(wc * TN + j) * 32 + fr][16 * s + fk];
      }
      product(c0, fw[0], fa[0]);     // a1 w1
      product(c1, fw[1], fa[0]);     // a1 w2
      product(c1, fw[0], fa[1]);     // a2 w1
      if constexpr (NP == 3) {
        product(c1, fw[1], fa[1]);   // a2 w2
        product(c1, fw[2], fa[0]);   // a1 w3
        product(c1, fw[0], fa[2]);   // a3 w1
      }
    }
    __syncthreads();
    if (kt + 1 < KT) {
      store_tiles();
      __syncthreads();
    }
  }
  // D[weight row][token]: the lane owns token fr of its block; registers 4 v .. 4 v + 3 are weight rows 8 v + fg .. + 3
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        floatx4 quad;
#pragma unroll
        for (int e = 0; e < 4; ++e) quad[e] = c0[j][i][4 * v + e] + c1[j][i][4 * v + e];
        store_split_quad<EPI>(quad, m0 + (wr * TM + i) * 32 + fr, n0 + (wc * TN + j) * 32 + 8 * v + fg, M, N, bias, res, out);
      }
}

// The same product for M <= 32 rows - ONE request's query on a split handle (mrk_rank with a bi- / cross-encoder field_match), where
// the critical path is what counts.  One workgroup per 32 x 32 block of the output (N / 32 of them); its four wavefronts own a quarter
// of K each (S = K / 64 steps of 16) and continue ONE pair of accumulators in turn, wavefront 0 first, handing C0 and C1 over through
// LDS (8 KB, the kernel's only LDS and barriers) - the chain of gemm_split_kernel, hence its bits.
//
// Nothing is staged: a lane's 16-byte load of a W plane (row l & 31, k 16 s + 8 (l >> 5) .. + 7) IS the instruction's A fragment, and
// its two 16-byte loads of the f32 activations at the same place become the B fragments through split_bf16, in registers.  That split
// is the expensive part (~14 VALU operations per element, 8 elements per lane and step - several times the step's three MFMAs), so
// it is kept off the chain: every wavefront holds two groups of up to SKINNY_G steps in registers, asks for both at once when
// the kernel starts (every wavefront's loads are in flight from the first cycle) and splits them as they arrive, all four wavefronts
// side by side, BEFORE it waits for its turn.  Up to 2 SKINNY_G steps per wavefront (K <= 128 SKINNY_G) the turn itself is MFMAs
// only.  A longer share walks on in groups inside the turn: the next group's loads fly during the MFMAs of the one at hand, its split
// waits on them.  The first group is the ragged one (S - SKINNY_G (groups - 1) steps, wave-uniform guards), every later one is whole.
constexpr int SKINNY_G = NP == 2 ? 8 : 4;

template <int EPI>
__global__ __launch_bounds__(256) void gemm_split_skinny_kernel(const float *__restrict__ A, const uint16_t *__restrict__ W, const float *__restrict__ bias,
                                                                const float *__restrict__ res, float *__restrict__ out, int M, int N, int K) {
  constexpr int G = SKINNY_G;
  __shared__ floatx4 hand[8][64];   // C0 then C1, four registers a row: 16 bytes per lane, conflict-free both ways
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 31, fk = (lane >> 5) * 8, fg = (lane >> 5) * 4;
  const int n0 = blockIdx.x * 32, S = K / 64;
  const int groups = (S + G - 1) / G, first = S - G * (groups - 1);
  const size_t plane = (size_t)N * K;
  const uint16_t *wrow = W + (size_t)(n0 + fr) * K + wave * S * 16 + fk;
  const float *arow = A + (size_t)(fr < M ? fr : M - 1) * K + wave * S * 16 + fk;   // rows past M repeat the last one and are never stored

  // steps s0 .. s0 + n - 1 of the wavefront's share: W fragments as they are, A as f32
  auto fetch = [&](uintx4 (&fw)[G][NP], floatx4 (&ra)[G][2], int s0, int n) {
#pragma unroll
    for (int t = 0; t < G; ++t)
      if (t < n) {
#pragma unroll
        for (int p = 0; p < NP; ++p) fw[t][p] = *(const uintx4 *)(wrow + p * plane + 16 * (s0 + t));
        ra[t][0] = *(const floatx4 *)(arow + 16 * (s0 + t));
        ra[t][1] = *(const floatx4 *)(arow + 16 * (s0 + t) + 4);
      }
  };
  // ... A's 8 consecutive k of a step into the bf16 fragment of every plane (element e in bits 16 (e & 1) of word e / 2)
  auto split = [&](const floatx4 (&ra)[G][2], uintx4 (&fa)[G][NP], int n) {
#pragma unroll
    for (int t = 0; t < G; ++t)
      if (t < n) {
        uint16_t b[8][NP];
#pragma unroll
        for (int e = 0; e < 8; ++e) split_bf16(ra[t][e >> 2][e & 3], b[e]);
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
          for (int q = 0; q < 4; ++q) fa[t][p][q] = (uint32_t)b[2 * q][p] | ((uint32_t)b[2 * q + 1][p] << 16);
      }
  };
  floatx16 c0, c1;
#pragma unroll
  for (int r = 0; r < 16; ++r) c0[r] = c1[r] = 0.f;
  // ... and their term products in the canonical order
  auto steps = [&](const uintx4 (&fw)[G][NP], const uintx4 (&fa)[G][NP], int n) {
#pragma unroll
    for (int t = 0; t < G; ++t)
      if (t < n) {
        bf16x8 w[NP], a[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          w[p] = __builtin_bit_cast(bf16x8, fw[t][p]);
          a[p] = __builtin_bit_cast(bf16x8, fa[t][p]);
        }
        c0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0], a[0], c0, 0, 0, 0);     // a1 w1
        c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[1], a[0], c1, 0, 0, 0);     // a1 w2
        c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0], a[1], c1, 0, 0, 0);     // a2 w1
        if constexpr (NP == 3) {
          c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[1], a[1], c1, 0, 0, 0);   // a2 w2
          c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[2], a[0], c1, 0, 0, 0);   // a1 w3
          c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0], a[2], c1, 0, 0, 0);   // a3 w1
        }
      }
  };

  uintx4 w0[G][NP], w1[G][NP], a0[G][NP], a1[G][NP];   // group 0, 2, 4 ... lives in w0 / a0, group 1, 3, ... in w1 / a1
  floatx4 r0[G][2], r1[G][2];
  fetch(w0, r0, 0, first);
  if (groups > 1) fetch(w1, r1, first, G);
  split(r0, a0, first);
  if (groups > 1) split(r1, a1, G);
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
      if (w > 0) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const floatx4 h0 = hand[v][lane], h1 = hand[4 + v][lane];
#pragma unroll
          for (int e = 0; e < 4; ++e) { c0[4 * v + e] = h0[e]; c1[4 * v + e] = h1[e]; }
        }
      }
      steps(w0, a0, first);
      for (int g = 1; g < groups; g += 2) {   // group g from w1 / a1, then group g + 1 from w0 / a0
        if (g + 1 < groups) fetch(w0, r0, first + G * g, G);
        steps(w1, a1, G);
        if (g + 1 < groups) {
          split(r0, a0, G);
          if (g + 2 < groups) fetch(w1, r1, first + G * (g + 1), G);
          steps(w0, a0, G);
          if (g + 2 < groups) split(r1, a1, G);
        }
      }
      if (w < 3) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          hand[v][lane] = floatx4{c0[4 * v], c0[4 * v + 1], c0[4 * v + 2], c0[4 * v + 3]};
          hand[4 + v][lane] = floatx4{c1[4 * v], c1[4 * v + 1], c1[4 * v + 2], c1[4 * v + 3]};
        }
      }
    }
    if (w < 3) __syncthreads();
  }
  if (wave != 3) return;
  // D[weight row][token], as in gemm_split_kernel: the lane owns token fr; registers 4 v .. 4 v + 3 are weight rows 8 v + fg .. + 3
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    floatx4 quad;
#pragma unroll
    for (int e = 0; e < 4; ++e) quad[e] = c0[4 * v + e] + c1[4 * v + e];
    store_split_quad<EPI>(quad, fr, n0 + 8 * v + fg, M, N, bias, res, out);
  }
}

// split_launch_plan (launch_shape.hpp) decides, nothing here does
template <int EPI>
void launch_gemm_split(const float *A, const uint16_t *W, const float *bias, const float *res, float *out, int M, int N, int K, hipStream_t s) {
  const SplitPlan p = split_launch_plan(M, N, K, switches().encoder_split_skinny);
  const dim3 grid(p.workgroups), block(p.threads);
  switch (p.kernel) {
    case SPLIT_SKINNY: hipLaunchKernelGGL((gemm_split_skinny_kernel<EPI>), grid, block, 0, s, A, W, bias, res, out, M, N, K); break;
    case SPLIT_TILE_32x64: hipLaunchKernelGGL((gemm_split_kernel<1, 2, 1, 1, false, EPI>), grid, block, 0, s, A, W, bias, res, out, M, N, K); break;
    case SPLIT_TILE_64: hipLaunchKernelGGL((gemm_split_kernel<2, 2, 1, 1, true, EPI>), grid, block, 0, s, A, W, bias, res, out, M, N, K); break;
    case SPLIT_TILE_128: hipLaunchKernelGGL((gemm_split_kernel<2, 2, 2, 2, true, EPI>), grid, block, 0, s, A, W, bias, res, out, M, N, K); break;
  }
}

// ---- attention of a split handle (MRK_ENCODER_SPLIT_ATTENTION=1): S = scale Q K^T and O = softmax(S + mask) V as split products.
//
// Where K and V are split: ONCE per layer, by split_kv_kernel, into bf16 planes in global memory ([plane][token][K of all heads | V of
// all heads], EncoderScratch::kv) - every query block of a sequence reads the same K / V rows, and a wavefront that split them in its
// own registers would spend ~14 VALU operations an element on each of them again (S / 32 times per row).  One head per wavefront means
// the wavefronts of a workgroup share no K / V, so LDS planes would be shared by nobody; the planes in memory are shared by every query
// block, and the attention kernel needs neither LDS nor a barrier.  Q is split once per wavefront in registers, P once per key block.
//
// The kernel: one wavefront per (32 queries, head, sequence), ATT_HEADS wavefronts (heads) per workgroup, as attention_kernel /
// attention_f32_mfma_kernel.  Scores are computed transposed, S^T = K Q^T: K rows are the instruction's A operand (a lane's 16-byte
// load of a K plane - key l & 31, d 16 t + 8 (l >> 5) .. + 7 - IS the fragment), the query's Q terms the B operand, the contraction
// walks the head dimension in DH / 16 steps.  A lane then owns query column l & 31 and 16 of the block's 32 keys (register 4 v + e =
// key 8 v + 4 (l >> 5) + e): the softmax is a per-lane reduction plus one exchange with lane ^ 32, f32 with libm expf, running maximum
// and sum over key blocks of 32, and registers 8 c .. 8 c + 7, split, are the B fragment of step c of O^T = V^T P^T - k slot j of that
// step stands for key 16 c + 8 (j >> 2) + 4 (l >> 5) + (j & 3) on both operands, so step c covers exactly keys 16 c .. 16 c + 15 of the block
// and the contraction ascends in steps of 16 keys.  V^T's fragment (row d = l & 31, those 8 keys) is gathered from the V planes with
// eight 2-byte loads: 32 consecutive lanes read 64 consecutive bytes of one key's row.
//
// Canonical order, both products, a = the query side (Q, P), b = the key side (K, V): C0 += a1 b1, C1 += a1 b2, C1 += a2 b1 per step,
// two accumulators from +0.  S^T = scale (C0 + C1) per key block; O keeps its C0 and C1 across key blocks, both rescaled by the running
// maximum's exp(m_old - m_new) as attention_f32_mfma_kernel rescales its one, and ends as (C0 + C1) / l.
//
// What a (sequence, head, query)'s bits depend on: its own sequence.  Key blocks start at the sequence's first token, in the padded
// and the packed form alike; a key past the sequence's end or with mask 0 gets probability +0 in both planes, i.e. +0 terms into
// accumulators that hold +0 or a sum; a block without a live key (the sequence's own mask decides, uniformly over the wavefront)
// leaves the state untouched; a live block always runs both of its 16-key steps.  A query column never meets another column's data.
// The next key block's K fragments are loaded before the softmax of the block at hand and fly under it; the V gathers of a step are
// issued before the split of its probabilities.
__global__ __launch_bounds__(256) void split_kv_kernel(const float *__restrict__ qkv, uint16_t *__restrict__ kv, int M, int H) {
  const int per_row = 2 * H / 8;   // pieces of 8 consecutive elements of a token's [K | V]
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)M * per_row) return;
  const size_t m = i / per_row;
  const int j = (int)(i % per_row) * 8;
  const float *src = qkv + m * 3 * H + H + j;
  const floatx4 lo = *(const floatx4 *)src, hi = *(const floatx4 *)(src + 4);
  uint16_t t[8][NP];
#pragma unroll
  for (int e = 0; e < 8; ++e) split_bf16(e < 4 ? lo[e] : hi[e - 4], t[e]);
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    uintx4 w;
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] = (uint32_t)t[2 * q][p] | ((uint32_t)t[2 * q + 1][p] << 16);
    *(uintx4 *)(kv + ((size_t)p * M + m) * 2 * H + j) = w;
  }
}

// 8 f32 values as the bf16 fragment of every plane (element e in bits 16 (e & 1) of word e / 2)
__device__ __forceinline__ void split_fragment(const float (&x)[8], bf16x8 (&f)[NP]) {
  uint16_t t[8][NP];
#pragma unroll
  for (int e = 0; e < 8; ++e) split_bf16(x[e], t[e]);
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    uintx4 w;
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] = (uint32_t)t[2 * q][p] | ((uint32_t)t[2 * q + 1][p] << 16);
    f[p] = __builtin_bit_cast(bf16x8, w);
  }
}

// one step of the canonical order: a = the query side (B operand), b = the key side (A operand)
__device__ __forceinline__ void split_step(floatx16 &c0, floatx16 &c1, const bf16x8 (&b)[NP], const bf16x8 (&a)[NP]) {
  c0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b[0], a[0], c0, 0, 0, 0);     // a1 b1
  c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b[1], a[0], c1, 0, 0, 0);     // a1 b2
  c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b[0], a[1], c1, 0, 0, 0);     // a2 b1
  if constexpr (NP == 3) {
    c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b[1], a[1], c1, 0, 0, 0);   // a2 b2
    c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b[2], a[0], c1, 0, 0, 0);   // a1 b3
    c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b[0], a[2], c1, 0, 0, 0);   // a3 b1
  }
}

template <int DH>
__global__ __launch_bounds__(64 * ATT_HEADS, 2) void attention_split_kernel(const float *__restrict__ qkv, const uint16_t *__restrict__ kv,
                                                                        const int32_t *__restrict__ mask, const int32_t *__restrict__ cu, int seq_pad,
                                                                        int M, int H, int heads, float scale, float *__restrict__ ctx) {
  constexpr int KS = DH / 16, DB = DH / 32;   // steps of S^T's contraction; 32-row blocks of O^T
  const int lane = threadIdx.x & 63, c = lane & 31, g = lane >> 5;
  const int q0 = blockIdx.x * 32, head = blockIdx.y * ATT_HEADS + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), b = blockIdx.z;
  if (head >= heads) return;
  const size_t first = cu ? (size_t)cu[b] : (size_t)b * seq_pad;
  const int seq = cu ? cu[b + 1] - cu[b] : seq_pad;
  if (q0 >= seq) return;   // (packed: the grid covers the longest sequence)
  const int32_t *mrow = mask ? mask + first : nullptr;
  // wavefront-uniform bases (scalar registers) and 32-bit lane offsets from them: a key's row lies < max_pos x 2 H elements past `first`
  const uint32_t kvrow = 2u * H;
  const size_t plane = (size_t)M * kvrow;
  const uint16_t *kbase[NP], *vbase[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    kbase[p] = kv + p * plane + first * kvrow + head * DH;
    vbase[p] = kbase[p] + H;
  }

  bf16x8 qf[KS][NP];
  {
    const int qi = q0 + c < seq ? q0 + c : seq - 1;   // rows past the sequence repeat its last one and are never stored
    const float *q = qkv + (first + qi) * 3 * H + head * DH + 8 * g;
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      const floatx4 lo = *(const floatx4 *)(q + 16 * t), hi = *(const floatx4 *)(q + 16 * t + 4);
      const float x[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      split_fragment(x, qf[t]);
    }
  }
  // the K fragments of the key block at k0: key k0 + c (past the end: the last key, its scores are masked below)
  auto load_k = [&](bf16x8 (&kf)[KS][NP], int k0) {
    const uint32_t at = (uint32_t)(k0 + c < seq ? k0 + c : seq - 1) * kvrow + 8 * g;
#pragma unroll
    for (int t = 0; t < KS; ++t)
#pragma unroll
      for (int p = 0; p < NP; ++p) kf[t][p] = *(const bf16x8 *)(kbase[p] + (at + 16 * t));
  };

  floatx16 o0[DB], o1[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) o0[d][r] = o1[d][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  bf16x8 kf[KS][NP];
  load_k(kf, 0);
  for (int k0 = 0; k0 < seq; k0 += 32) {
    floatx16 s0, s1;
#pragma unroll
    for (int r = 0; r < 16; ++r) s0[r] = s1[r] = 0.f;
#pragma unroll
    for (int t = 0; t < KS; ++t) split_step(s0, s1, kf[t], qf[t]);
    if (k0 + 32 < seq) load_k(kf, k0 + 32);
    float p[16];
    float bm = -FLT_MAX;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = k0 + 8 * (r >> 2) + 4 * g + (r & 3);
      const bool live = key < seq && (mrow == nullptr || mrow[key < seq ? key : seq - 1] != 0);
      p[r] = live ? (s0[r] + s1[r]) * scale : -FLT_MAX;
      bm = fmaxf(bm, p[r]);
    }
    bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
    // a block of dead keys leaves the state untouched, as in attention_f32_mfma_kernel (liveness does not depend on the query: the
    // branch is uniform); a sequence without any live key ends as 0 * inf = NaN, like that kernel's and the fp32 oracle's
    if (bm == -FLT_MAX) continue;
    const float m_new = fmaxf(m_run, bm);
    const float alpha = expf(m_run - m_new);
    float ls = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      p[r] = p[r] == -FLT_MAX ? 0.f : expf(p[r] - m_new);
      ls += p[r];
    }
    ls += __shfl_xor(ls, 32, 64);
    l_run = l_run * alpha + ls;
    m_run = m_new;
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        o0[d][r] *= alpha;
        o1[d][r] *= alpha;
      }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      // V^T's fragments of the step: slot j = key k0 + 16 s + 8 (j >> 2) + 4 g + (j & 3), the key of register 8 s + j of p
      bf16x8 vf[DB][NP];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int key = k0 + 16 * s + 8 * (j >> 2) + 4 * g + (j & 3);
        const uint32_t at = (uint32_t)(key < seq ? key : seq - 1) * kvrow + c;   // past the end: the last key, its probability is +0
#pragma unroll
        for (int d = 0; d < DB; ++d)
#pragma unroll
          for (int pl = 0; pl < NP; ++pl) vf[d][pl][j] = __builtin_bit_cast(__bf16, vbase[pl][at + 32 * d]);
      }
      bf16x8 pf[NP];
      const float x[8] = {p[8 * s], p[8 * s + 1], p[8 * s + 2], p[8 * s + 3], p[8 * s + 4], p[8 * s + 5], p[8 * s + 6], p[8 * s + 7]};
      split_fragment(x, pf);
#pragma unroll
      for (int d = 0; d < DB; ++d) split_step(o0[d], o1[d], vf[d], pf);
    }
  }
  if (q0 + c >= seq) return;
  const float inv = 1.0f / l_run;   // (l_run == 0: no live key at all -> 0 * inf = NaN)
  float *dst = ctx + (first + q0 + c) * H + head * DH;
  // O^T[d][query]: registers 4 v .. 4 v + 3 are d = 32 block + 8 v + 4 g .. + 3 of the lane's query
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      floatx4 quad;
#pragma unroll
      for (int e = 0; e < 4; ++e) quad[e] = (o0[d][4 * v + e] + o1[d][4 * v + e]) * inv;
      *(floatx4 *)(dst + 32 * d + 8 * v + 4 * g) = quad;
    }
}

}  // namespace

void gemm_split(int epilogue, const float *A, const uint16_t *W_planes, const float *bias, const float *res, float *out, int M, int N, int K,
                hipStream_t s) {
  if (!gemm_split_takes(N, K) || M <= 0) throw StatusError(MRK_ERR_UNSUPPORTED, "encoder: the split product takes N % 64 == 0 and K % 32 == 0, got N " +
                                                                                   std::to_string(N) + ", K " + std::to_string(K));
  if (epilogue == DENSE_GELU) launch_gemm_split<DENSE_GELU>(A, W_planes, bias, res, out, M, N, K, s);
  else if (epilogue == DENSE_RES) launch_gemm_split<DENSE_RES>(A, W_planes, bias, res, out, M, N, K, s);
  else launch_gemm_split<DENSE_NONE>(A, W_planes, bias, res, out, M, N, K, s);
}

void attention_split(const float *qkv, uint16_t *kv_planes, const int32_t *mask, const int32_t *cu, int n, int seq, int M, int H, int heads,
                     float scale, float *ctx, hipStream_t s) {
  const int DH = heads > 0 ? H / heads : 0;
  if (!attention_split_takes(DH) || n <= 0 || seq <= 0 || M <= 0)
    throw StatusError(MRK_ERR_UNSUPPORTED, "encoder: split attention takes head sizes 32 and 64, got " + std::to_string(DH));
  const SplitAttentionPlan p = split_attention_plan(n, seq, M, H, heads);
  hipLaunchKernelGGL(split_kv_kernel, dim3(p.split_workgroups), dim3(p.split_threads), 0, s, qkv, kv_planes, M, H);
  const dim3 grid(p.query_blocks, p.head_groups, p.sequences), block(p.threads);
  if (DH == 32) hipLaunchKernelGGL((attention_split_kernel<32>), grid, block, 0, s, qkv, kv_planes, mask, cu, seq, M, H, heads, scale, ctx);
  else hipLaunchKernelGGL((attention_split_kernel<64>), grid, block, 0, s, qkv, kv_planes, mask, cu, seq, M, H, heads, scale, ctx);
}

}  // namespace mrk
