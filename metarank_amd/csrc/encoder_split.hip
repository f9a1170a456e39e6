// The dense products of an encoder loaded with MRK_ENCODER_SPLIT, on gfx950's bf16 matrix instruction.
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

}  // namespace

void gemm_split(int epilogue, const float *A, const uint16_t *W_planes, const float *bias, const float *res, float *out, int M, int N, int K,
                hipStream_t s) {
  if (!gemm_split_takes(N, K) || M <= 0) throw StatusError(MRK_ERR_UNSUPPORTED, "encoder: the split product takes N % 64 == 0 and K % 32 == 0, got N " +
                                                                                   std::to_string(N) + ", K " + std::to_string(K));
  if (epilogue == DENSE_GELU) launch_gemm_split<DENSE_GELU>(A, W_planes, bias, res, out, M, N, K, s);
  else if (epilogue == DENSE_RES) launch_gemm_split<DENSE_RES>(A, W_planes, bias, res, out, M, N, K, s);
  else launch_gemm_split<DENSE_NONE>(A, W_planes, bias, res, out, M, N, K, s);
}

}  // namespace mrk
