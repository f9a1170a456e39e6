// Instruction-issue micro-benchmark for gfx950: what a SIMD sustains per wave64 instruction, by instruction class and by
// resident wavefronts per SIMD.  The scorer (csrc/score_qs.hip) and the assembly kernels are bound by instruction issue;
// rounds 1-5 priced every instruction at 4 cycles ("a wavefront issues one instruction per 4 cycles whatever its type").
// This program measures it instead:
//   hipcc --offload-arch=gfx950 -O2 -o issue_bench tools/native/issue_bench.hip && ./issue_bench [substring of the rows to run]
// Output: one line per (body, waves per SIMD): cycles per instruction per SIMD at the nominal 2.4 GHz.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#define CK(x)                                                                          \
  do {                                                                                 \
    hipError_t e_ = (x);                                                               \
    if (e_ != hipSuccess) {                                                            \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_));      \
      exit(1);                                                                         \
    }                                                                                  \
  } while (0)

// every body: `iters` trips of an unrolled block of K instructions; results folded into out[] so nothing is dead
#define REP4(x) x x x x
#define REP8(x) REP4(x) REP4(x)
#define REP16(x) REP8(x) REP8(x)

__global__ void __launch_bounds__(256) k_valu_andor(int iters, uint32_t *out) {
  uint32_t a0 = threadIdx.x, a1 = 1, a2 = 2, a3 = 3, a4 = 4, a5 = 5, a6 = 6, a7 = 7, m = 0x10001u * (threadIdx.x & 15);
  for (int i = 0; i < iters; ++i) {
    REP8(asm volatile("v_and_or_b32 %0, %8, %9, %0\n\tv_and_or_b32 %1, %8, %9, %1\n\tv_and_or_b32 %2, %8, %9, %2\n\tv_and_or_b32 %3, %8, %9, %3\n\t"
                      "v_and_or_b32 %4, %8, %9, %4\n\tv_and_or_b32 %5, %8, %9, %5\n\tv_and_or_b32 %6, %8, %9, %6\n\tv_and_or_b32 %7, %8, %9, %7"
                      : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "s"(i));)
  }
  out[blockIdx.x * 256 + threadIdx.x] = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7;
}
constexpr int K_VALU_ANDOR = 64;

__global__ void __launch_bounds__(256) k_valu_pk16(int iters, uint32_t *out) {
  uint32_t a0 = threadIdx.x, a1 = 1, a2 = 2, a3 = 3, a4 = 4, a5 = 5, a6 = 6, a7 = 7;
  for (int i = 0; i < iters; ++i) {
    REP8(asm volatile("v_pk_sub_i16 %0, %8, %0\n\tv_pk_sub_i16 %1, %8, %1\n\tv_pk_sub_i16 %2, %8, %2\n\tv_pk_sub_i16 %3, %8, %3\n\t"
                      "v_pk_ashrrev_i16 %4, 15, %4\n\tv_pk_ashrrev_i16 %5, 15, %5\n\tv_pk_ashrrev_i16 %6, 15, %6\n\tv_pk_ashrrev_i16 %7, 15, %7"
                      : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "s"(i));)
  }
  out[blockIdx.x * 256 + threadIdx.x] = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7;
}
constexpr int K_VALU_PK16 = 64;

__global__ void __launch_bounds__(256) k_valu_addf64(int iters, double *out) {
  double a0 = threadIdx.x, a1 = 1, a2 = 2, a3 = 3, a4 = 4, a5 = 5, a6 = 6, a7 = 7, m = 1e-9 * threadIdx.x;
  for (int i = 0; i < iters; ++i) {
    REP8(asm volatile("v_add_f64 %0, %0, %8\n\tv_add_f64 %1, %1, %8\n\tv_add_f64 %2, %2, %8\n\tv_add_f64 %3, %3, %8\n\t"
                      "v_add_f64 %4, %4, %8\n\tv_add_f64 %5, %5, %8\n\tv_add_f64 %6, %6, %8\n\tv_add_f64 %7, %7, %8"
                      : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m));)
  }
  out[blockIdx.x * 256 + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;
}
constexpr int K_VALU_ADDF64 = 64;

// one dependent chain of f64 adds (the leaf sum of one row)
__global__ void __launch_bounds__(256) k_valu_addf64_chain(int iters, double *out) {
  double a0 = threadIdx.x, m = 1e-9 * threadIdx.x;
  for (int i = 0; i < iters; ++i) {
    REP16(asm volatile("v_add_f64 %0, %0, %1\n\tv_add_f64 %0, %0, %1\n\tv_add_f64 %0, %0, %1\n\tv_add_f64 %0, %0, %1" : "+v"(a0) : "v"(m));)
  }
  out[blockIdx.x * 256 + threadIdx.x] = a0;
}
constexpr int K_VALU_ADDF64_CHAIN = 64;

__global__ void __launch_bounds__(256) k_salu(int iters, uint32_t *out) {
  uint32_t s0 = blockIdx.x, s1 = 1, s2 = 2, s3 = 3;
  for (int i = 0; i < iters; ++i) {
    REP16(asm volatile("s_lshr_b32 %0, %0, 1\n\ts_pack_ll_b32_b16 %1, %1, %0\n\ts_lshr_b32 %2, %2, 1\n\ts_pack_ll_b32_b16 %3, %3, %2"
                       : "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3) : : "scc");)
  }
  out[blockIdx.x * 256 + threadIdx.x] = s0 ^ s1 ^ s2 ^ s3;
}
constexpr int K_SALU = 64;

// VALU and SALU side by side in ONE wavefront's stream (1 : 1)
__global__ void __launch_bounds__(256) k_valu_salu(int iters, uint32_t *out) {
  uint32_t a0 = threadIdx.x, a1 = 1, a2 = 2, a3 = 3, m = 0x10001u * (threadIdx.x & 15);
  uint32_t s0 = blockIdx.x, s1 = 1, s2 = 2, s3 = 3;
  for (int i = 0; i < iters; ++i) {
    REP8(asm volatile("v_and_or_b32 %0, %8, %9, %0\n\ts_lshr_b32 %4, %4, 1\n\tv_and_or_b32 %1, %8, %9, %1\n\ts_pack_ll_b32_b16 %5, %5, %4\n\t"
                      "v_and_or_b32 %2, %8, %9, %2\n\ts_lshr_b32 %6, %6, 1\n\tv_and_or_b32 %3, %8, %9, %3\n\ts_pack_ll_b32_b16 %7, %7, %6"
                      : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3) : "v"(m), "s"(i) : "scc");)
  }
  out[blockIdx.x * 256 + threadIdx.x] = a0 ^ a1 ^ a2 ^ a3 ^ s0 ^ s1 ^ s2 ^ s3;
}
constexpr int K_VALU_SALU = 64;  // 32 VALU + 32 SALU

// the scorer's tree step as it is today: per node an M0 write, a mask replication, one ds_read_addtid, three VALU;
// 15 nodes + 13 VALU of leaf bookkeeping stand-ins = 58 VALU + 30 SALU + 15 LDS per "tree"
__global__ void __launch_bounds__(256) k_tree_now(int iters, uint32_t *out) {
  __shared__ uint32_t slab[64 * 64];
  for (int i = threadIdx.x; i < 64 * 64; i += 256) slab[i] = i * 2654435761u;
  __syncthreads();
  uint32_t acc_a = 0, acc_b = 0, kk = 0x00400040u;
  uint32_t mv = (uint32_t)(blockIdx.x & 7) << 24 | 0x5a5au;
  for (int i = 0; i < iters; ++i) {
    uint32_t c[15], mm[15];
#pragma unroll
    for (int s = 0; s < 15; ++s) {
      asm volatile("s_lshr_b32 m0, %2, 16\n\ts_pack_ll_b32_b16 %1, %2, %2\n\tds_read_addtid_b32 %0" : "=v"(c[s]), "=s"(mm[s]) : "s"(mv + (s << 24)) : "memory", "scc");
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int s = 0; s < 15; ++s) asm volatile("v_pk_sub_i16 %0, %1, %0" : "+v"(c[s]) : "s"(kk));
#pragma unroll
    for (int s = 0; s < 15; ++s) asm volatile("v_pk_ashrrev_i16 %0, 15, %0" : "+v"(c[s]));
#pragma unroll
    for (int s = 0; s < 15; s += 2) {
      asm volatile("v_and_or_b32 %0, %1, %2, %0" : "+v"(acc_a) : "v"(c[s]), "s"(mm[s]));
      if (s + 1 < 15) asm volatile("v_and_or_b32 %0, %1, %2, %0" : "+v"(acc_b) : "v"(c[s + 1]), "s"(mm[s + 1]));
    }
    REP8(asm volatile("v_xor_b32 %0, %0, %1" : "+v"(acc_a) : "v"(acc_b));)
    REP4(asm volatile("v_xor_b32 %0, %0, %1" : "+v"(acc_b) : "v"(acc_a));)
    asm volatile("v_xor_b32 %0, %0, %1" : "+v"(acc_b) : "v"(acc_a));
  }
  out[blockIdx.x * 256 + threadIdx.x] = acc_a ^ acc_b;
}
constexpr int K_TREE_NOW = 58 + 30 + 15;

// the same with NO scalar work per node: the replicated mask and the LDS byte offset come ready-made (scalar
// registers loaded once), the read is a plain ds_read_b32 with a VGPR address formed by one v_add per node
__global__ void __launch_bounds__(256) k_tree_valu_addr(int iters, uint32_t *out) {
  __shared__ uint32_t slab[64 * 64];
  for (int i = threadIdx.x; i < 64 * 64; i += 256) slab[i] = i * 2654435761u;
  __syncthreads();
  uint32_t acc_a = 0, acc_b = 0, kk = 0x00400040u, mm = 0x5a5a5a5au;
  const uint32_t lane_off = (threadIdx.x & 63) * 4, voff = (blockIdx.x & 7) << 8;
  for (int i = 0; i < iters; ++i) {
    uint32_t c[15];
#pragma unroll
    for (int s = 0; s < 15; ++s) {
      uint32_t addr;
      asm volatile("v_add_u32 %0, %1, %2" : "=v"(addr) : "s"(voff + (s << 8)), "v"(lane_off));
      asm volatile("ds_read_b32 %0, %1" : "=v"(c[s]) : "v"(addr) : "memory");
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int s = 0; s < 15; ++s) asm volatile("v_pk_sub_i16 %0, %1, %0" : "+v"(c[s]) : "s"(kk));
#pragma unroll
    for (int s = 0; s < 15; ++s) asm volatile("v_pk_ashrrev_i16 %0, 15, %0" : "+v"(c[s]));
#pragma unroll
    for (int s = 0; s < 15; s += 2) {
      asm volatile("v_and_or_b32 %0, %1, %2, %0" : "+v"(acc_a) : "v"(c[s]), "s"(mm));
      if (s + 1 < 15) asm volatile("v_and_or_b32 %0, %1, %2, %0" : "+v"(acc_b) : "v"(c[s + 1]), "s"(mm));
    }
    REP8(asm volatile("v_xor_b32 %0, %0, %1" : "+v"(acc_a) : "v"(acc_b));)
    REP4(asm volatile("v_xor_b32 %0, %0, %1" : "+v"(acc_b) : "v"(acc_a));)
    asm volatile("v_xor_b32 %0, %0, %1" : "+v"(acc_b) : "v"(acc_a));
  }
  out[blockIdx.x * 256 + threadIdx.x] = acc_a ^ acc_b;
}
constexpr int K_TREE_VALU_ADDR = 58 + 15 + 15;

// M0 written by s_mov from a ready-made offset register, mask ready-made: one SALU per node instead of two
__global__ void __launch_bounds__(256) k_tree_m0_only(int iters, uint32_t *out) {
  __shared__ uint32_t slab[64 * 64];
  for (int i = threadIdx.x; i < 64 * 64; i += 256) slab[i] = i * 2654435761u;
  __syncthreads();
  uint32_t acc_a = 0, acc_b = 0, kk = 0x00400040u, mm = 0x5a5a5a5au;
  const uint32_t voff = (blockIdx.x & 7) << 8;
  for (int i = 0; i < iters; ++i) {
    uint32_t c[15];
#pragma unroll
    for (int s = 0; s < 15; ++s)
      asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tds_read_addtid_b32 %0" : "=v"(c[s]) : "s"(voff + (s << 8)) : "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int s = 0; s < 15; ++s) asm volatile("v_pk_sub_i16 %0, %1, %0" : "+v"(c[s]) : "s"(kk));
#pragma unroll
    for (int s = 0; s < 15; ++s) asm volatile("v_pk_ashrrev_i16 %0, 15, %0" : "+v"(c[s]));
#pragma unroll
    for (int s = 0; s < 15; s += 2) {
      asm volatile("v_and_or_b32 %0, %1, %2, %0" : "+v"(acc_a) : "v"(c[s]), "s"(mm));
      if (s + 1 < 15) asm volatile("v_and_or_b32 %0, %1, %2, %0" : "+v"(acc_b) : "v"(c[s + 1]), "s"(mm));
    }
    REP8(asm volatile("v_xor_b32 %0, %0, %1" : "+v"(acc_a) : "v"(acc_b));)
    REP4(asm volatile("v_xor_b32 %0, %0, %1" : "+v"(acc_b) : "v"(acc_a));)
    asm volatile("v_xor_b32 %0, %0, %1" : "+v"(acc_b) : "v"(acc_a));
  }
  out[blockIdx.x * 256 + threadIdx.x] = acc_a ^ acc_b;
}
constexpr int K_TREE_M0_ONLY = 58 + 30 + 15;  // (s_nop counted as an issue slot)

// the byte-mode tree step (score_qs.hip qs_score_byte_split_kernel): cells clamped to 255 and k <= 254, so one v_pk_sub_i16
// leaves a clean 0xFF / 0x00 high byte per row; leaves 0-7 are ORed into acc_a, 8-15 into acc_b, a node whose left subtree
// crosses position 8 ("crossing", z per tree) into both; one v_perm_b32 merges them.  Per tree: M0 write + s_nop + read per node,
// 15 v_pk_sub, (x + z) + (15 - x) = 15 + z v_and_or_b32 entered by wavefront-uniform switches, 1 v_perm, 12 VALU of leaf
// bookkeeping stand-ins (today's 13 less the acc_a | acc_b merge) = 43 + z VALU + 30 SALU + 15 LDS (+ the switches' SALU)
// one straight-line ladder per count (no fall-through between cases: the CFG stays a plain multiway branch).  TWO: slots
// alternate between two accumulators, so that no v_and_or_b32 reads the one before it (the compiler puts an s_nop between
// dependent inline-asm VALU ops), merged by one v_or_b32 per ladder
template <bool TWO, int B, int E>
__device__ __forceinline__ void byte_ladder(uint32_t &acc, uint32_t &acc2, const uint32_t (&c)[15], const uint32_t (&m)[15]) {
#pragma unroll
  for (int s = B; s < E; ++s) {
    if (TWO && (s & 1)) asm("v_and_or_b32 %0, %1, %2, %0" : "+v"(acc2) : "v"(c[s]), "s"(m[s]));
    else asm("v_and_or_b32 %0, %1, %2, %0" : "+v"(acc) : "v"(c[s]), "s"(m[s]));
  }
}
// the same ladders as independent guarded blocks of G slots: A runs blocks that start below a, B blocks that end above x.  A block
// may overrun the ladder's bound by up to G - 1 slots: harmless, a B-only slot's A mask and an A-only slot's B mask are 0
template <int G, bool A_SIDE>
__device__ __forceinline__ void byte_blocks(uint32_t &acc, const uint32_t (&c)[15], const uint32_t (&m)[15], int bound) {
#pragma unroll
  for (int b0 = 0; b0 < 15; b0 += G) {
    if (A_SIDE ? b0 < bound : b0 + G > bound) {
#pragma unroll
      for (int s = b0; s < b0 + G && s < 15; ++s) asm("v_and_or_b32 %0, %1, %2, %0" : "+v"(acc) : "v"(c[s]), "s"(m[s]));
    }
  }
}
#define BYTE_CASES(F) F(0) F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10) F(11) F(12) F(13) F(14) F(15)
template <int MODE>  // 0 switch, 1 switch + two chains, 2 compile-time x = 6 / a = 8, 4 / 2 guarded blocks of 4 / 2 slots
__global__ void __launch_bounds__(256) k_tree_byte(int iters, uint32_t *out, int x, int a) {
  uint32_t acc_a2 = 0, acc_b2 = 0;
  __shared__ uint32_t slab[64 * 64];
  for (int i = threadIdx.x; i < 64 * 64; i += 256) slab[i] = (i * 2654435761u) & 0x00ff00ffu;
  __syncthreads();
  uint32_t acc_a = 0, acc_b = 0, kk = 0x00400040u, ma[15], mb[15];
#pragma unroll
  for (int s = 0; s < 15; ++s) {  // per-slot masks in scalar registers, as the kernel's node loads leave them
    ma[s] = __builtin_amdgcn_readfirstlane(0x5a005a00u + (s << 9) + x);
    mb[s] = __builtin_amdgcn_readfirstlane(0x3c003c00u + (s << 9) + a);
  }
  const uint32_t voff = (blockIdx.x & 7) << 8;
  for (int i = 0; i < iters; ++i) {
    uint32_t c[15];
#pragma unroll
    for (int s = 0; s < 15; ++s)
      asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tds_read_addtid_b32 %0" : "=v"(c[s]) : "s"(voff + (s << 8)) : "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int s = 0; s < 15; ++s) asm volatile("v_pk_sub_i16 %0, %1, %0" : "+v"(c[s]) : "s"(kk));
    constexpr bool TWO = MODE == 1;
    if constexpr (MODE == 2) {
      byte_ladder<false, 0, 8>(acc_a, acc_a2, c, ma);
      byte_ladder<false, 6, 15>(acc_b, acc_b2, c, mb);
    } else if constexpr (MODE == 4 || MODE == 3) {
      byte_blocks<MODE == 4 ? 4 : 2, true>(acc_a, c, ma, a);
      byte_blocks<MODE == 4 ? 4 : 2, false>(acc_b, c, mb, x);
    } else {
    switch (a) {  // slots [0, a)
#define CASE_A(n) case n: byte_ladder<TWO, 0, n>(acc_a, acc_a2, c, ma); break;
      BYTE_CASES(CASE_A)
#undef CASE_A
    }
    switch (x) {  // slots [x, 15)
#define CASE_B(n) case n: byte_ladder<TWO, n, 15>(acc_b, acc_b2, c, mb); break;
      BYTE_CASES(CASE_B)
#undef CASE_B
    }
    }
    if (TWO) {
      acc_a |= acc_a2;
      acc_b |= acc_b2;
    }
    asm volatile("v_perm_b32 %0, %1, %0, %2" : "+v"(acc_a) : "v"(acc_b), "s"(0x07030501u));
    REP8(asm volatile("v_xor_b32 %0, %0, %1" : "+v"(acc_a) : "v"(acc_b));)
    REP4(asm volatile("v_xor_b32 %0, %0, %1" : "+v"(acc_b) : "v"(acc_a));)
  }
  out[blockIdx.x * 256 + threadIdx.x] = acc_a ^ acc_b;
}

// The byte-mode step WHOLE, as the kernel issues it, round 7's against round 17's ("lean"): the guarded blocks of 4 above plus what
// surrounds them.  LEAN = false: two v_mov zero fills, one asm statement per v_and_or_b32 (the compiler pads dependent ones with
// s_nop), exit leaves by v_not / v_ffbl x 2 / v_lshl_or, the store address by v_lshl_add_u32 from the tree's number, ds_write_b16.
// LEAN = true: a block is ONE asm statement and the block that opens a ladder (slots 0-3 of A, 12-14 of B: they always run) starts
// from the inline constant 0; 8 trips are unrolled, so the store goes to a loop-invariant address plus an immediate; the cell
// reads carry the slab's immediate offset.  (Not modelled: the adding rows and the scalar loads.)
template <bool FIRST, int B0>
__device__ __forceinline__ void lean_block(uint32_t &acc, const uint32_t (&c)[15], const uint32_t (&m)[15]) {
  if constexpr (B0 == 12) {
    if constexpr (FIRST)
      asm volatile("v_and_or_b32 %0, %1, %4, 0\n\tv_and_or_b32 %0, %2, %5, %0\n\tv_and_or_b32 %0, %3, %6, %0"
                   : "=&v"(acc) : "v"(c[12]), "v"(c[13]), "v"(c[14]), "s"(m[12]), "s"(m[13]), "s"(m[14]));
    else
      asm volatile("v_and_or_b32 %0, %1, %4, %0\n\tv_and_or_b32 %0, %2, %5, %0\n\tv_and_or_b32 %0, %3, %6, %0"
                   : "+v"(acc) : "v"(c[12]), "v"(c[13]), "v"(c[14]), "s"(m[12]), "s"(m[13]), "s"(m[14]));
  } else {
    if constexpr (FIRST)
      asm volatile("v_and_or_b32 %0, %1, %5, 0\n\tv_and_or_b32 %0, %2, %6, %0\n\tv_and_or_b32 %0, %3, %7, %0\n\tv_and_or_b32 %0, %4, %8, %0"
                   : "=&v"(acc) : "v"(c[B0]), "v"(c[B0 + 1]), "v"(c[B0 + 2]), "v"(c[B0 + 3]), "s"(m[B0]), "s"(m[B0 + 1]), "s"(m[B0 + 2]), "s"(m[B0 + 3]));
    else
      asm volatile("v_and_or_b32 %0, %1, %5, %0\n\tv_and_or_b32 %0, %2, %6, %0\n\tv_and_or_b32 %0, %3, %7, %0\n\tv_and_or_b32 %0, %4, %8, %0"
                   : "+v"(acc) : "v"(c[B0]), "v"(c[B0 + 1]), "v"(c[B0 + 2]), "v"(c[B0 + 3]), "s"(m[B0]), "s"(m[B0 + 1]), "s"(m[B0 + 2]), "s"(m[B0 + 3]));
  }
}
template <bool LEAN>
__global__ void __launch_bounds__(256) k_tree_byte_whole(int iters, uint32_t *out, int x, int a) {
  constexpr int SLAB = 4096;          // [exit leaves of 8 trees x 4 wavefronts: 4 KB][slab: 16 KB] (LEAN reads the slab at offset:SLAB)
  __shared__ uint32_t lds[(SLAB + 64 * 64 * 4) / 4];
  for (int i = threadIdx.x; i < (int)(sizeof(lds) / 4); i += 256) lds[i] = (i * 2654435761u) & 0x00ff00ffu;
  __syncthreads();
  uint32_t kk = 0x00400040u, ma[15], mb[15];
#pragma unroll
  for (int s = 0; s < 15; ++s) {
    ma[s] = __builtin_amdgcn_readfirstlane(0x5a005a00u + (s << 9) + x);
    mb[s] = __builtin_amdgcn_readfirstlane(0x3c003c00u + (s << 9) + a);
  }
  const uint32_t voff = (blockIdx.x & 7) << 8;
  const uint32_t idx0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)lds + threadIdx.x * 2;  // stores stay inside [0, SLAB)
  uint32_t sink = 0;
  auto step = [&](auto J, int tt) {
    constexpr int j = decltype(J)::value;
    uint32_t c[15], acc_a, acc_b;
#pragma unroll
    for (int s = 0; s < 15; ++s) {
      if constexpr (LEAN) asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tds_read_addtid_b32 %0 offset:%2" : "=v"(c[s]) : "s"(voff + (s << 8)), "n"(SLAB) : "memory");
      else asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tds_read_addtid_b32 %0" : "=v"(c[s]) : "s"(SLAB + voff + (s << 8)) : "memory");
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int s = 0; s < 15; ++s) asm volatile("v_pk_sub_i16 %0, %1, %0" : "+v"(c[s]) : "s"(kk));
    if constexpr (LEAN) {
      lean_block<true, 0>(acc_a, c, ma);
      if (a > 4) lean_block<false, 4>(acc_a, c, ma);
      if (a > 8) lean_block<false, 8>(acc_a, c, ma);
      if (a > 12) lean_block<false, 12>(acc_a, c, ma);
      lean_block<true, 12>(acc_b, c, mb);
      if (x < 12) lean_block<false, 8>(acc_b, c, mb);
      if (x < 8) lean_block<false, 4>(acc_b, c, mb);
      if (x < 4) lean_block<false, 0>(acc_b, c, mb);
    } else {
      asm volatile("v_mov_b32 %0, 0\n\tv_mov_b32 %1, 0" : "=v"(acc_a), "=v"(acc_b));
      byte_blocks<4, true>(acc_a, c, ma, a);
      byte_blocks<4, false>(acc_b, c, mb, x);
    }
    uint32_t l0, l1, pair;
    asm volatile("v_perm_b32 %0, %1, %0, %2\n\tv_not_b32 %0, %0" : "+v"(acc_a) : "v"(acc_b), "s"(0x07030501u));
    asm volatile("v_ffbl_b32 %0, %2\n\tv_ffbl_b32_sdwa %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1" : "=&v"(l0), "=&v"(l1) : "v"(acc_a));
    if constexpr (LEAN) {
      asm volatile("v_lshl_or_b32 %0, %2, 8, %1" : "=v"(pair) : "v"(l0), "v"(l1));
      asm volatile("ds_write_b16 %0, %1 offset:%2" : : "v"(idx0), "v"(pair), "n"(j * 512) : "memory");
    } else {
      uint32_t addr;
      asm volatile("v_lshl_or_b32 %0, %3, 8, %2\n\tv_lshl_add_u32 %1, %4, 9, %5" : "=&v"(pair), "=&v"(addr) : "v"(l0), "v"(l1), "s"(tt), "v"(idx0));
      asm volatile("ds_write_b16 %0, %1" : : "v"(addr), "v"(pair) : "memory");
    }
    sink ^= pair;
  };
  if constexpr (LEAN) {
    for (int i = 0; i < iters; i += 8) {
      step(std::integral_constant<int, 0>{}, 0); step(std::integral_constant<int, 1>{}, 1);
      step(std::integral_constant<int, 2>{}, 2); step(std::integral_constant<int, 3>{}, 3);
      step(std::integral_constant<int, 4>{}, 4); step(std::integral_constant<int, 5>{}, 5);
      step(std::integral_constant<int, 6>{}, 6); step(std::integral_constant<int, 7>{}, 7);
    }
  } else {
#pragma unroll 1
    for (int i = 0; i < iters; ++i) step(std::integral_constant<int, 0>{}, i & 7);
  }
  out[blockIdx.x * 256 + threadIdx.x] = sink;
}

// dependent LDS search chain: 8 dependent ds_read_b32 + compare/select (the binning search of the assembly kernel)
__global__ void __launch_bounds__(256) k_lds_chain(int iters, uint32_t *out) {
  __shared__ uint32_t slab[64 * 64];
  for (int i = threadIdx.x; i < 64 * 64; i += 256) slab[i] = (i * 2654435761u) & 0x3ffcu;
  __syncthreads();
  uint32_t a = threadIdx.x * 4;
  for (int i = 0; i < iters; ++i) {
    REP8(asm volatile("ds_read_b32 %0, %0\n\ts_waitcnt lgkmcnt(0)" : "+v"(a) : : "memory");)
  }
  out[blockIdx.x * 256 + threadIdx.x] = a;
}
constexpr int K_LDS_CHAIN = 8;

static const char *g_only = nullptr;  // argv[1]: run only the rows whose name contains it

template <typename T, typename K, typename... Extra>
static void run(const char *name, K kern, int k_per_iter, int n_cus, T *d_out, Extra... extra) {
  const int iters = 4096;
  if (g_only && !strstr(name, g_only)) return;
  fprintf(stderr, "%s\n", name);
  for (int w : {1, 2, 4, 8}) {  // 256-thread workgroups per CU = wavefronts per SIMD
    const int grid = n_cus * w;
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, 0, iters / 8, d_out, extra...);  // warm
    CK(hipDeviceSynchronize());
    float best = 1e30f;
    for (int rep = 0; rep < 5; ++rep) {
      CK(hipEventRecord(e0, 0));
      hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, 0, iters, d_out, extra...);
      CK(hipEventRecord(e1, 0));
      CK(hipEventSynchronize(e1));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      if (ms < best) best = ms;
    }
    // every SIMD runs w wavefronts, each issuing iters * k instructions
    const double instr_per_simd = (double)iters * k_per_iter * w;
    const double cyc = best * 1e-3 * 2.4e9 / instr_per_simd;
    printf("%-22s waves/SIMD %d  %8.3f ms  %6.2f cycles/instruction/SIMD (2.4 GHz)   %7.1f cycles per trip per wavefront\n", name, w, best, cyc,
           best * 1e-3 * 2.4e9 / iters);
  }
}

int main(int argc, char **argv) {
  if (argc > 1) g_only = argv[1];
  setvbuf(stdout, nullptr, _IOLBF, 0);
  fprintf(stderr, "start\n");
  hipDeviceProp_t p;
  CK(hipGetDeviceProperties(&p, 0));
  const int n_cus = p.multiProcessorCount;
  printf("device %s, %d CUs, clock %d kHz\n", p.gcnArchName, n_cus, p.clockRate);
  void *d;
  CK(hipMalloc(&d, (size_t)n_cus * 8 * 256 * 8));
  run("valu v_and_or_b32", k_valu_andor, K_VALU_ANDOR, n_cus, (uint32_t *)d);
  run("valu v_pk_*_i16", k_valu_pk16, K_VALU_PK16, n_cus, (uint32_t *)d);
  run("valu v_add_f64 indep", k_valu_addf64, K_VALU_ADDF64, n_cus, (double *)d);
  run("valu v_add_f64 chain", k_valu_addf64_chain, K_VALU_ADDF64_CHAIN, n_cus, (double *)d);
  run("salu", k_salu, K_SALU, n_cus, (uint32_t *)d);
  run("valu+salu 1:1", k_valu_salu, K_VALU_SALU, n_cus, (uint32_t *)d);
  run("tree step (today)", k_tree_now, K_TREE_NOW, n_cus, (uint32_t *)d);
  run("tree step (m0 only)", k_tree_m0_only, K_TREE_M0_ONLY, n_cus, (uint32_t *)d);
  run("tree step (valu addr)", k_tree_valu_addr, K_TREE_VALU_ADDR, n_cus, (uint32_t *)d);
  // x = A-only nodes, a = x + z nodes touch acc_a; 43 + z VALU (+ 2: two chains) + 30 SALU + 15 LDS per trip
  const char *modes[] = {"switch", "switch 2ch", "fixed", "blk2", "blk4"};
  for (int mode : {0, 1, 3, 4})
    for (int z : {0, 2, 7}) {
      const int x = z == 7 ? 0 : 7 - z / 2;
      char name[48];
      snprintf(name, sizeof name, "tree step (byte %s z=%d)", modes[mode], z);
      auto k = mode == 0 ? k_tree_byte<0> : mode == 1 ? k_tree_byte<1> : mode == 3 ? k_tree_byte<3> : k_tree_byte<4>;
      run(name, k, 43 + z + (mode == 1 ? 2 : 0) + 30 + 15, n_cus, (uint32_t *)d, x, x + z);
    }
  run("tree step (byte fixed z=2)", k_tree_byte<2>, 43 + 2 + 30 + 15, n_cus, (uint32_t *)d, 6, 8);
  // round 7's whole step against round 17's: 15 + (blocks' v_and_or_b32) + 8 VALU (r7) / + 5 (lean), 30 SALU, 16 LDS
  for (int z : {0, 2, 7}) {
    const int x = z == 7 ? 0 : 7 - z / 2, a = x + z;
    const int andor = 4 * ((a + 3) / 4 < 4 ? (a + 3) / 4 : 4) - (a > 12 ? 1 : 0) + (15 - 4 * (x / 4));
    char name[48];
    snprintf(name, sizeof name, "tree step (r7 whole z=%d)", z);
    run(name, k_tree_byte_whole<false>, 15 + andor + 8 + 30 + 16, n_cus, (uint32_t *)d, x, a);
    snprintf(name, sizeof name, "tree step (lean z=%d)", z);
    run(name, k_tree_byte_whole<true>, 15 + andor + 5 + 30 + 16, n_cus, (uint32_t *)d, x, a);
  }
  run("lds dependent chain", k_lds_chain, K_LDS_CHAIN, n_cus, (uint32_t *)d);
  CK(hipFree(d));
  return 0;
}
