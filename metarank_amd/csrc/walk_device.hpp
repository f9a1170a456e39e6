// The tree walk of the forest scorer, shared by score.hip (score_kernel: a matrix tile per workgroup) and by the one-request
// kernels of rank_device.hpp (rank_one_walk_body: the request's matrix never leaves LDS): the node decisions of both
// libraries, the dense-row preprocessing of a cell, and the walk of U trees of one row at once over a chunk of the
// tree-walk image that lies in LDS (forest.hpp PackedForest).  Part of the translation unit of the run-time specialised
// kernels (jit.cpp), so fixed-width integers only.
#pragma once
#include <hip/hip_runtime.h>

#include "device_types.hpp"

namespace mrk {

namespace {

#ifndef MRK_SCORE_U
#define MRK_SCORE_U 4
#endif
constexpr int WALK_U = MRK_SCORE_U;  // trees walked concurrently per lane

struct alignas(16) Node16 {
  uint32_t w0, w1;  // thr (f64) | thr (f32) + feat/flags
  uint32_t w2, w3;
};

__device__ __forceinline__ bool in_bitset(const uint32_t *__restrict__ bits, uint32_t begin,
                                          uint32_t words, int c) {
  uint32_t w = (uint32_t)c >> 5;
  if (w >= words) return false;
  return (bits[begin + w] >> (c & 31)) & 1u;
}

// LightGBM Tree::NumericalDecision / CategoricalDecision on a value that already went through the
// dense-row zero flush (|v| <= 1e-35 -> 0.0).  Returns true for "go left".
__device__ __forceinline__ bool decide64(uint32_t w0, uint32_t w1, uint32_t w2, double v,
                                         const uint32_t *__restrict__ cat_bits) {
  const uint32_t flags = (w2 >> 16) & 0xffu;
  const bool nan_left = (w2 >> 24) & 1u;
  const bool isn = v != v;
  if (__builtin_expect(flags & NF_CATEGORICAL, 0)) {
    if (isn) return false;
    int iv = (int)v;  // v_cvt_i32_f64 saturates; out-of-range -> not in the bitset / negative
    if (iv < 0) return false;
    return in_bitset(cat_bits, w0, w1, iv);
  }
  const double thr = __hiloint2double((int)w1, (int)w0);
  bool left = v <= thr;
  if ((flags & NF_MISS_ZERO) && v == 0.0) left = (flags & NF_DEFAULT_LEFT) != 0;
  return isn ? nan_left : left;
}

// XGBoost RegTree::GetNext with a float feature value; NaN is "missing".
__device__ __forceinline__ bool decide32(uint32_t w0, uint32_t w1, uint32_t w3, float v,
                                         const uint32_t *__restrict__ cat_bits) {
  const uint32_t flags = (w1 >> 16) & 0xffu;
  const bool def_left = (flags & NF_DEFAULT_LEFT) != 0;
  if (v != v) return def_left;
  if (__builtin_expect(flags & NF_CATEGORICAL, 0)) {
    // common::Decision: invalid category (negative or >= 2^24) or beyond the bitset -> left;
    // member of the set -> right.
    if (v < 0.f || v >= 16777216.f) return true;
    int c = (int)v;
    return !in_bitset(cat_bits, w0, w3, c);
  }
  return v < __uint_as_float(w0);
}

template <bool F64>
struct RowT;
template <>
struct RowT<true> { using type = double; };
template <>
struct RowT<false> { using type = float; };

// dense-row preprocessing applied once per cell when the tile is staged
template <bool F64>
__device__ __forceinline__ typename RowT<F64>::type prep(double x, int *flag, int bit = 1) {
  if constexpr (F64) {
    // LightGBM RowFunctionFromDenseMatric keeps a cell only if |x| > kZeroThreshold (1e-35f) or NaN;
    // everything else reads back as 0.0 from the prediction buffer.
    const double kZero = (double)1e-35f;
    return (fabs(x) > kZero || x != x) ? x : 0.0;
  } else {
    // ltrlib narrows Double -> Float before DMatrix (round-to-nearest-even, overflow -> inf);
    // XGBoost rejects +-inf when `missing` is NaN ("Input data contains `inf`").
    float f = (float)x;
    if (__builtin_isinf(f)) atomicOr(flag, bit);
    return f;
  }
}

// Trees [t0, t0 + U) of the chunk in LDS (`s_chunk`: its image, `s_refs`: its TreeRef rows, `nt` trees) walked for ONE row
// by this lane.  gather(feat, walking) is the row's value of column `feat` (`walking` false: the slot has finished - any
// in-range value).  On return node[u] = ~(exit leaf) and lbase[u] = the byte offset of tree t0 + u's leaf array in the
// chunk; slots past `nt` hold leaf 0 of the last tree and are never added.
template <bool F64, int U, typename Gather>
__device__ __forceinline__ void walk_trees(const uint8_t *s_chunk, const TreeRef *s_refs, int t0, int nt,
                                           const uint32_t *__restrict__ cat_bits, const Gather &gather, int (&node)[U], uint32_t (&lbase)[U]) {
  uint32_t nbase[U];
  int maxd = 0;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int t = min(t0 + u, nt - 1);
    const TreeRef tr = s_refs[t];
    nbase[u] = tr.node_off;
    lbase[u] = tr.leaf_off;
    const bool live = (t0 + u) < nt && tr.n_nodes != 0;
    node[u] = live ? 0 : -1;  // -1 == ~0: single-leaf tree (or padding slot, never added)
    maxd = max(maxd, live ? (int)tr.depth : 0);
  }
  for (int d = 0; d < maxd; ++d) {
    // Phase-structured so that the U dependency chains overlap: all node reads are issued
    // back to back, then all feature gathers, then the (branch-free) numerical decisions.
    // Categorical nodes are rare and fixed up afterwards under one wave-level branch.
    Node16 nd[U];
    bool walking[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      walking[u] = node[u] >= 0;  // finished lanes re-read node 0; keep their gather in range
      nd[u] = *(const Node16 *)(s_chunk + nbase[u] + (uint32_t)max(node[u], 0) * 16u);
    }
    bool left[U];
    uint32_t any_flags = 0;
    if constexpr (F64) {
      double v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t feat = walking[u] ? (nd[u].w2 & 0xffffu) : 0u;
        v[u] = gather(feat, walking[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t flags = (nd[u].w2 >> 16) & 0xffu;
        any_flags |= walking[u] ? flags : 0u;
        const double thr = __hiloint2double((int)nd[u].w1, (int)nd[u].w0);
        bool l = v[u] <= thr;
        if ((flags & NF_MISS_ZERO) && v[u] == 0.0) l = (flags & NF_DEFAULT_LEFT) != 0;
        left[u] = (v[u] != v[u]) ? (((nd[u].w2 >> 24) & 1u) != 0) : l;
      }
      if (__builtin_expect((any_flags & NF_CATEGORICAL) != 0, 0)) {
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (walking[u] && (((nd[u].w2 >> 16) & NF_CATEGORICAL) != 0))
            left[u] = decide64(nd[u].w0, nd[u].w1, nd[u].w2, v[u], cat_bits);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int next = left[u] ? (int)(short)(nd[u].w3 & 0xffffu) : (int)(short)(nd[u].w3 >> 16);
        node[u] = walking[u] ? next : node[u];
      }
    } else {
      float v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t feat = walking[u] ? (nd[u].w1 & 0xffffu) : 0u;
        v[u] = gather(feat, walking[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t flags = (nd[u].w1 >> 16) & 0xffu;
        any_flags |= walking[u] ? flags : 0u;
        const bool l = v[u] < __uint_as_float(nd[u].w0);
        left[u] = (v[u] != v[u]) ? ((flags & NF_DEFAULT_LEFT) != 0) : l;
      }
      if (__builtin_expect((any_flags & NF_CATEGORICAL) != 0, 0)) {
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (walking[u] && (((nd[u].w1 >> 16) & NF_CATEGORICAL) != 0))
            left[u] = decide32(nd[u].w0, nd[u].w1, nd[u].w3, v[u], cat_bits);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int next = left[u] ? (int)(short)(nd[u].w2 & 0xffffu) : (int)(short)(nd[u].w2 >> 16);
        node[u] = walking[u] ? next : node[u];
      }
    }
  }
}

}  // namespace

}  // namespace mrk
