// The LDS bitonic network of one workgroup over (key, u16 index) pairs under pair_lt: eval.hip orders a group's scores with it,
// train.hip the same scores for the LambdaRank pass.
#pragma once
#include <hip/hip_runtime.h>

#include "sort_device.hpp"

namespace mrk {

// s_key[0, p2) (and, IDX, the indices beside them), p2 a power of two; the caller has synchronised, and is synchronised on return
template <bool IDX>
__device__ void lds_bitonic(unsigned long long *s_key, unsigned short *s_idx, int p2) {
  const int tid = threadIdx.x, T = blockDim.x;
  for (int k = 2; k <= p2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < p2; i += T) {
        const int p = i ^ j;
        if (p > i) {
          const unsigned long long ka = s_key[i], kb = s_key[p];
          const int ia = IDX ? s_idx[i] : 0, ib = IDX ? s_idx[p] : 0;
          const bool up = (i & k) == 0;
          if (up ? pair_lt(kb, ib, ka, ia) : pair_lt(ka, ia, kb, ib)) {
            s_key[i] = kb;
            s_key[p] = ka;
            if (IDX) {
              s_idx[i] = (unsigned short)ib;
              s_idx[p] = (unsigned short)ia;
            }
          }
        }
      }
      __syncthreads();
    }
}

}  // namespace mrk
