// Sort keys of the ordering kernels (rank.hip: requests of <= SORT_MAX_ITEMS candidates in one workgroup; bigsort.hip:
// larger ones).  Reference: ml/Ranker.scala:52-67 (`sortBy(-_.score)`: stable, java.lang.Double.compare on the negated
// score) and ml/onnx/Normalize.scala:25-40 (ascending Ordering.Double).
#pragma once
#ifndef MRK_SORT_HOST   // (tests/native/sort_wave_test.cpp compiles sort_wave_step for the host, with stand-ins of its own)
#include <hip/hip_runtime.h>
#endif

#include <cstdint>

namespace mrk {

// unsigned keys whose integer order is java.lang.Double.compare's order of the doubles
__device__ __forceinline__ unsigned long long asc_key(double v) {
  unsigned long long bits = (unsigned long long)__double_as_longlong(v);
  if (v != v) bits = 0x7ff8000000000000ULL;  // Double.compare canonicalises NaN: above +Infinity
  return (bits & 0x8000000000000000ULL) ? ~bits : (bits | 0x8000000000000000ULL);
}
__device__ __forceinline__ double asc_value(unsigned long long key) {
  const unsigned long long bits = (key & 0x8000000000000000ULL) ? (key & 0x7fffffffffffffffULL) : ~key;
  return __longlong_as_double((long long)bits);
}
// sortBy(-_.score): ascending Double.compare on the negated score (NaN last, +0.0 before -0.0)
__device__ __forceinline__ unsigned long long sort_key(double score) { return asc_key(-score); }

__device__ __forceinline__ bool pair_lt(unsigned long long ka, int ia, unsigned long long kb, int ib) {
  return ka < kb || (ka == kb && ia < ib);
}

// The wavefront-per-request ordering (rank.hip sort_wave_kernel; requests of <= SORT_WAVE_MAX candidates): lane l holds the keys
// of candidates l and l + 64 (i0, i1) and counts, for both, the candidates that precede them in the stable order.  One step of
// that count: candidate j's key kj, broadcast to every lane, against the lane's two.  (key, index) pairs are distinct, so a
// candidate's count over j = 0 .. n - 1 IS its position (sort_kernel's rule).
constexpr int SORT_WAVE_MAX = 128;
struct SortWaveStep { int lo, hi; };   // increments of the lane's two counters
__host__ __device__ __forceinline__ SortWaveStep sort_wave_step(unsigned long long mine0, int i0, unsigned long long mine1, int i1, unsigned long long kj, int j) {
  return SortWaveStep{(kj < mine0 || (kj == mine0 && j < i0)) ? 1 : 0, (kj < mine1 || (kj == mine1 && j < i1)) ? 1 : 0};
}

// what the multi-workgroup sort orders: element i of a request is vals[i * stride] (negate: by descending score, else
// ascending), or - the sample arrays of its own recursion - a ready-made key raw[i]
struct SortSrc {
  const double *vals;
  const unsigned long long *raw;
  long long stride;
  int negate;
};
__device__ __forceinline__ unsigned long long src_key(const SortSrc &s, int i) {
  if (s.raw) return s.raw[i];
  const double v = s.vals[(long long)i * s.stride];
  return s.negate ? sort_key(v) : asc_key(v);
}

}  // namespace mrk
