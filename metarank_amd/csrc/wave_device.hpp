// Wave-local helpers of the wave-per-section pre-pass (rank_device.hpp prepass_diversity_wave): a prefix scan by ballot and
// the commons-math LEGACY median of up to 64 values held one per lane - lanes of ONE wavefront talking through LDS in
// program order, no workgroup barrier.  Its own header so that tests/native/wave_test.cpp can compile it for the host: 64
// threads stand in for the 64 lanes, the ballot and the LDS ordering point become barriers (both are only ever reached by all
// lanes together), and the medians are compared bit for bit with a sorted-array restatement of the percentile.
#ifndef MRK_WAVE_DEVICE_HPP
#define MRK_WAVE_DEVICE_HPP

namespace mrk {

namespace {

// keeps the compiler from moving this wavefront's LDS accesses across (the LDS unit executes them in order anyway)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// exclusive prefix sum of a 0/1 flag over the wavefront + total
__device__ __forceinline__ int wave_scan_flag(bool flag, int &total) {
  const unsigned long long ball = __ballot(flag);
  total = __popcll(ball);
  return __popcll(ball & ((1ull << (threadIdx.x & 63)) - 1ull));
}

// median_of for n_raw <= 64 values, one wavefront (the rank-sort branch: one value per lane)
__device__ __forceinline__ double wave_median_of(double *s_vals, int n_raw) {
  const int lane = threadIdx.x & 63;
  if (n_raw == 1) return s_vals[0];
  const bool mine = lane < n_raw;
  const double v = mine ? s_vals[lane] : 0.0;
  const bool isn = v != v;
  const int n_nan = __popcll(__ballot(mine && isn));
  int rank = 0;
  if (mine && !isn)
    for (int j = 0; j < n_raw; ++j) {
      const double w = s_vals[j];
      rank += (w < v || (w == v && j < lane)) ? 1 : 0;
    }
  wave_lds_sync();
  if (mine && !isn) s_vals[rank] = v;
  wave_lds_sync();
  const int m = n_raw - n_nan;
  if (m <= 0) return __longlong_as_double(0x7ff8000000000000LL);
  const double pos = 0.5 * (double)(m + 1);
  const double fpos = floor(pos);
  const int ipos = (int)fpos;
  const double dif = pos - fpos;
  if (pos < 1.0) return s_vals[0];
  if (pos >= (double)m) return s_vals[m - 1];
  const double lower = s_vals[ipos - 1], upper = s_vals[ipos];
  return __dadd_rn(lower, __dmul_rn(dif, __dsub_rn(upper, lower)));
}

// ---- a request's pre-pass on all lanes of its workgroup (rank_device.hpp; tests/native/wave_seg_test.cpp runs these on the host)

// the position of the j-th (from 0) set bit of m; j < popcount(m)
__device__ __forceinline__ int wave_nth_set(unsigned long long m, int j) {
  int pos = 0;
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) {
    const int c = __popcll(m & ((1ull << w) - 1ull));   // set bits among the next w positions
    const bool up = j >= c;
    j -= up ? c : 0;
    m = up ? m >> w : m;
    pos += up ? w : 0;
  }
  return pos;
}

// wave_scan_flag by segments, turned round.  The wavefront is `segs` segments of `width` lanes (segs * width <= 64; lanes past the
// last segment belong to none) and every segment has a ballot of its own over the SAME 64 candidates - `ball` is the one of this
// lane's segment.  Lane j of a segment gets the candidate whose exclusive prefix count in that ballot is j, as long as
// j < min(limit, popcount): the first `limit` flagged candidates of each segment, in candidate order, one per lane.  -1: none.
__device__ __forceinline__ int wave_seg_source(unsigned long long ball, int lane, int width, int segs, int limit) {
  const int seg = lane / width, j = lane - seg * width;
  if (seg >= segs || j >= limit || j >= __popcll(ball)) return -1;
  return wave_nth_set(ball, j);
}

// wave_median_of by segments (same layout as wave_seg_source), in registers: lane j of a segment holds value j of its segment's
// n_raw (<= width) values - the first n_raw present values in request order - and every lane of the segment gets the segment's
// median: the LEGACY rule and the NaN removal of wave_median_of, per segment, the same bits.  No LDS: a value's rank is counted by
// reading the segment's lanes one after the other (read_lane(v, src) = lane src's v; all 64 lanes call it together), the two order
// statistics come from the lanes that hold those ranks.  Lanes of no segment get NaN.
template <typename ReadLane>
__device__ __forceinline__ double wave_seg_median_of(double v_in, int n_raw, int width, int segs, const ReadLane &read_lane) {
  const int lane = threadIdx.x & 63;
  const int seg = lane / width, j = lane - seg * width;
  const bool in = seg < segs;
  const int first = in ? seg * width : 0;
  const int n = in ? n_raw : 0;
  const bool mine = j < n;
  const double v = mine ? v_in : 0.0;
  const bool isn = v != v;
  const unsigned long long seg_lanes = (width >= 64 ? ~0ull : (1ull << width) - 1ull) << first;
  const int n_nan = __popcll(__ballot(mine && isn) & seg_lanes);
  int rank = 0;
  for (int i = 0; i < width; ++i) {   // (uniform)
    const double w = read_lane(v, first + i);
    rank += (mine && !isn && i < n && (w < v || (w == v && i < j))) ? 1 : 0;
  }
  const double v0 = read_lane(v, first);
  const int m = n - n_nan;
  const double pos = 0.5 * (double)(m + 1);
  const double fpos = floor(pos);
  const int ipos = (int)fpos;
  const double dif = pos - fpos;
  const bool edge = pos < 1.0 || pos >= (double)m;   // one order statistic, not two
  const int r_lo = pos >= (double)m ? m - 1 : (pos < 1.0 ? 0 : ipos - 1);
  const unsigned long long at_lo = __ballot(mine && !isn && rank == r_lo) & seg_lanes;
  const unsigned long long at_hi = __ballot(mine && !isn && rank == ipos) & seg_lanes;
  const double lower = read_lane(v, at_lo ? __builtin_ctzll(at_lo) : lane);
  const double upper = read_lane(v, at_hi ? __builtin_ctzll(at_hi) : lane);
  if (n == 1) return v0;
  if (m <= 0) return __longlong_as_double(0x7ff8000000000000LL);
  if (edge) return lower;
  return __dadd_rn(lower, __dmul_rn(dif, __dsub_rn(upper, lower)));
}

// The interacted_with tasks of one bounded list: (interacted item k, field u) for k < len and u < n (n <= 4 entries on the list),
// numbered u * len + k - a round of 64 consecutive tasks holds mostly one field, so its insert loop is as long as that field's
// lists - and dealt to the lanes of a wavefront one round at a time.
__device__ __forceinline__ uint32_t iw_task_rounds(uint32_t len, uint32_t n) { return (len * n + 63u) >> 6; }

__device__ __forceinline__ bool iw_task_of(uint32_t round, uint32_t lane, uint32_t len, uint32_t n, uint32_t &k, uint32_t &u) {
  const uint32_t t = round * 64u + lane;
  const bool valid = t < len * n;
  u = valid ? (t >= len ? 1u : 0u) + (t >= 2u * len ? 1u : 0u) + (t >= 3u * len ? 1u : 0u) : 0u;
  k = valid ? t - u * len : 0u;
  return valid;
}

}  // namespace

}  // namespace mrk

#endif  // MRK_WAVE_DEVICE_HPP
