// The median of a numeric `diversity` feature over more values than the pre-pass sorts in LDS (min(top, n_items) >
// PREP_MAX_VALUES; BASELINE config 4: 100 000 candidates, bench c4x: 4 M): a multi-workgroup GATHER + RADIX SELECT, every step
// ONE launch for all such (request, pre-pass entry) pairs of the batch (grid y = the entry, select.hpp SelectPlan).
// DiversityFeature.scala:113-126: the first `top` candidates in request order that hold a double - the first present cell decides
// string vs number -, NaN removed, commons-math Percentile(50) with LEGACY estimation.  Bit-exact: integer counts everywhere, so
// nothing depends on the order in which workgroups or lanes arrive.
//
//   1. take      256 lanes per 1 024-candidate tile read the tag and the bits of their candidates' (slot, item_col) cells - the only
//                random gathers - and leave the Double.compare key of every double (sort_device.hpp asc_key; NaN: its canonical key,
//                above +Infinity; no double: KEY_NONE) in `raw`, request order.  A tile publishes its count of doubles and its first
//                present (index << 8 | tag).
//   2. scan      one workgroup per entry: exclusive prefix of the tile counts (wave scans + one LDS level, 256 tiles a round with a
//                carry), the request's first present cell -> the mode.  Not a double: preset = 0, the pre-pass keeps the entry.
//   3. compact   the tiles again, now streaming `raw`: the keys of the first `top` doubles go to `keys`, in request order.  NaNs stay
//                in as the largest keys and are counted: with m = taken - NaNs, every rank below m is a non-NaN value.
//   4. select    most significant digit first, 11-bit digits (6 passes: 5 x 11 + 9 bits): a pass counts the digit of every key that
//                matches the prefix found so far in an LDS histogram (integer atomics), flushes its non-zero bins to the entry's global
//                histogram; a one-workgroup step picks the digit that holds rank k0 = ipos - 1 and the rank inside it.  Entries of up
//                to SELECT_SMALL_MAX taken values run all of it - and steps 5, 6 - in ONE workgroup and one launch instead.
//   5. tail      v[ipos] without a second select: the count of keys <= key0 and the least key above it.
//   6. finish    one lane decodes both keys, applies the LEGACY rule with unfused arithmetic (both order statistics are read even when
//                their weight is 0: 0 * Infinity is NaN on the JVM too) and writes mode / scalar / preset of the entry's PrepOut - in
//                device memory, before the pre-pass and assembly kernels of the same stream read them.
// Vector stores only, no grid-wide barrier: the launches order the passes.  Every kernel leaves at once for an entry whose request is
// not in the shard of this run, like the pre-pass.
#include <hip/hip_runtime.h>

#include "rank_launch.hpp"
#include "runtime.hpp"
#include "sort_device.hpp"

namespace mrk {

namespace {

constexpr int SEL_THREADS = 256;
constexpr int SEL_PER_LANE = SELECT_TILE / SEL_THREADS;
constexpr int SEL_ONE_THREADS = 1024;                        // the one-workgroup select
constexpr int SEL_PASSES = 6;
constexpr unsigned long long KEY_NAN = 0xfff8000000000000ull;   // asc_key of the canonical NaN: above +Infinity's 0xfff0...
constexpr unsigned long long KEY_NONE = ~0ull;                  // not a double (no key of a value: they end at KEY_NAN)
constexpr unsigned long long FIRST_NONE = ~0ull;
static_assert(SELECT_BINS == 8 * SEL_THREADS, "pick_digit: 8 bins per lane of 256");

struct SelState {
  uint32_t n_taken;    // doubles taken: min(doubles of the request, top)
  uint32_t n_nan;      // NaNs among them
  uint32_t is_double;  // the first present cell is a double and the request is in this run's shard: the entry is this file's
  uint32_t k;          // rank still to find inside the keys that match `prefix`
  unsigned long long prefix;   // the digits found so far; after the last pass: key0
  unsigned long long min_gt;   // least key above key0
  uint32_t c_le;       // keys <= key0
  uint32_t pad[3];
};
static_assert(sizeof(SelState) == SELECT_STATE_BYTES, "select.hpp sizes the state array");

struct SelectDev {
  const SelectEntry *entries;
  SelState *state;
  uint32_t *hist;                   // [entry][SELECT_BINS]
  uint32_t *tile_cnt;               // doubles per tile; after the scan: doubles before the tile
  unsigned long long *tile_first;
  unsigned long long *raw, *keys;
};

__device__ __forceinline__ bool in_shard(const BatchDev &b, const ReqDev &rq) {
  return !(rq.item_begin >= b.item_hi || rq.item_begin + rq.n_items <= b.item_lo);
}
__device__ __forceinline__ int pass_shift(int p) { return p < 5 ? 53 - 11 * p : 0; }
__device__ __forceinline__ int pass_bits(int p) { return p < 5 ? 11 : 9; }
// LEGACY: pos = 0.5 (m + 1), ipos = floor(pos); the lower order statistic is rank ipos - 1 (m <= 1: rank 0)
__device__ __forceinline__ uint32_t lower_rank(uint32_t m) { return m <= 1u ? 0u : (m + 1u) / 2u - 1u; }

// inclusive prefix sum over the wavefront
__device__ __forceinline__ uint32_t wave_inclusive(uint32_t v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}

__global__ __launch_bounds__(SEL_THREADS) void select_take_kernel(StoreDev st, ProgramDev prog, BatchDev b, SelectDev s) {
  __shared__ int s_cnt;
  __shared__ unsigned long long s_first;
  const SelectEntry en = s.entries[blockIdx.y];
  const ReqDev rq = b.reqs[en.req];
  const int tid = threadIdx.x, i0 = (int)blockIdx.x * SELECT_TILE;
  if (i0 >= rq.n_items || !in_shard(b, rq)) return;
  if (tid == 0) { s_cnt = 0; s_first = FIRST_NONE; }
  __syncthreads();
  const ColRef col = prog.prep[en.prep].item_col;
  const TableDev items = st.tab[SC_ITEM];
  int slot[SEL_PER_LANE];
#pragma unroll
  for (int j = 0; j < SEL_PER_LANE; ++j) {   // the slots, then the cells: independent loads, issued together
    const int i = i0 + j * SEL_THREADS + tid;
    slot[j] = i < rq.n_items ? b.item_slot[rq.item_begin + i] : -1;
  }
  uint32_t tag[SEL_PER_LANE];
  unsigned long long bits[SEL_PER_LANE];
#pragma unroll
  for (int j = 0; j < SEL_PER_LANE; ++j) {
    tag[j] = TAG_MISSING;
    bits[j] = 0;
    if (slot[j] >= 0 && col.tag >= 0) {
      const uint8_t *rec = items.rows + (size_t)slot[j] * items.stride;
      tag[j] = rec[col.tag];
      bits[j] = *(const unsigned long long *)(rec + col.val);
    }
  }
  int n_double = 0;
  unsigned long long first = FIRST_NONE;
#pragma unroll
  for (int j = 0; j < SEL_PER_LANE; ++j) {
    const int i = i0 + j * SEL_THREADS + tid;
    if (i >= rq.n_items) continue;
    const bool dbl = tag[j] == TAG_DOUBLE;
    s.raw[(size_t)en.raw_off + i] = dbl ? asc_key(__longlong_as_double((long long)bits[j])) : KEY_NONE;
    n_double += dbl ? 1 : 0;
    if (tag[j] != TAG_MISSING && first == FIRST_NONE) first = ((unsigned long long)i << 8) | tag[j];   // (a lane's candidates ascend with j)
  }
  if (n_double) atomicAdd(&s_cnt, n_double);
  if (first != FIRST_NONE) atomicMin(&s_first, first);
  __syncthreads();
  if (tid == 0) {
    s.tile_cnt[(size_t)en.tile_off + blockIdx.x] = (uint32_t)s_cnt;
    s.tile_first[(size_t)en.tile_off + blockIdx.x] = s_first;
  }
}

__global__ __launch_bounds__(SEL_THREADS) void select_scan_kernel(ProgramDev prog, BatchDev b, SelectDev s) {
  __shared__ uint32_t s_wave[SEL_THREADS / 64];
  __shared__ unsigned long long s_first;
  const int e = blockIdx.x;
  const SelectEntry en = s.entries[e];
  const ReqDev rq = b.reqs[en.req];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool active = in_shard(b, rq);   // uniform
  for (int d = tid; d < SELECT_BINS; d += SEL_THREADS) s.hist[(size_t)e * SELECT_BINS + d] = 0u;
  if (tid == 0) s_first = FIRST_NONE;
  __syncthreads();
  uint32_t carry = 0;
  unsigned long long first = FIRST_NONE;
  const int n_tiles = active ? (rq.n_items + SELECT_TILE - 1) / SELECT_TILE : 0;
  for (int t0 = 0; t0 < n_tiles; t0 += SEL_THREADS) {
    const int t = t0 + tid;
    const uint32_t c = t < n_tiles ? s.tile_cnt[(size_t)en.tile_off + t] : 0u;
    const unsigned long long f = t < n_tiles ? s.tile_first[(size_t)en.tile_off + t] : FIRST_NONE;
    first = f < first ? f : first;
    const uint32_t incl = wave_inclusive(c);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SEL_THREADS / 64; ++w) {
      before += w < wave ? s_wave[w] : 0u;
      total += s_wave[w];
    }
    if (t < n_tiles) s.tile_cnt[(size_t)en.tile_off + t] = carry + before + incl - c;
    carry += total;
    __syncthreads();
  }
  if (first != FIRST_NONE) atomicMin(&s_first, first);
  __syncthreads();
  if (tid == 0) {
    const uint32_t top = (uint32_t)prog.prep[en.prep].top;
    const bool dbl = s_first != FIRST_NONE && (uint32_t)(s_first & 255u) == (uint32_t)TAG_DOUBLE;
    SelState z;
    z.n_taken = carry < top ? carry : top;
    z.n_nan = 0u;
    z.is_double = dbl ? 1u : 0u;
    z.k = 0u;
    z.prefix = 0ull;
    z.min_gt = KEY_NONE;
    z.c_le = 0u;
    z.pad[0] = z.pad[1] = z.pad[2] = 0u;
    s.state[e] = z;
    // strings (or nothing at all): the existing pre-pass takes the entry
    if (active && !dbl) b.prep_out[(size_t)en.req * prog.n_prep + en.prep].preset = 0;
  }
}

__global__ __launch_bounds__(SEL_THREADS) void select_compact_kernel(ProgramDev prog, BatchDev b, SelectDev s) {
  __shared__ uint32_t s_wave[SEL_THREADS / 64];
  const int e = blockIdx.y;
  if (!s.state[e].is_double) return;
  const SelectEntry en = s.entries[e];
  const int n_items = b.reqs[en.req].n_items;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i0 = (int)blockIdx.x * SELECT_TILE;
  if (i0 >= n_items) return;
  const uint32_t top = (uint32_t)prog.prep[en.prep].top;
  uint32_t running = s.tile_cnt[(size_t)en.tile_off + blockIdx.x];
  if (running >= top) return;   // `top` was reached in an earlier tile
  unsigned long long key[SEL_PER_LANE];
#pragma unroll
  for (int j = 0; j < SEL_PER_LANE; ++j) {
    const int i = i0 + j * SEL_THREADS + tid;
    key[j] = i < n_items ? s.raw[(size_t)en.raw_off + i] : KEY_NONE;
  }
  uint32_t n_nan = 0;
#pragma unroll
  for (int j = 0; j < SEL_PER_LANE; ++j) {   // candidates j * 256 ... j * 256 + 255 of the tile: a round of the workgroup
    const bool flag = key[j] != KEY_NONE;
    const unsigned long long ball = __ballot(flag);
    if (lane == 0) s_wave[wave] = (uint32_t)__popcll(ball);
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SEL_THREADS / 64; ++w) {
      before += w < wave ? s_wave[w] : 0u;
      total += s_wave[w];
    }
    const uint32_t rank = running + before + (uint32_t)__popcll(ball & ((1ull << lane) - 1ull));
    if (flag && rank < top) {   // rank < min(top, doubles of the request) <= the entry's share of `keys`
      s.keys[(size_t)en.keys_off + rank] = key[j];
      n_nan += key[j] == KEY_NAN ? 1u : 0u;
    }
    running += total;
    __syncthreads();
  }
  if (n_nan) atomicAdd(&s.state[e].n_nan, n_nan);
}

// digit `p` of every key of keys[0, n) that matches `prefix`, counted into hist (LDS); this workgroup is part `part` of `parts`
__device__ __forceinline__ void count_digits(const unsigned long long *keys, uint32_t n, int p, unsigned long long prefix, uint32_t *hist,
                                             uint32_t part, uint32_t parts) {
  const int shift = pass_shift(p);
  const uint32_t mask = (1u << pass_bits(p)) - 1u;
  const int up = p > 0 ? pass_shift(p - 1) : 0;
  auto add = [&](unsigned long long k) {
    if (p == 0 || (k >> up) == prefix) atomicAdd(&hist[(uint32_t)(k >> shift) & mask], 1u);
  };
  const ulonglong2 *k2 = (const ulonglong2 *)keys;   // (keys_off is even: 16-byte aligned)
  const uint32_t n2 = n >> 1;
  for (uint32_t q = part * blockDim.x + threadIdx.x; q < n2; q += parts * blockDim.x) {
    const ulonglong2 v = k2[q];
    add(v.x);
    add(v.y);
  }
  if ((n & 1u) && part == 0 && threadIdx.x == 0) add(keys[n - 1]);
}

// The digit whose bin holds rank k of hist[SELECT_BINS] -> out[0], the rank inside that bin -> out[1]; the bins are left zeroed for
// the next pass.  The whole workgroup calls; lanes 0 .. 255 own 8 consecutive bins each.  k < the sum of the bins.
__device__ __forceinline__ void pick_digit(uint32_t *hist, uint32_t k, uint32_t *s_wave, uint32_t *out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool mine = tid < SEL_THREADS;
  uint32_t c[8], sum = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    c[j] = mine ? hist[tid * 8 + j] : 0u;
    sum += c[j];
  }
  const uint32_t incl = wave_inclusive(sum);
  if (mine && lane == 63) s_wave[wave] = incl;
  __syncthreads();
  if (mine) {
    uint32_t excl = incl - sum;
#pragma unroll
    for (int w = 0; w < SEL_THREADS / 64; ++w) excl += w < wave ? s_wave[w] : 0u;
    if (k >= excl && k - excl < sum) {   // one lane
      bool found = false;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (!found && k - excl < c[j]) { out[0] = (uint32_t)(tid * 8 + j); out[1] = k - excl; found = true; }
        if (!found) excl += c[j];
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) hist[tid * 8 + j] = 0u;
  }
  __syncthreads();
}

// keys <= key0 and the least key above it, over this workgroup's part of keys[0, n): into the two LDS words
__device__ __forceinline__ void count_tail(const unsigned long long *keys, uint32_t n, unsigned long long key0, uint32_t *s_le,
                                           unsigned long long *s_min, uint32_t part, uint32_t parts) {
  uint32_t le = 0;
  unsigned long long mn = KEY_NONE;
  auto see = [&](unsigned long long k) {
    le += k <= key0 ? 1u : 0u;
    mn = (k > key0 && k < mn) ? k : mn;
  };
  const ulonglong2 *k2 = (const ulonglong2 *)keys;
  const uint32_t n2 = n >> 1;
  for (uint32_t q = part * blockDim.x + threadIdx.x; q < n2; q += parts * blockDim.x) {
    const ulonglong2 v = k2[q];
    see(v.x);
    see(v.y);
  }
  if ((n & 1u) && part == 0 && threadIdx.x == 0) see(keys[n - 1]);
  if (le) atomicAdd(s_le, le);
  if (mn != KEY_NONE) atomicMin(s_min, mn);
}

// commons-math Percentile(50), LEGACY, of m values whose order statistics ipos - 1 and ipos have the keys key0 / key1
// (rank_device.hpp median_of's arithmetic)
__device__ __forceinline__ void write_median(const BatchDev &b, const ProgramDev &prog, const SelectEntry &en, uint32_t m, unsigned long long key0,
                                             unsigned long long key1) {
  double med = __longlong_as_double(0x7ff8000000000000LL);
  if (m == 1u) med = asc_value(key0);
  else if (m > 1u) {
    const double pos = 0.5 * (double)(m + 1u);
    const double dif = pos - floor(pos);
    const double lower = asc_value(key0), upper = asc_value(key1);
    med = __dadd_rn(lower, __dmul_rn(dif, __dsub_rn(upper, lower)));
  }
  PrepOut *po = &b.prep_out[(size_t)en.req * prog.n_prep + en.prep];
  po->mode = DIV_DOUBLE;
  po->scalar = med;
  po->preset = 1;
}

// the whole select of an entry with at most SELECT_SMALL_MAX taken values: one workgroup, one launch
__global__ __launch_bounds__(SEL_ONE_THREADS) void select_one_kernel(ProgramDev prog, BatchDev b, SelectDev s) {
  __shared__ uint32_t s_hist[SELECT_BINS];
  __shared__ uint32_t s_wave[SEL_THREADS / 64];
  __shared__ uint32_t s_out[2];
  __shared__ uint32_t s_le;
  __shared__ unsigned long long s_min;
  const int e = blockIdx.x, tid = threadIdx.x;
  const SelState z = s.state[e];
  if (!z.is_double || z.n_taken > SELECT_SMALL_MAX) return;
  const SelectEntry en = s.entries[e];
  const unsigned long long *keys = s.keys + en.keys_off;
  const uint32_t n = z.n_taken, m = n - z.n_nan;
  for (int d = tid; d < SELECT_BINS; d += SEL_ONE_THREADS) s_hist[d] = 0u;
  if (tid == 0) { s_le = 0u; s_min = KEY_NONE; }
  __syncthreads();
  unsigned long long prefix = 0ull;
  uint32_t k = lower_rank(m);
  const uint32_t k1 = k + 1u;
  for (int p = 0; p < SEL_PASSES; ++p) {
    count_digits(keys, n, p, prefix, s_hist, 0u, 1u);
    __syncthreads();
    pick_digit(s_hist, k, s_wave, s_out);
    prefix = (prefix << pass_bits(p)) | s_out[0];
    k = s_out[1];
    __syncthreads();   // (s_out is written again in the next pass)
  }
  count_tail(keys, n, prefix, &s_le, &s_min, 0u, 1u);
  __syncthreads();
  if (tid == 0) write_median(b, prog, en, m, prefix, s_le > k1 ? prefix : s_min);
}

// ---- the multi-workgroup form: entries with more than SELECT_SMALL_MAX taken values
__device__ __forceinline__ bool takes_many(const SelState &z) { return z.is_double && z.n_taken > SELECT_SMALL_MAX; }

__global__ __launch_bounds__(SEL_THREADS) void select_hist_kernel(SelectDev s, int p) {
  __shared__ uint32_t s_hist[SELECT_BINS];
  const int e = blockIdx.y, tid = threadIdx.x;
  const SelState z = s.state[e];
  if (!takes_many(z)) return;
  if ((size_t)blockIdx.x * SEL_THREADS * 2 >= z.n_taken) return;   // no key for this workgroup
  for (int d = tid; d < SELECT_BINS; d += SEL_THREADS) s_hist[d] = 0u;
  __syncthreads();
  count_digits(s.keys + s.entries[e].keys_off, z.n_taken, p, z.prefix, s_hist, blockIdx.x, gridDim.x);
  __syncthreads();
  for (int d = tid; d < SELECT_BINS; d += SEL_THREADS) {
    const uint32_t c = s_hist[d];
    if (c) atomicAdd(&s.hist[(size_t)e * SELECT_BINS + d], c);
  }
}

__global__ __launch_bounds__(SEL_THREADS) void select_pick_kernel(SelectDev s, int p) {
  __shared__ uint32_t s_wave[SEL_THREADS / 64];
  __shared__ uint32_t s_out[2];
  const int e = blockIdx.x;
  const SelState z = s.state[e];
  if (!takes_many(z)) return;
  const uint32_t k = p == 0 ? lower_rank(z.n_taken - z.n_nan) : z.k;
  pick_digit(s.hist + (size_t)e * SELECT_BINS, k, s_wave, s_out);
  if (threadIdx.x == 0) {
    s.state[e].prefix = (z.prefix << pass_bits(p)) | s_out[0];
    s.state[e].k = s_out[1];
  }
}

__global__ __launch_bounds__(SEL_THREADS) void select_tail_kernel(SelectDev s) {
  __shared__ uint32_t s_le;
  __shared__ unsigned long long s_min;
  const int e = blockIdx.y;
  const SelState z = s.state[e];
  if (!takes_many(z)) return;
  if ((size_t)blockIdx.x * SEL_THREADS * 2 >= z.n_taken) return;
  if (threadIdx.x == 0) { s_le = 0u; s_min = KEY_NONE; }
  __syncthreads();
  count_tail(s.keys + s.entries[e].keys_off, z.n_taken, z.prefix, &s_le, &s_min, blockIdx.x, gridDim.x);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_le) atomicAdd(&s.state[e].c_le, s_le);
    if (s_min != KEY_NONE) atomicMin(&s.state[e].min_gt, s_min);
  }
}

__global__ __launch_bounds__(64) void select_finish_kernel(ProgramDev prog, BatchDev b, SelectDev s, int n_entries) {
  const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (e >= n_entries) return;
  const SelState z = s.state[e];
  if (!takes_many(z)) return;
  const uint32_t m = z.n_taken - z.n_nan;
  write_median(b, prog, s.entries[e], m, z.prefix, z.c_le > lower_rank(m) + 1u ? z.prefix : z.min_gt);
}

}  // namespace

// `scratch`: a SelectLayout(plan) block whose entries the caller has uploaded on the same stream.  18 launches when an entry can
// take more than SELECT_SMALL_MAX values, else 4 - however many entries the batch has.
void launch_diversity_select(mrk_ctx *ctx, const StoreDev &st, const ProgramDev &prog, const BatchDev &b, const SelectPlan &plan, void *scratch) {
  if (plan.entries.empty() || b.item_hi <= b.item_lo) return;
  ScopedKernelTimer timer(ctx, "median");
  const SelectLayout lay(plan);
  uint8_t *d = (uint8_t *)scratch;
  const SelectDev s{(const SelectEntry *)(d + lay.o_entries), (SelState *)(d + lay.o_state), (uint32_t *)(d + lay.o_hist), (uint32_t *)(d + lay.o_tile_cnt),
                    (unsigned long long *)(d + lay.o_tile_first), (unsigned long long *)(d + lay.o_raw), (unsigned long long *)(d + lay.o_keys)};
  const unsigned n = (unsigned)plan.entries.size();
  const dim3 tiles((unsigned)plan.max_tiles, n), each(n);
  hipStream_t q = ctx->launch;
  hipLaunchKernelGGL(select_take_kernel, tiles, dim3(SEL_THREADS), 0, q, st, prog, b, s);
  hipLaunchKernelGGL(select_scan_kernel, each, dim3(SEL_THREADS), 0, q, prog, b, s);
  hipLaunchKernelGGL(select_compact_kernel, tiles, dim3(SEL_THREADS), 0, q, prog, b, s);
  hipLaunchKernelGGL(select_one_kernel, each, dim3(SEL_ONE_THREADS), 0, q, prog, b, s);
  if (plan.max_take > SELECT_SMALL_MAX) {
    // 4 096 keys a workgroup (8 rounds of 256 lanes x 2 keys), at most 1 024 workgroups an entry: the flush of a workgroup's
    // non-zero bins stays small next to the keys it counted
    const unsigned parts = std::min(1024u, (plan.max_take + 4095u) / 4096u);
    for (int p = 0; p < SEL_PASSES; ++p) {
      hipLaunchKernelGGL(select_hist_kernel, dim3(parts, n), dim3(SEL_THREADS), 0, q, s, p);
      hipLaunchKernelGGL(select_pick_kernel, each, dim3(SEL_THREADS), 0, q, s, p);
    }
    hipLaunchKernelGGL(select_tail_kernel, dim3(parts, n), dim3(SEL_THREADS), 0, q, s);
    hipLaunchKernelGGL(select_finish_kernel, dim3((n + 63u) / 64u), dim3(64), 0, q, prog, b, s, (int)n);
  }
  MRK_HIP(hipGetLastError());
}

}  // namespace mrk
