// Device code of the COMPACT token -> count hash tables: the 4-byte entries the plain workgroup-per-request kernel
// (mrk_jit_rank_cells) keeps in LDS, where the tables' bytes set how many workgroups a CU holds.  Same tables as
// table_device.hpp's - bucket count cap / PROBE_W, home bucket tok_home, probe order, walked-past rule - so the same keys land
// in the same entries, ST_TABLE_FULL is raised for the same inserts and every count is the same; only the entry is narrower:
//   bits 12..31  key (token id, 1 <= id < 2^20)
//   bit  11      "an insert walked past this bucket" (on the bucket's FIRST entry only, as bit 63 of the wide form)
//   bits 0..10   count (<= 2 047)
//   0 = empty.
// The host launches the kernel only for batches whose every table fits both bounds (features.hpp compact_table_ok, capi_rank.cpp run_batch; the
// counts of a table cannot pass its insertions); nothing here checks them.
// Alignment: a table starts at an even entry (every capacity is even), that is 8 bytes, NOT 16 - so a 16-byte bucket is read as
// two 8-byte halves (one ds_read2_b64 on the device: one trip, like the wide form's four 8-byte reads of one address).
// Included after table_device.hpp (tok_home, wave_any, PROBE_W, TOK_BATCH, TableOps); compiled for the host by
// tests/native/table32_test.cpp.
#ifndef MRK_TABLE32_DEVICE_HPP
#define MRK_TABLE32_DEVICE_HPP

namespace mrk {

namespace {

constexpr uint32_t T32_KEY_SHIFT = 12;
constexpr uint32_t T32_WALKED = 1u << 11;
constexpr uint32_t T32_COUNT_MASK = T32_WALKED - 1u;   // 2 047
constexpr uint32_t T32_MAX_TOKEN = (1u << (32 - T32_KEY_SHIFT)) - 1u;

struct __attribute__((aligned(8))) T32Pair { uint32_t x, y; };

// one bucket into registers: PROBE_W / 2 8-byte reads at constant offsets from one address
__device__ __forceinline__ void table32_bucket(const uint32_t *bp, uint32_t (&e)[PROBE_W]) {
  const T32Pair *hp = (const T32Pair *)bp;
  T32Pair h[PROBE_W / 2];
#pragma unroll
  for (int k = 0; k < PROBE_W / 2; ++k) h[k] = hp[k];
#pragma unroll
  for (int k = 0; k < PROBE_W / 2; ++k) { e[2 * k] = h[k].x; e[2 * k + 1] = h[k].y; }
}

// (table_add_from of table_device.hpp, entry by entry)
__device__ __forceinline__ bool table32_add_from(uint32_t *tab, uint32_t nb, uint32_t tok, bool open, uint32_t bkt, uint32_t seen) {
  const uint32_t fresh = (tok << T32_KEY_SHIFT) | 1u;
  bool full = false;
  while (wave_any(open)) {
    uint32_t *bp = tab + bkt * (uint32_t)PROBE_W;
    uint32_t e[PROBE_W];
    table32_bucket(bp, e);
    uint32_t stop = PROBE_W;  // the FIRST entry of the bucket that holds tok or is empty
    bool at_key = false;
#pragma unroll
    for (int k = PROBE_W - 1; k >= 0; --k) {
      const uint32_t key = e[k] >> T32_KEY_SHIFT;
      if (key == tok || e[k] == 0u) { stop = (uint32_t)k; at_key = e[k] != 0u; }
    }
    const bool here = open && stop < (uint32_t)PROBE_W;
    uint32_t *at = bp + (stop < (uint32_t)PROBE_W ? stop : 0u);
    if (here && at_key) atomicAdd(at, 1u);
    const bool tried = here && !at_key;
    uint32_t prev = 0u;
    if (tried) prev = atomicCAS(at, 0u, fresh);
    const bool took = tried && prev == 0u;
    const bool same = tried && (prev >> T32_KEY_SHIFT) == tok;    // another lane put tok there in the meantime (tok >= 1: prev != 0)
    if (same) atomicAdd(at, 1u);
    const bool done = here && (at_key || took || same);
    const bool next = open && !here;
    if (MRK_TABLE_WALKED && next && !(e[0] & T32_WALKED)) atomicOr(bp, T32_WALKED);   // (the first entry of a full bucket is never empty)
    seen += next ? 1u : 0u;
    bkt = next ? (bkt + 1u == nb ? 0u : bkt + 1u) : bkt;
    full = full || (open && !done && seen >= nb);
    open = open && !done && seen < nb;
  }
  return !full;
}

// (table_get_from of table_device.hpp)
__device__ __forceinline__ uint32_t table32_get_from(const uint32_t *tab, uint32_t nb, uint32_t tok, bool open, uint32_t bkt, uint32_t seen, uint32_t res) {
  // A bucket holds a key at most once, so the entry that holds tok is the one whose bits 12..31 vanish under `^ tok << 12`: the
  // minimum of the four, when it is below 4 096, IS that entry's mark and count - one xor per entry and two three-way minimums
  // instead of a shift, a compare and two selects per entry (the first build of this form ran 17 % more VALU instructions than the
  // 8-byte tables: LOG.md round 19).  Key 0 - a lane that rides along - matches an empty entry: count 0.
  const uint32_t tk = tok << T32_KEY_SHIFT;
  for (; wave_any(open); ++seen) {
    const uint32_t *bp = tab + bkt * (uint32_t)PROBE_W;
    uint32_t e[PROBE_W];
    table32_bucket(bp, e);
    uint32_t hit = 0xffffffffu, lo = 0xffffffffu;
#pragma unroll
    for (int k = 0; k < PROBE_W; ++k) {
      hit = min(hit, e[k] ^ tk);
      lo = min(lo, e[k]);   // 0 = an empty entry
    }
    const uint32_t r2 = hit < (1u << T32_KEY_SHIFT) ? hit & T32_COUNT_MASK : 0u;
    res = open ? r2 : res;
    // found, or an empty entry, or no insert ever walked past this bucket, or every bucket seen: done
    open = open && r2 == 0u && lo != 0u && (!MRK_TABLE_WALKED || (e[0] & T32_WALKED) != 0u) && seen + 1u < nb;
    bkt = bkt + 1u == nb ? 0u : bkt + 1u;
  }
  return res;
}

__device__ __forceinline__ bool table_add(uint32_t *tab, uint32_t cap, uint32_t tok, bool want) {
  const uint32_t nb = cap / (uint32_t)PROBE_W;
  return table32_add_from(tab, nb, tok, want, tok_home(tok, nb), 0u);
}

__device__ __forceinline__ uint32_t table_get(const uint32_t *tab, uint32_t cap, uint32_t tok_in, bool want) {
  const uint32_t tok = want ? tok_in : 0u;   // a lane that rides along looks for key 0: an empty entry, count 0
  const uint32_t nb = cap / (uint32_t)PROBE_W;
  return table32_get_from(tab, nb, tok, want, tok_home(tok, nb), 0u, 0u);
}

template <> struct TableOps<uint32_t> {
  static __device__ __forceinline__ bool add(uint32_t *tab, uint32_t cap, uint32_t tok, bool want) { return table_add(tab, cap, tok, want); }
  static __device__ __forceinline__ uint32_t get(const uint32_t *tab, uint32_t cap, uint32_t tok, bool want) { return table_get(tab, cap, tok, want); }
};

}  // namespace

}  // namespace mrk

#endif  // MRK_TABLE32_DEVICE_HPP
