// The plan of a batch's device medians (select.hip): which (request, numeric-diversity pre-pass entry) pairs take the
// gather + radix-select kernels, and where each keeps its scratch.  Plain values, no HIP: features.cpp fills it while it resolves
// a batch, capi_rank.cpp sizes and uploads it with the batch's other buffers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mrk {

constexpr int SELECT_TILE = 1024;          // candidates a workgroup of the take / compaction passes covers
constexpr int SELECT_BINS = 2048;          // 11-bit digits (8 KB of LDS cost no occupancy, and 8-bit digits need 8 passes over the keys instead of 6)
// Taken values up to which ONE workgroup runs every pass of the select in a single launch.  Arithmetic, not a measurement: a CU reads
// about 64 B a clock from L2, so 32 768 keys (256 KB) stream in ~2 us and the seven passes in ~15 us - what the 14 launches of the
// multi-workgroup form cost in launch gaps alone (~4 us each) before they move a byte.
constexpr uint32_t SELECT_SMALL_MAX = 32768;
constexpr int SELECT_MAX_ENTRIES = 65535;  // entries are the y dimension of every launch

// one (request, pre-pass entry) with min(top, n_items) > PREP_MAX_VALUES; offsets in elements of the scratch arrays
struct SelectEntry {
  int32_t req, prep;
  uint32_t tile_off;   // first of its ceil(n_items / SELECT_TILE) tile partials
  uint32_t raw_off;    // first of its n_items gathered keys (even: 16-byte loads)
  uint32_t keys_off;   // first of its min(top, n_items) taken keys (even)
  uint32_t pad;
};

struct SelectPlan {
  std::vector<SelectEntry> entries;
  uint64_t tiles = 0, raw = 0, keys = 0;   // totals of the three arrays
  int max_tiles = 0;                       // of any entry
  uint32_t max_take = 0;                   // largest min(top, n_items): decides whether the multi-workgroup passes are launched at all
  void clear() { entries.clear(); tiles = raw = keys = 0; max_tiles = 0; max_take = 0; }
  void add(int32_t req, int32_t prep, int n_items, int top) {
    const uint32_t take = (uint32_t)(top < n_items ? top : n_items);
    const int n_tiles = (n_items + SELECT_TILE - 1) / SELECT_TILE;
    entries.push_back({req, prep, (uint32_t)tiles, (uint32_t)raw, (uint32_t)keys, 0u});
    tiles += (uint64_t)n_tiles;
    raw += ((uint64_t)n_items + 1) & ~1ull;
    keys += ((uint64_t)take + 1) & ~1ull;
    if (n_tiles > max_tiles) max_tiles = n_tiles;
    if (take > max_take) max_take = take;
  }
  bool fits() const { return entries.size() <= (size_t)SELECT_MAX_ENTRIES && tiles <= 0xffffffffull && raw <= 0xffffffffull && keys <= 0xffffffffull; }
};

constexpr size_t SELECT_STATE_BYTES = 48;   // select.hip SelState

// the scratch block: [entries][state][histograms][tile counts][tile firsts][raw keys][taken keys], each at a multiple of 256 bytes
struct SelectLayout {
  size_t o_entries, o_state, o_hist, o_tile_cnt, o_tile_first, o_raw, o_keys, bytes;
  explicit SelectLayout(const SelectPlan &p) {
    size_t off = 0;
    auto place = [&](size_t n) { size_t o = off; off = (off + n + 255) / 256 * 256; return o; };
    const size_t e = p.entries.size();
    o_entries = place(e * sizeof(SelectEntry));
    o_state = place(e * SELECT_STATE_BYTES);
    o_hist = place(e * SELECT_BINS * 4);
    o_tile_cnt = place((size_t)p.tiles * 4);
    o_tile_first = place((size_t)p.tiles * 8);
    o_raw = place((size_t)p.raw * 8);
    o_keys = place((size_t)p.keys * 8);
    bytes = off;
  }
};

}  // namespace mrk
