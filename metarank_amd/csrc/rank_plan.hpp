// Which kernels a loaded batch runs: host-side arithmetic over plain values (no HIP, no mrk_batch, no mrk_model), decided ONCE
// per run by capi_rank.cpp and pinned by CPU tests (tests/test_launch_shapes_cpu.py) like the launch shapes it builds on.
#pragma once
#include "jit.hpp"
#include "launch_shape.hpp"
#include "switches.hpp"

namespace mrk {

// a loaded batch as build_batch left it
struct BatchShape {
  int n_req = 0, total_items = 0, max_items = 0;
  uint32_t fused_entries = 1;          // the largest request's pre-pass table entries (at least 1)
  int fused_vals = 1;                  // ... median values, rounded up to a power of two
  int fused_threads = 64, fused_split = 1, fused_slices = 1;   // fused_launch_shape
  bool fused_ok = false;               // a request's tables fit a workgroup's LDS
  bool compact_tables = true;          // ... and the 4-byte entries of mrk_jit_rank_cells (features.hpp compact_table_ok)
  bool overrides = false;              // per-item overrides
  bool want_matrix = false;            // the caller reads the f64 matrix
  bool normalises = false;             // a column normalised across the request (bi- / cross-encoder `norm`)
  int n_prep = 0, dim = 0;             // the program's pre-pass entries and matrix columns
};

// the fused_* half of a load's shape, from what the load counted: the largest request's table entries and median values
inline uint32_t table_entries(uint64_t max_req_entries) { return (uint32_t)std::max<uint64_t>(max_req_entries, 1); }
inline int median_vals_cap(int max_doubles) {
  int vals = 1;
  while (vals < max_doubles) vals <<= 1;
  return vals;
}
inline void fused_batch_shape(BatchShape &b, uint64_t max_req_entries, int max_doubles, const Switches &sw) {
  b.fused_entries = table_entries(max_req_entries);
  b.fused_vals = median_vals_cap(max_doubles);
  const FusedShape s = fused_launch_shape(b.n_req, b.max_items, sw.fused_threads, sw.fused_split, sw.fused_slices, sw.split_max_req);
  b.fused_split = s.split;
  b.fused_slices = s.slices;
  b.fused_threads = s.threads();
  // small requests: both phases in one workgroup, tables in LDS (<= 64 KB keeps two workgroups per CU)
  b.fused_ok = sw.rank_fused && b.n_prep <= HOST_FUSED_MAX_PREP && b.max_items <= 1024 && max_req_entries <= (1u << 20) &&
               fused_lds_bytes(b.fused_entries, b.fused_vals, b.fused_threads, HOST_QS_LDS_THR, HOST_FUSED_RT_MAX_SPLIT, true) <= 64 * 1024;
}

// what the plan reads of a model
struct ModelShape {
  bool present = false, qs_ok = false, f64 = true;   // a bit-vector image; LightGBM's f64 leaves
  uint32_t thr_cap = 0, rt_doubles = 0;              // QsDev: threshold staging doubles, resident threshold doubles
  int n_views = 0;
  size_t max_chunk_bytes = 0;                        // the tree-walk image's largest chunk
  int max_chunk_trees = 0;
};

// the model is one the walking one-request kernels are for (the serving queue: unless MRK_RANK_ONE_WALK=0)
inline bool walk_one_model(const ModelShape &m, const Switches &sw) { return m.present && sw.rank_one_walk != 0 && (!m.qs_ok || sw.scorer_walk); }

// LDS of a one-request workgroup of `threads` lanes for this model: the bit-vector kernel's (rank_one_body) or the walking one's
inline size_t one_request_lds_bytes(const ModelShape &m, bool walk, int dim, uint32_t tab_entries, int vals_cap, int threads) {
  if (!walk) return rank_one_lds_bytes(tab_entries, vals_cap, threads, m.thr_cap, m.n_views, m.f64, (size_t)m.rt_doubles * 8);
  return rank_one_walk_lds_bytes(dim, m.f64, m.max_chunk_bytes, m.max_chunk_trees, walk_leaf_trees(m.max_chunk_trees),
                                 fused_lds_bytes(tab_entries, vals_cap, threads, 0u, 0, true));
}

// A request ONE workgroup of `threads` lanes can take within `lds_cap` (mrk_rank's one-launch kernels: the batch's threads, 96 KB;
// the serving queue's slots: 512 lanes, 128 KB): at most a scorer tile of candidates, no per-item overrides, tables the
// workgroup's LDS holds.  (The walking kernel gives every candidate a lane that owns its row.)
inline bool one_workgroup_takes(const ModelShape &m, bool walk, int dim, int n_prep, int max_items, bool overrides, uint64_t max_req_entries, int vals_cap,
                                int threads, size_t lds_cap) {
  if (max_items > WALK_TILE_ROWS || overrides || n_prep > HOST_FUSED_MAX_PREP || max_req_entries > (1u << 20) || threads > 512 || (walk && threads < max_items)) return false;
  return one_request_lds_bytes(m, walk, dim, table_entries(max_req_entries), vals_cap, threads) <= lds_cap;
}

enum class RankPath {
  One,         // pre-pass + assembly + forest + ordering in ONE launch, results straight into pinned memory (rank_one_body)
  OneWalk,     // the same for a forest scored by the tree walk (rank_one_walk_body)
  FusedCells,  // a workgroup per request assembles into the scorer's binned tile; scorer; sort
  ItemCells,   // pre-pass, then item-parallel assembly into the tile (requests too large for one workgroup); scorer; sort
  Matrix,      // assembly into the f64 matrix (explain, normalised columns, models without a bit-vector image, no model); tree walk; sort
};

struct RankPlan {
  RankPath path = RankPath::Matrix;
  int kernel = JIT_NONE;      // the JIT_* kernel that carries the assembly (JIT_NONE: the interpreting kernel)
  bool items_rt = false;      // ItemCells: ask for JIT_ITEMS_RT too (the resident-table form wins where it exists)
  bool prepass = false;       // ItemCells: ... and for JIT_PREPASS
  bool keyed = false;         // the kernels are keyed by the forest's view signature
  bool whole_matrix = false;  // a shard of a normalising program assembles and normalises the WHOLE batch, then scores its slice
  // FusedCells, when `kernel` is there (its interpreting stand-in: 8-byte entries, no split sizing)
  int entry_bytes = 8;        // of a table entry: 4 in mrk_jit_rank_cells
  bool split_kernel = false;  // `kernel` is the op-split / sliced kernel, even at op split 1 and one slice
};

// batch items [lo, hi); sort: order the requests afterwards; direct: the caller reads the results through the batch's pinned
// buffer only (mrk_rank and its batching front)
inline RankPlan plan_rank(const BatchShape &b, const ModelShape &m, const Switches &sw, int lo, int hi, bool sort, bool direct) {
  RankPlan p;
  const int rows = hi - lo;
  const bool whole = lo == 0 && hi == b.total_items;
  // MRK_RANK_CELLS=0 / MRK_SCORER=walk keep the f64 matrix between assembly and scoring (A/B measurements).  A column normalised
  // across the request needs every raw value of the request before any of them can be binned: such models go through the f64
  // matrix.  A SHARD of such a model assembles and normalises the whole batch - every rank holds the whole store, and the
  // normalised column (one cosine per candidate) is the cheap part of that model - and scores its own slice: the forest is what
  // the ranks share out.  (Exchanging the raw column instead would put a collective between assembly and scoring.)
  p.whole_matrix = b.normalises && !whole;
  const bool cells = sw.rank_cells && !sw.scorer_walk && m.present && m.qs_ok && !b.want_matrix && rows > 0 && !b.normalises;
  // a handful of small requests whose caller reads pinned memory: one launch
  const bool few = sw.rank_one && direct && sort && whole && rows > 0 && b.fused_ok && b.n_req >= 1 && b.n_req <= sw.rank_one_max && b.fused_slices == 1;
  auto takes = [&](bool walk) {
    return one_workgroup_takes(m, walk, b.dim, b.n_prep, b.max_items, b.overrides, b.fused_entries, b.fused_vals, b.fused_threads, RANK_ONE_LDS_CAP);
  };
  if (cells) {
    // (the kernels that write the scorer's tile are keyed by the forest's view signature too: their sinks hold it as constants)
    p.keyed = sw.thr_stage;
    if (few && takes(false)) {
      p.path = RankPath::One;
      p.kernel = JIT_ONE;
    } else if (b.fused_ok) {
      // The plain workgroup-per-request kernel keeps its tables in 4-byte entries (table32_device.hpp): a batch with a table they
      // do not hold takes the op-split / sliced kernel at op split 1 and one slice - 8-byte entries, the same results.  Per
      // launch, not per request; no second copy of the plain kernel, no format switch inside a kernel.
      const bool plain = b.fused_split == 1 && b.fused_slices == 1 && b.compact_tables;
      p.path = RankPath::FusedCells;
      p.kernel = plain ? JIT_RANK : JIT_SPLIT;
      p.entry_bytes = plain ? 4 : 8;
      p.split_kernel = !plain;
    } else {
      p.path = RankPath::ItemCells;
      p.kernel = JIT_ITEMS;
      p.items_rt = true;
      p.prepass = b.n_prep > 0 && sw.jit_prepass;
    }
    return p;
  }
  if (few && sw.rank_one_walk == 1 && walk_one_model(m, sw) && !b.want_matrix && !b.normalises && takes(true)) {
    p.path = RankPath::OneWalk;
    p.kernel = JIT_ONE_WALK;
    return p;
  }
  // a model scored from the f64 matrix: the hot path too (the specialised matrix kernel has no op-split form: a split batch of a
  // matrix-scored model runs the interpreting kernel)
  if (b.fused_ok && m.present && b.fused_split == 1 && b.fused_slices == 1) p.kernel = JIT_MATRIX;
  return p;
}

// A values run (mrk_values, mrk_batch_run(batch, NULL) over a values program).  Small requests: ONE launch that writes rows and
// status words straight into the batch's pinned block (rank_values_body).  Anything else (requests sliced over several workgroups
// or too large for one, per-item overrides, a request-normalised column, a caller that asked for the device matrix,
// MRK_VALUES_ONE=0): the assembly launch(es) into the device matrix, fetched by a copy.
struct ValuesPlan {
  bool one = false;
  int kernel = JIT_NONE;   // JIT_VALUES, or the matrix path's JIT_MATRIX when the shape is plain
};
inline ValuesPlan plan_values(const BatchShape &b, const Switches &sw) {
  ValuesPlan p;
  p.one = sw.values_one && b.fused_ok && b.n_req >= 1 && b.total_items > 0 && b.dim > 0 && b.fused_slices == 1 && b.fused_threads <= 512 && !b.overrides &&
          !b.normalises && !b.want_matrix;
  p.kernel = p.one ? JIT_VALUES : b.fused_ok && b.fused_split == 1 && b.fused_slices == 1 ? JIT_MATRIX : JIT_NONE;
  return p;
}

}  // namespace mrk
