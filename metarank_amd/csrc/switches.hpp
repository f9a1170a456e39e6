// Experiment switches: plain values, no HIP - launch_shape.hpp's rules read them on machines without a device.
#pragma once
#include <string>

namespace mrk {

// Experiment switches (DESIGN.md "Experiment switches"): environment variables read ONCE, when the library is first
// used - never on a launch path.  Tests and the measurement scripts that flip a switch inside one process call the
// exported mrk_debug_reload_switches() afterwards.
struct Switches {
  bool rank_fused = true;      // MRK_RANK_FUSED=0: pre-pass and assembly as separate kernels, tables in an HBM arena
  bool rank_cells = true;      // MRK_RANK_CELLS=0: keep the f64 matrix between assembly and scoring
  bool scorer_walk = false;    // MRK_SCORER=walk: the tree-walk scorer even where the bit-vector scorer applies
  int fused_threads = 0;       // MRK_FUSED_THREADS: item lanes of the fused kernel's workgroups (0: by request size)
  bool prepass_lds = true;     // MRK_PREPASS_LDS=0: the stand-alone pre-pass kernel builds its hash tables in the HBM arena
  int fused_slices = 0;        // MRK_FUSED_SLICES=n: workgroups per request of the fused kernel (0: by batch shape; 1: off)
  int fused_split = 0;         // MRK_FUSED_SPLIT=1|2|4: op split of the fused kernel's workgroups (0: 4 / 2 for batches of <= 16 requests)
  bool rank_combine = true;    // MRK_RANK_COMBINE=0: no batching front in mrk_rank
  bool rank_serve = true;      // MRK_RANK_SERVE=0: mrk_serve_rank never takes the persistent-workgroup queue (everything through mrk_rank)
  int serve_life_us = 20000;   // MRK_SERVE_LIFE_US: ... and leaves after the request it is serving once it is this old, idle or not (bounds what a hipFree on another thread waits for)
  int serve_spin_callers = 8;  // MRK_SERVE_SPIN_CALLERS: up to this many callers of the serving queue wait for their answer spinning; the ones beyond
                               // sleep through most of the device's time first (a host with a CPU quota throttles 64 spinning threads)
  int serve_sleep_extra_us = 8;   // MRK_SERVE_SLEEP_EXTRA_US: ... that sleep = the device's smoothed time per request + this
  int serve_poll_us = 4;          // MRK_SERVE_POLL_US: ... and after it looks for its answer this often instead of spinning (0: spin)
  int serve_overload_ms = 200;    // MRK_SERVE_OVERLOAD_MS: a queue with more slots than the process has CPUs sends everybody through the front for this long
                                  // once callers overflow its slots in numbers (0: never)
  int serve_idle_us = 2000;    // MRK_SERVE_IDLE_US: a serving workgroup without a request for this long leaves its CU (relaunched by the next request)
  bool rank_one = true;        // MRK_RANK_ONE=0: mrk_rank's small batches take the three-launch path instead of the one-launch kernel
  bool values_one = true;      // MRK_VALUES_ONE=0: mrk_values / values batches take the assembly launch(es) + copy instead of the one-launch values kernel
  int rank_one_walk = -1;      // MRK_RANK_ONE_WALK: forests scored by the tree walk in ONE workgroup (rank_one_walk_body).  unset: the serving queue takes them, mrk_rank keeps its three launches
                               // (its one-launch form has not been measured against them yet: LOG.md round 10); 1: mrk_rank takes the one launch too; 0: neither - as before that kernel (same-build A/B)
  int combine_max = 256;       // MRK_RANK_COMBINE_MAX
  int rank_lanes = 3;          // MRK_RANK_LANES: batches of mrk_rank's front in flight at once (1 ... 8)
  int table_load_pct = 75;     // MRK_TABLE_LOAD_PCT
  int host_threads = 0;        // MRK_HOST_THREADS (0: min(8, hardware threads))
  int jit_mode = 4;            // MRK_RANK_JIT: 0 off, 1 on (wait for the compiler), 2 require, 3 async, 4 auto (default: disk cache at once, else async)
  int jit_waves = 0;           // MRK_JIT_WAVES
  int fused_lds_min = 0;       // MRK_FUSED_LDS_MIN: least dynamic LDS the fused assembly kernel asks for (experiments: fewer resident workgroups)
  std::string jit_defines;     // MRK_JIT_DEFINES: macros prepended to the specialised kernels' source (experiments)
  bool thr_stage = true;       // MRK_THR_STAGE=0: the assembly kernels search threshold tables in global memory instead of staging them in LDS (experiments)
  bool jit_shipped = true;     // MRK_JIT_SHIPPED=0: ignore the code objects shipped next to the library (tests of the compile paths)
  bool items_lds = true;       // MRK_ITEMS_LDS=0: the item-parallel assembly kernel probes the pre-pass tables in the HBM arena even where a workgroup's request's tables fit its LDS
  // Round 6 (r06_x, native closed-loop callers of mrk_rank, same box): the one-launch kernel for combined batches of up to 128
  // requests (was 16: bigger ones took three launches + a copy) and op-split workgroups for up to 64: 188 k -> 228 k requests/s at
  // 64 callers, 315 k -> 339 k at 128, 351 k -> 397 k at 256 (the last measured with 128 / 32).
  int rank_one_max = 128;      // MRK_RANK_ONE_MAX: most requests of a batch the one-launch kernel takes (mrk_rank's combined batches)
  int split_max_req = 64;      // MRK_SPLIT_MAX_REQ: batches of up to this many small requests get op-split workgroups (launch_shape.hpp)
  bool items_rt = true;        // MRK_ITEMS_RT=0: the item-parallel kernel stages threshold tables per wavefront and column even where all of them fit in LDS (A/B of the resident-table kernel)
  int items_rt_threads = 0;    // MRK_ITEMS_RT_THREADS=256|512: lanes of the resident-table kernel's workgroups (default: by launch size)
  bool jit_sig = true;         // MRK_JIT_SIG=0: the specialised kernels are keyed by the program only and read the forest's column descriptors from memory (A/B of the view-signature folding)
  bool jit_record_regs = true; // MRK_JIT_REGS=0: the specialised kernel reads the candidate's record cell by cell instead of keeping it in registers
  std::string jit_cache_dir;   // MRK_JIT_CACHE_DIR, else $XDG_CACHE_HOME/mrk_jit, else ~/.cache/mrk_jit; "" / "off": none
  int big_sort_cap = 4096;     // MRK_BIG_SORT_CAP: pairs a bucket of the multi-workgroup sort orders in LDS (smaller: tests reach the global-memory path)
  bool jit_prepass = true;     // MRK_JIT_PREPASS=0: the stand-alone pre-pass (config 4) interprets the program even when the assembly is specialised
  int big_sort_bucket = 0;     // MRK_BIG_SORT_BUCKET: target pairs per bucket of the multi-workgroup sort (0: 1 024)
  int big_sort_tile = 0;       // MRK_BIG_SORT_TILE: candidates per workgroup of its classify / scatter passes (0: n / 512, at least 1 024)
  int qs_split = -1;           // MRK_QS_SPLIT
  int qs_kernel = 1;           // MRK_QS_KERNEL
  bool qs_byte = true;         // MRK_QS_BYTE=0: the split scorer keeps the 16-bit node test for forests that qualify for byte mode (A/B runs)
  int qs_r = 2;                // MRK_QS_R
  int walk_tile = 0;           // MRK_WALK_TILE=256: the tree-walk scorer's rows per workgroup (default: 512 where the tile fits)
  bool encoder_graph = false;  // MRK_ENCODER_GRAPH
  int encoder_skinny = 15;     // MRK_ENCODER_SKINNY
  bool encoder_packed = true;  // MRK_ENCODER_PACKED=0: padded batches for pooled / logit calls too
  int semantic_window = 4;     // MRK_SEMANTIC_WINDOW=k: mrk_index_build_texts runs windows of about k pieces in length order (rows still land in input order; measured faster); 0: input order
  bool encoder_f32_mfma = true;  // MRK_ENCODER_F32_MFMA=0: the f32 products / attention on the vector unit (the test instrument)
  int als_stage_max = 0;       // MRK_ALS_STAGE_MAX=n: the ALS sweeps stage the gathered factor rows of rows of up to n entries in LDS (0: what 16 KiB hold; smaller: tests reach the gather path)
};
const Switches &switches();
void reload_switches();

}  // namespace mrk
