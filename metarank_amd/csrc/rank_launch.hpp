// The host-callable launch and view functions of the rank side's device code, declared once: the .hip file that defines one includes
// this header (a signature that drifts is a compile error there), and so does every file that calls one.
#pragma once
#include "device_types.hpp"
#include "qs_device.hpp"
#include "rank.hpp"
#include "runtime.hpp"
#include "sort_device.hpp"   // SortSrc

namespace mrk {

// rank.hip
void launch_prepass(mrk_ctx *ctx, const StoreDev &st, const ProgramDev &prog, const BatchDev &b, uint32_t max_req_entries, void *jit_fn);
void launch_assemble(mrk_ctx *ctx, const StoreDev &st, const ProgramDev &prog, const BatchDev &b);
void launch_sort(mrk_ctx *ctx, const BatchDev &b, int max_items);
void launch_status_or(hipStream_t stream, const int32_t *all, int world, int n_req, int32_t *status);
void launch_normalize(mrk_ctx *ctx, const BatchDev &b, int dim, int col, int mode);
void launch_normalize_big(mrk_ctx *ctx, const BatchDev &b, int dim, int col, int item_begin, int n, int *order, void *scratch);
void launch_assemble_cells(mrk_ctx *ctx, const StoreDev &st, const ProgramDev &prog, const BatchDev &b, const QsDev &q,
                           uint16_t *cells, bool f64, void *jit_fn, uint32_t max_req_entries, void *jit_rt_fn = nullptr, uint32_t thr_total = 0);
size_t launch_rank_fused(mrk_ctx *ctx, const StoreDev &st, const ProgramDev &prog, const BatchDev &b, uint32_t tab_entries,
                         int vals_cap, int threads, int op_split, int slices, const QsDev *q, uint16_t *cells, bool f64, void *jit_fn, size_t rt_bytes = 0,
                         int entry_bytes = 8, bool split_kernel = false);
void launch_rank_serve(mrk_ctx *ctx, hipStream_t stream, const StoreDev &st, const ProgramDev &prog, const QsDev &q, const QsForestDev &f, const ServeGangDev &gang,
                       int n_slots, int threads, size_t lds, bool f64, void *jit_fn);
void launch_rank_one(mrk_ctx *ctx, const StoreDev &st, const ProgramDev &prog, const BatchDev &b, uint32_t tab_entries, int vals_cap,
                     int threads, int op_split, const QsDev &q, const QsForestDev &f, const OneOut &out, bool f64, void *jit_fn);
void launch_rank_one_walk(mrk_ctx *ctx, const StoreDev &st, const ProgramDev &prog, const BatchDev &b, uint32_t tab_entries, int vals_cap,
                          int threads, int op_split, const WalkDev &w, const OneOut &out, bool f64, size_t lds, void *jit_fn);
void launch_rank_values(mrk_ctx *ctx, const StoreDev &st, const ProgramDev &prog, const BatchDev &b, uint32_t tab_entries, int vals_cap,
                        int threads, int op_split, const ValuesOut &out, void *jit_fn);
void launch_rank_serve_walk(mrk_ctx *ctx, hipStream_t stream, const StoreDev &st, const ProgramDev &prog, const WalkDev &w, const ServeGangDev &gang,
                            int n_slots, int threads, size_t lds, bool f64, void *jit_fn);
// bigsort.hip
void launch_big_sort(mrk_ctx *ctx, hipStream_t stream, const SortSrc &src, int n, int *out_order, void *scratch);
size_t big_sort_scratch_bytes(int n);
// score.hip
void launch_score_batch(mrk_ctx *ctx, mrk_model *m, const double *d_x, int rows, int cols, double *d_out,
                        int *d_status, const uint32_t *d_row_req);
// score_qs.hip
QsDev qs_device_view(const mrk_model *m);
QsForestDev qs_forest_view(const mrk_model *m);
// resolve.hip
void launch_resolve_ids(hipStream_t stream, const IdTableDev &tab, const uint8_t *d_bytes, const uint32_t *d_offs, uint32_t bytes_len, const ReqDev *d_reqs,
                        int n_req, int total, int32_t *d_item_slot, uint32_t *d_item_req, int32_t *d_load_status);

}  // namespace mrk
