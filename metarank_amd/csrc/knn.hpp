// Exact similar-items index on the device (knn.hip): the table, its scratch and the launches capi_index.cpp drives.
#pragma once
#include "runtime.hpp"

namespace mrk {

// The embedding table in HBM.  Rows are cut into blocks of 64 (one wavefront's lanes); inside a block the dimensions are cut
// into groups of G = 16 / elem_bytes (4 floats or 2 doubles) and stored group-major, lane-minor:
//   element (row r, dimension d) = vals[((r / 64) * groups + d / G) * 64 * G + (r % 64) * G + d % G]
// so lane l of a wavefront reads its row's group g with ONE 16-byte load and the 64 lanes' loads are 1 KiB of consecutive
// bytes.  Rows past `rows` in the last block and dimensions past `cols` in the last group are zero and never enter a sum.
struct KnnTable {
  DevBuf d_vals;
  DevBuf d_snv;          // sqrt(nrv) per row, f64
  int64_t rows = 0, n_blocks = 0;
  int cols = 0, elem_bytes = 8, groups = 0;
  size_t vals_bytes() const { return (size_t)n_blocks * groups * 64 * 16; }
};

struct KnnScratch {
  DevBuf keys;                  // queries of one launch x rows: Double.compare keys of the distances
  DevBuf cand_keys, cand_rows;  // per query and segment the n best
  DevBuf snu;                   // sqrt(nru) per query
};

void knn_table_alloc(KnnTable &t, int64_t rows, int cols, int elem_bytes, hipStream_t stream);
// rows [row0, row0 + n) of the table from a row-major device copy of the caller's values (src_elem_bytes 4 / 8)
void knn_pack(KnnTable &t, const void *d_src, int src_elem_bytes, int64_t row0, int64_t n, hipStream_t stream);
// OnnxBiEncoder.avgpool of n packed sequences straight into the table (f32 storage, cols a multiple of 4): d_x is the encoder's
// hidden states [M, cols], d_cu the n + 1 token offsets; sequence b becomes row d_dst_row[b], or row0 + b when d_dst_row is null
void knn_pool_pack(KnnTable &t, const float *d_x, const int32_t *d_cu, const int64_t *d_dst_row, int64_t row0, int n, hipStream_t stream);
void knn_norms(KnnTable &t, hipStream_t stream);
// d_out[i * cols + d] = the stored value (row d_rows[i], dimension d) widened to f64
void knn_fetch_rows(const KnnTable &t, const int64_t *d_rows, int n, double *d_out, hipStream_t stream);
// most queries one knn_search call takes for a table of this many rows (its key scratch stays under 256 MiB where it can)
int knn_query_chunk(int64_t rows);
// the n (1 <= n <= min(rows, KNN_MAX_N)) nearest rows of each of nq (<= knn_query_chunk) queries: d_out_rows / d_out_dist are
// nq x n, ascending by (Double.compare(distance), row)
void knn_search(mrk_ctx *ctx, const KnnTable &t, KnnScratch &s, const double *d_queries, int nq, int n, int32_t *d_out_rows,
                double *d_out_dist);

}  // namespace mrk

struct mrk_index;

namespace mrk {

// capi_index.cpp: an ordinary index whose rows are the rows x cols f64 matrix at d_values (row-major, on the context's device),
// stored as f64 under ids[r]; the rows are cut into the table's blocks by knn_pack on ctx->stream and never visit the host.
// MRK_ERR_INVALID_ARG for a shape outside mrk_index_build's limits or a duplicate id.  Caller holds ctx->mu.
mrk_index *index_from_device_f64(mrk_ctx *ctx, const char *const *ids, const double *d_values, int64_t rows, int cols);

}  // namespace mrk
