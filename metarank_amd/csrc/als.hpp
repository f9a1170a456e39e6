// The eALS iterations on the device (als.hip): the launches capi_als.cpp drives.  DESIGN.md section 17.
#pragma once
#include "runtime.hpp"

namespace mrk {

constexpr int ALS_GRAM_CHUNK = 512;   // rows per chunk of a K x K product: part of the stated order of summation, not a tuning knob

// one side of a sweep: the rows that are updated (`self`), their entries, and the matrix the entries point into (`other`)
struct AlsSide {
  const int32_t *d_off = nullptr, *d_idx = nullptr, *d_order = nullptr;   // rows + 1 offsets, entries, rows by descending length
  const double *d_entry_wc = nullptr;   // user side: w - c_i per entry (CSR order); item side: null (w - c_i is the row's)
  int64_t rows = 0;
};

// entries of a row whose gathered factor rows are staged in LDS (MRK_ALS_STAGE_MAX, else what 16 KiB hold; always >= 1)
int als_stage_rows(int K);
// bytes of the chunk partials a product over `rows` rows needs
size_t als_gram_scratch_bytes(int64_t rows, int K);
// d_S[f * K + k] = sum over rows r of (c_r *) (M[r][f] * M[r][k]); d_conf null: unweighted
void als_launch_gram(mrk_ctx *ctx, hipStream_t s, const char *timer, const double *d_M, const double *d_conf, int64_t rows, int K, double *d_partial,
                     double *d_S);
// one sweep: every row of `self` is re-solved against `other`, d_S = the product over `other`'s rows; d_conf = c_i per item;
// d_rhat: one double per entry.  item_side: the rows are items (the update weighs the S terms by the row's c_i)
void als_launch_sweep(mrk_ctx *ctx, hipStream_t s, bool item_side, const AlsSide &side, double *d_self, const double *d_other, const double *d_S,
                      const double *d_conf, double lambda, int K, double *d_rhat);

}  // namespace mrk
