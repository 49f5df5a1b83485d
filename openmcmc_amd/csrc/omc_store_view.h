// How a summary sees the device store and validates a selection of it: one view, one index check, one column-moments pass.
// store is [n_iter][C][size], read where it lies as rows of draws:
//   pooled:    one set of R = n_iter C rows, row r at r * size;
//   per chain: C batches of R = n_iter rows, row r of chain c at (r * C + c) * size.
// Selected element j of the n is column idx[j] of a row (j itself without an index).
#pragma once
#include "omc_common.h"

struct StoreView {
  const double* data;
  const int64_t* idx;  // [n] or NULL
  int64_t row_stride, batch_stride, R, batches, n;

  // draw 0 of selected element j in batch b; its draw r lies r * row_stride further on
  __device__ __forceinline__ const double* column(int64_t b, int64_t j) const { return data + b * batch_stride + (idx ? idx[j] : j); }
};

inline StoreView omc_store_view(const omc_ctx* ctx, int64_t n_iter, int64_t size, bool pooled, const double* data = nullptr,
                                const int64_t* idx = nullptr, int64_t n = 0) {
  const int64_t C = ctx->n_chains;
  return StoreView{data, idx, pooled ? size : C * size, pooled ? 0 : size, pooled ? n_iter * C : n_iter, pooled ? 1 : C, idx ? n : size};
}

// omc_store_shared.hip
// One read-back for one or two selections, before anything reads through them: OMC_INVALID_ARG if an entry of idx_a lies outside
// [0, size_a) or one of idx_b outside [0, size_b).  A NULL selection passes.  word: a device word of the caller's workspace, or
// NULL for the head of ctx->store_ws.
omc_status omc_store_check_index(omc_ctx* ctx, int32_t* word, const int64_t* idx_a, int64_t n_a, int64_t size_a,
                                 const int64_t* idx_b = nullptr, int64_t n_b = 0, int64_t size_b = 0);
// the launch alone, for a caller with a read-back of its own: *word = 1 on an entry outside, else untouched
void omc_store_check_index_launch(omc_ctx* ctx, const int64_t* idx_a, int64_t n_a, int64_t size_a, const int64_t* idx_b, int64_t n_b,
                                  int64_t size_b, int32_t* word);
// mean and unbiased variance [batches][n] of the view's columns (either may be NULL); partial moments in ctx->store_ws
omc_status omc_col_moments(omc_ctx* ctx, const StoreView& v, double* mean_out, double* var_out);
