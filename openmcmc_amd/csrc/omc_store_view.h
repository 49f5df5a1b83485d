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

// what an entry point that answers a bad selection with a bare OMC_INVALID_ARG asks of it: a context, at least min_iter iterations,
// a store of rows of size >= 1, n_idx >= 1 selected elements, and without an index every element of a row
inline bool omc_selection_ok(const omc_ctx* ctx, int64_t n_iter, int64_t min_iter, int64_t size, const double* store, const int64_t* idx,
                             int64_t n_idx) {
  return ctx && n_iter >= min_iter && size >= 1 && store && n_idx >= 1 && (idx || n_idx == size);
}

// Row slices of a pass whose workgroups each own one of `groups` sets of columns and a slice of the rows: about 2048 workgroups, no
// slice shorter than 256 rows, at most 1024 slices -- a function of the shape only.  Returns the slices.
inline int64_t omc_row_slices(int64_t groups, int64_t rows, int64_t* rows_per_block) {
  int64_t slices = (2048 + groups - 1) / groups;
  if (slices > (rows + 255) / 256) slices = (rows + 255) / 256;
  if (slices < 1) slices = 1;
  if (slices > 1024) slices = 1024;
  *rows_per_block = (rows + slices - 1) / slices;
  return slices;
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
