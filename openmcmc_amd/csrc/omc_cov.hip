// Posterior covariance / correlation of the device store on the fp64 matrix cores (gfx950: v_mfma_f64_16x16x4_f64).
//
// What it replaces: np.cov / np.corrcoef on MCMC.store[param] of the reference (host arrays there); here the store stays on
// the device and is read where it lies: store [n_iter][C][size], seen as rows of draws.
//   pooled:    one matrix over the R = n_iter C rows, row r at r * size;
//   per chain: C matrices, chain c over its n_iter rows at (it * C + c) * size  -- "batch" b, row stride C * size.
// out[b][i][j] = sum_r (a[r][ia_i] - ma_i)(b[r][ib_j] - mb_j) / (rows - 1), two passes:
//   1. means (and variances, for the correlation) of the selected columns: omc_col_moments (omc_store_shared.hip), the pass
//      behind omc_store_moments, with or without an index;
//   2. k_cov_mfma: the tiling of k_gram_mfma (omc_gram.hip: 128 x 128 output tile per workgroup, 4 waves in 2 x 2 of
//      64 x 64 = 4 x 4 MFMA tiles, 128 accumulator registers; slab of 16 rows x 128 columns per panel, the next one fetched
//      into registers under the multiplications; LDS row stride 128 + 16), with these differences:
//      * the value is centred in fp64 as it is loaded, before it goes to LDS.  Why not sum x x' - R m m': with |mean| = t sd
//        the two terms agree in their leading log2(t^2) bits and the difference keeps eps t^2 of relative error -- 4.8e-8
//        at t = 1e3, nothing at t = 1e8.  Centred, an error d of the mean enters as R d d' (sum (x - m) = 0): second order;
//        what is left is the rounding of x - m itself, eps relative to |x - m|;
//      * a thread's eight slab elements share one column (e = q * 256 + tid, column e % 128 = tid % 128), so the column's
//        offset in the row (the index entry, or the column itself) and its mean are read once per workgroup into registers;
//        the inner loads are then the same coalesced 8-byte loads with or without an index, and a contiguous index run
//        costs what no index costs;
//      * two panels from two tensors (cross form): rectangular grid of tiles.  Symmetric form (b is a): tiles on and below the
//        diagonal only, the diagonal tile multiplies its one panel with itself and its upper-right wave (all i < j) idles;
//      * waves whose 64 x 64 block lies outside the output idle too: widths below a tile take this kernel with zero padding
//        (a 1 x n or 36 x 36 output is bound by reading the rows, not by the padded MFMAs -- DESIGN section 5);
//      * grid x = (batch, tile), y = slice of the contraction; partial tiles to the workspace;
//   3. k_cov_join adds the slices in index order (no atomics: two calls are bit-equal), divides, scales to a correlation,
//      mirrors the lower triangle in the symmetric form.
// NaN needs no code: a NaN draw makes its column's mean NaN, so every centred value of the column, so its row / column.
#include "omc_common.h"
#include "omc_store_view.h"

typedef double double4_t __attribute__((ext_vector_type(4)));

#define CV_TS 128  // output tile
#define CV_BK 16   // rows per slab
#define CV_LD (CV_TS + 16)

namespace {

// one operand: rows of a store and the columns of it that take part (the fields of its StoreView, and the means)
struct CovSide {
  const double* data;
  const int64_t* idx;  // [n] or NULL
  const double* mean;  // [batches][n]
  int64_t row_stride, batch_stride;
  int n;
};

// partial tile of one (batch, tile, slice): part[slice][batch][i][j] = sum over the slice's rows of centred a_i b_j
__global__ void __launch_bounds__(256, 2) k_cov_mfma(int64_t R, CovSide sa, CovSide sb, int symmetric, int tiles_b, int pairs,
                                                     int64_t kchunk, double* __restrict__ part) {
  __shared__ double As[CV_BK][CV_LD];
  __shared__ double Bs[CV_BK][CV_LD];
  const int64_t batch = blockIdx.x / pairs, batches = gridDim.x / pairs;
  int t = (int)(blockIdx.x - batch * pairs), bi = 0, bj;
  if (symmetric) {  // tile pair below or on the diagonal from the linear index: bi >= bj
    while (t >= bi + 1) { t -= bi + 1; ++bi; }
    bj = t;
  } else {
    bi = t / tiles_b;
    bj = t - bi * tiles_b;
  }
  const bool one_panel = symmetric && bi == bj;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int64_t kbeg = (int64_t)blockIdx.y * kchunk;
  const int64_t kend = (kbeg + kchunk < R) ? kbeg + kchunk : R;
  const int ci = bi * CV_TS, cj = bj * CV_TS;
  // this wave's 64 x 64 block holds an output entry that is read (the join reads i >= j only in the symmetric form)
  const bool wave_on = ci + wr * 64 < sa.n && cj + wc * 64 < sb.n && !(one_panel && wr < wc);

  // slab element e = q * 256 + tid : row e / 128 = 2 q + tid / 128, column e % 128 = tid % 128 for every q
  const int c = tid & 127, r_lo = tid >> 7;
  const bool oka = ci + c < sa.n, okb = !one_panel && cj + c < sb.n;
  const double* pa = sa.data;
  const double* pb = sb.data;
  double ma = 0.0, mb = 0.0;
  if (oka) {
    pa += batch * sa.batch_stride + (sa.idx ? sa.idx[ci + c] : (int64_t)(ci + c));
    ma = sa.mean[batch * sa.n + ci + c];
  }
  if (okb) {
    pb += batch * sb.batch_stride + (sb.idx ? sb.idx[cj + c] : (int64_t)(cj + c));
    mb = sb.mean[batch * sb.n + cj + c];
  }

  double4_t acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = double4_t{0.0, 0.0, 0.0, 0.0};

  // A row or column outside the slice reads as the mean, so that it is stored as zero.  The subtraction waits in stage():
  // next to the load it would need the value at once, and the loads would no longer fly under the multiplications.
  double ra[8], rb[8];
  auto fetch = [&](int64_t k0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int64_t k = k0 + 2 * q + r_lo;
      const bool rowok = k < kend;
      ra[q] = (rowok && oka) ? pa[k * sa.row_stride] : ma;
      if (!one_panel) rb[q] = (rowok && okb) ? pb[k * sb.row_stride] : mb;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      As[2 * q + r_lo][c] = ra[q] - ma;
      if (!one_panel) Bs[2 * q + r_lo][c] = rb[q] - mb;
    }
  };

  fetch(kbeg);
  for (int64_t k0 = kbeg; k0 < kend; k0 += CV_BK) {
    __syncthreads();  // the previous slab has been consumed
    stage();
    __syncthreads();
    if (k0 + CV_BK < kend) fetch(k0 + CV_BK);  // in flight under the multiplications below
    if (!wave_on) continue;
    const double(*Bp)[CV_LD] = one_panel ? As : Bs;
#pragma unroll
    for (int kk = 0; kk < CV_BK; kk += 4) {
      const int kr = kk + (lane >> 4), cl = lane & 15;
      double a[4], b[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) a[m] = As[kr][wr * 64 + m * 16 + cl];
#pragma unroll
      for (int m = 0; m < 4; ++m) b[m] = Bp[kr][wc * 64 + m * 16 + cl];
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[m][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], b[q], acc[m][q], 0, 0, 0);
    }
  }
  if (!wave_on) return;
  // C/D of the f64 form: column = lane & 15, row = (lane >> 4) + 4 * register
  double* out = part + ((int64_t)blockIdx.y * batches + batch) * sa.n * sb.n;
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = ci + wr * 64 + m * 16 + (lane >> 4) + 4 * r, j = cj + wc * 64 + q * 16 + (lane & 15);
        if (i < sa.n && j < sb.n) out[(int64_t)i * sb.n + j] = acc[m][q][r];
      }
}

// out[b][i][j] = (sum over the slices, in index order) / (rows - 1); symmetric form: of element (max(i,j), min(i,j)).
// correlation: / (sd_i sd_j) with the variances of the means pass, clipped to [-1, 1] (NaN stays NaN), NaN where a variance is
// zero, exactly 1 where both sides are the same element of the same store.
__global__ void __launch_bounds__(256) k_cov_join(int64_t batches, int n_a, int n_b, int splits, int64_t rows, int symmetric,
                                                  int correlation, const double* __restrict__ part, const double* __restrict__ var_a,
                                                  const double* __restrict__ var_b, const int64_t* __restrict__ idx_a,
                                                  const int64_t* __restrict__ idx_b, double* __restrict__ out) {
  const int64_t mat = (int64_t)n_a * n_b, total = batches * mat;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t batch = e / mat, w = e - batch * mat;
    const int i = (int)(w / n_b), j = (int)(w - (int64_t)i * n_b);
    const int64_t src = batch * mat + ((symmetric && i < j) ? (int64_t)j * n_b + i : w);
    double s = 0.0;
    for (int k = 0; k < splits; ++k) s += part[(int64_t)k * total + src];
    s = rows > 1 ? s / (double)(rows - 1) : 0.0;
    if (correlation) {
      const double vi = var_a[batch * n_a + i], vj = var_b[batch * n_b + j];
      const int64_t ei = idx_a ? idx_a[i] : i, ej = idx_b ? idx_b[j] : j;
      s = s / (sqrt(vi) * sqrt(vj));
      s = s > 1.0 ? 1.0 : (s < -1.0 ? -1.0 : s);
      if (symmetric && ei == ej && vi == vi) s = 1.0;
      if (vi == 0.0 || vj == 0.0) s = __longlong_as_double(0x7ff8000000000000LL);
    }
    out[e] = s;
  }
}

}  // namespace

extern "C" omc_status omc_store_cov(omc_ctx* ctx, int64_t n_iter, int64_t size_a, const double* store_a, const int64_t* idx_a,
                                    int64_t n_a, int64_t size_b, const double* store_b, const int64_t* idx_b, int64_t n_b,
                                    int32_t pooled, int32_t correlation, double* out) {
  if (!ctx || n_iter < 1 || size_a < 1 || !store_a || n_a < 1 || !out) return OMC_INVALID_ARG;
  const bool symmetric = store_b == nullptr;
  if (symmetric) { store_b = store_a; size_b = size_a; idx_b = idx_a; n_b = n_a; }
  if (size_b < 1 || n_b < 1 || (!idx_a && n_a != size_a) || (!idx_b && n_b != size_b)) return OMC_INVALID_ARG;
  const StoreView va = omc_store_view(ctx, n_iter, size_a, pooled != 0, store_a, idx_a, n_a);
  const StoreView vb = omc_store_view(ctx, n_iter, size_b, pooled != 0, store_b, idx_b, n_b);
  const int64_t R = va.R, batches = va.batches;
  const int64_t ta = (n_a + CV_TS - 1) / CV_TS, tb = (n_b + CV_TS - 1) / CV_TS;
  const int64_t pairs = symmetric ? ta * (ta + 1) / 2 : ta * tb;
  if (n_a > 0x7fffffffLL || n_b > 0x7fffffffLL || pairs * batches > 0x7fffffffLL) return OMC_INVALID_ARG;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  // slices of the contraction: two workgroups per CU over all (batch, tile) pairs, a slice at least a few slabs long --
  // a function of the shape and the device only
  int64_t splits = (2 * ctx->dev_cus) / (pairs * batches);
  if (splits < 1) splits = 1;
  const int64_t max_splits = (R + 4 * CV_BK - 1) / (4 * CV_BK);
  if (splits > max_splits) splits = max_splits;
  int64_t kchunk = (R + splits - 1) / splits;
  kchunk = (kchunk + CV_BK - 1) / CV_BK * CV_BK;
  splits = (R + kchunk - 1) / kchunk;
  // workspace: means and variances of both sides, the word of the index check, then the partial tiles [splits][batches][n_a][n_b]
  const size_t n_ma = (size_t)batches * n_a, n_mb = symmetric ? 0 : (size_t)batches * n_b;
  const size_t n_part = (size_t)splits * batches * n_a * n_b;
  omc_status st = omc_ensure(ctx, ctx->cov_ws, (2 * n_ma + 2 * n_mb + 1 + n_part) * sizeof(double));
  if (st != OMC_OK) return st;
  double* mean_a = ctx->cov_ws;
  double* var_a = mean_a + n_ma;
  double* mean_b = symmetric ? mean_a : var_a + n_ma;
  double* var_b = symmetric ? var_a : mean_b + n_mb;
  int32_t* bad = (int32_t*)(var_a + n_ma + 2 * n_mb);
  double* part = (double*)bad + 1;

  // an index outside the store is found before anything reads through it: one read-back for both sides
  st = omc_store_check_index(ctx, bad, idx_a, n_a, size_a, symmetric ? nullptr : idx_b, n_b, size_b);
  if (st != OMC_OK) return st;
  st = omc_col_moments(ctx, va, mean_a, var_a);
  if (st != OMC_OK) return st;
  if (!symmetric) {
    st = omc_col_moments(ctx, vb, mean_b, var_b);
    if (st != OMC_OK) return st;
  }
  const CovSide sa = {va.data, va.idx, mean_a, va.row_stride, va.batch_stride, (int)va.n};
  const CovSide sb = {vb.data, vb.idx, mean_b, vb.row_stride, vb.batch_stride, (int)vb.n};
  hipLaunchKernelGGL(k_cov_mfma, dim3((unsigned)(pairs * batches), (unsigned)splits), dim3(256), 0, s, R, sa, sb, (int)symmetric, (int)tb,
                     (int)pairs, kchunk, part);
  OMC_HIP_CHECK(hipGetLastError());
  int64_t grid = (batches * n_a * n_b + 255) / 256;
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(k_cov_join, dim3((unsigned)grid), dim3(256), 0, s, batches, (int)n_a, (int)n_b, (int)splits, R, (int)symmetric,
                     (int)(correlation != 0), part, var_a, var_b, idx_a, idx_b, out);
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}
