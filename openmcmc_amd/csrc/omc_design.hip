// Design-matrix helpers of the regression-shaped conditionals: Gram matrix, right-hand side, fitted values (fp64 MFMA GEMMs,
// own or through rocBLAS), weighted residual sums and the per-chain copy.  Reference call sites: sampler.py:89-118,183-192,
// location_scale.py:234-242.
#include <math.h>

#include "omc_blas.h"

__global__ void k_copy_rows(int64_t p, const double* src, int64_t ld_s, double* dst, int64_t ld_d) {
  const int64_t c = blockIdx.y;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p; i += (int64_t)gridDim.x * blockDim.x)
    dst[c * ld_d + i] = src[c * ld_s + i];
}

// Xw[i][j] = w[i] * X[i][j]
__global__ void k_scale_rows(int64_t n, int64_t p, const double* X, const double* w, double* out) {
  const int64_t total = n * p;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = X[i] * w[i / p];
}

__global__ void __launch_bounds__(256) k_weighted_resid_sq(int64_t n, const double* y, const double* f, int64_t ld_f,
                                                          const double* w, double* out) {
  __shared__ double red[4];
  const int64_t c = blockIdx.x;
  const double* fc = f + c * ld_f;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
    const double r = y[i] - fc[i];
    acc = fma((w ? w[i] : 1.0) * r, r, acc);
  }
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[c] = red[0] + red[1] + red[2] + red[3];
}

// for the canonical dense draw (omc_dense.hip), which copies w into mean_out
void omc_launch_copy_rows(omc_ctx* ctx, unsigned gx, int64_t p, const double* src, int64_t ld_s, double* dst, int64_t ld_d) {
  hipLaunchKernelGGL(k_copy_rows, dim3(gx, (unsigned)ctx->n_chains), dim3(256), 0, ctx->stream, p, src, ld_s, dst, ld_d);
}

extern "C" {

// X is [n][p] row-major = column-major p x n (lda = p).
omc_status omc_gram(omc_ctx* ctx, int64_t n, int64_t p, const double* X, const double* w, double* G_out) {
  if (!ctx || n < 1 || p < 1 || !X || !G_out) return OMC_INVALID_ARG;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  if (!ctx->gram_use_rocblas && p <= 46340) return omc_gram_mfma_launch(ctx, n, p, X, w, G_out);  // own fp64 MFMA kernel (omc_gram.hip)
  omc_status st = omc_ensure_blas(ctx);
  if (st != OMC_OK) return st;
  const double* B = X;
  if (w) {
    st = omc_ensure(ctx, ctx->dense_tmp, (size_t)n * p * sizeof(double));
    if (st != OMC_OK) return st;
    hipLaunchKernelGGL(k_scale_rows, dim3(omc_gx(n * p)), dim3(256), 0, ctx->stream, n, p, X, w, ctx->dense_tmp);
    OMC_HIP_CHECK(hipGetLastError());
    B = ctx->dense_tmp;
  }
  const double one = 1.0, zero = 0.0;
  OMC_BLAS_CHECK(rocblas_dgemm((rocblas_handle)ctx->blas, rocblas_operation_none, rocblas_operation_transpose,
                               (rocblas_int)p, (rocblas_int)p, (rocblas_int)n, &one, X, (rocblas_int)p, B,
                               (rocblas_int)p, &zero, G_out, (rocblas_int)p));
  return OMC_OK;
}

omc_status omc_design_rhs(omc_ctx* ctx, int64_t n, int64_t p, const double* X, const double* w, const double* y,
                          double* out) {
  if (!ctx || n < 1 || p < 1 || !X || !y || !out) return OMC_INVALID_ARG;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  omc_status st = omc_ensure_blas(ctx);
  if (st != OMC_OK) return st;
  const double* v = y;
  if (w) {
    st = omc_ensure(ctx, ctx->dense_tmp, (size_t)n * sizeof(double));
    if (st != OMC_OK) return st;
    hipLaunchKernelGGL(k_scale_rows, dim3(omc_gx(n)), dim3(256), 0, ctx->stream, n, (int64_t)1, y, w, ctx->dense_tmp);
    OMC_HIP_CHECK(hipGetLastError());
    v = ctx->dense_tmp;
  }
  const double one = 1.0, zero = 0.0;
  // out = A v with A = column-major p x n
  OMC_BLAS_CHECK(rocblas_dgemv((rocblas_handle)ctx->blas, rocblas_operation_none, (rocblas_int)p, (rocblas_int)n, &one, X,
                               (rocblas_int)p, v, 1, &zero, out, 1));
  return OMC_OK;
}

// out[c][i] = sum_s part[s][c][i]  (slices of a long contraction, added in slice order: deterministic)
__global__ void __launch_bounds__(256) k_sum_slices(int64_t n, int64_t C, int S, const double* __restrict__ part, double* __restrict__ out,
                                                    int64_t ld_out) {
  const int64_t c = blockIdx.y;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    double acc = 0.0;
    for (int s = 0; s < S; ++s) acc += part[((int64_t)s * C + c) * n + i];
    out[c * ld_out + i] = acc;
  }
}

omc_status omc_design_predict(omc_ctx* ctx, int64_t n, int64_t p, const double* X, const double* beta, int64_t ld_beta,
                              double* fitted, int64_t ld_fitted) {
  if (!ctx || n < 1 || p < 1 || !X || !beta || !fitted || ld_beta < p || ld_fitted < n) return OMC_INVALID_ARG;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  omc_status st = omc_ensure_blas(ctx);
  if (st != OMC_OK) return st;
  const double one = 1.0, zero = 0.0;
  // A short output under a long contraction (the transposed use: A'W applied to per-chain vectors of the observation space,
  // n = parameters, p = observations) leaves the library with a handful of output tiles -- 16 workgroups for 1000 x 256 x
  // 10 000, 1.6 ms.  Then the contraction is cut into slices (one strided-batched GEMM, a slice per batch entry) and the
  // slices are added in order.
  const int64_t C = ctx->n_chains;
  const int64_t tiles = ((n + 127) / 128) * ((C + 127) / 128);
  if (p >= 4096 && tiles < 128) {
    int64_t S = 256 / tiles;
    if (S > p / 512) S = p / 512;
    if (S > 64) S = 64;
    if (S >= 2) {
      const int64_t ks = p / S;  // the last slice takes the remainder in a call of its own
      st = omc_ensure(ctx, ctx->slice_buf, (size_t)S * C * n * sizeof(double));
      if (st != OMC_OK) return st;
      double* part = ctx->slice_buf;
      OMC_BLAS_CHECK(rocblas_dgemm_strided_batched((rocblas_handle)ctx->blas, rocblas_operation_transpose, rocblas_operation_none,
                                                   (rocblas_int)n, (rocblas_int)C, (rocblas_int)ks, &one, X, (rocblas_int)p,
                                                   (rocblas_stride)ks, beta, (rocblas_int)ld_beta, (rocblas_stride)ks, &zero, part,
                                                   (rocblas_int)n, (rocblas_stride)(n * C), (rocblas_int)(S - 1)));
      const int64_t k_last = p - (S - 1) * ks;
      OMC_BLAS_CHECK(rocblas_dgemm((rocblas_handle)ctx->blas, rocblas_operation_transpose, rocblas_operation_none, (rocblas_int)n,
                                   (rocblas_int)C, (rocblas_int)k_last, &one, X + (S - 1) * ks, (rocblas_int)p,
                                   beta + (S - 1) * ks, (rocblas_int)ld_beta, &zero, part + (S - 1) * n * C, (rocblas_int)n));
      int64_t gx_ = (n + 255) / 256;
      if (gx_ > 64) gx_ = 64;
      hipLaunchKernelGGL(k_sum_slices, dim3((unsigned)gx_, (unsigned)C), dim3(256), 0, ctx->stream, n, C, (int)S, part, fitted, ld_fitted);
      OMC_HIP_CHECK(hipGetLastError());
      return OMC_OK;
    }
  }
  // fitted (col-major n x C, ld = ld_fitted) = A' (n x p) * Beta (col-major p x C, ld = ld_beta)
  OMC_BLAS_CHECK(rocblas_dgemm((rocblas_handle)ctx->blas, rocblas_operation_transpose, rocblas_operation_none,
                               (rocblas_int)n, (rocblas_int)ctx->n_chains, (rocblas_int)p, &one, X, (rocblas_int)p, beta,
                               (rocblas_int)ld_beta, &zero, fitted, (rocblas_int)ld_fitted));
  return OMC_OK;
}

omc_status omc_chain_copy(omc_ctx* ctx, int64_t n, const double* src, int64_t ld_src, double* dst, int64_t ld_dst) {
  if (!ctx || n < 1 || !src || !dst || ld_src < n || ld_dst < n) return OMC_INVALID_ARG;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  if (src == dst && ld_src == ld_dst) return OMC_OK;
  unsigned g = omc_gx(n);
  if (g > 64) g = 64;
  hipLaunchKernelGGL(k_copy_rows, dim3(g, (unsigned)ctx->n_chains), dim3(256), 0, ctx->stream, n, src, ld_src, dst, ld_dst);
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}

omc_status omc_weighted_resid_sq(omc_ctx* ctx, int64_t n, const double* y, const double* fitted, int64_t ld_fitted,
                                 const double* w, double* out) {
  if (!ctx || n < 1 || !y || !fitted || ld_fitted < n || !out) return OMC_INVALID_ARG;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_weighted_resid_sq, dim3((unsigned)ctx->n_chains), dim3(256), 0, ctx->stream, n, y, fitted,
                     ld_fitted, w, out);
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}

}  // extern "C"
