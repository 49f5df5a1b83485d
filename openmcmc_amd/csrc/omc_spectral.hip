// Spectral route of the dense Normal-Normal draw: Q_c = a_c I + b_c M with one shared M = V diag(ev) V', so that a draw is
// three products over all chains and one scaling kernel instead of a factorisation per chain (omc_dense.hip).  Reference call
// sites: sampler.py:176-197, gmrf.py:196,339.
#include <math.h>

#include "omc_blas.h"

// Spectral route: in the eigenbasis of the one shared matrix, Q_c = diag(d_c), d_c[i] = a_c + b_c ev[i].
//   t holds V' rhs_c on entry; on exit m_c = t / d (into `mean` if given) and y_c = m_c + z / sqrt(d) (into t);
//   logdet_c = sum log d; a non-positive d latches the chain like a failed factorisation.
__global__ void __launch_bounds__(256) k_spectral_scale(omc_dense_terms T, int kmat, int64_t p, int64_t C, const double* ev,
                                                        int64_t chain_offset, omc_rng_key key, const double* z, int64_t ld_z,
                                                        double* t, int64_t ld_t, double* mean, int64_t ld_m, double* logdet,
                                                        long long* bad) {
  __shared__ double red[4];
  const int64_t c = blockIdx.x;
  double a = 0.0, b = 0.0;
#pragma unroll
  for (int k = 0; k < OMC_MAX_TERMS; ++k) {
    if (k >= T.n_terms) continue;
    const double sk = T.scale[k] ? T.scale[k][c] : 1.0;
    if (k == kmat) b = sk;
    else a += sk;
  }
  double acc = 0.0;
  bool neg = false;
  const int64_t npairs = (p + 1) / 2;
  for (int64_t q = threadIdx.x; q < npairs; q += blockDim.x) {
    double z0, z1;
    if (z) {
      z0 = z[c * ld_z + 2 * q];
      z1 = (2 * q + 1 < p) ? z[c * ld_z + 2 * q + 1] : 0.0;
    } else {
      omc_normal_pair(omc_rng_block(key, chain_offset + c, (uint32_t)q), z0, z1);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t i = 2 * q + h;
      if (i >= p) continue;
      const double d = fma(b, ev[i], a);
      neg |= !(d > 0.0);
      const double r = 1.0 / d, m = t[c * ld_t + i] * r;
      if (mean) mean[c * ld_m + i] = m;
      t[c * ld_t + i] = fma(h ? z1 : z0, sqrt(r), m);
      acc += log(d);
    }
  }
  if (neg) atomicMin((unsigned long long*)bad, (unsigned long long)c);
  if (!logdet) return;
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) logdet[c] = red[0] + red[1] + red[2] + red[3];
}

extern "C" {

// out = in' for a p x p matrix (32 x 32 tiles through LDS): omc_dgemm_small takes its left operand untransposed
__global__ void __launch_bounds__(256) k_transpose_sq(int64_t p, const double* __restrict__ in, double* __restrict__ out) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t i0 = (int64_t)blockIdx.y * 32, j0 = (int64_t)blockIdx.x * 32;
  for (int r = ty; r < 32; r += 8)
    if (i0 + r < p && j0 + tx < p) tile[r][tx] = in[(i0 + r) * p + j0 + tx];
  __syncthreads();
  for (int r = ty; r < 32; r += 8)
    if (j0 + r < p && i0 + tx < p) out[(j0 + r) * p + i0 + tx] = tile[tx][r];
}

// The three products of the draw (V' B, V Y, V M: p x p times the p x C block of all chains) go through omc_dgemm_small, whose
// every output column is one accumulation over the contraction that does not depend on the number of columns or on the
// column's place among them: a chain's draw is then the same bits in a context of any size (chains shard over GPUs).  A
// library GEMM picks its kernel, and with it the order of summation, by the number of columns ("spectral_use_rocblas" 1
// keeps that route for cross-checks).  The products are launched with the in-workgroup split of the contraction fixed at 4
// (SPECTRAL_KSPLIT), not with the context's "mh_gemm_ksplit": that option tunes the Metropolis-Hastings steps and must not
// move this draw's bits.  omc_dgemm_small has no transposed left operand, so V' is written out once per draw into the
// workspace (p x p doubles next to the two [C][p] blocks).
// (omc_dense_spectral_sample itself sets no upper limit on p -- only the eigensolver's entry point does -- and the own
// kernel's indices are ints: beyond 46340 the library route.)
#define SPECTRAL_KSPLIT 4
static bool spectral_own_gemm(const omc_ctx* ctx, int64_t p) { return !ctx->spectral_use_rocblas && p <= 46340; }

omc_status omc_dense_spectral_prepare(omc_ctx* ctx, int64_t p, const double* M, double* V_out, double* ev_out) {
  if (!ctx || p < 1 || p > 32768 || !M || !V_out || !ev_out) return OMC_INVALID_ARG;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  omc_status st = omc_ensure_blas(ctx);
  if (st != OMC_OK) return st;
  rocblas_handle h = (rocblas_handle)ctx->blas;
  st = omc_ensure(ctx, ctx->dense_tmp, (size_t)p * sizeof(double));
  if (st != OMC_OK) return st;
  st = omc_ensure(ctx, ctx->dense_info, sizeof(int));
  if (st != OMC_OK) return st;
  OMC_HIP_CHECK(hipMemcpyAsync(V_out, M, (size_t)p * p * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  OMC_BLAS_CHECK(rocsolver_dsyevd(h, rocblas_evect_original, rocblas_fill_lower, (rocblas_int)p, V_out, (rocblas_int)p, ev_out,
                                  ctx->dense_tmp, ctx->dense_info));
  int info = 0;
  OMC_HIP_CHECK(hipMemcpyAsync(&info, ctx->dense_info, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  OMC_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (info != 0) { omc_set_error_text("omc_dense_spectral_prepare: the eigensolver did not converge"); return OMC_HIP_ERROR; }
  return OMC_OK;
}

omc_status omc_dense_spectral_sample(omc_ctx* ctx, int64_t p, const omc_dense_terms* terms, int32_t k_mat, const double* V,
                                     const double* ev, const double* rhs_chain, int64_t ld_rhs, const double* z_inject,
                                     int64_t ld_z, uint64_t draw_index, double* x_out, int64_t ld_x, double* mean_out,
                                     int64_t ld_mean, double* logdet_out) {
  if (!ctx || p < 1 || !terms || terms->n_terms < 1 || terms->n_terms > OMC_MAX_TERMS || k_mat < 0 || k_mat >= terms->n_terms)
    return OMC_INVALID_ARG;
  if (!V || !ev || !x_out || ld_x < p || (rhs_chain && ld_rhs < p) || (z_inject && ld_z < p) || (mean_out && ld_mean < p))
    return OMC_INVALID_ARG;
  if (terms->diag_chain || !terms->mat[k_mat]) return OMC_INVALID_ARG;
  for (int k = 0; k < terms->n_terms; ++k)
    if (k != k_mat && terms->mat[k]) return OMC_INVALID_ARG;  // every other term must be a scaled identity
  const int64_t C = ctx->n_chains;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  const bool own = spectral_own_gemm(ctx, p);
  omc_status st = own ? OMC_OK : omc_ensure_blas(ctx);  // (the own products need no library handle)
  if (st != OMC_OK) return st;
  rocblas_handle h = own ? nullptr : (rocblas_handle)ctx->blas;
  st = omc_ensure(ctx, ctx->dense_factor, ((size_t)2 * C * p + (own ? (size_t)p * p : 0)) * sizeof(double));
  if (st != OMC_OK) return st;
  double* W = ctx->dense_factor;       // [C][p]: V' rhs, then y
  double* Mw = W + C * p;              // [C][p]: m in the eigenbasis
  double* Vt = Mw + C * p;             // [p][p]: V' (own products only)
  const omc_dense_terms T = omc_dense_terms_clean(terms, false);
  // b_c into x_out, W = V' B  (all chains: one GEMM; [C][p] row-major = column-major p x C)
  omc_launch_dense_rhs(ctx, omc_gx(p), T, p, rhs_chain, ld_rhs, x_out, ld_x);
  OMC_HIP_CHECK(hipGetLastError());
  const double one = 1.0, zero = 0.0;
  if (own) {
    const unsigned tg = (unsigned)((p + 31) / 32);
    hipLaunchKernelGGL(k_transpose_sq, dim3(tg, tg), dim3(256), 0, ctx->stream, p, V, Vt);
    OMC_HIP_CHECK(hipGetLastError());
    st = omc_dgemm_small(ctx, (int)p, (int)C, Vt, p, x_out, ld_x, (int)p, nullptr, 0, nullptr, 0, 0, 0, nullptr, W, p, nullptr,
                         SPECTRAL_KSPLIT);
    if (st != OMC_OK) return st;
  } else {
    OMC_BLAS_CHECK(rocblas_dgemm(h, rocblas_operation_transpose, rocblas_operation_none, (rocblas_int)p, (rocblas_int)C, (rocblas_int)p,
                                 &one, V, (rocblas_int)p, x_out, (rocblas_int)ld_x, &zero, W, (rocblas_int)p));
  }
  hipLaunchKernelGGL(k_spectral_scale, dim3((unsigned)C), dim3(256), 0, ctx->stream, T, (int)k_mat, p, C, ev, ctx->chain_offset,
                     omc_make_key(ctx->seed, draw_index, OMC_RNG_NORMAL), z_inject, ld_z, W, p, mean_out ? Mw : nullptr, p,
                     logdet_out, ctx->d_bad_chain);
  OMC_HIP_CHECK(hipGetLastError());
  if (own) {
    st = omc_dgemm_small(ctx, (int)p, (int)C, V, p, W, p, (int)p, nullptr, 0, nullptr, 0, 0, 0, nullptr, x_out, ld_x, nullptr,
                         SPECTRAL_KSPLIT);
    if (st != OMC_OK || !mean_out) return st;
    return omc_dgemm_small(ctx, (int)p, (int)C, V, p, Mw, p, (int)p, nullptr, 0, nullptr, 0, 0, 0, nullptr, mean_out, ld_mean, nullptr,
                           SPECTRAL_KSPLIT);
  }
  OMC_BLAS_CHECK(rocblas_dgemm(h, rocblas_operation_none, rocblas_operation_none, (rocblas_int)p, (rocblas_int)C, (rocblas_int)p, &one,
                               V, (rocblas_int)p, W, (rocblas_int)p, &zero, x_out, (rocblas_int)ld_x));
  if (mean_out)
    OMC_BLAS_CHECK(rocblas_dgemm(h, rocblas_operation_none, rocblas_operation_none, (rocblas_int)p, (rocblas_int)C, (rocblas_int)p, &one,
                                 V, (rocblas_int)p, Mw, (rocblas_int)p, &zero, mean_out, (rocblas_int)ld_mean));
  return OMC_OK;
}

}  // extern "C"
