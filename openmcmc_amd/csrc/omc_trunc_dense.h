// The truncated Gibbs scan for a dense precision (omc_dense_gibbs_truncated): one kernel, two instantiations, each compiled in
// the file whose other kernels decide how the truncated-normal quantile is inlined into it -- without the per-chain diagonal in
// omc_truncated.hip (the quantile an out-of-line call with a stack frame, as in the band scan next to it), with it in
// omc_truncmix.hip (the quantile inline, no scratch: tests/test_truncated_mixture_resources.py).  Not part of the ABI.
#pragma once
#include "omc_common.h"
#include "omc_truncnorm.h"

// One wave per chain: Q_c = sum_k s_k[c] M_k (+ diag(d_c) with DIAG: the per-chain diagonal T.diag_chain of a mixture prior)
// assembled row by row on the fly, the chain's vector in LDS; d_i enters the diagonal a and the row product as d_i x_i.
template <bool DIAG>
__global__ void __launch_bounds__(64) k_dense_gibbs_truncated(int64_t C, int64_t chain_offset, int64_t p, omc_dense_terms T,
                                                              const double* rhs_chain, int64_t ld_rhs, const double* lower,
                                                              const double* upper, const double* u_in, int64_t ld_u,
                                                              omc_rng_key key, double* x, int64_t ld_x, long long* bad) {
  extern __shared__ double xs[];  // the chain's vector
  const int64_t c = blockIdx.x;
  const int lane = threadIdx.x;
  double s[OMC_MAX_TERMS];
#pragma unroll
  for (int k = 0; k < OMC_MAX_TERMS; ++k) s[k] = T.scale[k] ? T.scale[k][c] : 1.0;
  const double* dc = DIAG ? T.diag_chain + c * p : nullptr;
  for (int64_t j = lane; j < p; j += 64) xs[j] = x[c * ld_x + j];
  __syncthreads();
  bool fail = false;
  for (int64_t i = 0; i < p; ++i) {
    double dot = 0.0;
    for (int64_t j = lane; j < p; j += 64) {
      double q = 0.0;
#pragma unroll
      for (int k = 0; k < OMC_MAX_TERMS; ++k)
        if (k < T.n_terms) q = fma(s[k], T.mat[k] ? T.mat[k][i * p + j] : (i == j ? 1.0 : 0.0), q);
      if (DIAG && j == i) q += dc[i];
      dot = fma(q, xs[j], dot);
    }
    dot = omc_wave_sum(dot);
    if (lane == 0) {
      double a = 0.0, b = rhs_chain ? rhs_chain[c * ld_rhs + i] : 0.0;
#pragma unroll
      for (int k = 0; k < OMC_MAX_TERMS; ++k)
        if (k < T.n_terms) {
          a = fma(s[k], T.mat[k] ? T.mat[k][i * p + i] : 1.0, a);
          if (T.rhs[k]) b = fma(s[k], T.rhs[k][i], b);
        }
      if (DIAG) a += dc[i];
      if (!(a > 0.0)) fail = true;
      const double lo = lower ? lower[i] : -INFINITY, hi = upper ? upper[i] : INFINITY;
      double mean, sd;
      omc_trunc_site(a, b, dot, xs[i], p == 1, mean, sd);
      xs[i] = omc_truncated_normal_rv(mean, sd, lo, hi, omc_elem_uniform(u_in, c * ld_u + i, key, chain_offset + c, i));
    }
    __syncthreads();
  }
  for (int64_t j = lane; j < p; j += 64) x[c * ld_x + j] = xs[j];
  if (fail && lane == 0) atomicMin((unsigned long long*)bad, (unsigned long long)c);
}

// the launch of one instantiation for arguments that omc_dense_gibbs_truncated has checked
template <bool DIAG>
omc_status omc_trunc_dense_launch(omc_ctx* ctx, int64_t p, const omc_dense_terms* terms, const double* rhs_chain, int64_t ld_rhs,
                                  const double* lower, const double* upper, const double* u_inject, int64_t ld_u,
                                  uint64_t draw_index, double* x, int64_t ld_x) {
  const omc_dense_terms T = omc_dense_terms_clean(terms, true);  // (the kernel reads all OMC_MAX_TERMS slots)
  return omc_launch(ctx, k_dense_gibbs_truncated<DIAG>, dim3((unsigned)ctx->n_chains), dim3(64), (size_t)p * sizeof(double),
                    ctx->n_chains, ctx->chain_offset, p, T, rhs_chain, ld_rhs, lower, upper, u_inject, ld_u,
                    omc_make_key(ctx->seed, draw_index, OMC_RNG_UNIFORM), x, ld_x, ctx->d_bad_chain);
}
