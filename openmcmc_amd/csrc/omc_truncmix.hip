// Truncated mixture priors: NormalNormal.sample when the parameter's MixtureParameterVector / MixtureParameterMatrix prior
// has domain limits (sampler.py:194-205 -> gmrf.gibbs_canonical_truncated_normal, gmrf.py:201-266).  Under a spike component
// the near-limit truncated-normal quantile is the common path of these scans.  This file has no other caller of it, so it is
// compiled into the two kernels below (no stack frame, no scratch: tests/test_truncated_mixture_resources.py); in
// omc_truncated.hip and omc_rj.hip, whose other kernels call it out of line, the same source takes 124 to 156 bytes of scratch a lane.
//
//   k_small_gibbs_truncated         the ragged route: Q_c = diag(prior_prec[c]) + lik_scale[c] gram[c] on the live
//                                   count[c] x count[c] block (the operator of omc_small_sample_canonical), one scan of
//                                   single-site truncated updates in natural order;
//   k_dense_gibbs_truncated<true>   the dense route with a per-chain diagonal added to Q_c (omc_trunc_dense.h).
// The domain rule of the log-density (location_scale.py:162-188) is k_diag_gauss_logpdf<true> of omc_scalar.hip.
#include <math.h>

#include "omc_common.h"
#include "omc_trunc_dense.h"
#include "omc_truncnorm.h"

namespace {

// One wave per chain, lane j = site j (kmax <= 64).  The chain's rows of Q go to LDS once; what does not depend on the state
// (Q_jj, 1/Q_jj, the conditional sd, b_j and the uniform of site j) is computed by lane j before the scan, and each site of
// the scan reads it with a scalar readlane.  Site i: the row product Q_i. x as one wave sum (every lane holds Q_ij x_j with
// the current x_j), then the truncated draw, evaluated identically in every lane (no divergence), and lane i keeps it.
// The row product is an explicit sum per site, not a running residual: it is the same butterfly as k_dense_gibbs_truncated's,
// and no rounding is carried from site to site.
__global__ void __launch_bounds__(64) k_small_gibbs_truncated(int64_t C, int64_t chain_offset, int kmax, const double* gram,
                                                              const double* gram_rhs, const double* lik_scale,
                                                              const double* prior_prec, const double* prior_mean,
                                                              const double* count, double lower, double upper,
                                                              const double* u_in, omc_rng_key key, double* x, long long* bad) {
  extern __shared__ double qs[];  // rows of Q_c: [k][kmax]
  const int64_t c = blockIdx.x;
  const int lane = threadIdx.x;
  const int k = count ? min(max((int)count[c], 0), kmax) : kmax;
  const double tau = lik_scale ? lik_scale[c] : 1.0;
  const bool on = lane < k;
  const double* g = gram + c * kmax * kmax;
  for (int i = 0; i < k; ++i) {
    double q = 0.0;
    if (on) {
      q = tau * g[i * kmax + lane];
      if (lane == i) q += prior_prec[c * kmax + lane];
    }
    if (lane < kmax) qs[i * kmax + lane] = q;  // (the buffer holds kmax x kmax: lanes >= kmax stage nothing)
  }
  double xj = on ? x[c * kmax + lane] : 0.0;
  // per-site constants of lane j: v and sd as omc_trunc_site (omc_truncnorm.h) makes them; its mean follows at the site's turn
  double a = 1.0, v = 1.0, sd = 1.0, b = 0.0, u = 0.5;
  if (on) {
    a = tau * g[lane * kmax + lane] + prior_prec[c * kmax + lane];
    b = prior_prec[c * kmax + lane] * (prior_mean ? prior_mean[c * kmax + lane] : 0.0) + tau * gram_rhs[c * kmax + lane];
    if (k == 1) {
      sd = 1.0 / sqrt(a);
    } else {
      v = 1.0 / a;
      sd = sqrt(v);
    }
    u = omc_elem_uniform(u_in, c * kmax + lane, key, chain_offset + c, lane);
  }
  const bool fail = on && !(a > 0.0);
  __syncthreads();
  for (int i = 0; i < k; ++i) {
    const double dot = omc_wave_sum((on ? qs[i * kmax + lane] : 0.0) * xj);  // Q_i. x (lanes >= k add 0)
    const double ai = omc_readlane_d(a, i), bi = omc_readlane_d(b, i), xi_old = omc_readlane_d(xj, i);
    const double vi = omc_readlane_d(v, i), sdi = omc_readlane_d(sd, i), ui = omc_readlane_d(u, i);
    // gmrf.py:255-262 (k == 1: mean = b / Q, gmrf.py:244-247)
    const double mean = (k == 1) ? bi / ai : vi * ((bi - dot) + ai * xi_old);
    // the near-limit quantile is the common path under a spike component.  The statement attribute inlines
    // omc_truncated_normal_rv and, through it, omc_truncnorm_ppf (gfx950 -O3); the tail inversion omc_ndtri_exp_lower stays
    // an out-of-line call (two call sites), with no scratch and no spilled VGPRs (24 SGPRs saved in VGPR lanes around it)
    double xi;
    [[clang::always_inline]] xi = omc_truncated_normal_rv(mean, sdi, lower, upper, ui);
    if (lane == i) xj = xi;
  }
  if (lane < kmax) x[c * kmax + lane] = on ? xj : 0.0;
  if (__ballot(fail) != 0 && lane == 0) atomicMin((unsigned long long*)bad, (unsigned long long)c);
}

}  // namespace

// the diag_chain form of omc_dense_gibbs_truncated (which validates the arguments and calls this)
omc_status omc_dense_gibbs_truncated_diag_launch(omc_ctx* ctx, int64_t p, const omc_dense_terms* terms, const double* rhs_chain,
                                                 int64_t ld_rhs, const double* lower, const double* upper,
                                                 const double* u_inject, int64_t ld_u, uint64_t draw_index, double* x,
                                                 int64_t ld_x) {
  return omc_trunc_dense_launch<true>(ctx, p, terms, rhs_chain, ld_rhs, lower, upper, u_inject, ld_u, draw_index, x, ld_x);
}

extern "C" omc_status omc_small_gibbs_truncated(omc_ctx* ctx, int64_t kmax, const double* gram, const double* gram_rhs,
                                                const double* lik_scale, const double* prior_prec, const double* prior_mean,
                                                const double* count, double lower, double upper, const double* u_inject,
                                                uint64_t draw_index, double* x) {
  if (!ctx || kmax < 1 || kmax > 64 || !gram || !gram_rhs || !prior_prec || !x || !(lower < upper)) return OMC_INVALID_ARG;
  const size_t lds = (size_t)kmax * kmax * sizeof(double);
  return omc_launch(ctx, k_small_gibbs_truncated, dim3((unsigned)ctx->n_chains), dim3(64), lds, ctx->n_chains, ctx->chain_offset,
                    (int)kmax, gram, gram_rhs, lik_scale, prior_prec, prior_mean, count, lower, upper, u_inject,
                    omc_make_key(ctx->seed, draw_index, OMC_RNG_UNIFORM), x, ctx->d_bad_chain);
}
