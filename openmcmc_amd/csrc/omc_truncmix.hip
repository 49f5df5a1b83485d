// Truncated mixture priors: NormalNormal.sample when the parameter's MixtureParameterVector / MixtureParameterMatrix prior
// has domain limits (sampler.py:194-205 -> gmrf.gibbs_canonical_truncated_normal, gmrf.py:201-266), and the domain rule
// of its log-density (location_scale.py:162-188).  Kept apart from omc_truncated.hip and omc_rj.hip so that the object
// code of their kernels does not change.
//
//   k_small_gibbs_truncated        the ragged route: Q_c = diag(prior_prec[c]) + lik_scale[c] gram[c] on the live
//                                  count[c] x count[c] block (the operator of omc_small_sample_canonical), one scan of
//                                  single-site truncated updates in natural order;
//   k_dense_gibbs_truncated_diag   the dense route: k_dense_gibbs_truncated with a per-chain diagonal added to Q_c;
//   k_diag_gauss_logpdf_limits     k_diag_gauss_logpdf (omc_scalar.hip) with -inf for a chain that has a LIVE element
//                                  outside scalar limits.
#include <math.h>

#include "omc_common.h"
#include "omc_truncnorm.h"

static inline unsigned grid1(int64_t n, int block) { return (unsigned)((n + block - 1) / block); }

namespace {

// v of lane i (i wave-uniform) in every lane, through two scalar reads
__device__ __forceinline__ double readlane_d(double v, int i) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, i);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), i);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// sum over the wave, butterfly order: lanes l and l^sh add the same two values, so every lane ends with the same bits
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int sh = 32; sh > 0; sh >>= 1) v += __shfl_xor(v, sh, 64);
  return v;
}

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
  // per-site constants of lane j
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
    if (u_in) {
      u = u_in[c * kmax + lane];
    } else {
      const uint4 w = omc_rng_block(key, chain_offset + c, (uint32_t)(lane >> 1));
      u = (lane & 1) ? omc_u53(w.z, w.w) : omc_u53(w.x, w.y);
    }
  }
  const bool fail = on && !(a > 0.0);
  __syncthreads();
  for (int i = 0; i < k; ++i) {
    const double dot = wave_sum((on ? qs[i * kmax + lane] : 0.0) * xj);  // Q_i. x (lanes >= k add 0)
    const double ai = readlane_d(a, i), bi = readlane_d(b, i), xi_old = readlane_d(xj, i);
    const double vi = readlane_d(v, i), sdi = readlane_d(sd, i), ui = readlane_d(u, i);
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

// k_dense_gibbs_truncated (omc_truncated.hip) with Q_c = sum_k s_k[c] M_k + diag(d_c): d_i enters the diagonal a and the
// row product as d_i x_i.  One wave per chain, the chain's vector in LDS.
__global__ void __launch_bounds__(64) k_dense_gibbs_truncated_diag(int64_t C, int64_t chain_offset, int64_t p, int n_terms,
                                                                   const double* m0, const double* m1, const double* m2,
                                                                   const double* m3, const double* s0, const double* s1,
                                                                   const double* s2, const double* s3, const double* r0,
                                                                   const double* r1, const double* r2, const double* r3,
                                                                   const double* diag_chain, const double* rhs_chain,
                                                                   int64_t ld_rhs, const double* lower, const double* upper,
                                                                   const double* u_in, int64_t ld_u, omc_rng_key key, double* x,
                                                                   int64_t ld_x, long long* bad) {
  extern __shared__ double xs[];
  const int64_t c = blockIdx.x;
  const int lane = threadIdx.x;
  const double* M[4] = {m0, m1, m2, m3};
  const double* R[4] = {r0, r1, r2, r3};
  double s[4] = {s0 ? s0[c] : 1.0, s1 ? s1[c] : 1.0, s2 ? s2[c] : 1.0, s3 ? s3[c] : 1.0};
  const double* dc = diag_chain + c * p;
  for (int64_t j = lane; j < p; j += 64) xs[j] = x[c * ld_x + j];
  __syncthreads();
  bool fail = false;
  for (int64_t i = 0; i < p; ++i) {
    double dot = 0.0;
    for (int64_t j = lane; j < p; j += 64) {
      double q = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < n_terms) q = fma(s[k], M[k] ? M[k][i * p + j] : (i == j ? 1.0 : 0.0), q);
      if (j == i) q += dc[i];
      dot = fma(q, xs[j], dot);
    }
    dot = wave_sum(dot);
    if (lane == 0) {
      double a = 0.0, b = rhs_chain ? rhs_chain[c * ld_rhs + i] : 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < n_terms) {
          a = fma(s[k], M[k] ? M[k][i * p + i] : 1.0, a);
          if (R[k]) b = fma(s[k], R[k][i], b);
        }
      a += dc[i];
      if (!(a > 0.0)) fail = true;
      const double lo = lower ? lower[i] : -INFINITY, hi = upper ? upper[i] : INFINITY;
      double mean, sd;
      if (p == 1) {
        mean = b / a;
        sd = 1.0 / sqrt(a);
      } else {
        const double v = 1.0 / a;
        sd = sqrt(v);
        mean = v * ((b - dot) + a * xs[i]);
      }
      double u;
      if (u_in) {
        u = u_in[c * ld_u + i];
      } else {
        const uint4 w = omc_rng_block(key, chain_offset + c, (uint32_t)(i >> 1));
        u = (i & 1) ? omc_u53(w.z, w.w) : omc_u53(w.x, w.y);
      }
      xs[i] = omc_truncated_normal_rv(mean, sd, lo, hi, u);
    }
    __syncthreads();
  }
  for (int64_t j = lane; j < p; j += 64) x[c * ld_x + j] = xs[j];
  if (fail && lane == 0) atomicMin((unsigned long long*)bad, (unsigned long long)c);
}

// k_diag_gauss_logpdf (omc_scalar.hip), same sums in the same order, and -inf for a chain with a live x_j < lower or
// x_j > upper (entries at and beyond count[c] are not looked at).  One wave per chain, four chains per block.
__global__ void __launch_bounds__(256) k_diag_gauss_logpdf_limits(int64_t C, int64_t kmax, const double* x, const double* mean,
                                                                  const double* prec, const double* count, double lower,
                                                                  double upper, double* out, int accumulate) {
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (c >= C) return;
  const int64_t k = count ? (int64_t)count[c] : kmax;
  double ld = 0.0, q = 0.0;
  bool outside = false;
  for (int64_t j = lane; j < k; j += 64) {
    const double d = prec[c * kmax + j];
    const double xv = x[c * kmax + j];
    const double r = xv - (mean ? mean[c * kmax + j] : 0.0);
    ld += log(d);
    q = fma(d * r, r, q);
    outside = outside || xv < lower || xv > upper;
  }
  ld = wave_sum(ld);
  q = wave_sum(q);
  const double lp = __ballot(outside) != 0 ? -INFINITY : 0.5 * (ld - (double)k * 1.8378770664093453 - q);
  if (lane == 0) out[c] = accumulate ? out[c] + lp : lp;
}

}  // namespace

// the diag_chain form of omc_dense_gibbs_truncated (which validates the arguments and calls this)
omc_status omc_dense_gibbs_truncated_diag_launch(omc_ctx* ctx, int64_t p, const omc_dense_terms* terms, const double* rhs_chain,
                                                 int64_t ld_rhs, const double* lower, const double* upper,
                                                 const double* u_inject, int64_t ld_u, uint64_t draw_index, double* x,
                                                 int64_t ld_x) {
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  const double *m[4] = {0, 0, 0, 0}, *s[4] = {0, 0, 0, 0}, *r[4] = {0, 0, 0, 0};
  for (int k = 0; k < terms->n_terms; ++k) { m[k] = terms->mat[k]; s[k] = terms->scale[k]; r[k] = terms->rhs[k]; }
  hipLaunchKernelGGL(k_dense_gibbs_truncated_diag, dim3((unsigned)ctx->n_chains), dim3(64), (size_t)p * sizeof(double),
                     ctx->stream, ctx->n_chains, ctx->chain_offset, p, (int)terms->n_terms, m[0], m[1], m[2], m[3], s[0], s[1],
                     s[2], s[3], r[0], r[1], r[2], r[3], terms->diag_chain, rhs_chain, ld_rhs, lower, upper, u_inject, ld_u,
                     omc_make_key(ctx->seed, draw_index, OMC_RNG_UNIFORM), x, ld_x, ctx->d_bad_chain);
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}

extern "C" {


omc_status omc_small_gibbs_truncated(omc_ctx* ctx, int64_t kmax, const double* gram, const double* gram_rhs,
                                     const double* lik_scale, const double* prior_prec, const double* prior_mean,
                                     const double* count, double lower, double upper, const double* u_inject,
                                     uint64_t draw_index, double* x) {
  if (!ctx || kmax < 1 || kmax > 64 || !gram || !gram_rhs || !prior_prec || !x || !(lower < upper)) return OMC_INVALID_ARG;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  const size_t lds = (size_t)kmax * kmax * sizeof(double);
  hipLaunchKernelGGL(k_small_gibbs_truncated, dim3((unsigned)ctx->n_chains), dim3(64), lds, ctx->stream, ctx->n_chains,
                     ctx->chain_offset, (int)kmax, gram, gram_rhs, lik_scale, prior_prec, prior_mean, count, lower, upper,
                     u_inject, omc_make_key(ctx->seed, draw_index, OMC_RNG_UNIFORM), x, ctx->d_bad_chain);
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}

omc_status omc_diag_gauss_logpdf_limits(omc_ctx* ctx, int64_t kmax, const double* x, const double* mean, const double* prec,
                                        const double* count, double lower, double upper, double* out, int32_t accumulate) {
  if (!ctx || kmax < 1 || !x || !prec || !out) return OMC_INVALID_ARG;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_diag_gauss_logpdf_limits, dim3(grid1(ctx->n_chains, 4)), dim3(256), 0, ctx->stream, ctx->n_chains, kmax,
                     x, mean, prec, count, lower, upper, out, (int)accumulate);
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}

}  // extern "C"
