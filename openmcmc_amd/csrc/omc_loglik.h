// The pointwise Normal log-density of a stored draw and the running log-sum-exp pair, inline on the device: shared by
// omc_loglik.hip (column summaries) and omc_psis.hip (importance ratios computed while the mean entry is read), so that the two
// give the same bits.  Every product is rounded or fused explicitly: nothing is left to the compiler's contraction.
#pragma once
#include <math.h>

#include <hip/hip_runtime.h>

constexpr double OMC_HALF_LOG_2PI = 0.91893853320467274178;  // 0.5 log(2 pi), rounded to fp64

// h = 0.5 log(tau) - c: the part of the log-density that belongs to the precision alone (NaN for tau < 0, -inf for tau == 0)
__device__ __forceinline__ double omc_normal_ll_head(double tau) { return fma(0.5, log(tau), -OMC_HALF_LOG_2PI); }

// ll = h - 0.5 tau r r with r = y - x: one IEEE subtraction, 0.5 tau exact, one rounded product, one fused multiply-add
__device__ __forceinline__ double omc_normal_ll(double h, double tau, double y, double x) {
  const double r = __dsub_rn(y, x);
  const double q = __dmul_rn(0.5 * tau, r);
  return fma(-q, r, h);
}

// is ll a number a column's summaries can hold?  (a NaN or infinite element, a precision that is not positive and finite: no)
__device__ __forceinline__ bool omc_ll_finite(double ll) { return fabs(ll) < __longlong_as_double(0x7ff0000000000000LL); }

// (M, s): log sum = M + log(s) with M the largest term so far and s >= 1 the sum of exp(term - M); nothing yet: (-inf, 0).
// Adds the pair (Mb, sb), Mb finite and sb > 0 -- a single term is (v, 1) --: ONE exp, the rescaling of the side with the smaller
// maximum, and one fused multiply-add; the other side's factor is exp(0) = 1 exactly.  Symmetric in its two sides.
__device__ __forceinline__ void omc_lse_add(double& M, double& s, double Mb, double sb) {
  const double e = exp(-fabs(Mb - M));
  const bool up = Mb > M;
  s = up ? fma(s, e, sb) : fma(sb, e, s);
  M = up ? Mb : M;
}
// the same for a side that may be empty
__device__ __forceinline__ void omc_lse_join(double& M, double& s, double Mb, double sb) {
  if (sb == 0.0) return;
  omc_lse_add(M, s, Mb, sb);
}
