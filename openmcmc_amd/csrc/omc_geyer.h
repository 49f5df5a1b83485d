// Geyer's initial monotone sequence on the lag sums S(t) of the J split series of an element, as omc_store_rhat_ess defines it
// (include/omcmc_hip.h): the one copy of the rule.  Shared by omc_diag.hip (k_diag_step: fp64 lag sums of the draws, a block of
// lags per launch) and omc_essq.hip (k_essq_lags: exact integer lag sums of an indicator series, every block inside one launch).
// The state is advanced over the lags that are at hand and picked up again where it stopped; the arithmetic does not depend on
// how the lags are cut into blocks.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

// W, var_plus; even, odd: rho of the last evaluated pair; acc: sum of the monotone pair sums so far; minq: their running minimum;
// pp: index of the last evaluated pair
struct GeyerState { double W, vp, even, odd, acc, minq, pp; };

enum { GEYER_NAN = 0, GEYER_CONSTANT = 1, GEYER_GO = 2 };

// W and var_plus from S(0) = S0 and the variance of the series means BM; S(t) is asked for lag 1 only, and only when the
// sequence starts.  GEYER_NAN: a NaN draw somewhere in the element; GEYER_CONSTANT: every draw equal (ess = J M, rhat NaN);
// GEYER_GO: rhat = sqrt(vp / W) (+inf when W == 0 < B_M) and the first pair is set up.
template <typename F>
__device__ __forceinline__ int geyer_start(GeyerState& g, double S0, double BM, int64_t J, int64_t M, F S) {
  const double JM = (double)J * (double)M;
  g.W = S0 / ((double)J * (double)(M - 1));
  g.vp = g.W * (double)(M - 1) / (double)M + BM;
  if (S0 != S0 || BM != BM) return GEYER_NAN;
  if (g.W == 0.0 && BM == 0.0) return GEYER_CONSTANT;
  g.even = 1.0;
  g.odd = 1.0 - (g.W - S(1) / JM) / g.vp;
  return GEYER_GO;
}

// The pairs whose lags lie below t_end, S(t) their lag sums: true once the sequence has ended, false when the next pair's lags
// belong to a later block.
template <typename F>
__device__ __forceinline__ bool geyer_advance(GeyerState& g, int64_t M, double JM, int64_t t_end, F S) {
  for (;;) {
    const int64_t p = (int64_t)g.pp + 1;  // next pair: rho(2p), rho(2p + 1), evaluated while t = 2p - 1 < M - 3 and the last sum > 0
    if (!(2 * p - 1 < M - 3 && g.even + g.odd > 0.0)) return true;
    if (2 * p + 1 >= t_end) return false;  // its lags belong to the next block
    const double q = g.pp == 0.0 ? g.even + g.odd : fmin(g.even + g.odd, g.minq);  // the monotone step: running minimum of the pair sums
    g.acc += q;
    g.minq = q;
    g.even = 1.0 - (g.W - S(2 * p) / JM) / g.vp;
    g.odd = 1.0 - (g.W - S(2 * p + 1) / JM) / g.vp;
    g.pp = (double)p;
  }
}

// ess and the lags used, of a sequence that has ended
__device__ __forceinline__ void geyer_finish(const GeyerState& g, double JM, double& ess, int32_t& lags) {
  // the last evaluated pair enters through r[max_t + 1] = r[2 pp] only: even if it was written (sum >= 0) or positive
  const double rlast = (g.even + g.odd >= 0.0 || g.even > 0.0) ? g.even : 0.0;
  double tau = -1.0 + 2.0 * g.acc + rlast;
  const double floor_tau = 1.0 / log10(JM);
  if (!(tau >= floor_tau)) tau = floor_tau;
  ess = JM / tau;
  lags = (int32_t)(2 * (int64_t)g.pp);
}
