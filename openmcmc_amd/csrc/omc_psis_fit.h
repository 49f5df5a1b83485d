// The generalised-Pareto fit of a sorted column of importance ratios, inline on the device: steps 1 - 6 of the omc_store_psis
// contract (include/omcmc_hip.h), shared by omc_psis.hip (k_psis_fit: elpd, k, T) and omc_loo_expect.hip (k_loo_fit: the fit record
// every draw's weight is made from), so that the two give the same bits.  Also the value a draw enters the sort with and the
// smoothed value of a tail position, which the expectation pass makes again per draw.
//
//   psis_fit_column  one workgroup of PSIS_THREADS = 512 per column, everything read from the sorted keys in the workspace (a tail
//                  may be S / 5 long: nothing assumes that it fits LDS).  x_(i) = v_(i) - v_(S-1).  The cut and the tail length T by
//                  a bisection with the tail's own predicate x > xc, so T is exact.  The m candidate slopes of the fit go round the
//                  eight waves: a wave sums log1p(-b_i a_j) over the tail, lane l taking j = l, l + 64, .. in ascending order, the
//                  64 lanes combined by the butterfly 32 .. 1 (a + b == b + a: every lane ends with the same bits); a_j =
//                  exp(x_j) - exp(xc) is made again from the key each time rather than kept.  The weights, one thread per
//                  candidate, each a serial sum in ascending j; their normalisation and b serially in thread 0.  The sum for k' and
//                  the two log-sum-exp over the smoothed column (its normaliser, and the weighted likelihood): thread t takes
//                  positions t, t + 512, .. in ascending order, and thread 0 joins the 512 partial results in thread order.
//                  Every order is a function of (S, T) alone.
#pragma once
#include <math.h>

#include "omc_common.h"
#include "omc_loglik.h"
#include "omc_quantile.h"

constexpr int PSIS_THREADS = 512;
constexpr int PSIS_M_MAX = 4 * PSIS_THREADS;            // candidate slopes of the fit at most: 30 + floor(sqrt(T))
constexpr double PSIS_LOG_MIN = -708.3964185322641;    // log(DBL_MIN)
constexpr double PSIS_EPS = 2.220446049250313e-16;     // 2^-52

// what the fit of a column leaves: every field in every thread, but L and elpd, which thread 0 alone holds
struct PsisFit {
  double vmax, xc, exc;  // max_s(-ll_s); the cut; exp(xc)
  double khat, sigma;    // +inf and 0 where nothing was fitted (T <= 4)
  double L, elpd;        // logsumexp of the smoothed column; the PSIS-LOO elpd
  int64_t t0, T;         // first tail position of the sorted column; T = S - t0
  bool smooth;           // khat is finite: the tail positions hold the fit's expected order statistics
};

// omc_psis.hip: what omc_store_psis and omc_store_loo_expect do alike on the host, on the arguments they have in common
struct PsisCall {
  int64_t n_iter, size;
  const double* store; const int64_t* idx; int64_t n_idx;
  const double *y, *prec; int64_t prec_size;
  const int64_t* tail_max;
};
// Everything that can refuse the call, in one place and before anything is written: the argument checks, with the caller's two
// complaints of its own (or NULL) -- null_text where the check of the pointers stands, own_text behind the shared checks --, the bound
// on the draws, and ONE read-back of the check words (head of ctx->store_ws): idx against [0, size), tail_max against [1, S - 1],
// vidx (or NULL) against [0, vsize).  Every text is "<who>: ..." through omc_invalid.
omc_status psis_prelude(omc_ctx* ctx, const char* who, const PsisCall& c, const char* null_text, const char* own_text, const int64_t* vidx,
                        int64_t vsize);
// flags zeroed, the draws of selection positions [k0, k0 + kc) as keys of psis_neg_ll (k_psis_gather), rank_sort
omc_status psis_gather_sort(omc_ctx* ctx, const PsisCall& c, int64_t k0, int64_t kc, int64_t S, int64_t P, uint64_t* keys, int32_t* flags);

// v = -ll of draw s at selection position k: the entry as it lies (y == NULL), or omc_normal_ll of a mean entry
__device__ __forceinline__ double psis_neg_ll(double x, int64_t s, int64_t k, const double* __restrict__ y, const double* __restrict__ prec,
                                              int64_t prec_size, int64_t n_idx) {
  if (!y) return -x;
  const double tau = prec[prec_size == 1 ? s : s * n_idx + k];
  return -omc_normal_ll(omc_normal_ll_head(tau), tau, y[k], x);
}

// the smoothed x' of tail position i = 0 .. T - 1 (step 5): min(log(sigma expm1(-k log1p(-p)) / k + exp(xc)), 0), p = (i + 0.5) / T
__device__ __forceinline__ double psis_smoothed_x(int64_t i, int64_t T, double khat, double sigma, double exc) {
  const double p = ((double)i + 0.5) / (double)T, lp = log1p(-p);
  const double g = fabs(khat) < PSIS_EPS ? -sigma * lp : sigma * expm1(-khat * lp) / khat;
  double x = sigma > 0.0 ? log(g + exc) : __longlong_as_double(0x7ff8000000000000LL);
  x = x > 0.0 ? 0.0 : x;  // min(x, 0); a NaN stays
  return x;
}

// the sum of the workgroup's 512 values in thread order, in every thread (red: 512 doubles of LDS)
__device__ __forceinline__ double psis_block_sum(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = red[0];
    for (int q = 1; q < PSIS_THREADS; ++q) t += red[q];
    red[0] = t;
  }
  __syncthreads();
  return red[0];
}

// col: the S sorted keys of a column whose values are all finite; Mt = tail_max of the column, 1 .. S - 1.  Called by all 512
// threads of the workgroup (48 KiB of LDS).
__device__ __forceinline__ PsisFit psis_fit_column(const uint64_t* __restrict__ col, int64_t S, int64_t Mt) {
  __shared__ double cand_b[PSIS_M_MAX], cand_l[PSIS_M_MAX];
  __shared__ double red[4][PSIS_THREADS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  PsisFit f;
  const double vmax = q_val(col[S - 1]);
  const double xcut = q_val(col[S - Mt - 1]) - vmax;
  const double xc = xcut > PSIS_LOG_MIN ? xcut : PSIS_LOG_MIN;
  // first position with x > xc: x is non-decreasing along the sorted column (every thread walks the same bisection)
  int64_t lo = 0, hi = S;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (q_val(col[mid]) - vmax > xc) hi = mid; else lo = mid + 1;
  }
  const int64_t t0 = lo, T = S - t0;
  const double exc = exp(xc);
  double khat = inf, sigma = 0.0;
  if (T > 4) {
    const int64_t n = T;
    const double dn = (double)n;
    const int m = 30 + (int)floor(sqrt(dn));  // <= PSIS_M_MAX: checked on the host from S
    const int64_t q = (int64_t)floor(dn / 4.0 + 0.5) - 1;
    const double a_last = exp(q_val(col[S - 1]) - vmax) - exc, a_q = exp(q_val(col[t0 + q]) - vmax) - exc;
    for (int i = wave; i < m; i += PSIS_THREADS / 64) {
      const double b = 1.0 / a_last + (1.0 - sqrt((double)m / ((double)(i + 1) - 0.5))) / (3.0 * a_q);
      double sum = 0.0;
      for (int64_t j = lane; j < n; j += 64) sum += log1p(-b * (exp(q_val(col[t0 + j]) - vmax) - exc));
      for (int w = 32; w >= 1; w >>= 1) sum += __shfl_xor(sum, w, 64);
      if (lane == 0) {
        const double ki = sum / dn;
        cand_b[i] = b;
        cand_l[i] = dn * (log(-b / ki) - ki - 1.0);
      }
    }
    __syncthreads();
    // w_i = 1 / sum_j exp(L_j - L_i): an overflowing exp is +inf and the weight 0
    double* cand_w = &red[0][0];  // 4 * PSIS_THREADS == PSIS_M_MAX doubles
    for (int i = tid; i < m; i += PSIS_THREADS) {
      const double li = cand_l[i];
      double sum = 0.0;
      for (int j = 0; j < m; ++j) sum += exp(cand_l[j] - li);
      cand_w[i] = 1.0 / sum;
    }
    __syncthreads();
    if (tid == 0) {  // the candidates below the cut are dropped, the rest divided by their sum
      double tot = 0.0;
      for (int i = 0; i < m; ++i) tot += cand_w[i] >= 10.0 * PSIS_EPS ? cand_w[i] : 0.0;
      double b = 0.0;
      for (int i = 0; i < m; ++i)
        if (cand_w[i] >= 10.0 * PSIS_EPS) b += cand_b[i] * (cand_w[i] / tot);
      cand_b[0] = b;
    }
    __syncthreads();
    const double b = cand_b[0];
    double part = 0.0;
    for (int64_t j = tid; j < n; j += PSIS_THREADS) part += log1p(-b * (exp(q_val(col[t0 + j]) - vmax) - exc));
    const double kp = psis_block_sum(part, red[0]) / dn;
    sigma = -kp / b;
    khat = (dn * kp + 5.0) / (dn + 10.0);
  }
  // the smoothed column: its normaliser L = logsumexp(x') and G = logsumexp(x' + ll), ll = -v; elpd = G - L
  const bool smooth = khat == khat && fabs(khat) < inf;
  double ML = -inf, sL = 0.0, MG = -inf, sG = 0.0;
  for (int64_t s = tid; s < S; s += PSIS_THREADS) {
    const double v = q_val(col[s]);
    double x = v - vmax;
    if (s < t0) {
      omc_lse_add(ML, sL, x, 1.0);
    } else {
      if (smooth) x = psis_smoothed_x(s - t0, T, khat, sigma, exc);
      omc_lse_add(ML, sL, x, 1.0);
      omc_lse_add(MG, sG, x - v, 1.0);
    }
  }
  __syncthreads();
  red[0][tid] = ML; red[1][tid] = sL; red[2][tid] = MG; red[3][tid] = sG;
  __syncthreads();
  f.L = f.elpd = 0.0;
  if (tid == 0) {
    for (int q = 1; q < PSIS_THREADS; ++q) {
      omc_lse_join(ML, sL, red[0][q], red[1][q]);
      omc_lse_join(MG, sG, red[2][q], red[3][q]);
    }
    // a draw outside the tail has x' + ll = -max(-ll): t0 >= 1 of them
    omc_lse_join(MG, sG, -vmax, (double)t0);
    f.L = ML + log(sL);
    f.elpd = (MG + log(sG)) - f.L;
  }
  f.vmax = vmax; f.xc = xc; f.exc = exc; f.khat = khat; f.sigma = sigma; f.t0 = t0; f.T = T; f.smooth = smooth;
  return f;
}
