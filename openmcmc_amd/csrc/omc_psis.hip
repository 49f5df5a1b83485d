// Pareto-smoothed importance sampling leave-one-out of the device store (Vehtari, Simpson, Gelman, Yao, Gabry 2024; the
// generalised-Pareto fit of Zhang and Stephens 2009): per observation the PSIS-LOO expected log predictive density and the Pareto
// k of its importance ratios, without moving the store off the GPU.  The contract is in include/omcmc_hip.h (omc_store_psis).
//
// What it replaces: az.loo over a pointwise log-likelihood gathered from the loop over MCMC.store[...] that calls
// Normal.log_p(..., by_observation=True) of the reference per stored draw (distribution/location_scale.py:145-166).
//
// A chunk of Kc selected columns at a time:
//   k_psis_gather  the gather tile of omc_rank_sort.h: the S draws of a column as order-preserving keys of v = -ll, the log
//                  importance ratio up to a constant; ll is the entry as it lies, or omc_normal_ll (omc_loglik.h) of a mean entry
//                  computed on the way -- the same inline function as omc_store_loglik, so the two routes give the same bits.  It
//                  notes per column whether a NaN or an infinity was seen.
//   rank_sort      the key-only bitonic sort of every column (omc_store_shared.hip).
//   k_psis_fit     one workgroup of 512 per column, everything read from the sorted keys in the workspace (a tail may be S / 5
//                  long: nothing assumes that it fits LDS).  x_(i) = v_(i) - v_(S-1).  The cut and the tail length T by a bisection
//                  with the tail's own predicate x > xc, so T is exact.  The m candidate slopes of the fit go round the eight
//                  waves: a wave sums log1p(-b_i a_j) over the tail, lane l taking j = l, l + 64, .. in ascending order, the 64
//                  lanes combined by the butterfly 32 .. 1 (a + b == b + a: every lane ends with the same bits); a_j =
//                  exp(x_j) - exp(xc) is made again from the key each time rather than kept.  The weights, one thread per
//                  candidate, each a serial sum in ascending j; their normalisation and b serially in thread 0.  The sum for k' and
//                  the two log-sum-exp over the smoothed column (its normaliser, and the weighted likelihood): thread t takes
//                  positions t, t + 512, .. in ascending order, and thread 0 joins the 512 partial results in thread order.
//                  Every order is a function of (S, T) alone: repeated calls, and any "rank_tile" / "rank_chunk", give the same bits.
// No scratch.  The only atomics are the gather tile's flag words (an OR: independent of the order).
#include <math.h>

#include "omc_common.h"
#include "omc_loglik.h"
#include "omc_rank_sort.h"
#include "omc_store_view.h"

namespace {

constexpr int PSIS_THREADS = 512;
constexpr int PSIS_M_MAX = 4 * PSIS_THREADS;            // candidate slopes of the fit at most: 30 + floor(sqrt(T))
constexpr double PSIS_LOG_MIN = -708.3964185322641;    // log(DBL_MIN)
constexpr double PSIS_EPS = 2.220446049250313e-16;     // 2^-52

__global__ void __launch_bounds__(256) k_psis_check_tail(const int64_t* __restrict__ tail_max, int64_t n, int64_t S, int32_t* __restrict__ word) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < n && (tail_max[k] < 1 || tail_max[k] > S - 1)) *word = 1;
}

// y == NULL: the entry holds ll; else it holds the mean and ll is computed from y, prec [S][prec_size]
__global__ void __launch_bounds__(256) k_psis_gather(const double* __restrict__ store, const int64_t* __restrict__ idx, int64_t k0, int64_t Kc,
                                                     int64_t size, int64_t S, int64_t P, const double* __restrict__ y,
                                                     const double* __restrict__ prec, int64_t prec_size, int64_t n_idx,
                                                     uint64_t* __restrict__ keys, int32_t* __restrict__ flags) {
  const int64_t e0 = (int64_t)blockIdx.y * RANK_G_TE;
  rank_gather_tile(store, idx, k0, Kc, size, S, P, e0, (int64_t)blockIdx.x * RANK_G_TS, 0,
                   [](int64_t s) { return s; },
                   [=](double x, int64_t s, int64_t e_l) {  // draw s of selection position k0 + e0 + e_l (live: below n_idx)
                     if (!y) return -x;
                     const int64_t k = k0 + e0 + e_l;
                     const double tau = prec[prec_size == 1 ? s : s * n_idx + k];
                     return -omc_normal_ll(omc_normal_ll_head(tau), tau, y[k], x);
                   },
                   0, keys, flags);
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

__global__ void __launch_bounds__(PSIS_THREADS) k_psis_fit(int64_t k0, int64_t S, int64_t P, const uint64_t* __restrict__ keys,
                                                            const int32_t* __restrict__ flags, const int64_t* __restrict__ tail_max,
                                                            double* __restrict__ elpd_out, double* __restrict__ k_out,
                                                            int64_t* __restrict__ tail_out) {
  __shared__ double cand_b[PSIS_M_MAX], cand_l[PSIS_M_MAX];
  __shared__ double red[4][PSIS_THREADS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t e = blockIdx.x;
  const double nan = __longlong_as_double(0x7ff8000000000000LL), inf = __longlong_as_double(0x7ff0000000000000LL);
  if (flags[e] != 0) {  // a draw whose log-likelihood is not finite
    if (tid == 0) {
      elpd_out[k0 + e] = nan; k_out[k0 + e] = nan;
      if (tail_out) tail_out[k0 + e] = -1;
    }
    return;
  }
  const uint64_t* __restrict__ col = keys + e * P;
  const double vmax = q_val(col[S - 1]);
  const int64_t Mt = tail_max[k0 + e];  // 1 .. S - 1: checked before the launch
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
      if (smooth) {
        const double p = ((double)(s - t0) + 0.5) / (double)T, lp = log1p(-p);
        const double g = fabs(khat) < PSIS_EPS ? -sigma * lp : sigma * expm1(-khat * lp) / khat;
        x = sigma > 0.0 ? log(g + exc) : nan;
        x = x > 0.0 ? 0.0 : x;  // min(x, 0); a NaN stays
      }
      omc_lse_add(ML, sL, x, 1.0);
      omc_lse_add(MG, sG, x - v, 1.0);
    }
  }
  __syncthreads();
  red[0][tid] = ML; red[1][tid] = sL; red[2][tid] = MG; red[3][tid] = sG;
  __syncthreads();
  if (tid == 0) {
    for (int q = 1; q < PSIS_THREADS; ++q) {
      omc_lse_join(ML, sL, red[0][q], red[1][q]);
      omc_lse_join(MG, sG, red[2][q], red[3][q]);
    }
    // a draw outside the tail has x' + ll = -max(-ll): t0 >= 1 of them
    omc_lse_join(MG, sG, -vmax, (double)t0);
    elpd_out[k0 + e] = (MG + log(sG)) - (ML + log(sL));
    k_out[k0 + e] = khat;
    if (tail_out) tail_out[k0 + e] = T;
  }
}

omc_status psis_invalid(const char* text) {
  omc_set_error_text(text);
  return OMC_INVALID_ARG;
}

}  // namespace

extern "C" omc_status omc_store_psis(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx, int64_t n_idx,
                                     const double* y, const double* prec, int64_t prec_size, const int64_t* tail_max, double* elpd_out,
                                     double* k_out, int64_t* tail_out) {
  if (!ctx) return psis_invalid("omc_store_psis: no context");
  if (n_iter < 1 || n_iter * ctx->n_chains < 2) return psis_invalid("omc_store_psis: fewer than 2 stored draws (n_iter * C < 2)");
  if (size < 1) return psis_invalid("omc_store_psis: size < 1");
  if (!store || !tail_max || !elpd_out || !k_out) return psis_invalid("omc_store_psis: store, tail_max, elpd_out and k_out must not be NULL");
  if (n_idx < 1 || (!idx && n_idx != size)) return psis_invalid("omc_store_psis: n_idx < 1, or no index and n_idx != size");
  if ((y != nullptr) != (prec != nullptr)) return psis_invalid("omc_store_psis: y and prec must be given together");
  if (y && prec_size != 1 && prec_size != n_idx) return psis_invalid("omc_store_psis: prec_size must be 1 or n_idx");
  const int64_t S = n_iter * ctx->n_chains, P = rank_pow2(S);
  if (30 + (int64_t)floor(sqrt((double)(S - 1))) > PSIS_M_MAX) return psis_invalid("omc_store_psis: more stored draws than the fit takes (about 4 million)");
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  const size_t per_elem = (size_t)P * sizeof(uint64_t) + sizeof(int32_t);
  const int64_t Kc = rank_chunk(ctx, per_elem, n_idx);
  omc_status st = omc_ensure(ctx, ctx->rank_ws, RANK_HEAD + (size_t)Kc * per_elem + 64);
  if (st != OMC_OK) return st;
  char* ws = (char*)ctx->rank_ws.p;
  uint64_t* keys = (uint64_t*)(ws + RANK_HEAD);
  int32_t* flags = (int32_t*)(ws + RANK_HEAD + (size_t)Kc * P * sizeof(uint64_t));
  // one read-back for the index and the tail lengths, before anything is written: words 0 and 1 of the head
  int32_t* words = (int32_t*)ws;
  OMC_HIP_CHECK(hipMemsetAsync(words, 0, 2 * sizeof(int32_t), ctx->stream));
  omc_store_check_index_launch(ctx, idx, n_idx, size, nullptr, 0, 0, words);
  hipLaunchKernelGGL(k_psis_check_tail, dim3((unsigned)((n_idx + 255) / 256)), dim3(256), 0, ctx->stream, tail_max, n_idx, S, words + 1);
  OMC_HIP_CHECK(hipGetLastError());
  int32_t got[2] = {0, 0};
  OMC_HIP_CHECK(hipMemcpyAsync(got, words, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  OMC_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (got[0]) return psis_invalid("omc_store_psis: an index outside [0, size)");
  if (got[1]) return psis_invalid("omc_store_psis: a tail_max outside [1, n_iter * C - 1]");
  for (int64_t k0 = 0; k0 < n_idx; k0 += Kc) {
    const int64_t kc = n_idx - k0 < Kc ? n_idx - k0 : Kc;
    OMC_HIP_CHECK(hipMemsetAsync(flags, 0, (size_t)kc * sizeof(int32_t), ctx->stream));
    const dim3 grid((unsigned)((P + RANK_G_TS - 1) / RANK_G_TS), (unsigned)((kc + RANK_G_TE - 1) / RANK_G_TE));
    hipLaunchKernelGGL(k_psis_gather, grid, dim3(256), 0, ctx->stream, store, idx, k0, kc, size, S, P, y, prec, prec_size, n_idx, keys, flags);
    OMC_HIP_CHECK(hipGetLastError());
    st = rank_sort(ctx, keys, kc, P);
    if (st != OMC_OK) return st;
    hipLaunchKernelGGL(k_psis_fit, dim3((unsigned)kc), dim3(PSIS_THREADS), 0, ctx->stream, k0, S, P, keys, flags, tail_max, elpd_out, k_out,
                       tail_out);
    OMC_HIP_CHECK(hipGetLastError());
  }
  return OMC_OK;
}
