// Pareto-smoothed importance sampling leave-one-out of the device store (Vehtari, Simpson, Gelman, Yao, Gabry 2024; the
// generalised-Pareto fit of Zhang and Stephens 2009): per observation the PSIS-LOO expected log predictive density and the Pareto
// k of its importance ratios, without moving the store off the GPU.  The contract is in include/omcmc_hip.h (omc_store_psis).
//
// What it replaces: az.loo over a pointwise log-likelihood gathered from the loop over MCMC.store[...] that calls
// Normal.log_p(..., by_observation=True) of the reference per stored draw (distribution/location_scale.py:145-166).
//
// A chunk of Kc selected columns at a time:
//   k_psis_gather  (shared with omc_loo_expect.hip through psis_gather_sort) the gather tile of omc_rank_sort.h: the S draws of
//                  a column as order-preserving keys of v = -ll, the log importance ratio up to a constant; ll is the entry as it lies, or omc_normal_ll (omc_loglik.h) of a mean entry
//                  computed on the way -- the same inline function as omc_store_loglik, so the two routes give the same bits.  It
//                  notes per column whether a NaN or an infinity was seen.
//   rank_sort      the key-only bitonic sort of every column (omc_store_shared.hip).
//   k_psis_fit     one workgroup of 512 per column: psis_fit_column of omc_psis_fit.h (described there; shared with
//                  omc_loo_expect.hip, which keeps the fit instead of folding it) and the three stores.  Every order of additions is
//                  a function of (S, T) alone: repeated calls, and any "rank_tile" / "rank_chunk", give the same bits.
// No scratch.  The only atomics are the gather tile's flag words (an OR: independent of the order).
#include <math.h>

#include <string>

#include "omc_common.h"
#include "omc_loglik.h"
#include "omc_psis_fit.h"
#include "omc_rank_sort.h"
#include "omc_store_view.h"

namespace {

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
                     return psis_neg_ll(x, s, k0 + e0 + e_l, y, prec, prec_size, n_idx);
                   },
                   0, keys, flags);
}

__global__ void __launch_bounds__(PSIS_THREADS) k_psis_fit(int64_t k0, int64_t S, int64_t P, const uint64_t* __restrict__ keys,
                                                            const int32_t* __restrict__ flags, const int64_t* __restrict__ tail_max,
                                                            double* __restrict__ elpd_out, double* __restrict__ k_out,
                                                            int64_t* __restrict__ tail_out) {
  const int64_t e = blockIdx.x;
  if (flags[e] != 0) {  // a draw whose log-likelihood is not finite
    if (threadIdx.x == 0) {
      const double nan = __longlong_as_double(0x7ff8000000000000LL);
      elpd_out[k0 + e] = nan; k_out[k0 + e] = nan;
      if (tail_out) tail_out[k0 + e] = -1;
    }
    return;
  }
  const PsisFit f = psis_fit_column(keys + e * P, S, tail_max[k0 + e]);  // tail_max 1 .. S - 1: checked before the launch
  if (threadIdx.x == 0) {
    elpd_out[k0 + e] = f.elpd;
    k_out[k0 + e] = f.khat;
    if (tail_out) tail_out[k0 + e] = f.T;
  }
}

}  // namespace

omc_status psis_prelude(omc_ctx* ctx, const char* who, const PsisCall& c, const char* null_text, const char* own_text, const int64_t* vidx,
                        int64_t vsize) {
  const auto no = [who](const char* text) { return omc_invalid((std::string(who) + ": " + text).c_str()); };
  if (!ctx) return no("no context");
  if (c.n_iter < 1 || c.n_iter * ctx->n_chains < 2) return no("fewer than 2 stored draws (n_iter * C < 2)");
  if (c.size < 1) return no("size < 1");
  if (null_text) return no(null_text);
  if (c.n_idx < 1 || (!c.idx && c.n_idx != c.size)) return no("n_idx < 1, or no index and n_idx != size");
  if ((c.y != nullptr) != (c.prec != nullptr)) return no("y and prec must be given together");
  if (c.y && c.prec_size != 1 && c.prec_size != c.n_idx) return no("prec_size must be 1 or n_idx");
  if (own_text) return no(own_text);
  const int64_t S = c.n_iter * ctx->n_chains;
  if (30 + (int64_t)floor(sqrt((double)(S - 1))) > PSIS_M_MAX) return no("more stored draws than the fit takes (about 4 million)");
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  omc_status st = omc_ensure(ctx, ctx->store_ws, 64);
  if (st != OMC_OK) return st;
  int32_t* words = (int32_t*)ctx->store_ws.p;
  st = omc_words_zero(ctx, words, 3);
  if (st != OMC_OK) return st;
  omc_store_check_index_launch(ctx, c.idx, c.n_idx, c.size, nullptr, 0, 0, words);
  hipLaunchKernelGGL(k_psis_check_tail, dim3((unsigned)((c.n_idx + 255) / 256)), dim3(256), 0, ctx->stream, c.tail_max, c.n_idx, S, words + 1);
  omc_store_check_index_launch(ctx, vidx, c.n_idx, vsize, nullptr, 0, 0, words + 2);
  int32_t got[3] = {0, 0, 0};
  st = omc_words_read(ctx, words, 3, got);
  if (st != OMC_OK) return st;
  if (got[0]) return no("an index outside [0, size)");
  if (got[1]) return no("a tail_max outside [1, n_iter * C - 1]");
  if (got[2]) return no("a vidx outside [0, vsize)");
  return OMC_OK;
}

omc_status psis_gather_sort(omc_ctx* ctx, const PsisCall& c, int64_t k0, int64_t kc, int64_t S, int64_t P, uint64_t* keys, int32_t* flags) {
  OMC_HIP_CHECK(hipMemsetAsync(flags, 0, (size_t)kc * sizeof(int32_t), ctx->stream));
  const dim3 grid((unsigned)((P + RANK_G_TS - 1) / RANK_G_TS), (unsigned)((kc + RANK_G_TE - 1) / RANK_G_TE));
  hipLaunchKernelGGL(k_psis_gather, grid, dim3(256), 0, ctx->stream, c.store, c.idx, k0, kc, c.size, S, P, c.y, c.prec, c.prec_size, c.n_idx, keys,
                     flags);
  OMC_HIP_CHECK(hipGetLastError());
  return rank_sort(ctx, keys, kc, P);
}

extern "C" omc_status omc_store_psis(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx, int64_t n_idx,
                                     const double* y, const double* prec, int64_t prec_size, const int64_t* tail_max, double* elpd_out,
                                     double* k_out, int64_t* tail_out) {
  const PsisCall c = {n_iter, size, store, idx, n_idx, y, prec, prec_size, tail_max};
  const char* null_text = store && tail_max && elpd_out && k_out ? nullptr : "store, tail_max, elpd_out and k_out must not be NULL";
  omc_status st = psis_prelude(ctx, "omc_store_psis", c, null_text, nullptr, nullptr, 0);
  if (st != OMC_OK) return st;
  const int64_t S = n_iter * ctx->n_chains, P = rank_pow2(S);
  RankCarve ws(ctx, (size_t)P * sizeof(uint64_t) + sizeof(int32_t), n_idx);
  const int64_t Kc = ws.Kc;
  uint64_t* keys = ws.take<uint64_t>((size_t)Kc * P);
  int32_t* flags = ws.take<int32_t>(Kc);
  st = ws.done();
  if (st != OMC_OK) return st;
  for (int64_t k0 = 0; k0 < n_idx; k0 += Kc) {
    const int64_t kc = n_idx - k0 < Kc ? n_idx - k0 : Kc;
    st = psis_gather_sort(ctx, c, k0, kc, S, P, keys, flags);
    if (st != OMC_OK) return st;
    hipLaunchKernelGGL(k_psis_fit, dim3((unsigned)kc), dim3(PSIS_THREADS), 0, ctx->stream, k0, S, P, keys, flags, tail_max, elpd_out, k_out,
                       tail_out);
    OMC_HIP_CHECK(hipGetLastError());
  }
  return OMC_OK;
}
