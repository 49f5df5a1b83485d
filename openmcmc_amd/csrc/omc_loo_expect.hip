// PSIS-LOO expectations of the device store: per observation the leave-one-out mean, variance and distribution function of a
// per-draw quantity f under the Pareto-smoothed importance weights of omc_store_psis, the effective sample size of those weights,
// and the normalised log weights themselves -- az.loo_pit, az.psislw and the LOO predictive moments without moving the store off
// the GPU.  The contract is in include/omcmc_hip.h (omc_store_loo_expect).
//
// What it replaces: az.loo_pit / az.psislw over a pointwise log-likelihood gathered from the loop over MCMC.store[...] that calls
// Normal.log_p(..., by_observation=True) of the reference per stored draw (distribution/location_scale.py:145-166).
//
// The sort of omc_rank_sort.h is key-only: after it a smoothed weight belongs to a sorted position, not to a draw, and f still lies
// in the store in draw order.  A chunk of Kc selected columns at a time:
//   psis_gather_sort  omc_psis.hip's k_psis_gather and the key-only bitonic sort of every column (omc_store_shared.hip).
//   k_loo_fit      psis_fit_column of omc_psis_fit.h, one workgroup of 512 per column: the fit record (vmax, xc, exp(xc), k, sigma,
//                  L, t0, T; T = -1 for a column with an ll that is not finite) into the workspace.
//   k_loo_expect   laid out like k_loglik_part: a workgroup owns LE_COLS = 32 adjacent selection positions and a slice of the rows;
//                  thread (cl, rr), cl = 0 .. 15 along the row and rr = 0 .. 15 down it, carries TWO columns: 2 cl and 2 cl + 1 of the
//                  tile, read with one 16-byte load (VEC: no index, even sizes, 16-byte aligned entries, an even chunk), else cl and
//                  cl + 16, two 8-byte loads that each coalesce over the 16 lanes.  A column's rows go to row lane rr = row mod 16 of
//                  the slice in ascending order in both forms, so the two forms give the same bits.  v = -ll is made on load by the
//                  gather's own inline function, so a tail draw finds its key in the sorted column bit for bit: x = v - vmax <= xc
//                  (or nothing smoothed) is w = exp(min(x, 0)), one exp per element; a tail draw bisects the sorted column
//                  (rank_bound: lo keys below; hi, the keys not above, where the run of equal keys ends) and takes the mean of exp(x'_(p)), p in [lo, hi), ascending -- at
//                  most ceil(min(S / 5, 3 sqrt(S))) of the S draws of a column, a rare and divergent branch by design.  Per column a
//                  lane carries W = sum w, West's weighted (mean, m2) of f, sum w [f <= thr], sum w^2 and sum w / tau, each only
//                  where its output was asked for (a wave-uniform branch).  The 16 row lanes are joined 1 .. 15 in order through
//                  LDS -- the moments by Chan's update with weights for counts, the rest by addition -- into part [slices][6][Kc].
//                  lw_out is written on the way.  The sorted keys stay in rank_ws until the pass over the chunk has run.
//   k_loo_join     thread = column: the slices in slice order, the divisions by W, k and T from the fit record.
// Slices: omc_row_slices (omc_store_view.h) over the whole selection, a function of (S, n_idx) alone and not of the chunk.  No
// scratch.  The only atomics are the gather tile's flag words (an OR: independent of the order).
#include <math.h>

#include "omc_common.h"
#include "omc_loglik.h"
#include "omc_moments.h"
#include "omc_psis_fit.h"
#include "omc_rank_sort.h"
#include "omc_store_view.h"

namespace {

constexpr int LE_COLS = 32, LE_ROWS = 16;  // k_loo_expect: selection positions and row lanes of a workgroup
constexpr int LE_PART = 6;                 // partial results of a column and slice: W, mean, m2, below, sum w^2, sum w / tau
constexpr int32_t LE_MOM = 1, LE_BELOW = 2, LE_ESS = 4, LE_IP = 8;  // LooArgs.want
constexpr int F_ENTRY = 0, F_MEAN = 1, F_CDF = 2;

struct LooFit {  // 64 bytes per column of the chunk
  double vmax, xc, exc, khat, sigma, L;
  int64_t t0, T;
};

struct LooArgs {
  const double* store; const int64_t* idx; const double* y; const double* prec; const double* values; const int64_t* vidx;
  const double* thr; const uint64_t* keys; const LooFit* fit; double* part; double* lw_out;
  int64_t S, P, size, vsize, n_idx, prec_size, rows_per_block, k0, kc;
  int32_t want;
};

__global__ void __launch_bounds__(PSIS_THREADS) k_loo_fit(int64_t k0, int64_t S, int64_t P, const uint64_t* __restrict__ keys,
                                                           const int32_t* __restrict__ flags, const int64_t* __restrict__ tail_max,
                                                           LooFit* __restrict__ fit) {
  const int64_t e = blockIdx.x;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  if (flags[e] != 0) {  // a draw whose log-likelihood is not finite
    if (threadIdx.x == 0) fit[e] = LooFit{nan, nan, nan, nan, nan, nan, 0, -1};
    return;
  }
  const PsisFit f = psis_fit_column(keys + e * P, S, tail_max[k0 + e]);  // tail_max 1 .. S - 1: checked before the launch
  if (threadIdx.x == 0) fit[e] = LooFit{f.vmax, f.xc, f.exc, f.khat, f.sigma, f.L, f.t0, f.T};
}

// a column of a thread: its fit, what belongs to its selection position, and the running sums
struct LooCol {
  double vmax, xc, exc, khat, sigma, L;
  int64_t t0, T;
  const uint64_t* col;
  bool live, smooth;
  double y, thr;
  double W, mean, m2, below, w2, ip;

  __device__ __forceinline__ void init(const LooArgs& g, int64_t e, bool ok) {
    W = mean = m2 = below = w2 = ip = 0.0;
    y = thr = 0.0;
    live = false; smooth = false;
    vmax = xc = exc = khat = sigma = L = 0.0;
    t0 = 0; T = -1;
    col = g.keys;
    if (!ok) return;
    const LooFit f = g.fit[e];
    vmax = f.vmax; xc = f.xc; exc = f.exc; khat = f.khat; sigma = f.sigma; L = f.L; t0 = f.t0; T = f.T;
    live = T >= 0;
    smooth = live && khat == khat && fabs(khat) < __longlong_as_double(0x7ff0000000000000LL);
    col = g.keys + e * g.P;
    if (g.y) y = g.y[g.k0 + e];
    if (g.thr) thr = g.thr[g.k0 + e];
  }

  // the weight of the draw with v = -ll, and its log less the normaliser (the exponent itself where w is a single exponential)
  __device__ __forceinline__ double weight(double v, int64_t P, double& lw) const {
    const uint64_t key = rank_key(v);
    const double x = q_val(key) - vmax;
    if (!smooth || !(x > xc)) {
      const double xm = x > 0.0 ? 0.0 : x;
      lw = xm - L;
      return exp(xm);
    }
    // t0 <= lo < hi <= S: the key is in the column, so the keys <= key end where the run of equal keys from lo ends (what
    // rank_bound(.., true) gives, without a second bisection: ties are rare and short)
    const int64_t lo = rank_bound(col, P, key, false);
    int64_t hi = lo + 1;
    while (hi < P && col[hi] == key) ++hi;
    const double x0 = psis_smoothed_x(lo - t0, T, khat, sigma, exc);
    double w = exp(x0);
    if (hi - lo == 1) {
      lw = x0 - L;
      return w;
    }
    for (int64_t p = lo + 1; p < hi; ++p) w += exp(psis_smoothed_x(p - t0, T, khat, sigma, exc));
    w /= (double)(hi - lo);
    lw = log(w) - L;
    return w;
  }

  // West's weighted update and the plain sums; a draw of weight 0 adds nothing
  __device__ __forceinline__ void add(int32_t want, double w, double f, double rcp_tau) {
    if (w == 0.0) return;
    const double Wn = W + w;
    if (want & LE_MOM) {
      const double d = f - mean;
      mean = fma(d, w / Wn, mean);
      m2 = fma(__dmul_rn(w, d), f - mean, m2);
    }
    W = Wn;
    if (want & LE_BELOW) below += f <= thr ? w : 0.0;
    if (want & LE_ESS) w2 = fma(w, w, w2);
    if (want & LE_IP) ip = fma(w, rcp_tau, ip);
  }
};

template <bool VEC, int F>
__global__ void __launch_bounds__(256) k_loo_expect(LooArgs g) {
  __shared__ double sm[LE_PART][LE_ROWS][LE_COLS];
  const int tid = threadIdx.x, cl = tid & 15, rr = tid >> 4;
  const int c0 = VEC ? 2 * cl : cl, c1 = VEC ? 2 * cl + 1 : cl + 16;  // the thread's two columns of the tile
  const int64_t e0 = (int64_t)blockIdx.x * LE_COLS + c0, e1 = (int64_t)blockIdx.x * LE_COLS + c1;  // positions in the chunk
  const bool ok0 = e0 < g.kc, ok1 = e1 < g.kc;  // (VEC: kc is even, both or none)
  const int64_t k0 = g.k0 + e0, k1 = g.k0 + e1;  // selection positions
  // 0 <= idx[k] < size and 0 <= vidx[k] < vsize: checked before the launch
  const int64_t s0 = ok0 ? (g.idx ? g.idx[k0] : k0) : 0, s1 = ok1 ? (g.idx ? g.idx[k1] : k1) : 0;
  int64_t v0 = 0, v1 = 0;
  if (F == F_ENTRY) {
    v0 = ok0 ? (g.vidx ? g.vidx[k0] : k0) : 0;
    v1 = ok1 ? (g.vidx ? g.vidx[k1] : k1) : 0;
  }
  LooCol a0, a1;
  a0.init(g, e0, ok0);
  a1.init(g, e1, ok1);
  const bool need_tau = F == F_CDF || (g.want & LE_IP);
  const int64_t r_begin = (int64_t)blockIdx.y * g.rows_per_block;
  const int64_t r_end = r_begin + g.rows_per_block < g.S ? r_begin + g.rows_per_block : g.S;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  for (int64_t r = r_begin + rr; r < r_end; r += LE_ROWS) {
    double x0 = 0.0, x1 = 0.0, f0 = 0.0, f1 = 0.0, t0 = 1.0, t1 = 1.0;
    if (VEC) {
      if (ok0) {
        const double2 v = *(const double2*)(g.store + r * g.size + s0);
        x0 = v.x; x1 = v.y;
        if (F == F_ENTRY) {
          const double2 u = *(const double2*)(g.values + r * g.vsize + v0);
          f0 = u.x; f1 = u.y;
        }
      }
    } else {
      if (ok0) x0 = g.store[r * g.size + s0];
      if (ok1) x1 = g.store[r * g.size + s1];
      if (F == F_ENTRY) {
        if (ok0) f0 = g.values[r * g.vsize + v0];
        if (ok1) f1 = g.values[r * g.vsize + v1];
      }
    }
    if (need_tau) {
      if (g.prec_size == 1) {
        t0 = t1 = g.prec[r];
      } else {
        if (ok0) t0 = g.prec[r * g.n_idx + k0];
        if (ok1) t1 = g.prec[r * g.n_idx + k1];
      }
    }
    double lw0 = nan, lw1 = nan, w0 = 0.0, w1 = 0.0;
    if (a0.live) w0 = a0.weight(psis_neg_ll(x0, r, k0, g.y, g.prec, g.prec_size, g.n_idx), g.P, lw0);
    if (a1.live) w1 = a1.weight(psis_neg_ll(x1, r, k1, g.y, g.prec, g.prec_size, g.n_idx), g.P, lw1);
    if (F == F_MEAN) {
      f0 = x0; f1 = x1;
    } else if (F == F_CDF) {  // the Normal predictive distribution function at the observation
      f0 = 0.5 * erfc(-__dmul_rn(sqrt(t0), __dsub_rn(a0.y, x0)) * 0.70710678118654752440);
      f1 = 0.5 * erfc(-__dmul_rn(sqrt(t1), __dsub_rn(a1.y, x1)) * 0.70710678118654752440);
    }
    double q0 = 0.0, q1 = 0.0;
    if (g.want & LE_IP) {
      q0 = 1.0 / t0;
      q1 = g.prec_size == 1 ? q0 : 1.0 / t1;
    }
    if (a0.live) a0.add(g.want, w0, f0, q0);
    if (a1.live) a1.add(g.want, w1, f1, q1);
    if (g.lw_out) {
      if (ok0) g.lw_out[r * g.n_idx + k0] = lw0;
      if (ok1) g.lw_out[r * g.n_idx + k1] = lw1;
    }
  }
  if (g.want == 0) return;  // lw_out alone: nothing to join (uniform over the grid)
  sm[0][rr][c0] = a0.W; sm[1][rr][c0] = a0.mean; sm[2][rr][c0] = a0.m2; sm[3][rr][c0] = a0.below; sm[4][rr][c0] = a0.w2; sm[5][rr][c0] = a0.ip;
  sm[0][rr][c1] = a1.W; sm[1][rr][c1] = a1.mean; sm[2][rr][c1] = a1.m2; sm[3][rr][c1] = a1.below; sm[4][rr][c1] = a1.w2; sm[5][rr][c1] = a1.ip;
  __syncthreads();
  const int64_t e = (int64_t)blockIdx.x * LE_COLS + tid;
  if (tid < LE_COLS && e < g.kc) {
    double W = sm[0][0][tid], mean = sm[1][0][tid], m2 = sm[2][0][tid], below = sm[3][0][tid], w2 = sm[4][0][tid], ip = sm[5][0][tid];
    for (int q = 1; q < LE_ROWS; ++q) {
      omc_chan(W, mean, m2, sm[0][q][tid], sm[1][q][tid], sm[2][q][tid]);
      below += sm[3][q][tid]; w2 += sm[4][q][tid]; ip += sm[5][q][tid];
    }
    double* o = g.part + (int64_t)blockIdx.y * LE_PART * g.kc + e;
    o[0] = W; o[g.kc] = mean; o[2 * g.kc] = m2; o[3 * g.kc] = below; o[4 * g.kc] = w2; o[5 * g.kc] = ip;
  }
}

__global__ void __launch_bounds__(256) k_loo_join(int64_t k0, int64_t kc, int slices, int32_t want, const double* __restrict__ part,
                                                  const LooFit* __restrict__ fit, double* __restrict__ mean_out, double* __restrict__ var_out,
                                                  double* __restrict__ below_out, double* __restrict__ ess_out,
                                                  double* __restrict__ invprec_out, double* __restrict__ k_out, int64_t* __restrict__ tail_out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= kc) return;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const int64_t T = fit[e].T;
  const bool bad = T < 0;
  if (k_out) k_out[k0 + e] = bad ? nan : fit[e].khat;
  if (tail_out) tail_out[k0 + e] = T;
  if (want == 0) return;
  double W = 0.0, mean = 0.0, m2 = 0.0, below = 0.0, w2 = 0.0, ip = 0.0;
  for (int q = 0; q < slices; ++q) {
    const double* o = part + (int64_t)q * LE_PART * kc + e;
    omc_chan(W, mean, m2, o[0], o[kc], o[2 * kc]);
    below += o[3 * kc]; w2 += o[4 * kc]; ip += o[5 * kc];
  }
  if (mean_out) mean_out[k0 + e] = bad ? nan : mean;
  if (var_out) var_out[k0 + e] = bad ? nan : m2 / W;
  if (below_out) below_out[k0 + e] = bad ? nan : below / W;
  if (ess_out) ess_out[k0 + e] = bad ? nan : W * W / w2;
  if (invprec_out) invprec_out[k0 + e] = bad ? nan : ip / W;
}

template <int F>
void le_launch(omc_ctx* ctx, const dim3& grid, bool vec, const LooArgs& g) {
  if (vec) hipLaunchKernelGGL((k_loo_expect<true, F>), grid, dim3(256), 0, ctx->stream, g);
  else hipLaunchKernelGGL((k_loo_expect<false, F>), grid, dim3(256), 0, ctx->stream, g);
}

}  // namespace

extern "C" omc_status omc_store_loo_expect(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx, int64_t n_idx,
                                           const double* y, const double* prec, int64_t prec_size, const int64_t* tail_max, int32_t f_kind,
                                           const double* values, int64_t vsize, const int64_t* vidx, const double* thr, double* mean_out,
                                           double* var_out, double* below_out, double* ess_out, double* invprec_out, double* k_out,
                                           int64_t* tail_out, double* lw_out) {
  const char* own = nullptr;  // what this entry point alone asks of its arguments
  if (f_kind < F_ENTRY || f_kind > F_CDF) own = "f_kind must be 0 (entry), 1 (mean) or 2 (cdf)";
  else if (f_kind == F_ENTRY && (!values || vsize < 1)) own = "f_kind entry needs values and vsize >= 1";
  else if (f_kind == F_ENTRY && !vidx && n_idx != vsize) own = "f_kind entry without vidx needs n_idx == vsize";
  else if (f_kind != F_ENTRY && !y) own = "f_kind mean and cdf need y and prec (a mean entry)";
  else if (invprec_out && !y) own = "invprec_out needs y and prec (a mean entry)";
  else if ((below_out != nullptr) != (thr != nullptr)) own = "below_out and thr must be given together";
  else if (!mean_out && !var_out && !below_out && !ess_out && !invprec_out && !k_out && !tail_out && !lw_out) own = "every output is NULL";
  const PsisCall c = {n_iter, size, store, idx, n_idx, y, prec, prec_size, tail_max};
  omc_status st = psis_prelude(ctx, "omc_store_loo_expect", c, store && tail_max ? nullptr : "store and tail_max must not be NULL", own,
                               f_kind == F_ENTRY ? vidx : nullptr, vsize);
  if (st != OMC_OK) return st;
  const int64_t S = n_iter * ctx->n_chains, P = rank_pow2(S);
  int64_t rpb;  // slices over the whole selection: a function of (S, n_idx) alone and not of the chunk
  const int64_t slices = omc_row_slices((n_idx + LE_COLS - 1) / LE_COLS, S, &rpb);
  RankCarve ws(ctx, (size_t)P * sizeof(uint64_t) + sizeof(LooFit) + (size_t)slices * LE_PART * sizeof(double) + sizeof(int32_t), n_idx);
  const int64_t Kc = ws.Kc;
  uint64_t* keys = ws.take<uint64_t>((size_t)Kc * P);
  LooFit* fit = ws.take<LooFit>(Kc);
  double* part = ws.take<double>((size_t)Kc * slices * LE_PART);
  int32_t* flags = ws.take<int32_t>(Kc);
  st = ws.done();
  if (st != OMC_OK) return st;
  LooArgs g;
  g.store = store; g.idx = idx; g.y = y; g.prec = prec; g.values = f_kind == F_ENTRY ? values : nullptr;
  g.vidx = f_kind == F_ENTRY ? vidx : nullptr; g.thr = thr; g.keys = keys; g.fit = fit; g.part = part; g.lw_out = lw_out;
  g.S = S; g.P = P; g.size = size; g.vsize = vsize; g.n_idx = n_idx; g.prec_size = prec_size; g.rows_per_block = rpb;
  g.k0 = 0; g.kc = 0;
  g.want = ((mean_out || var_out) ? LE_MOM : 0) | (below_out ? LE_BELOW : 0) | (ess_out ? LE_ESS : 0) | (invprec_out ? LE_IP : 0);
  const bool pass = g.want != 0 || lw_out != nullptr;  // else k_out and tail_out alone: the fit is all there is to do
  bool vec_ok = !idx && size % 2 == 0 && ((uintptr_t)store & 15) == 0;
  if (f_kind == F_ENTRY) vec_ok = vec_ok && !vidx && vsize % 2 == 0 && ((uintptr_t)values & 15) == 0;
  for (int64_t k0 = 0; k0 < n_idx; k0 += Kc) {
    const int64_t kc = n_idx - k0 < Kc ? n_idx - k0 : Kc;
    st = psis_gather_sort(ctx, c, k0, kc, S, P, keys, flags);
    if (st != OMC_OK) return st;
    hipLaunchKernelGGL(k_loo_fit, dim3((unsigned)kc), dim3(PSIS_THREADS), 0, ctx->stream, k0, S, P, keys, flags, tail_max, fit);
    OMC_HIP_CHECK(hipGetLastError());
    if (pass) {
      g.k0 = k0; g.kc = kc;
      const dim3 egrid((unsigned)((kc + LE_COLS - 1) / LE_COLS), (unsigned)slices);
      const bool vec = vec_ok && k0 % 2 == 0 && kc % 2 == 0;
      if (f_kind == F_ENTRY) le_launch<F_ENTRY>(ctx, egrid, vec, g);
      else if (f_kind == F_MEAN) le_launch<F_MEAN>(ctx, egrid, vec, g);
      else le_launch<F_CDF>(ctx, egrid, vec, g);
      OMC_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_loo_join, dim3((unsigned)((kc + 255) / 256)), dim3(256), 0, ctx->stream, k0, kc, (int)slices, g.want, part, fit,
                       mean_out, var_out, below_out, ess_out, invprec_out, k_out, tail_out);
    OMC_HIP_CHECK(hipGetLastError());
  }
  return OMC_OK;
}
