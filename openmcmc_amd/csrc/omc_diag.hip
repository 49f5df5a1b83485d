// Convergence diagnostics of the device-resident store: split R-hat and the effective sample size (ESS) of every element,
// without moving the store off the GPU ("device store, on-device summaries").
//
// store is [N][C][size].  Every chain is split into its first and its last M = N / 2 iterations (the middle draw of an odd
// N is dropped): J = 2 C series x_j[0..M) per element.  What is computed (include/omcmc_hip.h, omc_store_rhat_ess):
//   m_j = mean(x_j),  S(t) = sum_j sum_{i=0}^{M-1-t} (x_j[i] - m_j)(x_j[i+t] - m_j)   (= J M mean_j g_j(t))
//   W = S(0) / (J (M - 1)),  B_M = var(m_j, ddof 1),  var_plus = W (M - 1) / M + B_M,  rhat = sqrt(var_plus / W),
//   rho(t) = 1 - (W - S(t) / (J M)) / var_plus, and Geyer's initial monotone sequence on rho for the ESS.
//
// Series means are taken around the series' first draw (m = x[0] + mean(x - x[0])), and the variance of the means by
// Welford / Chan updates (omc_moments.h): a constant series then has deviations of exactly zero, equal means a variance of exactly zero, so
// the edge cases of the contract (every draw equal; W == 0 < B_M) are exact tests, not tolerances.
//
// Lag sums, one lane per (series, element), consecutive lanes on consecutive elements (every row load a coalesced run of
// the [C][size] slab): the lane streams i over its M draws and keeps the last L lagged operands in a register ring, so a
// block of L lags costs L FMAs per draw.  The loop is unrolled by L: every ring index is a compile-time constant.
//   short form (M <= 64): a workgroup stages one chain's two halves for 64 elements in LDS (one read of the store) and
//     computes means and every lag from there -- eight waves, each one half and 16 of the 64 lags;
//   long form: a means pass, then blocks of L = 32 lags (32 accumulators and a 32-slot ring: 256 VGPRs, no scratch); block 0 reads the store once (x[i] is its own lagged operand:
//     the second load of the address is served by the cache), every later block twice (x[i] and x[i - t0]).  Blocks stop when every element's Geyer sequence has ended.
// A workgroup covers 64 elements and a fixed group of series; it writes one partial per (group, lag, element), and
// k_diag_step adds the groups' partials in a fixed order and advances each element's Geyer state by the block.  The number
// of groups depends on C and size only: repeated calls are bit-equal.  No floating-point atomics anywhere.
#include <math.h>

#include "omc_common.h"
#include "omc_geyer.h"
#include "omc_lag_block.h"
#include "omc_moments.h"

namespace {

constexpr int D_TILE = 64;    // elements per workgroup (one wave's lanes)
constexpr int D_L = 32;       // lags per block
constexpr int D_SHORT = 64;   // longest half-series of the short form (every lag in one pass)
constexpr int D_STATE = 8;    // per-element Geyer state, [D_STATE][size]

// d_lag_block<L>(t0, M, y, post, acc) (omc_lag_block.h): with z(i) = post(y(i)), acc[l] += sum_{i = t0 + l}^{M-1} z(i) z(i - t0 - l),
// l < L, the lane's contribution to S(t0 + l)

// Long form, pass 1: the two split means of every (chain, element); the middle draw of an odd N only for its NaN.
// means [J][size], series j = 2 c + h
__global__ void __launch_bounds__(256) k_diag_means(const double* __restrict__ store, int64_t N, int64_t M, int64_t C, int64_t size,
                                                    double* __restrict__ means) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= C * size) return;
  const int64_t row = C * size;
  const double* p = store + idx;  // idx = c * size + k
  double mid = 0.0;
  if (N & 1) mid = p[M * row];
  for (int h = 0; h < 2; ++h) {
    const double* q = p + (h ? N - M : 0) * row;
    const double x0 = q[0];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    int64_t i = 0;
    for (; i + 4 <= M; i += 4) {
      double v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = q[(i + u) * row];
#pragma unroll
      for (int u = 0; u < 4; ++u) s[u] += v[u] - x0;
    }
    for (; i < M; ++i) s[0] += q[i * row] - x0;
    double m = x0 + ((s[0] + s[1]) + (s[2] + s[3])) / (double)M;
    if (mid != mid) m = mid;
    means[(2 * (idx / size) + h) * size + idx % size] = m;
  }
}

// Long form, one block of L lags [t0, t0 + L): workgroup (tile, group g) = 64 elements x series [g spg, (g + 1) spg),
// four waves taking every fourth series.  part [G][L][size]; block 0 also writes the groups' moments of the series means,
// part_b [G][3][size].  Tiles without an active element (tile_active, NULL in block 0) return at once.
template <int L>
__global__ void __launch_bounds__(256) k_diag_lags(const double* __restrict__ store, int64_t N, int64_t M, int64_t C, int64_t size,
                                                   const double* __restrict__ means, int64_t t0, int64_t spg,
                                                   const int32_t* __restrict__ tile_active, double* __restrict__ part,
                                                   double* __restrict__ part_b) {
  __shared__ double red[L][D_TILE];
  __shared__ double redb[3][D_TILE];
  const int tile = blockIdx.x, g = blockIdx.y;
  if (tile_active && !tile_active[tile]) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t k = (int64_t)tile * D_TILE + lane;
  const int64_t kc = k < size ? k : size - 1;  // lanes past the end read a valid element and write nothing
  const int64_t J = 2 * C, row = C * size;
  const int64_t s1 = (g + 1) * spg < J ? (g + 1) * spg : J;
  double acc[L];
#pragma unroll
  for (int l = 0; l < L; ++l) acc[l] = 0.0;
  double bn = 0.0, bm = 0.0, bq = 0.0;
  for (int64_t s = (int64_t)g * spg + wave; s < s1; s += 4) {
    const double m = means[s * size + kc];
    const double* q = store + (s >> 1) * size + kc + ((s & 1) ? N - M : 0) * row;
    d_lag_block<L>(t0, M, [&](int64_t i) { return q[i * row]; }, [&](double x) { return x - m; }, acc);
    if (t0 == 0) omc_welford(bn, bm, bq, m);
  }
  // the four waves' sums in a fixed order: ((w3 + w2) + w1) + w0
  for (int w = 3; w >= 0; --w) {
    if (wave == w) {
#pragma unroll
      for (int l = 0; l < L; ++l) {
        const double v = w == 3 ? acc[l] : acc[l] + red[l][lane];
        if (w > 0) red[l][lane] = v;
        else if (k < size) part[((int64_t)g * L + l) * size + k] = v;
      }
      if (t0 == 0) {
        if (w < 3) omc_chan(bn, bm, bq, redb[0][lane], redb[1][lane], redb[2][lane]);
        if (w > 0) {
          redb[0][lane] = bn; redb[1][lane] = bm; redb[2][lane] = bq;
        } else if (k < size) {
          double* o = part_b + (int64_t)g * 3 * size;
          o[k] = bn; o[size + k] = bm; o[2 * size + k] = bq;
        }
      }
    }
    __syncthreads();
  }
}

// Short form (M <= 64): workgroup (tile, group g) = 64 elements x chains [g cpg, (g + 1) cpg), eight waves.  Per chain: its
// two halves (and the middle draw of an odd N, for its NaN) into LDS [2][M][64], then wave w takes half w >> 2 and the 16
// lags [16 (w & 3), 16 (w & 3) + 16).  part [G][64][size], part_b [G][3][size].
constexpr int S_L = 16;  // lags per wave of the short form (16 accumulators and a 16-slot ring: 160 VGPRs, no scratch)
__global__ void __launch_bounds__(512) k_diag_short(const double* __restrict__ store, int64_t N, int64_t M, int64_t C, int64_t size,
                                                    int64_t cpg, double* __restrict__ part, double* __restrict__ part_b) {
  extern __shared__ double xs[];  // [2][M][64] draws, reused for the sums of the waves at the end ([64][64] at least)
  __shared__ double mid[D_TILE];
  __shared__ double redb[3][D_TILE];
  const int tile = blockIdx.x, g = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = wave >> 2, blk = wave & 3;
  const int64_t k = (int64_t)tile * D_TILE + lane;
  const int64_t kc = k < size ? k : size - 1;
  const int64_t row = C * size;
  const int64_t c1 = (g + 1) * cpg < C ? (g + 1) * cpg : C;
  double acc[S_L];
#pragma unroll
  for (int l = 0; l < S_L; ++l) acc[l] = 0.0;
  double bn = 0.0, bm = 0.0, bq = 0.0;
  const double* xh = xs + (int64_t)h * M * D_TILE + lane;
  for (int64_t c = (int64_t)g * cpg; c < c1; ++c) {
    const double* q = store + c * size + kc;
    // 2 M rows of 64 elements, eight waves on every eighth row: a chain of independent loads
#pragma unroll 8
    for (int64_t r = wave; r < 2 * M; r += 8) xs[r * D_TILE + lane] = q[(r < M ? r : r - M + (N - M)) * row];
    if (wave == 0) mid[lane] = (N & 1) ? q[M * row] : 0.0;
    __syncthreads();
    const double x0 = xh[0];
    double s = 0.0;
    for (int64_t i = 0; i < M; ++i) s += xh[i * D_TILE] - x0;
    double m = x0 + s / (double)M;
    if (mid[lane] != mid[lane]) m = mid[lane];
    d_lag_block<S_L>(S_L * blk, M, [&](int64_t i) { return xh[i * D_TILE]; }, [&](double x) { return x - m; }, acc);
    if (blk == 0) omc_welford(bn, bm, bq, m);
    __syncthreads();
  }
  // lag 16 blk + l: half 0 (wave blk) + half 1 (wave 4 + blk); moments of the means: wave 0, then wave 4
  double* red = xs;  // [64][64]
  if (h == 1) {
#pragma unroll
    for (int l = 0; l < S_L; ++l) red[(blk * S_L + l) * D_TILE + lane] = acc[l];
    if (blk == 0) { redb[0][lane] = bn; redb[1][lane] = bm; redb[2][lane] = bq; }
  }
  __syncthreads();
  if (h == 0 && k < size) {
#pragma unroll
    for (int l = 0; l < S_L; ++l) part[((int64_t)g * D_SHORT + blk * S_L + l) * size + k] = acc[l] + red[(blk * S_L + l) * D_TILE + lane];
    if (blk == 0) {
      omc_chan(bn, bm, bq, redb[0][lane], redb[1][lane], redb[2][lane]);
      double* o = part_b + (int64_t)g * 3 * size;
      o[k] = bn; o[size + k] = bm; o[2 * size + k] = bq;
    }
  }
}

// The groups' partials of one pass added in group order, one thread per (lag, element): the total lands in group 0's slot
// (each thread reads and writes its own column only).  part [G][nl][size]
__global__ void __launch_bounds__(256) k_diag_sum(int64_t size, int nl, int G, double* __restrict__ part) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int l = blockIdx.y;
  if (k >= size) return;
  double v = 0.0;
  for (int gg = 0; gg < G; ++gg) v += part[((int64_t)gg * nl + l) * size + k];
  part[(int64_t)l * size + k] = v;
}

// One thread per element, one wave per tile: the sums S(t) of lags [t0, t0 + nl) (k_diag_sum's totals), then the
// element's Geyer state advanced by the rule of omc_geyer.h (t0 == 0: W, B_M, rhat and the state set up first).  st [D_STATE][size]:
//   0 W, 1 var_plus, 2 even, 3 odd (the last evaluated pair), 4 sum of the monotone pair sums so far, 5 their running
//   minimum, 6 index of the last evaluated pair, 7 1 while the sequence goes on.
// tile_active[tile]: the tile still holds an active element; *any_active set when any tile does.
__global__ void __launch_bounds__(64) k_diag_step(int64_t size, int64_t M, int64_t J, int G, int64_t t0, int nl, const double* __restrict__ part,
                                                  const double* __restrict__ part_b, double* __restrict__ st, int32_t* __restrict__ tile_active,
                                                  int32_t* __restrict__ any_active, double* __restrict__ rhat_out, double* __restrict__ ess_out,
                                                  int32_t* __restrict__ lag_out) {
  const int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x;
  bool active = false;
  if (k < size) {
    const double JM = (double)J * (double)M;
    auto S = [&](int64_t t) { return part[(t - t0) * size + k]; };  // S(t), t in [t0, t0 + nl)
    GeyerState g = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool go = true;
    if (t0 == 0) {
      double bn = 0.0, bm = 0.0, bq = 0.0;
      for (int gg = 0; gg < G; ++gg) {
        const double* o = part_b + (int64_t)gg * 3 * size;
        omc_chan(bn, bm, bq, o[k], o[size + k], o[2 * size + k]);
      }
      const double BM = bq / (double)(J - 1);
      const double nan = __longlong_as_double(0x7ff8000000000000LL);
      const int kind = geyer_start(g, S(0), BM, J, M, S);
      if (kind != GEYER_GO) {  // a NaN draw somewhere in the element, or every draw equal
        if (rhat_out) rhat_out[k] = nan;
        if (ess_out) ess_out[k] = kind == GEYER_NAN ? nan : JM;
        if (lag_out) lag_out[k] = 0;
        go = false;
      } else if (rhat_out) {
        rhat_out[k] = sqrt(g.vp / g.W);  // +inf when W == 0 < B_M
      }
    } else {
      go = st[7 * size + k] != 0.0;
      g.W = st[k]; g.vp = st[size + k]; g.even = st[2 * size + k]; g.odd = st[3 * size + k];
      g.acc = st[4 * size + k]; g.minq = st[5 * size + k]; g.pp = st[6 * size + k];
    }
    if (go) {
      if (geyer_advance(g, M, JM, t0 + nl, S)) {
        double ess;
        int32_t lags;
        geyer_finish(g, JM, ess, lags);
        if (ess_out) ess_out[k] = ess;
        if (lag_out) lag_out[k] = lags;
      } else {
        active = true;
      }
    }
    st[k] = g.W; st[size + k] = g.vp; st[2 * size + k] = g.even; st[3 * size + k] = g.odd;
    st[4 * size + k] = g.acc; st[5 * size + k] = g.minq; st[6 * size + k] = g.pp; st[7 * size + k] = active ? 1.0 : 0.0;
  }
  const bool any = __ballot(active) != 0;
  if (threadIdx.x == 0) {
    tile_active[blockIdx.x] = any ? 1 : 0;
    if (any) atomicOr(any_active, 1);
  }
}

}  // namespace

extern "C" omc_status omc_store_rhat_ess(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, double* rhat_out,
                                         double* ess_out, int32_t* lag_out) {
  if (!ctx || n_iter < 4 || size < 1 || !store) return OMC_INVALID_ARG;
  const int64_t C = ctx->n_chains, J = 2 * C, M = n_iter / 2;
  if (ctx->diag_algo == 1 && M > D_SHORT) return OMC_INVALID_ARG;  // the short form holds at most 64 draws per half
  const bool short_form = ctx->diag_algo == 1 || (ctx->diag_algo == 0 && M <= D_SHORT);
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  const int64_t tiles = (size + D_TILE - 1) / D_TILE;
  if (tiles > 0x7fffffffLL || C * size / 256 > 0x7fffffffLL) return OMC_INVALID_ARG;
  // groups of series (long form: of four; short form: whole chains) for about 2048 workgroups: a function of C and size only
  const int64_t units = short_form ? C : (J + 3) / 4;
  int64_t G = (2048 + tiles - 1) / tiles;
  if (G > units) G = units;
  if (G > 65535) G = 65535;
  const int64_t per = (units + G - 1) / G;  // units per group
  G = (units + per - 1) / per;
  const int nl = short_form ? D_SHORT : D_L;
  // workspace: partial lag sums [G][nl][size], partial moments of the means [G][3][size], state [D_STATE][size],
  // long form also the means [J][size]; tile flags and the any-active word
  const size_t n_part = (size_t)G * nl * size, n_b = (size_t)G * 3 * size, n_st = (size_t)D_STATE * size;
  const size_t n_means = short_form ? 0 : (size_t)J * size;
  const size_t bytes = (n_part + n_b + n_st + n_means) * sizeof(double) + (size_t)(tiles + 1) * sizeof(int32_t);
  omc_status s0 = omc_ensure(ctx, ctx->store_ws, bytes);
  if (s0 != OMC_OK) return s0;
  double* part = (double*)ctx->store_ws.p;
  double* part_b = part + n_part;
  double* st = part_b + n_b;
  double* means = st + n_st;
  int32_t* tile_active = (int32_t*)(means + n_means);
  int32_t* any_active = tile_active + tiles;
  hipStream_t s = ctx->stream;
  const dim3 grid((unsigned)tiles, (unsigned)G);
  if (short_form) {
    const size_t lds = (size_t)2 * (M > D_SHORT / 2 ? M : D_SHORT / 2) * D_TILE * sizeof(double);
    hipLaunchKernelGGL(k_diag_short, grid, dim3(512), lds, s, store, n_iter, M, C, size, per, part, part_b);
    hipLaunchKernelGGL(k_diag_sum, dim3((unsigned)((size + 255) / 256), (unsigned)nl), dim3(256), 0, s, size, nl, (int)G, part);
    hipLaunchKernelGGL(k_diag_step, dim3((unsigned)tiles), dim3(64), 0, s, size, M, J, (int)G, (int64_t)0, nl, part, part_b, st,
                       tile_active, any_active, rhat_out, ess_out, lag_out);
    OMC_HIP_CHECK(hipGetLastError());
    return OMC_OK;
  }
  hipLaunchKernelGGL(k_diag_means, dim3((unsigned)((C * size + 255) / 256)), dim3(256), 0, s, store, n_iter, M, C, size, means);
  for (int64_t t0 = 0; t0 < M; t0 += D_L) {
    hipLaunchKernelGGL(k_diag_lags<D_L>, grid, dim3(256), 0, s, store, n_iter, M, C, size, means, t0, 4 * per,
                       t0 == 0 ? (const int32_t*)nullptr : (const int32_t*)tile_active, part, part_b);
    hipLaunchKernelGGL(k_diag_sum, dim3((unsigned)((size + 255) / 256), (unsigned)nl), dim3(256), 0, s, size, nl, (int)G, part);
    OMC_HIP_CHECK(hipMemsetAsync(any_active, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(k_diag_step, dim3((unsigned)tiles), dim3(64), 0, s, size, M, J, (int)G, t0, nl, part, part_b, st, tile_active,
                       any_active, rhat_out, ess_out, lag_out);
    OMC_HIP_CHECK(hipGetLastError());
    int32_t any = 0;  // one word per pass: does any element still need lags?
    OMC_HIP_CHECK(hipMemcpyAsync(&any, any_active, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    OMC_HIP_CHECK(hipStreamSynchronize(s));
    if (!any) break;
  }
  return OMC_OK;
}
