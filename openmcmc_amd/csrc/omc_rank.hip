// Ranks of the device-resident store and the rank-normalised diagnostics built on them (Vehtari, Gelman, Simpson, Carpenter,
// Buerkner 2021): rank-normalised split R-hat (bulk and folded), bulk-ESS and tail-ESS, without moving the store off the GPU.
// The contract is in include/omcmc_hip.h (omc_store_ranks, omc_store_rank_diagnostics, omc_store_rank_schedule).
//
// store is [N][C][size].  A chunk of Kc selected elements is worked on at a time:
//   k_rank_gather  (omc_store_shared.hip, through rank_gather_sort) the gather tile of omc_rank_sort.h: the draws of the chunk,
//                  read where they lie, as order-preserving 64-bit keys (-0.0 first made +0.0) in columns keys [Kc][P], P the next power of two >= the S draws of a column, the
//                  rest of a column the all-ones key; it notes per element whether a NaN (bit 0) or an infinity (bit 1) was
//                  seen.  With `fold` the value is |x - med|, med the element's median from k_rank_stats.
//   rank_sort      the key-only bitonic sort of every column (omc_store_shared.hip, shared with omc_hdi.hip).
//   k_rank_emit    for every draw the number of smaller and of equal keys by bisection in its sorted column (ties are exact, no
//                  payload is carried through the sort; the second bisection only where the next key is equal): the average rank, or z = ndtri((r - 3/8) / (S + 1/4)), and with the
//                  same read of the store the tail indicators x <= q05, x <= q95.
//   k_rank_stats   median and the two tail quantiles from the sorted column, numpy's interpolation (omc_quantile.h).
// The four series of a chunk -- z, z of the folded draws, the two indicators -- lie side by side as one store [N][C][4 Kc], and
// ONE call of omc_store_rhat_ess runs over them (it uses ctx->store_ws; everything here lives in ctx->rank_ws).
//
// Kc: the workspace of a chunk is Kc (8 P + 32 N C + 100) bytes -- keys, the four series, per-element words -- and Kc is what fits
// RANK_BUDGET (omc_rank_sort.h), at least 1; option "rank_chunk" forces it.
#include <math.h>

#include <vector>

#include "omc_common.h"
#include "omc_quantile.h"
#include "omc_rank_sort.h"
#include "omc_store_view.h"
#include "omc_truncnorm.h"

namespace {

// stats [Kc][3] = median ((a + b) / 2 of the two middle order statistics: S is even), q05, q95 of the S sorted draws
__global__ void k_rank_stats(int64_t Kc, int64_t S, int64_t P, const uint64_t* __restrict__ keys, double* __restrict__ stats) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= Kc) return;
  const uint64_t* col = keys + e * P;
  stats[3 * e] = (q_val(col[S / 2 - 1]) + q_val(col[S / 2])) / 2.0;
  for (int t = 0; t < 2; ++t) {
    int64_t lo, hi;
    double fr;
    q_ranks(S, t ? 0.95 : 0.05, lo, hi, fr);
    stats[3 * e + 1 + t] = q_lerp(q_val(col[lo]), q_val(col[hi]), fr);
  }
}

enum { RANK_EMIT_RANKS = 0, RANK_EMIT_Z = 1, RANK_EMIT_ZFOLD = 2 };
struct RankEmit {
  const double* store; const int64_t* idx; const uint64_t* keys; const int32_t* flags; const double* stats; double* out;
  int64_t k0, Kc, size, C, S, P, n_rows, mid_row0, ld_out;
  int mode;
};

// One thread per (row of the store, element of the chunk): a wave takes 64 consecutive rows of ONE element, the four waves of a
// workgroup four adjacent elements over the same rows, and the workgroups walk the rows first.  What is in flight at a time then
// bisects in a handful of columns, which stay in L2; with the elements on consecutive lanes instead, every lane of a load looked into
// another column and the lower levels of every bisection missed L2, a 128-byte line for 8 bytes (6.1 ms per launch for 204
// columns of 131 072 keys, against 2.1 ms for sorting them).  The four waves read neighbouring 8-byte pieces of the same lines of the
// store and write neighbouring pieces of the output rows.
//   RANKS: out[row ld_out + k0 + e] = average rank, NaN in the middle row and for an element with a NaN draw;
//   Z:     out = series [n_rows][4 Kc]: z at e, the indicators x <= q05 at 2 Kc + e and x <= q95 at 3 Kc + e;
//   ZFOLD: z of |x - med| at Kc + e.  (Z, ZFOLD: zeros in the middle row and for an element with a non-finite draw.)
__global__ void __launch_bounds__(256) k_rank_emit(RankEmit a) {
  const int64_t row = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63), e = (int64_t)blockIdx.y * 4 + (threadIdx.x >> 6);
  if (row >= a.n_rows || e >= a.Kc) return;
  const bool mid = a.mid_row0 >= 0 && row >= a.mid_row0 && row < a.mid_row0 + a.C;
  const int32_t fl = a.flags[e];
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const bool dead = mid || (a.mode == RANK_EMIT_RANKS ? (fl & 1) != 0 : fl != 0);
  double r = 0.0, x = 0.0;
  if (!dead) {
    x = a.store[row * a.size + (a.idx ? a.idx[a.k0 + e] : a.k0 + e)];
    const double v = a.mode == RANK_EMIT_ZFOLD ? fabs(x - a.stats[3 * e]) : x;
    const uint64_t key = rank_key(v);
    const uint64_t* col = a.keys + e * a.P;
    // the draw is in its column, so col[less] == key; where the next key is already larger -- nearly always with continuous draws --
    // the second bisection is not needed
    const int64_t less = rank_bound(col, a.P, key, false);
    const int64_t le = (less + 1 >= a.P || col[less + 1] > key) ? less + 1 : rank_bound(col, a.P, key, true);
    r = (double)less + 0.5 * (double)(le - less + 1);
  }
  if (a.mode == RANK_EMIT_RANKS) {
    a.out[row * a.ld_out + a.k0 + e] = dead ? nan : r;
    return;
  }
  const double z = dead ? 0.0 : omc_ndtri_as241((r - 0.375) / ((double)a.S + 0.25));
  double* o = a.out + row * 4 * a.Kc + e;
  if (a.mode == RANK_EMIT_ZFOLD) {
    o[a.Kc] = z;
  } else {
    o[0] = z;
    o[2 * a.Kc] = (!dead && x <= a.stats[3 * e + 1]) ? 1.0 : 0.0;
    o[3 * a.Kc] = (!dead && x <= a.stats[3 * e + 2]) ? 1.0 : 0.0;
  }
}

// rh4, es4 [4 Kc]: omc_store_rhat_ess of the four series
__global__ void k_rank_combine(int64_t Kc, int64_t k0, const int32_t* __restrict__ flags, const double* __restrict__ rh4,
                               const double* __restrict__ es4, double* __restrict__ rhat_out, double* __restrict__ bulk_out,
                               double* __restrict__ tail_out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= Kc) return;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const bool bad = flags[e] != 0;
  const double ra = rh4[e], rb = rh4[Kc + e], ta = es4[2 * Kc + e], tb = es4[3 * Kc + e];
  if (rhat_out) rhat_out[k0 + e] = (bad || ra != ra || rb != rb) ? nan : (ra > rb ? ra : rb);
  if (bulk_out) bulk_out[k0 + e] = bad ? nan : es4[e];
  if (tail_out) tail_out[k0 + e] = (bad || ta != ta || tb != tb) ? nan : (ta < tb ? ta : tb);
}

dim3 rank_emit_grid(const RankEmit& a) { return dim3((unsigned)((a.n_rows + 63) / 64), (unsigned)((a.Kc + 3) / 4)); }

}  // namespace

extern "C" omc_status omc_store_rank_schedule(int64_t S, int32_t tile, int64_t* out, int64_t cap, int64_t* n_out) {
  if (S < 1 || !n_out || cap < 0 || (cap > 0 && !out)) return OMC_INVALID_ARG;
  if (tile != 0 && (tile < 64 || tile > RANK_TILE_DEFAULT || (tile & (tile - 1)))) return OMC_INVALID_ARG;
  const std::vector<RankLaunch> L = rank_schedule(rank_pow2(S), tile ? tile : RANK_TILE_DEFAULT);
  *n_out = (int64_t)L.size();
  if ((int64_t)L.size() > cap) return OMC_INVALID_ARG;
  for (size_t i = 0; i < L.size(); ++i) {
    out[3 * i] = L[i].kind; out[3 * i + 1] = L[i].k; out[3 * i + 2] = L[i].j;
  }
  return OMC_OK;
}

extern "C" omc_status omc_store_ranks(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx, int64_t n_idx,
                                      int32_t split, double* rank_out) {
  if (!omc_selection_ok(ctx, n_iter, split ? 4 : 1, size, store, idx, n_idx) || !rank_out) return OMC_INVALID_ARG;
  const int64_t N = n_iter, C = ctx->n_chains;
  const RankGeom g = rank_geom(N, C, split != 0);
  if ((N * C + 63) / 64 > 0x7fffffffLL) return OMC_INVALID_ARG;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  RankCarve ws(ctx, (size_t)g.P * sizeof(uint64_t) + sizeof(int32_t), n_idx);
  const int64_t Kc = ws.Kc;
  uint64_t* keys = ws.take<uint64_t>((size_t)Kc * g.P);
  int32_t* flags = ws.take<int32_t>(Kc);
  omc_status st = ws.done();
  if (st == OMC_OK) st = omc_store_check_index(ctx, ws.head(), idx, n_idx, size);
  if (st != OMC_OK) return st;
  for (int64_t k0 = 0; k0 < n_idx; k0 += Kc) {
    const int64_t kc = n_idx - k0 < Kc ? n_idx - k0 : Kc;
    st = rank_gather_sort(ctx, store, idx, k0, kc, size, g, nullptr, keys, flags);
    if (st != OMC_OK) return st;
    RankEmit a;
    a.store = store; a.idx = idx; a.keys = keys; a.flags = flags; a.stats = nullptr; a.out = rank_out;
    a.k0 = k0; a.Kc = kc; a.size = size; a.C = C; a.S = g.S; a.P = g.P; a.n_rows = N * C; a.mid_row0 = g.mid_row0; a.ld_out = n_idx;
    a.mode = RANK_EMIT_RANKS;
    hipLaunchKernelGGL(k_rank_emit, rank_emit_grid(a), dim3(256), 0, ctx->stream, a);
    OMC_HIP_CHECK(hipGetLastError());
  }
  return OMC_OK;
}

extern "C" omc_status omc_store_rank_diagnostics(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx,
                                                 int64_t n_idx, double* rhat_out, double* ess_bulk_out, double* ess_tail_out) {
  if (!omc_selection_ok(ctx, n_iter, 4, size, store, idx, n_idx)) return OMC_INVALID_ARG;
  const int64_t N = n_iter, C = ctx->n_chains;
  const RankGeom g = rank_geom(N, C, true);
  if ((N * C + 63) / 64 > 0x7fffffffLL) return OMC_INVALID_ARG;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  // per element: keys [P], the four series [N C][4], median and two quantiles, R-hat and ESS of the four series, the flag word
  RankCarve ws(ctx, (size_t)g.P * sizeof(uint64_t) + (size_t)N * C * 4 * sizeof(double) + (3 + 8) * sizeof(double) + sizeof(int32_t), n_idx);
  const int64_t Kc = ws.Kc;
  uint64_t* keys = ws.take<uint64_t>((size_t)Kc * g.P);
  double* series = ws.take<double>((size_t)N * C * 4 * Kc);
  double* stats = ws.take<double>(3 * Kc);
  double* rh4 = ws.take<double>(4 * Kc);
  double* es4 = ws.take<double>(4 * Kc);
  int32_t* flags = ws.take<int32_t>(Kc);
  omc_status st = ws.done();
  if (st == OMC_OK) st = omc_store_check_index(ctx, ws.head(), idx, n_idx, size);
  if (st != OMC_OK) return st;
  hipStream_t s = ctx->stream;
  for (int64_t k0 = 0; k0 < n_idx; k0 += Kc) {
    const int64_t kc = n_idx - k0 < Kc ? n_idx - k0 : Kc;
    RankEmit a;
    a.store = store; a.idx = idx; a.keys = keys; a.flags = flags; a.stats = stats; a.out = series;
    a.k0 = k0; a.Kc = kc; a.size = size; a.C = C; a.S = g.S; a.P = g.P; a.n_rows = N * C; a.mid_row0 = g.mid_row0; a.ld_out = 0;
    // the draws: z and the tail indicators
    st = rank_gather_sort(ctx, store, idx, k0, kc, size, g, nullptr, keys, flags);
    if (st != OMC_OK) return st;
    hipLaunchKernelGGL(k_rank_stats, dim3((unsigned)((kc + 255) / 256)), dim3(256), 0, s, kc, g.S, g.P, keys, stats);
    a.mode = RANK_EMIT_Z;
    hipLaunchKernelGGL(k_rank_emit, rank_emit_grid(a), dim3(256), 0, s, a);
    // the folded draws |x - med|
    st = rank_gather_sort(ctx, store, idx, k0, kc, size, g, stats, keys, nullptr);
    if (st != OMC_OK) return st;
    a.mode = RANK_EMIT_ZFOLD;
    hipLaunchKernelGGL(k_rank_emit, rank_emit_grid(a), dim3(256), 0, s, a);
    OMC_HIP_CHECK(hipGetLastError());
    st = omc_store_rhat_ess(ctx, N, 4 * kc, series, rh4, es4, nullptr);
    if (st != OMC_OK) return st;
    hipLaunchKernelGGL(k_rank_combine, dim3((unsigned)((kc + 255) / 256)), dim3(256), 0, s, kc, k0, flags, rh4, es4, rhat_out, ess_bulk_out,
                       ess_tail_out);
    OMC_HIP_CHECK(hipGetLastError());
  }
  return OMC_OK;
}
