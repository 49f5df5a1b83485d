// Highest-density intervals of the device-resident store: for every selected column of draws the shortest interval between two
// stored draws that holds a given share of them (ArviZ's unimodal hdi).  The contract is in include/omcmc_hip.h (omc_store_hdi).
//
// store is [N][C][size].  A column is all N C draws of an element (pooled, S = N C) or the N draws of one chain of it (per
// chain, S = N, CC = C columns per element).  A chunk of Kc selected elements, Kc CC columns, is worked on at a time; column
// q = c Kc + e of the chunk belongs to chain c (0 when pooled) of element e:
//   k_hdi_gather   the gather tile of omc_rank_sort.h: the draws, read where they lie, as order-preserving keys in columns
//                  keys [Kc CC][P], P the next power of two >= S.  A NaN draw takes the all-ones key, which is also the padding:
//                  both sort behind every number.  It notes per column whether a NaN (bit 0) or an infinity (bit 1) was seen.
//   rank_sort      the key-only bitonic sort of every column (omc_store_shared.hip, shared with omc_rank.hip).
//   k_hdi_count    n = the keys of a sorted column below the all-ones key, by bisection: the draws that are not NaN.
//   k_hdi_window   for every probability of the call m = min(floor(prob n), n - 1) and the minimum over i = 0 .. n - m - 1 of
//                  (w, i), w = x[i + m] - x[i], in lexicographic order.  w >= 0 (or NaN in a column with an infinity, whose
//                  result is not used), so the bits of w order like w and the pair is compared as two integers: no
//                  floating-point comparison, no floating-point atomic, and the minimum is the same in whatever order pairs are
//                  combined -- lanes, then the waves of a workgroup through LDS, then the slices of a column.  Lanes stride
//                  over i and read keys[i] once for all probabilities and keys[i + m] per probability, both coalesced.
//                  A column of S <= HDI_SMALL draws is one wave's work; a longer one is cut into slices of HDI_SLICE windows
//                  (the slicing depends on S alone) with a workgroup of 256 per slice.  A column of one slice has its
//                  interval written at once; otherwise every workgroup leaves its pairs, and
//   k_hdi_window_final
//                  a wave per column combines the pairs of the slices and writes the interval.
// Everything lives in ctx->rank_ws: per column 8 P bytes of keys, the flag word, n, and 128 bytes of pairs per slice.
#include <math.h>

#include "omc_common.h"
#include "omc_quantile.h"
#include "omc_rank_sort.h"
#include "omc_store_view.h"

namespace {

constexpr int HDI_PROBS = 8;              // probabilities of a call at most
constexpr int64_t HDI_SMALL = 4096;       // columns up to this many draws: one wave
constexpr int64_t HDI_SLICE = 16384;      // windows of a slice of a longer column
constexpr int64_t HDI_NONE = 0x7fffffffffffffffLL;  // the index of "no window"

// Draw s of column (c, e) is row s rstride + c of the store seen as [N C][size]: rstride = 1, c = 0 pooled; rstride = C per chain.
// Workgroup b of the grid: draw tile b % n_st, element tile (b / n_st) % n_et, chain b / (n_st n_et).
__global__ void __launch_bounds__(256) k_hdi_gather(const double* __restrict__ store, const int64_t* __restrict__ idx, int64_t k0, int64_t Kc,
                                                    int64_t size, int64_t rstride, int64_t S, int64_t P, int64_t n_st, int64_t n_et,
                                                    uint64_t* __restrict__ keys, int32_t* __restrict__ flags) {
  const int64_t b = blockIdx.x, rest = b / n_st, c = rest / n_et;
  rank_gather_tile(store, idx, k0, Kc, size, S, P, (rest % n_et) * RANK_G_TE, (b % n_st) * RANK_G_TS, c * Kc,
                   [=](int64_t s) { return s * rstride + c; }, [](double x, int64_t, int64_t) { return x; }, 0, keys, flags);
}

// n_valid [n_col]: the keys of each sorted column that are not the all-ones key
__global__ void k_hdi_count(int64_t n_col, int64_t P, const uint64_t* __restrict__ keys, int64_t* __restrict__ n_valid) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < n_col) n_valid[q] = rank_bound(keys + q * P, P, ~0ull, false);
}

struct HdiArgs {
  const uint64_t* keys; const int32_t* flags; const int64_t* n_valid; uint64_t* part; double* out; int64_t* n_valid_out;
  int64_t k0, Kc, n_idx, CC, P, n_slices;
  int32_t n_probs, omit_nan;
  double probs[HDI_PROBS];
};

// m of the contract for n >= 1 valid draws: one fp64 product, as numpy's float64 * int
__device__ __forceinline__ int64_t hdi_m(double prob, int64_t n) {
  const int64_t m = (int64_t)floor(prob * (double)n);
  return m < n - 1 ? m : n - 1;
}

__device__ __forceinline__ void hdi_min(uint64_t& w, int64_t& i, uint64_t w2, int64_t i2) {
  if (w2 < w || (w2 == w && i2 < i)) { w = w2; i = i2; }
}

// the interval of probability p of column q from the first narrowest window i (HDI_NONE: the column has no valid draw)
__device__ __forceinline__ void hdi_emit(const HdiArgs& a, int64_t q, int p, double prob, int64_t n, int64_t i) {
  const int64_t c = q / a.Kc, e = q - c * a.Kc, at = c * a.n_idx + a.k0 + e;
  const int32_t fl = a.flags[q];
  const bool bad = (fl & 2) != 0 || (!a.omit_nan && (fl & 1) != 0) || n < 1 || i == HDI_NONE;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const uint64_t* col = a.keys + q * a.P;
  double* o = a.out + 2 * ((int64_t)p * a.CC * a.n_idx + at);
  const int64_t lo = bad ? 0 : i, hi = bad ? 0 : i + hdi_m(prob, n);  // both below n <= P
  o[0] = bad ? nan : q_val(col[lo]);
  o[1] = bad ? nan : q_val(col[hi]);
  if (p == 0 && a.n_valid_out) a.n_valid_out[at] = n;
}

// Workgroup b: slice b % n_slices (windows [slice HDI_SLICE, (slice + 1) HDI_SLICE)) of column b / n_slices; NT threads.
// n_slices == 1: the interval is written; else the pair of (column, probability, slice) goes to part [n_col][8][n_slices][2].
template <int NT>
__global__ void __launch_bounds__(NT) k_hdi_window(HdiArgs a) {
  __shared__ uint64_t sw[NT / 64][HDI_PROBS];
  __shared__ int64_t si[NT / 64][HDI_PROBS];
  const int tid = threadIdx.x;
  const int64_t q = (int64_t)blockIdx.x / a.n_slices, slice = (int64_t)blockIdx.x - q * a.n_slices;
  const uint64_t* __restrict__ col = a.keys + q * a.P;
  const int64_t n = a.n_valid[q];
  int64_t last[HDI_PROBS], m[HDI_PROBS], bi[HDI_PROBS];  // last: windows of the probability (all loops over p are unrolled)
  uint64_t bw[HDI_PROBS];
  int64_t most = 0;
#pragma unroll
  for (int p = 0; p < HDI_PROBS; ++p) {
    m[p] = (p < a.n_probs && n > 0) ? hdi_m(a.probs[p], n) : 0;
    last[p] = (p < a.n_probs) ? n - m[p] : 0;
    most = last[p] > most ? last[p] : most;
    bw[p] = ~0ull;
    bi[p] = HDI_NONE;
  }
  const int64_t end = (slice + 1) * HDI_SLICE < most ? (slice + 1) * HDI_SLICE : most;
  for (int64_t i = slice * HDI_SLICE + tid; i < end; i += NT) {
    const double x0 = q_val(col[i]);
#pragma unroll
    for (int p = 0; p < HDI_PROBS; ++p)
      if (i < last[p]) {  // i + m < n <= P; the lane's i ascend, so a tie keeps the earlier
        const uint64_t w = (uint64_t)__double_as_longlong(q_val(col[i + m[p]]) - x0);
        if (w < bw[p]) { bw[p] = w; bi[p] = i; }
      }
  }
#pragma unroll
  for (int p = 0; p < HDI_PROBS; ++p) {
    if (p < a.n_probs) {
      for (int j = 32; j >= 1; j >>= 1) {
        const uint64_t w2 = __shfl_xor((unsigned long long)bw[p], j, 64);
        const int64_t i2 = (int64_t)__shfl_xor((unsigned long long)bi[p], j, 64);
        hdi_min(bw[p], bi[p], w2, i2);
      }
      if ((tid & 63) == 0) { sw[tid >> 6][p] = bw[p]; si[tid >> 6][p] = bi[p]; }
    }
  }
  __syncthreads();
  if (tid < a.n_probs) {
    uint64_t w = sw[0][tid];
    int64_t i = si[0][tid];
    for (int v = 1; v < NT / 64; ++v) hdi_min(w, i, sw[v][tid], si[v][tid]);
    if (a.n_slices == 1) {
      double prob = 0.0;
#pragma unroll
      for (int p = 0; p < HDI_PROBS; ++p) prob = tid == p ? a.probs[p] : prob;
      hdi_emit(a, q, tid, prob, n, i);
    } else {
      uint64_t* o = a.part + 2 * ((q * HDI_PROBS + tid) * a.n_slices + slice);
      o[0] = w;
      o[1] = (uint64_t)i;
    }
  }
}

// one wave per column: the pairs of its slices combined, the interval written
__global__ void __launch_bounds__(64) k_hdi_window_final(HdiArgs a) {
  const int64_t q = blockIdx.x;
  const int64_t n = a.n_valid[q];
#pragma unroll
  for (int p = 0; p < HDI_PROBS; ++p) {
    if (p < a.n_probs) {
      const uint64_t* part = a.part + 2 * (q * HDI_PROBS + p) * a.n_slices;
      uint64_t w = ~0ull;
      int64_t i = HDI_NONE;
      for (int64_t s = threadIdx.x; s < a.n_slices; s += 64) hdi_min(w, i, part[2 * s], (int64_t)part[2 * s + 1]);
      for (int j = 32; j >= 1; j >>= 1) {
        const uint64_t w2 = __shfl_xor((unsigned long long)w, j, 64);
        const int64_t i2 = (int64_t)__shfl_xor((unsigned long long)i, j, 64);
        hdi_min(w, i, w2, i2);
      }
      if (threadIdx.x == 0) hdi_emit(a, q, p, a.probs[p], n, i);
    }
  }
}

}  // namespace

extern "C" omc_status omc_store_hdi(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx, int64_t n_idx,
                                    const double* probs, int32_t n_probs, int32_t per_chain, int32_t omit_nan, double* out,
                                    int64_t* n_valid_out) {
  if (!omc_selection_ok(ctx, n_iter, 1, size, store, idx, n_idx) || !probs || n_probs < 1 || n_probs > HDI_PROBS || !out) return OMC_INVALID_ARG;
  for (int p = 0; p < n_probs; ++p)
    if (!(probs[p] > 0.0 && probs[p] < 1.0)) return OMC_INVALID_ARG;
  const int64_t N = n_iter, C = ctx->n_chains;
  const int64_t CC = per_chain ? C : 1, S = per_chain ? N : N * C, P = rank_pow2(S);
  const int64_t n_slices = (S + HDI_SLICE - 1) / HDI_SLICE;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  // per column: keys [P], n, the pairs of every slice and probability, the flag word
  const size_t per_col = (size_t)P * sizeof(uint64_t) + sizeof(int64_t) + (n_slices > 1 ? (size_t)n_slices * HDI_PROBS * 16 : 0) + sizeof(int32_t);
  RankCarve ws(ctx, per_col * (size_t)CC, n_idx);
  const int64_t Kc = ws.Kc, n_col_max = Kc * CC;
  const int64_t n_st = (P + RANK_G_TS - 1) / RANK_G_TS, n_et_max = (Kc + RANK_G_TE - 1) / RANK_G_TE;
  if (n_st * n_et_max * CC > 0x7fffffffLL || n_col_max * n_slices > 0x7fffffffLL) return OMC_INVALID_ARG;
  uint64_t* keys = ws.take<uint64_t>((size_t)n_col_max * P);
  int64_t* n_valid = ws.take<int64_t>(n_col_max);
  uint64_t* part = ws.take<uint64_t>(n_slices > 1 ? (size_t)n_col_max * n_slices * HDI_PROBS * 2 : 0);
  int32_t* flags = ws.take<int32_t>(n_col_max);
  omc_status st = ws.done();
  if (st == OMC_OK) st = omc_store_check_index(ctx, ws.head(), idx, n_idx, size);
  if (st != OMC_OK) return st;
  hipStream_t s = ctx->stream;
  HdiArgs a;
  a.keys = keys; a.flags = flags; a.n_valid = n_valid; a.part = part; a.out = out; a.n_valid_out = n_valid_out;
  a.n_idx = n_idx; a.CC = CC; a.P = P; a.n_slices = n_slices;
  a.n_probs = n_probs; a.omit_nan = omit_nan != 0;
  for (int p = 0; p < HDI_PROBS; ++p) a.probs[p] = p < n_probs ? probs[p] : 0.0;
  for (int64_t k0 = 0; k0 < n_idx; k0 += Kc) {
    const int64_t kc = n_idx - k0 < Kc ? n_idx - k0 : Kc, n_col = kc * CC, n_et = (kc + RANK_G_TE - 1) / RANK_G_TE;
    OMC_HIP_CHECK(hipMemsetAsync(flags, 0, (size_t)n_col * sizeof(int32_t), s));
    hipLaunchKernelGGL(k_hdi_gather, dim3((unsigned)(n_st * n_et * CC)), dim3(256), 0, s, store, idx, k0, kc, size, per_chain ? C : (int64_t)1,
                       S, P, n_st, n_et, keys, flags);
    OMC_HIP_CHECK(hipGetLastError());
    st = rank_sort(ctx, keys, n_col, P);
    if (st != OMC_OK) return st;
    hipLaunchKernelGGL(k_hdi_count, dim3((unsigned)((n_col + 255) / 256)), dim3(256), 0, s, n_col, P, keys, n_valid);
    a.k0 = k0; a.Kc = kc;
    if (S <= HDI_SMALL) {
      hipLaunchKernelGGL(k_hdi_window<64>, dim3((unsigned)n_col), dim3(64), 0, s, a);
    } else {
      hipLaunchKernelGGL(k_hdi_window<256>, dim3((unsigned)(n_col * n_slices)), dim3(256), 0, s, a);
      if (n_slices > 1) hipLaunchKernelGGL(k_hdi_window_final, dim3((unsigned)n_col), dim3(64), 0, s, a);
    }
    OMC_HIP_CHECK(hipGetLastError());
  }
  return OMC_OK;
}
