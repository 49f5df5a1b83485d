// The sort of the store summaries that need every order statistic of a column (omc_rank.hip: ranks and the rank-normalised
// diagnostics; omc_hdi.hip: highest-density intervals), with what goes with it: the key of a draw, the launch list, the index
// check, the chunk that fits the workspace and the bisection in a sorted column.  Included by both translation units; each gets
// its own copy of the two kernels under the same names.
//
//   k_rank_sort_tile / k_rank_sort_global
//                  a bitonic network over every column, keys only.  Its addressing depends on P and the tile T alone, never on
//                  the data.  Stage k (k = 2, 4, .. P) compare-exchanges at strides j = k / 2 .. 1, ascending where the
//                  position within the column has bit k clear.  Strides inside a tile of T keys run in LDS, one workgroup per
//                  tile: the first launch sorts every tile (all stages up to T), and each later stage ends in one launch that
//                  does its strides T / 2 .. 1; strides of 64 and more go through LDS with a barrier per stride, the last six
//                  (32 .. 1) stay inside a wave, a key per lane exchanged by __shfl_xor.  Every stride >= T is one pass over
//                  global memory.  rank_schedule() lists the launches; the entry points walk that list and
//                  omc_store_rank_schedule hands it to the tests, which replay it in numpy.
//
// Kc: what fits RANK_BUDGET = 1 GiB (a choice, not a measurement: large enough for a few hundred elements of a store with a
// million pooled draws, small beside the store) at the caller's bytes per element, at least 1; option "rank_chunk" forces it.
#pragma once
#include <vector>

#include "omc_common.h"
#include "omc_quantile.h"

namespace {

constexpr size_t RANK_BUDGET = (size_t)1 << 30;
constexpr int64_t RANK_KC_MAX = (int64_t)1 << 17;  // elements of a chunk at most (grid.y of k_rank_emit: Kc / 4)
constexpr int RANK_TILE_DEFAULT = 8192;            // keys of an LDS tile: 64 KiB

struct RankLaunch { int64_t kind, k, j; };  // kind 0: sort every tile (stages 2 .. k); 1: global pass (k, j); 2: tile strides j .. 1 of stage k

int64_t rank_pow2(int64_t S) {
  int64_t P = 1;
  while (P < S) P <<= 1;
  return P;
}

// the launches that sort columns of P keys with tiles of T (both powers of two)
std::vector<RankLaunch> rank_schedule(int64_t P, int64_t T) {
  std::vector<RankLaunch> L;
  if (P < 2) return L;
  if (T > P) T = P;
  L.push_back({0, T, T / 2});
  for (int64_t k = 2 * T; k <= P; k <<= 1) {
    for (int64_t j = k / 2; j >= T; j >>= 1) L.push_back({1, k, j});
    L.push_back({2, k, T / 2});
  }
  return L;
}

__device__ __forceinline__ uint64_t rank_key(double v) {
  if (v == 0.0) v = 0.0;  // -0.0 and +0.0 are one value
  return q_key(v);
}

// words[0] = 1: an index outside [0, size)
__global__ void k_rank_check(const int64_t* __restrict__ idx, int64_t n_idx, int64_t size, int32_t* __restrict__ words) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n_idx && (idx[t] < 0 || idx[t] >= size)) words[0] = 1;
}

// compare-exchange at stride j <= 32 of stage k inside a wave: lane l holds the key at position pos (pos & 63 == l)
__device__ __forceinline__ uint64_t rank_wave_step(uint64_t v, int64_t pos, int j, int64_t k) {
  const uint64_t o = __shfl_xor((unsigned long long)v, j, 64);
  const bool up = (pos & k) == 0, low = (pos & j) == 0;
  const uint64_t mn = v < o ? v : o, mx = v < o ? o : v;
  return low == up ? mn : mx;
}

// strides jtop .. 1 of stage k on the tile in LDS; c0 = the tile's first position within its column
__device__ __forceinline__ void rank_tile_stage(uint64_t* __restrict__ t, int T, int64_t c0, int64_t k, int jtop) {
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int j = jtop; j >= 64; j >>= 1) {
    for (int p = tid; p < T / 2; p += nt) {
      const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), i2 = i | j;
      const uint64_t a = t[i], b = t[i2];
      if ((a > b) == (((c0 + i) & k) == 0)) { t[i] = b; t[i2] = a; }
    }
    __syncthreads();
  }
  const int Tr = T < 64 ? 64 : T;
  for (int base = tid; base < Tr; base += nt) {  // (T < 64 or a multiple of 64, nt a multiple of 64: whole waves take a step)
    uint64_t v = base < T ? t[base] : ~0ull;
    for (int j = jtop < 32 ? jtop : 32; j >= 1; j >>= 1) v = rank_wave_step(v, c0 + base, j, k);
    if (base < T) t[base] = v;
  }
  __syncthreads();
}

// One workgroup per tile of T keys (T <= P, both powers of two; tiles of all columns lie one behind the other).
// whole != 0: stages 2 .. T (the tile comes out sorted, ascending where its position has bit T clear -- bit P is never set);
// whole == 0: strides T / 2 .. 1 of stage k.
__global__ void __launch_bounds__(1024) k_rank_sort_tile(uint64_t* __restrict__ keys, int T, int64_t P, int64_t k, int whole) {
  extern __shared__ uint64_t rank_lds[];
  uint64_t* g = keys + (int64_t)blockIdx.x * T;
  const int64_t c0 = ((int64_t)blockIdx.x * T) & (P - 1);
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int i = tid; i < T; i += nt) rank_lds[i] = g[i];
  __syncthreads();
  if (whole) {
    // stages up to 64 never leave the wave
    const int Tr = T < 64 ? 64 : T, kw = T < 64 ? T : 64;
    for (int base = tid; base < Tr; base += nt) {
      uint64_t v = base < T ? rank_lds[base] : ~0ull;
      for (int kk = 2; kk <= kw; kk <<= 1)
        for (int j = kk >> 1; j >= 1; j >>= 1) v = rank_wave_step(v, c0 + base, j, kk);
      if (base < T) rank_lds[base] = v;
    }
    __syncthreads();
    for (int kk = 128; kk <= T; kk <<= 1) rank_tile_stage(rank_lds, T, c0, kk, kk >> 1);
  } else {
    rank_tile_stage(rank_lds, T, c0, k, T >> 1);
  }
  for (int i = tid; i < T; i += nt) g[i] = rank_lds[i];
}

// stride j >= T of stage k over all columns: one thread per pair, n_pairs = Kc P / 2
__global__ void __launch_bounds__(256) k_rank_sort_global(uint64_t* __restrict__ keys, int64_t n_pairs, int64_t P, int64_t k, int64_t j) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n_pairs) return;
  const int64_t i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), i2 = i | j;  // j < P: both in the same column, i2 < 2 n_pairs
  const uint64_t a = keys[i], b = keys[i2];
  if ((a > b) == (((i & (P - 1)) & k) == 0)) { keys[i] = b; keys[i2] = a; }
}

// keys of a sorted column (P of them, a power of two) that are < key (upper == false) or <= key (upper == true): every read is at
// an index below P whatever the keys hold
__device__ __forceinline__ int64_t rank_bound(const uint64_t* __restrict__ col, int64_t P, uint64_t key, bool upper) {
  int64_t lo = 0;
  for (int64_t step = P >> 1; step >= 1; step >>= 1) {
    const uint64_t c = col[lo + step - 1];
    if (upper ? c <= key : c < key) lo += step;
  }
  const uint64_t c = col[lo];
  return lo + ((upper ? c <= key : c < key) ? 1 : 0);
}

int64_t rank_tile_of(const omc_ctx* ctx, int64_t P) {
  const int64_t T = ctx->rank_tile ? ctx->rank_tile : RANK_TILE_DEFAULT;
  return T < P ? T : P;
}

// sorts the Kc columns of P keys
omc_status rank_sort(omc_ctx* ctx, uint64_t* keys, int64_t Kc, int64_t P) {
  const int64_t T = rank_tile_of(ctx, P);
  const int64_t blocks = Kc * P / T, n_pairs = Kc * P / 2;
  if (blocks > 0x7fffffffLL || (n_pairs + 255) / 256 > 0x7fffffffLL) return OMC_INVALID_ARG;
  const size_t lds = (size_t)T * sizeof(uint64_t);
  static bool lds_raised[64];  // per device: the tile kernel may take more than the default 48 KiB of dynamic LDS (asked for once)
  if (lds > 48 * 1024 && !(ctx->device >= 0 && ctx->device < 64 && lds_raised[ctx->device])) {
    OMC_HIP_CHECK(hipFuncSetAttribute((const void*)k_rank_sort_tile, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      RANK_TILE_DEFAULT * (int)sizeof(uint64_t)));
    if (ctx->device >= 0 && ctx->device < 64) lds_raised[ctx->device] = true;
  }
  int64_t nt = T / 8;  // eight keys per thread, whole waves
  if (nt < 64) nt = 64;
  if (nt > 1024) nt = 1024;
  for (const RankLaunch& l : rank_schedule(P, T)) {
    if (l.kind == 1)
      hipLaunchKernelGGL(k_rank_sort_global, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, ctx->stream, keys, n_pairs, P, l.k, l.j);
    else
      hipLaunchKernelGGL(k_rank_sort_tile, dim3((unsigned)blocks), dim3((unsigned)nt), lds, ctx->stream, keys, (int)T, P, l.k,
                         (int)(l.kind == 0));
  }
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}

// index check on the device, one word read back before anything is written; words = the head of the workspace
omc_status rank_check(omc_ctx* ctx, const int64_t* idx, int64_t n_idx, int64_t size, int32_t* words) {
  if (!idx) return OMC_OK;
  OMC_HIP_CHECK(hipMemsetAsync(words, 0, sizeof(int32_t), ctx->stream));
  hipLaunchKernelGGL(k_rank_check, dim3((unsigned)((n_idx + 255) / 256)), dim3(256), 0, ctx->stream, idx, n_idx, size, words);
  OMC_HIP_CHECK(hipGetLastError());
  int32_t got = 0;
  OMC_HIP_CHECK(hipMemcpyAsync(&got, words, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  OMC_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return got ? OMC_INVALID_ARG : OMC_OK;
}

int64_t rank_chunk(const omc_ctx* ctx, size_t per_elem, int64_t n_idx) {
  int64_t Kc = ctx->rank_chunk > 0 ? ctx->rank_chunk : (int64_t)(RANK_BUDGET / per_elem);
  if (Kc < 1) Kc = 1;
  if (Kc > RANK_KC_MAX) Kc = RANK_KC_MAX;
  return Kc < n_idx ? Kc : n_idx;
}

constexpr size_t RANK_HEAD = 64;  // bytes in front of the per-element arrays: the word of rank_check

}  // namespace
