// What the summaries of the device store share, compiled once: the check of a selection, the column moments and the sort of
// columns of keys.  The declarations, and how a summary sees the store, are in omc_store_view.h and omc_rank_sort.h.
//
//   k_store_check_index   sets a word if an entry of one or two selections lies outside its store's row; the host reads the word
//                         back before anything reads through the selection.
//   k_store_moments_part / _join
//                         mean and unbiased variance of the view's columns (omc_store_moments; the means and variances of
//                         omc_store_cov): a workgroup owns 16 adjacent selected columns of a batch and a slice of the rows,
//                         16 row lanes each running Welford's update; the lanes are combined 1 .. 15 in order by Chan's
//                         update, and the slices, through a [slices][batches][3][n] scratch, in slice order.  Deterministic:
//                         slice boundaries and combination order are functions of the shape alone.  Two instantiations of
//                         the one source, with and without an index: with the index a run-time branch the pass was up to 2 %
//                         slower than the two kernels it replaces (profiles/store_refactor_ab.txt).
//   k_rank_gather         the draws of a chunk of selected elements, whole or split in halves, as columns of keys (the gather tile of
//                         omc_rank_sort.h; rank_gather_sort: omc_rank.hip, omc_essq.hip).
//   k_rank_sort_tile / k_rank_sort_global
//                         the key-only bitonic sort of every summary that needs order statistics (described in omc_rank_sort.h).
#include "omc_moments.h"
#include "omc_rank_sort.h"
#include "omc_store_view.h"

namespace {

constexpr int M_COLS = 16, M_ROWS = 16;  // k_store_moments_part: columns and row lanes of a workgroup

__global__ void k_store_check_index(const int64_t* __restrict__ idx_a, int64_t n_a, int64_t size_a, const int64_t* __restrict__ idx_b,
                                    int64_t n_b, int64_t size_b, int32_t* __restrict__ word) {
  int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t* idx = idx_a;
  int64_t size = size_a;
  if (j >= n_a) {
    j -= n_a; idx = idx_b; size = size_b;
    if (j >= n_b) return;
  }
  if (idx[j] < 0 || idx[j] >= size) *word = 1;
}

// part [slices][batches][3][n] (count, mean, m2); workgroup x = (batch, tile of M_COLS columns), y = slice of rows_per_block rows
template <bool IDX>
__global__ void __launch_bounds__(256) k_store_moments_part(StoreView v, int64_t tiles, int64_t rows_per_block, double* __restrict__ part) {
  __shared__ double sm[3][M_ROWS][M_COLS];
  const int tid = threadIdx.x, col = tid & (M_COLS - 1), rr = tid >> 4;
  const int64_t batch = IDX ? blockIdx.x / tiles : 0, tile = blockIdx.x - batch * tiles;  // (no index: one batch, omc_col_moments)
  const int64_t j = tile * M_COLS + col;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
  const int64_t r1 = (r0 + rows_per_block < v.R) ? r0 + rows_per_block : v.R;
  double cnt = 0.0, mean = 0.0, m2 = 0.0;
  if (j < v.n) {
    if (IDX) {
      const double* p = v.data + batch * v.batch_stride + v.idx[j];
      for (int64_t r = r0 + rr; r < r1; r += M_ROWS) omc_welford(cnt, mean, m2, p[r * v.row_stride]);
    } else {
      for (int64_t r = r0 + rr; r < r1; r += M_ROWS) omc_welford(cnt, mean, m2, v.data[r * v.row_stride + j]);
    }
    if (mean != mean) {  // a non-finite value among the lane's: the mean of their plain sum, +-inf or NaN (omc_moments.h)
      const double* p = v.data + (IDX ? batch * v.batch_stride + v.idx[j] : j);
      double sum = 0.0;
      for (int64_t r = r0 + rr; r < r1; r += M_ROWS) sum += p[r * v.row_stride];
      mean = sum / cnt;
    }
  }
  sm[0][rr][col] = cnt; sm[1][rr][col] = mean; sm[2][rr][col] = m2;
  __syncthreads();
  if (rr == 0 && j < v.n) {
    for (int q = 1; q < M_ROWS; ++q) omc_chan(cnt, mean, m2, sm[0][q][col], sm[1][q][col], sm[2][q][col]);
    double* o = part + ((int64_t)blockIdx.y * v.batches + batch) * 3 * v.n;
    o[j] = cnt; o[v.n + j] = mean; o[2 * v.n + j] = m2;
  }
}
// thread x: column j; the batches walk grid y (no division: with every column in one batch this is a kernel of K threads)
__global__ void k_store_moments_join(int64_t batches, int64_t n, int slices, const double* __restrict__ part, double* __restrict__ mean_out,
                                     double* __restrict__ var_out) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  for (int64_t batch = blockIdx.y; batch < batches; batch += gridDim.y) {
    double cnt = 0.0, mean = 0.0, m2 = 0.0;
    for (int s = 0; s < slices; ++s) {
      const double* o = part + ((int64_t)s * batches + batch) * 3 * n;
      omc_chan(cnt, mean, m2, o[j], o[n + j], o[2 * n + j]);
    }
    if (mean_out) mean_out[batch * n + j] = mean;
    if (var_out) var_out[batch * n + j] = cnt > 1.0 ? m2 / (cnt - 1.0) : 0.0;
  }
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

// the gather tile of omc_rank_sort.h over the draws of RankGeom; stats (or NULL): fold the draws, |x - stats[3 e]|
__global__ void __launch_bounds__(256) k_rank_gather(const double* __restrict__ store, const int64_t* __restrict__ idx, int64_t k0, int64_t Kc,
                                                     int64_t size, int64_t C, int64_t S, int64_t P, int64_t first, int64_t skip,
                                                     int64_t mid_row0, const double* __restrict__ stats, uint64_t* __restrict__ keys,
                                                     int32_t* __restrict__ flags) {
  const int64_t e0 = (int64_t)blockIdx.y * RANK_G_TE, e = e0 + (threadIdx.x & (RANK_G_TE - 1));
  const bool fold = stats != nullptr;
  const double med = (fold && e < Kc) ? stats[3 * e] : 0.0;
  int32_t bits = 0;
  if (mid_row0 >= 0 && blockIdx.x == 0 && e < Kc) {
    const int64_t col = idx ? idx[k0 + e] : k0 + e;
    for (int64_t c = threadIdx.x / RANK_G_TE; c < C; c += 256 / RANK_G_TE) bits |= rank_flag_bits(store[(mid_row0 + c) * size + col]);
  }
  rank_gather_tile(store, idx, k0, Kc, size, S, P, e0, (int64_t)blockIdx.x * RANK_G_TS, 0,
                   [=](int64_t s) { return s < first ? s : s + skip; }, [=](double x, int64_t, int64_t) { return fold ? fabs(x - med) : x; }, bits, keys, flags);
}

}  // namespace

void omc_store_check_index_launch(omc_ctx* ctx, const int64_t* idx_a, int64_t n_a, int64_t size_a, const int64_t* idx_b, int64_t n_b,
                                  int64_t size_b, int32_t* word) {
  if (!idx_a) n_a = 0;
  if (!idx_b) n_b = 0;
  if (n_a + n_b < 1) return;
  hipLaunchKernelGGL(k_store_check_index, dim3((unsigned)((n_a + n_b + 255) / 256)), dim3(256), 0, ctx->stream, idx_a, n_a, size_a, idx_b,
                     n_b, size_b, word);
}

omc_status omc_store_check_index(omc_ctx* ctx, int32_t* word, const int64_t* idx_a, int64_t n_a, int64_t size_a, const int64_t* idx_b,
                                 int64_t n_b, int64_t size_b) {
  if (!idx_a && !idx_b) return OMC_OK;
  if (!word) {
    omc_status st = omc_ensure(ctx, ctx->store_ws, 64);
    if (st != OMC_OK) return st;
    word = (int32_t*)ctx->store_ws.p;
  }
  omc_status st = omc_words_zero(ctx, word, 1);
  if (st != OMC_OK) return st;
  omc_store_check_index_launch(ctx, idx_a, n_a, size_a, idx_b, n_b, size_b, word);
  int32_t got = 0;
  st = omc_words_read(ctx, word, 1, &got);
  if (st != OMC_OK) return st;
  return got ? OMC_INVALID_ARG : OMC_OK;
}

omc_status omc_col_moments(omc_ctx* ctx, const StoreView& view, double* mean_out, double* var_out) {
  StoreView v = view;
  if (!v.idx) {  // every column takes part: the batches are adjacent columns of one matrix, tiled without regard to their borders
    v.n *= v.batches; v.batches = 1; v.batch_stride = 0;
  }
  const int64_t tiles = (v.n + M_COLS - 1) / M_COLS, groups = tiles * v.batches;
  int64_t rpb;
  const int64_t slices = omc_row_slices(groups, v.R, &rpb);
  omc_status st = omc_ensure(ctx, ctx->store_ws, (size_t)slices * v.batches * 3 * v.n * sizeof(double));
  if (st != OMC_OK) return st;
  double* part = (double*)ctx->store_ws.p;
  const dim3 grid((unsigned)groups, (unsigned)slices);
  if (v.idx) hipLaunchKernelGGL(k_store_moments_part<true>, grid, dim3(256), 0, ctx->stream, v, tiles, rpb, part);
  else hipLaunchKernelGGL(k_store_moments_part<false>, grid, dim3(256), 0, ctx->stream, v, tiles, rpb, part);
  hipLaunchKernelGGL(k_store_moments_join, dim3((unsigned)((v.n + 255) / 256), (unsigned)(v.batches < 65535 ? v.batches : 65535)), dim3(256), 0,
                     ctx->stream, v.batches, v.n, (int)slices, part, mean_out, var_out);
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}

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

omc_status rank_sort(omc_ctx* ctx, uint64_t* keys, int64_t Kc, int64_t P) {
  int64_t T = ctx->rank_tile ? ctx->rank_tile : RANK_TILE_DEFAULT;
  if (T > P) T = P;
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

omc_status rank_gather_sort(omc_ctx* ctx, const double* store, const int64_t* idx, int64_t k0, int64_t kc, int64_t size, const RankGeom& g,
                            const double* stats, uint64_t* keys, int32_t* flags) {
  if (flags) OMC_HIP_CHECK(hipMemsetAsync(flags, 0, (size_t)kc * sizeof(int32_t), ctx->stream));
  const dim3 grid((unsigned)((g.P + RANK_G_TS - 1) / RANK_G_TS), (unsigned)((kc + RANK_G_TE - 1) / RANK_G_TE));
  hipLaunchKernelGGL(k_rank_gather, grid, dim3(256), 0, ctx->stream, store, idx, k0, kc, size, ctx->n_chains, g.S, g.P, g.first, g.skip,
                     g.mid_row0, stats, keys, flags);
  OMC_HIP_CHECK(hipGetLastError());
  return rank_sort(ctx, keys, kc, g.P);
}

int64_t rank_chunk(const omc_ctx* ctx, size_t per_elem, int64_t n_idx) {
  int64_t Kc = ctx->rank_chunk > 0 ? ctx->rank_chunk : (int64_t)(RANK_BUDGET / per_elem);
  if (Kc < 1) Kc = 1;
  if (Kc > RANK_KC_MAX) Kc = RANK_KC_MAX;
  return Kc < n_idx ? Kc : n_idx;
}
