// Marginal histograms, ranges and counts of the device store: one read of the store, integer results.
//
// What it replaces: np.histogram / np.nanmin / np.nanmax on MCMC.store[param] of the reference (host arrays there: mcmc.py:105-111);
// here the store stays on the device and is read where it lies: store [n_iter][C][size], seen as rows of draws through a
// StoreView (omc_store_view.h): one set of R = n_iter C rows pooled, C batches of n_iter rows per chain.
// k_hist_count: a workgroup owns a tile of TE consecutive selected elements (lanes along the elements: a wave reads 512
//   contiguous bytes of a row when TE = 64; under an index the column offset is read once per thread) and walks slices of RB
//   rows.  Every lane finds its value's bin by comparisons with the edges in LDS (hist_bin, omc_hist_layout.h) and adds one to a
//   32-bit LDS counter.  At the end the non-zero
//   counters go to the zeroed int64 output with 64-bit integer atomic adds from the vector lanes, consecutive bins on
//   consecutive lanes.  Integer addition commutes: the result does not depend on the order of arrival, nor on the form.
//   The LDS image and TE, RB come from hist_layout() (omc_hist_layout.h), on both sides.
// k_hist_minmax_part / _join: the same tiling without counters: per-lane running minimum, maximum and count of the non-NaN
//   draws, an LDS reduction over the row lanes, per-slice partials joined in slice order.
// k_hist_check: NaN or decreasing edges, and whether every row of edges is evenly spaced; two words the host reads back, with
//   the verdict of the index check (omc_store_shared.hip) in the first, before anything is written.
#include "omc_common.h"
#include "omc_hist_layout.h"
#include "omc_store_view.h"

#define HIST_MM_RB 1024     // k_hist_minmax_part: rows of a slice
#define HIST_MM_SLICES 1024  // ... and the most partials of a column
#define HIST_MM_RL (HIST_THREADS / HIST_TE_MAX)

namespace {

struct HistArgs {
  const double* data;   // the fields of the store's StoreView
  const int64_t* idx;   // [n_idx] or NULL
  const double* edges;  // [n_bins + 1] or [n_idx][n_bins + 1]
  int64_t* counts;      // [batches][n_idx][n_bins], zeroed
  int64_t* outside;     // [batches][n_idx][3], zeroed, or NULL
  int64_t row_stride, batch_stride, R, n_idx, tiles, slices;
  int n_bins;
};

// words[0] = 1: a NaN edge or a decreasing pair; words[1] = 1: some row of edges is not evenly spaced (each edge within a quarter
// of a bin of e0 + j (eN - e0) / n_bins, eN > e0 finite)
__global__ void k_hist_check(const double* __restrict__ edges, int64_t edge_rows, int n_bins, int32_t* __restrict__ words) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= edge_rows * (n_bins + 1)) return;
  const int64_t row = t / (n_bins + 1);
  const int j = (int)(t - row * (n_bins + 1));
  const double* E = edges + row * (n_bins + 1);
  const double e = E[j];
  if (e != e || (j < n_bins && E[j + 1] < e)) words[0] = 1;
  const double e0 = E[0], w = (E[n_bins] - e0) / (double)n_bins;
  if (!(w > 0.0 && w < __longlong_as_double(0x7ff0000000000000LL)) || !(fabs(e - fma((double)j, w, e0)) <= 0.25 * w)) words[1] = 1;
}

template <bool PER, bool UNIFORM>
__global__ void __launch_bounds__(HIST_THREADS) k_hist_count(HistArgs a) {
  extern __shared__ double hist_lds[];
  const int nb = a.n_bins;
  const HistLayout L = hist_layout(nb, PER ? 1 : 0);
  double* sE = hist_lds;
  uint32_t* sC = (uint32_t*)((char*)hist_lds + L.counts_off);
  uint32_t* sO = (uint32_t*)((char*)hist_lds + L.outside_off);
  const int tid = threadIdx.x, te = L.TE, e = tid & (te - 1), rl = tid / te, RL = HIST_THREADS / te;
  const int64_t batch = blockIdx.x / a.tiles, tile = blockIdx.x - batch * a.tiles;
  const int64_t j0 = tile * te, elem = j0 + e;
  const int n_el = (a.n_idx - j0 < te) ? (int)(a.n_idx - j0) : te;  // elements of this tile that exist

  if (PER) {
    const double* src = a.edges + j0 * (nb + 1);
    for (int i = tid; i < n_el * (nb + 1); i += HIST_THREADS) {
      const int el = i / (nb + 1);
      sE[el * L.ES + (i - el * (nb + 1))] = src[i];
    }
  } else {
    for (int i = tid; i <= nb; i += HIST_THREADS) sE[i] = a.edges[i];
  }
  for (int i = tid; i < te * L.CS; i += HIST_THREADS) sC[i] = 0u;
  for (int i = tid; i < te * 3; i += HIST_THREADS) sO[i] = 0u;
  __syncthreads();

  uint32_t below = 0u, above = 0u, nans = 0u;
  if (e < n_el) {
    const double* myE = PER ? sE + e * L.ES : sE;
    uint32_t* myC = sC + e * L.CS;
    const double e0 = myE[0], eN = myE[nb];
    const double scale = UNIFORM ? (double)nb / (eN - e0) : 0.0;
    const double* p = a.data + batch * a.batch_stride + (a.idx ? a.idx[elem] : elem);
    auto bin = [&](double v) {
      if (v != v) { ++nans; return; }
      if (v < e0) { ++below; return; }
      if (v > eN) { ++above; return; }
      atomicAdd(&myC[hist_bin<UNIFORM>(myE, nb, e0, scale, v)], 1u);
    };
    for (int64_t slice = blockIdx.y; slice < a.slices; slice += gridDim.y) {
      const int64_t r0 = slice * L.RB;
      const int64_t r1 = (r0 + L.RB < a.R) ? r0 + L.RB : a.R;
      for (int64_t r = r0 + rl; r < r1; r += 4 * RL) {
        double v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (r + k * RL < r1) ? p[(r + k * RL) * a.row_stride] : 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (r + k * RL < r1) bin(v[k]);
      }
    }
    if (below) atomicAdd(&sO[e * 3], below);
    if (above) atomicAdd(&sO[e * 3 + 1], above);
    if (nans) atomicAdd(&sO[e * 3 + 2], nans);
  }
  __syncthreads();

  int64_t* out = a.counts + (batch * a.n_idx + j0) * nb;
  for (int i = tid; i < n_el * nb; i += HIST_THREADS) {
    const int el = i / nb;
    const uint32_t c = sC[el * L.CS + (i - el * nb)];
    if (c) atomicAdd((unsigned long long*)(out + i), (unsigned long long)c);
  }
  if (a.outside) {
    int64_t* oo = a.outside + (batch * a.n_idx + j0) * 3;
    for (int i = tid; i < n_el * 3; i += HIST_THREADS) {
      const uint32_t c = sO[i];
      if (c) atomicAdd((unsigned long long*)(oo + i), (unsigned long long)c);
    }
  }
}

// minimum, maximum and count of the non-NaN draws of the selected columns over slices of rows.  direct: one partial per column,
// written to the outputs as they are defined (NaN, NaN, 0 without a draw); else part [3][gridDim.y][batches n_idx].
__global__ void __launch_bounds__(HIST_THREADS) k_hist_minmax_part(StoreView view, int64_t tiles, int64_t slices, int direct,
                                                                   double* __restrict__ part, double* __restrict__ min_out,
                                                                   double* __restrict__ max_out, int64_t* __restrict__ count_out) {
  const int64_t row_stride = view.row_stride, R = view.R, n_idx = view.n;
  __shared__ double smn[HIST_MM_RL][HIST_TE_MAX], smx[HIST_MM_RL][HIST_TE_MAX];
  __shared__ int64_t scn[HIST_MM_RL][HIST_TE_MAX];
  const int tid = threadIdx.x, e = tid & (HIST_TE_MAX - 1), rl = tid / HIST_TE_MAX;
  const int64_t batch = blockIdx.x / tiles, tile = blockIdx.x - batch * tiles, batches = gridDim.x / tiles;
  const int64_t elem = tile * HIST_TE_MAX + e;
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  double mn = inf, mx = -inf;
  int64_t cnt = 0;
  if (elem < n_idx) {
    const double* p = view.column(batch, elem);
    for (int64_t slice = blockIdx.y; slice < slices; slice += gridDim.y) {
      const int64_t r0 = slice * HIST_MM_RB;
      const int64_t r1 = (r0 + HIST_MM_RB < R) ? r0 + HIST_MM_RB : R;
      for (int64_t r = r0 + rl; r < r1; r += 4 * HIST_MM_RL) {
        double v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (r + k * HIST_MM_RL < r1) ? p[(r + k * HIST_MM_RL) * row_stride] : mn;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (r + k * HIST_MM_RL < r1 && v[k] == v[k]) {
            mn = v[k] < mn ? v[k] : mn;
            mx = v[k] > mx ? v[k] : mx;
            ++cnt;
          }
      }
    }
  }
  smn[rl][e] = mn; smx[rl][e] = mx; scn[rl][e] = cnt;
  __syncthreads();
  if (rl == 0 && elem < n_idx) {
    for (int q = 1; q < HIST_MM_RL; ++q) {
      mn = smn[q][e] < mn ? smn[q][e] : mn;
      mx = smx[q][e] > mx ? smx[q][e] : mx;
      cnt += scn[q][e];
    }
    const int64_t o = batch * n_idx + elem, cols = batches * n_idx;
    if (direct) {
      const double nan = __longlong_as_double(0x7ff8000000000000LL);
      if (min_out) min_out[o] = cnt ? mn : nan;
      if (max_out) max_out[o] = cnt ? mx : nan;
      if (count_out) count_out[o] = cnt;
    } else {
      part[(int64_t)blockIdx.y * cols + o] = mn;
      part[((int64_t)gridDim.y + blockIdx.y) * cols + o] = mx;
      ((int64_t*)part)[(2 * (int64_t)gridDim.y + blockIdx.y) * cols + o] = cnt;
    }
  }
}
__global__ void k_hist_minmax_join(int64_t cols, int parts, const double* __restrict__ part, double* __restrict__ min_out,
                                   double* __restrict__ max_out, int64_t* __restrict__ count_out) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= cols) return;
  const double inf = __longlong_as_double(0x7ff0000000000000LL), nan = __longlong_as_double(0x7ff8000000000000LL);
  double mn = inf, mx = -inf;
  int64_t cnt = 0;
  for (int s = 0; s < parts; ++s) {
    const double a = part[(int64_t)s * cols + o], b = part[((int64_t)parts + s) * cols + o];
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
    cnt += ((const int64_t*)part)[(2 * (int64_t)parts + s) * cols + o];
  }
  if (min_out) min_out[o] = cnt ? mn : nan;
  if (max_out) max_out[o] = cnt ? mx : nan;
  if (count_out) count_out[o] = cnt;
}

}  // namespace

// the index check and k_hist_check on the same two words, read back once: the launches behind it write nothing before the host has
// seen them (also omc_hist2d.hip)
omc_status omc_hist_check(omc_ctx* ctx, const int64_t* idx, int64_t n_idx, int64_t size, const double* edges, int64_t edge_rows, int n_bins,
                          int32_t got[2]) {
  omc_status st = omc_ensure(ctx, ctx->store_ws, 64);
  if (st != OMC_OK) return st;
  int32_t* words = (int32_t*)ctx->store_ws.p;
  st = omc_words_zero(ctx, words, 2);
  if (st != OMC_OK) return st;
  omc_store_check_index_launch(ctx, idx, n_idx, size, nullptr, 0, 0, words);
  const int64_t n = edge_rows * (n_bins + 1);
  hipLaunchKernelGGL(k_hist_check, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, edges, edge_rows, n_bins, words);
  return omc_words_read(ctx, words, 2, got);
}

extern "C" omc_status omc_store_histogram_layout(int32_t n_bins, int32_t edges_per_element, int32_t* out) {
  if (n_bins < 1 || n_bins > HIST_MAX_BINS || !out) return OMC_INVALID_ARG;
  const HistLayout l = hist_layout(n_bins, edges_per_element != 0);
  const int32_t v[10] = {l.TE, l.RB, l.ES, l.CS, l.edges_off, l.counts_off, l.outside_off, l.end, HIST_LDS_BUDGET, HIST_THREADS};
  for (int i = 0; i < 10; ++i) out[i] = v[i];
  return OMC_OK;
}

extern "C" omc_status omc_store_minmax(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx, int64_t n_idx,
                                       int32_t pooled, double* min_out, double* max_out, int64_t* count_out) {
  if (!omc_selection_ok(ctx, n_iter, 1, size, store, idx, n_idx)) return OMC_INVALID_ARG;
  const StoreView v = omc_store_view(ctx, n_iter, size, pooled != 0, store, idx, n_idx);
  const int64_t R = v.R, batches = v.batches;
  const int64_t tiles = (n_idx + HIST_TE_MAX - 1) / HIST_TE_MAX;
  if (tiles * batches > 0x7fffffffLL) return OMC_INVALID_ARG;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  omc_status st = omc_store_check_index(ctx, nullptr, idx, n_idx, size);
  if (st != OMC_OK) return st;
  const int64_t slices = (R + HIST_MM_RB - 1) / HIST_MM_RB;
  // enough workgroups for the CUs, one partial per column where the tiles alone fill them (the per-chain form of a long store)
  int64_t parts = (8 * (int64_t)ctx->dev_cus + tiles * batches - 1) / (tiles * batches);
  if (parts > slices) parts = slices;
  if (parts > HIST_MM_SLICES) parts = HIST_MM_SLICES;
  const int64_t cols = batches * n_idx;
  double* part = nullptr;
  if (parts > 1) {
    st = omc_ensure(ctx, ctx->store_ws, (size_t)3 * parts * cols * sizeof(double));
    if (st != OMC_OK) return st;
    part = (double*)ctx->store_ws.p;
  }
  hipLaunchKernelGGL(k_hist_minmax_part, dim3((unsigned)(tiles * batches), (unsigned)parts), dim3(HIST_THREADS), 0, ctx->stream, v, tiles, slices,
                     (int)(parts == 1), part, min_out, max_out, count_out);
  if (parts > 1)
    hipLaunchKernelGGL(k_hist_minmax_join, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, ctx->stream, cols, (int)parts, part, min_out,
                       max_out, count_out);
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}

extern "C" omc_status omc_store_histogram(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx,
                                          int64_t n_idx, int32_t pooled, int32_t n_bins, const double* edges, int32_t edges_per_element,
                                          int64_t* counts_out, int64_t* outside_out) {
  if (!omc_selection_ok(ctx, n_iter, 1, size, store, idx, n_idx) || n_bins < 1 || n_bins > HIST_MAX_BINS || !edges || !counts_out)
    return OMC_INVALID_ARG;
  const StoreView v = omc_store_view(ctx, n_iter, size, pooled != 0, store, idx, n_idx);
  const int64_t R = v.R, batches = v.batches;
  if (R >= (1LL << 32)) return OMC_UNSUPPORTED;  // a workgroup's 32-bit counters see at most R rows
  const bool per = edges_per_element != 0;
  const HistLayout L = hist_layout(n_bins, per);
  if (L.end > HIST_LDS_BUDGET || L.TE < 1) return OMC_UNSUPPORTED;  // (cannot happen: static_assert of omc_hist_layout.h)
  const int64_t tiles = (n_idx + L.TE - 1) / L.TE;
  if (tiles * batches > 0x7fffffffLL) return OMC_INVALID_ARG;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  int32_t got[2];
  omc_status st = omc_hist_check(ctx, idx, n_idx, size, edges, per ? n_idx : 1, n_bins, got);
  if (st != OMC_OK) return st;
  if (got[0]) return OMC_INVALID_ARG;
  OMC_HIP_CHECK(hipMemsetAsync(counts_out, 0, (size_t)batches * n_idx * n_bins * sizeof(int64_t), s));
  if (outside_out) OMC_HIP_CHECK(hipMemsetAsync(outside_out, 0, (size_t)batches * n_idx * 3 * sizeof(int64_t), s));
  HistArgs a;
  a.data = v.data; a.idx = v.idx; a.edges = edges; a.counts = counts_out; a.outside = outside_out;
  a.row_stride = v.row_stride; a.batch_stride = v.batch_stride; a.R = R; a.n_idx = v.n; a.tiles = tiles; a.slices = (R + L.RB - 1) / L.RB; a.n_bins = n_bins;
  const bool uniform = got[1] == 0 && ctx->hist_algo != 1;
  const dim3 grid((unsigned)(tiles * batches), (unsigned)(a.slices < 65535 ? a.slices : 65535));
  const size_t lds = (size_t)L.end;
  if (per) {
    if (uniform) hipLaunchKernelGGL((k_hist_count<true, true>), grid, dim3(HIST_THREADS), lds, s, a);
    else hipLaunchKernelGGL((k_hist_count<true, false>), grid, dim3(HIST_THREADS), lds, s, a);
  } else {
    if (uniform) hipLaunchKernelGGL((k_hist_count<false, true>), grid, dim3(HIST_THREADS), lds, s, a);
    else hipLaunchKernelGGL((k_hist_count<false, false>), grid, dim3(HIST_THREADS), lds, s, a);
  }
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}
