// Joint 2-D histograms and occupancy maps of the device store: one read of the selected columns, integer results.
//
// What it replaces: np.histogram2d on two rows of MCMC.store[param] of the reference (host arrays there: mcmc.py:105-111), and,
// for the NaN-padded vectors a reversible-jump run leaves, the loop over stored states of np.histogramdd(...) > 0; here the
// stores stay on the device and are read where they lie, with the layout conventions of omc_hist.hip: store [n_iter][C][size],
// pooled = one set of R = n_iter C rows, per chain = C batches of n_iter rows.  Pair k = (element idx_x[k] of store_x, element
// idx_y[k] of store_y) of the same row.
// k_hist2d_pair (a grid per pair): the tiling of k_hist_count with nx ny counters per pair -- a workgroup owns TE consecutive
//   pairs (lanes along the pairs: a wave reads contiguous runs of a row of either store) and walks slices of RB rows.
// k_hist2d_pool (one grid for all pairs, the map of a ragged parameter): a workgroup owns the grid and walks slices of RB rows,
//   the lanes of a wave along the pairs of a row -- 64 >> s rows of 1 << s lanes at a time when a row has at most 32 pairs, four
//   such passes in flight.  With occupancy every lane keeps the cells its (up to four) pairs fell into, keyed by (row of the
//   pass, cell); the wave then takes the first remaining key with a ballot, its owner adds one to the cell's second counter, and
//   every slot holding that key retires: a cell is counted once per row whatever the order.
// Per axis the bin rule is k_hist_count's: hist_bin (omc_hist_layout.h).
// Two forms of either kernel: 32-bit counters in LDS, the non-zero ones added to the zeroed int64 output at the end with 64-bit
// integer atomic adds from the vector lanes (consecutive cells on consecutive lanes); or, for grids beyond the LDS budget and
// for row counts a 32-bit counter could not hold, those atomic adds straight from the counting loop (DIRECT).  Integer addition
// commutes: the result depends neither on the order of arrival nor on the form.  The LDS images and TE, RB come from
// hist2d_layout_form() (omc_hist2d_layout.h), on both sides.  Validation is omc_hist.hip's omc_hist_check, once per axis.
#include "omc_common.h"
#include "omc_hist2d_layout.h"
#include "omc_store_view.h"

namespace {

struct Hist2dArgs {
  StoreView x, y;                  // the two stores (may be the same): the same R rows, n = n_pairs selected elements of each
  const double *ex, *ey;           // [nx + 1], [ny + 1] or [n_pairs][..]
  unsigned long long* counts;      // [batches][n_pairs][nx][ny] or [batches][nx][ny], zeroed
  unsigned long long* outside;     // [..][2], zeroed, or NULL
  unsigned long long* occupied;    // [batches][nx][ny], zeroed, or NULL
  int64_t tiles, slices;
  int nx, ny;
  int pair_shift;   // k_hist2d_pool: a row takes 1 << pair_shift lanes of a wave (6: the whole wave)
  int chunk_shift;  // ... and 1 << chunk_shift of the four slots of a lane (rows of more than 64 pairs)
};

struct Hist2dAxis {
  const double* E;
  int nb;
  double e0, eN, scale;
};
template <bool UNIFORM>
__device__ __forceinline__ Hist2dAxis hist2d_axis(const double* E, int nb) {
  Hist2dAxis a;
  a.E = E; a.nb = nb; a.e0 = E[0]; a.eN = E[nb];
  a.scale = UNIFORM ? (double)nb / (a.eN - a.e0) : 0.0;
  return a;
}
// the axis' bin of v (not NaN), -1 outside [E[0], E[nb]]
template <bool UNIFORM>
__device__ __forceinline__ int hist2d_bin(const Hist2dAxis& a, double v) {
  return (v < a.e0 || v > a.eN) ? -1 : hist_bin<UNIFORM>(a.E, a.nb, a.e0, a.scale, v);
}

template <bool PER, bool UNIFORM, bool DIRECT>
__global__ void __launch_bounds__(HIST_THREADS) k_hist2d_pair(Hist2dArgs a) {
  extern __shared__ double hist2d_lds[];
  const int nx = a.nx, ny = a.ny, cells = nx * ny;
  const Hist2dLayout L = hist2d_layout_form(nx, ny, PER ? 1 : 0, HIST2D_PER_PAIR, DIRECT ? 1 : 0);
  double* sEx = hist2d_lds;
  double* sEy = (double*)((char*)hist2d_lds + L.ey_off);
  uint32_t* sC = (uint32_t*)((char*)hist2d_lds + L.counts_off);
  unsigned long long* sO = (unsigned long long*)((char*)hist2d_lds + L.outside_off);
  const int tid = threadIdx.x, te = L.TE, e = tid & (te - 1), rl = tid / te, RL = HIST_THREADS / te;
  const int64_t batch = blockIdx.x / a.tiles, tile = blockIdx.x - batch * a.tiles;
  const int64_t j0 = tile * te, pair = j0 + e;
  const int n_el = (a.x.n - j0 < te) ? (int)(a.x.n - j0) : te;  // pairs of this tile that exist

  if (PER) {
    const double* srcx = a.ex + j0 * (nx + 1);
    for (int i = tid; i < n_el * (nx + 1); i += HIST_THREADS) {
      const int el = i / (nx + 1);
      sEx[el * L.EXS + (i - el * (nx + 1))] = srcx[i];
    }
    const double* srcy = a.ey + j0 * (ny + 1);
    for (int i = tid; i < n_el * (ny + 1); i += HIST_THREADS) {
      const int el = i / (ny + 1);
      sEy[el * L.EYS + (i - el * (ny + 1))] = srcy[i];
    }
  } else {
    for (int i = tid; i <= nx; i += HIST_THREADS) sEx[i] = a.ex[i];
    for (int i = tid; i <= ny; i += HIST_THREADS) sEy[i] = a.ey[i];
  }
  if (!DIRECT)
    for (int i = tid; i < te * L.CS; i += HIST_THREADS) sC[i] = 0u;
  for (int i = tid; i < te * 2; i += HIST_THREADS) sO[i] = 0ull;
  __syncthreads();

  if (e < n_el) {
    const Hist2dAxis ax = hist2d_axis<UNIFORM>(PER ? sEx + e * L.EXS : sEx, nx);
    const Hist2dAxis ay = hist2d_axis<UNIFORM>(PER ? sEy + e * L.EYS : sEy, ny);
    uint32_t* myC = sC + e * L.CS;
    unsigned long long* myG = a.counts + (batch * a.x.n + pair) * cells;
    const double* px = a.x.column(batch, pair);
    const double* py = a.y.column(batch, pair);
    unsigned long long out_n = 0ull, nan_n = 0ull;
    for (int64_t slice = blockIdx.y; slice < a.slices; slice += gridDim.y) {
      const int64_t r0 = slice * L.RB;
      const int64_t r1 = (r0 + L.RB < a.x.R) ? r0 + L.RB : a.x.R;
      for (int64_t r = r0 + rl; r < r1; r += 4 * RL) {
        double vx[4], vy[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const bool in = r + k * RL < r1;
          vx[k] = in ? px[(r + k * RL) * a.x.row_stride] : 0.0;
          vy[k] = in ? py[(r + k * RL) * a.y.row_stride] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (r + k * RL >= r1) continue;
          if (vx[k] != vx[k] || vy[k] != vy[k]) { ++nan_n; continue; }
          const int jx = hist2d_bin<UNIFORM>(ax, vx[k]), jy = hist2d_bin<UNIFORM>(ay, vy[k]);
          if ((jx | jy) < 0) { ++out_n; continue; }
          if (DIRECT) atomicAdd(myG + (jx * ny + jy), 1ull);
          else atomicAdd(&myC[jx * ny + jy], 1u);
        }
      }
    }
    if (out_n) atomicAdd(&sO[e * 2], out_n);
    if (nan_n) atomicAdd(&sO[e * 2 + 1], nan_n);
  }
  __syncthreads();

  if (!DIRECT) {
    unsigned long long* out = a.counts + (batch * a.x.n + j0) * cells;
    for (int i = tid; i < n_el * cells; i += HIST_THREADS) {
      const int el = i / cells;
      const uint32_t c = sC[el * L.CS + (i - el * cells)];
      if (c) atomicAdd(out + i, (unsigned long long)c);
    }
  }
  if (a.outside) {
    unsigned long long* oo = a.outside + (batch * a.x.n + j0) * 2;
    for (int i = tid; i < n_el * 2; i += HIST_THREADS)
      if (sO[i]) atomicAdd(oo + i, sO[i]);
  }
}

template <bool UNIFORM, bool DIRECT, bool OCC>
__global__ void __launch_bounds__(HIST_THREADS) k_hist2d_pool(Hist2dArgs a) {
  extern __shared__ double hist2d_lds[];
  const int nx = a.nx, ny = a.ny, cells = nx * ny;
  const Hist2dLayout L = hist2d_layout_form(nx, ny, 0, OCC ? HIST2D_POOLED_OCC : HIST2D_POOLED, DIRECT ? 1 : 0);
  double* sEx = hist2d_lds;
  double* sEy = (double*)((char*)hist2d_lds + L.ey_off);
  uint32_t* sC = (uint32_t*)((char*)hist2d_lds + L.counts_off);
  uint32_t* sOcc = (uint32_t*)((char*)hist2d_lds + L.occ_off);
  unsigned long long* sO = (unsigned long long*)((char*)hist2d_lds + L.outside_off);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t batch = blockIdx.x;

  for (int i = tid; i <= nx; i += HIST_THREADS) sEx[i] = a.ex[i];
  for (int i = tid; i <= ny; i += HIST_THREADS) sEy[i] = a.ey[i];
  if (!DIRECT) {
    for (int i = tid; i < cells; i += HIST_THREADS) sC[i] = 0u;
    if (OCC)
      for (int i = tid; i < cells; i += HIST_THREADS) sOcc[i] = 0u;
  }
  if (tid < 2) sO[tid] = 0ull;
  __syncthreads();

  const Hist2dAxis ax = hist2d_axis<UNIFORM>(sEx, nx), ay = hist2d_axis<UNIFORM>(sEy, ny);
  // slot u of a lane: row group u >> chunk_shift of the iteration, pairs 64 (u & (cpr - 1)) + p0 of the row; a row group is
  // rpp rows side by side in the wave, this lane on row s of it
  const int sh = a.pair_shift, csh = a.chunk_shift, rpp = 64 >> sh, cpr = 1 << csh, gpi = 4 >> csh;
  const int s = lane >> sh, p0 = lane & ((1 << sh) - 1);
  int64_t ox[4], oy[4];  // column offsets of the slots' pairs among the first 256
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t p = 64 * (u & (cpr - 1)) + p0;
    const bool in = p < a.x.n;
    ox[u] = in ? (a.x.idx ? a.x.idx[p] : p) : 0;
    oy[u] = in ? (a.y.idx ? a.y.idx[p] : p) : 0;
  }
  const double* bx = a.x.data + batch * a.x.batch_stride;
  const double* by = a.y.data + batch * a.y.batch_stride;
  unsigned long long* G = a.counts + batch * cells;
  unsigned long long* GO = OCC ? a.occupied + batch * cells : nullptr;
  unsigned long long out_n = 0ull, nan_n = 0ull;
  const int rows_it = gpi * rpp;  // rows of a wave's iteration
  for (int64_t slice = blockIdx.y; slice < a.slices; slice += gridDim.y) {
    const int64_t r0 = slice * L.RB;
    const int64_t r1 = (r0 + L.RB < a.x.R) ? r0 + L.RB : a.x.R;
    for (int64_t rb = r0 + wave * rows_it; rb < r1; rb += 4 * rows_it) {
      for (int64_t base = 0; base < a.x.n; base += 64 * 4) {  // (one trip unless a row has more than 256 pairs)
        double vx[4], vy[4];
        bool in[4];
        int key[4], cell[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int64_t r = rb + (u >> csh) * rpp + s, p = base + 64 * (u & (cpr - 1)) + p0;
          in[u] = r < r1 && p < a.x.n;
          int64_t cx = ox[u], cy = oy[u];
          if (base && in[u]) {
            cx = a.x.idx ? a.x.idx[p] : p;
            cy = a.y.idx ? a.y.idx[p] : p;
          }
          vx[u] = in[u] ? bx[r * a.x.row_stride + cx] : 0.0;
          vy[u] = in[u] ? by[r * a.y.row_stride + cy] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          key[u] = -1; cell[u] = 0;
          if (!in[u]) continue;
          if (vx[u] != vx[u] || vy[u] != vy[u]) { ++nan_n; continue; }
          const int jx = hist2d_bin<UNIFORM>(ax, vx[u]), jy = hist2d_bin<UNIFORM>(ay, vy[u]);
          if ((jx | jy) < 0) { ++out_n; continue; }
          const int c = jx * ny + jy;
          if (DIRECT) atomicAdd(G + c, 1ull);
          else atomicAdd(&sC[c], 1u);
          cell[u] = c;
          key[u] = ((u >> csh) * rpp + s) * cells + c;
        }
        if (OCC) {  // every lane of the wave gets here: rb and base do not depend on the lane
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            for (;;) {  // slot by slot: the first remaining key of the slot, read from its lane through a scalar register
              const unsigned long long left = __ballot(key[u] >= 0);
              if (!left) break;
              const int first = __ffsll(left) - 1;
              const int k = __builtin_amdgcn_readlane(key[u], first);
              if (lane == first) {
                if (DIRECT) atomicAdd(GO + cell[u], 1ull);
                else atomicAdd(&sOcc[cell[u]], 1u);
              }
#pragma unroll
              for (int v = u; v < 4; ++v)  // (only the slots of the same row group can hold the key again)
                if ((v >> csh) == (u >> csh) && key[v] == k) key[v] = -1;
            }
          }
        }
      }
    }
  }
  if (out_n) atomicAdd(&sO[0], out_n);
  if (nan_n) atomicAdd(&sO[1], nan_n);
  __syncthreads();

  if (!DIRECT) {
    for (int i = tid; i < cells; i += HIST_THREADS) {
      const uint32_t c = sC[i];
      if (c) atomicAdd(G + i, (unsigned long long)c);
      if (OCC) {
        const uint32_t o = sOcc[i];
        if (o) atomicAdd(GO + i, (unsigned long long)o);
      }
    }
  }
  if (a.outside && tid < 2 && sO[tid]) atomicAdd(a.outside + batch * 2 + tid, sO[tid]);
}

template <bool PER, bool UNIFORM>
void launch_pair(bool direct, dim3 grid, size_t lds, hipStream_t s, const Hist2dArgs& a) {
  if (direct) hipLaunchKernelGGL((k_hist2d_pair<PER, UNIFORM, true>), grid, dim3(HIST_THREADS), lds, s, a);
  else hipLaunchKernelGGL((k_hist2d_pair<PER, UNIFORM, false>), grid, dim3(HIST_THREADS), lds, s, a);
}
template <bool UNIFORM, bool OCC>
void launch_pool(bool direct, dim3 grid, size_t lds, hipStream_t s, const Hist2dArgs& a) {
  if (direct) hipLaunchKernelGGL((k_hist2d_pool<UNIFORM, true, OCC>), grid, dim3(HIST_THREADS), lds, s, a);
  else hipLaunchKernelGGL((k_hist2d_pool<UNIFORM, false, OCC>), grid, dim3(HIST_THREADS), lds, s, a);
}

}  // namespace

extern "C" omc_status omc_store_histogram2d_layout(int32_t nx, int32_t ny, int32_t edges_per_pair, int32_t pool_pairs, int32_t* out) {
  if (nx < 1 || nx > HIST_MAX_BINS || ny < 1 || ny > HIST_MAX_BINS || pool_pairs < 0 || pool_pairs > 2 || (edges_per_pair && pool_pairs) ||
      !out)
    return OMC_INVALID_ARG;
  const Hist2dLayout l = hist2d_layout(nx, ny, edges_per_pair != 0, pool_pairs);
  const int32_t v[14] = {l.direct, l.TE, l.RB, l.EXS, l.EYS, l.CS, l.ex_off, l.ey_off, l.counts_off, l.occ_off, l.outside_off, l.end,
                         HIST_LDS_BUDGET, HIST_THREADS};
  for (int i = 0; i < 14; ++i) out[i] = v[i];
  return OMC_OK;
}

extern "C" omc_status omc_store_histogram2d(omc_ctx* ctx, int64_t n_iter, int64_t size_x, const double* store_x, const int64_t* idx_x,
                                            int64_t size_y, const double* store_y, const int64_t* idx_y, int64_t n_pairs, int32_t pooled,
                                            int32_t pool_pairs, int32_t nx, const double* edges_x, int32_t ny, const double* edges_y,
                                            int32_t edges_per_pair, int64_t* counts_out, int64_t* outside_out, int64_t* occupied_out) {
  if (!omc_selection_ok(ctx, n_iter, 1, size_x, store_x, idx_x, n_pairs) || !omc_selection_ok(ctx, n_iter, 1, size_y, store_y, idx_y, n_pairs) ||
      nx < 1 || nx > HIST_MAX_BINS || ny < 1 || ny > HIST_MAX_BINS || !edges_x || !edges_y || !counts_out ||
      (edges_per_pair && pool_pairs) || (occupied_out && !pool_pairs))
    return OMC_INVALID_ARG;
  if (occupied_out && n_pairs > HIST2D_OCC_PAIRS) return OMC_UNSUPPORTED;  // a row's cells must stay in one wave
  const StoreView vx = omc_store_view(ctx, n_iter, size_x, pooled != 0, store_x, idx_x, n_pairs);
  const StoreView vy = omc_store_view(ctx, n_iter, size_y, pooled != 0, store_y, idx_y, n_pairs);
  const int64_t R = vx.R, batches = vx.batches;
  const bool per = edges_per_pair != 0;
  const int shape = !pool_pairs ? HIST2D_PER_PAIR : (occupied_out ? HIST2D_POOLED_OCC : HIST2D_POOLED);
  Hist2dLayout L = hist2d_layout(nx, ny, per, shape);
  if (!L.direct && (ctx->hist2d_algo & 1)) L = hist2d_layout_form(nx, ny, per, shape, 1);
  const int64_t tiles = pool_pairs ? 1 : (n_pairs + L.TE - 1) / L.TE;
  if (tiles * batches > 0x7fffffffLL) return OMC_INVALID_ARG;
  int64_t slices = (R + L.RB - 1) / L.RB, gy = slices < 65535 ? slices : 65535;
  // a workgroup's 32-bit counters see the rows it walks, times the pairs pooled into one grid
  if (!L.direct && (double)((slices + gy - 1) / gy) * (double)L.RB * (double)(pool_pairs ? n_pairs : 1) >= 4294967296.0) {
    L = hist2d_layout_form(nx, ny, per, shape, 1);
    slices = (R + L.RB - 1) / L.RB;
    gy = slices < 65535 ? slices : 65535;
  }
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  int32_t gx[2], gyw[2];
  omc_status st = omc_hist_check(ctx, idx_x, n_pairs, size_x, edges_x, per ? n_pairs : 1, nx, gx);
  if (st != OMC_OK) return st;
  st = omc_hist_check(ctx, idx_y, n_pairs, size_y, edges_y, per ? n_pairs : 1, ny, gyw);
  if (st != OMC_OK) return st;
  if (gx[0] || gyw[0]) return OMC_INVALID_ARG;
  const int64_t cells = (int64_t)nx * ny, grids = batches * (pool_pairs ? 1 : n_pairs);
  OMC_HIP_CHECK(hipMemsetAsync(counts_out, 0, (size_t)grids * cells * sizeof(int64_t), s));
  if (outside_out) OMC_HIP_CHECK(hipMemsetAsync(outside_out, 0, (size_t)grids * 2 * sizeof(int64_t), s));
  if (occupied_out) OMC_HIP_CHECK(hipMemsetAsync(occupied_out, 0, (size_t)batches * cells * sizeof(int64_t), s));
  Hist2dArgs a;
  a.x = vx; a.y = vy; a.ex = edges_x; a.ey = edges_y;
  a.counts = (unsigned long long*)counts_out; a.outside = (unsigned long long*)outside_out; a.occupied = (unsigned long long*)occupied_out;
  a.tiles = tiles; a.slices = slices; a.nx = nx; a.ny = ny;
  a.pair_shift = 6; a.chunk_shift = 0;
  if (n_pairs <= 32) {
    a.pair_shift = 0;
    while ((1 << a.pair_shift) < n_pairs) ++a.pair_shift;
  } else if (n_pairs > 64) {
    a.chunk_shift = n_pairs > 128 ? 2 : 1;
  }
  const bool uniform = gx[1] == 0 && gyw[1] == 0 && !(ctx->hist2d_algo & 2);
  const bool direct = L.direct != 0;
  const dim3 grid((unsigned)(tiles * batches), (unsigned)gy);
  const size_t lds = (size_t)L.end;
  if (!pool_pairs) {
    if (per) {
      if (uniform) launch_pair<true, true>(direct, grid, lds, s, a);
      else launch_pair<true, false>(direct, grid, lds, s, a);
    } else {
      if (uniform) launch_pair<false, true>(direct, grid, lds, s, a);
      else launch_pair<false, false>(direct, grid, lds, s, a);
    }
  } else if (occupied_out) {
    if (uniform) launch_pool<true, true>(direct, grid, lds, s, a);
    else launch_pool<false, true>(direct, grid, lds, s, a);
  } else {
    if (uniform) launch_pool<true, false>(direct, grid, lds, s, a);
    else launch_pool<false, false>(direct, grid, lds, s, a);
  }
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}
