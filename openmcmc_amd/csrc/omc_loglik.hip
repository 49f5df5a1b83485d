// Column summaries of the pointwise Normal log-density of the device store: for every observation the log-sum-exp, the mean and
// the unbiased variance, over all stored draws, of ll = 0.5 log(tau) - 0.5 log(2 pi) - 0.5 tau (y - x)^2 -- what WAIC needs, and the
// pointwise entry itself where it is asked for.  The contract is in include/omcmc_hip.h (omc_store_loglik).
//
// What it replaces: the loop over MCMC.store[...] of the reference that calls Normal.log_p(..., by_observation=True) per stored
// draw (distribution/location_scale.py:145-166; host arrays there).  store is the mean entry [n_iter][C][size]; a ROW is the size
// contiguous doubles of one (iteration, chain), S = n_iter C rows.  Selection position k = 0 .. n_idx - 1 is element idx[k] of
// the row (k itself without an index); y and a vector precision are aligned with k.
//
//   k_loglik_head  prec_size == 1: h[row] = 0.5 log(tau[row]) - c, one logarithm per ROW, into the workspace.
//   k_loglik_part  a workgroup owns LL_COLS = 32 adjacent selection positions and a slice of the rows; thread (cl, rr), cl = 0 .. 15
//                  along the row and rr = 0 .. 15 down it, carries TWO columns: 2 cl and 2 cl + 1 of the tile, read with one 16-byte
//                  load (VEC: no index, an even size, a 16-byte aligned store), else cl and cl + 16, two 8-byte loads that each
//                  coalesce over the 16 lanes (through the index, read once per thread, where there is one).  Two rows are in
//                  flight per thread.  A column's rows go to row lane rr = row mod 16 of the slice in ascending order in both
//                  forms, so the two forms give the same bits.  Per column a lane carries the pair (M, s) of omc_loglik.h --
//                  one exp per element -- next to Welford's (mean, m2) of omc_moments.h, the count and its reciprocal shared by
//                  the thread's two columns (one division per row, not per element), and notes a term that is not finite (it
//                  enters neither).  The 16 row lanes are joined 1 .. 15 in order through LDS -- (M, s) by
//                  omc_lse_join, the moments by Chan's update -- into part [slices][5][n_idx] (M, s, count, mean, m2; M = NaN marks
//                  a column with a term that is not finite).
//   k_loglik_join  thread = column: the slices in slice order; lse = M + log(s), var = m2 / (S - 1).
// Slices: about 2048 workgroups, no slice shorter than 256 rows, at most 1024 -- omc_col_moments' rule, a function of the shape
// alone.  No atomics, no scratch; repeated calls are bit-equal.
//
// Roundings a term of the log-sum-exp passes through on its way into the sum: every later addition into its accumulator is one
// fused multiply-add and, where the maximum moves, carries the error of one exp of the rescaling: at most 2 per addition or join.
// A lane takes L = ceil(rows_per_slice / 16) terms, min(16, rows_per_slice) lanes and `slices` slices are joined (an empty side adds
// nothing and is exact):   K = 2 ((L - 1) + (min(16, rows_per_slice) - 1) + (slices - 1))  <=  2 (S - 1).
#include "omc_common.h"
#include "omc_loglik.h"
#include "omc_moments.h"
#include "omc_store_view.h"

namespace {

constexpr int LL_COLS = 32, LL_ROWS = 16;  // k_loglik_part: selection positions and row lanes of a workgroup
constexpr int LL_FLY = 2;                  // rows a thread has in flight (1: 7.0 ms, 2: 4.6 ms, 4: 4.8 ms over the cfg3 store)
constexpr size_t LL_HEAD = 64;             // bytes in front of the arrays of ctx->store_ws: the word of the index check

struct LlArgs {
  const double* store; const int64_t* idx; const double* y; const double* prec; const double* head;
  double* part; double* ll_out;
  int64_t S, size, n_idx, prec_size, rows_per_block;
};

// a column of a thread: (M, s) and Welford's (mean, m2); the count is the thread's own, the rows it has taken, shared by its two
// columns -- a term that is not finite enters nothing, and its column is NaN whatever the moments then hold
struct LlAcc {
  double M, s, mean, m2;
  int bad;
  __device__ __forceinline__ void init() {
    M = -__longlong_as_double(0x7ff0000000000000LL); s = 0.0; mean = 0.0; m2 = 0.0; bad = 0;
  }
  __device__ __forceinline__ void add(double ll, double inv_n) {
    if (omc_ll_finite(ll)) {
      omc_lse_add(M, s, ll, 1.0);
      omc_welford_nth(inv_n, mean, m2, ll);
    } else {
      bad = 1;
    }
  }
};

__global__ void __launch_bounds__(256) k_loglik_head(int64_t S, const double* __restrict__ prec, double* __restrict__ head) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r < S) head[r] = omc_normal_ll_head(prec[r]);
}

template <bool VEC>
__global__ void __launch_bounds__(256) k_loglik_part(LlArgs g) {
  __shared__ double sm[5][LL_ROWS][LL_COLS];
  const int tid = threadIdx.x, cl = tid & 15, rr = tid >> 4;
  const int c0 = VEC ? 2 * cl : cl, c1 = VEC ? 2 * cl + 1 : cl + 16;  // the thread's two columns of the tile
  const int64_t k0 = (int64_t)blockIdx.x * LL_COLS + c0, k1 = (int64_t)blockIdx.x * LL_COLS + c1;
  const bool ok0 = k0 < g.n_idx, ok1 = k1 < g.n_idx;  // (VEC: n_idx is even, both or none)
  const int64_t e0 = ok0 ? (g.idx ? g.idx[k0] : k0) : 0, e1 = ok1 ? (g.idx ? g.idx[k1] : k1) : 0;  // 0 <= idx[k] < size: checked before the launch
  const double y0 = ok0 ? g.y[k0] : 0.0, y1 = ok1 ? g.y[k1] : 0.0;
  const bool per_row = g.prec_size == 1;
  const int64_t r_begin = (int64_t)blockIdx.y * g.rows_per_block;
  const int64_t r_end = r_begin + g.rows_per_block < g.S ? r_begin + g.rows_per_block : g.S;
  LlAcc a0, a1;
  a0.init();
  a1.init();
  double cnt = 0.0;
  for (int64_t rb = r_begin + rr; rb < r_end; rb += LL_FLY * LL_ROWS) {
    double x0[LL_FLY], x1[LL_FLY], t0[LL_FLY], t1[LL_FLY], h[LL_FLY];
#pragma unroll
    for (int u = 0; u < LL_FLY; ++u) {
      const int64_t r = rb + u * LL_ROWS;
      x0[u] = x1[u] = 0.0; t0[u] = t1[u] = 1.0; h[u] = 0.0;
      if (r < r_end) {
        if (VEC) {
          if (ok0) {
            const double2 v = *(const double2*)(g.store + r * g.size + e0);
            x0[u] = v.x; x1[u] = v.y;
          }
        } else {
          if (ok0) x0[u] = g.store[r * g.size + e0];
          if (ok1) x1[u] = g.store[r * g.size + e1];
        }
        if (per_row) {
          t0[u] = t1[u] = g.prec[r];
          h[u] = g.head[r];
        } else {
          if (ok0) t0[u] = g.prec[r * g.n_idx + k0];
          if (ok1) t1[u] = g.prec[r * g.n_idx + k1];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < LL_FLY; ++u) {
      const int64_t r = rb + u * LL_ROWS;
      if (r < r_end) {
        const double l0 = omc_normal_ll(per_row ? h[u] : omc_normal_ll_head(t0[u]), t0[u], y0, x0[u]);
        const double l1 = omc_normal_ll(per_row ? h[u] : omc_normal_ll_head(t1[u]), t1[u], y1, x1[u]);
        cnt += 1.0;
        const double inv_n = 1.0 / cnt;  // one division for both columns
        if (ok0) a0.add(l0, inv_n);
        if (ok1) a1.add(l1, inv_n);
        if (g.ll_out) {
          if (ok0) g.ll_out[r * g.n_idx + k0] = l0;
          if (ok1) g.ll_out[r * g.n_idx + k1] = l1;
        }
      }
    }
  }
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  sm[0][rr][c0] = a0.bad ? nan : a0.M; sm[1][rr][c0] = a0.s; sm[2][rr][c0] = cnt; sm[3][rr][c0] = a0.mean; sm[4][rr][c0] = a0.m2;
  sm[0][rr][c1] = a1.bad ? nan : a1.M; sm[1][rr][c1] = a1.s; sm[2][rr][c1] = cnt; sm[3][rr][c1] = a1.mean; sm[4][rr][c1] = a1.m2;
  __syncthreads();
  const int64_t k = (int64_t)blockIdx.x * LL_COLS + tid;
  if (tid < LL_COLS && k < g.n_idx) {
    double M = sm[0][0][tid], s = sm[1][0][tid], num = sm[2][0][tid], mean = sm[3][0][tid], m2 = sm[4][0][tid];
    bool bad = M != M;
    for (int q = 1; q < LL_ROWS; ++q) {
      const double Mq = sm[0][q][tid];
      if (Mq != Mq) bad = true;
      else if (!bad) omc_lse_join(M, s, Mq, sm[1][q][tid]);
      omc_chan(num, mean, m2, sm[2][q][tid], sm[3][q][tid], sm[4][q][tid]);
    }
    double* o = g.part + (int64_t)blockIdx.y * 5 * g.n_idx + k;
    o[0] = bad ? nan : M; o[g.n_idx] = s; o[2 * g.n_idx] = num; o[3 * g.n_idx] = mean; o[4 * g.n_idx] = m2;
  }
}

__global__ void __launch_bounds__(256) k_loglik_join(int64_t n, int slices, const double* __restrict__ part, double* __restrict__ lse_out,
                                                     double* __restrict__ mean_out, double* __restrict__ var_out) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  double M = -__longlong_as_double(0x7ff0000000000000LL), s = 0.0, cnt = 0.0, mean = 0.0, m2 = 0.0;
  bool bad = false;
  for (int q = 0; q < slices; ++q) {
    const double* o = part + (int64_t)q * 5 * n + k;
    const double Mq = o[0];
    if (Mq != Mq) bad = true;
    else if (!bad) omc_lse_join(M, s, Mq, o[n]);
    omc_chan(cnt, mean, m2, o[2 * n], o[3 * n], o[4 * n]);
  }
  if (lse_out) lse_out[k] = bad ? nan : M + log(s);
  if (mean_out) mean_out[k] = bad ? nan : mean;
  if (var_out) var_out[k] = bad ? nan : m2 / (cnt - 1.0);
}

}  // namespace

extern "C" omc_status omc_store_loglik(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx, int64_t n_idx,
                                       const double* y, const double* prec, int64_t prec_size, double* lse_out, double* mean_out,
                                       double* var_out, double* ll_out) {
  if (!ctx) return omc_invalid("omc_store_loglik: no context");
  if (n_iter < 1 || n_iter * ctx->n_chains < 2) return omc_invalid("omc_store_loglik: fewer than 2 stored draws (n_iter * C < 2)");
  if (size < 1) return omc_invalid("omc_store_loglik: size < 1");
  if (!store || !y || !prec) return omc_invalid("omc_store_loglik: store, y and prec must not be NULL");
  if (n_idx < 1 || (!idx && n_idx != size)) return omc_invalid("omc_store_loglik: n_idx < 1, or no index and n_idx != size");
  if (prec_size != 1 && prec_size != n_idx) return omc_invalid("omc_store_loglik: prec_size must be 1 or n_idx");
  if (!lse_out && !mean_out && !var_out && !ll_out) return omc_invalid("omc_store_loglik: every output is NULL");
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  const StoreView v = omc_store_view(ctx, n_iter, size, true, store, idx, n_idx);  // pooled: S rows of row_stride = size doubles
  const int64_t S = v.R;
  const int64_t tiles = (n_idx + LL_COLS - 1) / LL_COLS;
  int64_t rpb;
  const int64_t slices = omc_row_slices(tiles, S, &rpb);
  if (tiles > 0x7fffffffLL || (S + 255) / 256 > 0x7fffffffLL) return omc_invalid("omc_store_loglik: more columns or rows than one launch takes");
  const size_t head_bytes = prec_size == 1 ? (size_t)S * sizeof(double) : 0;
  omc_status st = omc_ensure(ctx, ctx->store_ws, LL_HEAD + head_bytes + (size_t)slices * 5 * n_idx * sizeof(double));
  if (st != OMC_OK) return st;
  char* ws = (char*)ctx->store_ws.p;
  st = omc_store_check_index(ctx, (int32_t*)ws, idx, n_idx, size);
  if (st == OMC_INVALID_ARG) return omc_invalid("omc_store_loglik: an index outside [0, size)");  // (the helper's only use of that status)
  if (st != OMC_OK) return st;
  LlArgs g;
  g.store = v.data; g.idx = v.idx; g.y = y; g.prec = prec; g.head = (const double*)(ws + LL_HEAD);
  g.part = (double*)(ws + LL_HEAD + head_bytes); g.ll_out = ll_out;
  g.S = S; g.size = v.row_stride; g.n_idx = n_idx; g.prec_size = prec_size; g.rows_per_block = rpb;
  if (prec_size == 1)
    hipLaunchKernelGGL(k_loglik_head, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, ctx->stream, S, prec, (double*)(ws + LL_HEAD));
  const dim3 grid((unsigned)tiles, (unsigned)slices);
  const bool vec = !idx && size % 2 == 0 && ((uintptr_t)store & 15) == 0;
  if (vec) hipLaunchKernelGGL(k_loglik_part<true>, grid, dim3(256), 0, ctx->stream, g);
  else hipLaunchKernelGGL(k_loglik_part<false>, grid, dim3(256), 0, ctx->stream, g);
  if (lse_out || mean_out || var_out)
    hipLaunchKernelGGL(k_loglik_join, dim3((unsigned)((n_idx + 255) / 256)), dim3(256), 0, ctx->stream, n_idx, (int)slices, g.part, lse_out,
                       mean_out, var_out);
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}
