// Autocovariance, autocorrelation and integrated autocorrelation time of the device-resident store, per chain or pooled over the
// chains, for the elements a user selects.  The contract is in include/omcmc_hip.h (omc_store_autocorr).
//
// store is [N][C][size].  A column is the N draws of one chain of one selected element.  A chunk of Kc selected elements, W = C Kc
// columns, is worked on at a time; column q = c Kc + e of the chunk belongs to chain c of element k0 + e of the selection:
//   omc_col_moments   the columns' means, per chain (omc_store_shared.hip), into mean_out or the workspace.
//   k_acorr_prepass   one lane per column, pieces of A_PRE rows.  It notes per column whether a draw differs from the first (bit 0: a
//                     column without it has s(t) = 0 by rule, not by rounding) and whether the mean is not finite (bit 1: a NaN
//                     draw, or an infinite one, whose deviation is inf - inf).  With an index it also writes the centred draws
//                     d = x - m, gathered, into a compact [N][W] workspace; without one the lag kernel reads the store where it
//                     lies and centres as it loads.  The flags are OR-ed by integer atomics.
//   k_acorr_lags      one lane per column, consecutive lanes on consecutive columns (every row load a coalesced run).  A block of
//                     lags is 32 accumulators and a 32-slot register ring (d_lag_block, omc_lag_block.h): two loads per 32 FMAs.
//                     Grid = column tiles x groups of four blocks of lags x time slices; the four waves of a workgroup take four
//                     adjacent blocks of lags of the same 64 columns and the same slice, so they walk the same rows at the same
//                     time and all but one of their reads of a row are served by the caches.  A slice owns the products whose LEFT
//                     factor lies in its rows [r0, r1): for lags [t0, t0 + 32) it walks i = r0 + t0 .. min(N, r1 + t0 + 31) - 1, so
//                     it reads up to max_lag rows past its end, however short the slice is.  Partials go to part [slice][lag][W].
//   k_acorr_sum       one thread per (lag, output column): the slices in ascending order, then (pooled) the chains in ascending
//                     order, the flags applied, the one division: g [lag][output column].
//   k_acorr_emit      tiles of 32 lags x 32 output columns turned through LDS: g read along the columns, the (normalised) lags
//                     written along the lags, both coalesced.
//   k_acorr_tau       one thread per output column: Geyer's initial positive sequence on rho(t) = g(t) / g(0), left when it ends.
// Slices are A_SLICE rows (option "autocorr_slice": any other length), a function of N alone; nothing else depends on how many
// columns a call has, so the order of additions depends on N, max_lag, C and that option only.  No floating-point atomics.
// Workspace (ctx->rank_ws): per column 256 (max_lag / 32 + 1) bytes of partials per slice, 8 (max_lag + 1) bytes of g, 8 N bytes of
// centred draws with an index, one flag word; Kc as rank_chunk (omc_rank_sort.h) sizes it: what fits 1 GiB, at least one element.
#include <math.h>

#include "omc_common.h"
#include "omc_lag_block.h"
#include "omc_rank_sort.h"
#include "omc_store_view.h"

namespace {

constexpr int A_L = 32;              // lags per block
constexpr int A_TILE = 64;           // columns per workgroup of the lag kernel (one wave's lanes)
constexpr int A_WAVES = 4;           // blocks of lags per workgroup of the lag kernel, a wave each
constexpr int64_t A_PRE = 256;       // rows per workgroup of the pre-pass (more where N / 256 exceeds a grid's 65535)
constexpr int64_t A_SLICE = 2048;    // rows per time slice (a choice: a slice re-reads 31 rows of the next one per block of lags, 1.5 %)

struct AcArgs {
  const double* store; const int64_t* idx; const double* mean;  // mean [C][n_idx]
  double* cen;      // [N][W] centred draws of the chunk (with an index)
  double* part;     // [slices][n_lb A_L][W]
  double* g;        // [L + 1][W]: the autocovariances of the output columns (pooled: the first Kc of a row)
  int32_t* flags;   // [W]
  double* acf_out; double* tau_out; int32_t* window_out;
  int64_t N, C, size, n_idx, k0, Kc, W, L, rps, n_slices, n_lb, pre_rows;
  int32_t per_chain, normalize;
};

// column q of the chunk: its first draw in the store, and its place in mean [C][n_idx]
__device__ __forceinline__ const double* ac_column(const AcArgs& a, int64_t q, int64_t& at) {
  const int64_t c = q / a.Kc, e = q - c * a.Kc;
  at = c * a.n_idx + a.k0 + e;
  return a.store + c * a.size + (a.idx ? a.idx[a.k0 + e] : a.k0 + e);
}

// workgroup (x, y) = (256 columns, piece of pre_rows rows)
template <bool GATHER>
__global__ void __launch_bounds__(256) k_acorr_prepass(AcArgs a) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= a.W) return;
  int64_t at;
  const double* __restrict__ p = ac_column(a, q, at);
  const double m = a.mean[at], x0 = p[0];
  const int64_t row = a.C * a.size;
  const int64_t r0 = (int64_t)blockIdx.y * a.pre_rows, r1 = r0 + a.pre_rows < a.N ? r0 + a.pre_rows : a.N;
  bool moved = false;
#pragma unroll 8
  for (int64_t r = r0; r < r1; ++r) {
    const double x = p[r * row];
    moved |= !(x == x0);
    if (GATHER) a.cen[r * a.W + q] = x - m;
  }
  const int32_t bits = (moved ? 1 : 0) | ((blockIdx.y == 0 && !isfinite(m)) ? 2 : 0);
  if (bits) atomicOr(&a.flags[q], bits);
}

// workgroup (x, y, z) = (tile of 64 columns, group of blockDim.x / 64 blocks of lags, time slice), a wave per block of lags
template <bool CENTRED>
__global__ void __launch_bounds__(A_TILE * A_WAVES) k_acorr_lags(AcArgs a) {
  const int64_t q = (int64_t)blockIdx.x * A_TILE + (threadIdx.x & 63);
  const int64_t qc = q < a.W ? q : a.W - 1;  // lanes past the end read a valid column and write nothing
  const int64_t lb = (int64_t)blockIdx.y * (blockDim.x >> 6) + (threadIdx.x >> 6), slice = blockIdx.z;
  if (lb >= a.n_lb) return;  // (whole waves: the kernel has no barrier)
  const int64_t t0 = lb * A_L;
  const int64_t r0 = slice * a.rps, r1 = r0 + a.rps < a.N ? r0 + a.rps : a.N;
  const int64_t i0 = r0 + t0, i1 = r1 + t0 + A_L - 1 < a.N ? r1 + t0 + A_L - 1 : a.N;
  double acc[A_L];
#pragma unroll
  for (int l = 0; l < A_L; ++l) acc[l] = 0.0;
  if (CENTRED) {
    const double* __restrict__ p = a.cen + qc;
    const int64_t ld = a.W;
    d_lag_block<A_L>(t0, i0, i1, r1, [&](int64_t i) { return p[i * ld]; }, [](double x) { return x; }, acc);
  } else {
    int64_t at;
    const double* __restrict__ p = ac_column(a, qc, at);
    const double m = a.mean[at];
    const int64_t ld = a.C * a.size;
    d_lag_block<A_L>(t0, i0, i1, r1, [&](int64_t i) { return p[i * ld]; }, [&](double x) { return x - m; }, acc);
  }
  if (q < a.W) {
    double* o = a.part + ((slice * a.n_lb + lb) * A_L) * a.W + q;
#pragma unroll
    for (int l = 0; l < A_L; ++l) o[l * a.W] = acc[l];
  }
}

// thread x: output column j (per chain: column q = j; pooled: element j of the chunk); the lags walk grid y.  Every load is
// unconditional (a constant column's partials are read and dropped), so the loads of several chains are in flight at once.
__global__ void __launch_bounds__(256) k_acorr_sum(AcArgs a) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= (a.per_chain ? a.W : a.Kc)) return;
  const int64_t chains = a.per_chain ? 1 : a.C, slice_stride = a.n_lb * A_L * a.W;
  const double denom = a.per_chain ? (double)a.N : (double)a.N * (double)a.C;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  for (int64_t t = blockIdx.y; t <= a.L; t += gridDim.y) {
    double S = 0.0;
    int32_t seen = 0;
#pragma unroll 8
    for (int64_t c = 0; c < chains; ++c) {
      const int64_t q = c * a.Kc + j;
      const int32_t f = a.flags[q];
      const double* o = a.part + t * a.W + q;
      double s = 0.0;
      for (int64_t sl = 0; sl < a.n_slices; ++sl) s += o[sl * slice_stride];
      S += (f & 1) ? s : 0.0;
      seen |= f;
    }
    a.g[t * a.W + j] = (seen & 2) ? nan : S / denom;
  }
}

// where output column j of the chunk lies in the outputs: position in [C][n_idx] per chain, in [n_idx] pooled
__device__ __forceinline__ int64_t ac_out_at(const AcArgs& a, int64_t j) {
  const int64_t c = j / a.Kc, e = j - c * a.Kc;  // (pooled: j < Kc, c = 0)
  return c * a.n_idx + a.k0 + e;
}

// workgroup (x, y) = (32 output columns, 32 lags), 32 x 8 threads
__global__ void __launch_bounds__(256) k_acorr_emit(AcArgs a) {
  __shared__ double tile[32][33];
  __shared__ double g0[32];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t J = a.per_chain ? a.W : a.Kc, j0 = (int64_t)blockIdx.x * 32, t0 = (int64_t)blockIdx.y * 32;
  if (ty == 0) g0[tx] = j0 + tx < J ? a.g[j0 + tx] : 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t t = t0 + ty + 8 * r, j = j0 + tx;
    tile[ty + 8 * r][tx] = (t <= a.L && j < J) ? a.g[t * a.W + j] : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t j = j0 + ty + 8 * r, t = t0 + tx;
    if (j < J && t <= a.L) {
      const double gt = tile[tx][ty + 8 * r];
      a.acf_out[ac_out_at(a, j) * (a.L + 1) + t] = a.normalize ? gt / g0[ty + 8 * r] : gt;
    }
  }
}

// thread x: output column j; Geyer's initial positive sequence on rho(t) = g(t) / g(0)
__global__ void __launch_bounds__(256) k_acorr_tau(AcArgs a) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= (a.per_chain ? a.W : a.Kc)) return;
  const double* g = a.g + j;
  const double g0 = g[0];
  double tau = -1.0;
  int32_t window = 0;
  for (int64_t k = 0; 2 * k + 1 <= a.L; ++k) {
    const double pair = g[2 * k * a.W] / g0 + g[(2 * k + 1) * a.W] / g0;
    if (!(pair > 0.0)) break;
    tau += 2.0 * pair;
    window += 2;
  }
  const double one = g0 / g0;
  if (one != one) {  // g(0) is NaN, zero or infinite: no autocorrelation to sum
    tau = __longlong_as_double(0x7ff8000000000000LL);
    window = 0;
  }
  const int64_t at = ac_out_at(a, j);
  if (a.tau_out) a.tau_out[at] = tau;
  if (a.window_out) a.window_out[at] = window;
}

}  // namespace

extern "C" omc_status omc_store_autocorr(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx, int64_t n_idx,
                                         int64_t max_lag, int32_t per_chain, int32_t normalize, double* acf_out, double* tau_out,
                                         int32_t* window_out, double* mean_out) {
  if (!ctx) return omc_invalid("omc_store_autocorr: no context");
  if (n_iter < 2) return omc_invalid("omc_store_autocorr: n_iter < 2");
  if (size < 1) return omc_invalid("omc_store_autocorr: size < 1");
  if (!store || !acf_out) return omc_invalid("omc_store_autocorr: store and acf_out must not be NULL");
  if (n_idx < 1 || (!idx && n_idx != size)) return omc_invalid("omc_store_autocorr: n_idx < 1, or no index and n_idx != size");
  if (max_lag < 0 || max_lag > n_iter - 1) return omc_invalid("omc_store_autocorr: max_lag outside [0, n_iter - 1]");
  const int64_t N = n_iter, C = ctx->n_chains, L = max_lag;
  const int64_t rps = ctx->autocorr_slice > 0 ? ctx->autocorr_slice : A_SLICE;
  const int64_t n_slices = (N + rps - 1) / rps, n_lb = L / A_L + 1;
  if (n_slices > 65535 || n_lb > 65535) return omc_invalid("omc_store_autocorr: more time slices or blocks of lags than one launch takes (65535)");
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  int64_t pre_rows = A_PRE;
  if ((N + pre_rows - 1) / pre_rows > 65535) pre_rows = (N + 65534) / 65535;
  const size_t per_col = ((size_t)n_slices * n_lb * A_L + (size_t)(L + 1) + (idx ? (size_t)N : 0)) * sizeof(double) + sizeof(int32_t);
  const int64_t Kc = rank_chunk(ctx, per_col * (size_t)C, n_idx);
  const int64_t W_max = C * Kc;
  if ((W_max + 31) / 32 > 0x7fffffffLL) return omc_invalid("omc_store_autocorr: more columns than one launch takes");
  const size_t n_mean = mean_out ? 0 : (size_t)C * n_idx, n_part = (size_t)n_slices * n_lb * A_L * W_max, n_g = (size_t)(L + 1) * W_max,
               n_cen = idx ? (size_t)N * W_max : 0;
  omc_status st = omc_ensure(ctx, ctx->rank_ws, RANK_HEAD + (n_mean + n_part + n_g + n_cen) * sizeof(double) + (size_t)W_max * sizeof(int32_t));
  if (st != OMC_OK) return st;
  char* ws = (char*)ctx->rank_ws.p;
  double* mean = mean_out ? mean_out : (double*)(ws + RANK_HEAD);
  double* part = (double*)(ws + RANK_HEAD) + n_mean;
  double* g = part + n_part;
  double* cen = g + n_g;
  int32_t* flags = (int32_t*)(cen + n_cen);
  st = omc_store_check_index(ctx, (int32_t*)ws, idx, n_idx, size);
  if (st == OMC_INVALID_ARG) return omc_invalid("omc_store_autocorr: an index outside [0, size)");
  if (st != OMC_OK) return st;
  st = omc_col_moments(ctx, omc_store_view(ctx, N, size, false, store, idx, n_idx), mean, nullptr);
  if (st != OMC_OK) return st;
  hipStream_t s = ctx->stream;
  AcArgs a;
  a.store = store; a.idx = idx; a.mean = mean; a.cen = cen; a.part = part; a.g = g; a.flags = flags;
  a.acf_out = acf_out; a.tau_out = tau_out; a.window_out = window_out;
  a.N = N; a.C = C; a.size = size; a.n_idx = n_idx; a.L = L; a.rps = rps; a.n_slices = n_slices; a.n_lb = n_lb; a.pre_rows = pre_rows;
  a.per_chain = per_chain != 0; a.normalize = normalize != 0;
  const unsigned lag_rows = (unsigned)(L + 1 < 65535 ? L + 1 : 65535);
  const int64_t waves = n_lb < A_WAVES ? n_lb : A_WAVES;
  for (int64_t k0 = 0; k0 < n_idx; k0 += Kc) {
    const int64_t kc = n_idx - k0 < Kc ? n_idx - k0 : Kc, W = C * kc, J = per_chain ? W : kc;
    a.k0 = k0; a.Kc = kc; a.W = W;
    OMC_HIP_CHECK(hipMemsetAsync(flags, 0, (size_t)W * sizeof(int32_t), s));
    const dim3 pre(omc_grid1(W, 256), (unsigned)((N + pre_rows - 1) / pre_rows));
    const dim3 lags(omc_grid1(W, A_TILE), (unsigned)((n_lb + waves - 1) / waves), (unsigned)n_slices), lag_threads((unsigned)(A_TILE * waves));
    if (idx) {
      hipLaunchKernelGGL(k_acorr_prepass<true>, pre, dim3(256), 0, s, a);
      hipLaunchKernelGGL(k_acorr_lags<true>, lags, lag_threads, 0, s, a);
    } else {
      hipLaunchKernelGGL(k_acorr_prepass<false>, pre, dim3(256), 0, s, a);
      hipLaunchKernelGGL(k_acorr_lags<false>, lags, lag_threads, 0, s, a);
    }
    hipLaunchKernelGGL(k_acorr_sum, dim3(omc_grid1(J, 256), lag_rows), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_acorr_emit, dim3(omc_grid1(J, 32), (unsigned)n_lb), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_acorr_tau, dim3(omc_grid1(J, 256)), dim3(256), 0, s, a);
    OMC_HIP_CHECK(hipGetLastError());
  }
  return OMC_OK;
}
