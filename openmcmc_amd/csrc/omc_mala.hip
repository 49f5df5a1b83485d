// Metropolis-Hastings steps (ManifoldMALA, RandomWalk) for a Gaussian target with shared constant
// Hessian, batched over chains as level-3 BLAS on the d x C state matrix (rocBLAS: fp64 MFMA).
// Reference: sampler/metropolis_hastings.py:102-173, 212-269, 301-373; location_scale.py:222-232.
//
// The five steps (omc_mala_step, omc_mala_step_white, omc_mala_run_white, omc_rw_step, omc_rw_step_white) owe each other equal
// decisions, the run and the single whitened step bit for bit.  What that rests on is written once, under "shared arithmetic"
// below: the block reduction (mh_block_partials, mh_total4), the log target and the proposal term (MhTarget), the decision
// (mh_odds, MhOdds::decide), the counters (mh_count), the pair of normals (mh_normal_pair) and the random walk's move
// (mh_rw_move); the step's uniform is omc_chain_uniform (omc_common.h).  The kernels keep their own loops, registers and barriers.
#include <math.h>

#include "omc_blas.h"

static unsigned gx(int64_t n) {
  int64_t g = (n + 255) / 256;
  return (unsigned)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}

// ---- shared arithmetic: every piece of a step that two kernels must compute alike ----------------------------------------

// Sums of a workgroup of 256 threads, first half: each of the sums s... (doubles) is reduced over its wave (xor ladder), and
// lane 0 of wave w parks the k-th partial in red[k][w].  The barrier between this and the reading of red is the caller's
// (the kernels differ in who reads, and k_mala_white_run alternates between two buffers).
template <typename... S>
__device__ __forceinline__ void mh_block_partials(double (*red)[4], S&... s) {
  for (int o = 32; o >= 1; o >>= 1) ((s += __shfl_xor(s, o, 64)), ...);
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    int k = 0;
    ((red[k++][w] = s), ...);
  }
}
// ... second half: the four partials of one sum, always in this order
__device__ __forceinline__ double mh_total4(const double* r) { return (r[0] + r[1]) + (r[2] + r[3]); }

// The Gaussian target N(mu, Q^-1) and the proposal N(m, (L L')^-1) as functions of a squared norm ss = |L'(.)|^2.
// L = chol(Q / step^2) => chol(Q) = step L: log det Q = 2 (sum log diag L + d log step), |chol(Q)'(x - mu)|^2 = step^2 ss.
struct MhTarget {
  double sl, logdetQ, dnum, lp_scale;
  __device__ __forceinline__ double lp(double ss) const {  // gmrf.py:339-344
    return 0.5 * (logdetQ - dnum * 1.8378770664093453 - lp_scale * ss);
  }
  __device__ __forceinline__ double lq(double ss) const { return sl - 0.5 * ss; }  // metropolis_hastings.py:372-373
};
__device__ __forceinline__ MhTarget mh_target(double sumlogL, double log_step_term, int64_t d, double lp_scale) {
  return {sumlogL, 2.0 * (sumlogL + log_step_term), (double)d, lp_scale};
}

// The decision (metropolis_hastings.py:127-173) in two halves, so that a kernel chooses where its uniform is drawn.
// mh_odds: log_alpha from the totals of red: rows 0, 1 = |L'(x - mu)|^2 of the current and the proposed state; for an
// asymmetric proposal rows 2, 3 = |L'(x - m')|^2 (reverse) and |L'(x' - m)|^2 (forward).  decide: the test against log u;
// lp is the log target of the state the step leaves behind.
struct MhDecision { bool ok; double lp; };
struct MhOdds {
  double lp_cur, lp_prop, log_alpha;
  __device__ __forceinline__ MhDecision decide(double log_u) const {
    const bool ok = log_u < log_alpha;  // :173
    return {ok, ok ? lp_prop : lp_cur};
  }
};
__device__ __forceinline__ MhOdds mh_odds(const double (*red)[4], bool asymmetric, const MhTarget& tgt) {
  const double lp_cur = tgt.lp(mh_total4(red[0])), lp_prop = tgt.lp(mh_total4(red[1]));
  double log_alpha = lp_prop - lp_cur;
  if (asymmetric) {
    const double lq_rev = tgt.lq(mh_total4(red[2])), lq_fwd = tgt.lq(mh_total4(red[3]));
    log_alpha = lp_prop + lq_rev - (lp_cur + lq_fwd);  // :155
  }
  return {lp_cur, lp_prop, log_alpha};
}
__device__ __forceinline__ void mh_count(long long* acc_cnt, long long* prop_cnt, int64_t c, bool ok) {
  if (prop_cnt) prop_cnt[c] += 1;
  if (acc_cnt && ok) acc_cnt[c] += 1;
}

// Elements 2q, 2q + 1 of a chain's N(0, I) draw: from its row of the injected array (zrow != NULL), or block q of its normal
// stream (gc: the global chain).  Beyond the end (2q + 1 >= d, odd d) z[1] is not part of the draw.
__device__ __forceinline__ void mh_normal_pair(const double* zrow, int64_t d, int64_t q, const omc_rng_key& key, int64_t gc,
                                               double (&z)[2]) {
  if (zrow) {
    z[0] = zrow[2 * q];
    z[1] = (2 * q + 1 < d) ? zrow[2 * q + 1] : 0.0;
  } else {
    omc_normal_pair(omc_rng_block(key, gc, (uint32_t)q), z[0], z[1]);
  }
}

// x + step z in two roundings, like numpy's x + z * step
__device__ __forceinline__ double mh_rw_move(double x, double z, double step) {
#pragma clang fp contract(off)
  const double prod = z * step;
  return x + prod;
}

// z[c][:] from the injected array or the chain's normal stream
__global__ void k_draw_normals(int64_t d, int64_t chain_offset, omc_rng_key key, const double* zin, int64_t ld_z,
                               double* z, int64_t ld_o) {
  const int64_t c = blockIdx.y;
  const int64_t npairs = (d + 1) / 2;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < npairs; q += (int64_t)gridDim.x * blockDim.x) {
    double zq[2];
    mh_normal_pair(zin ? zin + c * ld_z : nullptr, d, q, key, chain_offset + c, zq);
    z[c * ld_o + 2 * q] = zq[0];
    if (2 * q + 1 < d) z[c * ld_o + 2 * q + 1] = zq[1];
  }
}
__global__ void k_sumlogdiag(int64_t d, const double* L, double* out) {
  __shared__ double red[1][4];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < d; i += blockDim.x) acc += log(L[i * d + i]);
  mh_block_partials(red, acc);
  __syncthreads();
  if (threadIdx.x == 0) out[0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
}
__global__ void k_scale_copy(int64_t total, const double* a, double scale, double* out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = scale * a[i];
}
__global__ void k_latch_info(const int* info, long long* bad) {
  if (info[0] != 0) atomicMin((unsigned long long*)bad, 0ull);
}

struct MhWork {
  double *R, *G, *M, *V, *XP, *T, *ss;  // d x C matrices (ld = d) and 4*C scalars
  int* flag;
};

static omc_status mh_workspace(omc_ctx* ctx, int64_t d, MhWork* w) {
  const int64_t C = ctx->n_chains;
  const size_t mat = (size_t)C * d;
  const size_t need = (13 * mat + 4 * (size_t)C) * sizeof(double) + (size_t)C * sizeof(int) + 64;
  omc_status st = omc_ensure(ctx, ctx->mh_work, need);
  if (st != OMC_OK) return st;
  double* base = ctx->mh_work;
  w->R = base; w->G = base + mat; w->M = base + 2 * mat; w->V = base + 3 * mat; w->XP = base + 4 * mat;
  w->T = base + 5 * mat;  // 8 * mat: T4 and its TRMM image
  w->ss = base + 13 * mat;
  w->flag = (int*)(w->ss + 4 * C);
  return OMC_OK;
}

// What every step does once its own argument test has passed: the chain limit (chains are a grid dimension), the device, the
// BLAS handle and, where the step uses it (w != NULL), the workspace.
static omc_status mh_enter(omc_ctx* ctx, int64_t d, MhWork* w) {
  if (ctx->n_chains > 65535) return OMC_UNSUPPORTED;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  omc_status st = omc_ensure_blas(ctx);
  if (st != OMC_OK) return st;
  return w ? mh_workspace(ctx, d, w) : OMC_OK;
}

static bool mh_own_gemm(const omc_ctx* ctx, int64_t d) { return !ctx->mh_use_rocblas && d <= 46340; }

// ---- several whitened steps per launch ----------------------------------------------------------------------------------
// The whitened step is element-wise in a = L'(x - mu) plus four sums and one decision per chain: nothing in it needs x.  K steps
// are therefore ONE launch that keeps a chain's a in registers (a workgroup per chain, a pair of elements per thread), leaves
// the whitened trajectory a_t behind, and ONE triangular product afterwards maps all K x C states back, x_t = mu + L^-T a_t,
// straight into the store slabs (mcmc.py:105-106 stores the state of every iteration) -- a d x d by d x (K C) product that
// fills the chip, where a product per step (d x C) occupies a quarter of it for 12 us.  Same draws (stream draw_index0 +
// t draw_stride for step t), same sums in the same order, same decision as K calls of omc_mala_step_white: bit-identical a
// and counters, and x of every stored step equal to what the single steps leave (same product, column by column).
template <int NP>
__global__ void __launch_bounds__(256) k_mala_white_run(int64_t d, int64_t C, int64_t chain_offset, uint64_t seed, uint64_t draw_index0,
                                                        uint64_t draw_stride, int n_steps, const double* __restrict__ zin, int64_t ld_z,
                                                        const double* __restrict__ u_in, const double* __restrict__ sumlogL,
                                                        double log_step_term, double lp_scale, double kappa, double* __restrict__ a,
                                                        double* __restrict__ a_traj, long long* __restrict__ acc_cnt,
                                                        long long* __restrict__ prop_cnt, double* __restrict__ logp_traj,
                                                        double* __restrict__ logp_last) {
  __shared__ double red[2][4][4];
  const int64_t c = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t npairs = (d + 1) / 2;
  double av[NP][2];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int64_t i = 2 * ((int64_t)tid + 256 * p) + e;
      av[p][e] = i < d ? a[c * d + i] : 0.0;
    }
  const MhTarget tgt = mh_target(sumlogL[0], log_step_term, d, lp_scale);
  long long n_acc = 0;
  double lp_state = 0.0;
  for (int t = 0; t < n_steps; ++t) {
    const omc_rng_key nkey = omc_make_key(seed, draw_index0 + (uint64_t)t * draw_stride, OMC_RNG_NORMAL);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    double ap[NP][2];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int64_t q = (int64_t)tid + 256 * p;
      ap[p][0] = ap[p][1] = 0.0;
      if (q < npairs) {
        double z[2];
        mh_normal_pair(zin ? zin + ((int64_t)t * C + c) * ld_z : nullptr, d, q, nkey, chain_offset + c, z);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          if (2 * q + e >= d) break;
          const double v = av[p][e];
          const double pv = fma(kappa, v, z[e]);
          const double rv = fma(-kappa, pv, v);
          ap[p][e] = pv;
          s0 = fma(v, v, s0);
          s1 = fma(pv, pv, s1);
          s2 = fma(rv, rv, s2);
          s3 = fma(z[e], z[e], s3);
        }
      }
    }
    // the step's uniform and its logarithm depend on nothing of the step: formed in front of the barrier, in the shadow of the
    // slowest wave's sums
    const double log_u = log(omc_chain_uniform(u_in, (int64_t)t * C + c,
                                               omc_make_key(seed, draw_index0 + (uint64_t)t * draw_stride, OMC_RNG_UNIFORM),
                                               chain_offset + c, 0u));
    double(*rd)[4] = red[t & 1];  // two buffers: a wave that is a step ahead never writes what a slower one still reads
    mh_block_partials(rd, s0, s1, s2, s3);
    __syncthreads();
    // every thread forms the decision: no second barrier, no broadcast
    const MhDecision dec = mh_odds(rd, true, tgt).decide(log_u);
    const bool ok = dec.ok;
    lp_state = dec.lp;
    n_acc += ok;
    if (ok) {
#pragma unroll
      for (int p = 0; p < NP; ++p) { av[p][0] = ap[p][0]; av[p][1] = ap[p][1]; }
    }
    if (a_traj) {
      double* row = a_traj + ((int64_t)t * C + c) * d;
#pragma unroll
      for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int64_t i = 2 * ((int64_t)tid + 256 * p) + e;
          if (i < d) row[i] = av[p][e];
        }
    }
    if (tid == 0 && logp_traj) logp_traj[(int64_t)t * C + c] = lp_state;
  }
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int64_t i = 2 * ((int64_t)tid + 256 * p) + e;
      if (i < d) a[c * d + i] = av[p][e];
    }
  if (tid == 0) {
    if (prop_cnt) prop_cnt[c] += n_steps;
    if (acc_cnt) acc_cnt[c] += n_acc;
    if (logp_last && n_steps > 0) logp_last[c] = lp_state;
  }
}

extern "C" {

omc_status omc_dense_cholesky(omc_ctx* ctx, int64_t d, const double* A, double scale, double* L_out,
                              double* sumlogdiag_out) {
  if (!ctx || d < 1 || d > 32768 || !A || !L_out || !(scale > 0.0)) return OMC_INVALID_ARG;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  omc_status st = omc_ensure_blas(ctx);
  if (st != OMC_OK) return st;
  st = omc_ensure(ctx, ctx->dense_info, sizeof(int) * (size_t)(ctx->n_chains > 1 ? ctx->n_chains : 1));
  if (st != OMC_OK) return st;
  hipLaunchKernelGGL(k_scale_copy, dim3(gx(d * d)), dim3(256), 0, ctx->stream, d * d, A, scale, L_out);
  OMC_HIP_CHECK(hipGetLastError());
  OMC_BLAS_CHECK(rocsolver_dpotrf((rocblas_handle)ctx->blas, rocblas_fill_lower, (rocblas_int)d, L_out, (rocblas_int)d,
                                  ctx->dense_info));
  hipLaunchKernelGGL(k_latch_info, dim3(1), dim3(1), 0, ctx->stream, ctx->dense_info, ctx->d_bad_chain);
  if (sumlogdiag_out) hipLaunchKernelGGL(k_sumlogdiag, dim3(1), dim3(256), 0, ctx->stream, d, L_out, sumlogdiag_out);
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}

// Shared constant Hessian: the drift matrix A1 = -(L L')^{-1} Q (one potrs), A1p = I + A1/2 and the explicit
// L^{-T} (one trsm on the identity) are formed once per (Q, L, step) and cached in the context.  The proposal mean
// is then m(x) = A1p x + c0, and a step is 3 GEMMs (x' = A1p x + L^{-T} z accumulated in place, m' = A1p x'),
// one TRMM for the three quadratic forms that need L' (the fourth, |L'(x' - m)|^2, is |z|^2), and three small
// kernels (draw, build, finish) -- 7 launches instead of the first version's 23 (2 GEMMs + 5 TRSMs + 4 TRMMs;
// TRSM with 512 right-hand sides is ~10x slower than the GEMM of the same shape).
__global__ void k_set_identity(int64_t d, double* A) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d * d; i += (int64_t)gridDim.x * blockDim.x)
    A[i] = (i / d == i % d) ? 1.0 : 0.0;
}
// A1p = I + 0.5 * A1  (the proposal mean of a chain is then ONE matrix product: m = A1p x + c0, c0 = -0.5 A1 mu)
__global__ void k_half_plus_identity(int64_t d, const double* A1, double* out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d * d; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = 0.5 * A1[i] + ((i / d == i % d) ? 1.0 : 0.0);
}
// a[c][:] += v
__global__ void k_add_shared(int64_t d, double* a, int64_t ld_a, const double* v) {
  const int64_t c = blockIdx.y;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d; i += (int64_t)gridDim.x * blockDim.x)
    a[c * ld_a + i] += v[i];
}
// T3 columns: [ x - mu | x' - mu | x - m' ]  with m' = mp + c0 (each block d x C)
__global__ void k_build_t3(int64_t d, int64_t C, const double* x, int64_t ld_x, const double* mu, const double* c0,
                           const double* xp, const double* mp, double* t3) {
  const int64_t c = blockIdx.y;
  const int64_t blk = C * d;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d; i += (int64_t)gridDim.x * blockDim.x) {
    const double xv = x[c * ld_x + i], pv = xp[c * d + i], mv = mu ? mu[i] : 0.0;
    t3[c * d + i] = xv - mv;
    t3[blk + c * d + i] = pv - mv;
    t3[2 * blk + c * d + i] = xv - (mp[c * d + i] + (c0 ? c0[i] : 0.0));
  }
}
// random walk: x' = x + step * z (mh_rw_move), T2 = [ x - mu | x' - mu ]
__global__ void k_rw_build(int64_t d, int64_t C, const double* x, int64_t ld_x, const double* mu, double step,
                           const double* z, double* xp, double* t2) {
  const int64_t c = blockIdx.y;
  const int64_t blk = C * d;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d; i += (int64_t)gridDim.x * blockDim.x) {
    const double xv = x[c * ld_x + i], mv = mu ? mu[i] : 0.0;
    const double pv = mh_rw_move(xv, z[c * d + i], step);
    xp[c * d + i] = pv;
    t2[c * d + i] = xv - mv;
    t2[blk + c * d + i] = pv - mv;
  }
}
// One workgroup per chain: the squared norms the decision needs, the decision, and the move of the accepted
// proposal into the state (metropolis_hastings.py:127-173).  n_cur / n_prop / n_rev: columns of L'(.) (n_rev and z
// NULL for the symmetric random walk); z: the proposal's N(0, I) draw, |z|^2 = |L'(x' - m)|^2.
__global__ void __launch_bounds__(256) k_mh_finish(int64_t d, int64_t chain_offset, omc_rng_key key, const double* u_in,
                                                   const double* sumlogL, double log_step_term, double lp_scale,
                                                   const double* n_cur, const double* n_prop, const double* n_rev,
                                                   const double* z, const double* xp, double* x, int64_t ld_x,
                                                   long long* acc_cnt, long long* prop_cnt) {
  __shared__ double red[4][4];
  __shared__ int accept;
  const int64_t c = blockIdx.x;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int64_t i = threadIdx.x; i < d; i += 256) {
    const double v0 = n_cur[c * d + i], v1 = n_prop[c * d + i];
    s0 = fma(v0, v0, s0);
    s1 = fma(v1, v1, s1);
    if (n_rev) {
      const double v2 = n_rev[c * d + i], v3 = z[c * d + i];
      s2 = fma(v2, v2, s2);
      s3 = fma(v3, v3, s3);
    }
  }
  mh_block_partials(red, s0, s1, s2, s3);
  __syncthreads();
  if (threadIdx.x == 0) {
    const MhTarget tgt = mh_target(sumlogL[0], log_step_term, d, lp_scale);
    const MhDecision dec = mh_odds(red, n_rev != nullptr, tgt).decide(log(omc_chain_uniform(u_in, c, key, chain_offset + c, 0u)));
    accept = dec.ok;
    mh_count(acc_cnt, prop_cnt, c, dec.ok);
  }
  __syncthreads();
  if (accept)
    for (int64_t i = threadIdx.x; i < d; i += 256) x[c * ld_x + i] = xp[c * d + i];
}

// lower triangle of a column-major d x d matrix, zeros above the diagonal: the triangular products below run as
// plain GEMMs on this image (rocBLAS's out-of-place TRMM reached 5.6 TFLOP/s at d = 500, its DGEMM 37)
// (grid-stride like every kernel launched with gx(), which caps the grid at 4096 blocks: as plain one-element-per-thread
//  kernels these two left everything beyond 2^20 elements -- d > 1024 -- unwritten)
__global__ void k_lower_copy(int64_t d, const double* L, double* out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d * d; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t col = i / d, row = i - col * d;
    out[i] = row >= col ? L[i] : 0.0;
  }
}

// U = L' as a dense upper-triangular column-major matrix (zeros below the diagonal): the own GEMM takes A as it stands
__global__ void k_lower_transpose(int64_t d, const double* L, double* out) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < d * d; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = e / d, i = e - k * d;  // out(i, k) = L(k, i) for k >= i
    out[e] = k >= i ? L[i * d + k] : 0.0;
  }
}
// both images of a factor, one behind the other: pair = [ L, zeros above | L', zeros below ]
static void lower_pair(omc_ctx* ctx, int64_t d, const double* L, double* pair) {
  hipLaunchKernelGGL(k_lower_copy, dim3(gx(d * d)), dim3(256), 0, ctx->stream, d, L, pair);
  hipLaunchKernelGGL(k_lower_transpose, dim3(gx(d * d)), dim3(256), 0, ctx->stream, d, L, pair + d * d);
}
// N = L' T (T, N: d x ncols, ld = d) from such a pair: the own GEMM on L', or rocBLAS on the zero-padded L
static omc_status lt_product(omc_ctx* ctx, int64_t d, int64_t ncols, const double* pair, const double* T, double* N) {
  if (mh_own_gemm(ctx, d))
    return omc_dgemm_small(ctx, (int)d, (int)ncols, pair + d * d, d, T, d, (int)d, nullptr, 0, nullptr, 0, 0, 1, nullptr, N, d);
  const double one = 1.0, zero = 0.0;
  const rocblas_int di = (rocblas_int)d;
  OMC_BLAS_CHECK(rocblas_dgemm((rocblas_handle)ctx->blas, rocblas_operation_transpose, rocblas_operation_none, di, (rocblas_int)ncols,
                               di, &one, pair, di, T, di, &zero, N, di));
  return OMC_OK;
}
// Z (ld = d) = the step's N(0, I) draw of every chain
static void draw_normals(omc_ctx* ctx, int64_t d, uint64_t draw_index, const double* z_inject, int64_t ld_z, double* Z) {
  const unsigned g = gx((d + 1) / 2);
  hipLaunchKernelGGL(k_draw_normals, dim3(g > 8 ? 8 : g, (unsigned)ctx->n_chains), dim3(256), 0, ctx->stream, d, ctx->chain_offset,
                     omc_make_key(ctx->seed, draw_index, OMC_RNG_NORMAL), z_inject, ld_z, Z, d);
}

static omc_status mala_prepare(omc_ctx* ctx, int64_t d, const double* Q, const double* L, double step) {
  auto& m = ctx->mala;
  if (m.Q == Q && m.L == L && m.step == step && m.d == d && m.prep) return OMC_OK;
  omc_status st = omc_ensure(ctx, m.prep, (size_t)5 * d * d * sizeof(double));
  if (st != OMC_OK) return st;
  rocblas_handle h = (rocblas_handle)ctx->blas;
  const rocblas_int di = (rocblas_int)d;
  double* A1 = m.prep;                // -(L L')^{-1} Q
  double* LinvT = m.prep + d * d;     // L^{-T}
  double* pair = m.prep + 2 * d * d;  // lower_pair(L): the zero-padded L for potrs, and both forms of the product L'T
  hipLaunchKernelGGL(k_scale_copy, dim3(gx(d * d)), dim3(256), 0, ctx->stream, d * d, Q, -1.0, A1);
  lower_pair(ctx, d, L, pair);
  OMC_BLAS_CHECK(rocsolver_dpotrs(h, rocblas_fill_lower, di, di, pair, di, A1, di));
  hipLaunchKernelGGL(k_set_identity, dim3(gx(d * d)), dim3(256), 0, ctx->stream, d, LinvT);
  const double one = 1.0;
  OMC_BLAS_CHECK(rocblas_dtrsm(h, rocblas_side_left, rocblas_fill_lower, rocblas_operation_transpose,
                               rocblas_diagonal_non_unit, di, di, &one, L, di, LinvT, di));
  hipLaunchKernelGGL(k_half_plus_identity, dim3(gx(d * d)), dim3(256), 0, ctx->stream, d, A1, m.prep + 4 * d * d);
  OMC_HIP_CHECK(hipGetLastError());
  m.Q = Q; m.L = L; m.step = step; m.d = d;
  return OMC_OK;
}

omc_status omc_mh_invalidate(omc_ctx* ctx) {
  if (!ctx) return OMC_INVALID_ARG;
  ctx->mala.reset(); ctx->white.reset(); ctx->rww.reset(); ctx->rw.reset();
  return OMC_OK;
}

omc_status omc_mala_step(omc_ctx* ctx, int64_t d, const double* Q, const double* mu, const double* L,
                         const double* sumlogL, double step, const double* z_inject, int64_t ld_z,
                         const double* u_inject, uint64_t draw_index, double* x, int64_t ld_x, int64_t* accept_count,
                         int64_t* proposal_count) {
  if (!ctx || d < 1 || !Q || !L || !sumlogL || !x || ld_x < d || (z_inject && ld_z < d) || !(step > 0.0))
    return OMC_INVALID_ARG;
  MhWork w{};
  omc_status st = mh_enter(ctx, d, &w);
  if (st != OMC_OK) return st;
  st = mala_prepare(ctx, d, Q, L, step);
  if (st != OMC_OK) return st;
  const int64_t C = ctx->n_chains;
  const double* A1 = ctx->mala.prep;
  const double* LinvT = ctx->mala.prep + d * d;
  const double* pair = ctx->mala.prep + 2 * d * d;  // lower_pair(L)
  const double* A1p = ctx->mala.prep + 4 * d * d;   // I + A1/2
  rocblas_handle h = (rocblas_handle)ctx->blas;
  const rocblas_int di = (rocblas_int)d, Ci = (rocblas_int)C;
  const double one = 1.0, zero = 0.0, minus_half = -0.5;
  const dim3 g2(gx(d) > 8 ? 8 : gx(d), (unsigned)C), b2(256);
  hipStream_t s = ctx->stream;
  // workspace roles: Z (draw), XP (proposal x'), V (A1p x'), T3 = [x-mu | x'-mu | x-m'] and its image under L'
  double* Z = w.R;
  double* T3 = w.T;
  double* N3 = w.T + 3 * C * d;
  double* c0 = nullptr;
  if (mu) {  // c0 = -1/2 A1 mu: the constant part of the proposal mean m(x) = A1p x + c0
    c0 = w.G;
    OMC_BLAS_CHECK(rocblas_dgemv(h, rocblas_operation_none, di, di, &minus_half, A1, di, mu, 1, &zero, c0, 1));
  }
  // proposal: x' = m(x) + L^{-T} z = A1p x + L^{-T} z (+ c0): two GEMMs into the same buffer, no element-wise pass
  draw_normals(ctx, d, draw_index, z_inject, ld_z, Z);
  if (mh_own_gemm(ctx, d)) {  // one launch: x' = A1p x + L^-T z + c0
    st = omc_dgemm_small(ctx, (int)d, (int)C, A1p, d, x, ld_x, (int)d, LinvT, d, Z, d, (int)d, 0, c0, w.XP, d);
    if (st != OMC_OK) return st;
    st = omc_dgemm_small(ctx, (int)d, (int)C, A1p, d, w.XP, d, (int)d, nullptr, 0, nullptr, 0, 0, 0, nullptr, w.V, d);
    if (st != OMC_OK) return st;
  } else {
    OMC_BLAS_CHECK(rocblas_dgemm(h, rocblas_operation_none, rocblas_operation_none, di, Ci, di, &one, A1p, di, x,
                                 (rocblas_int)ld_x, &zero, w.XP, di));
    OMC_BLAS_CHECK(rocblas_dgemm(h, rocblas_operation_none, rocblas_operation_none, di, Ci, di, &one, LinvT, di, Z, di, &one,
                                 w.XP, di));
    if (c0) hipLaunchKernelGGL(k_add_shared, g2, b2, 0, s, d, w.XP, d, c0);
    // proposed state's mean: m' = A1p x' (+ c0, added when T3 is built)
    OMC_BLAS_CHECK(rocblas_dgemm(h, rocblas_operation_none, rocblas_operation_none, di, Ci, di, &one, A1p, di, w.XP, di, &zero,
                                 w.V, di));
  }
  // |L'(x - mu)|^2, |L'(x' - mu)|^2, |L'(x - m')|^2 in one product; |L'(x' - m)|^2 = |z|^2 needs none
  hipLaunchKernelGGL(k_build_t3, g2, b2, 0, s, d, C, x, ld_x, mu, c0, w.XP, w.V, T3);
  st = lt_product(ctx, d, 3 * C, pair, T3, N3);
  if (st != OMC_OK) return st;
  // accept / reject and the move of accepted proposals.  L = chol(Q / step^2) => chol(Q) = step * L
  hipLaunchKernelGGL(k_mh_finish, dim3((unsigned)C), dim3(256), 0, s, d, ctx->chain_offset,
                     omc_make_key(ctx->seed, draw_index, OMC_RNG_UNIFORM), u_inject, sumlogL, (double)d * log(step),
                     step * step, N3, N3 + C * d, N3 + 2 * C * d, Z, w.XP, x, ld_x, (long long*)accept_count,
                     (long long*)proposal_count);
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}

// ---- the same step in whitened coordinates ---------------------------------------------------------------------
// With L = chol(Q / step^2) the drift matrix of the step above is a multiple of the identity: -(L L')^{-1} Q = -step^2 I,
// m(x) = x - (step^2 / 2)(x - mu).  In a = L'(x - mu) the whole step is element-wise:
//   a' = kappa a + z,  kappa = 1 - step^2 / 2                      (proposal: x' = m(x) + L^{-T} z)
//   |L'(x - mu)|^2 = |a|^2,  |L'(x' - mu)|^2 = |a'|^2              (log p of both states)
//   |L'(x' - m(x))|^2 = |z|^2,  |L'(x - m(x'))|^2 = |a - kappa a'|^2   (log q forward and reverse)
// and only the accepted proposals have to come back to x = mu + L^{-T} a': ONE triangular product per step (plus one
// for a = L'(x - mu) whenever the caller's x is not the one this routine left behind), against the three full and one
// triangular product of omc_mala_step -- 2 d^2 instead of 9 d^2 flop per chain.  Same draws, same decision rule; the
// numbers differ from omc_mala_step's by the rounding of different (shorter) sums.
__global__ void __launch_bounds__(256) k_mala_white(int64_t d, int64_t chain_offset, omc_rng_key nkey, omc_rng_key ukey,
                                                    const double* zin, int64_t ld_z, const double* u_in, const double* sumlogL,
                                                    double log_step_term, double lp_scale, double kappa, double* a,
                                                    double* a_prop, int* accept_out, long long* acc_cnt, long long* prop_cnt,
                                                    double* logp_out) {
  __shared__ double red[4][4];
  __shared__ int accept;
  const int64_t c = blockIdx.x;
  const int64_t npairs = (d + 1) / 2;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;  // |a|^2, |a'|^2, |a - kappa a'|^2, |z|^2: the rows mh_decide reads
  for (int64_t q = threadIdx.x; q < npairs; q += 256) {
    double z[2];
    mh_normal_pair(zin ? zin + c * ld_z : nullptr, d, q, nkey, chain_offset + c, z);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int64_t i = 2 * q + e;
      if (i >= d) break;
      const double av = a[c * d + i];
      const double ap = fma(kappa, av, z[e]);
      const double rv = fma(-kappa, ap, av);
      a_prop[c * d + i] = ap;
      s0 = fma(av, av, s0);
      s1 = fma(ap, ap, s1);
      s2 = fma(rv, rv, s2);
      s3 = fma(z[e], z[e], s3);
    }
  }
  mh_block_partials(red, s0, s1, s2, s3);
  __syncthreads();
  if (threadIdx.x == 0) {
    const MhTarget tgt = mh_target(sumlogL[0], log_step_term, d, lp_scale);
    const double log_u = log(omc_chain_uniform(u_in, c, ukey, chain_offset + c, 0u));
    const MhDecision dec = mh_odds(red, true, tgt).decide(log_u);
    accept = dec.ok;
    if (logp_out) logp_out[c] = dec.lp;
    accept_out[c] = dec.ok;
    mh_count(acc_cnt, prop_cnt, c, dec.ok);
  }
  __syncthreads();
  if (accept)
    for (int64_t i = threadIdx.x; i < d; i += 256) a[c * d + i] = a_prop[c * d + i];
}

static omc_status white_prepare(omc_ctx* ctx, int64_t d, const double* L, const double* mu) {
  auto& wh = ctx->white;
  if (wh.L == L && wh.mu == mu && wh.d == d && wh.prep) return OMC_OK;
  omc_status st = omc_ensure(ctx, wh.prep, (size_t)(2 * d * d + 2 * d) * sizeof(double));
  if (st != OMC_OK) return st;
  rocblas_handle h = (rocblas_handle)ctx->blas;
  const rocblas_int di = (rocblas_int)d;
  double* LinvT = wh.prep;          // L^{-T}, upper triangular
  double* Lt = wh.prep + d * d;     // L', upper triangular
  double* negLtmu = wh.prep + 2 * d * d;  // -L' mu
  double* negmu = negLtmu + d;
  hipLaunchKernelGGL(k_set_identity, dim3(gx(d * d)), dim3(256), 0, ctx->stream, d, LinvT);
  const double one = 1.0;
  OMC_BLAS_CHECK(rocblas_dtrsm(h, rocblas_side_left, rocblas_fill_lower, rocblas_operation_transpose,
                               rocblas_diagonal_non_unit, di, di, &one, L, di, LinvT, di));
  hipLaunchKernelGGL(k_lower_transpose, dim3(gx(d * d)), dim3(256), 0, ctx->stream, d, L, Lt);
  if (mu) {
    hipLaunchKernelGGL(k_scale_copy, dim3(gx(d)), dim3(256), 0, ctx->stream, d, mu, -1.0, negmu);
    st = omc_dgemm_small(ctx, (int)d, 1, Lt, d, negmu, d, (int)d, nullptr, 0, nullptr, 0, 0, 1, nullptr, negLtmu, d);
    if (st != OMC_OK) return st;
  }
  OMC_HIP_CHECK(hipGetLastError());
  wh.L = L; wh.mu = mu; wh.d = d; wh.x = nullptr;
  return OMC_OK;
}

// a = L'(x - mu) of the caller's state, in ctx->white.a: one product, unless x is what the last whitened step left there and the
// caller vouches that nobody has written it since.  After white_prepare.
static omc_status white_state(omc_ctx* ctx, int64_t d, const double* mu, const double* x, int64_t ld_x, int32_t state_is_current,
                              double** a) {
  auto& wh = ctx->white;
  const int64_t C = ctx->n_chains;
  omc_status st = omc_ensure(ctx, wh.a, (size_t)C * d * sizeof(double));
  if (st != OMC_OK) return st;
  *a = wh.a;
  if (state_is_current && wh.x == x && wh.ld == ld_x) return OMC_OK;
  const double* Lt = wh.prep + d * d;
  const double* negLtmu = mu ? wh.prep + 2 * d * d : nullptr;  // a = L'x - L'mu
  return omc_dgemm_small(ctx, (int)d, (int)C, Lt, d, x, ld_x, (int)d, nullptr, 0, nullptr, 0, 0, 1, negLtmu, *a, d);
}

omc_status omc_mala_step_white(omc_ctx* ctx, int64_t d, const double* mu, const double* L, const double* sumlogL, double step,
                               const double* z_inject, int64_t ld_z, const double* u_inject, uint64_t draw_index, double* x,
                               int64_t ld_x, int32_t state_is_current, int64_t* accept_count, int64_t* proposal_count, double* log_p_out) {
  if (!ctx || d < 1 || d > 46340 || !L || !sumlogL || !x || ld_x < d || (z_inject && ld_z < d) || !(step > 0.0))
    return OMC_INVALID_ARG;
  MhWork w{};
  omc_status st = mh_enter(ctx, d, &w);
  if (st != OMC_OK) return st;
  st = white_prepare(ctx, d, L, mu);
  if (st != OMC_OK) return st;
  double* a;
  st = white_state(ctx, d, mu, x, ld_x, state_is_current, &a);
  if (st != OMC_OK) return st;
  const int64_t C = ctx->n_chains;
  const double* LinvT = ctx->white.prep;
  hipLaunchKernelGGL(k_mala_white, dim3((unsigned)C), dim3(256), 0, ctx->stream, d, ctx->chain_offset,
                     omc_make_key(ctx->seed, draw_index, OMC_RNG_NORMAL), omc_make_key(ctx->seed, draw_index, OMC_RNG_UNIFORM),
                     z_inject, ld_z, u_inject, sumlogL, (double)d * log(step), step * step, 1.0 - 0.5 * step * step, a, w.XP,
                     w.flag, (long long*)accept_count, (long long*)proposal_count, log_p_out);
  OMC_HIP_CHECK(hipGetLastError());
  // x = mu + L^{-T} a on the chains that accepted (the others keep their x bit for bit)
  st = omc_dgemm_small(ctx, (int)d, (int)C, LinvT, d, a, d, (int)d, nullptr, 0, nullptr, 0, 0, 1, mu, x, ld_x, w.flag);
  if (st != OMC_OK) return st;
  ctx->white.x = x; ctx->white.ld = ld_x;
  return OMC_OK;
}

#define OMC_WHITE_RUN_BLOCK 32  // steps per launch (the whitened trajectory of a block: 32 x C x d doubles of workspace)

omc_status omc_mala_run_white(omc_ctx* ctx, int64_t d, const double* mu, const double* L, const double* sumlogL, double step,
                              const double* z_inject, int64_t ld_z, const double* u_inject, uint64_t draw_index0, uint64_t draw_stride,
                              int64_t n_steps, double* x, int64_t ld_x, int32_t state_is_current, double* x_store, double* logp_store,
                              int64_t* accept_count, int64_t* proposal_count, double* log_p_out) {
  if (!ctx || d < 1 || d > 2048 || !L || !sumlogL || !x || ld_x < d || (z_inject && ld_z < d) || !(step > 0.0) || n_steps < 0)
    return d > 2048 ? OMC_UNSUPPORTED : OMC_INVALID_ARG;
  omc_status st = mh_enter(ctx, d, nullptr);
  if (st != OMC_OK) return st;
  st = white_prepare(ctx, d, L, mu);
  if (st != OMC_OK) return st;
  const int64_t C = ctx->n_chains;
  const int64_t KB = OMC_WHITE_RUN_BLOCK;
  if (x_store) {
    // two trajectory buffers: the product of block b runs on the side stream while the steps of block b + 1 run here
    st = omc_ensure(ctx, ctx->white.traj, (size_t)2 * KB * C * d * sizeof(double));
    if (st != OMC_OK) return st;
    st = omc_ensure_aux(ctx);
    if (st != OMC_OK) return st;
    for (int i = 0; i < 4; ++i)
      if (!ctx->white.ev[i]) OMC_HIP_CHECK(hipEventCreateWithFlags(&ctx->white.ev[i], hipEventDisableTiming));
  }
  const double* LinvT = ctx->white.prep;
  double* a;
  st = white_state(ctx, d, mu, x, ld_x, state_is_current, &a);
  if (st != OMC_OK) return st;
  const int np = (int)(((d + 1) / 2 + 255) / 256);
  int64_t blk = 0;
  for (int64_t t0 = 0; t0 < n_steps; t0 += KB, ++blk) {
    const int nb = (int)((n_steps - t0 < KB) ? n_steps - t0 : KB);
    const int buf = (int)(blk & 1);
    double* traj = x_store ? ctx->white.traj + (size_t)buf * KB * C * d : nullptr;
    if (x_store && blk >= 2) OMC_HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->white.ev[2 + buf], 0));  // block b - 2's product has read this buffer
#define OMC_WRUN(NP)                                                                                                                   \
  hipLaunchKernelGGL((k_mala_white_run<NP>), dim3((unsigned)C), dim3(256), 0, ctx->stream, d, C, ctx->chain_offset, ctx->seed,         \
                     draw_index0 + (uint64_t)t0 * draw_stride, draw_stride, nb, z_inject ? z_inject + t0 * C * ld_z : nullptr, ld_z,   \
                     u_inject ? u_inject + t0 * C : nullptr, sumlogL, (double)d * log(step), step * step, 1.0 - 0.5 * step * step, a,    \
                     traj, (long long*)accept_count, (long long*)proposal_count, logp_store ? logp_store + t0 * C : nullptr, log_p_out)
    if (np <= 1) OMC_WRUN(1); else if (np == 2) OMC_WRUN(2); else OMC_WRUN(4);
#undef OMC_WRUN
    OMC_HIP_CHECK(hipGetLastError());
    if (x_store) {  // x_t = mu + L^-T a_t for the whole block, into the store slabs [t][c][:] -- on the side stream
      OMC_HIP_CHECK(hipEventRecord(ctx->white.ev[buf], ctx->stream));
      OMC_HIP_CHECK(hipStreamWaitEvent(ctx->aux_stream, ctx->white.ev[buf], 0));
      hipStream_t mine = ctx->stream;
      ctx->stream = ctx->aux_stream;  // (omc_dgemm_small launches on the context's stream)
      // (a few thousand columns and more: 64 x 64 tiles; below that the step's own small-tile kernel, bit for bit what the
      //  single steps compute)
      if (nb * C >= 4096 && !ctx->mh_use_rocblas)
        st = omc_dgemm_wide(ctx, (int)d, (int)(nb * C), LinvT, d, traj, d, (int)d, 1, mu, x_store + t0 * C * d, d);
      else
        st = omc_dgemm_small(ctx, (int)d, (int)(nb * C), LinvT, d, traj, d, (int)d, nullptr, 0, nullptr, 0, 0, 1, mu, x_store + t0 * C * d, d);
      ctx->stream = mine;
      if (st != OMC_OK) return st;
      OMC_HIP_CHECK(hipEventRecord(ctx->white.ev[2 + buf], ctx->aux_stream));
    }
  }
  if (x_store) {  // join: everything behind this call on the context's stream sees the whole store
    for (int i = 0; i < 2 && i < blk; ++i) OMC_HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->white.ev[2 + ((blk - 1 - i) & 1)], 0));
  }
  if (n_steps > 0) {
    if (x_store) {  // the state the run leaves is its last stored one
      OMC_HIP_CHECK(hipMemcpy2DAsync(x, (size_t)ld_x * sizeof(double), x_store + (n_steps - 1) * C * d, (size_t)d * sizeof(double),
                                     (size_t)d * sizeof(double), (size_t)C, hipMemcpyDeviceToDevice, ctx->stream));
    } else {
      st = omc_dgemm_small(ctx, (int)d, (int)C, LinvT, d, a, d, (int)d, nullptr, 0, nullptr, 0, 0, 1, mu, x, ld_x);
      if (st != OMC_OK) return st;
    }
  }
  ctx->white.x = x; ctx->white.ld = ld_x;
  return OMC_OK;
}

// lower_pair(LQ) in ctx->rw.prep, once per (LQ, d); *fresh (if asked for) is set when it had to be made
static omc_status rw_prepare(omc_ctx* ctx, int64_t d, const double* LQ, bool* fresh) {
  auto& rw = ctx->rw;
  if (rw.LQ == LQ && rw.d == d && rw.prep) return OMC_OK;
  omc_status st = omc_ensure(ctx, rw.prep, (size_t)2 * d * d * sizeof(double));
  if (st != OMC_OK) return st;
  lower_pair(ctx, d, LQ, rw.prep);
  rw.LQ = LQ; rw.d = d;
  if (fresh) *fresh = true;
  return OMC_OK;
}

omc_status omc_rw_step(omc_ctx* ctx, int64_t d, const double* mu, const double* LQ, const double* sumlogLQ, double step,
                       const double* z_inject, int64_t ld_z, const double* u_inject, uint64_t draw_index, double* x,
                       int64_t ld_x, int64_t* accept_count, int64_t* proposal_count) {
  if (!ctx || d < 1 || !LQ || !sumlogLQ || !x || ld_x < d || (z_inject && ld_z < d) || !(step > 0.0))
    return OMC_INVALID_ARG;
  MhWork w{};
  omc_status st = mh_enter(ctx, d, &w);
  if (st != OMC_OK) return st;
  const int64_t C = ctx->n_chains;
  const dim3 g2(gx(d) > 8 ? 8 : gx(d), (unsigned)C), b2(256);
  hipStream_t s = ctx->stream;
  double* Z = w.V;
  double* T2 = w.T;
  double* N2 = w.T + 2 * C * d;
  draw_normals(ctx, d, draw_index, z_inject, ld_z, Z);
  hipLaunchKernelGGL(k_rw_build, g2, b2, 0, s, d, C, x, ld_x, mu, step, Z, w.XP, T2);  // :250
  st = rw_prepare(ctx, d, LQ, nullptr);
  if (st != OMC_OK) return st;
  st = lt_product(ctx, d, 2 * C, ctx->rw.prep, T2, N2);
  if (st != OMC_OK) return st;
  hipLaunchKernelGGL(k_mh_finish, dim3((unsigned)C), dim3(256), 0, s, d, ctx->chain_offset,
                     omc_make_key(ctx->seed, draw_index, OMC_RNG_UNIFORM), u_inject, sumlogLQ, 0.0, 1.0, N2, N2 + C * d,
                     (const double*)nullptr, (const double*)nullptr, w.XP, x, ld_x, (long long*)accept_count,
                     (long long*)proposal_count);
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}

// ---- the random-walk step with the target's quadratic form carried in whitened coordinates -----------------------
// a = L_Q'(x - mu) (L_Q = chol(Q)):  x' = x + step z  =>  a' = a + step L_Q' z, log p(x') - log p(x) = (|a|^2 - |a'|^2) / 2.
// One triangular product per step (L_Q' z) instead of the two of omc_rw_step (L_Q'[x - mu | x' - mu]); x' itself is the
// same two-rounding x + step z as there, so for equal decisions the states are bit-identical.
__global__ void __launch_bounds__(256) k_rw_white(int64_t d, int64_t chain_offset, omc_rng_key ukey, const double* u_in,
                                                  const double* sumlogL, double step, const double* z, const double* wz,
                                                  double* a, double* x, int64_t ld_x, long long* acc_cnt, long long* prop_cnt,
                                                  double* logp_out) {
  __shared__ double red[2][4];
  __shared__ int accept;
  const int64_t c = blockIdx.x;
  double s0 = 0.0, s1 = 0.0;
  for (int64_t i = threadIdx.x; i < d; i += 256) {
    const double av = a[c * d + i];
    const double ap = fma(step, wz[c * d + i], av);
    s0 = fma(av, av, s0);
    s1 = fma(ap, ap, s1);
  }
  mh_block_partials(red, s0, s1);
  __syncthreads();
  if (threadIdx.x == 0) {
    const double sl = sumlogL[0];
    const MhTarget tgt{sl, 2.0 * sl, (double)d, 1.0};  // the factor is chol(Q) itself: no step term, no scale
    const MhDecision dec = mh_odds(red, false, tgt).decide(log(omc_chain_uniform(u_in, c, ukey, chain_offset + c, 0u)));
    accept = dec.ok;
    if (logp_out) logp_out[c] = dec.lp;
    mh_count(acc_cnt, prop_cnt, c, dec.ok);
  }
  __syncthreads();
  if (accept)
    for (int64_t i = threadIdx.x; i < d; i += 256) {
      a[c * d + i] = fma(step, wz[c * d + i], a[c * d + i]);
      x[c * ld_x + i] = mh_rw_move(x[c * ld_x + i], z[c * d + i], step);
    }
}

omc_status omc_rw_step_white(omc_ctx* ctx, int64_t d, const double* mu, const double* LQ, const double* sumlogLQ, double step,
                             const double* z_inject, int64_t ld_z, const double* u_inject, uint64_t draw_index, double* x,
                             int64_t ld_x, int32_t state_is_current, int64_t* accept_count, int64_t* proposal_count, double* log_p_out) {
  if (!ctx || d < 1 || d > 46340 || !LQ || !sumlogLQ || !x || ld_x < d || (z_inject && ld_z < d) || !(step > 0.0))
    return OMC_INVALID_ARG;
  MhWork w{};
  omc_status st = mh_enter(ctx, d, &w);
  if (st != OMC_OK) return st;
  const int64_t C = ctx->n_chains;
  hipStream_t s = ctx->stream;
  auto& rww = ctx->rww;
  bool fresh = false;
  st = rw_prepare(ctx, d, LQ, &fresh);
  if (st != OMC_OK) return st;
  const double* Lt = ctx->rw.prep + d * d;
  st = omc_ensure(ctx, rww.mu_neg, (size_t)2 * d * sizeof(double));
  if (st != OMC_OK) return st;
  double* negLtmu = nullptr;
  if (mu) {  // -L_Q' mu, once per (L_Q, mu)
    negLtmu = rww.mu_neg;
    if (fresh || rww.mu != mu) {
      hipLaunchKernelGGL(k_scale_copy, dim3(gx(d)), dim3(256), 0, s, d, mu, -1.0, rww.mu_neg + d);
      st = omc_dgemm_small(ctx, (int)d, 1, Lt, d, rww.mu_neg + d, d, (int)d, nullptr, 0, nullptr, 0, 0, 1, nullptr, negLtmu, d);
      if (st != OMC_OK) return st;
      fresh = true;
    }
  }
  if (rww.mu != mu) fresh = true;
  rww.mu = mu;
  st = omc_ensure(ctx, rww.a, (size_t)C * d * sizeof(double));
  if (st != OMC_OK) return st;
  double* a = rww.a;
  if (fresh || !(state_is_current && rww.x == x && rww.ld == ld_x)) {  // a = L_Q'(x - mu)
    st = omc_dgemm_small(ctx, (int)d, (int)C, Lt, d, x, ld_x, (int)d, nullptr, 0, nullptr, 0, 0, 1, negLtmu, a, d);
    if (st != OMC_OK) return st;
  }
  double* Z = w.V;
  double* WZ = w.XP;
  draw_normals(ctx, d, draw_index, z_inject, ld_z, Z);
  st = omc_dgemm_small(ctx, (int)d, (int)C, Lt, d, Z, d, (int)d, nullptr, 0, nullptr, 0, 0, 1, nullptr, WZ, d);
  if (st != OMC_OK) return st;
  hipLaunchKernelGGL(k_rw_white, dim3((unsigned)C), dim3(256), 0, s, d, ctx->chain_offset,
                     omc_make_key(ctx->seed, draw_index, OMC_RNG_UNIFORM), u_inject, sumlogLQ, step, Z, WZ, a, x, ld_x,
                     (long long*)accept_count, (long long*)proposal_count, log_p_out);
  OMC_HIP_CHECK(hipGetLastError());
  rww.x = x; rww.ld = ld_x;
  return OMC_OK;
}

}  // extern "C"
