// LinearCombinationWithTransform (parameter.py:231-297): a regression term A exp(x) under a Gaussian likelihood.
//   omc_transform_predict     out[c] = alpha cs[c] (X exp(x_c)) + add_chain[c] + add_shared        (parameter.py:253-279)
//   omc_transform_grad_hess   grad = scale s o u,  H = scale (s s') o G,  s = exp(x)                (location_scale.py:234-242
//                             with parameter.py:281-297: the Gauss-Newton Hessian, no second-derivative term)
//   omc_mala_transform_step   one whole ManifoldMALA update (metropolis_hastings.py:127-173, 301-373) for that model on its
//                             p x p sufficient statistics, one launch for every chain.
#include <math.h>

#include "omc_common.h"

// ------------------------------------------------------------------------------------------------
// out[c][i] = alpha cs[c] sum_j X[i][j] exp(x[c][j]) + add_chain[c][i] + add_shared[i].  One thread per output row, the
// transformed vector staged in LDS a chunk at a time (it never goes to memory), the sum in index order.
#define TF_CHUNK 512
__global__ void __launch_bounds__(256) k_transform_predict(int64_t n, int64_t p, const double* X, int64_t ld_X, const double* x,
                                                           int64_t ld_x, const double* add_chain, int64_t ld_add,
                                                           const double* add_shared, double alpha, const double* chain_scale,
                                                           double* out, int64_t ld_out) {
  __shared__ double e[TF_CHUNK];
  const int64_t c = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const double* xc = x + c * ld_x;
  const double* row = X + (i < n ? i : 0) * ld_X;
  double s = 0.0;
  for (int64_t j0 = 0; j0 < p; j0 += TF_CHUNK) {
    const int m = (int)((p - j0 < TF_CHUNK) ? p - j0 : TF_CHUNK);
    __syncthreads();
    for (int j = threadIdx.x; j < m; j += blockDim.x) e[j] = exp(xc[j0 + j]);
    __syncthreads();
    if (i < n)
      for (int j = 0; j < m; ++j) s = fma(row[j0 + j], e[j], s);
  }
  if (i >= n) return;
  double v = alpha * s;
  if (chain_scale) v *= chain_scale[c];
  if (add_chain) v += add_chain[c * ld_add + i];
  if (add_shared) v += add_shared[i];
  out[c * ld_out + i] = v;
}

// grad[c][i] = scale[c] s_i u[c][i];  H[c][i][j] = scale[c] (s_i s_j) G[i][j]
__global__ void __launch_bounds__(256) k_transform_grad_hess(int64_t p, const double* x, int64_t ld_x, const double* u,
                                                             int64_t ld_u, const double* G, const double* scale, double* grad,
                                                             double* H) {
  const int64_t c = blockIdx.y;
  const double sc = scale ? scale[c] : 1.0;
  const double* xc = x + c * ld_x;
  const int64_t total = p * p;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / p, j = t - i * p;
    const double si = exp(xc[i]);
    if (H) H[c * total + t] = sc * ((si * exp(xc[j])) * G[t]);
    if (grad && u && j == 0) grad[c * p + i] = sc * (si * u[c * ld_u + i]);
  }
}

// ------------------------------------------------------------------------------------------------
// The fused step.  One wave per chain, lane i owns element i of every vector and row i of the matrix being factorised, which
// lives in the wave's own LDS tile (rows of odd stride ld = p | 1: the 32 lanes of a half-wave reading one column fall on 32
// different bank pairs).  G and P are read once per point, element (i, j) at [j * p + i] -- consecutive lanes, consecutive
// addresses -- and stay in the caches (64 KB together at p = 64).  Vector elements travel between lanes by v_readlane (the loop
// counters are wave-uniform).  The factorisation is left-looking: column j takes its whole update in one pass of loads with no
// store in between (so the loads run ahead of the multiply-adds), then every lane writes its entry of the column; the next
// column reads row j + 1 across lanes, hence a tf_wave_sync() per column.  The order of the subtractions per entry is that of the
// right-looking form of k_small_spd_ops / k_small_sample_canonical.
// LDS accesses of one wave complete in issue order; this keeps the compiler from moving them across the point where lanes start
// reading what other lanes wrote.
__device__ __forceinline__ void tf_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct TfPoint {
  double mu;      // proposal mean at this point, element `lane`
  double target;  // log target up to its constant (wave-uniform)
  double sumlog;  // sum log L_ii (wave-uniform)
  bool ok;        // every pivot positive (wave-uniform)
};

// Gradient, Hessian / step^2, its natural-order Cholesky factor (left in `tile`, lower triangle) and the proposal mean
// mu = x + (1/2) Lambda^-1 g at the point xv (metropolis_hastings.py:344-347).
__device__ __forceinline__ TfPoint tf_point(int p, int ld, int lane, const double* __restrict__ Gt, const double* __restrict__ Pt,
                                            double* __restrict__ tile, double xv, double cv, double m0v, double tau, double lam,
                                            double inv_s2) {
  const bool on = lane < p;
  const int row = on ? lane : 0;  // lanes beyond p read row 0 and write nothing
  const double t = on ? exp(xv) : 0.0;
  const double d = on ? xv - m0v : 0.0;
  double Gt_i = 0.0, Pd = 0.0;
  for (int j = 0; j < p; ++j) {
    const double tj = omc_readlane_d(t, j), dj = omc_readlane_d(d, j);
    const double gij = Gt[j * p + row], pij = Pt[j * p + row];
    Gt_i = fma(gij, tj, Gt_i);
    Pd = fma(pij, dj, Pd);
    if (on && j <= lane) tile[lane * ld + j] = (tau * ((t * tj) * gij) + lam * pij) * inv_s2;
  }
  TfPoint r;
  const double g = tau * (t * (cv - Gt_i)) - lam * Pd;
  r.target = tau * omc_wave_sum(t * cv - 0.5 * (t * Gt_i)) - 0.5 * lam * omc_wave_sum(d * Pd);
  r.ok = true;
  r.sumlog = 0.0;
  r.mu = xv;
  const double* own = tile + row * ld;
  for (int j = 0; j < p; ++j) {
    tf_wave_sync();  // row j as far as columns < j have written it
    const double* rj = tile + j * ld;
    double acc = own[j];
    for (int k = 0; k < j; ++k) acc = fma(-own[k], rj[k], acc);
    const double dj = omc_readlane_d(acc, j);
    if (!(dj > 0.0)) { r.ok = false; break; }
    const double sd = sqrt(dj);
    r.sumlog += log(sd);
    if (on && lane >= j) tile[lane * ld + j] = (lane == j) ? sd : acc / sd;
  }
  if (!r.ok) return r;
  tf_wave_sync();
  // L w = g (forward), L' v = w (backward); the first reads the lane's own row, the second column `lane` of every row
  double w = on ? g : 0.0;
  for (int j = 0; j < p; ++j) {
    const double lj = own[j];
    if (lane == j) w /= lj;
    const double wj = omc_readlane_d(w, j);
    if (on && lane > j) w = fma(-lj, wj, w);
  }
  for (int j = p - 1; j >= 0; --j) {
    const double lj = tile[j * ld + row];
    if (lane == j) w /= lj;
    const double vj = omc_readlane_d(w, j);
    if (lane < j) w = fma(-lj, vj, w);
  }
  r.mu = on ? xv + 0.5 * w : 0.0;
  return r;
}

// | L' r |^2 for the factor in `tile` (metropolis_hastings.py:372-373)
__device__ __forceinline__ double tf_quad(int p, int ld, int lane, const double* tile, double r) {
  const int row = lane < p ? lane : 0;
  double w = 0.0;
  for (int i = 0; i < p; ++i) {
    const double ri = omc_readlane_d(r, i), li = tile[i * ld + row];
    if (lane <= i && lane < p) w = fma(li, ri, w);
  }
  return omc_wave_sum(w * w);
}

#define TF_WAVES_MAX 4
__global__ void __launch_bounds__(64 * TF_WAVES_MAX) k_mala_transform_step(
    int64_t C, int64_t chain_offset, int p, const double* G, const double* cvec, const double* P, const double* m0,
    const double* tau_c, const double* lam_c, double inv_s2, double* x, int64_t ld_x, const double* z_in, const double* u_in,
    omc_rng_key nkey, omc_rng_key ukey, long long* n_accept, long long* n_proposal, double* prop_out, double* lqf_out,
    double* lqr_out, double* logp_out, long long* bad) {
  extern __shared__ double sm[];  // one p x ld tile per wave
  const int ld = p | 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
  double* tile = sm + (int64_t)wave * p * ld;
  const int64_t c = (int64_t)blockIdx.x * n_waves + wave;
  if (c >= C) return;
  const bool on = lane < p;
  const double tau = tau_c ? tau_c[c] : 1.0, lam = lam_c ? lam_c[c] : 1.0;
  const double xv = on ? x[c * ld_x + lane] : 0.0;
  const double cv = on ? cvec[lane] : 0.0;
  const double m0v = (on && m0) ? m0[lane] : 0.0;
  double z = 0.0;
  if (on) {
    if (z_in) {
      z = z_in[c * p + lane];
    } else {
      double n0, n1;
      omc_normal_pair(omc_rng_block(nkey, chain_offset + c, (uint32_t)(lane >> 1)), n0, n1);
      z = (lane & 1) ? n1 : n0;
    }
  }
  // the accept uniform: block (p + 1) / 2 + 1 of the uniform stream, beyond the (p + 1) / 2 blocks a vector of p elements takes --
  // the block the host route's decision reads (metropolis_hastings.py: sub = (p + 1) // 2 + 1), so both routes accept alike.
  // Written out, not omc_chain_uniform: that changed this kernel's code (profiles/r08_mh_refactor_same_code.txt)
  double u;
  if (u_in) {
    u = u_in[c];
  } else {
    const uint4 w = omc_rng_block(ukey, chain_offset + c, (uint32_t)((p + 1) / 2 + 1));
    u = omc_u53(w.x, w.y);
  }
  // forward: x' = mu + L^-T z, log q(x' | x)
  const TfPoint cur = tf_point(p, ld, lane, G, P, tile, xv, cv, m0v, tau, lam, inv_s2);
  double xp = NAN, lqf = NAN, lqr = NAN, tgt_p = NAN;
  bool ok = cur.ok;
  if (ok) {
    double v = z;
    for (int j = p - 1; j >= 0; --j) {
      const double lj = tile[j * ld + (on ? lane : 0)];
      if (lane == j) v /= lj;
      const double vj = omc_readlane_d(v, j);
      if (lane < j) v = fma(-lj, vj, v);
    }
    xp = on ? cur.mu + v : 0.0;
    lqf = cur.sumlog - 0.5 * tf_quad(p, ld, lane, tile, xp - cur.mu);
    tf_wave_sync();  // the tile is rebuilt at the proposed point
    const TfPoint prp = tf_point(p, ld, lane, G, P, tile, xp, cv, m0v, tau, lam, inv_s2);
    ok = prp.ok;
    tgt_p = prp.target;
    if (ok) lqr = prp.sumlog - 0.5 * tf_quad(p, ld, lane, tile, xv - prp.mu);
  }
  const double la = tgt_p + lqr - (cur.target + lqf);
  const bool acc = ok && (log(u) < la);  // a NaN log_alpha rejects, as in the reference
  if (acc && on) x[c * ld_x + lane] = xp;
  if (on && prop_out) prop_out[c * p + lane] = xp;
  if (lane == 0) {
    if (!ok) atomicMin((unsigned long long*)bad, (unsigned long long)c);
    if (n_proposal) n_proposal[c] += 1;
    if (n_accept) n_accept[c] += acc ? 1 : 0;
    if (lqf_out) lqf_out[c] = lqf;
    if (lqr_out) lqr_out[c] = lqr;
    if (logp_out) logp_out[c] = acc ? tgt_p : cur.target;
  }
}

extern "C" {

omc_status omc_transform_predict(omc_ctx* ctx, int64_t n, int64_t p, const double* X, int64_t ld_X, const double* x, int64_t ld_x,
                                 const double* add_chain, int64_t ld_add, const double* add_shared, double alpha,
                                 const double* chain_scale, double* out, int64_t ld_out) {
  if (!ctx || n < 1 || p < 1 || !X || ld_X < p || !x || ld_x < p || (add_chain && ld_add < n) || !out || ld_out < n)
    return OMC_INVALID_ARG;
  if (ctx->n_chains > 65535) return OMC_UNSUPPORTED;
  return omc_launch(ctx, k_transform_predict, dim3(omc_grid1(n, 256), (unsigned)ctx->n_chains), dim3(256), 0, n, p, X, ld_X, x, ld_x,
                    add_chain, ld_add, add_shared, alpha, chain_scale, out, ld_out);
}

omc_status omc_transform_grad_hess(omc_ctx* ctx, int64_t p, const double* x, int64_t ld_x, const double* u, int64_t ld_u,
                                   const double* G, const double* scale, double* grad, double* H) {
  if (!ctx || p < 1 || !x || ld_x < p || (grad && (!u || ld_u < p)) || (H && !G) || (!grad && !H)) return OMC_INVALID_ARG;
  if (ctx->n_chains > 65535) return OMC_UNSUPPORTED;
  unsigned gx = omc_grid1(p * p, 256);
  if (gx > 64) gx = 64;
  return omc_launch(ctx, k_transform_grad_hess, dim3(gx, (unsigned)ctx->n_chains), dim3(256), 0, p, x, ld_x, u, ld_u, G, scale, grad,
                    H);
}

omc_status omc_mala_transform_step(omc_ctx* ctx, int64_t p, const double* G, const double* cvec, const double* P, const double* m0,
                                   const double* tau, const double* lam, double step, double* x, int64_t ld_x,
                                   const double* z_inject, const double* u_inject, uint64_t draw_index, int64_t* accept_count,
                                   int64_t* proposal_count, double* prop_out, double* lq_fwd_out, double* lq_rev_out,
                                   double* logp_out) {
  if (!ctx || p < 1 || p > 64 || !G || !cvec || !P || !(step > 0.0) || !x || ld_x < p) return OMC_INVALID_ARG;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  const int ld = (int)p | 1;
  const int waves = TF_WAVES_MAX;  // p = 64: 33 KB per wave, 130 KB of the 160 KB of a CU
  const size_t lds = (size_t)waves * p * ld * sizeof(double);
  static bool lds_raised[64];  // per device: the kernel may use up to the whole LDS of a CU (asked for once, not per launch)
  if (lds > 48 * 1024 && !(ctx->device >= 0 && ctx->device < 64 && lds_raised[ctx->device])) {
    OMC_HIP_CHECK(hipFuncSetAttribute((const void*)k_mala_transform_step, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    if (ctx->device >= 0 && ctx->device < 64) lds_raised[ctx->device] = true;
  }
  hipLaunchKernelGGL(k_mala_transform_step, dim3(omc_grid1(ctx->n_chains, waves)), dim3(64 * waves), lds, ctx->stream, ctx->n_chains,
                     ctx->chain_offset, (int)p, G, cvec, P, m0, tau, lam, 1.0 / (step * step), x, ld_x, z_inject, u_inject,
                     omc_make_key(ctx->seed, draw_index, OMC_RNG_NORMAL), omc_make_key(ctx->seed, draw_index, OMC_RNG_UNIFORM),
                     (long long*)accept_count, (long long*)proposal_count, prop_out, lq_fwd_out, lq_rev_out, logp_out,
                     ctx->d_bad_chain);
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}

}  // extern "C"
