// Batched tridiagonal GMRF conjugate-Gibbs draw for gfx950:  x_c ~ N(Q_c^{-1} b_c, Q_c^{-1}).
//
// What it computes (per chain, fp64), following gmrf.sample_normal_canonical of the reference
// (gmrf.py:167-198; factor gmrf.py:489-520, solves gmrf.py:414-462, draw gmrf.py:29-61):
//     D_0 = a_0,  l_{i-1} = b_{i-1}/D_{i-1},  D_i = a_i - l_{i-1} b_{i-1}      (SuperLU's unpivoted LU pivots U_ii)
//     u_i = r_i - l_{i-1} u_{i-1}                                                (L w = b, w_i = u_i/sqrt(D_i))
//     g_i = u_i/D_i + z_i/sqrt(D_i),   x_i = g_i - l_i x_{i+1}                   (L'x = w + z)
// where L = L_lu diag(sqrt(D)) is the natural-order Cholesky factor, so x equals the reference's
// draw for the same z (not merely in distribution).
//
// Two kernels:
//   k_tridiag_serial : one lane per chain, any n, streams l through a workspace.  Simple; the
//                      cross-check for the fast path and the fallback for very long chains.
//   k_tridiag_seg    : the fast path.  A chain is cut into segments of M consecutive nodes, one
//                      lane per segment (up to 1024 lanes = one workgroup per chain); each lane
//                      keeps its 3*M working values in registers.  The three serial recurrences
//                      (pivots, forward substitution, backward substitution) are each solved as
//                      "local pass + scan over segments + local pass":
//                        pivots   : D_i = f_i(D_{i-1}) is a Moebius map; a division-free 2x2
//                                   product per segment + a scan gives every segment's incoming
//                                   pivot to ~1e-7..1e-15; Newton multiple-shooting on the true
//                                   recurrence (one affine scan per sweep) then makes the
//                                   segment joins consistent to a few ulp;
//                        forward / backward substitution: affine maps, one scan each.
//                      Global memory is touched only through wave-private LDS tiles that turn
//                      the lane-owns-M-consecutive-nodes layout into fully coalesced 512-B
//                      wave accesses.  HBM traffic per chain-update is the x store (8n B) plus
//                      shared vectors served from L2; nothing is spilled between the passes.
//                      With gamma blocks attached the same launch also performs the
//                      Normal-Gamma updates and log_post of the sweep (omc_gmrf_sweep).
#include <math.h>
#include <time.h>

#include "omc_common.h"
#include "omc_tridiag_args.h"
#include "omc_tridiag_epilogue.h"

// ------------------------------------------------------------------------------------------
// serial kernel
__global__ void __launch_bounds__(64) k_tridiag_serial(TriArgs A) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= A.C) return;
  const int nt = A.T.n_terms;
  const int64_t n = A.n;
  double sc[OMC_MAX_TERMS];
  _Pragma("unroll") for (int k = 0; k < OMC_MAX_TERMS; ++k) if (k < nt) sc[k] = A.T.scale[k] ? A.T.scale[k][c] : 1.0;
  double* lw = A.work + c * n;
  double* xo = A.x + c * A.ld_x;
  const int64_t gc = A.chain_offset + c;
  bool bad = false;
  double lp = 0.0, bprev = 0.0, u = 0.0, logdet = 0.0, zodd = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    double av = 0.0, bv = 0.0, rv = 0.0;
    _Pragma("unroll") for (int k = 0; k < OMC_MAX_TERMS; ++k) if (k < nt) {
      av = fma(sc[k], A.T.diag[k] ? A.T.diag[k][i] : 1.0, av);
      if (A.T.off[k] && i < n - 1) bv = fma(sc[k], A.T.off[k][i], bv);
      if (A.T.rhs[k]) rv = fma(sc[k], A.T.rhs[k][i], rv);
    }
    if (A.rhs_chain) rv += A.rhs_chain[c * A.ld_rhs + i];
    double D = fma(-lp, bprev, av);
    bad |= !(D > 0.0);
    double rD = fast_rcp(D);
    u = fma(-lp, u, rv);
    double zi;
    if (A.z) {
      zi = A.z[c * A.ld_z + i];
    } else if (A.zero_z) {
      zi = 0.0;
    } else if ((i & 1) == 0) {
      omc_normal_pair(omc_rng_block(A.key, gc, (uint32_t)(i >> 1)), zi, zodd);
    } else {
      zi = zodd;
    }
    xo[i] = fma(u, rD, zi * sqrt(rD));
    logdet -= log(rD);
    lp = bv * rD;
    lw[i] = lp;
    bprev = bv;
  }
  const bool want_quad = A.quad || A.fused;
  double acc[OMC_MAX_TERMS] = {0, 0, 0, 0}, rnext[OMC_MAX_TERMS] = {0, 0, 0, 0};
  double x = 0.0;
  for (int64_t i = n - 1; i >= 0; --i) {
    x = fma(-lw[i], x, xo[i]);
    xo[i] = x;
    if (want_quad) {
      _Pragma("unroll") for (int k = 0; k < OMC_MAX_TERMS; ++k) if (k < nt) {
        double r = x - (A.T.center[k] ? A.T.center[k][i] : 0.0);
        double dk = A.T.diag[k] ? A.T.diag[k][i] : 1.0;
        double ok = (A.T.off[k] && i < n - 1) ? A.T.off[k][i] : 0.0;
        acc[k] += dk * r * r + 2.0 * ok * r * rnext[k];
        rnext[k] = r;
      }
    }
  }
  if (A.quad)
    _Pragma("unroll") for (int k = 0; k < OMC_MAX_TERMS; ++k) if (k < nt) A.quad[k * A.C + c] = acc[k];
  if (A.logdet) A.logdet[c] = logdet;
  if (bad) atomicMin((unsigned long long*)A.bad, (unsigned long long)c);
  if (A.fused) sweep_epilogue(A, c, acc);
}

// ------------------------------------------------------------------------------------------
// segmented kernel (its scan machinery, tile traffic and the kernel itself)
#include "omc_tridiag_seg.h"

// is_smoother: host-side test of the SIG 1 structure
static bool is_smoother(const TermsDev& T) {
  if (T.n_terms != 2) return false;
  for (int i = 0; i < 2; ++i) {  // i: the identity term
    const int p = 1 - i;
    if (!T.diag[i] && !T.off[i] && T.rhs[i] && T.center[i] && T.diag[p] && T.off[p] && !T.rhs[p] && !T.center[p]) return true;
  }
  return false;
}

// SIG 3: the smoother whose tridiagonal term carries the per-chain centre (and nothing else differs: no per-chain offsets,
// identity term with or without a shared centre)
static bool is_shifted_smoother(const TermsDev& T, const CentreChain& cc) {
  if (T.n_terms != 2 || !cc.v || cc.k < 0) return false;
  const int p = cc.k, i = 1 - cc.k;
  return !T.diag[i] && !T.off[i] && ((T.rhs[i] != nullptr) == (T.center[i] != nullptr)) && T.diag[p] && T.off[p] && !T.rhs[p] &&
         !T.center[p];
}

// reads the descriptors of the re-entered instantiations (OMC_KD_WORDS) for the host-side check below
__global__ void k_reentry_probe(uint32_t* out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  OMC_KD_WORDS(8, 1024, 1, out);
  OMC_KD_WORDS(10, 1024, 1, out + 3);
}

// the expectation, on the three descriptor words the probe returns (LLVM AMDGPUUsage, "Kernel Descriptor")
static bool reentry_descriptor_ok(uint32_t private_size, uint32_t rsrc2, uint32_t props_preload) {
  const uint32_t props = props_preload & 0xffffu, preload = props_preload >> 16;
  const bool user_sgprs = ((rsrc2 >> 1) & 0x1fu) == 2u && (props & 0x7fu) == 0x08u;  // kernarg segment pointer only
  const bool system_sgprs = ((rsrc2 >> 7) & 0xfu) == 0x1u;                           // workgroup id x; no y, z, info
  const bool no_private = private_size == 0u && (rsrc2 & 1u) == 0u && (props & (1u << 11)) == 0u;
  const bool wave64 = (props & (1u << 10)) == 0u;
  return user_sgprs && system_sgprs && no_private && wave64 && preload == 0u;
}

static int g_reentry_ok = -1;  // -1: not probed yet (process-wide: one code object)
static bool reentry_abi_ok(omc_ctx* ctx) {
  if (g_reentry_ok >= 0) return g_reentry_ok != 0;
  omc_buf<uint32_t> d;  // freed on return
  uint32_t h[6] = {~0u, ~0u, ~0u, ~0u, ~0u, ~0u};
  bool ok = hipMalloc(&d.p, sizeof(h)) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(k_reentry_probe, dim3(1), dim3(64), 0, ctx->stream, d.p);
    ok = hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, ctx->stream) == hipSuccess &&
         hipStreamSynchronize(ctx->stream) == hipSuccess;
  }
  ok = ok && reentry_descriptor_ok(h[0], h[1], h[2]) && reentry_descriptor_ok(h[3], h[4], h[5]);
  g_reentry_ok = ok ? 1 : 0;
  if (!ok) omc_set_error_text("omc_gmrf_run: the kernel descriptor does not match the restart's entry state; self-restarting workgroups are off");
  return ok;
}
int omc_reentry_probe_result(omc_ctx* ctx) { return reentry_abi_ok(ctx) ? 1 : 0; }

// ------------------------------------------------------------------------------------------
// small helpers
__global__ void k_tridiag_matvec(int64_t n, const double* diag, const double* off, const double* v, double* out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    double t = (diag ? diag[i] : 1.0) * v[i];
    if (off) {
      if (i > 0) t = fma(off[i - 1], v[i - 1], t);
      if (i < n - 1) t = fma(off[i], v[i + 1], t);
    }
    out[i] = t;
  }
}

// out[c][:] (+)= scale[c] * M v_c for per-chain vectors v_c (M tridiagonal from diag / off; NULL diag = identity)
__global__ void __launch_bounds__(256) k_tridiag_matvec_chain(int64_t n, const double* diag, const double* off, const double* v,
                                                              int64_t ld_v, const double* scale, double* out, int64_t ld_o,
                                                              int accumulate) {
  const int64_t c = blockIdx.y;
  const double s = scale ? scale[c] : 1.0;
  const double* vc = v + c * ld_v;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    double t = (diag ? diag[i] : 1.0) * vc[i];
    if (off) {
      if (i > 0) t = fma(off[i - 1], vc[i - 1], t);
      if (i < n - 1) t = fma(off[i], vc[i + 1], t);
    }
    out[c * ld_o + i] = accumulate ? fma(s, t, out[c * ld_o + i]) : s * t;
  }
}

// out[c][:] = a x_c + b y_c   (y per chain, or shared with ld_y == 0)
__global__ void __launch_bounds__(256) k_chain_lincomb(int64_t n, double a, const double* x, int64_t ld_x, double b, const double* y,
                                                       int64_t ld_y, double* out, int64_t ld_o) {
  const int64_t c = blockIdx.y;
  // b == 0: y is not read at all (the BLAS convention: 0 * inf or 0 * NaN in y must not reach the result -- a scale of
  // +inf is what the Normal-Gamma update's zero-rate guard produces, sampler.py:285-286)
  if (b == 0.0) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
      out[c * ld_o + i] = a * x[c * ld_x + i];
    return;
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[c * ld_o + i] = fma(a, x[c * ld_x + i], b * y[c * ld_y + i]);
}

// one workgroup per chain: quad[k][c] = (x-m_k)' M_k (x-m_k)
// One pass over the chain's row for all NT terms: the row (the only per-chain operand) is read once, a vector a term does
// not have is not read at all (uniform branches on flags set before the loop: an identity term around a shared centre
// runs at the row's bandwidth), and the element indices are 32-bit on uniform base pointers (scalar-base loads, no
// 64-bit address arithmetic per load).  Every term's sum is accumulated in the order it always was.
template <int NT, bool CCV>
__device__ __forceinline__ void quadform_row(const TermsDev& T, const CentreChain& CC, int64_t n, const double* xc, const double* ccv,
                                             double (&acc)[OMC_MAX_TERMS]) {
  bool hd[NT], ho[NT], hc[NT], hcc[NT], any_off = false;
#pragma unroll
  for (int k = 0; k < NT; ++k) {
    hd[k] = T.diag[k] != nullptr; ho[k] = T.off[k] != nullptr && n > 1; hc[k] = T.center[k] != nullptr;
    hcc[k] = CCV && CC.k == k;
    any_off |= ho[k];
  }
  const unsigned nn = (unsigned)n, step = blockDim.x;  // (n < 2^31: checked by the entry point)
  for (unsigned i = threadIdx.x; i < nn; i += step) {
    const bool has_next = i + 1 < nn;
    const unsigned in = has_next ? i + 1 : i;
    const double xi = xc[i];
    double xn = 0.0, ci = 0.0, cn = 0.0;
    if (any_off) xn = xc[in];
    if constexpr (CCV) {
      ci = ccv[i];
      if (any_off) cn = ccv[in];
    }
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      const double r = xi - (hc[k] ? T.center[k][i] : 0.0) - (hcc[k] ? ci : 0.0);
      acc[k] = fma((hd[k] ? T.diag[k][i] : 1.0) * r, r, acc[k]);
      if (ho[k] && has_next) {
        const double rn = xn - (hc[k] ? T.center[k][in] : 0.0) - (hcc[k] ? cn : 0.0);
        acc[k] = fma(2.0 * T.off[k][i] * r, rn, acc[k]);
      }
    }
  }
}

__global__ void __launch_bounds__(256) k_tridiag_quadform(TermsDev T, CentreChain CC, int64_t n, int64_t C, const double* x,
                                                         int64_t ld_x, double* quad) {
  __shared__ double red[OMC_MAX_TERMS][4];
  const int64_t c = blockIdx.x;
  const double* xc = x + c * ld_x;
  const double* ccv = CC.v ? CC.v + c * CC.ld : nullptr;
  double acc[OMC_MAX_TERMS];
#pragma unroll
  for (int k = 0; k < OMC_MAX_TERMS; ++k) acc[k] = 0.0;
  if (ccv) {
    switch (T.n_terms) {
      case 1: quadform_row<1, true>(T, CC, n, xc, ccv, acc); break;
      case 2: quadform_row<2, true>(T, CC, n, xc, ccv, acc); break;
      case 3: quadform_row<3, true>(T, CC, n, xc, ccv, acc); break;
      default: quadform_row<4, true>(T, CC, n, xc, ccv, acc); break;
    }
  } else {
    switch (T.n_terms) {
      case 1: quadform_row<1, false>(T, CC, n, xc, ccv, acc); break;
      case 2: quadform_row<2, false>(T, CC, n, xc, ccv, acc); break;
      case 3: quadform_row<3, false>(T, CC, n, xc, ccv, acc); break;
      default: quadform_row<4, false>(T, CC, n, xc, ccv, acc); break;
    }
  }
#pragma unroll
  for (int k = 0; k < OMC_MAX_TERMS; ++k) {
    double a = acc[k];
    for (int d = 32; d >= 1; d >>= 1) a += __shfl_xor(a, d, 64);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = a;
  }
  __syncthreads();
  if (threadIdx.x < OMC_MAX_TERMS && (int)threadIdx.x < T.n_terms) {
    const int k = threadIdx.x;
    quad[k * C + c] = red[k][0] + red[k][1] + red[k][2] + red[k][3];
  }
}

// log det of one shared tridiagonal matrix of any length: D_i = a_i - b_{i-1}^2 / D_{i-1}, sum log D_i (gmrf.py:489-520)
__global__ void __launch_bounds__(64) k_tridiag_logdet_serial(int64_t n, const double* diag, const double* off, double* logdet,
                                                              long long* bad) {
  if (blockIdx.x != 0) return;
  // One dependent chain -- but the chain is the recurrence alone.  The wave fetches 64 columns at a time (one coalesced
  // load per vector, the next 64 while the current ones are consumed), every lane runs the same recurrence on values
  // handed round by v_readlane (no branch, no load inside the chain), and the logarithm is taken of a running product of
  // mantissas, once per 64 columns.  (One lane with its loads inside the chain: a trip to memory per column, 7.6 ms at
  // n = 20 000 and 22 ms at n = 50 000 -- more than ten sweeps of the model this is the set-up of.)
  const int lane = threadIdx.x;
  auto fetch = [&](int64_t i0, double& a, double& b) {  // padding: a = 1, b = 0 (pivot 1, log 0)
    const int64_t i = i0 + lane;
    a = (diag && i < n) ? diag[i] : 1.0;
    b = (off && i >= 1 && i < n) ? off[i - 1] : 0.0;
  };
  auto bcast = [&](double v, int t) -> double {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), t), __builtin_amdgcn_readlane(__double2loint(v), t));
  };
  double D = 1.0, mant = 1.0;
  long long ex = 0;
  bool neg = false;
  double a_cur, b_cur, a_nxt, b_nxt;
  fetch(0, a_cur, b_cur);
  for (int64_t i0 = 0; i0 < n; i0 += 64) {
    fetch(i0 + 64, a_nxt, b_nxt);
#pragma unroll
    for (int t = 0; t < 64; ++t) {
      const double a = bcast(a_cur, t), b = bcast(b_cur, t);
      D = fma(-b * omc_rcp_nr(D), b, a);  // (the first column: b = 0)
      const bool ok = D > 0.0;
      neg |= !ok;
      const double Dp = ok ? D : 1.0;
      mant *= __builtin_amdgcn_frexp_mant(Dp);
      ex += __builtin_amdgcn_frexp_exp(Dp);
      if ((t & 15) == 15) {
        ex += __builtin_amdgcn_frexp_exp(mant);
        mant = __builtin_amdgcn_frexp_mant(mant);
      }
    }
    a_cur = a_nxt; b_cur = b_nxt;
  }
  if (lane == 0) {
    logdet[0] = neg ? NAN : log(mant) + (double)ex * 0.69314718055994530942;
    if (neg) atomicMin((unsigned long long*)bad, 0ull);
  }
}

// ------------------------------------------------------------------------------------------
// host side
static bool terms_to_dev(const omc_tridiag_terms* t, TermsDev* d, CentreChain* cc = nullptr) {
  if (!t || t->n_terms < 1 || t->n_terms > OMC_MAX_TERMS) return false;
  d->n_terms = t->n_terms;
  for (int k = 0; k < OMC_MAX_TERMS; ++k) {
    const bool on = k < t->n_terms;
    d->diag[k] = on ? t->diag[k] : nullptr;
    d->off[k] = on ? t->off[k] : nullptr;
    d->rhs[k] = on ? t->rhs[k] : nullptr;
    d->center[k] = on ? t->center[k] : nullptr;
    d->scale[k] = on ? t->scale[k] : nullptr;
  }
  if (cc) {  // at most one term with a per-chain centre per call
    *cc = CentreChain{};
    for (int k = 0; k < t->n_terms; ++k)
      if (t->center_chain[k]) {
        cc->k = cc->v ? -1 : k;  // (-1: more than one -- the entry points answer OMC_UNSUPPORTED)
        cc->v = t->center_chain[k];
      }
    cc->ld = t->ld_center_chain;
  }
  return true;
}
static bool has_center_chain(const CentreChain& cc) { return cc.v != nullptr; }

static void args_defaults(omc_ctx* ctx, TriArgs* A, int64_t n) {
  A->T = TermsDev{};  // every pointer null, no terms: a caller that fills the terms by hand cannot leave a field behind
  A->cc = CentreChain{};
  A->n = n; A->C = ctx->n_chains; A->chain_offset = ctx->chain_offset;
  A->rhs_chain = nullptr; A->ld_rhs = 0;
  A->z = nullptr; A->ld_z = 0; A->zero_z = 0;
  A->key = omc_make_key(ctx->seed, 0, OMC_RNG_NORMAL);
  A->x = nullptr; A->ld_x = 0; A->quad = nullptr; A->logdet = nullptr;
  A->bad = ctx->d_bad_chain;
  A->fallbacks = ctx->d_fallbacks;
  A->newton_max = ctx->tridiag_newton_max;
  A->perturb_start = ctx->tridiag_perturb_ppb * 1e-9;
  A->work = nullptr;
  A->fused = 0;
  A->stamps = ctx->stamps;
  A->sweep_times = nullptr; A->sweep_times_cap = 0; A->sweep_times_pos = 0;  // (omc_gmrf_run switches the sweep clock on)
  A->log_post = nullptr;
  A->gb_dev = nullptr; A->gdraw_dev = nullptr;
  A->n_sweeps = 0; A->reenter = 0; A->block_sweeps = 0; A->early_draws = 0; A->epoch = 0; A->seed = ctx->seed; A->handoff = nullptr; A->timeouts = ctx->d_fallbacks + 1;
  for (int k = 0; k < OMC_MAX_TERMS; ++k) A->gdraw[k] = 0;
  for (int i = 0; i < OMC_RUN_MAX; ++i) { A->rec[i].draw = 0; A->rec[i].x = nullptr; A->rec[i].log_post = nullptr; A->rec[i].slot_off = -1; }
  for (int k = 0; k < OMC_MAX_TERMS; ++k) {
    A->gb[k].enabled = 0; A->gb[k].a0 = A->gb[k].b0 = A->gb[k].half_npos = A->gb[k].lnorm = 0.0;
    A->gb[k].g_inject = nullptr; A->gb[k].store = nullptr; A->gb[k].scale_out = nullptr;
    A->gb[k].logdet_unscaled = nullptr; A->gb[k].key = A->key;
  }
}

// CLOCK_MONOTONIC in seconds: the clock of Python's time.perf_counter on Linux, so a caller can place the launch log on
// its own time axis
static double omc_host_clock() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

static int pow2_ceil(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

// nodes-per-lane variants: M -> (largest n, launch bound of the one-chain-per-workgroup form)
template <int M> struct SegCfg;
// SMOOTHER: 1 where the structure-specialised instantiation (SIG 1) exists -- the variants auto_seg picks
template <> struct SegCfg<8>  { static constexpr int MAXT = 1024; static constexpr int SMOOTHER = 1; };
template <> struct SegCfg<10> { static constexpr int MAXT = 1024; static constexpr int SMOOTHER = 1; };
template <> struct SegCfg<16> { static constexpr int MAXT = 640; static constexpr int SMOOTHER = 0; };  // measured at cfg3 with SIG 1:
template <> struct SegCfg<20> { static constexpr int MAXT = 512; static constexpr int SMOOTHER = 0; };  // 125 and 112 us against 102 for M = 10
template <> struct SegCfg<32> { static constexpr int MAXT = 512; static constexpr int SMOOTHER = 0; };
static int64_t seg_max_n(int seg) {
  switch (seg) {
    case 8: return 8 * 1024;
    case 10: return 10 * 1024;
    case 16: return 16 * 640;
    case 20: return 20 * 512;
    case 32: return 32 * 512;
  }
  return 0;
}

template <int M>
static bool launch_seg(omc_ctx* ctx, const TriArgs& A_in) {
  TriArgs A = A_in;
  const int S = (int)((A.n + M - 1) / M);
  if (S <= 64) {
    const int G = pow2_ceil(S);
    const int64_t chains_per_block = 4 * (64 / G);
    const int64_t grid = (A.C + chains_per_block - 1) / chains_per_block;
    hipLaunchKernelGGL((k_tridiag_seg<M, false, 256>), dim3((unsigned)grid), dim3(256), 0, ctx->stream, A, G);
  } else {
    const int threads = 64 * ((S + 63) / 64);
    // the specialised instantiation owns the CU (its LDS image is sized for a full workgroup); a short chain
    // leaves room for a second workgroup of the generic one, which then wins (n = 2000: 38 against 53 us)
    const bool special = SegCfg<M>::SMOOTHER && !ctx->tridiag_generic && is_smoother(A.T) && !has_center_chain(A.cc) && A.n >= 2 &&
                         2 * threads > SegCfg<M>::MAXT;
    // self-restarting workgroups: the specialised instantiation only (it keeps no private memory, so the three entry
    // registers are all a restart has to reproduce)
    if (!special) A.reenter = 0;
    if (!special && A.fused) {
      // the Normal-Gamma blocks in device memory for the generic instantiation (stream-ordered copy: the previous launch
      // has read its image by the time this one is written)
      const size_t gb_bytes = sizeof(A.gb), gd_bytes = sizeof(A.gdraw);
      if (!ctx->d_gamma_tab && hipMalloc(&ctx->d_gamma_tab.p, gb_bytes + gd_bytes) != hipSuccess) return false;
      if (hipMemcpyAsync(ctx->d_gamma_tab, A.gb, gb_bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return false;
      if (hipMemcpyAsync((char*)ctx->d_gamma_tab.p + gb_bytes, A.gdraw, gd_bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        return false;
      A.gb_dev = (const GammaDev*)ctx->d_gamma_tab.p;
      A.gdraw_dev = (const unsigned long long*)((char*)ctx->d_gamma_tab.p + gb_bytes);
    }
    // workgroup-per-chain form: one workgroup per (sweep, chain), or per chain when the workgroups restart themselves
    const int64_t wg_per_chain = A.n_sweeps <= 0 ? 1 : (!A.reenter ? A.n_sweeps : (A.block_sweeps > 0 ? (A.n_sweeps + A.block_sweeps - 1) / A.block_sweeps : 1));
    const unsigned wg_grid = (unsigned)(A.C * wg_per_chain);
    // the shifted smoother (SIG 3): single-sweep launches without per-chain offsets (not the fused sweep: its epilogue's
    // log-posterior would need the shared centre's terms spelled out for e-coordinates)
    const bool shifted = SegCfg<M>::SMOOTHER && !ctx->tridiag_generic && is_shifted_smoother(A.T, A.cc) && !A.rhs_chain && !A.fused &&
                         A.n_sweeps <= 0 && A.n >= 2 && 2 * threads > SegCfg<M>::MAXT;
    if (shifted)
      hipLaunchKernelGGL((k_tridiag_seg<M, true, SegCfg<M>::MAXT, 3 * SegCfg<M>::SMOOTHER>), dim3(wg_grid), dim3(threads), 0,
                         ctx->stream, A, threads);
    else if (special && SegCfg<M>::SMOOTHER && A.early_draws && !A.reenter && !A.z && !A.zero_z)  // the waiting form (see the kernel)
      hipLaunchKernelGGL((k_tridiag_seg<M, true, SegCfg<M>::MAXT, 2 * SegCfg<M>::SMOOTHER>), dim3(wg_grid), dim3(threads), 0,
                         ctx->stream, A, threads);
    else if (special)
      hipLaunchKernelGGL((k_tridiag_seg<M, true, SegCfg<M>::MAXT, SegCfg<M>::SMOOTHER>), dim3(wg_grid), dim3(threads), 0,
                         ctx->stream, A, threads);
    else
      hipLaunchKernelGGL((k_tridiag_seg<M, true, SegCfg<M>::MAXT>), dim3(wg_grid), dim3(threads), 0, ctx->stream,
                         A, threads);
  }
  return true;
}

static bool launch_seg_any(omc_ctx* ctx, const TriArgs& A, int seg) {
  switch (seg) {
    case 8: return launch_seg<8>(ctx, A);
    case 10: return launch_seg<10>(ctx, A);
    case 16: return launch_seg<16>(ctx, A);
    case 20: return launch_seg<20>(ctx, A);
    case 32: return launch_seg<32>(ctx, A);
  }
  return false;
}

static int auto_seg(int64_t n) {
  // fewest nodes per lane that still fits one workgroup (measured on cfg3: 10 beats 16 and 20)
  if (n <= seg_max_n(8)) return 8;
  if (n <= seg_max_n(10)) return 10;
  return 32;
}

// true if launch_tridiag would run the workgroup-per-chain form of the segmented kernel for n nodes (the only form
// that takes several sweeps per launch)
static bool takes_wg_per_chain(const omc_ctx* ctx, int64_t n) {
  if (ctx->tridiag_algo == 1) return false;
  const int seg = ctx->tridiag_seg ? ctx->tridiag_seg : auto_seg(n);
  if (n > seg_max_n(seg)) return false;
  return (n + seg - 1) / seg > 64;
}

// true if launch_tridiag would pick the structure-specialised instantiation (the one that takes several sweeps per launch)
static bool takes_specialised(const omc_ctx* ctx, const TermsDev& T, int64_t n) {
  if (!takes_wg_per_chain(ctx, n) || ctx->tridiag_generic || !is_smoother(T) || n < 2) return false;
  const int seg = ctx->tridiag_seg ? ctx->tridiag_seg : auto_seg(n);
  const int threads = 64 * (int)(((n + seg - 1) / seg + 63) / 64);
  switch (seg) {
    case 8: return SegCfg<8>::SMOOTHER && 2 * threads > SegCfg<8>::MAXT;
    case 10: return SegCfg<10>::SMOOTHER && 2 * threads > SegCfg<10>::MAXT;
    case 16: return SegCfg<16>::SMOOTHER && 2 * threads > SegCfg<16>::MAXT;
    case 20: return SegCfg<20>::SMOOTHER && 2 * threads > SegCfg<20>::MAXT;
    case 32: return SegCfg<32>::SMOOTHER && 2 * threads > SegCfg<32>::MAXT;
  }
  return false;
}

static omc_status launch_tridiag(omc_ctx* ctx, TriArgs& A) {
  int algo = ctx->tridiag_algo;
  int seg = ctx->tridiag_seg;
  const int64_t n = A.n;
  if (algo == 0) algo = (n <= seg_max_n(32)) ? 2 : 1;
  if (algo == 2) {
    if (seg == 0) seg = auto_seg(n);
    if (n > seg_max_n(seg)) {
      if (ctx->tridiag_algo == 2) return OMC_UNSUPPORTED;
      algo = 1;
    }
  }
  if (algo == 2) {
    if (!launch_seg_any(ctx, A, seg)) return OMC_INVALID_ARG;
  } else {
    if (!A.x) return OMC_INVALID_ARG;
    const omc_status st = omc_ensure(ctx, ctx->workspace, (size_t)A.C * (size_t)n * sizeof(double));
    if (st != OMC_OK) return st;
    A.work = ctx->workspace;
    const int64_t grid = (A.C + 63) / 64;
    hipLaunchKernelGGL(k_tridiag_serial, dim3((unsigned)grid), dim3(64), 0, ctx->stream, A);
  }
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}

// ------------------------------------------------------------------------------------------
// Chains too long for one workgroup (n > 16 384).  The one-lane-per-chain kernel is a cliff there (28 ms per sweep at
// n = 20 000 x 1024 chains); the segmented kernels of the band route (omc_band.hip, bandwidth 1) take any n at 2-5 ms.
// The tridiagonal terms are put into that route's band storage (a stream-ordered device copy of 2 n doubles per term into
// a context buffer), the draw is omc_band_sample_canonical -- same natural-order factor, same draw streams, equal to the
// tridiagonal kernels' result to rounding -- and what the fused sweep adds (quadratic forms, Normal-Gamma updates, log
// posterior) follows as the library's own separate launches.
__global__ void __launch_bounds__(256) k_band_from_tridiag(int64_t n, const double* diag, const double* off, double* band) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    band[i] = diag ? diag[i] : 1.0;
    band[n + i] = (off && i < n - 1) ? off[i] : 0.0;
  }
}

static bool long_chain_route(const omc_ctx* ctx, int64_t n) { return ctx->tridiag_algo == 0 && n > seg_max_n(32); }

static omc_status long_chain_draw(omc_ctx* ctx, int64_t n, const omc_tridiag_terms* t, const double* rhs_chain, int64_t ld_rhs,
                                  const double* z, int64_t ld_z, uint64_t draw_index, double* x, int64_t ld_x, double* mean,
                                  int64_t ld_mean, double* logdet) {
  omc_band_terms bt;
  bt.n_terms = t->n_terms;
  const size_t per = 2 * (size_t)n * sizeof(double);
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  {
    const omc_status st = omc_ensure(ctx, ctx->long_band, per * OMC_MAX_TERMS);
    if (st != OMC_OK) return st;
  }
  for (int k = 0; k < OMC_MAX_TERMS; ++k) {
    bt.band[k] = nullptr; bt.bw[k] = 0; bt.rhs[k] = nullptr; bt.scale[k] = nullptr;
    if (k >= t->n_terms) continue;
    bt.rhs[k] = t->rhs[k];
    bt.scale[k] = t->scale[k];
    if (t->diag[k] || t->off[k]) {
      double* b = ctx->long_band + (size_t)k * 2 * (size_t)n;
      int64_t grid = (n + 255) / 256;
      if (grid > 1024) grid = 1024;
      hipLaunchKernelGGL(k_band_from_tridiag, dim3((unsigned)grid), dim3(256), 0, ctx->stream, n, t->diag[k], t->off[k], b);
      bt.band[k] = b;
      bt.bw[k] = t->off[k] ? 1 : 0;
    }
  }
  OMC_HIP_CHECK(hipGetLastError());
  return omc_band_sample_canonical(ctx, n, 1, &bt, rhs_chain, ld_rhs, z, ld_z, draw_index, x, ld_x, mean, ld_mean, logdet);
}

extern "C" {

int32_t omc_reentry_descriptor_ok(uint32_t private_segment_fixed_size, uint32_t compute_pgm_rsrc2, uint32_t properties_and_preload) {
  return reentry_descriptor_ok(private_segment_fixed_size, compute_pgm_rsrc2, properties_and_preload) ? 1 : 0;
}

omc_status omc_tridiag_sample_canonical(omc_ctx* ctx, int64_t n, const omc_tridiag_terms* terms,
                                        const double* rhs_chain, int64_t ld_rhs, const double* z_inject,
                                        int64_t ld_z, uint64_t draw_index, double* x_out, int64_t ld_x,
                                        double* mean_out, int64_t ld_mean, double* quad_out, double* logdet_out) {
  if (!ctx || n < 1 || !x_out || ld_x < n) return OMC_INVALID_ARG;
  if ((rhs_chain && ld_rhs < n) || (z_inject && ld_z < n) || (mean_out && ld_mean < n)) return OMC_INVALID_ARG;
  TriArgs A{};
  args_defaults(ctx, &A, n);
  if (!terms_to_dev(terms, &A.T, &A.cc)) return OMC_INVALID_ARG;
  if (has_center_chain(A.cc) && (A.cc.k < 0 || !takes_wg_per_chain(ctx, n) || A.cc.ld < n)) return OMC_UNSUPPORTED;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  if (long_chain_route(ctx, n)) {
    omc_status st = long_chain_draw(ctx, n, terms, rhs_chain, ld_rhs, z_inject, ld_z, draw_index, x_out, ld_x, mean_out, ld_mean,
                                    logdet_out);
    if (st != OMC_OK || !quad_out) return st;
    return omc_tridiag_quadform(ctx, n, terms, x_out, ld_x, quad_out);
  }
  A.rhs_chain = rhs_chain; A.ld_rhs = ld_rhs;
  A.key = omc_make_key(ctx->seed, draw_index, OMC_RNG_NORMAL);
  if (mean_out) {  // mu = Q^{-1} b is the same solve with z = 0 (gmrf.py:196)
    A.zero_z = 1;
    A.x = mean_out; A.ld_x = ld_mean;
    omc_status st = launch_tridiag(ctx, A);
    if (st != OMC_OK) return st;
  }
  A.z = z_inject; A.ld_z = ld_z; A.zero_z = 0;
  A.x = x_out; A.ld_x = ld_x; A.quad = quad_out; A.logdet = logdet_out;
  A.cc.quad_skip = quad_out ? ctx->tridiag_quad_skip : 0;  // (honoured by the generic workgroup-per-chain instantiation only)
  return launch_tridiag(ctx, A);
}

omc_status omc_gmrf_sweep(omc_ctx* ctx, int64_t n, const omc_tridiag_terms* terms, const omc_gamma_block* blocks,
                          const double* rhs_chain, int64_t ld_rhs, const double* z_inject, int64_t ld_z,
                          uint64_t draw_index, double* x_out, int64_t ld_x, double* log_post_out) {
  if (!ctx || n < 1 || !x_out || ld_x < n || !blocks) return OMC_INVALID_ARG;
  if ((rhs_chain && ld_rhs < n) || (z_inject && ld_z < n)) return OMC_INVALID_ARG;
  TriArgs A{};
  args_defaults(ctx, &A, n);
  if (!terms_to_dev(terms, &A.T, &A.cc)) return OMC_INVALID_ARG;
  if (has_center_chain(A.cc) && (A.cc.k < 0 || !takes_wg_per_chain(ctx, n) || A.cc.ld < n)) return OMC_UNSUPPORTED;
  for (int k = 0; k < A.T.n_terms; ++k) {
    const omc_gamma_block& b = blocks[k];
    GammaDev& g = A.gb[k];
    g.enabled = b.enabled ? 1 : 0;
    if (g.enabled) {
      if (!terms->scale[k] || b.n_pos < 0 || !(b.a0 + 0.5 * (double)b.n_pos > 0.0)) return OMC_INVALID_ARG;
      if (log_post_out && !(b.a0 > 0.0 && b.b0 > 0.0)) return OMC_INVALID_ARG;
    }
    if (log_post_out && !b.logdet_unscaled) return OMC_INVALID_ARG;
    g.a0 = b.a0; g.b0 = b.b0; g.half_npos = 0.5 * (double)b.n_pos;
    g.lnorm = (g.enabled && log_post_out) ? b.a0 * log(b.b0) - lgamma(b.a0) : 0.0;
    g.g_inject = b.g_inject; g.store = b.store;
    g.scale_out = const_cast<double*>(terms->scale[k]);
    g.logdet_unscaled = b.logdet_unscaled;
    g.key = omc_make_key(ctx->seed, b.draw_index, OMC_RNG_GAMMA);
  }
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  if (long_chain_route(ctx, n)) {
    // the sweep as separate launches: draw, quadratic forms, Normal-Gamma updates, log posterior (model.py:57-70)
    const int nt = terms->n_terms;
    const int64_t C = ctx->n_chains;
    {
      const omc_status st0 = omc_ensure(ctx, ctx->long_quad, (size_t)OMC_MAX_TERMS * C * sizeof(double));
      if (st0 != OMC_OK) return st0;
    }
    omc_status st = long_chain_draw(ctx, n, terms, rhs_chain, ld_rhs, z_inject, ld_z, draw_index, x_out, ld_x, nullptr, 0, nullptr);
    if (st != OMC_OK) return st;
    st = omc_tridiag_quadform(ctx, n, terms, x_out, ld_x, ctx->long_quad);
    if (st != OMC_OK) return st;
    for (int k = 0; k < nt; ++k) {
      const omc_gamma_block& b = blocks[k];
      if (!b.enabled) continue;
      double* const sc = const_cast<double*>(terms->scale[k]);
      st = omc_normal_gamma_update(ctx, b.a0, b.b0, b.n_pos, ctx->long_quad + k * C, b.g_inject, b.draw_index, sc);
      if (st != OMC_OK) return st;
      if (b.store) {
        st = omc_chain_copy(ctx, 1, sc, 1, b.store, 1);
        if (st != OMC_OK) return st;
      }
    }
    if (log_post_out) {
      int first = 1;
      for (int k = 0; k < nt; ++k) {
        const omc_gamma_block& b = blocks[k];
        st = omc_scaled_gauss_logpdf(ctx, n, terms->scale[k], b.logdet_unscaled, ctx->long_quad + k * C, log_post_out, first ? 0 : 1);
        if (st != OMC_OK) return st;
        first = 0;
        if (b.enabled) {
          st = omc_gamma_logpdf(ctx, terms->scale[k], b.a0, b.b0, log_post_out, 1);
          if (st != OMC_OK) return st;
        }
      }
    }
    return OMC_OK;
  }
  A.rhs_chain = rhs_chain; A.ld_rhs = ld_rhs;
  A.z = z_inject; A.ld_z = ld_z;
  A.key = omc_make_key(ctx->seed, draw_index, OMC_RNG_NORMAL);
  A.x = x_out; A.ld_x = ld_x;
  A.zero_z = ctx->debug_zero_z;
  A.fused = 1;
  A.log_post = log_post_out;
  return launch_tridiag(ctx, A);
}

omc_status omc_gmrf_run(omc_ctx* ctx, int64_t n, const omc_tridiag_terms* terms, const omc_gamma_block* blocks,
                        int64_t n_burn, int64_t n_iter, int64_t n_thin, uint64_t draw_index0, uint64_t draws_per_sweep,
                        double* x_store, int64_t ld_x, int64_t x_slot_stride, int64_t first_slot, int64_t n_slots,
                        double* log_post_store, double* scratch_x) {
  if (!ctx || !terms || !blocks || n_burn < 0 || n_iter < 0 || n_thin < 1 || n_slots < 1 || first_slot < 0 || !x_store ||
      !scratch_x || x_slot_stride < ctx->n_chains * ld_x)
    return OMC_INVALID_ARG;
  const int64_t C = ctx->n_chains;
  omc_gamma_block b[OMC_MAX_TERMS];
  // mcmc.py:97-98: every iteration, burn-in included, is n_thin sweeps
  const int64_t burn = n_burn * n_thin, total = burn + n_iter * n_thin;
  if (n < 1 || ld_x < n) return OMC_INVALID_ARG;
  if (ctx->run_sweeps_per_launch > 1 && takes_wg_per_chain(ctx, n) && C * (int64_t)OMC_RUN_MAX < (int64_t)1 << 31) {
    // Several sweeps per launch: workgroup (sweep, chain) = block sweep * C + chain.  A chain's sweep s+1 needs only the
    // scales its sweep s drew; they travel through the chain's hand-over line (see OMC_HANDOFF_WORDS).  Blocks are
    // dispatched in index order, so a producer is always on the chip before its consumer; the consumer's wait is
    // bounded anyway and a hand-over that never came is reported by omc_ctx_status.  What this buys: the ramp, tail
    // and boundary of a launch (7.4 us against 21 us per round of workgroups) are paid once per OMC_RUN_MAX sweeps.
    TriArgs A{};
    args_defaults(ctx, &A, n);
    if (!terms_to_dev(terms, &A.T, &A.cc)) return OMC_INVALID_ARG;
  if (has_center_chain(A.cc) && (A.cc.k < 0 || !takes_wg_per_chain(ctx, n) || A.cc.ld < n)) return OMC_UNSUPPORTED;
    for (int k = 0; k < A.T.n_terms; ++k) {
      const omc_gamma_block& bk = blocks[k];
      GammaDev& g = A.gb[k];
      g.enabled = bk.enabled ? 1 : 0;
      if (g.enabled) {
        if (!terms->scale[k] || bk.n_pos < 0 || !(bk.a0 + 0.5 * (double)bk.n_pos > 0.0)) return OMC_INVALID_ARG;
        if (log_post_store && !(bk.a0 > 0.0 && bk.b0 > 0.0)) return OMC_INVALID_ARG;
        if (bk.g_inject) return OMC_INVALID_ARG;
      }
      if (log_post_store && !bk.logdet_unscaled) return OMC_INVALID_ARG;
      g.a0 = bk.a0; g.b0 = bk.b0; g.half_npos = 0.5 * (double)bk.n_pos;
      g.lnorm = (g.enabled && log_post_store) ? bk.a0 * log(bk.b0) - lgamma(bk.a0) : 0.0;
      g.g_inject = nullptr; g.store = bk.store;
      g.scale_out = const_cast<double*>(terms->scale[k]);
      g.logdet_unscaled = bk.logdet_unscaled;
      A.gdraw[k] = bk.draw_index;
    }
    OMC_HIP_CHECK(hipSetDevice(ctx->device));
    if (!ctx->d_handoff) {
      const size_t bytes = (size_t)C * OMC_HANDOFF_WORDS * sizeof(unsigned long long);
      OMC_HIP_CHECK(hipMalloc(&ctx->d_handoff.p, bytes));
      OMC_HIP_CHECK(hipMemsetAsync(ctx->d_handoff, 0, bytes, ctx->stream));
      ctx->run_epoch = 1;
    }
    A.handoff = ctx->d_handoff;
    A.ld_x = ld_x;
    A.zero_z = ctx->debug_zero_z;
    A.fused = 1;
    // (the generic instantiation: one sweep per launch, see the kernel)
    const int per = ctx->run_sweeps_per_launch < OMC_RUN_MAX ? ctx->run_sweeps_per_launch : OMC_RUN_MAX;
    // Which form of the launch: one self-restarting workgroup per chain (a chain's sweeps stay on one CU: no dispatch
    // gaps, restart under the epilogue) pays when the chains fill the CUs in whole rounds; otherwise one workgroup per
    // (sweep, chain) -- the dispatcher then balances the CUs sweep by sweep, and with fewer chains than CUs the next
    // sweep of a chain starts on an idle CU under the tail of the previous one (384 chains: 31.4 against 39.2 us per
    // sweep, 128 chains: 19.0 against 19.9; 256 and 1024 chains: the restarting form by 6 % and 3 %).
    const int dev_cus = ctx->dev_cus;
    const int64_t rounds = (C + dev_cus - 1) / dev_cus;
    const bool whole_rounds = C >= dev_cus && (double)C >= 0.95 * (double)(rounds * dev_cus);
    A.reenter = (whole_rounds || ctx->run_reenter_force) ? ctx->run_reenter : 0;
    if (!takes_specialised(ctx, A.T, n) || has_center_chain(A.cc)) A.reenter = 0;  // the generic instantiation: one workgroup per (sweep, chain)
    if (A.reenter && per > 1 && !reentry_abi_ok(ctx)) A.reenter = 0;  // (see k_reentry_probe)
    if (A.reenter && C * (int64_t)per >= ((int64_t)1 << 26)) A.reenter = 0;  // (a restart's register carries sweep * C + chain in 26 bits)
    A.early_draws = (A.reenter == 0 && 2 * C <= dev_cus && !has_center_chain(A.cc)) ? 1 : 0;  // a waiting workgroup per chain has a CU to itself
    // (sweep, chain) grid: two sweeps of one launch must not write the same store slot -- their workgroups are not ordered
    // against each other (the self-restarting form walks a chain's sweeps in order and may lap the ring)
    const int64_t stored_per_launch_max = (A.reenter == 0 && n_slots < per) ? n_slots : per;
    ctx->launch_log_n = 0; ctx->launch_log_total = 0;
    const bool clock_on = ctx->sweep_times && ctx->sweep_times_cap >= OMC_SWEEP_RING_MIN;
    if (ctx->run_ev_begin) OMC_HIP_CHECK(hipEventRecord(ctx->run_ev_begin, ctx->stream));
    for (int64_t t0 = 0; t0 < total;) {
      int k_sw = (int)(total - t0 < per ? total - t0 : per);
      if (stored_per_launch_max < per) {  // end the launch before a store slot would repeat inside it
        int64_t stored_seen = 0;
        for (int i = 0; i < k_sw; ++i) {
          const int64_t t = t0 + i;
          if (t >= burn && ((t - burn + 1) % n_thin == 0) && ++stored_seen > stored_per_launch_max) { k_sw = i; break; }
        }
      }
      for (int i = 0; i < k_sw; ++i) {
        const int64_t t = t0 + i;
        const bool stored = t >= burn && ((t - burn + 1) % n_thin == 0);
        const int64_t it = stored ? (t - burn + 1) / n_thin - 1 : 0;
        const int64_t slot = (first_slot + it) % n_slots;
        A.rec[i].draw = draw_index0 + (uint64_t)t * draws_per_sweep;
        // a draw that is neither stored nor the run's last is not written at all: the next sweep redraws x from its full
        // conditional without reading it (80 KB per chain and sweep of stores that burn-in and thinning would throw away)
        A.rec[i].x = stored ? x_store + slot * x_slot_stride : (t == total - 1 ? scratch_x : nullptr);
        A.rec[i].log_post = (stored && log_post_store) ? log_post_store + slot * C : nullptr;
        A.rec[i].slot_off = stored ? slot * C : -1;
      }
      A.n_sweeps = k_sw;
      // Self-restarting workgroups in blocks: a workgroup walks `block_sweeps` sweeps of its chain, then a fresh one (block
      // index + C, dispatched when a CU falls free) takes the chain over through the global hand-over line.  One block
      // per launch ties a chain to one CU for the whole launch and the launch ends with its slowest CU (four rounds of
      // 20 sweeps: a tail of ~60 us measured by the sweep clock); shorter blocks let the dispatcher level the CUs.
      A.block_sweeps = k_sw;
      if (A.reenter && ctx->run_block_sweeps > 0 && ctx->run_block_sweeps < k_sw) A.block_sweeps = ctx->run_block_sweeps;
      A.epoch = ctx->run_epoch;
      ctx->run_epoch += (uint32_t)k_sw;
      // the non-specialised paths still read these
      A.key = omc_make_key(ctx->seed, A.rec[0].draw, OMC_RNG_NORMAL);
      A.x = A.rec[0].x;
      A.log_post = A.rec[0].log_post;
      if (clock_on) {
        A.sweep_times = ctx->sweep_times; A.sweep_times_cap = ctx->sweep_times_cap; A.sweep_times_pos = ctx->sweep_times_pos;
      }
      const double t_begin = omc_host_clock();
      omc_status st = launch_tridiag(ctx, A);
      if (st != OMC_OK) return st;
      if (ctx->launch_log_n < OMC_LAUNCH_LOG_MAX) {
        omc_ctx::LaunchRec& r = ctx->launch_log[ctx->launch_log_n++];
        r.t_begin = t_begin; r.t_end = omc_host_clock(); r.n_sweeps = k_sw; r.form = A.reenter;
        r.ring_pos = clock_on ? ctx->sweep_times_pos : -1;
      }
      ctx->launch_log_total++;
      if (clock_on) ctx->sweep_times_pos = (ctx->sweep_times_pos + k_sw) % ctx->sweep_times_cap;
      t0 += k_sw;
    }
    if (ctx->run_ev_end) OMC_HIP_CHECK(hipEventRecord(ctx->run_ev_end, ctx->stream));
    return OMC_OK;
  }
  ctx->launch_log_n = 0; ctx->launch_log_total = 0;
  for (int64_t t = 0; t < total; ++t) {
    const bool stored = t >= burn && ((t - burn + 1) % n_thin == 0);
    const int64_t i = stored ? (t - burn + 1) / n_thin - 1 : 0;
    const int64_t slot = (first_slot + i) % n_slots;
    const uint64_t base = draw_index0 + (uint64_t)t * draws_per_sweep;
    for (int k = 0; k < terms->n_terms && k < OMC_MAX_TERMS; ++k) {
      b[k] = blocks[k];
      b[k].draw_index = base + blocks[k].draw_index;
      b[k].store = (stored && blocks[k].store) ? blocks[k].store + slot * C : nullptr;
    }
    const double t_begin = omc_host_clock();
    omc_status st = omc_gmrf_sweep(ctx, n, terms, b, nullptr, 0, nullptr, 0, base,
                                   stored ? x_store + slot * x_slot_stride : scratch_x, ld_x,
                                   (stored && log_post_store) ? log_post_store + slot * C : nullptr);
    if (st != OMC_OK) return st;
    if (ctx->launch_log_n < OMC_LAUNCH_LOG_MAX) {
      omc_ctx::LaunchRec& r = ctx->launch_log[ctx->launch_log_n++];
      r.t_begin = t_begin; r.t_end = omc_host_clock(); r.n_sweeps = 1; r.form = 0; r.ring_pos = -1;
    }
    ctx->launch_log_total++;
  }
  return OMC_OK;
}

int32_t omc_tridiag_takes_center_chain(omc_ctx* ctx, int64_t n) { return (ctx && n >= 1 && takes_wg_per_chain(ctx, n)) ? 1 : 0; }

omc_status omc_tridiag_quadform(omc_ctx* ctx, int64_t n, const omc_tridiag_terms* terms, const double* x,
                                int64_t ld_x, double* quad_out) {
  if (!ctx || n < 1 || !x || ld_x < n || !quad_out) return OMC_INVALID_ARG;
  if (n >= (int64_t)1 << 31) return OMC_UNSUPPORTED;  // (32-bit element indices in the kernel)
  TermsDev T{};
  CentreChain CC{};
  if (!terms_to_dev(terms, &T, &CC)) return OMC_INVALID_ARG;
  if (has_center_chain(CC) && CC.k < 0) return OMC_UNSUPPORTED;
  if (has_center_chain(CC) && CC.ld < n) return OMC_INVALID_ARG;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_tridiag_quadform, dim3((unsigned)ctx->n_chains), dim3(256), 0, ctx->stream, T, CC, n,
                     ctx->n_chains, x, ld_x, quad_out);
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}

omc_status omc_tridiag_matvec(omc_ctx* ctx, int64_t n, const double* diag, const double* off, const double* v,
                              double* out) {
  if (!ctx || n < 1 || !v || !out || v == out) return OMC_INVALID_ARG;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  const int64_t grid = (n + 255) / 256;
  hipLaunchKernelGGL(k_tridiag_matvec, dim3((unsigned)(grid > 2048 ? 2048 : grid)), dim3(256), 0, ctx->stream, n,
                     diag, off, v, out);
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}

omc_status omc_tridiag_matvec_chain(omc_ctx* ctx, int64_t n, const double* diag, const double* off, const double* v, int64_t ld_v,
                                    const double* scale, double* out, int64_t ld_out, int32_t accumulate) {
  if (!ctx || n < 1 || !v || !out || ld_v < n || ld_out < n || v == out) return OMC_INVALID_ARG;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  int64_t gx_ = (n + 255) / 256;
  if (gx_ > 64) gx_ = 64;
  hipLaunchKernelGGL(k_tridiag_matvec_chain, dim3((unsigned)gx_, (unsigned)ctx->n_chains), dim3(256), 0, ctx->stream, n, diag, off, v, ld_v,
                     scale, out, ld_out, (int)accumulate);
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}

omc_status omc_chain_lincomb(omc_ctx* ctx, int64_t n, double a, const double* x, int64_t ld_x, double b, const double* y, int64_t ld_y,
                             double* out, int64_t ld_out) {
  if (!ctx || n < 1 || !x || !y || !out || ld_x < n || ld_out < n || (ld_y != 0 && ld_y < n)) return OMC_INVALID_ARG;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  int64_t gx_ = (n + 255) / 256;
  if (gx_ > 64) gx_ = 64;
  hipLaunchKernelGGL(k_chain_lincomb, dim3((unsigned)gx_, (unsigned)ctx->n_chains), dim3(256), 0, ctx->stream, n, a, x, ld_x, b, y, ld_y,
                     out, ld_out);
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}

omc_status omc_tridiag_logdet(omc_ctx* ctx, int64_t n, const double* diag, const double* off, double* logdet) {
  if (!ctx || n < 1 || !logdet) return OMC_INVALID_ARG;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  if (n > seg_max_n(32)) {  // beyond one workgroup: the plain recurrence on one lane (set-up time only, once per model)
    hipLaunchKernelGGL(k_tridiag_logdet_serial, dim3(1), dim3(64), 0, ctx->stream, n, diag, off, logdet, ctx->d_bad_chain);
    OMC_HIP_CHECK(hipGetLastError());
    return OMC_OK;
  }
  TriArgs A{};
  args_defaults(ctx, &A, n);
  A.T.n_terms = 1;  // (args_defaults has cleared every pointer of the terms)
  A.T.diag[0] = diag;
  A.T.off[0] = off;
  A.C = 1; A.chain_offset = 0;
  A.zero_z = 1;
  A.logdet = logdet;
  // the segmented kernel needs no x storage; use it regardless of the algo option
  launch_seg_any(ctx, A, auto_seg(n));
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}

}  // extern "C"
