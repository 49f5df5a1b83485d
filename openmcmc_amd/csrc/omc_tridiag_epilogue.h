// The sweep's epilogue (omc_tridiag.hip): Normal-Gamma updates, hand-over of the new scales and log-posterior of one chain,
// run by one lane (serial and sub-wave kernels) or spread over the 64 lanes of one wave (workgroup-per-chain kernel).
#pragma once
#include "omc_tridiag_args.h"

__device__ __forceinline__ double fast_rcp(double d) { return omc_rcp_nr(d); }

// Normal-Gamma updates + log_post of one chain, run by one lane (sampler.py:252-288, model.py:57-70)
__device__ __forceinline__ void sweep_epilogue(const TriArgs& A, int64_t c, const double* quad) {
  double lp = 0.0;
  bool failed = false;
  const double nd = (double)A.n;
  _Pragma("unroll") for (int k = 0; k < OMC_MAX_TERMS; ++k) if (k < A.T.n_terms) {
    const GammaDev& g = A.gb[k];
    double s = A.T.scale[k] ? A.T.scale[k][c] : 1.0;
    if (g.enabled) {
      const double a = g.a0 + g.half_npos;
      const double b = g.b0 + 0.5 * quad[k];
      const double sc = (b == 0.0) ? INFINITY : omc_rcp_nr(b);
      const double gd = g.g_inject ? g.g_inject[c] : omc_standard_gamma(g.key, A.chain_offset + c, a, &failed);
      s = gd * sc;
      g.scale_out[c] = s;
      if (g.store) g.store[c] = s;
    }
    if (A.log_post) {
      double lpk = 0.5 * (nd * log(s) + g.logdet_unscaled[0] - nd * 1.8378770664093453 - s * quad[k]);
      if (g.enabled) lpk += g.lnorm + (g.a0 - 1.0) * log(s) - g.b0 * s;
      lp += lpk;
    }
  }
  if (A.log_post) A.log_post[c] = lp;
  if (failed) atomicMin((unsigned long long*)A.bad, (unsigned long long)c);
}

__device__ __forceinline__ double read_lane_d(double v, int l) {  // l wave-uniform
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// log-posterior of one sweep from the per-term scales, quadratic forms and log-determinants: lanes 16 k (k = term)
// hold s, qk, ldet of their term; lane 0 stores the sum (model.py:57-70 -> gmrf.py:321-348, distribution.py:241-261).
// Split from the epilogue so that a self-restarting workgroup can leave it to a wave that has slack (see the kernel).
template <bool DEV = false>
__device__ __forceinline__ void sweep_log_post_wave(const TriArgs& A, int64_t c, int lane, double s, double qk, double ldet,
                                                    double* lp_out) {
  const int k = lane >> 4, j = lane & 15;
  const bool term_on = k < A.T.n_terms;
  GammaDev g;
  if constexpr (DEV) {
    g = A.gb_dev[k];
  } else {
    g = A.gb[0];
#pragma unroll
    for (int t = 1; t < OMC_MAX_TERMS; ++t) {
      if (k == t) g = A.gb[t];
    }
  }
  double lp = 0.0;
  if (term_on && j == 0) {
    const double nd = (double)A.n;
    // the lean fdlibm log kernel (< 1 ulp) for finite positive scales, the library's log for the rest (zero-rate guard:
    // scale = inf)
    const double ls = (s > 0.0 && s < INFINITY) ? omc_log_unit(s) : log(s);
    lp = 0.5 * (nd * ls + ldet - nd * 1.8378770664093453 - s * qk);
    if (g.enabled) lp += g.lnorm + (g.a0 - 1.0) * ls - g.b0 * s;
  }
  // terms are summed in order 0,1,2,3 as the serial epilogue does
  const double t0 = read_lane_d(lp, 0), t1 = read_lane_d(lp, 16), t2 = read_lane_d(lp, 32), t3 = read_lane_d(lp, 48);
  if (lane == 0) lp_out[c] = ((t0 + t1) + t2) + t3;
}

// The same epilogue spread over the 64 lanes of one wave (the workgroup-per-chain kernel runs it on
// wave 0 while the other waves are already storing x): lanes 16k..16k+15 belong to term k and each
// evaluates one Marsaglia-Tsang attempt; the lowest accepted attempt is the serial answer.
// The same epilogue spread over the 64 lanes of one wave (the workgroup-per-chain kernel runs it on
// wave 0): lanes 16k..16k+15 belong to term k.
//
// Part 1, `sweep_gamma_draws_wave`: the standard-gamma draws Gamma(a,1).  They depend only on the
// prior shape and the node count, not on the data, so the kernel makes them at its very start, in the
// shadow of the first global loads; each lane evaluates one Marsaglia-Tsang attempt, the lowest
// accepted attempt is the serial answer.  Part 2, `sweep_epilogue_wave`: scale by 1/b once the
// quadratic forms are known, store, log_post.
template <bool DEV = false>
__device__ __forceinline__ double sweep_gamma_draws_wave(const TriArgs& A, int64_t c, int lane, bool* failed, int sw = 0) {
  const int k = lane >> 4, j = lane & 15;
  const bool term_on = k < A.T.n_terms;
  GammaDev g;
  uint64_t gdr;
  if constexpr (DEV) {
    g = A.gb_dev[k];
    gdr = A.gdraw_dev[k];
  } else {
    g = A.gb[0];
    gdr = A.gdraw[0];
#pragma unroll
    for (int t = 1; t < OMC_MAX_TERMS; ++t)
      if (k == t) { g = A.gb[t]; gdr = A.gdraw[t]; }
  }
  g.key = sweep_gamma_key(A, sw, g, gdr);
  const bool draw = term_on && g.enabled;
  double gd = 0.0;
  if (__ballot(draw) == 0ull) return gd;
  if (draw && g.g_inject) {
    gd = g.g_inject[c];
  } else if (draw) {
    const omc_gamma_prep p = omc_gamma_prepare(g.key, A.chain_offset + c, g.a0 + g.half_npos);
    double v = 0.0;
    // Attempt 0 alone first: it is accepted with probability > 0.95 (-> 1 for large shapes), mostly by the
    // log-free squeeze test, and with one lane per term active the wave rarely has to walk the log branch
    // that some lane of a full 16-attempt evaluation nearly always needs.
    bool ok = (j == 0) && omc_gamma_attempt(g.key, A.chain_offset + c, p, 0u, v);
    const unsigned long long first = __ballot(ok), want = __ballot(j == 0);
    if (first != want) {  // wave-uniform: some term's first attempt was rejected -> evaluate the other 15 as well
      if (j != 0) ok = omc_gamma_attempt(g.key, A.chain_offset + c, p, (uint32_t)j, v);
    }
    const unsigned long long m = (__ballot(ok) >> (16 * k)) & 0xffffull;  // accepted attempts of this group
    if (m == 0ull) {  // astronomically rare: continue serially on the group's first lane
      if (j == 0) {
        ok = false;
        for (uint32_t at = 16; at < 256 && !ok; ++at) ok = omc_gamma_attempt(g.key, A.chain_offset + c, p, at, v);
        *failed = !ok;
        gd = ok ? v : p.boost * p.d;
      }
    } else {
      gd = __shfl(v, __ffsll((long long)m) - 1 + 16 * k, 64);
    }
  }
  return gd;
}

template <bool DEV = false>
__device__ __forceinline__ void sweep_epilogue_wave(const TriArgs& A, int64_t c, double q0, double q1, double q2, double q3,
                                                    double s_old, double ldet, double gd, bool failed, int lane, int sw = 0,
                                                    unsigned long long* lds_hand = nullptr, bool defer_lp = false,
                                                    double* lds_q = nullptr) {
  const int k = lane >> 4, j = lane & 15;
  const bool term_on = k < A.T.n_terms;
  // per-lane copy of this lane's term, selected with compile-time indices (a dynamically indexed
  // kernel-argument array would be spilled to scratch)
  GammaDev g;
  double s = s_old;  // this lane's term; scalars were loaded before the quad phase
  if constexpr (DEV) {
    g = A.gb_dev[k];
  } else {
    g = A.gb[0];
#pragma unroll
    for (int t = 1; t < OMC_MAX_TERMS; ++t) {
      if (k == t) g = A.gb[t];
    }
  }
  const double qk = (k == 0) ? q0 : ((k == 1) ? q1 : ((k == 2) ? q2 : q3));
  if (!term_on) s = 1.0;
  double* const lp_out = sweep_log_post(A, sw);
  // deferred log-posterior: the quadratic forms go to LDS ahead of the scale granules (one wave's LDS writes land in
  // order: whoever has seen the granules finds these)
  if (lp_out && defer_lp && term_on && j == 0) __hip_atomic_store(lds_q + k, qk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (term_on && g.enabled) {
    const double b = g.b0 + 0.5 * qk;
    s = gd * ((b == 0.0) ? INFINITY : omc_rcp_nr(b));  // sampler.py:285-287
    if (j == 0) {
      if (run_mode(A)) {  // hand the new scale to the workgroup of the chain's next sweep (same launch): FIRST -- a consumer
                          // on another CU waits for exactly these stores, and vector-memory operations leave in order
        const uint32_t tag = A.epoch + (uint32_t)sw + 1u;
        unsigned long long* h = A.handoff + c * OMC_HANDOFF_WORDS + 2 * k;
        const unsigned long long lo = ((unsigned long long)tag << 32) | (uint32_t)__double2loint(s);
        const unsigned long long hi = ((unsigned long long)tag << 32) | (uint32_t)__double2hiint(s);
        if (lds_hand) {  // self-restarting workgroup: the consumer is this workgroup -- the same granules through LDS
          __hip_atomic_store(lds_hand + 2 * k, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          __hip_atomic_store(lds_hand + 2 * k + 1, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        __hip_atomic_store(h, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(h + 1, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      // the caller's scale array: written by the launch's last sweep only (two XCDs' write-through stores to one
      // address within a launch have no defined order)
      if (!run_mode(A) || sw == A.n_sweeps - 1) g.scale_out[c] = s;
      double* const st = sweep_gamma_store(A, sw, g);
      if (st) st[c] = s;
    }
  }
  if (lp_out && !defer_lp) sweep_log_post_wave<DEV>(A, c, lane, s, qk, ldet, lp_out);
  if (failed) atomicMin((unsigned long long*)A.bad, (unsigned long long)c);
}
