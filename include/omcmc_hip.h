/*
 * omcmc_hip.h -- C ABI of libomcmc_hip.so, the MI355X (gfx950) sampler core.
 *
 * The reference (sede-open/openMCMC v1.0.7) is pure Python and has no FFI: the boundary it
 * offers is the duck-typed plugin API MCMCSampler.sample(state)->state called from
 * MCMC.run_mcmc (mcmc.py:97-100).  This header is what a ctypes binding for that path needs:
 * every entry point replaces the arithmetic behind one group of reference call sites, cited
 * per function as file:line relative to /root/reference/src/openmcmc/.  INTEGRATION.md shows
 * the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C, no torch / STL types; every `const double*` / `double*` is a DEVICE pointer
 *     (hipMalloc, or torch.Tensor.data_ptr() of a float64 ROCm tensor) unless marked [host];
 *   - "C" = number of chains held by the context; per-chain vectors are chain-major:
 *     element i of chain c lives at base[c*ld + i] (ld >= n, leading stride in elements);
 *     per-chain scalars are arrays of length C; vectors shared by all chains have length n;
 *   - all arithmetic is IEEE fp64;
 *   - calls on one context are issued to that context's HIP stream and return without
 *     synchronising; numerical failures (non-positive pivot) are latched on the device and
 *     read with omc_ctx_status(), which synchronises;
 *   - every function returns an omc_status; nothing is retained after omc_ctx_destroy;
 *   - every entry point that consumes randomness takes an optional pointer to injected draws
 *     (the parity tests replay the reference's draws through it) and otherwise uses the
 *     in-kernel Philox4x32-10 stream keyed by (seed, global chain id, draw_index), so results
 *     do not depend on how chains are sharded over GPUs.
 */
#ifndef OMCMC_HIP_H
#define OMCMC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  OMC_OK = 0,
  OMC_INVALID_ARG = 1,  /* -> ValueError  (gmrf.py:508-509, gmrf.py:149-150)                */
  OMC_NOT_POSDEF = 2,   /* -> numpy.linalg.LinAlgError (gmrf.py:518 dense fallback raises)   */
  OMC_HIP_ERROR = 3,    /* -> RuntimeError                                                   */
  OMC_UNSUPPORTED = 4   /* -> NotImplementedError                                            */
} omc_status;

typedef struct omc_ctx omc_ctx;

#define OMC_MAX_TERMS 4
#define OMC_SELECT_MAX 8   /* state entries per omc_chain_select_multi call */

/* A conditional precision in "shared structure x per-chain scalar" form
 *     Q_c = sum_k scale[k][c] * M_k,   M_k symmetric tridiagonal, shared by all chains,
 *     rhs_c = sum_k scale[k][c] * rhs[k]  (+ optional per-chain vector),
 * which is what NormalNormal.sample assembles from ScaledMatrix precisions (sampler.py:176-192,
 * parameter.py:329): term 0 is usually the prior (lambda*P, rhs = P m), the others likelihoods
 * (tau*W, rhs = A'W(y-d)).  center[k] is the vector the quadratic form of term k is taken
 * around: quad[k][c] = (x_c - center_k)' M_k (x_c - center_k), the quantity NormalGamma.sample
 * needs (sampler.py:276,284) and Normal.log_p reuses (gmrf.py:343-344).                    */
typedef struct {
  int32_t n_terms;                      /* 1..OMC_MAX_TERMS                                  */
  const double* diag[OMC_MAX_TERMS];    /* [n]   shared; NULL = all ones                     */
  const double* off[OMC_MAX_TERMS];     /* [n-1] shared; NULL = zeros (diagonal M_k)         */
  const double* rhs[OMC_MAX_TERMS];     /* [n]   shared M_k m_k;  NULL = zeros               */
  const double* center[OMC_MAX_TERMS];  /* [n]   shared m_k;      NULL = zeros               */
  const double* scale[OMC_MAX_TERMS];   /* [C]   per-chain scalar; NULL = 1                  */
  /* Per-chain part of a term's centre (ABI 2): a hierarchical model's prior mean that is itself sampled, or a
   * sampled response whose mean is the parameter (sampler.py:181-192 with state[...] differing per chain).  Term k
   * is then centred at center[k] + center_chain[k][c]:  rhs_c += scale[k][c] * M_k center_chain[k][c]  (formed
   * inside the launch: no product vector travels through memory) and quad[k][c] is taken around that centre.
   * NULL = none; at most ONE term of a call may have one.  Taken by the workgroup-per-chain form of the draw
   * (omc_tridiag_takes_center_chain) and by omc_tridiag_quadform; every other entry point -- and a call with two
   * such terms -- returns OMC_UNSUPPORTED.                                                                */
  const double* center_chain[OMC_MAX_TERMS];  /* [C][ld_center_chain]                        */
  int64_t ld_center_chain;
} omc_tridiag_terms;

/* ---- context ---------------------------------------------------------------------------- */

/* device: HIP device ordinal.  stream: the hipStream_t every call of this context is issued to
 * (e.g. torch.cuda.current_stream().cuda_stream; 0 is the legacy default stream); with
 * create_stream != 0 `stream` is ignored and the library creates and owns a non-blocking stream.
 * chain_id_offset: global id of local chain 0 (rank * chains_per_rank), used only to key the
 * random stream.                                                                             */
omc_status omc_ctx_create(int32_t device, int64_t n_chains, uint64_t seed, int64_t chain_id_offset,
                          void* stream, int32_t create_stream, omc_ctx** out);
omc_status omc_ctx_destroy(omc_ctx* ctx);
/* Synchronises the stream.  *first_bad_chain = -1 if no failure has been latched since the
 * last call, else the smallest LOCAL chain index whose factorisation met a non-positive pivot
 * (returns OMC_NOT_POSDEF; the latch is cleared).                                            */
omc_status omc_ctx_status(omc_ctx* ctx, int64_t* first_bad_chain);
omc_status omc_ctx_synchronize(omc_ctx* ctx);
/* Options, by name.  Every option is listed here with the values it accepts and its default; a value outside them and an
 * unknown name return OMC_INVALID_ARG and change nothing.  (One table in the library holds the names and ranges:
 * openmcmc_amd/csrc/omc_options.h.)
 * Tridiagonal draw:
 *   "tridiag_algo"          0..2, default 0: 0 auto, 1 serial lane-per-chain, 2 segmented.
 *   "tridiag_seg"           0, 8, 10, 16, 20 or 32, default 0: nodes per lane of the segmented kernel, 0 auto.
 *   "tridiag_generic"       any value, kept as value != 0, default 0: 1 = never use the instantiation specialised for the two-term
 *                           smoother structure (cross-checks).
 *   "tridiag_quad_skip"     0..15, default 0: bit k set = the generic workgroup-per-chain draw skips term k's fused quadratic form
 *                           (a hierarchical sweep knows which of them a later block will invalidate); that quad_out entry is then
 *                           meaningless.
 *   "tridiag_newton_max"    0..64, default 4: Newton corrections of the segment joins before the sequential fallback takes over;
 *                           0 forces it.
 *   "tridiag_perturb_ppb"   0..1 000 000 000, default 0 (tests): relative error, in 1e-9, put on the segments' start pivots so that
 *                           the join test must reject them.
 *   "debug_zero_z"          any value, kept as (int)value, default 0 (timing what-if only): non-zero = the fused tridiagonal sweeps
 *                           skip the generation of their normal draws and use zeros; the results are not draws.
 * omc_gmrf_run:
 *   "run_sweeps_per_launch" 1..32, default 32: sweeps omc_gmrf_run issues per launch.
 *   "run_reenter"           0..2, default 2: within such a launch a chain's workgroup restarts itself for the next sweep instead of
 *                           one workgroup per sweep and chain; 2: without a barrier in front of the restart, the scales handed from
 *                           sweep to sweep through LDS.  By default the restarting form is taken when the chains fill the CUs in
 *                           whole rounds and the (sweep, chain) grid otherwise; an explicit setting holds for every chain count.
 *   "run_block_sweeps"      0..32, default 0: sweeps a self-restarting workgroup walks before a fresh workgroup takes over; 0 = all
 *                           sweeps of the launch.
 *   "run_event_begin", "run_event_end"   any value, default 0: a caller-owned hipEvent_t (as an integer; 0 = none) that
 *                           omc_gmrf_run records on the context's stream in front of its first / behind its last launch
 *                           (several-sweeps-per-launch route).
 *   "sweep_times_cap", then "sweep_times_ptr"   the sweep clock: capacity (in sweeps; 0 or >= 64, default 0) and device address
 *                           (any value, default 0 = off; a non-zero address needs a capacity >= 64) of a caller-owned ring
 *                           [cap][C][2] of uint64: wave 0 of the workgroup of every (sweep, chain) leaves the device's
 *                           constant-rate counter (s_memrealtime; rate: counter "wall_clock_khz") at its entry and at its exit in
 *                           record (position + sweep) mod cap.  The position restarts at 0 when either option is set and advances
 *                           by the sweeps of every launch (counter "sweep_times_pos"); a change of the capacity switches the clock
 *                           off until a pointer is given for the new one.  One 16-byte store per workgroup and sweep.
 *   "stamps_ptr"            any value, default 0 = off (diagnostic): device address of a caller-owned buffer [C][16][16] of uint64
 *                           for the phase stamps of the segmented tridiagonal kernel, and in the library built with
 *                           OMC_KERNEL_STAMPS of k_band_blocked and k_chol_panel.
 * Store summaries:
 *   "diag_algo"             0..2, default 0: 0 auto; 1 the short-series form of omc_store_rhat_ess, M <= 64; 2 its blocks of lags.
 *   "hist_algo"             0..1, default 0: 1 = omc_store_histogram always finds the bin by bisection, also with evenly spaced
 *                           edges: same counts.
 *   "reduce_algo"           0..2, default 0: 0 auto; 1 omc_store_reduce takes the short-row form, rows staged in LDS, where a row
 *                           fits; 2 always a wave per row: same results, SUM to rounding.
 *   "hist2d_algo"           0..3, default 0: bit 0 = omc_store_histogram2d always takes the direct form, atomic adds to the output
 *                           without counters in LDS; bit 1 = it always finds the bins by bisection; same counts either way.
 *   "rank_tile"             0 or a power of two 64..8192, default 0 = 8192: keys of an LDS tile of the sort behind
 *                           omc_store_ranks; same results bit for bit.
 *   "rank_chunk"            >= 0 (int64), default 0 = auto: the elements omc_store_ranks / omc_store_rank_diagnostics /
 *                           omc_store_hdi / omc_store_autocorr work on at a time.
 *   "autocorr_slice"        >= 0 (int64), default 0 = 2048: the rows of a time slice of omc_store_autocorr; same results to
 *                           rounding.
 * Band route:
 *   "band_algo"             0..3, default 0: 0 auto; 1 narrow bands one lane per chain in ONE piece; 2 one workgroup per chain, a
 *                           column per step; 3 one workgroup per chain in blocks of 16 columns, the next block factorised ahead, the
 *                           window update on the matrix cores -- auto takes it from w = 9, and from w = 4 on up to 3072 chains,
 *                           where a lane per chain leaves the SIMDs to lone waves.
 *   "band_seg_overlap"      8..65536, default 192: columns of warm-up before a segment of the segmented narrow-band route.
 *   "band_seg_count"        0 or 2..128, default 0: the number of segments of that route, 0 = chosen for the device's SIMDs; same
 *                           results to rounding.
 *   "band_blocked_threads"  0, 4, 8, 16 or 512, default 0: the blocked band kernel picks its form by what fits a CU -- four waves
 *                           per chain for bands narrower than 16, 128-register forms with several workgroups to a CU when there are
 *                           more chains than CUs; 512 keeps eight waves and one workgroup per CU, 4 / 16 / 8 force the
 *                           128-register forms: same results to rounding.
 * Dense route and design-matrix helpers:
 *   "dense_overlap"         0..1, default 1: the blocked dense factorisation runs the two halves of the chains on two streams,
 *                           forked from and joined into the context's stream by events; bit-identical results.
 *   "dense_use_rocsolver"   any value, kept as value != 0, default 0: 1 = rocSOLVER's potrf instead of the blocked route
 *                           (cross-checks).
 *   "dense_blocked_min"     1..32768, default 144: smallest order that takes the blocked factorisation; rocSOLVER's small kernels
 *                           below.
 *   "dense_panel_old"       0..1, default 0: 1 = the blocked factorisation's panel as ONE kernel per block column, as in rounds
 *                           1-3, instead of the register-resident diagonal factor + matrix-core row update; same factor bit for
 *                           bit (cross-checks and A/B timing).
 *   "spectral_use_rocblas"  any value, kept as value != 0, default 0: 1 = the products of omc_dense_spectral_sample through
 *                           rocBLAS DGEMM instead of the library's own fp64 MFMA GEMM (cross-checks; the own products give a chain
 *                           the same bits in a context of any size).
 *   "gram_use_rocblas"      any value, kept as value != 0, default 0: 1 = omc_gram through rocBLAS (a scaled copy of X and a
 *                           DGEMM) instead of the library's own MFMA kernel (cross-checks).
 * Metropolis-Hastings steps:
 *   "mh_gemm_ksplit"        1, 2 or 4, default 4: groups of four waves per workgroup that cut the contraction of the steps' own
 *                           small-state GEMM; same results to rounding.
 *   "mh_use_rocblas"        any value, kept as value != 0, default 0: 1 = the products of the fused steps through rocBLAS DGEMM
 *                           instead of the own GEMM (cross-checks).                                                        */
omc_status omc_ctx_set_option(omc_ctx* ctx, const char* name, int64_t value);
/* Diagnostic counters, by name (synchronises): "tridiag_join_fallbacks" = chain-updates of the segmented
 * tridiagonal kernel whose pivot joins did not meet the Newton tolerance within its iteration limit and were
 * made consistent by the sequential recurrence instead (same pivots as the serial kernel; slow, rare);
 * "band_join_retries" = groups of 64 chains of the segmented narrow-band route whose segment joins did not close
 * within the warm-up and were redone with four times the warm-up; "band_join_fallbacks" = those that did not close
 * then either and were factorised in one piece instead; "run_handoff_timeouts" = sweeps of a several-sweeps launch whose
 * scales never arrived from the chain's previous sweep (that sweep and the chain's later ones then run on NaN scales, and
 * omc_ctx_status reports the run as failed).  Not counters, no synchronisation: "wall_clock_khz" (rate of the sweep clock),
 * "sweep_times_pos"; "reenter_abi_ok" = 1 if the kernel descriptors of the loaded code object ask the dispatcher for exactly the
 * entry state a self-restarting workgroup reproduces (read back from the device on first use; 0 switches "run_reenter" off
 * for the process).                                                                                             */
omc_status omc_ctx_counter(omc_ctx* ctx, const char* name, int64_t* value);
/* Launch log of the LAST omc_gmrf_run call on this context [host]: *n_launches = kernel launches it issued; for the first
 * min(cap, 64) of them out[5 i .. 5 i + 4] = {host CLOCK_MONOTONIC seconds just before and just after the launch call,
 * sweeps in the launch, launch form (0: one workgroup per (sweep, chain); 1, 2: self-restarting workgroups), ring position
 * of the launch's first sweep in the sweep clock or -1}.  Together with the sweep clock it tells where the time of a slow
 * run went: the host issuing late, the queue starting late, or sweeps that ran long (and which chains').          */
omc_status omc_ctx_launch_log(omc_ctx* ctx, double* out, int64_t cap, int64_t* n_launches);
/* [host, no GPU] The test behind "reenter_abi_ok", on three words of an AMDGPU kernel descriptor (bytes 4-7, 52-55 and
 * 56-59: PRIVATE_SEGMENT_FIXED_SIZE, COMPUTE_PGM_RSRC2, kernel code properties | kernarg preload spec << 16): 1 if a
 * workgroup of that kernel is handed exactly s[0:1] = kernel-argument pointer, s2 = workgroup id x, v0 = work-item id and
 * has no private segment -- the entry state omc_gmrf_run's self-restarting workgroups reproduce by hand.  The build-time
 * test (tests/test_kernel_resources.py) feeds it the descriptors of the compiled code object.                        */
int32_t omc_reentry_descriptor_ok(uint32_t private_segment_fixed_size, uint32_t compute_pgm_rsrc2, uint32_t properties_and_preload);
const char* omc_last_error(void);          /* [host] text of the last HIP failure, thread-local */
int32_t omc_abi_version(void);

/* ---- Normal/GMRF conjugate-Gibbs draw, tridiagonal precision -------------------------------
 * Replaces, for every chain at once, gmrf.sample_normal_canonical (gmrf.py:167-198):
 *   L = sparse_cholesky(Q) (gmrf.py:489-520), mu = cho_solve((L,True), b) (gmrf.py:437-462),
 *   x = mu + solve(L', z) (gmrf.py:29-61, 414-434),  z ~ N(0, I),
 * with Q and b assembled as in NormalNormal.sample (sampler.py:176-192).
 *   rhs_chain  [C][ld_rhs] optional per-chain addition to b (NULL = none)
 *   z_inject   [C][ld_z]   injected N(0,1) draws (NULL = generate, keyed by draw_index)
 *   x_out      [C][ld_x]   the draw
 *   mean_out   [C][ld_mean] optional mu = Q^{-1} b (NULL = skip)
 *   quad_out   [n_terms][C] optional quadratic forms around center[k] (NULL = skip)
 *   logdet_out [C]         optional log det Q_c = 2 sum log L_ii (NULL = skip)
 * Chains longer than one workgroup takes (n > 16 384) go through the segmented band kernels (omc_band_sample_canonical,
 * w = 1), and that route is stricter in two ways: z_inject must not alias x_out or mean_out (OMC_INVALID_ARG; the
 * workgroup-per-chain kernels accept z_inject == x_out), and the option "tridiag_quad_skip" is ignored -- every requested
 * quad_out row is computed (by omc_tridiag_quadform behind the draw).                                  */
omc_status omc_tridiag_sample_canonical(omc_ctx* ctx, int64_t n, const omc_tridiag_terms* terms,
                                        const double* rhs_chain, int64_t ld_rhs,
                                        const double* z_inject, int64_t ld_z, uint64_t draw_index,
                                        double* x_out, int64_t ld_x,
                                        double* mean_out, int64_t ld_mean,
                                        double* quad_out, double* logdet_out);

/* ---- one whole Gibbs sweep of the "GMRF smoother" block structure in ONE launch ------------
 * Equivalent to the sampler list [NormalNormal(x), NormalGamma(scale_0), NormalGamma(scale_1), ...]
 * of MCMC.run_mcmc (mcmc.py:99-100) followed by the per-iteration bookkeeping (mcmc.py:105-108),
 * for a Gaussian block whose conditional precision is given by `terms`:
 *   1. x_c ~ N(Q_c^{-1} b_c, Q_c^{-1})                      (as omc_tridiag_sample_canonical)
 *   2. for every term k with blocks[k].enabled: scale[k][c] ~ Gamma(a0 + n_pos/2,
 *      rate = b0 + quad_k/2), written IN PLACE into terms->scale[k] (and to blocks[k].store)
 *      (as omc_normal_gamma_update with blocks[k].draw_index);
 *   3. log_post_out[c] = sum_k log N(. ; center_k, (scale_k M_k)^{-1}) + sum_{k enabled}
 *      log Gamma(scale_k; a0, b0) with the NEW scales (model.py:57-70), if log_post_out != NULL;
 *      needs blocks[k].logdet_unscaled = device scalar log det M_k for every term.
 * The draw goes straight to x_out, which may be a slab of the device-resident store.         */
typedef struct {
  int32_t enabled;                /* 0: scale[k] is a fixed input, no prior term in log_post   */
  double a0, b0;                  /* Gamma prior shape, rate (sampler.py:278-279)               */
  int64_t n_pos;                  /* #{diag(M_k) > 0}  (sampler.py:283)                         */
  const double* g_inject;         /* [C] injected Gamma(a,1) draws, or NULL                     */
  uint64_t draw_index;            /* keys this block's gamma stream when g_inject == NULL       */
  double* store;                  /* [C] optional copy of the new scale (store[param]), or NULL */
  const double* logdet_unscaled;  /* device scalar log det M_k; NULL allowed iff no log_post    */
} omc_gamma_block;

/* 1 if omc_tridiag_sample_canonical / omc_gmrf_sweep accept terms->center_chain for chains of n nodes under the
 * context's current options (the workgroup-per-chain form of the kernel), else 0.                            */
int32_t omc_tridiag_takes_center_chain(omc_ctx* ctx, int64_t n);

/* The log-posterior of a sweep in ONE launch: out[c] = host_const + sum over the pieces, in the order given, of
 *   kind 0  0.5 (n log s_c + mult * logdet - n log 2 pi - s_c quad_c)      Normal.log_p with a scalar x shared-matrix precision
 *           (location_scale.py:145-167 -> gmrf.py:321-348; quad from omc_*_quadform or a draw's fused form), s = 1 if scale NULL
 *   kind 1  log Gamma(x_c; shape, rate)                                     Gamma.log_p (distribution.py:241-261)
 * -- the same arithmetic, piece by piece and in the same order, as omc_scaled_gauss_logpdf / omc_gamma_logpdf called with
 * accumulate (model.py:57-70 sums the members one after the other).  At most OMC_LOGP_MAX pieces.                          */
#define OMC_LOGP_MAX 8
typedef struct {
  int32_t kind;
  double n;                /* kind 0: dimension x replicates                       */
  const double* scale;     /* kind 0: [C] or NULL                                  */
  const double* logdet;    /* kind 0: device scalar log det M                      */
  double logdet_mult;      /* kind 0: usually 1 (replicates: their number)         */
  const double* quad;      /* kind 0: [C]                                          */
  const double* x;         /* kind 1: [C]                                          */
  double shape, rate;      /* kind 1                                               */
} omc_logp_piece;
omc_status omc_log_post_sum(omc_ctx* ctx, int32_t n_pieces, const omc_logp_piece* pieces /* host */, double host_const,
                            double* out);

omc_status omc_gmrf_sweep(omc_ctx* ctx, int64_t n, const omc_tridiag_terms* terms,
                          const omc_gamma_block* blocks /* [n_terms], host */,
                          const double* rhs_chain, int64_t ld_rhs,
                          const double* z_inject, int64_t ld_z, uint64_t draw_index,
                          double* x_out, int64_t ld_x, double* log_post_out);

/* The whole MCMC.run_mcmc loop (mcmc.py:97-111) for that sampler list, issued from C: (n_burn + n_iter) *
 * n_thin sweeps back to back with no host work in between.  Sweep t (0-based) uses draw index
 * draw_index0 + t * draws_per_sweep for the Gaussian block and that base + blocks[k].draw_index for
 * gamma block k.  Iteration i (the last sweep of every group of n_thin after the burn-in) is stored:
 *   x      -> x_store + slot * x_slot_stride        ([C][ld_x] slab; written directly by the sweep)
 *   scale  -> blocks[k].store + slot * C            (when blocks[k].store != NULL)
 *   log_p  -> log_post_store + slot * C             (when != NULL)
 * with slot = (first_slot + i) % n_slots.  A sweep that is not stored leaves its draw in scratch_x [C][ld_x] if it is
 * the last of the run (the state to continue from); the draws of other unstored sweeps may not be written at all.  */
omc_status omc_gmrf_run(omc_ctx* ctx, int64_t n, const omc_tridiag_terms* terms, const omc_gamma_block* blocks,
                        int64_t n_burn, int64_t n_iter, int64_t n_thin, uint64_t draw_index0,
                        uint64_t draws_per_sweep, double* x_store, int64_t ld_x, int64_t x_slot_stride,
                        int64_t first_slot, int64_t n_slots, double* log_post_store, double* scratch_x);

/* quad_out[k][c] = (x_c - center_k)' M_k (x_c - center_k) for an existing x (sampler.py:276-284
 * when the Gaussian block was not just drawn; gmrf.py:343-344).                              */
omc_status omc_tridiag_quadform(omc_ctx* ctx, int64_t n, const omc_tridiag_terms* terms,
                                const double* x, int64_t ld_x, double* quad_out);

/* Shared-vector helpers used once per model, not per sweep:
 *   out = M v for a shared tridiagonal M (rhs[k] = M_k m_k, sampler.py:183)
 *   *logdet [device, 1] = log det M via the same factorisation (gmrf.py:342), status latched */
omc_status omc_tridiag_matvec(omc_ctx* ctx, int64_t n, const double* diag, const double* off,
                              const double* v, double* out);
/* Per-chain vectors on the right-hand side (hierarchical models: a sampled prior mean, a sampled response):
 *   omc_tridiag_matvec_chain: out[c] (+)= scale[c] * M v_c -- the term Q_rsp @ mean of sampler.py:181-183 when the mean is
 *     itself per chain, and W (y_c - d) of sampler.py:190-192 when the response is (M tridiagonal; NULL diag = identity);
 *   omc_chain_lincomb: out[c] = a x_c + b y_c (y per chain, or shared with ld_y = 0): the residual of location_scale.py:
 *     153-160 when both sides of a Normal are per chain; b == 0 means y is not read (an inf or NaN there does not reach out). */
omc_status omc_tridiag_matvec_chain(omc_ctx* ctx, int64_t n, const double* diag, const double* off, const double* v, int64_t ld_v,
                                    const double* scale, double* out, int64_t ld_out, int32_t accumulate);
omc_status omc_chain_lincomb(omc_ctx* ctx, int64_t n, double a, const double* x, int64_t ld_x, double b, const double* y, int64_t ld_y,
                             double* out, int64_t ld_out);
/* dst[c][0..n) = src[c][0..n) for every chain: the current value of a parameter into its slab of the sample store
 * (sampler/sampler.py:89-118, `store[param][:, [iteration]] = state[param]`) -- a copy kernel on the context's stream (the
 * runtime's device-to-device memcpy moved the 82 MB of a 10 000 x 1024 state at 0.26 TB/s).                        */
omc_status omc_chain_copy(omc_ctx* ctx, int64_t n, const double* src, int64_t ld_src, double* dst, int64_t ld_dst);
omc_status omc_tridiag_logdet(omc_ctx* ctx, int64_t n, const double* diag, const double* off,
                              double* logdet);

/* ---- Normal/Normal conjugate-Gibbs draw, DENSE conditional precision ------------------------
 * The same update as omc_tridiag_sample_canonical for Q_c = sum_k scale[k][c] * M_k with M_k shared
 * dense symmetric p x p matrices (NULL = identity): the regression case of NormalNormal.sample where
 * the likelihood Hessian is the Gram matrix G = A' W A (sampler.py:185-186 -> location_scale.py:
 * 238-241) and b = P m + A' W (y - d) (sampler.py:183,190-192).  Per chain: dense Cholesky
 * (gmrf.py:481 np.linalg.cholesky = LAPACK potrf; here rocSOLVER potrf_strided_batched),
 * mu = cho_solve (gmrf.py:462), x = mu + L^{-T} z (gmrf.py:434; the reference calls a general LU
 * solve there, the result is the same triangular solve).  Factors live in a workspace owned by
 * the context (C * p * p doubles, allocated on first use).                                      */
typedef struct {
  int32_t n_terms;                      /* 1..OMC_MAX_TERMS                                  */
  const double* mat[OMC_MAX_TERMS];     /* [p*p] shared symmetric; NULL = identity           */
  const double* rhs[OMC_MAX_TERMS];     /* [p]   shared; NULL = zeros                        */
  const double* scale[OMC_MAX_TERMS];   /* [C]   per-chain scalar; NULL = 1                  */
  const double* diag_chain;             /* [C][p] per-chain diagonal added to Q_c (a mixture prior precision
                                           diag(prec[allocation]), parameter.py:501); NULL = none           */
} omc_dense_terms;

omc_status omc_dense_sample_canonical(omc_ctx* ctx, int64_t p, const omc_dense_terms* terms,
                                      const double* rhs_chain, int64_t ld_rhs,
                                      const double* z_inject, int64_t ld_z, uint64_t draw_index,
                                      double* x_out, int64_t ld_x,
                                      double* mean_out, int64_t ld_mean, double* logdet_out);

/* Spectral route of the same conditional draw for Q_c = a_c I + b_c M with ONE shared symmetric M -- the regression
 * likelihood's Gram matrix next to a scalar prior precision (examples/3, BASELINE configs[1]), where only two scalars
 * differ from chain to chain and from sweep to sweep.  M = V diag(ev) V' once per model (omc_dense_spectral_prepare,
 * rocSOLVER dsyevd), then  mu_c = V diag(1/(a_c + b_c ev)) V' b_c  and  x_c = mu_c + V diag((a_c + b_c ev)^-1/2) z_c:
 * two (three with mean_out) GEMMs over all chains and one scaling kernel instead of C factorisations of order p
 * (p^3/3 flop per chain).  mu_c and log det Q_c = sum_i log(a_c + b_c ev_i) are the reference's values
 * (gmrf.py:196, 339) up to rounding; x_c is a draw from the same N(mu_c, Q_c^-1) but not the reference's
 * path-wise image of z (that is L^-T z, gmrf.py:61): replays with injected draws use omc_dense_sample_canonical.
 *   terms: as above; terms->mat[k_mat] is M, every other term a scaled identity (mat NULL), no diag_chain.       */
omc_status omc_dense_spectral_prepare(omc_ctx* ctx, int64_t p, const double* M, double* V_out, double* ev_out);
omc_status omc_dense_spectral_sample(omc_ctx* ctx, int64_t p, const omc_dense_terms* terms, int32_t k_mat, const double* V,
                                     const double* ev, const double* rhs_chain, int64_t ld_rhs, const double* z_inject,
                                     int64_t ld_z, uint64_t draw_index, double* x_out, int64_t ld_x, double* mean_out,
                                     int64_t ld_mean, double* logdet_out);

/* Design-matrix helpers; X is [n][p] row-major (a NumPy array as is), shared by all chains; w is an
 * optional [n] diagonal weight (NULL = ones).
 *   omc_gram:            G[p][p] = X' diag(w) X                 (location_scale.py:238-241; fp64 MFMA GEMM)
 *   omc_design_rhs:      out[p]  = X' diag(w) y                 (sampler.py:192)
 *   omc_design_predict:  fitted[c][:] = X beta_c                (parameter.py:196; one GEMM for all chains)
 *   omc_weighted_resid_sq: out[c] = (y - f_c)' diag(w) (y - f_c) (sampler.py:276,284)              */
omc_status omc_gram(omc_ctx* ctx, int64_t n, int64_t p, const double* X, const double* w, double* G_out);
omc_status omc_design_rhs(omc_ctx* ctx, int64_t n, int64_t p, const double* X, const double* w,
                          const double* y, double* out);
omc_status omc_design_predict(omc_ctx* ctx, int64_t n, int64_t p, const double* X,
                              const double* beta, int64_t ld_beta, double* fitted, int64_t ld_fitted);
omc_status omc_weighted_resid_sq(omc_ctx* ctx, int64_t n, const double* y, const double* fitted,
                                 int64_t ld_fitted, const double* w, double* out);

/* ---- Metropolis-Hastings on a Gaussian target with a shared constant Hessian -----------------
 * Target Normal("x", mean=mu, precision=Q) with Q dense d x d and mu shared by all chains (cfg4).
 *
 * omc_dense_cholesky: L = chol(scale * A) (lower, LAPACK potrf as gmrf.py:481), *sumlogdiag =
 *   sum_i log L_ii (device scalar); used once per model for L = chol(H / step^2)
 *   (metropolis_hastings.py:345-346) and L_Q = chol(Q) (gmrf.py:339).
 *
 * omc_mala_step: one ManifoldMALA.sample for every chain (metropolis_hastings.py:102-125, 301-373):
 *   g = -Q (x - mu), H = Q (location_scale.py:222-232); m = x + 1/2 (H/step^2)^{-1} g (347);
 *   x' = m + L^{-T} z (317 -> gmrf.py:61); log q = sum log L_ii - 1/2 |L'(. - m)|^2 forward and
 *   reverse (350-373); log alpha = lp' + q_rev - lp - q_fwd (155); accept iff log u < log alpha (173).
 *   As level-3 BLAS on the d x C state matrix.  Because H is constant, the drift matrix
 *   -(H/step^2)^{-1} Q and L^{-T} are formed once per (Q, L, step) (cached in the context, so Q and L
 *   must stay unchanged while they are in use); a step is then 4 GEMMs (the product with L' runs on a copy
 *   of L with an explicitly zero upper triangle).
 * omc_rw_step: one untruncated RandomWalk.sample (metropolis_hastings.py:212-269): x' = x + step z.
 *   The zero-padded copy of LQ is cached in the context the same way (LQ must stay unchanged while in use).
 *   z_inject [C][ld_z] / u_inject [C]: injected N(0,1) / U(0,1) draws (NULL = generate);
 *   accept_count / proposal_count [C] int64 (NULL = not kept): the AcceptRate counters
 *   (metropolis_hastings.py:25-66), INT path: bit-exact.                                        */
omc_status omc_dense_cholesky(omc_ctx* ctx, int64_t d, const double* A, double scale, double* L_out,
                              double* sumlogdiag_out);
omc_status omc_mala_step(omc_ctx* ctx, int64_t d, const double* Q, const double* mu, const double* L,
                         const double* sumlogL, double step, const double* z_inject, int64_t ld_z,
                         const double* u_inject, uint64_t draw_index, double* x, int64_t ld_x,
                         int64_t* accept_count, int64_t* proposal_count);
/* The same step when L = chol(Q / step^2) (what ManifoldMALA factorises for a Gaussian target: H = Q), in whitened
 * coordinates a = L'(x - mu): the drift -(L L')^{-1} Q is then -step^2 I, so
 *   a' = (1 - step^2/2) a + z;  |L'(x-mu)|^2 = |a|^2, |L'(x'-mu)|^2 = |a'|^2, |L'(x'-m)|^2 = |z|^2,
 *   |L'(x-m')|^2 = |a - (1 - step^2/2) a'|^2  -- every term of log alpha (metropolis_hastings.py:155, 350-373) element-wise,
 * and only accepted proposals are mapped back, x = mu + L^{-T} a' (one triangular product; rejected chains keep their x
 * bit for bit).  Same draws and decision rule as omc_mala_step; results agree to the rounding of the two evaluation
 * orders.  The context keeps a for the state at x: state_is_current != 0 promises that x has not been written by anyone
 * else since this function last returned for the same x (otherwise a = L'(x - mu) is recomputed: one more product).
 * L and mu must stay unchanged while in use (omc_mh_invalidate drops what was derived from them).                */
/* log_p_out (both whitened steps; NULL = not wanted): [C] the log density of the target at the state the step leaves behind
 * -- what Model.log_p would evaluate for the one-Normal model of this route (mcmc.py:99-111), taken from the quantities the
 * acceptance test has formed anyway.                                                                                  */
omc_status omc_mala_step_white(omc_ctx* ctx, int64_t d, const double* mu, const double* L, const double* sumlogL, double step,
                               const double* z_inject, int64_t ld_z, const double* u_inject, uint64_t draw_index, double* x,
                               int64_t ld_x, int32_t state_is_current, int64_t* accept_count, int64_t* proposal_count, double* log_p_out);
/* n_steps of omc_mala_step_white in a row -- the loop of MCMC.run_mcmc over a one-sampler model (mcmc.py:97-111) -- issued
 * as ONE launch per block of 32 steps: a chain's whitened state stays in registers for the block, and one triangular
 * product per block maps the block's states back into the store.  Step t draws from stream draw_index0 + t * draw_stride
 * (what the loop would pass as draw_index); results are bit-identical to n_steps single calls (state, counters, log_p).
 *   z_inject [n_steps][C][ld_z], u_inject [n_steps][C]: injected draws (NULL = generate);
 *   x_store    [n_steps][C][d] or NULL: the state after every step (sampler.store of every iteration, sampler.py:89-118);
 *   logp_store [n_steps][C]    or NULL: the target's log density at those states (mcmc.py:108);
 *   x: the current state on entry (see state_is_current), the state after the last step on return; log_p_out [C] or NULL.
 * d <= 2048 (OMC_UNSUPPORTED beyond: use the single step).                                                            */
omc_status omc_mala_run_white(omc_ctx* ctx, int64_t d, const double* mu, const double* L, const double* sumlogL, double step,
                              const double* z_inject, int64_t ld_z, const double* u_inject, uint64_t draw_index0,
                              uint64_t draw_stride, int64_t n_steps, double* x, int64_t ld_x, int32_t state_is_current,
                              double* x_store, double* logp_store, int64_t* accept_count, int64_t* proposal_count, double* log_p_out);
omc_status omc_rw_step(omc_ctx* ctx, int64_t d, const double* mu, const double* LQ, const double* sumlogLQ,
                       double step, const double* z_inject, int64_t ld_z, const double* u_inject,
                       uint64_t draw_index, double* x, int64_t ld_x, int64_t* accept_count,
                       int64_t* proposal_count);
/* The same random-walk step with a = L_Q'(x - mu) carried by the context (LQ = chol(Q)): a' = a + step L_Q' z,
 * log p(x') - log p(x) = (|a|^2 - |a'|^2)/2 -- one triangular product per step instead of two; x' = x + step z is
 * formed exactly as in omc_rw_step.  state_is_current as for omc_mala_step_white.                                  */
omc_status omc_rw_step_white(omc_ctx* ctx, int64_t d, const double* mu, const double* LQ, const double* sumlogLQ, double step,
                             const double* z_inject, int64_t ld_z, const double* u_inject, uint64_t draw_index, double* x,
                             int64_t ld_x, int32_t state_is_current, int64_t* accept_count, int64_t* proposal_count, double* log_p_out);
/* omc_mh_invalidate: drops the matrices cached for the last (Q, L, step) / LQ.  The cache is keyed by device
 * addresses; call this whenever Q, L or LQ were rewritten in place or re-created (a new buffer may land on a recycled
 * address).  The reference has nothing to invalidate: it refactorises every step (metropolis_hastings.py:345-346). */
omc_status omc_mh_invalidate(omc_ctx* ctx);

/* ---- Normal-Gamma conjugate update ---------------------------------------------------------
 * NormalGamma.sample (sampler.py:252-288) for a scalar precision per chain:
 *   a = a0 + n_pos/2, b = b0 + quad[c]/2, out[c] = Gamma(a, scale = 1/b); b == 0 -> scale inf.
 *   g_inject [C] injected standard-gamma draws Gamma(a,1) (NULL = generate, Marsaglia-Tsang). */
omc_status omc_normal_gamma_update(omc_ctx* ctx, double a0, double b0, int64_t n_pos,
                                   const double* quad, const double* g_inject,
                                   uint64_t draw_index, double* out);

/* ---- log-density pieces of Model.log_p (model.py:57-70) ------------------------------------
 * Gaussian with precision scale[c]*M, M shared (location_scale.py:145-167 -> gmrf.py:321-348):
 *   lp = 0.5*(n*log(scale[c]) + logdet_M - n*log(2 pi) - scale[c]*quad[c])
 * Gamma prior (distribution.py:241-261): lp = a log b - lgamma(a) + (a-1) log x - b x.
 * accumulate != 0 adds into out[c] instead of overwriting.                                    */
omc_status omc_scaled_gauss_logpdf(omc_ctx* ctx, int64_t n, const double* scale,
                                   const double* logdet_unscaled /* device, 1 */,
                                   const double* quad, double* out, int32_t accumulate);
omc_status omc_gamma_logpdf(omc_ctx* ctx, const double* x, double shape, double rate,
                            double* out, int32_t accumulate);

/* ---- reversible-jump move bookkeeping (INT / index path: bit-exact) ---------------------------
 * ReversibleJump.get_move_type, get_move_probabilities and the deletion index of death_proposal
 * (reversible_jump.py:310-373, 173) for every chain:
 *   n[c] == n_max -> death; n[c] == 1 -> birth; otherwise birth iff u <= birth_probability, where the
 *   uniform is consumed ONLY in that last case (as in the reference);
 *   p_birth/p_death with the edge cases at n_max, n_max-1, 1, 2;
 *   del_index[c] = randint(0, n[c]) for a death, -1 for a birth.
 *   u_inject [C] / idx_inject [C] (int64): injected draws (NULL = Philox: uniform from block 0,
 *   unbiased bounded integer by Lemire's rejection from block 1).  Any n[c] < 1 or > n_max is
 *   latched as a failure of that chain (the reference raises ValueError for n == 0).           */
omc_status omc_rj_move(omc_ctx* ctx, int64_t n_max, double birth_probability, const int64_t* n,
                       const double* u_inject, const int64_t* idx_inject, uint64_t draw_index,
                       int32_t* birth_out, double* p_birth_out, double* p_death_out, int64_t* del_index_out);
/* The same move with the outputs ReversibleJump.proposal makes of it (reversible_jump.py:122-144, 165-191): count [C] is
 * the float64 count the state holds; count_prop = count +- 1; with d = density_const + density_chain[c] (the log prior
 * density of the last element of every associated parameter, :132,143; density_chain may be NULL)
 *   birth: lq_fwd = log p_birth + d, lq_rev = log p_death;   death: lq_fwd = log p_death, lq_rev = log p_birth + d.  */
omc_status omc_rj_move_densities(omc_ctx* ctx, int64_t n_max, double birth_probability, const double* count,
                                 const double* u_inject, const int64_t* idx_inject, uint64_t draw_index,
                                 const double* density_chain, double density_const, int32_t* birth_out,
                                 int64_t* del_index_out, double* count_prop_out, double* lq_fwd_out, double* lq_rev_out);

/* One draw of a variable-size parameter into its store slab (sampler.py:112-116): dst[c][j] = src[c][j] for
 * j < count[c], NaN beyond, j < width; chain c at src + c*src_chain_stride / dst + c*dst_chain_stride.          */
omc_status omc_store_ragged(omc_ctx* ctx, int64_t width, const double* src, int64_t src_chain_stride, const double* count,
                            double* dst, int64_t dst_chain_stride);

/* ---- banded precisions of any bandwidth (RW2, seasonal, lattice GMRFs) --------
 * The same conditional draw as omc_tridiag_sample_canonical for Q_c = sum_k scale[k][c] * M_k with every M_k
 * symmetric of bandwidth bw[k] <= w (w <= 128), factorised in natural order (the reference's unpermuted SuperLU /
 * LAPACK route, gmrf.py:489-520, so the draw matches path-wise for the same z):
 *   band[k]  [(bw[k]+1) x n], band[k][d*n + i] = M_k[i+d, i] (d-th sub-diagonal contiguous, as scipy's
 *            M.diagonal(-d) padded to n); NULL = identity (bw 0);
 *   rhs[k]   [n] shared M_k m_k or NULL;  scale[k] [C] or NULL = 1;
 *   x = Q^{-1} b + L^{-T} z; mean (optional) = Q^{-1} b; logdet (optional) [C] = log det Q_c.
 * x, mean and z_inject are three different arrays (OMC_INVALID_ARG otherwise: the narrow-band route writes rows of
 * x while other rows' draws are still being read).
 * Uses a per-context workspace of C * n * (w+1) doubles for the factor (twice that on the segmented route).   */
typedef struct {
  int32_t n_terms;
  const double* band[OMC_MAX_TERMS];
  int32_t bw[OMC_MAX_TERMS];
  const double* rhs[OMC_MAX_TERMS];
  const double* scale[OMC_MAX_TERMS];
} omc_band_terms;

omc_status omc_band_sample_canonical(omc_ctx* ctx, int64_t n, int64_t w, const omc_band_terms* terms,
                                     const double* rhs_chain, int64_t ld_rhs, const double* z_inject, int64_t ld_z,
                                     uint64_t draw_index, double* x, int64_t ld_x, double* mean, int64_t ld_mean,
                                     double* logdet);
/* quad[c] = (x_c - center)' M (x_c - center) for one shared band matrix (NormalGamma.sample sampler.py:276,284;
 * Normal.log_p gmrf.py:343-344); band NULL with w = 0 is the identity, center NULL = 0.                      */
omc_status omc_band_quadform(omc_ctx* ctx, int64_t n, int64_t w, const double* band, const double* center,
                             const double* x, int64_t ld, double* quad);
/* out[c] (+)= scale[c] * M v_c for a shared band matrix and per-chain vectors: Q_rsp @ mean with a sampled prior mean
 * (sampler.py:181-183) and W (y_c - d) with a sampled response (sampler.py:190-192) on the band route; band NULL with
 * w = 0 is the identity, scale NULL = 1.                                                                          */
omc_status omc_band_matvec_chain(omc_ctx* ctx, int64_t n, int64_t w, const double* band, const double* v, int64_t ld_v,
                                 const double* scale, double* out, int64_t ld_out, int32_t accumulate);

/* ---- truncated Gaussian full conditional ------------------------------------
 * gmrf.gibbs_canonical_truncated_normal (gmrf.py:201-266), the branch NormalNormal.sample takes when the
 * parameter's prior has domain limits (sampler.py:199-205): ONE scan of single-site updates in index order,
 *   x_i ~ N_[lower_i, upper_i]( (b_i - sum_j Q_ij x_j + Q_ii x_i) / Q_ii, 1/Q_ii ),  x_j already updated for j < i,
 * each by inverse CDF of a uniform (gmrf.py:264 -> scipy truncnorm.rvs == ppf(U)).  x is updated in place
 * (the scan starts from the current state).  Q and b in the same "shared structure x per-chain scalar" forms as
 * the untruncated entry points; lower / upper: device [n] (NULL = unbounded on that side).
 * u_inject [C][ld_u] injected uniforms; in-kernel uniforms are Philox blocks i/2 of (seed, chain, draw_index).
 * The scan is sequential in i by definition, the parallelism is over chains (tridiagonal: one lane per chain;
 * dense: one wave per chain, p <= 8192).  omc_dense_gibbs_truncated takes terms->diag_chain: Q_c gets the per-chain
 * diagonal of a truncated mixture prior (parameter.py:501) and its prec * mean arrives through rhs_chain.                */
omc_status omc_tridiag_gibbs_truncated(omc_ctx* ctx, int64_t n, const omc_tridiag_terms* terms,
                                       const double* rhs_chain, int64_t ld_rhs, const double* lower,
                                       const double* upper, const double* u_inject, int64_t ld_u,
                                       uint64_t draw_index, double* x, int64_t ld_x);
/* the same scan for a banded precision (band storage and terms of omc_band_sample_canonical), one lane per chain */
omc_status omc_band_gibbs_truncated(omc_ctx* ctx, int64_t n, int64_t w, const omc_band_terms* terms, const double* rhs_chain,
                                    int64_t ld_rhs, const double* lower, const double* upper, const double* u_inject, int64_t ld_u,
                                    uint64_t draw_index, double* x, int64_t ld_x);
omc_status omc_dense_gibbs_truncated(omc_ctx* ctx, int64_t p, const omc_dense_terms* terms,
                                     const double* rhs_chain, int64_t ld_rhs, const double* lower,
                                     const double* upper, const double* u_inject, int64_t ld_u,
                                     uint64_t draw_index, double* x, int64_t ld_x);
/* Normal.log_p returns -inf when the response lies outside [lower, upper] (location_scale.py:162-188):
 *   out[c] = -inf for every chain with an element of x[c] below lower or above upper; other chains untouched. */
omc_status omc_domain_penalty(omc_ctx* ctx, int64_t n, const double* x, int64_t ld, const double* lower,
                              const double* upper, double* out);

/* ---- generic Metropolis-Hastings blocks, ragged state, reversible-jump transitions ----------------
 * Ragged parameters (dimension changes under reversible jump: knots, their coefficients, the basis)
 * are held padded to n_max with zeros; count[c] -- the float64 the reference keeps in
 * state["n_basis"] -- is the number of live leading entries of chain c.  `count`/`index` pairs below
 * gate a chain: it takes part iff count == NULL or index < count[c] (RandomWalkLoop over knots:
 * metropolis_hastings.py:286-288 runs range(n_basis) steps, chains with fewer knots sit the step out).
 * `sub` is the first Philox block the call may use within (seed, chain, draw_index): lets one sampler
 * call make several independent draws.
 *
 * omc_rw_propose: RandomWalk.proposal (metropolis_hastings.py:212-269) for p elements per chain,
 *   x[c*x_chain_stride + e*x_elem_stride] -> z[c*z_chain_stride + e*z_elem_stride]:
 *   lower/upper == NULL: z = x + step*N(0,1), lq_fwd = lq_rev = 0 (symmetric, :250-251);
 *   else truncated normal on [lower[e], upper[e]] (device, p each) by inverse CDF of a uniform
 *   (gmrf.py:269-292 -> scipy truncnorm.rvs == ppf(U)), lq_fwd = sum_e log q(z|x), lq_rev = sum_e log q(x|z)
 *   (:255-257 -> gmrf.py:295-318).  step[e*step_elem_stride] device (stride 0 = scalar step).
 *   draw_inject [C][p]: the uniforms (truncated) or normals (untruncated) to use instead of Philox.   */
omc_status omc_rw_propose(omc_ctx* ctx, int64_t p, const double* x, int64_t x_chain_stride,
                          int64_t x_elem_stride, const double* step, int64_t step_elem_stride,
                          const double* lower, const double* upper, const double* count, int64_t index,
                          const double* draw_inject, uint64_t draw_index, uint32_t sub, double* z,
                          int64_t z_chain_stride, int64_t z_elem_stride, double* lq_fwd, double* lq_rev);

/* ManifoldMALA.proposal / _proposal_params / _log_proposal_density (metropolis_hastings.py:301-373) when the Hessian
 * is DIAGONAL per chain (hdiag [C][kmax], e.g. the mixture-Normal prior of a variable-size coefficient vector):
 *   precision = h/step^2, L_jj = sqrt(h_j)/step, m = x + (1/2) precision^{-1} grad;
 *   propose != 0: x_other = m + z / L is WRITTEN (zeros beyond count[c]), lq = log q(x_other | x);
 *   propose == 0: x_other is READ, lq = log q(x_other | x) (the reverse move, with grad / hdiag of the proposed state
 *   passed as x's); log q = sum_j log L_jj - |L'(x_other - m)|^2 / 2.  z_inject [C][kmax] standard normals.      */
omc_status omc_mala_diag(omc_ctx* ctx, int64_t kmax, const double* x, const double* grad, const double* hdiag,
                         const double* count, double step, int32_t propose, const double* z_inject, uint64_t draw_index,
                         uint32_t sub, double* x_other, double* lq);

/* MetropolisHastings._accept_reject_proposal + accept_proposal (metropolis_hastings.py:127-173):
 *   log_alpha = lp_prop + lq_rev - (lp_cur + lq_fwd); accept[c] = log(u) < log_alpha (NaN rejects);
 *   counters (int64, per chain) incremented for participating chains; lq_* / log_alpha / counters may be NULL. */
omc_status omc_mh_accept(omc_ctx* ctx, const double* lp_cur, const double* lp_prop, const double* lq_fwd,
                         const double* lq_rev, const double* count, int64_t index, const double* u_inject,
                         uint64_t draw_index, uint32_t sub, int32_t* accept, double* log_alpha,
                         int64_t* accept_count, int64_t* proposal_count);

/* current_state = prop_state for accepted chains (metropolis_hastings.py:157-159):
 *   dst[c][0..width) = src[c][0..width) where accept[c] != 0.                                          */
omc_status omc_chain_select(omc_ctx* ctx, const int32_t* accept, int64_t width, const double* src, double* dst);
/* the same for n_items (<= OMC_SELECT_MAX) entries in one launch: entry e is widths[e] doubles per chain, chain-major,
 * copied from srcs[e] to dsts[e] on the accepted chains (host arrays of n_items elements).                      */
omc_status omc_chain_select_multi(omc_ctx* ctx, const int32_t* accept, int32_t n_items, const int64_t* widths,
                                  const double* const* srcs, double* const* dsts);

/* np.concatenate / np.delete along the ragged axis (reversible_jump.py:131, 175) for every chain:
 *   birth[c] != 0: dst = src with new_vals[c][0..rows) appended at position count[c] (NULL = zeros);
 *   birth[c] == 0: dst = src with entry del_index[c] removed, later entries shifted down.
 *   element (c, r, j) lives at base[c*chain_stride + r*row_stride + j*col_stride], j < kmax the ragged axis;
 *   dst is fully written (zeros beyond the new count); src and dst must not alias.                     */
omc_status omc_ragged_resize(omc_ctx* ctx, int64_t rows, int64_t kmax, const double* count, const int32_t* birth,
                             const int64_t* del_index, const double* new_vals, const double* src, double* dst,
                             int64_t chain_stride, int64_t row_stride, int64_t col_stride);

/* Gaussian-kernel basis on per-chain knots, the design matrix of the reference's reversible-jump example
 * (tests/test_reversible_jump.py:24-40: norm.pdf(X, loc=knot, scale=scale) per column):
 *   B[c][j][i] = exp(-t^2/2) / sqrt(2 pi) / s,  t = (X[i] - knots[c][j]) / s,  s = scales[c][j] or scale0 (scales NULL)
 *   for j < count[c], 0 beyond.  column >= 0 rewrites only that column (one knot moved), -1 all of them.
 *   prev_count (C, or NULL; needs count): B already holds zeros in the columns >= prev_count[c] of chain c (a buffer
 *   this function filled before with that count) -- only columns < max(count[c], prev_count[c]) are written.    */
omc_status omc_gaussian_basis(omc_ctx* ctx, int64_t n, int64_t kmax, const double* X, const double* knots,
                              const double* scales, double scale0, const double* count, const double* prev_count,
                              int64_t column, double* B);

/* RandomWalkLoop over the knots of that basis under a regression likelihood, every knot of every chain in one launch
 * (metropolis_hastings.py:276-289 -> :212-269 proposal, :127-173 accept/reject) for
 *   y ~ N(B_c beta_c + add_chain[c] + add_shared, (tau[c] diag(w))^-1),  knots a priori uniform on [lower, upper]:
 *   for k < count[c], in order: z ~ truncated N(theta[c][k], step^2) on [lower, upper]; accepted with probability
 *   min(1, exp(dloglik + log q(theta|z) - log q(z|theta))); an accepted move writes theta[c][k] = z and column k of B_c.
 *   The same draws as the launch-by-launch route: stream (draw_index, uniform), Philox block 2k for the proposal of knot k
 *   and 2k+1 for its accept uniform; inject_z / inject_u (kmax x C, [k][c]) replace them (tests).  w, tau, add_* may be
 *   NULL (ones / zeros).  accept_count / proposal_count (C) are incremented; accept_out / log_alpha_out (kmax x C,
 *   [k][c], entries k < count[c] written) may be NULL.  The chain's residual lives in registers: n <= 10 240.       */
omc_status omc_knot_loop(omc_ctx* ctx, int64_t n, int64_t kmax, const double* X, double scale, const double* y,
                         const double* add_shared, const double* add_chain, const double* w, const double* tau,
                         const double* beta, double* theta, const double* count, double* B, double step, double lower,
                         double upper, const double* inject_z, const double* inject_u, uint64_t draw_index,
                         int64_t* accept_count, int64_t* proposal_count, int32_t* accept_out, double* log_alpha_out);

/* Per-chain design matrices B_c (n x kmax; column j of chain c contiguous at B[(c*kmax + j)*n]):
 *   omc_design_predict_batched: out[c] = chain_scale[c] * (alpha * B_c coef_c + add_chain[c] + add_shared)
 *     (LinearCombination.predictor / predictor_conditional, parameter.py:162-197, for a basis that depends on
 *     per-chain knots; with alpha = -1, chain_scale = tau it is the per-chain part of b = A'W(y - d), sampler.py:192);
 *     add_chain [C][n], add_shared [n], chain_scale [C] may be NULL;
 *   omc_design_gram_batched:    gram[c] = B_c' diag(w) B_c (kmax x kmax, row-major),
 *     rhs[c] = B_c' diag(w) (resid_shared - resid_chain[c])   (location_scale.py:238-241, sampler.py:192);
 *     w [n] shared or NULL = ones; resid_* / rhs may be NULL; count [C] (NULL = kmax): only the leading count[c]
 *     columns are live, the rest of gram / rhs is written as 0.  kmax <= 36.
 *   omc_design_resid_sq_batched: out[c] = sum_i w[i] (y[i] - (B_c coef_c + add_chain[c] + add_shared)[i])^2, the
 *     quadratic form of Normal.log_p for a regression on a per-chain basis (gmrf.py:343-344 on the residual of
 *     parameter.py:162-197) without materialising the fitted values; y [n] shared; w, add_chain, add_shared may be
 *     NULL.  Rows are summed in a fixed order (parts, then an ordered sum of the parts).                        */
omc_status omc_design_predict_batched(omc_ctx* ctx, int64_t n, int64_t kmax, const double* B, const double* coef,
                                      const double* add_chain, const double* add_shared, double alpha,
                                      const double* chain_scale, double* out);
omc_status omc_design_resid_sq_batched(omc_ctx* ctx, int64_t n, int64_t kmax, const double* B, const double* coef,
                                       const double* add_chain, const double* add_shared, const double* y,
                                       const double* w, double* out);
omc_status omc_design_gram_batched(omc_ctx* ctx, int64_t n, int64_t kmax, const double* B, const double* w,
                                   const double* resid_shared, const double* resid_chain, const double* count,
                                   double* gram, double* rhs);
/* The same Gram matrix with the basis picked per chain: chain c uses (B_alt, count_alt) where select[c] != 0, (B, count)
 * otherwise -- the matched reversible-jump transition (reversible_jump.py:240-242, 290-292) needs X'X of the LARGER of
 * the current and the proposed basis only (proposed for a birth, current for a death).                          */
omc_status omc_design_gram_select(omc_ctx* ctx, int64_t n, int64_t kmax, const double* B, const double* count,
                                  const double* B_alt, const double* count_alt, const int32_t* select, const double* w,
                                  double* gram);

/* NormalNormal.sample (sampler.py:176-197 -> gmrf.py:167-198) for a small ragged parameter:
 *   Q_c = diag(prior_prec[c]) + lik_scale[c]*gram[c],  b_c = prior_prec[c]*prior_mean[c] + lik_scale[c]*gram_rhs[c]
 *   on the live count[c] x count[c] block; x = Q^{-1}b + L^{-T}z, natural-order Cholesky; entries beyond
 *   count[c] are written as 0.  kmax <= 64.  z_inject [C][kmax]; prior_mean / lik_scale / count / mu may be NULL. */
omc_status omc_small_sample_canonical(omc_ctx* ctx, int64_t kmax, const double* gram, const double* gram_rhs,
                                      const double* lik_scale, const double* prior_prec, const double* prior_mean,
                                      const double* count, const double* z_inject, uint64_t draw_index,
                                      double* x, double* mu);

/* The same operator under domain limits (sampler.py:194-205 -> gmrf.gibbs_canonical_truncated_normal, gmrf.py:201-266):
 * a truncated mixture prior on a ragged parameter (a cfg5 basis with beta >= 0).  ONE scan of single-site updates in natural
 * order on the live block of x [C][kmax], in place (the scan starts from x):
 *   x_i ~ N_[lower, upper]( (b_i - Q_i. x + Q_ii x_i) / Q_ii, 1/Q_ii ),  x_j already updated for j < i;
 * count[c] == 1 takes the reference's p == 1 branch (mean = b / Q); count[c] == 0 leaves the chain at 0; entries at and
 * beyond count[c] are written as 0.  lower / upper: scalars (-inf / +inf = open on that side).  u_inject [C][kmax]
 * uniforms; NULL: Philox blocks i/2 of (seed, chain, draw_index), purpose OMC_RNG_UNIFORM, as the other truncated scans.
 * A non-positive Q_ii latches the chain.  kmax <= 64.                                                              */
omc_status omc_small_gibbs_truncated(omc_ctx* ctx, int64_t kmax, const double* gram, const double* gram_rhs,
                                     const double* lik_scale, const double* prior_prec, const double* prior_mean,
                                     const double* count, double lower, double upper, const double* u_inject,
                                     uint64_t draw_index, double* x);

/* Per-chain small SPD matrices A [C][k][k] (k <= 64): Av_out[c] = A_c v_c, quad_out[c] = v_c' A_c v_c, logdet_out[c] =
 * log det A_c by the natural-order Cholesky (a non-positive pivot latches the chain); any output may be NULL.  The pieces
 * of ManifoldMALA's proposal for a Hessian that depends on the parameter (metropolis_hastings.py:325-373): Lambda x,
 * (. - m)' Lambda (. - m) and sum log L_ii with Lambda_c = H_c / step^2; the solve itself is omc_small_sample_canonical. */
omc_status omc_small_spd_ops(omc_ctx* ctx, int64_t k, const double* A, const double* v, double* Av_out, double* quad_out,
                             double* logdet_out);

/* LinearCombinationWithTransform.predictor / predictor_conditional (parameter.py:253-279) for a per-chain vector under the
 * exponential transform and a shared design X [n][ld_X] (row-major, p columns):
 *   out[c] = alpha * chain_scale[c] * (X exp(x_c)) + add_chain[c] + add_shared
 * for any n, p (at most 65 535 chains per context, here and in omc_transform_grad_hess: OMC_UNSUPPORTED beyond).  exp is applied as x is read (exp(x) is never stored); it overflows to inf as numpy's does; the sum over the
 * columns runs in index order.  add_chain [C][ld_add], add_shared [n], chain_scale [C] may be NULL.                        */
omc_status omc_transform_predict(omc_ctx* ctx, int64_t n, int64_t p, const double* X, int64_t ld_X, const double* x, int64_t ld_x,
                                 const double* add_chain, int64_t ld_add, const double* add_shared, double alpha,
                                 const double* chain_scale, double* out, int64_t ld_out);

/* Branch (ii) of Normal.grad_log_p (location_scale.py:234-242) through LinearCombinationWithTransform.grad (parameter.py:281-297):
 * with s_c = exp(x_c), u_c = A'W sum_rep (y - fitted_c) [C][ld_u] and the shared G = n_rep A'WA [p][p],
 *   grad[c] = scale[c] * s_c o u_c [C][p],   H[c][i][j] = scale[c] * s_ci s_cj G_ij [C][p][p]
 * (the reference's Gauss-Newton form: no second-derivative term).  Any p.  scale [C] may be NULL (ones); either output may be
 * NULL (u is read only for grad, G only for H).                                                                            */
omc_status omc_transform_grad_hess(omc_ctx* ctx, int64_t p, const double* x, int64_t ld_x, const double* u, int64_t ld_u,
                                   const double* G, const double* scale, double* grad, double* H);

/* One ManifoldMALA update (metropolis_hastings.py:127-173 accept/reject, :301-373 proposal) of a per-chain vector x [C][ld_x],
 * p <= 64, whose target is  y ~ N(A exp(x) + shared terms, tau_c W),  x ~ N(m0, lam_c P), on the sufficient statistics
 * G = n_rep A'WA [p][p], cvec = A'W sum_rep (y - shared terms) [p] and the dense prior precision P [p][p]:
 *   t = exp(x);  g = tau_c t o (cvec - G t) - lam_c P (x - m0);  Lambda = (tau_c (t t') o G + lam_c P) / step^2 = L L'
 *   (natural order; a non-positive pivot latches the chain and leaves x as it is);  mu = x + Lambda^-1 g / 2;  x' = mu + L^-T z;
 *   log q(x'|x) = sum log L_ii - |L'(x' - mu)|^2 / 2, the same at x' for log q(x|x');  accept iff
 *   log u < target(x') - target(x) + log q(x|x') - log q(x'|x),  target = tau_c (t'cvec - t'G t / 2) - lam_c (x-m0)'P(x-m0) / 2.
 * One launch for every chain.  G and P are symmetric; the kernel reads element (i, j) at [j * p + i].  z_inject [C][p] / u_inject [C]; NULL: the normals of (seed, chain, draw_index) blocks i/2 and the
 * uniform of block (p+1)/2 + 1, the streams omc_small_sample_canonical and omc_mh_accept read on the launch-by-launch route.
 * m0 [p], tau [C], lam [C] may be NULL (zeros / ones).  accept_count / proposal_count [C] are incremented; prop_out [C][p],
 * lq_fwd_out, lq_rev_out and logp_out [C] (the target, up to its constant, at the state left in x) may be NULL.            */
omc_status omc_mala_transform_step(omc_ctx* ctx, int64_t p, const double* G, const double* cvec, const double* P, const double* m0,
                                   const double* tau, const double* lam, double step, double* x, int64_t ld_x,
                                   const double* z_inject, const double* u_inject, uint64_t draw_index, int64_t* accept_count,
                                   int64_t* proposal_count, double* prop_out, double* lq_fwd_out, double* lq_rev_out,
                                   double* logp_out);

/* ReversibleJump.matched_birth_transition / matched_death_transition (reversible_jump.py:195-308):
 *   with X the larger of the two bases (the proposed one for a birth, the current one for a death),
 *   G = (X'X + 1e-10 I)^{-1} X'X_small by LU with partial pivoting (np.linalg.solve);
 *   birth: coef* = G coef, last entry ~ truncated N(coef*_last, scale) on [lim_lo, lim_hi] (has_limits) or
 *          N(coef*_last, scale^2); lq_fwd += its log-density; lq_rev += log det [G | e_last];
 *   death: F = G with e_idx inserted at column idx; coef_aug = F^{-1} coef; coef* = coef_aug without idx;
 *          lq_fwd += log det F; lq_rev += log-density of coef_aug[idx] under (truncated) N(0, scale).
 *   gram_cur / gram_prop [C][kmax][kmax]: Gram matrices of the current and proposed bases (the products
 *   X'X_small are sub-blocks of the larger one).  draw_inject [C]: uniform (limits) or normal draw.      */
omc_status omc_rj_matched_transition(omc_ctx* ctx, int64_t kmax, const double* gram_cur, const double* gram_prop,
                                     const double* count, const int32_t* birth, const int64_t* del_index,
                                     const double* coef_cur, double scale, int32_t has_limits, double lim_lo,
                                     double lim_hi, const double* draw_inject, uint64_t draw_index, uint32_t sub,
                                     double* coef_prop, double* lq_fwd, double* lq_rev);

/* Log-density pieces for ragged parameters (accumulate != 0 adds into out[c]):
 *   omc_diag_gauss_logpdf: Normal with diagonal precision (MixtureParameterMatrix, parameter.py:474-538):
 *     0.5*(sum_j log prec_j - k log 2pi - sum_j prec_j (x_j - mean_j)^2) over the k = count[c] live entries;
 *   omc_poisson_logpmf:    Poisson.log_p (distribution.py:490-508): k log(rate) - rate - lgamma(k+1), k = x[c];
 *   omc_count_logpdf:      out = per_element * count[c]  (Uniform.log_p, distribution.py:422-442: every live
 *     replicate contributes -sum log(upper - lower));
 *   omc_mixture_gather:    MixtureParameterVector.predictor (parameter.py:447): out[c][j] = param[alloc[c][j]]
 *     for live j, `fill` beyond (param [m] shared with param_stride 0, or per chain [C][m] with param_stride m;
 *     alloc holds integer values as float64).                                                              */
/* LogNormal.log_p (location_scale.py:279-300) = Normal.log_p at log(response) minus sum log(response):
 *   out[c][i] = log x[c][i], sumlog[c] = sum_i log x[c][i] (sumlog may be NULL).                              */
omc_status omc_log_transform(omc_ctx* ctx, int64_t n, const double* x, int64_t ld_x, double* out, int64_t ld_o,
                             double* sumlog);

/* out[c] = sum_i (a[c][i] - center_a[i]) * (b[c][i] - center_b[i]).  With b = M x from omc_design_predict (one GEMM over
 * all chains) and center_b = M m this is the quadratic form (x - m)' M (x - m) of a DENSE shared precision: the
 * sufficient statistic of NormalGamma.sample (sampler.py:276,284) and of Normal.log_p (gmrf.py:343-344).      */
omc_status omc_centered_rowdot(omc_ctx* ctx, int64_t n, const double* a, int64_t ld_a, const double* center_a,
                               const double* b, int64_t ld_b, const double* center_b, double* out);

/* Poisson.rvs for every chain (distribution.py:508-523: scipy.stats.poisson.rvs, i.e. NumPy's legacy generator -- multiplication
 * method below rate 10, PTRS transformed rejection from 10 on): out[c] = one Poisson(rate[c * rate_stride]) count as a double
 * (rate_stride 0: one shared rate).  u_inject [C][ld_u]: the uniforms the draw consumes, in order, NaN-padded (the parity tests
 * replay the reference's generator through it; running off the tape latches the chain in omc_ctx_status); NULL: the chain's
 * Philox stream at draw_index.  Used for the prior draw of a jump parameter without an initial value (mcmc.py:78-85).  */
omc_status omc_poisson_draw(omc_ctx* ctx, const double* rate, int64_t rate_stride, const double* u_inject, int64_t ld_u,
                            uint64_t draw_index, double* out);
/* Uniform.rvs (distribution.py:444-458): out[c][e] = lower[e] + range[e] * U(0,1], e < p (lower/range device [p]);
 * u_inject [C][p]; in-kernel uniforms come from Philox blocks sub, sub+1, ... (two per block).               */
omc_status omc_uniform_draw(omc_ctx* ctx, int64_t p, const double* lower, const double* range, const double* u_inject,
                            uint64_t draw_index, uint32_t sub, double* out);
omc_status omc_diag_gauss_logpdf(omc_ctx* ctx, int64_t kmax, const double* x, const double* mean, const double* prec,
                                 const double* count, double* out, int32_t accumulate);
/* omc_diag_gauss_logpdf of a mixture Normal with domain limits (location_scale.py:162-188): the same value, and -inf for a
 * chain with a LIVE element (index < count[c]) below lower or above upper; the padding is not looked at.  lower / upper:
 * scalars (-inf / +inf = open).  One launch.                                                                      */
omc_status omc_diag_gauss_logpdf_limits(omc_ctx* ctx, int64_t kmax, const double* x, const double* mean, const double* prec,
                                        const double* count, double lower, double upper, double* out, int32_t accumulate);
/* Mixture models: a parameter vector whose prior mean / precision are picked per element
 * by a categorical allocation (parameter.py:376-538), the allocation's conditional draw and the per-component
 * precision update.
 *   omc_mixture_allocation: MixtureAllocation.sample (sampler.py:321-355): prob_k = prior[i or 0][k] *
 *     N(y[c][i]; mean[c][k], 1/prec[c][k]), normalised; alloc = #{k : U > cumsum_k}.  prior [prior_rows x K] shared
 *     (prior_rows 1 or p), mean / prec [C][K] (stride 0 = shared [K]), u_inject [C][p];
 *   omc_categorical_logpmf: Categorical.log_p (distribution.py:318-352, one trial per element):
 *     sum_i log prob[i or 0][alloc[c][i]];
 *   omc_mixture_normal_gamma: NormalGamma.sample for a MixtureParameterMatrix precision (sampler.py:276-287 with
 *     parameter.py:525-538): a_k = a0[k] + #{alloc == k}/2, b_k = b0[k] + sum_{alloc == k} resid^2 / 2,
 *     out[c][k] = Gamma(a_k, scale 1/b_k); a0 / b0 device [K], g_inject [C][K] standard gammas;
 *   omc_gamma_logpdf_vec: Gamma.log_p of a (K, 1) response with per-element shape / rate (device [K]).       */
omc_status omc_mixture_allocation(omc_ctx* ctx, int64_t p, int64_t K, const double* y, const double* prior,
                                  int64_t prior_rows, const double* mean, int64_t mean_stride, const double* prec,
                                  int64_t prec_stride, const double* u_inject, uint64_t draw_index, double* alloc);
omc_status omc_categorical_logpmf(omc_ctx* ctx, int64_t p, int64_t K, const double* alloc, const double* prob,
                                  int64_t prob_rows, double* out, int32_t accumulate);
omc_status omc_mixture_normal_gamma(omc_ctx* ctx, int64_t p, int64_t K, const double* resid, const double* alloc,
                                    const double* a0, const double* b0, const double* g_inject, uint64_t draw_index,
                                    double* out);
omc_status omc_gamma_logpdf_vec(omc_ctx* ctx, int64_t K, const double* x, const double* shape, const double* rate,
                                double* out, int32_t accumulate);
/* omc_gamma_logpdf_ragged: Gamma.log_p (distribution.py:241-261) of a ragged (1, k) response: the sum over the live
 *   entries, or with last_only != 0 the density of the LAST live entry (what ReversibleJump reads from
 *   log_p(..., by_observation=True)[-1], reversible_jump.py:132,143);
 * omc_diag_gauss_grad: gradient of the diagonal Gaussian log-density w.r.t. its response, -prec (x - mean) on the live
 *   entries, 0 beyond (location_scale.py:222-226).                                                              */
omc_status omc_gamma_logpdf_ragged(omc_ctx* ctx, int64_t kmax, const double* x, const double* count, double shape,
                                   double rate, int32_t last_only, double* out, int32_t accumulate);
omc_status omc_diag_gauss_grad(omc_ctx* ctx, int64_t kmax, const double* x, const double* mean, const double* prec,
                               const double* count, double* grad);
omc_status omc_poisson_logpmf(omc_ctx* ctx, const double* x, double rate, double* out, int32_t accumulate);
omc_status omc_count_logpdf(omc_ctx* ctx, const double* count, double per_element, double* out, int32_t accumulate);
omc_status omc_mixture_gather(omc_ctx* ctx, int64_t kmax, int64_t m, const double* param, int64_t param_stride,
                              const double* alloc, const double* count, double fill, double* out);
/* two tables gathered by one allocation in one launch (the mean and the precision of a mixture Normal) */
omc_status omc_mixture_gather2(omc_ctx* ctx, int64_t kmax, int64_t m, const double* alloc, const double* count,
                               const double* param_a, int64_t stride_a, double fill_a, double* out_a, const double* param_b,
                               int64_t stride_b, double fill_b, double* out_b);

/* ---- on-device posterior summaries of the device-resident store ----
 * store is [n_iter][C][size] (iteration-major, as MCMC writes it: mcmc.py:105-106 per chain).
 *   pooled == 0: mean_out / var_out [C][size]: per chain over its n_iter stored iterations;
 *   pooled != 0: mean_out / var_out [size]:    over all chains and iterations.
 * var is the unbiased sample variance (0 when there is a single sample); either output may be NULL.
 * Saves gathering the whole store (82 MB per iteration at cfg3) when only summaries are wanted.   */
omc_status omc_store_moments(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store,
                             int32_t pooled, double* mean_out, double* var_out);
/* Quantiles of the same store, np.quantile's default ("linear") method, what a user of the reference computes on
 * MCMC.store[param] (host arrays there: mcmc.py:105-111, sampler/sampler.py:89-118):
 *   q        [n_q]  (HOST) levels in [0, 1]
 *   pooled == 0: out [n_q][C][size]: per chain over its n_iter stored iterations (np.quantile(store_c, q, axis=-1));
 *   pooled != 0: out [n_q][size]:    over all chains and iterations.
 *   omit_nan != 0: NaN entries (the padding of variable-size parameters beyond the live length, sampler.py:81-87; iterations
 *   not yet written) are left out per element like np.nanquantile, an element with no valid value gives NaN;
 *   omit_nan == 0: an element with any NaN gives NaN (np.quantile).
 * Exact order statistics by radix refinement on the device (eight passes over the store per group of four levels; no sort,
 * no copy of the store), then numpy's interpolation operation by operation: results are bit-equal to np.quantile's.      */
omc_status omc_store_quantiles(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, int32_t pooled, int32_t n_q,
                               const double* q, int32_t omit_nan, double* out);
/* Convergence diagnostics of the same store, per element k: split R-hat and the effective sample size.  N = n_iter >= 4
 * (else OMC_INVALID_ARG), M = N / 2; every chain gives two series, its first and its last M iterations (the middle draw of
 * an odd N is dropped): J = 2 C series x_j[0..M).
 *   m_j = mean(x_j),  g_j(t) = (1/M) sum_{i=0}^{M-1-t} (x_j[i] - m_j)(x_j[i+t] - m_j),
 *   W = mean_j g_j(0) M / (M - 1),  B_M = var(m_0 .. m_{J-1}, ddof 1),  var_plus = W (M - 1) / M + B_M,
 *   rhat = sqrt(var_plus / W),  rho(t) = 1 - (W - mean_j g_j(t)) / var_plus;
 *   ess = J M / max(tau, 1 / log10(J M)), tau = -1 + 2 sum(r[0 .. max_t]) + r[max_t + 1] from Geyer's initial monotone
 *   sequence r on rho (initial positive pairs while t < M - 3, then a running minimum of the pair sums), as ArviZ's
 *   ess(method="mean").
 *   Any NaN draw of element k (any chain, any iteration): rhat = ess = NaN.  Every split draw equal: ess = J M, rhat = NaN.
 *   Every series constant but the series differ (W == 0 < B_M): rhat = +inf.
 *   rhat_out, ess_out [size]; lag_out [size] = max_t + 1, the lags the element's sequence used (0 where it was not run:
 *   NaN or constant elements); any output may be NULL.
 * Direct lag sums on the device, one lane per (series, element): M <= 64 reads the store once, longer series read it
 * 1 + 1 + 2 (ceil((max_t + 2) / 32) - 1) times (the means, then blocks of 32 lags until every element's sequence has ended;
 * the host reads one word per block).  Option "diag_algo" (0 auto; 1 the short-series form, M <= 64 only; 2 blocks of
 * lags) forces a form: same results to rounding.  Deterministic: repeated calls are bit-equal.                    */
omc_status omc_store_rhat_ess(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store,
                              double* rhat_out, double* ess_out, int32_t* lag_out);
/* Second moments of the same store: posterior covariance / correlation matrix of its elements, what a user of the reference
 * computes with np.cov / np.corrcoef on MCMC.store[param].
 *   store_a [n_iter][C][size_a], store_b [n_iter][C][size_b] (device).  store_b == NULL: "b is a", the symmetric form
 *           (size_b, idx_b, n_b are then ignored and taken from a);
 *   idx_a   [n_a] (device) the elements of a that take part, in that order, repeats allowed; NULL = all of them (n_a must then
 *           equal size_a).  idx_b likewise.  An index outside [0, size) is OMC_INVALID_ARG, found on the device before any
 *           launch reads through it (the host reads one word back); out is then untouched;
 *   pooled != 0: out [n_a][n_b] over all R = n_iter C draws around the pooled means, divisor R - 1: the off-diagonal block of
 *           np.cov(a2d, b2d), a2d = store_a.reshape(R, size_a).T;
 *   pooled == 0: out [C][n_a][n_b], chain c over its own n_iter draws around its own means, divisor n_iter - 1;
 *   a single draw gives 0, as omc_store_moments defines its variance;
 *   correlation != 0: out_ij = c_ij / (sqrt(v_i) sqrt(v_j)), v the variances of the call's means pass (omc_store_moments'
 *           values), clipped to [-1, 1]; an element with zero variance gives NaN in its row / column (np.corrcoef); in the
 *           symmetric form an entry whose two sides are the same element (the diagonal, repeats of an index) is exactly 1.
 *   NaN is propagated like np.cov: an element with a NaN draw (among the draws the entry is taken over: any chain when
 *   pooled, that chain otherwise) makes its whole row / column NaN and nothing else.  There is no omit_nan form: leaving
 *   NaN out pair by pair (pairwise deletion) is a different estimator, with a different divisor per entry and no guarantee
 *   of a positive semi-definite result.
 *   Symmetric form: out == out' bit for bit (one triangle of tiles is computed and mirrored).
 * Two passes over the selected columns: their means, then the products of the values centred in fp64 as they are loaded, on
 * the fp64 matrix cores; the contraction is cut into slices whose partial tiles are added in a fixed order (no atomics):
 * repeated calls are bit-equal.  Runs on the context's stream; workspace (the partial tiles) from the context.        */
omc_status omc_store_cov(omc_ctx* ctx, int64_t n_iter,
                         int64_t size_a, const double* store_a, const int64_t* idx_a, int64_t n_a,
                         int64_t size_b, const double* store_b, const int64_t* idx_b, int64_t n_b,
                         int32_t pooled, int32_t correlation, double* out);
/* Range of the same store per element, np.nanmin / np.nanmax of MCMC.store[param] (host arrays in the reference:
 * mcmc.py:105-111), with the layout conventions of omc_store_cov: idx [n_idx] (device) the elements that take part, in that order,
 * repeats allowed, NULL = all of them (n_idx must then equal size); an index outside [0, size) is OMC_INVALID_ARG, found on the
 * device before any output is written.
 *   pooled != 0: min_out / max_out / count_out [n_idx] over all n_iter C draws; pooled == 0: [C][n_idx], chain c over its own.
 *   count_out (int64) = the non-NaN draws; an element without one gives NaN, NaN, 0; +-inf are ordinary values; any output may
 *   be NULL.  One read of the selected columns; per-slice partials joined in a fixed order (workspace from the context).   */
omc_status omc_store_minmax(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx, int64_t n_idx,
                            int32_t pooled, double* min_out, double* max_out, int64_t* count_out);
/* Marginal histogram of every selected element of the same store: np.histogram(MCMC.store[param][i], bins=edges) of the
 * reference's host arrays (mcmc.py:105-111) for all i at once; store, idx, n_idx, pooled as omc_store_minmax.
 *   edges   (device) [n_bins + 1] shared by all elements, or [n_idx][n_bins + 1] when edges_per_element != 0; non-decreasing,
 *           equal neighbours and +-inf allowed (as in numpy).  A NaN edge or a decreasing pair is OMC_INVALID_ARG, found on the
 *           device before anything is counted: the outputs are then untouched.  1 <= n_bins <= 1024, else OMC_INVALID_ARG.
 *   The bin rule is numpy's, comparisons with the edges alone: v falls in bin j when edges[j] <= v < edges[j + 1], the last bin
 *   is closed (edges[n_bins - 1] <= v <= edges[n_bins]); with equal neighbours that is the last j with edges[j] <= v,
 *   np.searchsorted(edges, v, 'right') - 1.  Evenly spaced edges get an arithmetic guess of the bin, put right by comparing with
 *   the neighbouring edges (option "hist_algo" = 1: always the bisection; same counts).
 *   counts_out  int64 [n_idx][n_bins] pooled, [C][n_idx][n_bins] per chain;
 *   outside_out int64 [..][3] = draws below edges[0], draws above edges[n_bins], NaN draws; may be NULL.
 *   Every row: sum(counts) + sum(outside) = the draws taken, n_iter C pooled, n_iter per chain.  Outputs are overwritten.
 * One read of the selected columns: 32-bit counters in LDS per workgroup, added to the zeroed outputs with 64-bit integer
 * atomics -- integer sums do not depend on the order: repeated calls and both forms are bit-equal.  n_iter C >= 2^32 (a
 * workgroup's counters) is OMC_UNSUPPORTED.  Runs on the context's stream; the host reads two words back (the validation).  */
omc_status omc_store_histogram(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx, int64_t n_idx,
                               int32_t pooled, int32_t n_bins, const double* edges, int32_t edges_per_element, int64_t* counts_out,
                               int64_t* outside_out);
/* [host, no GPU] The tiling and LDS image omc_store_histogram takes at n_bins (1..1024, else OMC_INVALID_ARG): out[10] = {TE
 * (elements of a workgroup's tile), RB (rows of a slice), stride of an element's edges (doubles; 0 when shared), stride of an
 * element's counters (words), byte offsets of the edges, the counters and the outside counts, end of the image = bytes launched,
 * the budget the tile was chosen for, threads of a workgroup}.                                                           */
omc_status omc_store_histogram_layout(int32_t n_bins, int32_t edges_per_element, int32_t* out);
/* Kernel density estimate, bandwidth and mode of n_cols columns from their bin counts: what scipy.stats.gaussian_kde / ArviZ's kde
 * give for a column of MCMC.store[param] on the host (mcmc.py:105-111 of the reference), from counts such as
 * omc_store_histogram's over evenly spaced edges.  Everything is a function of (counts, lo, hi) alone: counts added over ranks
 * (same edges) give the estimate of all ranks' chains.  All arrays on the device.
 *   counts  int64 [n_cols][G], 8 <= G <= 1024 (else OMC_INVALID_ARG); lo, hi [n_cols] the grid [a, b] of every column.
 *           delta = (b - a) / G, grid points g_j = a + (j + 1/2) delta (the bin centres), N = sum_j c_j, p_j = c_j / N.
 *   rule    0 given: h = bw_in[col] (bw_in NULL is OMC_INVALID_ARG); else from the binned moments m = sum p_j g_j,
 *           sd^2 = N / (N - 1) sum p_j (g_j - m)^2 and the binned quantile q(u) = a + delta (j + (u N - C_j) / c_j), C_j the exclusive
 *           prefix sum of c and j the first bin with C_j + c_j >= u N (exact integers), IQR = q(3/4) - q(1/4):
 *           1 Scott      h = 1.06 sd N^(-1/5);
 *           2 Silverman  h = 0.9 min(sd, IQR / 1.34) N^(-1/5), sd alone when IQR == 0;
 *           3 ISJ, the improved Sheather-Jones rule of Botev, Grotowski and Kroese (2010): a_k = sum_j p_j cos(pi k (2 j + 1) / (2 G)),
 *             k = 1..G-1, the cosine from a table of cos(pi m / (2 G)) by the exact integer k (2 j + 1) mod 4 G;
 *             f_s(t) = 2 pi^(2 s) sum_k k^(2 s) a_k^2 exp(-k^2 pi^2 t); from f_7(t), for s = 6..2:
 *             t_s = (2 c_s kappa_s / (N f_(s+1)))^(2 / (3 + 2 s)), c_s = (1 + 2^-(s + 1/2)) / 3, kappa_s = 1 3 .. (2 s - 1) / sqrt(2 pi),
 *             f_s(t_s); Phi(t) = t - (2 N sqrt(pi) f_2(t_2))^(-2/5).  The root: Phi at t_i = 2^(-(6 + i) / 2), i = 0..46, from the
 *             largest t down; the first adjacent pair, both finite, of opposite signs (>= 0 counts as positive); exactly 60
 *             bisection steps, the midpoint replacing the end whose sign it shares (steps after the ends have met in fp64 change
 *             nothing and are not run); t* the midpoint of what is left;
 *             h = sqrt(t*) (b - a).  Without such a pair h is Silverman's and the column's flag is 1;
 *           4 experimental: the mean of Silverman's and ISJ's (ArviZ's default), flag 1 when ISJ fell back.
 *           Every rule's h is multiplied by bw_fct (finite and > 0, else OMC_INVALID_ARG).
 *   density_out [n_cols][G]: f(g_k) = 1 / (N h) sum_j c_j [phi((g_k - g_j) / h) + R_lo + R_hi], phi the standard normal density, no
 *           truncation; reflect bit 0: the grid starts at a lower bound, R_lo = phi((k + j + 1) delta / h), the image of g_j
 *           mirrored at a; bit 1: it ends at an upper bound, R_hi = phi((2 G - 1 - k - j) delta / h); else 0.  phi comes from a table
 *           exp(-(d delta / h)^2 / 2), d = 0..2 G - 1: every distance is an integer multiple of delta.
 *   bw_out [n_cols] the h used; mode_out [n_cols] the grid point of the largest density, the lowest of equals;
 *   flag_out int32 [n_cols]: 0 ok; 1 ISJ fell back to Silverman; 2 degenerate -- density, bw and mode NaN, other columns
 *           unaffected: hi <= lo or an end not finite; under a rule N < 2 or fewer than two non-empty bins; under rule 0 N == 0 or
 *           a bandwidth that is not finite and positive.  Any output may be NULL.
 *   A negative count is OMC_INVALID_ARG, found on the device before anything is written (one word read back); the outputs are
 *   untouched by every OMC_INVALID_ARG.  N is exact below 2^53.
 * One workgroup per column (one wave up to 128 bins, four above: the choice depends on G alone and both add in the same order);
 * every sum runs in an order that G alone fixes, no atomics: repeated calls are bit-equal.  Runs on the context's stream.     */
omc_status omc_kde_binned(omc_ctx* ctx, int64_t n_cols, int32_t G, const int64_t* counts, const double* lo, const double* hi,
                          int32_t rule, const double* bw_in, double bw_fct, int32_t reflect, double* density_out, double* bw_out,
                          int32_t* flag_out, double* mode_out);
/* [host, no GPU] The LDS image of omc_kde_binned's kernel at G bins (8..1024, else OMC_INVALID_ARG): out[8] = {threads of a
 * workgroup, byte offsets of the counts [G], of A2 [G], of the quarter-wave cosines [G + 1], of the Gaussian table [2 G] and of the
 * block sums [64] (all doubles), end of the image = bytes launched, the budget}.                                          */
omc_status omc_kde_layout(int32_t G, int32_t* out);
/* Joint kernel density estimate, kernel covariance, joint mode and highest-density-region levels of n_grids pairs of coordinates
 * from their 2-D bin counts: what scipy.stats.gaussian_kde on two rows / az.plot_kde(x, y, hdi_probs=...) give for two columns of
 * MCMC.store[param] on the host (mcmc.py:105-111 of the reference), from counts such as omc_store_histogram2d's over evenly spaced
 * edges.  Everything is a function of (counts, grid) alone: int64 counts of several ranks over the same edges can be added, and one
 * call gives the estimate of all ranks' chains, bit-equal to the call on the whole.  All arrays on the device; any output may be NULL.
 *   counts  int64 [n_grids][nx][ny], the layout of omc_store_histogram2d's counts_out; 8 <= nx, ny <= 256, else OMC_INVALID_ARG.
 *           A negative count is OMC_INVALID_ARG, found on the device before anything is written (one read-back of two words); the
 *           outputs are untouched by every OMC_INVALID_ARG.
 *   lo_x, hi_x, lo_y, hi_y [n_grids]: grid g spans [lo_x, hi_x] x [lo_y, hi_y]; delta_x = (hi_x - lo_x) / nx, bin centres
 *           X_i = lo_x + (i + 1/2) delta_x, the same for y.  N = sum_ij c_ij (exact below 2^53), p_ij = c_ij / N.
 *   Binned moments: m_x = sum_i (sum_j p_ij) X_i, s_xx = N / (N - 1) sum_i (sum_j p_ij) (X_i - m_x)^2, likewise m_y, s_yy;
 *           s_xy = N / (N - 1) sum_ij p_ij (X_i - m_x) (Y_j - m_y).
 *   rule    0 given: the symmetric kernel covariance H = (h_xx, h_xy, h_yy) = bw_in[g][0..2] (bw_in NULL is OMC_INVALID_ARG);
 *           1 Scott: H = N^(-1/3) S -- in two dimensions also Silverman's rule, (N (d + 2) / 4)^(-2 / (d + 4)) at d = 2, and what
 *             scipy.stats.gaussian_kde and ArviZ's 2-D KDE use (factor N^(-1/6) on the sample covariance with ddof 1).
 *           Every H is multiplied by bw_fct^2 (bw_fct finite and > 0, else OMC_INVALID_ARG).
 *   density_out [n_grids][nx][ny]: f(X_k, Y_l) = 1 / (N 2 pi sqrt(det H)) sum_i sum_j c_ij exp(-q / 2), q = A u^2 + 2 B u v + C v^2,
 *           u = (k - i) delta_x, v = (l - j) delta_y, (A, B, C) = (h_yy, -h_xy, h_xx) / det H.  No truncation, and no reflection at
 *           a bound: reflecting a correlated kernel is not defined here (out of scope).  q is evaluated as the completed square
 *           A (u + (B / A) v)^2 + v^2 / h_yy, B / A = -h_xy / h_yy: the same number, as two non-negative terms.  Summed term by
 *           term, the three terms cancel at a high correlation and the tails lose digits (4.8e-12 relative in fp64 at 0.99);
 *           a restatement that is to agree within 1e-10 takes this form or more precision.
 *   bw_out [n_grids][3] the H used; mode_out [n_grids][2] = (X_k, Y_l) of the largest density, the lowest flat index k ny + l of
 *           equals, each centre formed as lo + (k + 1/2) delta with both roundings.
 *   Regions: probs [n_probs] (device), 0 <= n_probs <= 16, each in (0, 1), else OMC_INVALID_ARG (found on the device with the
 *           counts); NULL with n_probs 0: no levels.  D_0 >= D_1 >= .. the nx ny densities of a grid in descending order (the
 *           key-only sort of the store summaries on the bit patterns: non-negative doubles order as unsigned integers),
 *           S_r = D_0 + .. + D_r, S = S at r = nx ny - 1; level_pos_out int64 [n_grids][n_probs] = the first r with
 *           S_r >= prob S, level_out [n_grids][n_probs] = D_r: {f >= level} is the highest-density region that holds that share
 *           of the mass (ArviZ's _find_hdi_contours).  The order of the additions in S_r depends on nx ny alone: with
 *           len = ceil(nx ny / 256), the running sum of segment t = [t len, (t + 1) len) starts from the sum of the sums of the
 *           segments before it (each added up from zero in ascending order, the segments in ascending order) and takes its own
 *           densities in ascending r.
 *   flag_out int32 [n_grids]: 0 ok; 2 degenerate -- every output of that grid NaN (level_pos -1), other grids unaffected: an end
 *           not finite or hi <= lo; under rule 1 N < 2 or fewer than two non-empty rows or columns (decided on the integers);
 *           under rule 0 N == 0; h_xx or h_yy not finite and positive, h_xy not finite; h_xy^2 >= (1 - 2^-20) h_xx h_yy: the
 *           kernel is singular or nearly so -- far outside rounding's reach, so that exactly collinear cells always flag and
 *           honest inputs never do.
 * Work is split over (grid, tile of output cells): omc_kde2d_layout.  Every sum runs in an order that (nx, ny) alone fixes; no
 * atomics; repeated calls are bit-equal, and a grid alone gives the bits it gives inside a batch.  Empty cells and rows are
 * skipped: adding +0 to a non-negative finite sum changes no bit.  Runs on the context's stream.                                */
omc_status omc_kde2d_binned(omc_ctx* ctx, int64_t n_grids, int32_t nx, int32_t ny, const int64_t* counts, const double* lo_x,
                            const double* hi_x, const double* lo_y, const double* hi_y, int32_t rule, const double* bw_in,
                            double bw_fct, int32_t n_probs, const double* probs, double* density_out, double* bw_out,
                            double* mode_out, double* level_out, int64_t* level_pos_out, int32_t* flag_out);
/* [host, no GPU] The tiling and LDS image of omc_kde2d_binned's convolution at (nx, ny) (each 8..256, else OMC_INVALID_ARG):
 * out[16] = {TX, TY (rows and columns of an output tile), RY (adjacent columns a lane owns, TY = 64 RY), RB (rows of a count
 * block), threads of a workgroup, tiles along x, tiles along y, stride of a count row (doubles: ny rounded up to RY), slots of a
 * plane of weights, byte offsets of the counts [RB + 1][stride], the rows' flags [RB + 1], the rows' masks of non-empty runs
 * [RB + 1][2] (64-bit) and the weights [4 waves][RY][slots], bytes of a wave's weights, end of the image = bytes launched, the
 * budget}.                                                                                                                  */
omc_status omc_kde2d_layout(int32_t nx, int32_t ny, int32_t* out);
/* Joint histogram of pairs of elements of the same store(s): np.histogram2d(x, y, bins=[edges_x, edges_y]) of two rows of the
 * reference's host arrays MCMC.store[param] (mcmc.py:105-111), for all pairs at once; layout conventions of omc_store_histogram.
 *   store_x [n_iter][C][size_x], store_y [n_iter][C][size_y] (device): the same tensor or two; pair k = (element idx_x[k] of
 *           store_x, element idx_y[k] of store_y) read from the same row.  idx_x, idx_y [n_pairs] (device), in that order, repeats
 *           allowed; NULL = all elements (n_pairs must then equal that store's size).
 *   pooled != 0: one batch of R = n_iter C rows; pooled == 0: C batches, chain c over its own n_iter rows.
 *   edges_x [nx + 1], edges_y [ny + 1] (device) shared by all pairs, or [n_pairs][nx + 1], [n_pairs][ny + 1] when
 *           edges_per_pair != 0 (one flag for both axes; per-pair shape only).  1 <= nx, ny <= 1024.  Non-decreasing, equal
 *           neighbours and +-inf allowed.  A NaN edge, a decreasing pair of edges or an index outside [0, size) is
 *           OMC_INVALID_ARG, found on the device before anything is written: the outputs are then untouched.
 *   Per axis the bin rule is omc_store_histogram's (the last j with edges[j] <= v, the last bin closed; an arithmetic guess with
 *   evenly spaced edges, put right by comparisons).  A pair is counted in cell (jx, jy) when both coordinates lie inside their
 *   edge ranges: a NaN in either coordinate drops the pair, as np.histogram2d does.
 *   pool_pairs == 0: counts_out int64 [batches][n_pairs][nx][ny], outside_out int64 [batches][n_pairs][2];
 *   pool_pairs != 0: all pairs into one grid, counts_out [batches][nx][ny], outside_out [batches][2] -- the map of a ragged
 *           (NaN-padded) parameter; occupied_out int64 [batches][nx][ny] (NULL = not wanted; pooled pairs only, else
 *           OMC_INVALID_ARG) = the rows, (iteration, chain) states, in which the cell received at least one of the row's
 *           pairs: the sum over stored states of np.histogramdd(...) > 0.  occupied <= counts cell by cell, occupied <= R.
 *           With occupied_out, n_pairs > 256 is OMC_UNSUPPORTED (a row's cells are compared within one wave).
 *   outside = {pairs with both coordinates non-NaN and at least one outside its edge range, pairs with a NaN coordinate}; may be
 *   NULL.  Every output row: sum(counts) + outside[0] + outside[1] = the pairs taken.  Outputs are overwritten.
 * One read of the selected columns.  LDS form: 32-bit counters per workgroup, the non-zero ones added to the zeroed outputs with
 * 64-bit integer atomics.  Direct form: those atomic adds straight from the counting loop -- taken when the counters of one pair
 * do not fit the LDS budget, when the rows a workgroup walks times the pairs pooled into one counter reach 2^32, or with option
 * "hist2d_algo" bit 0.  Integer sums do not depend on the order: repeated calls and both forms are bit-equal; no
 * floating-point atomics.  Runs on the context's stream; the host reads two words back per axis (the validation).          */
omc_status omc_store_histogram2d(omc_ctx* ctx, int64_t n_iter, int64_t size_x, const double* store_x, const int64_t* idx_x,
                                 int64_t size_y, const double* store_y, const int64_t* idx_y, int64_t n_pairs, int32_t pooled,
                                 int32_t pool_pairs, int32_t nx, const double* edges_x, int32_t ny, const double* edges_y,
                                 int32_t edges_per_pair, int64_t* counts_out, int64_t* outside_out, int64_t* occupied_out);
/* [host, no GPU] The tiling and LDS image omc_store_histogram2d takes at (nx, ny) (each 1..1024, else OMC_INVALID_ARG);
 * pool_pairs: 0 a grid per pair, 1 pooled pairs, 2 pooled pairs with the occupancy grid (edges_per_pair must then be 0).
 * out[14] = {form (0 LDS, 1 direct: the counters of one pair do not fit), TE (pairs of a workgroup's tile; 1 pooled), RB (rows of
 * a slice), strides of a pair's x and y edges (doubles; 0 when shared), stride of a pair's counters (words; 0 in the direct
 * form), byte offsets of the x edges, the y edges, the counters, the occupancy counters and the outside counts, end of the
 * image = bytes launched, the budget the tile was chosen for, threads of a workgroup}.                                  */
omc_status omc_store_histogram2d_layout(int32_t nx, int32_t ny, int32_t edges_per_pair, int32_t pool_pairs, int32_t* out);
/* Co-allocation (posterior similarity, co-clustering) matrix of the allocation vectors in the same store -- the labels 0 .. K - 1
 * that MixtureAllocation draws, stored as fp64: (Z[:, :, None] == Z[:, None, :]).sum(0) of the gathered labels Z [rows][n_idx] of
 * the reference's host arrays MCMC.store[param] (mcmc.py:105-111).  Invariant to label switching, which the mean or a quantile of
 * a label is not.  Contract common to omc_store_coalloc and omc_store_partition_score:
 *   store   [n_iter][C][size] (device), seen as omc_store_cov sees it; idx [n_idx] (device) the elements that take part, in that
 *           order, repeats allowed; NULL = all of them (n_idx must then equal size).  An index outside [0, size) is
 *           OMC_INVALID_ARG, found on the device before anything is written (the host reads one word back);
 *   pooled != 0: one batch of R = n_iter C rows; pooled == 0: C batches, chain c over its own R = n_iter rows;
 *   1 <= n_labels <= 64: more is OMC_UNSUPPORTED, less OMC_INVALID_ARG;
 *   the label rule: a draw v carries label k iff v == k for an integer 0 <= k < n_labels; -0.0 is label 0.  NaN is "element
 *           absent" (the padding of variable-size parameters); any other value (fractional, negative, >= n_labels, +-inf) is "not
 *           a label".  An absent or non-label draw matches nothing, not even itself -- numpy's NaN == NaN is False, extended to
 *           the non-labels;
 *   every output is overwritten; nothing is written on an error status, whose cause omc_last_error names.
 * omc_store_coalloc:
 *   per_label == 0: counts_out int64 [batches][n_idx][n_idx], entry (i, j) = the rows in which elements i and j both carry a label
 *           and the same one; the diagonal = the rows in which the element carries a label at all;
 *   per_label != 0: counts_out int64 [batches][n_labels][n_idx][n_idx], entry (k, i, j) = the rows with z_i == k and z_j == k:
 *           (Z[:, :, None] == k) & (Z[:, None, :] == k) summed over the rows -- for spike-and-slab the joint inclusion count of two
 *           coefficients.  Its diagonal is the marginal label count (omc_store_histogram on the edges 0, 1, .., K), its sum over
 *           k the plain form;
 *   flags_out int64 [batches][n_idx][2] = {NaN draws, other non-label draws} of every selected element; may be NULL.
 *   out == out' bit for bit: one triangle of tiles is computed and mirrored.
 * One read of the selected columns turns every draw into a byte; the counts are the Gram product of the one-hot int8 indicators
 * of the labels on the int8 matrix cores, accumulated in int32 over slices of fewer than 2^31 rows and joined in int64.  Every
 * result is an exact integer: repeated calls are bit-equal.  Runs on the context's stream; workspace from the context (the
 * label bytes of at most 1 GiB of rows at a time, the slices' partial tiles).                                              */
omc_status omc_store_coalloc(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx, int64_t n_idx,
                             int32_t n_labels, int32_t pooled, int32_t per_label, int64_t* counts_out, int64_t* flags_out);
/* Least-squares partition (Dahl 2006) of the same selection: the stored state whose co-membership matrix is nearest to the
 * similarity matrix, which is the stored state of least posterior expected Binder loss.
 *   counts  int64 [batches][n_idx][n_idx] (device): the per_label == 0 output of omc_store_coalloc for the same arguments;
 *   score_out int64 [n_iter][C]: for the stored state s of batch b, over positions i < j of the selection,
 *           score = sum_{i<j} [z_i^s == z_j^s] (R_b - 2 counts[b][i][j])
 *           = R_b sum_{i<j} (c_ij^s - counts_ij / R_b)^2 minus a term that does not depend on s, an exact integer:
 *           ((Z[s][:, None] == Z[s][None, :]) * np.triu(R - 2 * counts, 1)).sum();
 *   best_out int64 [batches][2] = {row of the first minimum of the batch's scores, that score}: np.argmin's first-minimum rule;
 *           the row is it C + c pooled and it per chain.
 *   n_idx (n_idx - 1) / 2 x R >= 2^62 is OMC_UNSUPPORTED.
 * One read of the selected columns (the same bytes); the compares run on the vector ALU against tiles of R - 2 counts in LDS, the
 * partial scores are added with 64-bit integer atomics: repeated calls are bit-equal.  Runs on the context's stream.      */
omc_status omc_store_partition_score(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx,
                                     int64_t n_idx, int32_t n_labels, int32_t pooled, const int64_t* counts, int64_t* score_out,
                                     int64_t* best_out);
/* Ranks of the draws of every selected element of the same store; store, idx, n_idx, the NULL convention and the out-of-range rule
 * as omc_store_minmax (an index outside [0, size) is OMC_INVALID_ARG, found on the device before any output is written).
 * With N = n_iter >= 4: M = N / 2, J = 2 C, S = J M; the SPLIT DRAWS of an element are the first M and the last M iterations of
 * every chain (the middle row of an odd N is dropped, as omc_store_rhat_ess drops it).
 *   rank_out [N][C][n_idx] fp64: the 1-based average rank of the draw x among the element's draws y,
 *            r = #{y < x} + (#{y == x} + 1) / 2 -- scipy.stats.rankdata(method="average"), bit for bit (integers and halves);
 *   split != 0: among the S split draws, the dropped middle row is written as NaN, N >= 4 (else OMC_INVALID_ARG);
 *   split == 0: among all N C draws, N >= 1.
 *   -0.0 and +0.0 are equal; +-inf are ordinary values; an element with any NaN draw (the dropped row included) gets NaN in its
 *   whole column and affects nothing else.
 * A chunk of elements at a time: their draws are gathered as order-preserving 64-bit keys into columns padded to the next power of
 * two P >= S, every column is sorted by a key-only bitonic network (data-independent addressing; strides inside a tile of T keys
 * in LDS, larger strides one pass over global memory each: omc_store_rank_schedule), and every draw finds the keys below and equal
 * to its own by bisection.  Options "rank_tile" (T) and "rank_chunk" (elements per chunk; by default what fits a workspace of
 * 1 GiB at 8 P bytes per element, at least one): same results bit for bit.  Workspace from the context (its own, not the one of
 * the other store summaries).  With d = log2(P / T) the sort is d + 1 launches over tiles and d (d + 1) / 2 global passes of 16
 * bytes per key: meant for the elements one inspects, not for every element of a long store.                              */
omc_status omc_store_ranks(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx, int64_t n_idx,
                           int32_t split, double* rank_out);
/* Rank-normalised convergence diagnostics of the same store (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021; what Stan and
 * ArviZ report by default), per selected element; store, idx, n_idx as omc_store_ranks, N = n_iter >= 4 (else OMC_INVALID_ARG).
 * E(.) and R(.) are the ess and the rhat omc_store_rhat_ess defines for an [N][C] series; all of its edge rules carry over.
 *   z        = ndtri((r - 3/8) / (S + 1/4)), r the split rank of the draw (the dropped middle row is 0: it is never read);
 *   ess_bulk = E(z);
 *   f = |x - med|, med = np.median of the split draws ((a + b) / 2 of the two middle order statistics), zf = f rank-normalised
 *            the same way;  rhat = max(R(z), R(zf)), NaN when either is NaN;
 *   q_p      = np.quantile of the split draws, default "linear" method, p = 0.05 and 0.95 (the two order statistics read from the
 *            sorted column, numpy's interpolation operation by operation as in omc_store_quantiles: bit-equal);
 *            I_p = (x <= q_p) ? 1 : 0;  ess_tail = min(E(I_05), E(I_95)).
 *   An element with any non-finite draw (NaN or +-inf, any chain, any iteration) gives NaN in all three outputs and affects nothing
 *   else.  A constant element gives rhat = NaN and ess = S (the rules of omc_store_rhat_ess on constant series).
 *   rhat_out, ess_bulk_out, ess_tail_out [n_idx]; any of them may be NULL.
 * Per chunk of elements: the sort of omc_store_ranks twice (the draws, the folded draws), the four series z, zf, I_05, I_95 side
 * by side as a store [N][C][4 Kc], and one call of omc_store_rhat_ess over them (options "diag_algo" applies).  The chunk is what
 * fits 1 GiB at 8 P + 32 N C bytes per element ("rank_chunk" forces it: same results to rounding, the grouping of the lag sums
 * depends on the size).  Deterministic: repeated calls are bit-equal.                                                       */
omc_status omc_store_rank_diagnostics(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx,
                                      int64_t n_idx, double* rhat_out, double* ess_bulk_out, double* ess_tail_out);
/* The effective sample size of indicator series of the same store: ArviZ's ess(method="quantile") and ess(method="local"), the
 * numbers that say whether a reported quantile or interval end point has converged.  store, idx, n_idx, the NULL convention and the
 * out-of-range index rule as omc_store_rank_diagnostics; N = n_iter >= 4 (else OMC_INVALID_ARG); M = N / 2, J = 2 C, S = J M, the
 * split draws those of omc_store_rhat_ess (the middle row of an odd N is dropped, and read only for its NaN / inf).
 *   prob_lo, prob_hi [n_p] on the HOST, 1 <= n_p <= 32.  prob_lo[i] < 0: no lower end, I = (x <= q_hi) (ArviZ's _ess_quantile);
 *            otherwise 0 <= lo <= hi <= 1 and I = (q_lo <= x && x <= q_hi) (_ess_local).  Anything else (NaN included) is
 *            OMC_INVALID_ARG, found before any launch.
 *   q_p      = np.quantile of the element's S split draws, default "linear" method, read from the sorted column with numpy's
 *            interpolation operation by operation (bit-equal).  For an even N this is ArviZ's quantile of all draws; for an odd N
 *            it differs from it by the dropped row.
 *   With b_j[0..M) the 0/1 series of one (element, interval), all exact in int64:
 *     n_j = sum_s b_j[s],  Nn = sum_j n_j,  Q = sum_j n_j^2,
 *     A(t) = sum_j sum_{s < M - t} b_j[s] b_j[s + t],
 *     H(t) = sum_j n_j (sum_{s < M - t} b_j[s] + sum_{s >= t} b_j[s]),
 *     Z(t) = M^2 A(t) - M H(t) + (M - t) Q                (Z(0) = M (M Nn - Q)),
 *   and in omc_store_rhat_ess's notation S(t) = (double)Z(t) / ((double)M (double)M),
 *   B_M = (double)(J Q - Nn^2) / ((double)M (double)M (double)J (double)(J - 1)); W, var_plus, rho(t), Geyer's initial monotone
 *   sequence, the floor on tau and every edge rule are those of omc_store_rhat_ess, one copy of the code: a constant series (every
 *   draw inside, or every draw outside the interval) gives ess = J M with lags 0, and W == 0 < B_M runs to the M - 3 limit.
 *   Z(t) and J Q - Nn^2 must be exact: J M^3 >= 2^62 or J M >= 2^31 is OMC_UNSUPPORTED.
 *   ess_out [n_p][n_idx] fp64; lag_out [n_p][n_idx] int32, the lags the sequence used (as omc_store_rhat_ess);
 *   q_out [n_p][n_idx][2] fp64: the thresholds q_lo, q_hi, [..][0] NaN where there is no lower end;
 *   counts_out [n_p][n_idx][2 + 2 n_cnt] int64 = Nn, Q, then the pairs A(t), H(t) for t < n_cnt, 0 <= n_cnt <= M (else
 *            OMC_INVALID_ARG): when given, these lags are evaluated whether or not the sequence needs them (for tests).
 *   Any output may be NULL.  An element with any non-finite draw (NaN or +-inf) gives NaN, lags 0 and zero counts in every
 *   interval (its q_out is whatever the interpolation gives) and affects nothing else.
 *   algo: 0 auto, 1 the bits of a column staged in LDS (8 J ceil(M / 64) + 4 J <= 144 KiB, else OMC_INVALID_ARG; two workgroups
 *   share a compute unit up to half of that), 2 the bits read from global memory / L2.  0 takes form 1 where it fits.
 * Per chunk of elements: the gather and the sort of omc_store_ranks with the split geometry, the thresholds, one read of the
 * chunk's columns that packs 64 draws into a word per interval (bits [Kc][n_p][J][ceil(M / 64)], every series on its own word,
 * the bits past M zero), and one launch in which a workgroup per (element, interval) walks its own Geyer sequence to the end in
 * blocks of 64 lags -- popcounts of a word ANDed with its shifted successor -- with no host round trip.  Every sum is an integer
 * and the fp64 steps follow one fixed sequence from them: repeated calls, any "rank_tile", any "rank_chunk" and both forms are
 * BIT-EQUAL.  No floating-point atomics.  Workspace from the context's rank workspace: 8 P + n_p (8 J ceil(M / 64) + 4 J + 16)
 * bytes per element of a chunk.                                                                                          */
omc_status omc_store_ess_indicator(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx, int64_t n_idx,
                                   const double* prob_lo, const double* prob_hi, int32_t n_p, int32_t algo, double* ess_out,
                                   int32_t* lag_out, double* q_out, int64_t* counts_out, int64_t n_cnt);
/* Order statistics of the same store at given positions: out [n_idx][n_pos] fp64 = sorted column of element e at pos[e][k], pos
 * [n_idx][n_pos] int64 on the DEVICE; store, idx, n_idx as omc_store_ranks.  split != 0: the column is the S split draws (n_iter
 * >= 4), else all n_iter C draws.  A position outside the column is OMC_INVALID_ARG, found on the device (with the index check,
 * one read-back) before out is written.  An element with a NaN draw gives NaN.  Equal to np.sort(column)[pos], except that a zero
 * comes back as +0.0 (the keys merge the two zeros).  The gather and the sort of omc_store_ranks, then a pick; options "rank_tile"
 * and "rank_chunk" apply: same bits.  What mcse_quantile needs: its positions depend on the ESS through a beta quantile the host
 * evaluates.                                                                                                              */
omc_status omc_store_order_stats(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx, int64_t n_idx,
                                 int32_t split, const int64_t* pos, int64_t n_pos, double* out);
/* [host, no GPU] The launches that sort columns of S keys with tiles of `tile` keys (0 = 8192, or a power of two 64 .. 8192, else
 * OMC_INVALID_ARG; S >= 1): P = the next power of two >= S, T = min(tile, P); out [cap][3] = (kind, k, j) per launch, *n_out their
 * number (set also when cap is too small, which is OMC_INVALID_ARG).  A compare-exchange at stride j of stage k orders the keys at
 * positions i and i + j (bit j of i clear) ascending where bit k of i is clear, descending otherwise.
 *   kind 0: every tile, all stages k' = 2, 4 .. k (= T), each with its strides k' / 2 .. 1 (j = T / 2 is given for information);
 *   kind 1: one stride j >= T of stage k over global memory;
 *   kind 2: every tile, the strides j (= T / 2), j / 2 .. 1 of stage k.
 * P = 1 needs no launch; otherwise 1 + d launches of kinds 0 and 2 and d (d + 1) / 2 of kind 1, d = log2(P / T).            */
omc_status omc_store_rank_schedule(int64_t S, int32_t tile, int64_t* out, int64_t cap, int64_t* n_out);
/* Highest-density intervals of the same store: per selected column of draws the shortest interval that holds a share `prob` of
 * them (ArviZ's unimodal hdi, what az.summary prints as hdi_3% / hdi_97%); store, idx, n_idx, the NULL convention and the
 * out-of-range rule as omc_store_ranks.  A column is all n_iter * C draws of an element (per_chain == 0) or the n_iter draws of
 * one chain of it (per_chain != 0).  For a column with n valid draws sorted ascending x[0 .. n) and 0 < prob < 1:
 *   m    = min(floor(prob * n), n - 1)              (the fp64 product, as numpy's float64 * int)
 *   w[i] = x[i + m] - x[i],  i = 0 .. n - m - 1     (one fp64 subtraction each)
 *   i*   = the FIRST index of the minimum of w      (np.argmin)
 *   hdi  = (x[i*], x[i* + m])
 *   Both limits are stored draws, no arithmetic is done on them: results are exact.  -0.0 and +0.0 are one value (a zero limit
 *   comes out as +0.0).  m == 0 (prob * n < 1) gives (x[0], x[0]); n == 0 gives (NaN, NaN); a column with a +-inf draw gives
 *   (NaN, NaN) and affects nothing else.  omit_nan != 0: NaN draws are left out and n is the number of the others;
 *   omit_nan == 0: a column with any NaN draw gives (NaN, NaN).
 *   probs [n_probs] on the HOST, 1 <= n_probs <= 8, every one inside (0, 1), else OMC_INVALID_ARG (NaN included);
 *   out [n_probs][n_idx][2] or, per chain, [n_probs][C][n_idx][2] fp64: lower and upper limit;
 *   n_valid_out (may be NULL) [n_idx] or [C][n_idx] int64: the non-NaN draws of the column, whatever omit_nan says.
 * A chunk of elements at a time (per chain: C columns per element): the gather and the sort of omc_store_ranks, with NaN draws on
 * the all-ones key of the padding, n by bisection for that key, and one pass over the sorted column for all probabilities that
 * keeps the minimum of the pairs (w, i) in lexicographic order, compared as integers, so that ties go to the lowest i in whatever
 * order lanes, waves and workgroups are combined: repeated calls are bit-equal.  A column of up to 4096 draws is one wave's work; longer ones are
 * cut into slices of 16384 windows, a workgroup each, with a second small launch where there are several; the slicing depends on the column length alone.  Options "rank_tile" and
 * "rank_chunk" apply: same results bit for bit.  Workspace as omc_store_ranks (8 P bytes per column and a few words).        */
omc_status omc_store_hdi(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx, int64_t n_idx,
                         const double* probs, int32_t n_probs, int32_t per_chain, int32_t omit_nan, double* out,
                         int64_t* n_valid_out);
/* Per-draw reductions of the same store: one number per stored state (iteration, chain) over the selected elements of its row --
 * np.nansum(MCMC.store[param], axis=0) and kin (np.nanmax, np.nanargmax, np.count_nonzero(x > t, axis=0) ...) on the reference's
 * host arrays (mcmc.py:105-111): the field's maximum and where it sits, the area above a threshold, a contrast w'x, the live size
 * and the total of a NaN-padded variable-size parameter, the maximal standardised deviation behind a simultaneous band.  The
 * result is shaped like log_post, so every other summary of the store applies to it.
 *   store, idx, n_idx and the NULL convention as omc_store_minmax (order kept, repeats allowed, n_idx may exceed size); an index
 *   outside [0, size) is OMC_INVALID_ARG, found on the device before any output is written.  Selection position k = 0 .. n_idx - 1
 *   is element idx[k] of the row (k itself without an index) with value x.
 *   a, b      (device) [n_idx], aligned with the selection (position k), not with size; NULL where the op does not need them.
 *   out       [n_iter][C] fp64;  count_out (may be NULL) [n_iter][C] int64: the selected elements of the row whose TERM is not NaN.
 *     op                     term of position k                     result of the row
 *     OMC_REDUCE_SUM         a[k] * x  (a == NULL: x)               the sum of the terms
 *     OMC_REDUCE_MIN / MAX   x                                      the smallest / largest term
 *     OMC_REDUCE_ARGMIN / ARGMAX  x                                 the position k (as a double) of the FIRST smallest / largest term
 *     OMC_REDUCE_COUNT_ABOVE x                                      the number of positions with x > a[k]  (a required)
 *     OMC_REDUCE_SUPNORM     fabs(x - a[k]) / b[k]                  the largest term  (a and b required; one IEEE subtraction and
 *                                                                   one IEEE division per term: nothing fused, no reciprocal)
 *   NaN terms (a NaN draw; 0 / 0 under SUPNORM for an element that never moved):
 *     omit_nan != 0: they are left out.  A row without a term left gives 0 for SUM (np.nansum) and for COUNT_ABOVE, NaN otherwise.
 *     omit_nan == 0: a NaN term makes SUM, MIN, MAX and SUPNORM NaN; ARGMIN / ARGMAX give the position of the first NaN term
 *                    (numpy's rule); COUNT_ABOVE does not count it.
 *   +-inf are ordinary values; -0.0 and +0.0 are equal (the first of them is the extreme).
 *   OMC_INVALID_ARG, with a text in omc_last_error: an unknown op, a required vector that is NULL, n_iter < 1, size < 1.
 * Everything but SUM is exact and does not depend on how the work is cut.  SUM adds the terms a lane owns in ascending position and
 * the lanes in a fixed butterfly: |SUM - exact sum of the terms| <= n_idx 2^-53 sum |term| (products rounded or fused), and the order
 * depends on the form, on (size, n_idx) and on the row's alignment to 16 bytes only: repeated calls are bit-equal.  No atomics.
 * Two forms, option "reduce_algo" (0 automatic, 1 short, 2 long): long rows get one wave each (four from 32768 selected elements), 16-byte
 * loads without an index, a gathered 8-byte load per lane with one; short rows (automatic: size <= 128) are staged, a tile of
 * consecutive rows at a time, into LDS with 16-byte loads and reduced there by a power-of-two group of lanes per row.  A row
 * that does not fit 48 KiB of LDS takes the long form whatever the option says.  One read of the store, 8 or 16 bytes written
 * per row.  Runs on the context's stream; with an index the host reads one word back (the validation; workspace store_ws).        */
enum { OMC_REDUCE_SUM = 0, OMC_REDUCE_MIN = 1, OMC_REDUCE_MAX = 2, OMC_REDUCE_ARGMIN = 3, OMC_REDUCE_ARGMAX = 4,
       OMC_REDUCE_COUNT_ABOVE = 5, OMC_REDUCE_SUPNORM = 6 };
omc_status omc_store_reduce(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx, int64_t n_idx,
                            int32_t op, int32_t omit_nan, const double* a, const double* b, double* out, int64_t* count_out);
/* First failures of the stored states of the same store against per-element sides: the integer counts from which joint excursion
 * sets, contour-avoiding sets, contour credible regions and the reliability of a contour map are computed (Bolin and Lindgren
 * 2015, 2017; R's excursions) -- "over which set of elements is the field above u at ALL of them at once with probability 0.95",
 * which the pointwise P(x_k > u) of a histogram cannot answer.  On host arrays it is a (rows x n_idx) boolean temporary and a
 * permuted argmax; here it is one read of the store for up to 8 slots.
 *   store, idx, n_idx and the NULL convention as omc_store_reduce (order kept, repeats allowed, n_idx may exceed size); an index
 *   outside [0, size) is OMC_INVALID_ARG, found on the device before any output is written.  Selection position k = 0 .. n - 1,
 *   n = n_idx, is element idx[k] of the row (k itself without an index) with value x.  Rows s = 0 .. R - 1, R = n_iter C, pooled
 *   over chains.
 *   One SLOT l = 0 .. n_slots - 1 is a triple of device arrays aligned with the selection (position k), the tables [n_slots][n]:
 *     lo, hi   fp64 bounds; -inf and +inf mean "no bound on that side"
 *     pos      int32, a permutation of 0 .. n - 1: the place of element k in the order in which the slot's elements are taken
 *   Row s AGREES at k iff  x == x && (lo[k] == -inf || x > lo[k]) && (hi[k] == +inf || x < hi[k]):
 *     a NaN draw is on no side; +-inf draws are ordinary values (a -inf draw agrees with lo = -inf, not with any finite lo);
 *     bounds are strict (a draw equal to a bound does not agree).
 *   The FIRST FAILURE of row s is  r_s = min({pos[k] : s does not agree at k} u {n}): an integer minimum, the same however the
 *   work is cut.
 *   h_out     [n_slots][n + 1] int64:  h[j] = #{s : r_s == j}.
 *   rows_out  [n_slots][n_iter][C] int32 (may be NULL): r_s itself.
 *   From h the caller has J[j] = R - sum_{i <= j} h[i], the rows that agree at all of the first j + 1 elements of the order, and the
 *   excursion function F_k = J[pos[k]] / R (one IEEE division per element).  Counts taken by several contexts over the same
 *   tables -- chains sharded over ranks -- add.
 *   Only the range of pos is checked, on the device before any output is written; a pos that is no permutation gives the h the
 *   definition above gives.
 *   algo      0 automatic, 1 the short form, 2 the long form (below): tests and A/B runs reach each form on any shape.  It is an
 *             argument, not a context option like "reduce_algo": the forms give the same integers, so nothing else depends on it.
 *   OMC_INVALID_ARG, with a text in omc_last_error and the outputs untouched: ctx, store, lo, hi, pos or h_out NULL, n_iter < 1,
 *     size < 1, n_idx < 1 (or no index and n_idx != size), n_idx > 2^31 - 2, n_slots outside 1 .. 8, algo outside 0 .. 2, an index
 *     outside [0, size), a pos entry outside [0, n_idx), more than 2^31 - 1 workgroups.
 * No floating point reaches a result: r is a minimum of int32, h is added with 64-bit integer atomics.  Repeated calls and both
 * forms are equal in every bit.
 * How: one read of the store for all slots.  Long rows: a workgroup owns 32 consecutive rows, a wave eight of them one after the
 * other; 16-byte loads without an index (a row that starts 8 bytes off a 16-byte boundary gives its first element to lane 0, a
 * last element without a partner goes to lane 63), a gathered 8-byte load per lane with one.  Short rows (automatic: size <= 128,
 * omc_store_reduce's crossover) are staged, a tile of consecutive rows at a time, into LDS with 16-byte loads and walked by a
 * power-of-two group of lanes per row; a row that does not fit 40 KiB of LDS takes the long form whatever algo says.  A lane
 * keeps n_slots running minima (1, 2, 4 or 8 registers), lanes are joined by a butterfly of integer min.  The slot tables, 20
 * n_slots bytes per selected element, are read through the caches (a wave needs the tables of the whole row; at n = 10 000 and 8
 * slots they are 1.6 MB: more than a workgroup's LDS, less than an XCD's L2).  The r of a workgroup's rows meet in LDS, where the
 * first of equal values within 32 rows adds their number to h with one atomic: to h_out, or in the short form, where
 * n_slots (n + 1) <= 2048, to counters in LDS, which the workgroup adds to h_out after its last rows (at most eight workgroups per
 * compute unit walk the rows).  No scratch.  Workspace (store_ws): two words,
 * which the host reads back (the validation).  Runs on the context's stream.                                                   */
omc_status omc_store_first_failure(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx,
                                   int64_t n_idx, int32_t n_slots, const double* lo, const double* hi, const int32_t* pos,
                                   int32_t algo, int64_t* h_out, int32_t* rows_out);
/* Autocovariance, autocorrelation and integrated autocorrelation time of the same store: the plot next to the trace, and the
 * one principled way to choose a thinning.  store, idx, n_idx and the NULL convention as omc_store_reduce (order kept, repeats
 * allowed, n_idx may exceed size); an index outside [0, size) is OMC_INVALID_ARG, found on the device before any output is written.
 * With N = n_iter, L = max_lag, u = 2^-53, for chain c and selection position k with draws x[0 .. N):
 *   m      = the column's mean as omc_col_moments gives it on the per-chain view of the selection (Welford's and Chan's updates:
 *            exact for equal draws); written to mean_out [C][n_idx] (may be NULL)
 *   d_i    = x_i - m                                           (one IEEE subtraction)
 *   s_c(t) = sum_{i = 0}^{N - 1 - t} d_i d_{i + t},  t = 0 .. L   (products rounded or fused)
 *   per_chain != 0: acf_out [C][n_idx][L + 1] = g(t) = s_c(t) / N                        (one division)
 *   per_chain == 0: acf_out [n_idx][L + 1]    = g(t) = S(t) / (N C),  S(t) = sum_c s_c(t), the chains added in ascending c: the
 *                   chains' autocovariances around their OWN means, averaged
 *   normalize != 0: g(t) / g(0) instead, one more IEEE division of the two rounded values (bit-equal to dividing the
 *                   normalize == 0 result by its lag-0 entry)
 *   tau_out [C][n_idx] or [n_idx] (may be NULL): the integrated autocorrelation time by Geyer's initial positive sequence on
 *                   rho(t) = g(t) / g(0): tau = -1, then for k = 0, 1, ... while 2 k + 1 <= L and G = rho(2 k) + rho(2 k + 1) > 0:
 *                   tau += 2 G (sequential fp64 additions in that order)
 *   window_out, int32, shaped like tau_out (may be NULL): the lags used, 2 * (pairs taken).  window >= L (L odd) or >= L - 1
 *                   (L even): the sequence ran into max_lag, tau is a lower bound -- raise max_lag.
 * Edge rules.  A column whose mean is not finite -- a NaN draw, or an infinite one, which is not special-cased: its deviation is
 * inf - inf -- gives NaN in every lag; per chain that column only, pooled that element only.  A column whose draws all equal its
 * first draw (compared as values) has s(t) = 0 exactly, whatever the mean rounds to; pooled it adds 0 to S.  Where rho(0) = g(0) / g(0)
 * is NaN (g(0) NaN, zero -- every contributing draw equal -- or infinite) the normalised lags are NaN by that division, tau is
 * NaN and window is 0.
 * OMC_INVALID_ARG, with a text in omc_last_error and the outputs untouched: n_iter < 2, size < 1, max_lag < 0,
 * max_lag > n_iter - 1, n_idx < 1 (or no index and n_idx != size), store or acf_out NULL, an index outside [0, size), more than
 * 65535 time slices or blocks of 32 lags.
 * Accuracy: |s(t) - exact sum of d_i d_{i+t}| <= (terms + 1) u sum |d_i d_{i+t}|, terms = N - t per chain and C (N - t) pooled:
 * the bound of any order of additions of rounded or fused products (as omc_store_reduce's SUM).  The order of additions depends
 * on N, L, C and option "autocorr_slice" only -- not on size, n_idx or the index --; no floating-point atomics; repeated calls
 * are bit-equal and so are the rows of repeated index entries.
 * How: a chunk of selected elements at a time (C columns per element).  The means; a pre-pass that flags, per column, a draw that
 * differs from the first and a mean that is not finite (integer OR) and, with an index, gathers the centred draws into a
 * compact [N][C chunk] workspace (without an index the store is read where it lies and centred on load); the lag kernel, one
 * lane per column, consecutive lanes on consecutive columns, grid = column tiles x blocks of 32 lags x time slices, each block of
 * lags 32 accumulators and a 32-slot register ring (two loads per 32 FMAs), four adjacent blocks of lags to a workgroup; a slice owns the products
 * whose left factor lies in its rows and reads up to L rows past its end; partials [slice][lag][column] are added slices first,
 * then chains, both ascending, divided, normalised, and walked by the Geyer loop.  Slices are 2048 rows (option "autocorr_slice":
 * 0 = that, else rows per slice, at least 1; results for different settings agree within the bound, not bit for bit), so a few
 * long columns still fill the device.  Workspace (rank_ws): per column 256 (L / 32 + 1) bytes per slice, 8 (L + 1) bytes, 8 N bytes
 * with an index, one word; the chunk is what fits 1 GiB, at least one element (option "rank_chunk" forces it), so the workspace stays bounded by
 * 1 GiB, or by one element's C columns where those alone need more, however large the store is.  Store bytes read: the means' and
 * the pre-pass's one read each of the selected columns; without an index the lag kernel's 2 (L / 32 + 1) loads of every row,
 * which the waves of a workgroup share through the caches.  Runs on the
 * context's stream; with an index the host reads one word back (the validation).                                              */
omc_status omc_store_autocorr(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx, int64_t n_idx,
                              int64_t max_lag, int32_t per_chain, int32_t normalize, double* acf_out, double* tau_out,
                              int32_t* window_out, double* mean_out);
/* Linear maps and posterior-predictive draws of the same store: m numbers per stored state (iteration, chain), each a linear
 * combination of the selected elements of its row -- the fitted curve A beta on a grid, a set of contrasts or regional totals, the
 * predictor of a reversible-jump model summed over its live components, the replicates y_rep = A beta + eps / sqrt(tau) of a
 * posterior-predictive check: the loop over MCMC.store[...] of the reference that calls LinearCombination.predictor / Normal.rvs per
 * stored draw.  The result is shaped like a store entry [n_iter][C][m], so every other summary of the store applies to it.
 *   store, idx, n_idx and the NULL convention as omc_store_reduce (order kept, repeats allowed, n_idx may exceed size); an index
 *   outside [0, size) is OMC_INVALID_ARG, found on the device before anything reads through it; out is then untouched.  Selection
 *   position k = 0 .. n_idx - 1 is element idx[k] of the row (k itself without an index) with value x[k].
 *   W         (device) [m][n_idx], row stride ld_w >= n_idx;   offset (device) [m] or NULL
 *   base      (device) [n_iter][C][m] or NULL; may be out itself (accumulate in place: an element is read and written by the same thread)
 *   prec      (device) [n_iter][C][prec_size], prec_size 0 (no noise; prec NULL), 1 or m;   z_inject (device) [n_iter][C][m] or NULL
 *   out       (device) [n_iter][C][m]:
 *     out[it][c][j] = base[it][c][j] + offset[j] + sum_k W[j][k] x[k]   (+ z[it][c][j] / sqrt(prec[it][c][j or 0]) with prec_size > 0)
 *   NaN.  omit_nan != 0: a NaN x[k] is left out -- its term is 0 whatever W[j][k] is (np.nansum of the terms; the NaN padding of a
 *     variable-size parameter means "component absent"); a row with nothing left gives base + offset.  omit_nan == 0: plain IEEE, as
 *     store2d[:, idx] @ W.T in numpy: a NaN among the selected elements of a row makes all m outputs of that row NaN, inf * 0 is NaN.
 *     Rows, columns and positions that pad a tile never reach a written output.
 *   Noise.  z is z_inject where given (the library's convention for path-wise replays), else element j of the chain's normal
 *     stream (purpose OMC_RNG_NORMAL, global chain chain_id_offset + c) at draw index (1 << 41) + it + (replicate << 44),
 *     replicate 0 .. 15: a pure function of (seed, global chain, it, j, replicate), whatever the launch geometry and however the
 *     chains are sharded.  One IEEE square root and one IEEE division per term; a precision that is not positive gives what IEEE
 *     gives (inf, NaN).
 *   OMC_INVALID_ARG, with a text in omc_last_error: ctx, store, W or out NULL, n_iter < 1, size < 1, m < 1, n_idx < 1 (or no index
 *     and n_idx != size), ld_w < n_idx, prec_size not 0, 1 or m, prec and prec_size not given together, z_inject without prec,
 *     replicate > 15, an index outside [0, size), more than 2^31 - 1 tiles of 64 rows or 65535 tiles of 128 outputs.
 * Guarantees.  The contraction of a row is never split across workgroups and uses no atomics.  The order in which a row's terms
 * are added depends on (n_idx, m) and the kernel's constants only -- not on the row's position, on R = n_iter C, on C or on the
 * row's alignment.  So repeated calls are bit-equal, and a row's outputs are bit-equal however the rows are regrouped: fewer
 * iterations, or chains sharded over contexts (the noise included).  Error of the linear part:
 *   |out - exact| <= (n_idx + 2) 2^-53 (|base| + |offset| + sum_k |W[j][k] x[k]|),
 * the bound of any order of additions of rounded or fused products (the form omc_store_reduce and omc_store_autocorr state).
 * How: one kernel family on v_mfma_f64_16x16x4_f64.  A workgroup owns 64 rows and 128 output columns (with m <= 64: 128 rows and
 * 64 columns, the same additions in the same order) and walks the whole contraction in slabs of 32 positions; rows and the W slab are staged in LDS (16-byte loads along the row without an index when
 * size is even and store 16-byte aligned, else 8-byte loads, gathered through the index where there is one; NaN zeroed on the
 * way in), the next slab is fetched under the multiplications, blocks of 16 columns without a real output are skipped.  With
 * m <= 128 the store is read exactly once; wider m takes a second grid dimension over column tiles, each reading the store.
 * No scratch.  Workspace: the word of the index check (store_ws); with an index the host reads that word back.  Runs on the
 * context's stream.                                                                                                            */
omc_status omc_store_project(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx, int64_t n_idx,
                             int64_t m, const double* W, int64_t ld_w, const double* offset, const double* base, int32_t omit_nan,
                             const double* prec, int64_t prec_size, const double* z_inject, uint64_t replicate, double* out);
/* Column summaries of the pointwise Normal log-density of the same store: what WAIC needs of a fitted model, and the pointwise
 * entry itself -- the loop over MCMC.store[...] of the reference that calls Normal.log_p(..., by_observation=True) per stored draw
 * (distribution/location_scale.py:145-166), reduced over the draws while the entry is read.
 *   store is a MEAN entry [n_iter][C][size] (a stored parameter, or what omc_store_project made); idx, n_idx and the NULL
 *   convention as omc_store_reduce (order kept, repeats allowed); an index outside [0, size) is OMC_INVALID_ARG, found on the
 *   device before anything reads through it.  Selection position k is element idx[k] of a row (k itself without an index).
 *   y     (device) [n_idx], aligned with the selection
 *   prec  (device) [n_iter][C][prec_size], prec_size 1 or n_idx
 * With S = n_iter C >= 2 rows, c = 0.5 log(2 pi) rounded to fp64, and for row s and position k the element x and precision tau:
 *     h  = 0.5 log(tau) - c            (one fused multiply-add; with prec_size == 1 one logarithm per ROW, not per element)
 *     r  = y[k] - x                    (one IEEE subtraction)
 *     ll = h - (0.5 tau r) r           (0.5 tau exact, one rounded product, one fused multiply-add)
 *   lse_out  [n_idx]  log sum_s exp(ll)         mean_out [n_idx]  the mean of ll over s
 *   var_out  [n_idx]  its unbiased variance (divisor S - 1)
 *   ll_out   [n_iter][C][n_idx]  ll itself, in the store's layout (whatever IEEE gives)
 *   Any output may be NULL, not all.  A column that holds an ll that is not finite -- a NaN or infinite element, a precision that
 *   is not positive and finite -- gives NaN in lse, mean and var; no other column is affected.
 *   OMC_INVALID_ARG, with a text in omc_last_error and every output untouched: ctx, store, y or prec NULL, S < 2, size < 1,
 *     n_idx < 1 (or no index and n_idx != size), prec_size not 1 or n_idx, every output NULL, an index outside [0, size).
 * How: one read of the entry, 8 bytes written per element only with ll_out.  A workgroup owns 32 adjacent selection positions
 * and a slice of the rows (about 2048 workgroups, no slice shorter than 256 rows, at most 1024 slices: omc_store_moments' rule);
 * lanes run along the row -- 16-byte loads without an index where size is even and store 16-byte aligned, else 8-byte loads -- and
 * 16 row lanes walk down it.  A lane carries the running maximum M and the rescaled sum s (one exp per element) next to Welford's
 * update; lanes and slices are joined in a fixed order, (M, s) pairs by M = max and one rescaling, moments by Chan's update.  No
 * atomics: slices and order are functions of the shape alone, so repeated calls are bit-equal (and the two load forms give the
 * same bits).  Error of lse: with E = max_s (|0.5 log tau| + c + 0.5 tau r^2) and u = 2^-53, within 4 u E + (K + 4) u + u |lse| of the
 * exact value, K = 2 ((L - 1) + (min(16, rows) - 1) + (slices - 1)) <= 2 (S - 1) the roundings a term passes through, rows the
 * rows of a slice and L = ceil(rows / 16).  No scratch.  Workspace (store_ws): 40 n_idx bytes per slice, 8 S bytes with
 * prec_size == 1, the word of the index check; with an index the host reads that word back.  Runs on the context's stream.     */
omc_status omc_store_loglik(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx, int64_t n_idx,
                            const double* y, const double* prec, int64_t prec_size, double* lse_out, double* mean_out,
                            double* var_out, double* ll_out);
/* Pareto-smoothed importance sampling leave-one-out (PSIS-LOO; Vehtari, Simpson, Gelman, Yao, Gabry 2024 -- what az.loo reports)
 * per selected column of the same store: the expected log predictive density of the observation with itself left out, and the
 * Pareto k of its importance ratios.  store, idx, n_idx as omc_store_loglik.  With y == NULL (then prec NULL) store is an entry
 * of pointwise log-likelihoods read as it lies; else it is a mean entry and ll is computed on load from y, prec, prec_size as
 * omc_store_loglik computes it (the same inline function: the two routes are bit-equal).
 *   tail_max (device) int64 [n_idx], 1 <= tail_max[k] <= S - 1, S = n_iter C >= 2; anything else is OMC_INVALID_ARG, found on the
 *   device before any output is written (as an index outside [0, size)).
 * Per column, every ll_s finite:
 *   1. x_s = (-ll_s) - max_s(-ll_s), sorted ascending x_(0) .. x_(S-1); M = tail_max[k].
 *   2. xc = max(x_(S-M-1), log(DBL_MIN) = -708.3964185322641); the tail is the T draws with x > xc (ties with the cut are not tail;
 *      T by bisection in the sorted keys, exact).
 *   3. T <= 4: k = +inf, nothing is smoothed.
 *   4. Else a_i = exp(x_(S-T+i)) - exp(xc), ascending, and the fit of Zhang and Stephens (2009) with the priors of Vehtari et al.
 *      (2024): n = T, m = 30 + floor(sqrt(n)), q = floor(n / 4 + 0.5) - 1; for i = 1 .. m:
 *        b_i = 1 / a_(n-1) + (1 - sqrt(m / (i - 0.5))) / (3 a_q),  k_i = (1/n) sum_j log1p(-b_i a_j),  L_i = n (log(-b_i / k_i) - k_i - 1),
 *        w_i = 1 / sum_j exp(L_j - L_i)  (an overflowing exp is +inf, the weight 0); candidates with w_i < 10 * 2^-52 are dropped, the
 *      rest divided by their sum; b = sum b_i w_i, k' = (1/n) sum_j log1p(-b a_j), sigma = -k' / b, k = (n k' + 5) / (n + 10).
 *   5. k finite: with p_i = (i + 0.5) / T the tail value x_(S-T+i) becomes log(sigma expm1(-k log1p(-p_i)) / k + exp(xc))
 *      (|k| < 2^-52: log(-sigma log1p(-p_i) + exp(xc)); sigma <= 0: NaN), then every x becomes min(x, 0).
 *   6. w = x - logsumexp(x), elpd = logsumexp_s(w_s + ll_s), each draw with its own weight: a draw outside the tail has
 *      w + ll = -max(-ll) - logsumexp(x), and the smoothed values go to the tail draws in ascending order.
 *   elpd_out [n_idx] fp64;  k_out [n_idx] fp64;  tail_out [n_idx] int64 = T, or NULL.
 *   A column with an ll that is not finite gives NaN, NaN and -1 and affects nothing else.
 *   OMC_INVALID_ARG, with a text in omc_last_error: ctx, store, tail_max, elpd_out or k_out NULL, S < 2, size < 1, n_idx < 1 (or no
 *     index and n_idx != size), y and prec not given together, prec_size not 1 or n_idx (with y), an index or a tail_max out of
 *     range, S beyond what the fit's 2048 candidate slots take (30 + floor(sqrt(S - 1)) > 2048: about 4 million draws).
 * How: a chunk of columns at a time -- the gather of omc_store_ranks (keys of -ll), the sort of omc_store_ranks, then one workgroup
 * per column that reads the sorted tail from the workspace (nothing assumes that a tail fits LDS).  Every sum is taken in an
 * order that depends on (S, T) alone: repeated calls are bit-equal, and options "rank_tile" and "rank_chunk" apply with the same
 * results bit for bit.  No scratch.  Workspace as omc_store_ranks (rank_ws: 8 P bytes per column and a few words).  The host reads
 * two words back (the validation).  Runs on the context's stream.                                                             */
omc_status omc_store_psis(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx, int64_t n_idx,
                          const double* y, const double* prec, int64_t prec_size, const int64_t* tail_max, double* elpd_out,
                          double* k_out, int64_t* tail_out);
/* PSIS-LOO expectations per selected column of the same store: every DRAW gets its own smoothed importance weight, and weighted
 * sums of a second per-draw quantity f are taken with them -- the leave-one-out predictive mean and variance, the LOO-PIT of
 * az.loo_pit, the normalised smoothed log weights of az.psislw.  store, idx, n_idx, y, prec, prec_size and tail_max as
 * omc_store_psis: with y == NULL the entry holds ll, else it is a mean entry and ll comes from the same inline function (the two
 * routes are bit-equal); the index and tail_max are checked on the device before anything is written.
 *   f_kind  the quantity f_s of draw s at selection position k:
 *     0 ENTRY  element vidx[k] (k itself with vidx == NULL, then n_idx == vsize) of values [n_iter][C][vsize] (device); vidx is
 *              checked like idx.
 *     1 MEAN   the mean entry's own element x.  Needs y.
 *     2 CDF    0.5 erfc(-z 2^-1/2), z = sqrt(tau) (y[k] - x) (one rounded product of one IEEE subtraction; 2^-1/2 rounded to fp64):
 *              the Normal predictive distribution function at the observation.  Needs y.
 *   thr (device) [n_idx]: required exactly when below_out is given.
 * Per column, every ll_s finite: steps 1 - 5 of omc_store_psis give vmax = max_s(-ll_s), xc, T, k, sigma and the smoothed sorted
 * values x'_(p).  Draw s has v = -ll_s and x = v - vmax.
 *   x <= xc, or nothing was smoothed (T <= 4, or k not finite):  w_s = exp(min(x, 0)).
 *   Else, with lo the number of sorted keys < key(v) and hi the number <= key(v):  w_s = (sum_{p = lo}^{hi - 1} exp(x'_(p))) / (hi - lo),
 *     the sum in ascending p.  Tied tail draws share the weight of their positions evenly, a draw that is not tied takes exactly
 *     exp(x'_(lo)); the rule does not depend on the order of the draws in the store.
 *   W = sum_s w_s                                 (a draw of weight 0 adds nothing to any sum)
 *   mean_out    [n_idx]  sum w f / W
 *   var_out     [n_idx]  sum w (f - mean)^2 / W: the weighted population variance, by West's weighted update per lane
 *                        (mean += (f - mean) w / W_new, m2 += w (f - mean_old) (f - mean_new)) and Chan's join with weights for counts,
 *                        never as sum w f^2 - mean^2
 *   below_out   [n_idx]  sum w [f <= thr[k]] / W   (a NaN f counts as not below)
 *   ess_out     [n_idx]  W^2 / sum w^2
 *   invprec_out [n_idx]  sum (w / tau) / W.  Needs y.
 *   k_out [n_idx], tail_out [n_idx] int64: as omc_store_psis, bit-equal to it.
 *   lw_out [n_iter][C][n_idx], the store's layout: log(w_s) - L, L = logsumexp_p(x'_(p)) as the fit forms it (omc_store_psis step 6);
 *     log(w_s) is the exponent itself where w_s is a single exponential, the logarithm of the mean for tied tail draws.
 *   Any output may be NULL, not all; an accumulator nobody asked for is not updated.  A column with an ll that is not finite gives
 *   NaN in every fp64 output, -1 in tail_out and NaN down its lw_out column; no other column is affected.  An f that is not finite
 *   gives whatever IEEE gives in mean and var and leaves ess, k and tail alone.
 *   OMC_INVALID_ARG, with a text in omc_last_error and nothing written: ctx, store or tail_max NULL, S < 2, size < 1, n_idx < 1 (or
 *     no index and n_idx != size), y and prec not given together, prec_size not 1 or n_idx (with y), an index or a tail_max out of
 *     range, S beyond the fit's candidate slots (as omc_store_psis); f_kind outside 0 .. 2; ENTRY without values, with vsize < 1, or
 *     without vidx and n_idx != vsize; MEAN, CDF or invprec_out without y; below_out and thr not given together; a vidx outside
 *     [0, vsize); every output NULL.
 * How: a chunk of columns at a time -- gather, sort and fit as omc_store_psis (the fit is the same inline function; its record per
 * column goes to the workspace), then one pass laid out like omc_store_loglik: a workgroup owns 32 adjacent selection positions
 * and a slice of the rows (about 2048 workgroups over the whole selection, no slice shorter than 256 rows, at most 1024 slices:
 * a function of (S, n_idx) alone, not of the chunk), lanes along the row -- 16-byte loads without an index where the sizes are even
 * and the entries 16-byte aligned, else 8-byte loads --, 16 row lanes down it.  ll is made on load by the gather's own function, so
 * a tail draw finds its key in the sorted column bit for bit; only tail draws bisect (at most tail_max of the S draws of a column).
 * Lanes and slices are joined in a fixed order.  No atomics beyond the gather tile's flag OR; every sum is taken in an order
 * that depends on the shape and on (S, T) alone: repeated calls are bit-equal, and "rank_tile", "rank_chunk" and both load forms
 * give the same bits.  No scratch.  Workspace (rank_ws): per column of a chunk 8 P bytes of keys (P = S rounded up to a power of
 * two), 64 bytes of fit record, 48 bytes per slice and a flag word.  The host reads three words back (the validation).  Runs on
 * the context's stream.                                                                                                        */
omc_status omc_store_loo_expect(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx, int64_t n_idx,
                                const double* y, const double* prec, int64_t prec_size, const int64_t* tail_max, int32_t f_kind,
                                const double* values, int64_t vsize, const int64_t* vidx, const double* thr, double* mean_out,
                                double* var_out, double* below_out, double* ess_out, double* invprec_out, double* k_out,
                                int64_t* tail_out, double* lw_out);
/* Thinned copy of the store for a thinned gather: out[j] = store[first + j * every] (slabs of C * size doubles),
 * j = 0 .. ceil((n_iter - first) / every) - 1 (that count is left in *n_out when n_out is not NULL, host).           */
omc_status omc_store_thin(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, int64_t first, int64_t every,
                          double* out, int64_t* n_out);

/* ---- the one collective of the path: gather of the per-rank stores on a root (RCCL over xGMI) ----
 * Nothing in the reference to replace (it has one chain and no collective; SURVEY section 2.2 COLL row, section 8b
 * export list, section 8e): with the chains of MCMC.run_mcmc (mcmc.py:97-115) sharded over GPUs, this is what puts
 * MCMC.store back together.  One process per GPU; the communicator is RCCL's, bootstrapped from a unique id that the
 * caller ships to every rank by whatever channel it has (the Python mirror uses torch.distributed's object
 * broadcast; a non-Python caller its own).
 *   omc_comm_unique_id     [host] on ONE rank: fills id_out (omc_comm_unique_id_bytes() bytes, 128);
 *   omc_comm_create        on every rank, collectively: ncclCommInitRank on ctx's device;
 *   omc_gather_samples     on every rank, collectively, on ctx's stream (returns without synchronising):
 *       send   [n_outer][counts[rank]][row]  this rank's block (device), chains in local order
 *       recv   [n_outer][sum counts][row]    on `root` (device; ignored elsewhere): chains in rank order
 *       counts [world]                       (host) chains held by every rank; shards may be uneven, also 0
 *     All peers send at once, point to point into the root (xGMI gives every peer its own link); the root stages at
 *     most staging_limit_bytes (0 = 1 GiB) per round and interleaves on the device.                              */
typedef struct omc_comm omc_comm;
int64_t omc_comm_unique_id_bytes(void);
omc_status omc_comm_unique_id(char* id_out, int64_t id_bytes);
omc_status omc_comm_create(omc_ctx* ctx, int32_t world, int32_t rank, const char* id, int64_t id_bytes, omc_comm** out);
omc_status omc_comm_destroy(omc_comm* comm);
omc_status omc_gather_samples(omc_ctx* ctx, omc_comm* comm, const double* send, int64_t n_outer, int64_t row,
                              const int64_t* counts, double* recv, int32_t root, int64_t staging_limit_bytes);
/* The same gather with the peers' blocks already on this GPU: sends[r] = device pointer of rank r's [n_outer][counts[r]][row]
 * block (r = 0..world-1; sends[root] is the root's own block), no communicator.  It runs the root's side of
 * omc_gather_samples unchanged -- slab loop under the staging budget, staging offsets, direct placement for n_outer == 1,
 * the interleave kernel -- with a device-to-device copy standing where ncclRecv stands: what a process that keeps several
 * contexts (shards) on one GPU uses to join their stores, and what tests the root-side arithmetic without peers
 * (tests/test_gather_gpu.py: world 2, 3, 8, even and uneven counts, several staging limits).                          */
omc_status omc_gather_samples_local(omc_ctx* ctx, int32_t world, const double* const* sends, int64_t n_outer, int64_t row,
                                    const int64_t* counts, double* recv, int32_t root, int64_t staging_limit_bytes);

/* ---- raw random streams (tests, prior draws for missing state: mcmc.py:78-80) -------------- */
omc_status omc_fill_normal(omc_ctx* ctx, int64_t n, uint64_t draw_index, double* out, int64_t ld);
omc_status omc_fill_philox_u32(omc_ctx* ctx, int64_t n_words, uint64_t draw_index, uint32_t* out,
                               int64_t ld); /* raw words: INT path, bit-exact vs the host model */

#ifdef __cplusplus
}
#endif
#endif /* OMCMC_HIP_H */
