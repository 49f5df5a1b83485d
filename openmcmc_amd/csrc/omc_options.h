// The options of omc_ctx_set_option: one row per name.  Host code without a HIP call, so that a stand-alone program can hold the
// table to its documented behaviour without a device (tests/native/options_host.hip).  What every option means stands in
// include/omcmc_hip.h, its default at the member in omc_common.h.
#pragma once
#include <string.h>

#include "omc_common.h"

// A value in [lo, hi] that also passes `rule` is stored in the int member `i` (as value != 0 for a flag) or the int64 member `l`;
// `hook` then does what a plain store cannot: it stores a pointer or an event, or resets what depends on the option.  Its status
// is the option's.
struct omc_option {
  const char* name;
  int omc_ctx::*i;
  int64_t omc_ctx::*l;
  int64_t lo, hi;
  bool (*rule)(int64_t);
  bool flag;
  omc_status (*hook)(omc_ctx*, int64_t);
};

#define OMC_ANY INT64_MIN, INT64_MAX
#define OMC_OPT_INT(name, lo, hi) {#name, &omc_ctx::name, nullptr, lo, hi, nullptr, false, nullptr}
#define OMC_OPT_SET(name, lo, hi, ...) {#name, &omc_ctx::name, nullptr, lo, hi, [](int64_t v) { return __VA_ARGS__; }, false, nullptr}
#define OMC_OPT_FLAG(name) {#name, &omc_ctx::name, nullptr, OMC_ANY, nullptr, true, nullptr}
#define OMC_OPT_I64(name, lo, hi) {#name, nullptr, &omc_ctx::name, lo, hi, nullptr, false, nullptr}
#define OMC_OPT_HOOK(name, ...) {name, nullptr, nullptr, OMC_ANY, nullptr, false, [](omc_ctx* ctx, int64_t v) -> omc_status { __VA_ARGS__; return OMC_OK; }}

static const omc_option omc_options[] = {
    OMC_OPT_INT(tridiag_algo, 0, 2),
    OMC_OPT_SET(tridiag_seg, 0, 32, v == 0 || v == 8 || v == 10 || v == 16 || v == 20 || v == 32),
    OMC_OPT_INT(run_sweeps_per_launch, 1, 32),
    OMC_OPT_INT(run_block_sweeps, 0, 32),
    // an explicit choice holds for every chain count (tests, A/B runs)
    {"run_reenter", &omc_ctx::run_reenter, nullptr, 0, 2, nullptr, false, [](omc_ctx* ctx, int64_t) { ctx->run_reenter_force = 1; return OMC_OK; }},
    OMC_OPT_INT(tridiag_quad_skip, 0, 15),
    OMC_OPT_INT(tridiag_perturb_ppb, 0, 1000000000),
    OMC_OPT_INT(tridiag_newton_max, 0, 64),
    OMC_OPT_FLAG(tridiag_generic),
    OMC_OPT_INT(band_algo, 0, 3),
    OMC_OPT_INT(diag_algo, 0, 2),
    OMC_OPT_INT(hist_algo, 0, 1),
    OMC_OPT_INT(reduce_algo, 0, 2),
    OMC_OPT_INT(hist2d_algo, 0, 3),
    OMC_OPT_SET(rank_tile, 0, 8192, v == 0 || (v >= 64 && !(v & (v - 1)))),
    OMC_OPT_I64(rank_chunk, 0, INT64_MAX),
    OMC_OPT_I64(autocorr_slice, 0, INT64_MAX),
    OMC_OPT_INT(band_seg_overlap, 8, 65536),
    OMC_OPT_SET(band_seg_count, 0, 128, v != 1),
    OMC_OPT_SET(band_blocked_threads, 0, 512, v == 0 || v == 4 || v == 8 || v == 16 || v == 512),
    OMC_OPT_SET(mh_gemm_ksplit, 1, 4, v != 3),
    OMC_OPT_FLAG(mh_use_rocblas),
    OMC_OPT_FLAG(gram_use_rocblas),
    OMC_OPT_FLAG(spectral_use_rocblas),
    OMC_OPT_FLAG(dense_use_rocsolver),
    OMC_OPT_INT(debug_zero_z, INT64_MIN, INT64_MAX),
    OMC_OPT_INT(dense_blocked_min, 1, 32768),
    OMC_OPT_INT(dense_panel_old, 0, 1),
    OMC_OPT_INT(dense_overlap, 0, 1),
    // diagnostic: device ring [cap][n_chains][2] of uint64, 0 = off (set the capacity first)
    OMC_OPT_HOOK("sweep_times_ptr",
                 if (v != 0 && ctx->sweep_times_cap < OMC_SWEEP_RING_MIN) return OMC_INVALID_ARG;
                 ctx->sweep_times = (unsigned long long*)(uintptr_t)v;
                 ctx->sweep_times_pos = 0),
    // a ring set earlier was sized for the OLD capacity: the clock stays off until a pointer is given for the new one
    // (a larger capacity on the old pointer would have omc_gmrf_run write records past the ring's end)
    OMC_OPT_HOOK("sweep_times_cap",
                 if (v != 0 && v < OMC_SWEEP_RING_MIN) return OMC_INVALID_ARG;
                 if (v != ctx->sweep_times_cap) ctx->sweep_times = nullptr;
                 ctx->sweep_times_cap = v;
                 ctx->sweep_times_pos = 0),
    // a caller-owned hipEvent_t (0 = none): omc_gmrf_run records it on the context's stream in front of its first / behind its
    // last launch -- the timing events of a caller whose own event calls cost more than the launch (an interpreter)
    OMC_OPT_HOOK("run_event_begin", ctx->run_ev_begin = (hipEvent_t)(uintptr_t)v),
    OMC_OPT_HOOK("run_event_end", ctx->run_ev_end = (hipEvent_t)(uintptr_t)v),
    // diagnostic: device buffer [n_chains][16][16] of uint64, 0 = off
    OMC_OPT_HOOK("stamps_ptr", ctx->stamps = (unsigned long long*)(uintptr_t)v),
};

// OMC_INVALID_ARG, and nothing changed, for a name that is not in the table or a value that its row does not accept
inline omc_status omc_option_apply(omc_ctx* ctx, const char* name, int64_t value) {
  for (const omc_option& o : omc_options) {
    if (strcmp(name, o.name)) continue;
    if (value < o.lo || value > o.hi || (o.rule && !o.rule(value))) return OMC_INVALID_ARG;
    if (o.i) ctx->*o.i = o.flag ? (value != 0) : (int)value;
    if (o.l) ctx->*o.l = value;
    return o.hook ? o.hook(ctx, value) : OMC_OK;
  }
  return OMC_INVALID_ARG;
}
