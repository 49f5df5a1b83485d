// Context: creation and release, its BLAS handles and side stream, status latch, counters, options (the table: omc_options.h).
#include <string.h>

#include <string>

#include "omc_blas.h"
#include "omc_options.h"

static thread_local std::string g_last_error;

void omc_set_error(const char* what, hipError_t e) {
  g_last_error = std::string(what) + ": " + hipGetErrorString(e);
}

void omc_set_error_text(const char* text) { g_last_error = text; }
omc_status omc_invalid(const char* text) {
  omc_set_error_text(text);
  return OMC_INVALID_ARG;
}

omc_status omc_ensure_blas(omc_ctx* ctx) {
  if (!ctx->blas) {
    rocblas_handle h;
    OMC_BLAS_CHECK(rocblas_create_handle(&h));
    OMC_BLAS_CHECK(rocblas_set_stream(h, ctx->stream));
    OMC_BLAS_CHECK(rocblas_set_pointer_mode(h, rocblas_pointer_mode_host));
    ctx->blas = (void*)h;
  }
  return OMC_OK;
}

// side stream, its BLAS handle and the fork / join events of the blocked factorisation (made on first use)
omc_status omc_ensure_aux(omc_ctx* ctx) {
  if (ctx->blas_aux) return OMC_OK;
  OMC_HIP_CHECK(hipStreamCreateWithFlags(&ctx->aux_stream, hipStreamNonBlocking));
  OMC_HIP_CHECK(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
  OMC_HIP_CHECK(hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
  rocblas_handle h;
  OMC_BLAS_CHECK(rocblas_create_handle(&h));
  OMC_BLAS_CHECK(rocblas_set_stream(h, ctx->aux_stream));
  OMC_BLAS_CHECK(rocblas_set_pointer_mode(h, rocblas_pointer_mode_host));
  ctx->blas_aux = (void*)h;
  return OMC_OK;
}

void omc_ctx_release_blas(omc_ctx* ctx) {
  if (ctx->blas) rocblas_destroy_handle((rocblas_handle)ctx->blas);
  ctx->blas = nullptr;
  if (ctx->blas_aux) {
    rocblas_destroy_handle((rocblas_handle)ctx->blas_aux);
    hipEventDestroy(ctx->ev_fork);
    hipEventDestroy(ctx->ev_join);
    hipStreamDestroy(ctx->aux_stream);
    for (int i = 0; i < 4; ++i)  // omc_mala_run_white made them behind omc_ensure_aux
      if (ctx->white.ev[i]) { hipEventDestroy(ctx->white.ev[i]); ctx->white.ev[i] = nullptr; }
    ctx->blas_aux = nullptr;
  }
}

extern "C" {

const char* omc_last_error(void) { return g_last_error.c_str(); }

int32_t omc_abi_version(void) { return 2; }

omc_status omc_ctx_create(int32_t device, int64_t n_chains, uint64_t seed, int64_t chain_id_offset,
                          void* stream, int32_t create_stream, omc_ctx** out) {
  if (!out || n_chains <= 0 || chain_id_offset < 0) return OMC_INVALID_ARG;
  *out = nullptr;
  int count = 0;
  OMC_HIP_CHECK(hipGetDeviceCount(&count));
  if (device < 0 || device >= count) return OMC_INVALID_ARG;
  OMC_HIP_CHECK(hipSetDevice(device));
  omc_ctx* c = new omc_ctx();  // every default: omc_common.h
  c->device = device;
  if (hipDeviceGetAttribute(&c->dev_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || c->dev_cus <= 0) c->dev_cus = 256;
  c->n_chains = n_chains;
  c->seed = seed;
  c->chain_offset = chain_id_offset;
  c->own_stream = (create_stream != 0);
  c->stream = (hipStream_t)stream;
  const long long init[8] = {OMC_NO_BAD_CHAIN, 0, 0, 0, 0, 0, 0, 0};  // the status words
  const char* what = "hipStreamCreate";
  hipError_t e = c->own_stream ? hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) : hipSuccess;
  if (e != hipSuccess) c->own_stream = false;  // nothing to destroy
  if (e == hipSuccess) { what = "hipMalloc"; e = hipMalloc(&c->status_words.p, sizeof(init)); }
  if (e == hipSuccess) { what = "hipMemcpy"; e = hipMemcpy(c->status_words, init, sizeof(init), hipMemcpyHostToDevice); }
  if (e != hipSuccess) {
    omc_set_error(what, e);
    if (c->own_stream) hipStreamDestroy(c->stream);
    delete c;  // frees the status words
    return OMC_HIP_ERROR;
  }
  c->d_bad_chain = c->status_words;
  c->d_fallbacks = (unsigned long long*)(c->d_bad_chain + 1);
  *out = c;
  return OMC_OK;
}

omc_status omc_ctx_destroy(omc_ctx* ctx) {
  if (!ctx) return OMC_INVALID_ARG;
  hipSetDevice(ctx->device);
  hipStreamSynchronize(ctx->stream);
  omc_ctx_release_blas(ctx);
  const hipStream_t owned = ctx->own_stream ? ctx->stream : nullptr;
  delete ctx;  // every omc_buf of the context frees itself
  if (owned) hipStreamDestroy(owned);
  return OMC_OK;
}

omc_status omc_ctx_synchronize(omc_ctx* ctx) {
  if (!ctx) return OMC_INVALID_ARG;
  OMC_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return OMC_OK;
}

omc_status omc_ctx_status(omc_ctx* ctx, int64_t* first_bad_chain) {
  if (!ctx || !first_bad_chain) return OMC_INVALID_ARG;
  long long w[3] = {OMC_NO_BAD_CHAIN, 0, 0};
  OMC_HIP_CHECK(hipMemcpyAsync(w, ctx->d_bad_chain, sizeof(w), hipMemcpyDeviceToHost, ctx->stream));
  OMC_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  const long long v = w[0];
  if (w[2] != 0) {  // a several-sweeps launch whose hand-over never arrived: the results of that run are not to be used
    long long zero = 0;
    OMC_HIP_CHECK(hipMemcpyAsync(ctx->d_bad_chain + 2, &zero, sizeof(zero), hipMemcpyHostToDevice, ctx->stream));
    OMC_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    omc_set_error_text("omc_gmrf_run: a sweep's hand-over to the next sweep of its chain did not arrive (set run_sweeps_per_launch = 1)");
    *first_bad_chain = -1;
    return OMC_HIP_ERROR;
  }
  if (v == OMC_NO_BAD_CHAIN) {
    *first_bad_chain = -1;
    return OMC_OK;
  }
  *first_bad_chain = (int64_t)v;
  long long init = OMC_NO_BAD_CHAIN;
  OMC_HIP_CHECK(hipMemcpyAsync(ctx->d_bad_chain, &init, sizeof(init), hipMemcpyHostToDevice, ctx->stream));
  OMC_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return OMC_NOT_POSDEF;
}

omc_status omc_ctx_counter(omc_ctx* ctx, const char* name, int64_t* value) {
  if (!ctx || !name || !value) return OMC_INVALID_ARG;
  static const struct { const char* name; int word; } device_counters[] = {  // words behind d_fallbacks (omc_common.h)
      {"tridiag_join_fallbacks", 0}, {"run_handoff_timeouts", 1}, {"band_join_fallbacks", 2}, {"band_join_retries", 3}};
  for (const auto& dc : device_counters) {
    if (strcmp(name, dc.name)) continue;
    unsigned long long v = 0;
    OMC_HIP_CHECK(hipMemcpyAsync(&v, ctx->d_fallbacks + dc.word, sizeof(v), hipMemcpyDeviceToHost, ctx->stream));
    OMC_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    *value = (int64_t)v;
    return OMC_OK;
  }
  if (!strcmp(name, "wall_clock_khz")) {  // rate of the s_memrealtime counter the sweep clock records (not a counter; no sync)
    int khz = 0;
    OMC_HIP_CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device));
    *value = khz;
    return OMC_OK;
  }
  if (!strcmp(name, "reenter_abi_ok")) {  // probes the loaded kernel descriptors on first use (synchronises then)
    OMC_HIP_CHECK(hipSetDevice(ctx->device));
    *value = omc_reentry_probe_result(ctx);
    return OMC_OK;
  }
  if (!strcmp(name, "sweep_times_pos")) {  // ring index the next sweep of omc_gmrf_run will write (no sync)
    *value = ctx->sweep_times_pos;
    return OMC_OK;
  }
  return OMC_INVALID_ARG;
}

omc_status omc_ctx_launch_log(omc_ctx* ctx, double* out, int64_t cap, int64_t* n_launches) {
  if (!ctx || !n_launches || cap < 0 || (cap > 0 && !out)) return OMC_INVALID_ARG;
  *n_launches = ctx->launch_log_total;
  const int64_t m = ctx->launch_log_n < cap ? ctx->launch_log_n : cap;
  for (int64_t i = 0; i < m; ++i) {
    const omc_ctx::LaunchRec& r = ctx->launch_log[i];
    out[5 * i] = r.t_begin; out[5 * i + 1] = r.t_end; out[5 * i + 2] = (double)r.n_sweeps; out[5 * i + 3] = (double)r.form;
    out[5 * i + 4] = (double)r.ring_pos;
  }
  return OMC_OK;
}

omc_status omc_ctx_set_option(omc_ctx* ctx, const char* name, int64_t value) {
  if (!ctx || !name) return OMC_INVALID_ARG;
  return omc_option_apply(ctx, name, value);  // the table: omc_options.h
}

}  // extern "C"
