// Host build of the option table (openmcmc_amd/csrc/omc_options.h) on a default-constructed context, for the CPU test suite: no
// device, no HIP call.
//   hipcc -x hip --cuda-host-only -O2 -I include -I openmcmc_amd/csrc tests/native/options_host.hip -o <exe>
// stdin: one probe per line, `name value` (applied with omc_option_apply) or `!pos value` (puts the sweep clock's position there
// directly, as a run would: the options can only reset it).
// stdout, one record per line:
//   N name...             the names of the table, in its order
//   R name...             the members read below, in the order of every later record: one per option (read through the list in this
//                         file, not through the table), then run_reenter_force, sweep_times_pos, dev_cus, run_epoch
//   D value...            their values in the default-constructed context
//   P status value...     per probe: the status and the values afterwards
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "omc_options.h"

#define MEMBERS(X)                                                                                                                    \
  X(tridiag_algo) X(tridiag_seg) X(run_sweeps_per_launch) X(run_block_sweeps) X(run_reenter) X(tridiag_quad_skip)                     \
  X(tridiag_perturb_ppb) X(tridiag_newton_max) X(tridiag_generic) X(band_algo) X(diag_algo) X(hist_algo) X(reduce_algo)               \
  X(hist2d_algo) X(rank_tile) X(rank_chunk) X(autocorr_slice) X(band_seg_overlap) X(band_seg_count) X(band_blocked_threads)           \
  X(mh_gemm_ksplit) X(mh_use_rocblas) X(gram_use_rocblas) X(spectral_use_rocblas) X(dense_use_rocsolver) X(debug_zero_z)              \
  X(dense_blocked_min) X(dense_panel_old) X(dense_overlap) X(sweep_times_cap)
// options whose name is not their member's
#define RENAMED(X) X("sweep_times_ptr", sweep_times) X("run_event_begin", run_ev_begin) X("run_event_end", run_ev_end) X("stamps_ptr", stamps)
#define EXTRAS(X) X(run_reenter_force) X(sweep_times_pos) X(dev_cus) X(run_epoch)

static void names() {
  printf("R");
#define NAME(m) printf(" %s", #m);
#define NAME2(n, m) printf(" %s", n);
  MEMBERS(NAME) RENAMED(NAME2) EXTRAS(NAME)
  printf("\n");
}
static void values(const omc_ctx& c) {
#define VAL(m) printf(" %" PRId64, (int64_t)c.m);
#define VAL2(n, m) printf(" %" PRId64, (int64_t)(uintptr_t)c.m);
  MEMBERS(VAL) RENAMED(VAL2) EXTRAS(VAL)
  printf("\n");
}
static bool is_read(const char* name) {
#define HIT(m) if (!strcmp(name, #m)) return true;
#define HIT2(n, m) if (!strcmp(name, n)) return true;
  MEMBERS(HIT) RENAMED(HIT2)
  return false;
}

int main() {
  omc_ctx ctx;
  printf("N");
  for (const omc_option& o : omc_options) {
    if (!is_read(o.name)) { fprintf(stderr, "option %s of the table is not read by this program\n", o.name); return 2; }
    printf(" %s", o.name);
  }
  printf("\n");
  names();
  printf("D");
  values(ctx);
  char name[128];
  long long v;
  while (scanf("%127s %lld", name, &v) == 2) {
    int st = 0;
    if (!strcmp(name, "!pos")) ctx.sweep_times_pos = v;
    else st = (int)omc_option_apply(&ctx, name, (int64_t)v);
    printf("P %d", st);
    values(ctx);
  }
  return 0;
}
