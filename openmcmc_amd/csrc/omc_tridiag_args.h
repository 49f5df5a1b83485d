// Kernel arguments of the tridiagonal kernels (omc_tridiag.hip): the terms, the Normal-Gamma blocks, the per-sweep records of
// a multi-sweep launch, TriArgs itself, and the accessors that pick a sweep's stream, store and log-posterior out of them.
#pragma once
#include "omc_common.h"

struct TermsDev {
  int n_terms;
  const double* diag[OMC_MAX_TERMS];
  const double* off[OMC_MAX_TERMS];
  const double* rhs[OMC_MAX_TERMS];
  const double* center[OMC_MAX_TERMS];
  const double* scale[OMC_MAX_TERMS];
};
// per-chain part of the terms' centres [C][ld] (omc_tridiag_terms::center_chain).  Its own struct, at the END of the kernel
// arguments: the structure-specialised instantiation never reads it, and with the fields inside TermsDev the shifted
// argument offsets alone cost that instantiation 1 us per sweep (same-box A/B).
struct CentreChain {
  const double* v;  // the chains' vectors [C][ld], or NULL
  int64_t ld;
  int quad_skip;    // bit k: term k's fused quadratic form is not wanted (generic instantiation; option "tridiag_quad_skip")
  int k;            // the term it belongs to (ONE term per launch: with the code unrolled over all four terms the generic
                    // instantiation spilled 100 bytes per lane)
};

struct GammaDev {
  int enabled;
  double a0, b0, half_npos;
  double lnorm;  // a0*log(b0) - lgamma(a0), host-computed
  const double* g_inject;
  double* store;
  double* scale_out;  // writable alias of T.scale[k]
  const double* logdet_unscaled;
  omc_rng_key key;
};

// omc_gmrf_run: several sweeps of the same chains in ONE launch (blockIdx = sweep * C + chain).  What differs from
// sweep to sweep is small and wave-uniform; it sits in the kernel arguments, indexed by the sweep.
#define OMC_RUN_MAX 32
struct SweepRec {
  uint64_t draw;      // draw index of the sweep's standard-normal stream; the Gamma streams are draw + gdraw[k]
  double* x;          // where the draw goes: the sweep's store slab, or the scratch slab
  double* log_post;   // or NULL
  int64_t slot_off;   // offset (in doubles) of the sweep's slot in the per-chain scalar stores; < 0: not stored
};
// hand-over of a chain's freshly drawn scales from the workgroup of sweep s to the one of sweep s+1, which may sit on
// another XCD: data-tagged 8-byte granules {32 bits of the double, 32-bit tag}, written and read with agent-scope
// (sc1) accesses -- no flag, no fence, no ordering between granules needed (MI355X_MICROARCH.md, hand-off forms).
// One 128-byte line per chain: [term k][half] at word 2 k + half.
#define OMC_HANDOFF_WORDS 16

struct TriArgs {
  TermsDev T;
  int64_t n, C, chain_offset;
  const double* rhs_chain; int64_t ld_rhs;
  const double* z; int64_t ld_z;
  int zero_z;
  omc_rng_key key;
  double* x; int64_t ld_x;
  double* quad;
  double* logdet;
  long long* bad;
  double perturb_start;           // tests only: relative error put on every segment's Moebius start value
  int newton_max;                 // Newton corrections of the segment joins before the sequential fallback takes over
  unsigned long long* fallbacks;  // diagnostic counter: chains whose pivot joins went through the sequential fallback
  double* work;
  // fused sweep (omc_gmrf_sweep)
  unsigned long long* stamps;  // diagnostic: [chain][wave][16] s_memtime at phase boundaries, or NULL
  int fused;
  GammaDev gb[OMC_MAX_TERMS];
  // generic workgroup-per-chain instantiation: the same blocks and streams in device memory, where wave 0's lanes index them
  // by their term (indexing the ARGUMENT copy per lane makes the compiler keep a private image of all blocks: 360 bytes of
  // scratch per lane stored by every wave at entry, 160 instead of 107 us per sweep)
  const GammaDev* gb_dev;
  const unsigned long long* gdraw_dev;
  double* log_post;
  // several sweeps per launch (n_sweeps > 0; workgroup-per-chain form only)
  int n_sweeps;
  int reenter;                     // 1, 2: a workgroup restarts itself as its chain's next sweep
  int block_sweeps;                // ... for this many sweeps in a row; then a fresh workgroup (block index + C) takes the chain
                                   // over through the global hand-over line.  n_sweeps: one workgroup per chain for the launch
  int early_draws;                 // 1: all buffered pairs of draws are made before the scales are waited for (see the kernel)
  uint32_t epoch;                  // tag of sweep 0's inputs + 1 = tag its outputs carry; unique per context over launches
  uint64_t seed;
  uint64_t gdraw[OMC_MAX_TERMS];   // Gamma stream of term k = sweep's draw index + gdraw[k]
  unsigned long long* handoff;     // [C][OMC_HANDOFF_WORDS]
  unsigned long long* timeouts;    // counter: hand-overs that did not arrive (dispatch-order assumption broken)
  // diagnostic sweep clock: wave 0 of a (sweep, chain) workgroup leaves {s_memrealtime at entry, at exit} in record
  // (sweep_times_pos + sweep) mod sweep_times_cap of the ring [cap][C][2]; NULL = off
  unsigned long long* sweep_times;
  int64_t sweep_times_cap, sweep_times_pos;
  SweepRec rec[OMC_RUN_MAX];
  CentreChain cc;
};

__device__ __forceinline__ bool run_mode(const TriArgs& A) { return A.n_sweeps > 0; }
__device__ __forceinline__ omc_rng_key sweep_gamma_key(const TriArgs& A, int sw, const GammaDev& g, uint64_t gd) {
  return run_mode(A) ? omc_make_key(A.seed, A.rec[sw].draw + gd, OMC_RNG_GAMMA) : g.key;
}
__device__ __forceinline__ double* sweep_gamma_store(const TriArgs& A, int sw, const GammaDev& g) {
  if (!run_mode(A)) return g.store;
  const int64_t off = A.rec[sw].slot_off;
  return (g.store && off >= 0) ? g.store + off : nullptr;
}
__device__ __forceinline__ double* sweep_log_post(const TriArgs& A, int sw) { return run_mode(A) ? A.rec[sw].log_post : A.log_post; }
