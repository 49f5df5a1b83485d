// k_tridiag_seg, the segmented kernel of omc_tridiag.hip, with its compile-time switches, the phase stamps (OMC_STAMP) and
// the restart of a workgroup as its chain's next sweep (OMC_REENTER; OMC_KD_WORDS reads the descriptors that relies on).
#pragma once
#include "omc_tridiag_epilogue.h"
#include "omc_tridiag_scan.h"
#include "omc_tridiag_tile.h"

// Compile-time switches of k_tridiag_seg.  All of them are diagnostic or measuring builds: the default values are the
// product, and none is an open experiment (the forms that were tried and lost are recorded in docs/DESIGN_HISTORY.md).
//
// "Without one LDS transfer" variants: each turns off one use of the LDS-DMA path, so that a result that depends on a
// transfer's timing shows up as a difference between builds (profiles/r03h_determinism.txt found round 3's race this way).
#ifndef OMC_PARK_OFF
#define OMC_PARK_OFF 1  // specialised forms: the off-diagonal slice for the quadratic forms is parked in the draws' LDS slots
#endif
#ifndef OMC_PARK_DIAG
#define OMC_PARK_DIAG 1  // specialised forms: the tridiagonal term's diagonal slice is parked in the tile behind the forward pass
#endif
#ifndef OMC_SHIFT_PARK_C
#define OMC_SHIFT_PARK_C 1  // SIG 3: the draws' LDS slots take the chain's centre slice (HBM) instead of the off-diagonal slice (L2)
#endif
#ifndef OMC_PREFETCH_QUAD
#define OMC_PREFETCH_QUAD 1  // specialised forms: the quadratic forms' centre vector is prefetched under the reverse scan (0: loaded in the phase itself)
#endif
// Timing what-ifs (benchmarks/build_variant.sh, benchmarks/ab_headline.py): results are wrong by construction.
#ifndef OMC_WHATIF_NOSTORE
#define OMC_WHATIF_NOSTORE 0  // 1: the full waves' x stores are left out
#endif
#ifndef OMC_WHATIF_NOQLOAD
#define OMC_WHATIF_NOQLOAD 0  // 1: the quadratic forms' centre and off-diagonal loads are replaced by constants
#endif
#ifndef OMC_NO_STAMPS
#define OMC_NO_STAMPS 0  // 1: the phase stamps (OMC_STAMP) are compiled out
#endif


// Structure-specialised form of the workgroup-per-chain kernel (template parameter SIG).
//   SIG 0: any term structure (every pointer tested at run time).
//   SIG 1: the GMRF smoother of examples/4 and BASELINE configs[2]: two terms in either order,
//            term I = scaled identity precision (diag, off absent) with rhs and center,
//            term P = tridiagonal precision (diag, off present) without rhs and center,
//          so  a = sI + sP diagP,  b = sP offP,  r = sI rhsI (+ rhs_chain),
//              qI = |x - centerI|^2,  qP = x' M_P x.
// Knowing the structure at compile time removes the pointer tests and makes the load phases explicit, so
// that work which depends on nothing can be placed in their shadow: with one workgroup per CU all waves are
// in the same phase, and a phase that only waits for L2 (80 KB per vector and workgroup at ~30 B/clk per
// CU, 1.3 us) is otherwise dead time for the vector ALU.  The standard-normal draws are such work (pure
// functions of the Philox counter, 1.45 us per pair and workgroup): all but the last pair of a segment are
// generated while the precision and right-hand-side vectors are in flight and parked in LDS (`lds_z`,
// lane-private slots).  benchmarks/micro/overlap.hip measures the effect in isolation.  (Holding
// prefetched vectors of a later phase in registers instead was tried: at 128 VGPRs it spills, and the spill
// traffic costs more than the overlap gains.)

// sqrt(1/D) that scales a standard-normal draw: one Newton step on v_rsq_f64 (4e-15 relative, measured in
// benchmarks/micro/rcp_acc.hip) -- the draw's own scale, nothing downstream amplifies it
__device__ __forceinline__ double fast_sqrt(double r) {
  const double g = __builtin_amdgcn_rsq(r);
  const double s = r * g;
  return fma(fma(-s, s, r), 0.5 * g, s);
}


// diagnostic phase stamps (guide section 7, in-kernel stamps): lane 0 of every wave, only when enabled
#if OMC_NO_STAMPS
#define OMC_STAMP(k) do { } while (0)
#else
#define OMC_STAMP(k)                                                                                  \
  do {                                                                                                \
    if (A.stamps) {                                                                                   \
      __builtin_amdgcn_sched_barrier(0);                                                              \
      const unsigned long long _t = __builtin_amdgcn_s_memtime();                                     \
      if (lane == 0 && chain_ok) A.stamps[((c * 16) + wave) * 16 + (k)] = _t;                          \
      __builtin_amdgcn_sched_barrier(0);                                                              \
    }                                                                                                 \
  } while (0)
#endif

// join residual (relative) below which the pivots are accepted: ~72 ulp; the Moebius start already
// meets it for well-conditioned chains, weakly coupled ones take one or two Newton corrections
#define OMC_NEWTON_TOL 1.6e-14
#define OMC_NEWTON_MAX 4

// Register plan per lane (M nodes): Y = b -> l ; W = 1/D -> g -> x (draws are consumed as they are made).
// The combined diagonal a (then the right-hand side r) lives in the wave's LDS tile.
template <int M, bool MULTI, int MAXT, int SIG = 0>
__global__ void __launch_bounds__(MAXT) k_tridiag_seg(TriArgs A, int G) {
  static_assert(SIG == 0 || MULTI, "specialised structures exist for the workgroup-per-chain form only");
  // SIG 1, 2: the two-term smoother.  SIG 2 is its WAITING form -- the (sweep, chain) grid with at most half as many chains
  // as CUs, in-kernel draws: the workgroup of a chain's next sweep sits on an idle CU until the previous sweep's scales
  // arrive, so everything that does not depend on them is done up front (all three vector loads, the buffered draws, the
  // Normal-Gamma standard draws), and the poll of the hand-over line is tight.  Never self-restarting.
  // SIG 3 (round 3): the smoother whose tridiagonal term is centred at a PER-CHAIN vector c (a hierarchical model's sampled
  // prior mean, or the sampled field a mean block is conditioned on: omc_tridiag_terms.center_chain on that term).
  // Evaluated by a shift: x = c + e, where e is the plain smoother's draw for the identity term centred at ys - c --
  //   Q e = sP P c + sI ys - Q c = sI (ys - c)   --
  // so the stencil product P c is never formed and all the specialised kernel has to do differently is element-wise: the
  // right-hand side sI (ys - c), the identity term's quadratic form around ys - c (= (x - ys)'(x - ys) of the shifted x), and
  // x = c + e on the way out; the tridiagonal term's quadratic form e'Pe IS (x - c)'P(x - c), with the parking scheme intact.
  // Same conditional law and the same draw for the same z up to rounding (the two right-hand sides are equal in exact
  // arithmetic).  ys may be absent (zeros).
  constexpr bool SMO = SIG != 0;
  constexpr bool EARLY = SIG == 2;
  constexpr bool SHIFT = SIG == 3;
  using TM = TileMap<M>;
  constexpr int NWMAX = MAXT / 64;
  __shared__ double lds_tile[NWMAX][64 * (M + 1) + 2];  // + the successor slot of the last row (quad_wg)
  __shared__ Mob lds_mob[16], lds_mob2[16];
  __shared__ double lds_g[64];     // wave 0's Normal-Gamma standard draws, start of kernel -> epilogue
  __shared__ unsigned long long lds_hand[2 * OMC_MAX_TERMS];  // self-restarting workgroups: the scales from sweep to sweep
  __shared__ double lds_q[OMC_MAX_TERMS];  // ... and the quadratic forms of the sweep whose log-posterior is finished by the next
  __shared__ Aff lds_aff[4][16];   // scans alternate buffers instead of paying a trailing barrier
  __shared__ double lds_x[2][32];  // neighbour exchange of the Newton passes (alternating)
  __shared__ double lds_d[6][16];  // reductions: one slot per call site
  __shared__ int lds_any[16];      // any_wg of the join test
  // SIG 1: pairs of draws per lane made ahead of the forward pass (all but the last; at most 8: LDS)
  // SIG 0, M <= 10 (round 3): the generic instantiation parks the same pairs -- its LDS image leaves 66 KB free -- and makes
  // them under the loads of its three tile fills (`fill_draws`), where the vector ALU used to idle; it generated all of a
  // segment's draws inside the forward pass (10 000 cycles of pure vector-ALU time on the critical path).
  constexpr bool PARKZ = SMO || (MULTI && M <= 10);
  constexpr int NZB = PARKZ ? (M / 2 - 1 > 8 ? 8 : M / 2 - 1) : 0;
  __shared__ double lds_z[PARKZ ? NWMAX : 1][NZB > 0 ? 2 * NZB : 1][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int Wd = MULTI ? 64 : G;
  int64_t c;
  int s;
  Geom<M, MULTI> geo;
  geo.lane = lane; geo.wave = wave; geo.G = G;
  int sw = 0;  // sweep of this workgroup inside the launch (omc_gmrf_run: blockIdx = sweep * C + chain)
  bool restarted = false;  // this workgroup came here by its own restart (its predecessor sweep ran in this very workgroup)
  int left = 0;            // sweeps this workgroup will still restart itself for
  unsigned c_blk = 0;
  if (MULTI) {
    unsigned blk = blockIdx.x;
    // (Several sweeps per launch: the sweep index picks the sweep's record out of the kernel arguments.  Round 2 saw
    // "private copies" of the argument struct appear in the generic instantiation whenever such an index was added and blamed
    // the dynamic index; the cause was LLVM's limit of 300 users in the transform that forwards reads of a by-value kernel
    // argument to the kernel-argument segment -- see the note in the Makefile.  With the limit raised every instantiation
    // takes the sweep index, and none uses scratch.)
    if (A.n_sweeps > 1) {
      // A fresh workgroup: block index = (block of sweeps) * C + chain, and it starts at the block's first sweep.  A restarted
      // one carries what the restart put into the workgroup-id register: bit 31, the sweeps still to follow in its block
      // (bits 30:26) and the virtual index sweep * C + chain (OMC_REENTER at the end of the kernel).
      restarted = (blk >> 31) != 0u;
      const unsigned vblk = restarted ? (blk & 0x03ffffffu) : blk;
      const unsigned q = vblk / (unsigned)A.C;
      c_blk = vblk - q * (unsigned)A.C;
      if (restarted) {
        sw = (int)q;
        left = (int)((blk >> 26) & 31u);
      } else {
        const int g = (A.reenter && A.block_sweeps > 0) ? A.block_sweeps : 1;
        sw = (int)q * g;
        left = (A.n_sweeps - sw < g ? A.n_sweeps - sw : g) - 1;
      }
      blk = c_blk;
    }
    c = blk;
    s = threadIdx.x;
    geo.chain0 = c;
  } else {
    const int cpw = 64 / G;
    geo.chain0 = ((int64_t)blockIdx.x * nw + wave) * cpw;
    c = geo.chain0 + lane / G;
    s = lane % G;
  }
  double* tile = lds_tile[wave];
  const double* trow = tile + (MULTI ? lane : s) * (M + 1);  // shared vectors: every group reads rows 0..G-1
  double* crow = tile + lane * (M + 1);                      // per-chain data: one row per lane
  const int lbase = TileMap<M>::lane_base(lane);             // this lane's element of step 0 (coalesced mapping)
  const int pos = MULTI ? lane : s;
  const bool chain_ok = c < A.C;
  const int64_t cc = chain_ok ? c : 0;
  const int64_t n = A.n;
  const int64_t i0 = (int64_t)s * M;
  const int nt = (SMO) ? 2 : A.T.n_terms;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int r0 = TM::lane_col(lane);
  double* tl = tile + lbase;

  double sc[OMC_MAX_TERMS];
  // Sweeps after the first of a launch take the scales their Normal-Gamma blocks redraw from the hand-over line of
  // the chain (written by the workgroup of the previous sweep, possibly on another XCD); the loads are issued here
  // and examined where the scales are first needed (`take_scales`), behind the first pair of draws.
  const bool handed = MULTI && sw > 0;
  // a self-restarting workgroup takes them from its own LDS (written by its wave 0 a moment ago: a poll there costs a
  // hundred cycles, a poll of the global line a trip to L2)
  const bool hand_lds = SIG == 1 && A.reenter != 0 && restarted;
  // LDS comes as the previous workgroup on this CU left it -- possibly this very kernel under another context, whose
  // tags count from 1 like ours: the launch's first sweep wipes the granules (tag 0 is never waited for) long before
  // its epilogue writes them and the second sweep looks
  if (SIG == 1 && A.reenter != 0 && !restarted && threadIdx.x < 2 * OMC_MAX_TERMS)
    __hip_atomic_store(lds_hand + threadIdx.x, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  unsigned long long hw[2 * OMC_MAX_TERMS];
  // the two hand-over granules of term k: from the chain's hand-over line in memory, from this workgroup's LDS copy
  auto load_hand_global = [&](int k) __attribute__((always_inline)) {
    const unsigned long long* h = A.handoff + cc * OMC_HANDOFF_WORDS + 2 * k;
    hw[2 * k] = __hip_atomic_load(h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    hw[2 * k + 1] = __hip_atomic_load(h + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  auto load_hand_lds = [&](int k) __attribute__((always_inline)) {
    hw[2 * k] = __hip_atomic_load(lds_hand + 2 * k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    hw[2 * k + 1] = __hip_atomic_load(lds_hand + 2 * k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  };
#pragma unroll
  for (int k = 0; k < OMC_MAX_TERMS; ++k) {
    sc[k] = 1.0;
    hw[2 * k] = hw[2 * k + 1] = 0ull;
    if (k < nt && A.T.scale[k]) {
      if (handed && A.gb[k].enabled) {
        // (the LDS granules are read where they are needed: a read there costs nothing worth hiding)
        if (!hand_lds) load_hand_global(k);
      } else {
        sc[k] = A.T.scale[k][cc];
      }
    }
  }
  // is there a scale that travels from sweep to sweep at all (then waiting for it orders everything else its producer
  // wrote to LDS before it)?
  auto any_handed_f = [&]() {  // (recomputed from the kernel arguments where it is asked: nothing to keep live)
    bool any = false;
#pragma unroll
    for (int k = 0; k < OMC_MAX_TERMS; ++k) any |= (k < nt && A.T.scale[k] && A.gb[k].enabled);
    return any;
  };
  auto take_scales = [&]() {
    if (!handed) return;
    bool lost = false;  // the hand-over never came (reported through `timeouts`): this sweep runs on NaN scales, so that
                        // whatever it stores is recognisably not a sample
    const uint32_t want = A.epoch + (uint32_t)sw;
    auto tags_ok = [&]() {
      bool ok = true;
#pragma unroll
      for (int k = 0; k < OMC_MAX_TERMS; ++k)
        if (k < nt && A.T.scale[k] && A.gb[k].enabled)
          ok = ok && (uint32_t)(hw[2 * k] >> 32) == want && (uint32_t)(hw[2 * k + 1] >> 32) == want;
      return __builtin_amdgcn_readfirstlane((int)ok) != 0;  // every lane loaded the same words
    };
    if (EARLY && wave_u != 0) {
      // SIG 2: wave 0 alone polls the chain's hand-over line in memory; the other waves wait at a BARRIER (no polling
      // traffic of their own, released together the moment wave 0 arrives) and then read what wave 0 left in LDS.
      // Sixteen waves polling back to back got in each other's way: the per-wave timeline showed the last wave seeing
      // the scales 4 000 cycles after the first, and the first scan waits for the last wave.  The LDS words were wiped
      // at the workgroup's start (behind a barrier): LDS arrives as the CU's previous workgroup left it, and that may have
      // been another chain's sweep with exactly the tag waited for here.
      lds_barrier();
#pragma unroll
      for (int k = 0; k < OMC_MAX_TERMS; ++k)
        if (k < nt && A.T.scale[k] && A.gb[k].enabled) load_hand_lds(k);
      lost = !tags_ok();  // (wave 0 passes NaN on under the right tag when the hand-over never came; this cannot fail)
    } else if (hand_lds) {
      // The producer is this workgroup's wave 0, still in the previous sweep's epilogue if this wave is ahead of it: a
      // loop of LDS reads only (no vector-memory wait in it: the previous sweep's x stores are still draining).
      // Bounded; a hand-over that never comes is reported.
      for (int spin = 0;; ++spin) {
#pragma unroll
        for (int k = 0; k < OMC_MAX_TERMS; ++k)
          if (k < nt && A.T.scale[k] && A.gb[k].enabled) load_hand_lds(k);
        if (tags_ok()) break;
        if (spin >= (1 << 22)) {
          if (threadIdx.x == 0 && chain_ok) atomicAdd(A.timeouts, 1ull);
          lost = true;
          break;
        }
        __builtin_amdgcn_s_sleep(2);
      }
    } else {
      // In-order dispatch puts the producer (a lower block index) on the chip first, so this loop normally never
      // turns; it is bounded all the same (about a second), and a hand-over that never comes is reported.
      for (int spin = 0;; ++spin) {
        if (tags_ok()) break;
        // (SIG 2: the consumer was on its CU long before the producer finished -- the poll interval is part of every
        // chain-update's latency; 64 cycles instead of 4096 between looks, the bound scaled to the same ~1 s)
        if (spin >= (EARLY ? (1 << 22) : (1 << 19))) {
          if (threadIdx.x == 0 && chain_ok) atomicAdd(A.timeouts, 1ull);
          lost = true;
          break;
        }
        if (!EARLY) __builtin_amdgcn_s_sleep(64);  // (SIG 2: back-to-back looks, a load round trip apart)
#pragma unroll
        for (int k = 0; k < OMC_MAX_TERMS; ++k)
          if (k < nt && A.T.scale[k] && A.gb[k].enabled) load_hand_global(k);
      }
    }
#pragma unroll
    for (int k = 0; k < OMC_MAX_TERMS; ++k)
      if (k < nt && A.T.scale[k] && A.gb[k].enabled)
        sc[k] = lost ? __builtin_nan("") : __hiloint2double((int)(uint32_t)hw[2 * k + 1], (int)(uint32_t)hw[2 * k]);
    if (EARLY && wave_u == 0 && lane == 0) {  // pass the scales (or the NaN of a lost hand-over) on
#pragma unroll
      for (int k = 0; k < OMC_MAX_TERMS; ++k)
        if (k < nt && A.T.scale[k] && A.gb[k].enabled) {
          const unsigned long long tg = (unsigned long long)want << 32;
          __hip_atomic_store(lds_hand + 2 * k, tg | (uint32_t)__double2loint(sc[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          __hip_atomic_store(lds_hand + 2 * k + 1, tg | (uint32_t)__double2hiint(sc[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    if (EARLY && wave_u == 0) lds_barrier();  // releases the fifteen waves waiting for these words
  };
  // per-sweep arguments (draw stream, output slab)
  auto nkey_f = [&]() -> omc_rng_key { return (MULTI && run_mode(A)) ? omc_make_key(A.seed, A.rec[sw].draw, OMC_RNG_NORMAL) : A.key; };
  auto x_out = [&]() -> double* { return (MULTI && run_mode(A)) ? A.rec[sw].x : A.x; };
  // SIG 1: which of the two terms is the tridiagonal one (wave-uniform; selects, not indexed kernel arguments)
  const bool p_first = SMO && A.T.diag[0] != nullptr;
  double sP = 1.0, sI = 1.0;  // the two scales by role; selected where first needed (a use up here would put the wait for
                              // the scalar loads in front of the first vector loads and draws)
  const double* const vPd = p_first ? A.T.diag[0] : A.T.diag[1];
  const double* const vPo = p_first ? A.T.off[0] : A.T.off[1];
  const double* const vIr = p_first ? A.T.rhs[1] : A.T.rhs[0];
  const double* const vIc = p_first ? A.T.center[1] : A.T.center[0];
  const double* const vSh = (SHIFT && A.cc.v) ? A.cc.v + cc * A.cc.ld : nullptr;  // SIG 3: this chain's centre vector c

  // diagnostic sweep clock: the constant-rate counter at this wave's entry, kept in two scalar registers to its exit
  unsigned long long t_enter = 0ull;
  if (MULTI && A.sweep_times) t_enter = __builtin_amdgcn_s_memrealtime();
  double Y[M], W[M];
  OMC_STAMP(0);
  // Normal-Gamma standard draws, made up front (see sweep_gamma_draws_wave) by the chain's last wave: its
  // tile is the one that may be partly empty, so it has the least other work
  const bool epi_wave = MULTI && A.fused && wave == 0;
  // the draws are parked in LDS until the epilogue: two registers that would otherwise be live (or, as the
  // compiler prefers, spilled to scratch by every wave) across the whole kernel.  SIG 1 makes them later, where
  // wave 0's SIMD has issue slots to spare (the opening phase is bound by the vector ALU there).
  if (!SMO && epi_wave && chain_ok) {
    bool f = false;
    const double g = sweep_gamma_draws_wave<MULTI && !SMO>(A, c, lane, &f, sw);
    lds_g[lane] = f ? -g : g;  // a Gamma draw is positive; the sign flags a draw that did not terminate
  }

  OMC_STAMP(1);
  // draws: stream position of this segment; SIG 1 makes all but the last pair ahead of the forward pass
  const int64_t gc = A.chain_offset + cc;
  const uint32_t blk0 = (uint32_t)(i0 >> 1);
  const bool gen_z = !A.z && !A.zero_z;
  // one pair of draws of this segment (Philox block blk0 + jb of the chain) into its lane-private LDS slots
  auto park_pair = [&](int jb) __attribute__((always_inline)) {
    double z0, z1;
    omc_normal_pair(omc_rng_block(nkey_f(), gc, blk0 + (uint32_t)jb), z0, z1);
    lds_z[wave][2 * jb][lane] = z0;
    lds_z[wave][2 * jb + 1][lane] = z1;
  };
  // the same pair made over the M loads of one coalesced vector (draws_over_load: full or partly empty wave)
  auto park_pair_over_load = [&](int jb, double (&v)[M], const double* base, int nvalid) __attribute__((always_inline)) {
    double z0, z1;
    if (nvalid == 64 * M) draws_over_load<M, true>(nkey_f(), gc, blk0 + (uint32_t)jb, z0, z1, v, base, lane, nvalid);
    else draws_over_load<M, false>(nkey_f(), gc, blk0 + (uint32_t)jb, z0, z1, v, base, lane, nvalid);
    lds_z[wave][2 * jb][lane] = z0;
    lds_z[wave][2 * jb + 1][lane] = z1;
  };
  // SIG 1: may this wave's off-diagonal slice be parked in the draws' LDS slots (see the forward pass)?
  // (SIG 3 parks the chain's own centre slice there instead: that one comes from HBM, the off-diagonal slice from L2)
  const double* const vPark = (SHIFT && OMC_SHIFT_PARK_C) ? vSh : vPo;
  const bool park_off = OMC_PARK_OFF && SMO && gen_z && (A.quad || A.fused) &&
                        wave_valid<M>(wave_u, (int)n - ((SHIFT && OMC_SHIFT_PARK_C) ? 0 : 1)) == 64 * M &&
                        (reinterpret_cast<uintptr_t>(vPark) & 15u) == 0;
  const bool park_diag = OMC_PARK_DIAG && SMO && (A.quad || A.fused) && wave_valid<M>(wave_u, (int)n) == 64 * M &&
                         (reinterpret_cast<uintptr_t>(vPd) & 15u) == 0;
  // SIG 2, the chain's last (partly empty) wave.  It cannot take the LDS-DMA parking as it stands (the transfers would read
  // past the end of the shared vectors) and used to fetch its three quadratic-form vectors inside the phase itself; with
  // a CU to itself per chain every wave waits for that one at the reduction's barrier (the per-wave timeline: 2 000 cycles).
  // Here it gets its own variant: the diagonal slice read back from the staged tile before x overwrites it, the
  // off-diagonal slice parked by transfers whose source is clamped to the last whole 16-byte pair (the consumer masks by
  // index; an odd last element comes from a scalar load), the centre vector prefetched with predicated loads.  The
  // arithmetic and its order are those of the other forms: results stay bit-identical.
  const int e_nv = EARLY ? wave_valid<M>(wave_u, (int)n) : 0, e_nvo = EARLY ? wave_valid<M>(wave_u, (int)n - 1) : 0;
  const bool e_partial = EARLY && (A.quad || A.fused) && e_nv > 0 && e_nv < 64 * M && !(A.rhs_chain && chain_ok);
  const bool park_off_p = OMC_PARK_OFF && e_partial && gen_z && e_nvo >= 2 && (reinterpret_cast<uintptr_t>(vPo) & 15u) == 0;
  double e_edge_o = 0.0;

  // Fewer chains than CUs ((sweep, chain) grid): this workgroup has been placed on an idle CU while the chain's previous
  // sweep is still running elsewhere, and all it can do until that sweep's scales arrive is what does not depend on them --
  // the loads and the draws.  Then ALL buffered pairs are made up here (nothing else is live yet), not spread over the
  // phases behind the hand-over where they would sit on the chain's critical path from sweep to sweep.
  // That is the SIG 2 instantiation (the host picks it for such launches): the three shared vectors are requested first
  // (60 registers that nothing else wants yet), the draws are made while they travel, wave 0 adds the Normal-Gamma standard
  // draws (functions of the priors only), and only then are the scales waited for -- with a tight poll: what follows the
  // hand-over is the chain's critical path from sweep to sweep, and a poll interval is on it.
  // (SIG 1 keeps the run-time form of the early draws: the host no longer asks for it, but without this block the
  // register allocator spills three registers of the hot path)
  const bool early1 = !EARLY && SMO && gen_z && A.early_draws != 0;
  const bool gen_late = gen_z && !EARLY && !early1;
  if constexpr (SMO && !EARLY) {
    if (early1) {
#pragma unroll
      for (int jb = 0; jb < NZB; ++jb) park_pair(jb);
    }
  }
  double pre[M];  // SIG 1, 2: the right-hand side vector
  // SIG 2 stages the three vectors while it waits, UNSCALED, in the mapping the recurrences read them in: the off-diagonal
  // slice in Y, the right-hand side in Rrow (both through the tile's transpose), the diagonal slice in the tile itself.
  // When the scales arrive b = sP Y, a_j = sP tile_j + sI and r_j = sI Rrow_j are single operations at the places that read
  // them -- the same values, bit for bit, as the scaled images the other forms write into the tile -- and the three tile
  // fills (thirty LDS operations per wave, bound by the CU's LDS bandwidth: ~1 us) are off the chain's critical path.
  double Rrow[EARLY ? M : 1], ebm1_raw = 0.0, ezl0 = 0.0, ezl1 = 0.0;
  if constexpr (EARLY) {
    // draws first (light on registers), the loads behind them: the workgroup waits for its scales far longer than a load
    // takes, so nothing has to travel under the draws -- and sixty registers of loads in flight beside them would spill
    if (gen_z) {
#pragma unroll
      for (int jb = 0; jb < NZB; ++jb) park_pair(jb);
    }
    if (epi_wave && chain_ok) {
      bool f = false;
      const double g = sweep_gamma_draws_wave(A, c, lane, &f, sw);
      lds_g[lane] = f ? -g : g;
    }
    if (gen_z) {
      // the segment's last pair as well: one value goes into the pad slot of this lane's tile row (the slot that staggers
      // the rows over the banks: no tile operation of this form touches it -- the one that would, the transfer of the
      // diagonal slice, does not happen here), the other stays in a register pair
      omc_normal_pair(omc_rng_block(nkey_f(), gc, blk0 + (uint32_t)NZB), ezl0, ezl1);
      crow[M] = ezl0;
    }
    __builtin_amdgcn_sched_barrier(0);
    const int wbase = wave_u * 64 * M;
    const int env = wave_valid<M>(wave_u, (int)n), envo = wave_valid<M>(wave_u, (int)n - 1);
    ebm1_raw = vPo[(i0 > 0 && i0 < n) ? i0 - 1 : 0];
    auto stage = [&](const double* base, int nvalid) {  // coalesced loads -> the wave's tile (zeros beyond the vector's end)
      double tmp[M];
      coal_load<M>(tmp, base, lane, nvalid);
      wave_lds_fence();
#pragma unroll
      for (int t = 0; t < M; ++t) *TM::elem(tl, r0, t) = tmp[t];
      wave_lds_fence();
    };
    if (!(A.rhs_chain && chain_ok)) {
      stage(vIr + wbase, env);
#pragma unroll
      for (int j = 0; j < M; ++j) Rrow[j] = crow[j];
    }
    stage(vPo + wbase, envo);
#pragma unroll
    for (int j = 0; j < M; ++j) Y[j] = crow[j];
    stage(vPd + wbase, env);  // stays in the tile until the pivots are final
    __builtin_amdgcn_sched_barrier(0);
    if (handed) {  // (workgroup-uniform) the LDS hand-over words: wiped before anybody looks
      if (threadIdx.x < 2 * OMC_MAX_TERMS) __hip_atomic_store(lds_hand + threadIdx.x, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      lds_barrier();
    }
  }
  // SIG 0: one parked pair of draws, made under the loads of a tile fill (see PARKZ)
  auto fill_draws = [&](int jb) {
    if constexpr (PARKZ && !SMO) {
      if (gen_z && jb < NZB) park_pair(jb);
    }
  };
  // ---- conditional precision: b -> Y (registers), a -> LDS tile ----
  double bm1 = 0.0;  // coupling b_{i0-1} into the segment
  if constexpr (SMO) {
    const int wbase = wave_u * 64 * M;
    const int nv = wave_valid<M>(wave_u, (int)n), nvo = wave_valid<M>(wave_u, (int)n - 1);
    // one vector (20 registers) in flight beside the generation of one pair of draws: more than that spills
    auto vec_and_draws = [&](double (&v)[M], const double* base, int nvalid, int jb) {
      if (gen_late && jb < NZB) park_pair_over_load(jb, v, base, nvalid);
      else coal_load<M>(v, base, lane, nvalid);
      __builtin_amdgcn_sched_barrier(0);
    };
    {
      double po[M];
      double bm1_raw;
      if constexpr (EARLY) {
        bm1_raw = ebm1_raw;
      } else {
        // b_{i0-1}: only loaded here; any arithmetic on it would put a wait for all loads in front of the draws
        bm1_raw = vPo[(i0 > 0 && i0 < n) ? i0 - 1 : 0];
        vec_and_draws(po, vPo + wbase, nvo, 0);
      }
      take_scales();
      if (SIG == 1 && A.reenter == 2 && handed && hand_lds && wave_u == 1 && chain_ok && any_handed_f()) {
        // the previous sweep's log-posterior, left here by its epilogue (scales: just taken; quadratic forms: LDS)
        double* const lp_prev = A.rec[sw - 1].log_post;
        if (lp_prev) {
          const int k = lane >> 4;
          const double sk = (k == 0) ? sc[0] : ((k == 1) ? sc[1] : ((k == 2) ? sc[2] : sc[3]));
          const double qk = (k < nt) ? __hip_atomic_load(lds_q + (k < nt ? k : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : 0.0;
          double ldk = 0.0;
          _Pragma("unroll") for (int t = 0; t < OMC_MAX_TERMS; ++t)
            if (t < nt && k == t && A.gb[t].logdet_unscaled) ldk = A.gb[t].logdet_unscaled[0];
          sweep_log_post_wave(A, c, lane, (k < nt) ? sk : 1.0, qk, ldk, lp_prev);
        }
      }
      sP = p_first ? sc[0] : sc[1];
      sI = p_first ? sc[1] : sc[0];
      if constexpr (EARLY) {
#pragma unroll
        for (int j = 0; j < M; ++j) Y[j] *= sP;
        if (!(A.rhs_chain && chain_ok)) {  // r = sI rhs: scaled here, where nothing else is live yet
#pragma unroll
          for (int j = 0; j < M; ++j) Rrow[j] *= sI;
        }
      } else {
        wave_lds_fence();
#pragma unroll
        for (int t = 0; t < M; ++t) *TM::elem(tl, r0, t) = sP * po[t];
        wave_lds_fence();
      }
      bm1 = (i0 > 0 && i0 < n) ? sP * bm1_raw : 0.0;
    }
    if constexpr (EARLY) {
      OMC_STAMP(2);
    } else {
      double pd[M];
      vec_and_draws(pd, vPd + wbase, nv, 1);
#pragma unroll
      for (int j = 0; j < M; ++j) Y[j] = crow[j];
      OMC_STAMP(2);
      wave_lds_fence();
      if (nv == 64 * M) {
#pragma unroll
        for (int t = 0; t < M; ++t) *TM::elem(tl, r0, t) = fma(sP, pd[t], sI);
      } else {
#pragma unroll
        for (int t = 0; t < M; ++t) *TM::elem(tl, r0, t) = (lane + 64 * t < nv) ? fma(sP, pd[t], sI) : 1.0;
      }
      wave_lds_fence();
    }
  } else {
    take_scales();
    if (MULTI) tile_fill_comb_wg<M, COMB_OFF>(tile, lane, wave, lbase, A, sc, chain_ok, cc, [&](int b) { if (b == 0) fill_draws(0); });
    else tile_fill_comb<M, MULTI, COMB_OFF>(tile, geo, A, sc);
#pragma unroll
    for (int j = 0; j < M; ++j) Y[j] = crow[j];
    if (i0 > 0 && i0 < n)
      _Pragma("unroll") for (int k = 0; k < OMC_MAX_TERMS; ++k) if (k < nt)
        if (A.T.off[k]) bm1 = fma(sc[k], A.T.off[k][i0 - 1], bm1);
    OMC_STAMP(2);
    if (MULTI) tile_fill_comb_wg<M, COMB_DIAG>(tile, lane, wave, lbase, A, sc, chain_ok, cc, [&](int b) { if (b == 0) fill_draws(1); });
    else tile_fill_comb<M, MULTI, COMB_DIAG>(tile, geo, A, sc);
  }
  const double* arow = crow;
  // the combined diagonal as the recurrences read it (SIG 2: scaled on the way out of the tile, see above)
  auto a_at = [&](int j) -> double {
    // (beyond the chain's end the staged image is 0, so a = sI there instead of the other forms' 1: those nodes are
    // decoupled from the chain -- b = 0 -- and take part in no result; any positive pivot serves)
    if constexpr (EARLY) return fma(sP, arow[j], sI);
    else return arow[j];
  };

  OMC_STAMP(3);
  // ---- Moebius product of the segment, scan -> incoming pivot ----
  double Dst;
  double Dnext0 = 0.0;  // the start value the NEXT segment derives from the same scan (up to rounding)
  {
    Mob m{1.0, 0.0, 0.0, 1.0};
    double bp = bm1;
#pragma unroll
    for (int j = 0; j < M; ++j) {
      const double b2 = bp * bp, aj = a_at(j);
      const double na = fma(aj, m.a, -b2 * m.c), nb = fma(aj, m.b, -b2 * m.d);
      m.c = m.a; m.d = m.b; m.a = na; m.b = nb;
      bp = Y[j];
      if ((j & 7) == 7) {  // cheap guard against overflow inside long segments: scale by the exponent of the leading entry
        const int ex = -__builtin_amdgcn_frexp_exp(m.a);
        m = Mob{ldexp(m.a, ex), ldexp(m.b, ex), ldexp(m.c, ex), ldexp(m.d, ex)};
      }
    }
    // (up to 7 steps since the guard above: entries as large as |a|^7, and sixteen such factors meet in the row pass.
    // Rescaled, the row pass sees leading entries in [1/2, 1) and entries below 2^s: see mob_rescale)
    m = mob_rescale(m);
    OMC_STAMP(4);
    const Mob idm{1.0, 0.0, 0.0, 1.0};
    const Mob E = MULTI ? excl_scan_wg<Mob, false, true>(m, idm, lds_mob, lane, wave, nw, lds_mob2)
                        : excl_scan<Mob, false>(m, idm, pos, Wd, false, lds_mob, wave, nw);
    Dst = (E.a + E.b) / (E.c + E.d);
    if (A.perturb_start != 0.0 && s > 0) Dst *= 1.0 + A.perturb_start;  // tests: a start the join test must reject
    if (MULTI) {
      const Mob inc = compose(m, E);
      Dnext0 = (inc.a + inc.b) * fast_rcp(inc.c + inc.d);
      if (A.perturb_start != 0.0) Dnext0 *= 1.0 + A.perturb_start;  // tests: the successor's start is spoiled the same way
    }
  }

  OMC_STAMP(5);
  // ---- true pivot recurrence, Newton multiple shooting on the segment joins ----
  bool bad = false;
  double lin = 0.0;  // l_{i0-1}
  // one pass of the true recurrence over the segment from Dst: W = 1/D, returns the last pivot
  auto pivot_pass = [&]() -> double {
    wave_lds_fence();  // re-read a from LDS every pass instead of keeping a register copy
    const double rst = fast_rcp(Dst);
    lin = bm1 * rst;
    double lp = lin, bprev = bm1, Dend = Dst;
    bool badp = false;
#pragma unroll
    for (int j = 0; j < M; ++j) {
      const double D = fma(-lp, bprev, a_at(j));
      badp |= !(D > 0.0);
      const double r = fast_rcp(D);
      W[j] = r;
      bprev = Y[j];
      lp = bprev * r;
      Dend = D;
    }
    bad = badp;
    return Dend;
  };
  double Dend = pivot_pass();
  // Join test.  Workgroup form: every segment tests the join at its END against the start value its successor
  // took from the Moebius scan, which it can compute itself (Dnext0): no neighbour exchange, one barrier.  97 %
  // of the cfg3 chains stop here.  Otherwise (and in the sub-wave form) the joins are tested at the segment
  // starts with an exchange, and corrected: Newton on the joins with Jacobian prod l^2, one affine scan each.
  bool settled = false;
  if (MULTI) {
    const bool has_next = i0 + M < n;
    const int need = (has_next && fabs(Dend - Dnext0) > OMC_NEWTON_TOL * fabs(Dnext0)) ? 1 : 0;  // false for NaN: -> `bad`
    settled = !any_wg(need, lds_any, lane, wave, nw);
  }
  for (int it = 0; !settled; ++it) {
    double J = lin * lin;  // d(last pivot)/d(start pivot) of this segment = prod of l^2 over it
#pragma unroll
    for (int j = 0; j + 1 < M; ++j) {
      const double l = Y[j] * W[j];
      J *= l * l;
    }
    double Dp = Dend, Jp = J;
    if (MULTI) prev_lane2_wg(Dp, Jp, Dst, 0.0, lds_x[it & 1], lane, wave, nw);
    else prev_lane2<false>(Dp, Jp, Dst, 0.0, pos, Wd, lds_x[0], wave);
    const bool joined = (s > 0 && i0 < n);
    const double e = joined ? (Dp - Dst) : 0.0;
    if (!joined) Jp = 0.0;
    const int need = (fabs(e) > OMC_NEWTON_TOL * fabs(Dst)) ? 1 : 0;  // false for NaN: falls through to `bad`
    const int any = MULTI ? __syncthreads_or(need) : (__ballot(need) != 0ull);  // (rare path: any_wg here costs the hot path 3 spilled registers)
    if (!any) break;
    if (it >= A.newton_max) {
      // Newton has not brought every join below the tolerance (a recurrence that is not contractive over a
      // segment: weak coupling, or |l| > 1 on a stretch).  Nothing is left to chance from here: the joins are
      // made consistent by the sequential recurrence itself.  Every pass starts each segment from the TRUE end
      // value of its predecessor's last pass, so after pass k the first k+1 segments carry exactly the pivots of
      // the serial kernel, and where the recurrence contracts, the rest converges geometrically at the same time;
      // the loop stops when every join meets the tolerance the Newton path accepts, at the latest after one pass per
      // segment.  (It used to insist on bit-equal joins.  On a homogeneous chain -- every segment the same map, as in
      // the headline model -- that is a worst case by construction: the map has two floating-point fixed points one
      // ulp apart, the part of the chain that converged from the spoiled starts sits on the other one than the part
      // propagated from the chain's head, and the border between them moves one segment per pass: all ~1000 passes,
      // 1.4 ms per chain-update measured by benchmarks/join_fallback_cost.py, for a difference of one ulp.)
      // About 1.4 us per pass; rare; counted in `fallbacks`.
      if (A.fallbacks && chain_ok && s == 0) atomicAdd(A.fallbacks, 1ull);
      const int S = MULTI ? (int)blockDim.x : Wd;
      for (int pass = 0; pass < S; ++pass) {
        double Dq = Dend, Jq = 0.0;
        if (MULTI) prev_lane2_wg(Dq, Jq, Dst, 0.0, lds_x[pass & 1], lane, wave, nw);
        else prev_lane2<false>(Dq, Jq, Dst, 0.0, pos, Wd, lds_x[0], wave);
        // (a NaN pivot compares false: it is `bad`, not a reason to go on)
        const int moved = (joined && fabs(Dq - Dst) > OMC_NEWTON_TOL * fabs(Dst)) ? 1 : 0;
        const int some = MULTI ? __syncthreads_or(moved) : (__ballot(moved) != 0ull);
        if (!some) break;
        if (joined) Dst = Dq;
        Dend = pivot_pass();
      }
      break;
    }
    const Aff own{e, Jp};
    const Aff ex = MULTI ? excl_scan_wg<Aff, false>(own, Aff{0.0, 1.0}, lds_aff[it & 1], lane, wave, nw)
                          : excl_scan<Aff, false>(own, Aff{0.0, 1.0}, pos, Wd, false, lds_aff[0], wave, nw);
    Dst += fma(Jp, ex.p, e);  // delta_s = e_s + J_{s-1} delta_{s-1}
    Dend = pivot_pass();
  }
  OMC_STAMP(6);
  double logdet = 0.0;
  // a chain with a non-positive pivot is reported through `bad`; its lanes continue on 1/D = 1 so that nothing
  // downstream sees the square root of a negative number (wave-uniform branch: no per-node selects)
  if (__ballot(bad) != 0ull) {
#pragma unroll
    for (int j = 0; j < M; ++j) W[j] = bad ? 1.0 : W[j];
  }
#pragma unroll
  for (int j = 0; j < M; ++j) {
    Y[j] *= W[j];               // l_j = b_j / D_j
    if (A.logdet && i0 + j < n) logdet -= log(W[j]);
  }

  OMC_STAMP(7);
  // ---- right-hand side -> tile; forward substitution (local affine map, scan, true pass) ----
  bool rhs_done = false;
  if constexpr (SMO) {
    // per-chain offsets (rhs_chain) go through the general fill below; the draws are made ahead in either case
    const bool with_offsets = A.rhs_chain && chain_ok;
    if (SHIFT && !with_offsets && !vIr) {  // SIG 3 without a shared centre: nothing to load, the pair is made plainly
#pragma unroll
      for (int t = 0; t < M; ++t) pre[t] = 0.0;
      if (gen_late && NZB > 2) park_pair(2);
    } else if (!with_offsets && !EARLY) {  // (SIG 2 asked for the vector at its start)
      const int nvr = wave_valid<M>(wave_u, (int)n);
      const double* base = vIr + wave_u * 64 * M;
      if (gen_late && NZB > 2) park_pair_over_load(2, pre, base, nvr);
      else coal_load<M>(pre, base, lane, nvr);
    }
    double csh[SHIFT ? M : 1];  // SIG 3: the chain's centre slice, requested here so that it travels under the next pair of draws
    if constexpr (SHIFT) {
      if (!with_offsets) {
        wave_lds_fence();
#pragma unroll
        for (int t = 0; t < M; ++t) *TM::elem(tl, r0, t) = sI * pre[t];  // (frees `pre`: one vector in flight beside a pair of draws)
        wave_lds_fence();
        coal_load<M>(csh, vSh + wave_u * 64 * M, lane, wave_valid<M>(wave_u, (int)n));
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (gen_late) {
#pragma unroll
      for (int jb = 2; jb < NZB; ++jb) {
        if (jb == 2 && !with_offsets) continue;  // made under the load above
        park_pair(jb);
      }
    }
    if (!with_offsets) {
      if constexpr (SHIFT) {  // r = sI (ys - c): the shared part is in the tile already
        wave_lds_fence();
#pragma unroll
        for (int t = 0; t < M; ++t) {
          double* pe = TM::elem(tl, r0, t);
          *pe = fma(-sI, csh[t], *pe);
        }
        wave_lds_fence();
      } else if constexpr (!EARLY) {  // (SIG 2: Rrow holds the scaled vector since the scales arrived)
        wave_lds_fence();
#pragma unroll
        for (int t = 0; t < M; ++t) *TM::elem(tl, r0, t) = sI * pre[t];
        wave_lds_fence();
      }
      rhs_done = true;
    }
  }
  if (rhs_done) {
  } else if (MULTI) {
    // (per-chain centres: SIG 0 only; SIG 0 makes two more pairs of draws under this fill's loads)
    if constexpr (SMO) tile_fill_comb_wg<M, COMB_RHS, false>(tile, lane, wave, lbase, A, sc, chain_ok, cc);
    else tile_fill_comb_wg<M, COMB_RHS, true>(tile, lane, wave, lbase, A, sc, chain_ok, cc, [&](int b) { fill_draws(2 + b); });
    if constexpr (EARLY) {  // (per-chain offsets: the general fill above; read out once, like the staged vector)
#pragma unroll
      for (int j = 0; j < M; ++j) Rrow[j] = crow[j];
    }
  } else {
    tile_fill_comb<M, MULTI, COMB_RHS>(tile, geo, A, sc);
  }
  constexpr bool PFQ = SMO && OMC_PREFETCH_QUAD;
  constexpr int PFQ_LOADS = M;  // loads the prefetch puts behind the LDS-DMA
  static_assert(!PFQ || PFQ_LOADS <= 15, "vmcnt immediate");
  double qcp[PFQ ? M : 1];
  double qcc[SHIFT ? M : 1];  // SIG 3: the chain's centre slice in the coalesced mapping (quadratic form's centre, x = c + e)
  bool pfq = false;
  // vector-memory loads issue_pfq has put on the wire, counted WHERE they are issued: the count-based wait in front of the parked
  // diagonal (below) is taken only if this says that at least PFQ_LOADS loads went out behind the transfer -- the wait's safety
  // follows from the counter, not from a remark about which paths issue loads (round 3's race was such a remark going stale)
  int pfq_behind = 0;
  auto issue_pfq = [&]() {
    if constexpr (PFQ) {
      const bool wq = A.quad || A.fused;
      pfq = wq && park_off && wave_valid<M>(wave_u, (int)n) == 64 * M;  // wave-uniform; other waves load in the phase itself
      __builtin_amdgcn_sched_barrier(0);  // not into the forward pass: its registers are all taken
      if constexpr (EARLY) {
        if (e_partial) {  // (wave-uniform) the last wave's centre slice, predicated
          const int wbase = wave_u * 64 * M;
#pragma unroll
          for (int t = 0; t < M; ++t) qcp[t] = (lane + 64 * t < e_nv) ? (vIc + wbase)[(unsigned)(lane + 64 * t)] : 0.0;
        }
      }
      if (pfq) {
        const int wbase = wave_u * 64 * M;
        if (!SHIFT || vIc) {
#pragma unroll
          for (int t = 0; t < M; ++t) qcp[t] = (vIc + wbase)[(unsigned)(lane + 64 * t)];
          pfq_behind += M;
        } else {
#pragma unroll
          for (int t = 0; t < M; ++t) qcp[t] = 0.0;
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  OMC_STAMP(8);
  auto r_at = [&](int j) -> double {  // the right-hand side as the forward substitution reads it
    if constexpr (EARLY) return Rrow[j];
    else return crow[j];
  };
  {
    Aff f{0.0, 1.0};
    double lp = lin;
#pragma unroll
    for (int j = 0; j < M; ++j) {
      f.p = fma(-lp, f.p, r_at(j));
      f.q = -lp * f.q;
      lp = Y[j];
    }
    double u = (MULTI ? excl_scan_wg<Aff, false>(f, Aff{0.0, 1.0}, lds_aff[2], lane, wave, nw)
                      : excl_scan<Aff, false>(f, Aff{0.0, 1.0}, pos, Wd, false, lds_aff[0], wave, nw)).p;
    lp = lin;
    OMC_STAMP(9);
    // g_j = u_j/D_j + z_j/sqrt(D_j); the draws are produced here, pair by pair, so that no array of
    // z ever has to be kept in registers next to l and 1/D (Philox + Box-Muller interleave with the
    // serial u recurrence; the scheduling barrier keeps the five bodies from being overlapped)
    const double* zin = A.z ? A.z + cc * A.ld_z + i0 : nullptr;
#pragma unroll
    for (int j = 0; j < M; j += 2) {
      double z0 = 0.0, z1 = 0.0;
      if (zin) {
        if (i0 + j < n) z0 = zin[j];
        if (i0 + j + 1 < n) z1 = zin[j + 1];
        // injected draws (tests): waited for HERE.  Left pending, these loads meet the in-kernel-draw path at the join below,
        // and the compiler's wait-count pass -- which must assume either predecessor -- then puts an `s_waitcnt vmcnt(0)`
        // into the shared code: behind the quadratic-form prefetches of SIG 1 that wait exposed the whole L2 latency of
        // twelve loads on every sweep of the production path.
        if (SMO) __builtin_amdgcn_s_waitcnt(0x0F70);
      } else if (PARKZ && (j >> 1) < NZB) {
        if (gen_z) { z0 = lds_z[wave][j][lane]; z1 = lds_z[wave][j + 1][lane]; }
      } else if (!A.zero_z) {
        if constexpr (SMO) {
          // The parked draws have all been read: their LDS slots now take the first 128 NZB entries of this
          // wave's slice of the off-diagonal vector for the quadratic forms (LDS-DMA, no registers), under the
          // generation of the segment's last pair of draws.
          if (j == 2 * NZB && park_off) {
            lds_reads_done();
#pragma unroll
            for (int k = 0; k < NZB; ++k)
              __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(vPark + wave_u * 64 * M + 128 * k + 2 * lane),
                                               (__attribute__((address_space(3))) void*)&lds_z[wave][2 * k][0], 16, 0, 0);
          }
          if constexpr (EARLY) {
            if (j == 2 * NZB && park_off_p) {  // (wave-uniform)
              lds_reads_done();
              const int last_pair = (e_nvo - 2) & ~1;
#pragma unroll
              for (int k = 0; k < NZB; ++k) {
                const int e = 128 * k + 2 * lane;
                const int ec = (e + 1 < e_nvo) ? e : last_pair;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(vPo + wave_u * 64 * M + ec),
                                                 (__attribute__((address_space(3))) void*)&lds_z[wave][2 * k][0], 16, 0, 0);
              }
              if (e_nvo & 1) e_edge_o = vPo[wave_u * 64 * M + e_nvo - 1];
            }
          }
        }
        if constexpr (EARLY) {
          z0 = crow[M]; z1 = ezl1;  // (made while the scales were waited for: one pair of draws less on the critical path)
        } else {
          omc_normal_pair(omc_rng_block(nkey_f(), gc, blk0 + (uint32_t)(j >> 1)), z0, z1);
        }
      }
      u = fma(-lp, u, r_at(j));
      W[j] = fma(u, W[j], z0 * fast_sqrt(W[j]));
      lp = Y[j];
      u = fma(-lp, u, r_at(j + 1));
      W[j + 1] = fma(u, W[j + 1], z1 * fast_sqrt(W[j + 1]));
      lp = Y[j + 1];
      if (!(PARKZ && (j >> 1) < NZB - 1)) __builtin_amdgcn_sched_barrier(0);  // parked draws: let the pairs pipeline
    }
  }

  OMC_STAMP(10);
  const bool want_quad = A.quad || A.fused;
  // SIG 1: the tile's right-hand side is dead now; until x is written into it, it takes this wave's slice of
  // the tridiagonal term's diagonal (LDS-DMA, contiguous image), which the back pass below reads in the row
  // mapping for the x' diag x part of the quadratic form -- one vector less to wait for afterwards
  double aPd = 0.0;
  double eqd[EARLY ? M : 1];  // SIG 2, last wave: its diagonal slice in the coalesced mapping, taken before x overwrites the tile
  // SIG 2 without per-chain offsets: the wave's diagonal slice has been sitting in the tile, unscaled, since the workgroup
  // started (nothing wrote the tile after the pivots): no transfer, the back pass reads the staged rows
  const bool diag_staged = EARLY && !(A.rhs_chain && chain_ok);
  if constexpr (SMO) {
    if (park_diag && !diag_staged) {
      lds_reads_done();
#pragma unroll
      for (int k = 0; k < (64 * M) / 128; ++k)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(vPd + wave_u * 64 * M + 128 * k + 2 * lane),
                                         (__attribute__((address_space(3))) void*)(tile + 128 * k), 16, 0, 0);
    }
  }
  // SIG 1: the centre vector, the rest of what the quadratic forms read from L2, is fetched here into registers: the
  // reverse scan and the back pass (a tenth of the wave's lifetime, light on registers) cover its latency, and the
  // quadratic-form phase's x stores start a load round trip earlier (OMC_PREFETCH_QUAD; measured on
  // benchmarks/ab_headline.py).
  issue_pfq();
  // ---- backward substitution: local affine map, reverse scan, true pass ----
  double xnext;
  {
    Aff f{0.0, 1.0};
#pragma unroll
    for (int j = M - 1; j >= 0; --j) {
      f.p = fma(-Y[j], f.p, W[j]);
      f.q = -Y[j] * f.q;
    }
    xnext = (MULTI ? excl_scan_wg<Aff, true>(f, Aff{0.0, 1.0}, lds_aff[3], lane, wave, nw)
                   : excl_scan<Aff, false>(f, Aff{0.0, 1.0}, pos, Wd, true, lds_aff[0], wave, nw)).p;
    double x = xnext;
    OMC_STAMP(11);
    if constexpr (EARLY) {
      if (e_partial) {
        wave_lds_fence();
#pragma unroll
        for (int t = 0; t < M; ++t) eqd[t] = *TM::elem(tl, r0, t);
      }
    }
    if (SMO && park_diag) {
      // the LDS-DMA has landed: vector-memory operations retire in order, so it is enough that no more than the prefetch
      // loads issued BEHIND it are still out (they are not needed before the quadratic forms)
      // (SIG 3 without a shared centre issues NO prefetch loads -- issue_pfq sets the slice to zero --, and then "at most
      // PFQ_LOADS still out" says nothing about the transfer: the diagonal was read before it had landed now and then, and
      // the late transfer overwrote the x this wave had meanwhile put into the tile.  One chain in a few thousand sweeps of
      // the hierarchical smoother at n = 10 000 x 1024 chains, found by benchmarks/determinism_hier.py.)
      if (!diag_staged) {
        // (issue_pfq ran behind the transfer and left at least PFQ_LOADS loads behind it: then "at most PFQ_LOADS still out"
        //  means the transfer is not among them)
        if (PFQ && pfq_behind >= PFQ_LOADS) __builtin_amdgcn_s_waitcnt(0x0F70 | PFQ_LOADS);
        else __builtin_amdgcn_s_waitcnt(0x0F70);
      }
      wave_lds_fence();
      const double* drow = diag_staged ? crow : tile + lane * M;  // the staged rows (padded), or the transfer's contiguous image
#pragma unroll
      for (int j = M - 1; j >= 0; --j) {
        x = fma(-Y[j], x, W[j]);
        W[j] = x;
        aPd = fma(drow[j] * x, x, aPd);
      }
    } else {
#pragma unroll
      for (int j = M - 1; j >= 0; --j) {
        x = fma(-Y[j], x, W[j]);
        W[j] = x;
      }
    }
  }
  OMC_STAMP(12);
  double qsum[OMC_MAX_TERMS] = {0, 0, 0, 0};
  double my_scale = 1.0, my_logdet = 0.0;  // epilogue scalars of this lane's term (wave 0)
  if (MULTI) {
    // ---- store + fused quadratic forms, both in the coalesced mapping: lane handles nodes
    //      wbase + t*64 + lane; x comes back from the tile, the shared vectors straight from L2 ----
    wave_lds_fence();
#pragma unroll
    for (int j = 0; j < M; ++j) crow[j] = W[j];
    // x at the first node of the NEXT wave's tile = what the reverse scan handed this wave's last segment as
    // its successor value; it goes behind the last row so that every node finds x_{i+1} one element on
    if (lane == 63) tile[64 * (M + 1)] = xnext;
    wave_lds_fence();  // wave-private tile: no workgroup barrier needed
    double acc[OMC_MAX_TERMS] = {0, 0, 0, 0};
    // scalars of the epilogue: issue their loads now so the latency hides behind the quad phase
    if (epi_wave) {  // lane group k = lane >> 4 serves term k
      _Pragma("unroll") for (int k = 0; k < OMC_MAX_TERMS; ++k) if (k < nt && (lane >> 4) == k) {
        if (A.T.scale[k]) my_scale = handed ? sc[k] : A.T.scale[k][cc];
        if constexpr (SMO) {
          if (sweep_log_post(A, sw) && A.gb[k].logdet_unscaled) my_logdet = A.gb[k].logdet_unscaled[0];
        }
      }
      if constexpr (!SMO) {  // (the blocks' device image: see TriArgs::gb_dev)
        const double* const ldp = ((lane >> 4) < nt) ? A.gb_dev[lane >> 4].logdet_unscaled : nullptr;
        if (sweep_log_post(A, sw) && ldp) my_logdet = ldp[0];
      }
    }
    if constexpr (SMO) {
      // Normal-Gamma standard draws (functions of the priors only): here, in front of the load-bound phase of
      // the quadratic forms, wave 0's delay costs nothing -- the other waves' loads keep the L2 path busy
      if (!EARLY && epi_wave && chain_ok) {  // (SIG 2: made at the start, while the scales were waited for)
        bool f = false;
        const double g = sweep_gamma_draws_wave(A, c, lane, &f, sw);
        lds_g[lane] = f ? -g : g;
      }
      const int nv = wave_valid<M>(wave_u, (int)n);
      double qc[M], qd[M], qo[M];
      {
        const int wbase = wave_u * 64 * M;
        const int nvq = want_quad ? nv : 0, nvo = want_quad ? wave_valid<M>(wave_u, (int)n - 1) : 0;
        {
          if (park_off && SHIFT && OMC_SHIFT_PARK_C) {  // the parked slice is the chain's centre; the off-diagonal comes from L2
            const double* zf = &lds_z[wave][0][0];
            coal_load<M>(qo, vPo + wbase, lane, nvo);
            // the transfers (older than these M loads) have landed.  The M loads are M instructions issued right here on every
            // path: park_off says the wave is full, so nvo >= 64 M - 1 and no load has all its lanes predicated off
            __builtin_amdgcn_s_waitcnt(0x0F70 | M);
            wave_lds_fence();
#pragma unroll
            for (int t = 0; t < M; ++t)
              if (t < 2 * NZB) qcc[t] = zf[64 * t + lane];
#pragma unroll
            for (int t = 0; t < M; ++t) {
              if (t < 2 * NZB) continue;
              qcc[t] = (vSh + wbase)[(unsigned)(lane + 64 * t)];
            }
          } else if (park_off) {
            const double* zf = &lds_z[wave][0][0];
            __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the LDS-DMA has landed (the reverse scan's barrier drained it already)
            wave_lds_fence();
#pragma unroll
            for (int t = 0; t < M; ++t)
              if (t < 2 * NZB) qo[t] = zf[64 * t + lane];
#pragma unroll
            for (int t = 0; t < M; ++t) {
              if (t < 2 * NZB) continue;
              qo[t] = OMC_WHATIF_NOQLOAD ? 0.25 : (vPo + wbase)[(unsigned)(lane + 64 * t)];
            }
          } else if (EARLY && park_off_p) {
            const double* zf = &lds_z[wave][0][0];
            __builtin_amdgcn_s_waitcnt(0x0F70);  // the transfers (and the centre prefetch behind them) have landed
            wave_lds_fence();
#pragma unroll
            for (int t = 0; t < M; ++t) {
              const int idx = lane + 64 * t;
              double v = 0.0;
              if (t < 2 * NZB) v = zf[idx];
              else if (idx < nvo) v = (vPo + wbase)[(unsigned)idx];  // (a last wave of more than 512 nodes)
              qo[t] = (idx < nvo) ? (((nvo & 1) && idx == nvo - 1) ? e_edge_o : v) : 0.0;
            }
          } else {
            coal_load<M>(qo, vPo + wbase, lane, nvo);
          }
        }
        if (EARLY && e_partial) {
#pragma unroll
          for (int t = 0; t < M; ++t) qd[t] = eqd[t];
        } else if (park_diag) {
#pragma unroll
          for (int t = 0; t < M; ++t) qd[t] = 0.0;  // that part is in aPd already
        } else {
          coal_load<M>(qd, vPd + wbase, lane, nvq);
        }
        if (OMC_WHATIF_NOQLOAD) {
#pragma unroll
          for (int t = 0; t < M; ++t) qc[t] = 1.0;
        } else if (PFQ && (pfq || (EARLY && e_partial))) {
#pragma unroll
          for (int t = 0; t < M; ++t) qc[t] = qcp[t];
        } else if (SHIFT && !vIc) {
#pragma unroll
          for (int t = 0; t < M; ++t) qc[t] = 0.0;
        } else {
          coal_load<M>(qc, vIc + wbase, lane, nvq);
        }
        if constexpr (SHIFT) {
          if (!(park_off && OMC_SHIFT_PARK_C)) coal_load<M>(qcc, vSh + wbase, lane, nv);
#pragma unroll
          for (int t = 0; t < M; ++t) qc[t] -= qcc[t];  // the identity term's centre in e-coordinates: ys - c
        }
      }
      double aI = 0.0, aP = aPd;
      // x leaves from the same pass, behind the loads issued above (vmcnt retires in order: nothing waits on the
      // x stream, and the 80 KB of stores drain under the reduction and the epilogue instead of after them)
      double* const xb = x_out();
      double* xo = (xb && chain_ok) ? xb + cc * A.ld_x + wave_u * 64 * M : nullptr;
      // one full-wave element of x on its way out (SIG 3: x = c + e): written once and never read back by this kernel, so a
      // streaming (nontemporal) store
      auto store_x = [&](int t, double xv) __attribute__((always_inline)) {
        if (xo && !OMC_WHATIF_NOSTORE) __builtin_nontemporal_store(SHIFT ? xv + qcc[t] : xv, &xo[(unsigned)(lane + 64 * t)]);
      };
      if (!want_quad) {
        if (xo) {
#pragma unroll
          for (int t = 0; t < M; ++t)
            if (lane + 64 * t < nv) xo[(unsigned)(lane + 64 * t)] = SHIFT ? *TM::elem(tl, r0, t) + qcc[t] : *TM::elem(tl, r0, t);
        }
      } else if (nv == 64 * M && park_diag) {  // the diagonal part is in aPd already
#pragma unroll
        for (int t = 0; t < M; ++t) {
          const double* pe = TM::elem(tl, r0, t);
          const double xv = *pe, xn = *TM::succ(pe, r0, t), a = xv - qc[t];
          aI = fma(a, a, aI);
          aP = fma(2.0 * qo[t] * xn, xv, aP);
          store_x(t, xv);
        }
      } else if (nv == 64 * M) {
#pragma unroll
        for (int t = 0; t < M; ++t) {
          const double* pe = TM::elem(tl, r0, t);
          const double xv = *pe, xn = *TM::succ(pe, r0, t), a = xv - qc[t];
          aI = fma(a, a, aI);
          aP = fma(fma(2.0 * qo[t], xn, qd[t] * xv), xv, aP);
          store_x(t, xv);
        }
      } else {  // the chain's last wave: nodes beyond n hold finite fill values, their vectors were loaded as 0
#pragma unroll
        for (int t = 0; t < M; ++t) {
          const double* pe = TM::elem(tl, r0, t);
          const double xv = *pe, xn = *TM::succ(pe, r0, t), a = (lane + 64 * t < nv) ? xv - qc[t] : 0.0;
          aI = fma(a, a, aI);
          aP = fma(fma(2.0 * qo[t], xn, qd[t] * xv), xv, aP);
          if (xo && lane + 64 * t < nv) xo[(unsigned)(lane + 64 * t)] = SHIFT ? xv + qcc[t] : xv;
        }
      }
      acc[0] = p_first ? aP : aI;
      acc[1] = p_first ? aI : aP;
    } else {
      if (want_quad) quad_wg<M>(tile, lane, wave_u, lbase, A, acc, cc);
    }
    OMC_STAMP(13);
    if (want_quad) {
      sum4_wg(acc, qsum, nt, &lds_d[0][0], lane, wave, nw);  // all terms behind one barrier
      _Pragma("unroll") for (int k = 0; k < OMC_MAX_TERMS; ++k) if (k < nt) {
        if (A.quad && s == 0 && chain_ok) A.quad[k * A.C + c] = qsum[k];
      }
    }
  } else {
  if (A.x) {
    wave_lds_fence();
#pragma unroll
    for (int j = 0; j < M; ++j) crow[j] = W[j];
    tile_store_chain<M, MULTI>(tile, geo, A.x, A.ld_x, n, A.C);
  }

  // ---- fused quadratic forms (x - m_k)' M_k (x - m_k), segment-local form ----
  if (want_quad) {
    double X[M];  // residuals
    _Pragma("unroll") for (int k = 0; k < OMC_MAX_TERMS; ++k) if (k < nt) {
      // residual of this segment in X, residual of the next segment's first node in rn
      double rn = 0.0;
      if (A.T.center[k]) {
        tile_fill_shared<M, MULTI>(tile, geo, A.T.center[k], n, 0.0);
#pragma unroll
        for (int j = 0; j < M; ++j) X[j] = W[j] - trow[j];
        if (i0 + M < n) rn = xnext - A.T.center[k][i0 + M];
      } else {
#pragma unroll
        for (int j = 0; j < M; ++j) X[j] = W[j];
        if (i0 + M < n) rn = xnext;
      }
      double acc = 0.0;
      if (A.T.diag[k]) {
        tile_fill_shared<M, MULTI>(tile, geo, A.T.diag[k], n, 0.0);
#pragma unroll
        for (int j = 0; j < M; ++j) acc = fma(trow[j] * X[j], X[j], acc);
      } else {
#pragma unroll
        for (int j = 0; j < M; ++j)
          if (i0 + j < n) acc = fma(X[j], X[j], acc);
      }
      if (A.T.off[k]) {
        tile_fill_shared<M, MULTI>(tile, geo, A.T.off[k], n - 1, 0.0);
#pragma unroll
        for (int j = 0; j < M; ++j) acc = fma(2.0 * trow[j] * X[j], (j + 1 < M) ? X[(j + 1) % M] : rn, acc);
      }
      qsum[k] = group_sum<false>(acc, Wd, lds_d[0], wave, nw);
      if (A.quad && s == 0 && chain_ok) A.quad[k * A.C + c] = qsum[k];
    }
  }
  }
  OMC_STAMP(14);
  if (A.logdet) {
    const double t = MULTI ? sum_wg(logdet, lds_d[4], lane, wave, nw) : group_sum<false>(logdet, Wd, lds_d[0], wave, nw);
    if (s == 0 && chain_ok) A.logdet[c] = t;
  }
  if (bad && chain_ok) atomicMin((unsigned long long*)A.bad, (unsigned long long)c);
  if (MULTI) {
    if (epi_wave && chain_ok) {
      const double g = lds_g[lane];
      // restart without a barrier: the log-posterior of this sweep is left to wave 1 of the next one (it has the slack
      // this wave does not: everyone waits for the wave that ran the epilogue at the next sweep's first barrier)
      const bool defer_lp = SIG == 1 && A.reenter == 2 && left > 0 && nw > 1 && any_handed_f();
      sweep_epilogue_wave<!SMO>(A, c, qsum[0], qsum[1], qsum[2], qsum[3], my_scale, my_logdet, fabs(g), g < 0.0, lane, sw,
                          (SIG == 1 && A.reenter) ? lds_hand : nullptr, defer_lp, lds_q);
    }
    // x leaves last: a load issued behind a store would have to wait for the store to be
    // acknowledged (vmcnt retires in order); this way nothing ever waits on the x stream.
    // (The specialised forms have stored it from their quadratic-form pass already.)
    const bool store_here = !SMO;
    double* const xb = store_here ? x_out() : nullptr;
    if (store_here && xb && chain_ok) {
      double* xo = xb + cc * A.ld_x + wave_u * 64 * M;
      const int nvalid = wave_valid<M>(wave_u, (int)n);
      {
        if (nvalid == 64 * M) {
#pragma unroll
          for (int t = 0; t < TM::NS; ++t)
            xo[(unsigned)(lane + t * TM::LU)] = *TM::elem(tl, r0, t);
        } else {
#pragma unroll
          for (int t = 0; t < TM::NS; ++t) {
            const int idx = lane + t * TM::LU;
            if (idx < nvalid) xo[(unsigned)idx] = *TM::elem(tl, r0, t);
          }
        }
      }
    }
  } else if (A.fused && s == 0 && chain_ok) {
    sweep_epilogue(A, c, qsum);
  }
  OMC_STAMP(15);
  if (MULTI && A.sweep_times && threadIdx.x == 0 && chain_ok) {
    // wave 0 is the one that runs the epilogue: its exit is the end of the chain's sweep (self-restarting workgroups: its
    // next entry follows at once, so consecutive records of a chain tile the launch)
    const unsigned long long t_exit = __builtin_amdgcn_s_memrealtime();
    int64_t r = A.sweep_times_pos + sw;
    if (r >= A.sweep_times_cap) r -= A.sweep_times_cap;
    unsigned long long* const p = A.sweep_times + (r * A.C + c) * 2;
    p[0] = t_enter;
    p[1] = t_exit;
  }
  if (MULTI && SIG == 1 && A.reenter && left > 0) {
    // Restart as the workgroup of the chain's next sweep: same code from its first instruction, with the three
    // registers a fresh workgroup is handed (kernel-argument pointer, workgroup id, work-item id) set to what the
    // dispatcher would have put there for block index + C.  Nothing else is live at a kernel's entry.  What this
    // buys over a fresh workgroup: the x stores of this sweep drain under the next sweep's loads and draws instead of
    // holding the CU until they are acknowledged, and there is no dispatch gap between the sweeps of a chain.
    // (vmcnt is not zero on re-entry -- the waits of the next sweep only become conservative.)
    if (A.reenter != 2) lds_barrier();  // every wave is done with this sweep's LDS image (2: see DESIGN, no barrier)
    const uint64_t kptr = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr();
    const uint64_t kargs = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)kptr) |
                           ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(kptr >> 32)) << 32);
    const uint32_t next_blk = (uint32_t)__builtin_amdgcn_readfirstlane(
        (int)(0x80000000u | ((uint32_t)(left - 1) << 26) | ((uint32_t)(sw + 1) * (uint32_t)A.C + c_blk)));
    const uint32_t tid = threadIdx.x;
    // (device code may not name a kernel, so the entry point is reached through its linker symbol: a name that does
    // not match an instantiation fails the link, not the run)
#define OMC_REENTER(Mv, MAXTv, SIGv)                                                                                  \
  if constexpr (M == Mv && MAXT == MAXTv && SIG == SIGv)                                                              \
    asm volatile("s_mov_b64 exec, -1\n\ts_getpc_b64 s[4:5]\n\t"                                                      \
                 "s_add_u32 s4, s4, _Z13k_tridiag_segILi" #Mv "ELb1ELi" #MAXTv "ELi" #SIGv "EEv7TriArgsi@rel32@lo+4\n\t" \
                 "s_addc_u32 s5, s5, _Z13k_tridiag_segILi" #Mv "ELb1ELi" #MAXTv "ELi" #SIGv "EEv7TriArgsi@rel32@hi+12\n\t" \
                 "s_setpc_b64 s[4:5]" ::"{s[0:1]}"(kargs), "{s2}"(next_blk), "{v0}"(tid) : "memory", "s4", "s5")
    OMC_REENTER(8, 1024, 1);
    OMC_REENTER(10, 1024, 1);
#undef OMC_REENTER
  }
}


// ------------------------------------------------------------------------------------------
// Self-check of what the restart above takes for granted.  `s_setpc_b64` to the kernel's first instruction reproduces a
// fresh workgroup only if the kernel descriptor asks the dispatcher for exactly the three registers the restart sets:
// two user SGPRs (the kernel-argument pointer, nothing else: no dispatch / queue pointer, no dispatch id, no flat-scratch
// init, no preloaded kernel arguments), workgroup id x as the only system SGPR, the packed work-item id in v0, and no
// private segment.  The descriptors of the re-entered instantiations are read HERE, from the code object the runtime
// actually loaded (their `.kd` linker symbols), and compared on the host before the first restarting launch; a mismatch
// (another compiler, another flag) switches the restarting form off for the process instead of producing wrong chains.
// tests/test_kernel_resources.py checks the same facts at build time without a GPU.
#define OMC_KD_WORDS(Mv, MAXTv, SIGv, dst)                                                                               \
  do {                                                                                                                    \
    uint64_t kd_;                                                                                                         \
    asm volatile("s_getpc_b64 s[4:5]\n\t"                                                                                \
                 "s_add_u32 s4, s4, _Z13k_tridiag_segILi" #Mv "ELb1ELi" #MAXTv "ELi" #SIGv "EEv7TriArgsi.kd@rel32@lo+4\n\t"  \
                 "s_addc_u32 s5, s5, _Z13k_tridiag_segILi" #Mv "ELb1ELi" #MAXTv "ELi" #SIGv "EEv7TriArgsi.kd@rel32@hi+12\n\t" \
                 "s_mov_b64 %0, s[4:5]"                                                                                   \
                 : "=s"(kd_)::"s4", "s5");                                                                               \
    const uint32_t* w_ = (const uint32_t*)kd_;                                                                            \
    (dst)[0] = w_[1];  /* PRIVATE_SEGMENT_FIXED_SIZE */                                                                    \
    (dst)[1] = w_[13]; /* COMPUTE_PGM_RSRC2 */                                                                             \
    (dst)[2] = w_[14]; /* kernel code properties (low half), kernarg preload spec (high half) */                           \
  } while (0)
