// Tile traffic of k_tridiag_seg (omc_tridiag.hip): the wave-private LDS tile between "lane owns M consecutive nodes" and
// coalesced global accesses -- geometry, fences, fills, the store, the coalesced loads and the fused quadratic forms.
#pragma once
#include "omc_tridiag_args.h"

// ------------------------------------------------------------------------------------------
// Wave-private LDS tile: converts between "lane owns M consecutive nodes" (registers) and
// "64 consecutive lanes touch 64 consecutive doubles" (global memory).  Tile element e
// (0 <= e < 64*M; e = lane'*M + j) lives at tile[e + e/M]: row stride M+1 doubles, so the
// per-lane reads at stride M+1 (odd) are bank-conflict free for ds_read_b64.
template <int M, bool MULTI>
struct Geom {
  int lane, wave, G;   // G: lanes per chain (sub-wave groups) when !MULTI
  int64_t chain0;      // MULTI: the chain; else first chain of this wave
  __device__ __forceinline__ int64_t node(int e) const {
    const int lp = e / M, j = e - lp * M;
    const int seg = MULTI ? (wave * 64 + lp) : (lp & (G - 1));
    return (int64_t)seg * M + j;
  }
  __device__ __forceinline__ int64_t chain(int e) const { return MULTI ? chain0 : chain0 + (e / M) / G; }
};

__device__ __forceinline__ void wave_lds_fence() {
  // DS operations of one wave execute in order; this only stops the compiler from moving them.
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// In front of an LDS-DMA (global_load_lds) into a region this wave has been reading: the DMA's write reaches
// LDS through the vector-memory path, not the DS queue, so "DS operations execute in order" does not cover
// it -- a ds_read that has been issued but not yet served could see the new bytes.  Wait until every DS
// operation of the wave has returned (lgkmcnt(0); vmcnt and expcnt left alone).
__device__ __forceinline__ void lds_reads_done() {
  wave_lds_fence();
  __builtin_amdgcn_s_waitcnt(0xC07F);
  wave_lds_fence();
}

// shared vector v[0..lim) -> tile (fill beyond lim); every sub-wave group then reads rows 0..G-1
template <int M, bool MULTI>
__device__ __forceinline__ void tile_fill_shared(double* tile, const Geom<M, MULTI>& g, const double* v, int64_t lim,
                                                 double fill) {
  wave_lds_fence();
#pragma unroll 2
  for (int t = 0; t < M; ++t) {
    const int e = t * 64 + g.lane;
    const int64_t nd = g.node(e);
    tile[e + e / M] = (nd < lim) ? v[nd] : fill;
  }
  wave_lds_fence();
}
// per-chain vector v[chain*ld + node]; one tile row per lane
template <int M, bool MULTI>
__device__ __forceinline__ void tile_fill_chain(double* tile, const Geom<M, MULTI>& g, const double* v, int64_t ld,
                                                int64_t lim, int64_t C, double fill) {
  wave_lds_fence();
#pragma unroll 2
  for (int t = 0; t < M; ++t) {
    const int e = t * 64 + g.lane;
    const int64_t nd = g.node(e), ch = g.chain(e);
    tile[e + e / M] = (nd < lim && ch < C) ? v[ch * ld + nd] : fill;
  }
  wave_lds_fence();
}
template <int M, bool MULTI>
__device__ __forceinline__ void tile_store_chain(const double* tile, const Geom<M, MULTI>& g, double* v, int64_t ld,
                                                 int64_t lim, int64_t C) {
  wave_lds_fence();
#pragma unroll 2
  for (int t = 0; t < M; ++t) {
    const int e = t * 64 + g.lane;
    const int64_t nd = g.node(e), ch = g.chain(e);
    if (nd < lim && ch < C) v[ch * ld + nd] = tile[e + e / M];
  }
  wave_lds_fence();
}

// Per-chain combination of the shared term vectors, formed while the tile is filled (coalesced):
//   DIAG: a = sum_k s_k diag_k (1 beyond n), OFF: b = sum_k s_k off_k, RHS: r = sum_k s_k rhs_k + rhs_chain
enum { COMB_DIAG = 0, COMB_OFF = 1, COMB_RHS = 2 };
// nodes per lane handled per batch of loads (memory-level parallelism vs registers)
#define OMC_CH(M) ((M) % 5 == 0 ? 5 : 4)
template <int M, bool MULTI, int WHICH>
__device__ __forceinline__ void tile_fill_comb(double* tile, const Geom<M, MULTI>& g, const TriArgs& A,
                                               const double (&sc)[OMC_MAX_TERMS]) {
  const int nt = A.T.n_terms;
  const int64_t n = A.n;
  wave_lds_fence();
#pragma unroll 2
  for (int t = 0; t < M; ++t) {
    const int e = t * 64 + g.lane;
    const int64_t nd = g.node(e), ch = g.chain(e);
    double v = (WHICH == COMB_DIAG) ? 1.0 : 0.0;
    const int64_t lim = (WHICH == COMB_OFF) ? n - 1 : n;
    if (nd < lim) {
      v = 0.0;
      _Pragma("unroll") for (int k = 0; k < OMC_MAX_TERMS; ++k) if (k < nt) {
        const double* src = (WHICH == COMB_DIAG) ? A.T.diag[k] : (WHICH == COMB_OFF ? A.T.off[k] : A.T.rhs[k]);
        if (!src && WHICH != COMB_DIAG) continue;
        const double sk = MULTI ? sc[k] : ((A.T.scale[k] && ch < A.C) ? A.T.scale[k][ch] : 1.0);
        v = fma(sk, src ? src[nd] : 1.0, v);
      }
      if (WHICH == COMB_RHS && A.rhs_chain && ch < A.C) v += A.rhs_chain[ch * A.ld_rhs + nd];
    }
    tile[e + e / M] = v;
  }
  wave_lds_fence();
}

// Workgroup-per-chain form of the tile traffic.  A wave's tile is 64 rows (segments) of M nodes at row
// stride M+1.  In the coalesced mapping step t moves tile elements e = 64 t + lane (node wbase + e: one
// aligned 512-byte request per wave and step); element e lives at tile[e + e/M].  With 64 t = M A_t + B_t
// (compile-time) and lane = M q0 + r0:  e/M = A_t + q0 + (r0 >= M - B_t), so the address is a lane-only
// base (lane + q0), an immediate (64 t + A_t) and a one-bit carry: a compare and a select per element instead
// of running index arithmetic on the vector ALU (the kernel is bound by VALU issue).
template <int M>
struct TileMap {
  static constexpr int LU = 64;                 // lanes in use
  static constexpr int NS = M;                  // steps per tile
  static constexpr int CH = (M % 5 == 0) ? 5 : 4;  // steps per batch of loads (memory-level parallelism vs registers)
  __device__ static __forceinline__ int lane_base(int lane) { return lane + lane / M; }
  __device__ static __forceinline__ int lane_col(int lane) { return lane % M; }
  __device__ static constexpr int upto(int t) { return 64 * t; }  // elements of steps [0, t)
  // tile element of step t; tl = tile + lane_base, r0 = lane_col
  template <class P>
  __device__ static __forceinline__ P* elem(P* tl, int r0, int t) {
    const int At = (64 * t) / M, Bt = (64 * t) % M;
    P* p = tl + (64 * t + At);
    return (Bt != 0 && r0 >= M - Bt) ? p + 1 : p;
  }
  // its successor in node order: the next column, or column 0 of the next row
  template <class P>
  __device__ static __forceinline__ P* succ(P* p, int r0, int t) {
    const int Bt = (64 * t) % M;
    return (r0 == M - 1 - Bt) ? p + 2 : p + 1;
  }
};

// number of this wave's tile elements that lie below `lim` (wave-uniform)
template <int M>
__device__ __forceinline__ int wave_valid(int wave_u, int lim) {
  const int v = lim - wave_u * 64 * M;
  return v < 0 ? 0 : (v > 64 * M ? 64 * M : v);
}

// Right-hand-side part of the terms with a per-chain centre (omc_tridiag_terms::center_chain): v_i += s_k (M_k c_k)_i with
// c_k the chain's vector, in the coalesced mapping -- three predicated loads of c per node (the shifted ones come out of
// the cache lines the first one brought), nothing staged.  Wave-uniform skip when no term has one.
template <int M, int CH>
__device__ __forceinline__ void rhs_center_chain(double (&v)[CH], const TriArgs& A, const double (&sc)[OMC_MAX_TERMS], bool chain_ok,
                                                 int64_t cc, int wbase, int lane, int t0, int cnt, int nvalid) {
  if (!A.cc.v || !chain_ok) return;  // wave-uniform
  const int n = (int)A.n, kc = A.cc.k;
  const double* c = A.cc.v + cc * A.cc.ld + wbase;
  // the term's vectors and scale by wave-uniform selects (a dynamic index into the kernel arguments would cost a private copy)
  const double* dk = kc == 0 ? A.T.diag[0] : (kc == 1 ? A.T.diag[1] : (kc == 2 ? A.T.diag[2] : A.T.diag[3]));
  const double* ok = kc == 0 ? A.T.off[0] : (kc == 1 ? A.T.off[1] : (kc == 2 ? A.T.off[2] : A.T.off[3]));
  const double sk = kc == 0 ? sc[0] : (kc == 1 ? sc[1] : (kc == 2 ? sc[2] : sc[3]));
  // (plain predicated loads, element by element: batching them -- all loads of the batch first, at clamped positions -- was
  // no faster and cost the generic instantiation 100 bytes of scratch per lane)
#pragma unroll
  for (int t = 0; t < CH; ++t) {
    if (t >= cnt) continue;
    const int idx = lane + (t0 + t) * 64, i = wbase + idx;
    if (idx >= nvalid) continue;
    double r = (dk ? (dk + wbase)[(unsigned)idx] : 1.0) * c[(unsigned)idx];
    if (ok) {
      if (i > 0) r = fma((ok + wbase)[idx - 1], c[idx - 1], r);
      if (i + 1 < n) r = fma((ok + wbase)[(unsigned)idx], c[(unsigned)idx + 1u], r);
    }
    v[t] = fma(sk, r, v[t]);
  }
}

// Per-chain combination of the shared term vectors, formed while the tile is filled.  All loads of a
// batch are issued back to back (L2 latency is paid once per batch) and only then combined.  A batch
// that lies wholly inside the vector takes the test-free path; the chain's last wave takes the
// predicated one for its boundary batch and only writes fill values beyond it.
struct omc_no_work { __device__ __forceinline__ void operator()(int) const {} };
// `under_loads(b)`: work that depends on nothing, run once per batch b while that batch's first loads are in flight
template <int M, int WHICH, bool CCH = false, class F = omc_no_work>
__device__ __forceinline__ void tile_fill_comb_wg(double* tile, int lane, int wave, int lbase, const TriArgs& A,
                                                  const double (&sc)[OMC_MAX_TERMS], bool chain_ok, int64_t cc,
                                                  F under_loads = F()) {
  constexpr bool OVL = !__is_same(F, omc_no_work);
  using TM = TileMap<M>;
  constexpr int CH = TM::CH;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int nt = A.T.n_terms;
  const int n = (int)A.n;
  const int wbase = wave_u * 64 * M;
  const int nvalid = wave_valid<M>(wave_u, (WHICH == COMB_OFF) ? n - 1 : n);
  const double* rc = (WHICH == COMB_RHS && A.rhs_chain && chain_ok) ? A.rhs_chain + cc * A.ld_rhs + wbase : nullptr;
  const double fillv = (WHICH == COMB_DIAG) ? 1.0 : 0.0;
  double* tl = tile + lbase;
  const int r0 = TM::lane_col(lane);
  wave_lds_fence();
  {
#pragma unroll
    for (int t0 = 0; t0 < TM::NS; t0 += CH) {
      const int cnt = (TM::NS - t0 < CH) ? TM::NS - t0 : CH;
      double v[CH];
#pragma unroll
      for (int t = 0; t < CH; ++t) v[t] = 0.0;
      if (TM::upto(t0 + cnt) <= nvalid) {  // wave-uniform: the whole batch is inside
        // With work to overlap (OVL): the loads of the first two terms, then the work that depends on nothing, then their
        // combination; further terms one by one.  Without: every term loads and combines in turn (fewest registers).
        constexpr int KF = OVL ? 2 : 0;
        double ldf[KF > 0 ? KF : 1][CH];
        if constexpr (OVL) {
#pragma unroll
          for (int k = 0; k < KF; ++k) {
            if (k >= nt) continue;
            const double* src = (WHICH == COMB_DIAG) ? A.T.diag[k] : (WHICH == COMB_OFF ? A.T.off[k] : A.T.rhs[k]);
            if (!src) continue;
            const double* ps = src + wbase;
#pragma unroll
            for (int t = 0; t < CH; ++t)
              if (t < cnt) ldf[k][t] = ps[(unsigned)(lane + (t0 + t) * TM::LU)];
          }
          __builtin_amdgcn_sched_barrier(0);
          under_loads(t0 / CH);
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int k = 0; k < OMC_MAX_TERMS; ++k) {
          if (k >= nt) continue;
          const double* src = (WHICH == COMB_DIAG) ? A.T.diag[k] : (WHICH == COMB_OFF ? A.T.off[k] : A.T.rhs[k]);
          if (!src) {
            if (WHICH == COMB_DIAG) {
#pragma unroll
              for (int t = 0; t < CH; ++t) v[t] += sc[k];
            }
            continue;
          }
          if (k < KF) {
#pragma unroll
            for (int t = 0; t < CH; ++t)
              if (t < cnt) v[t] = fma(sc[k], ldf[k < KF ? k : 0][t], v[t]);
          } else {
            const double* ps = src + wbase;
            double ld[CH];
#pragma unroll
            for (int t = 0; t < CH; ++t)
              if (t < cnt) ld[t] = ps[(unsigned)(lane + (t0 + t) * TM::LU)];
#pragma unroll
            for (int t = 0; t < CH; ++t)
              if (t < cnt) v[t] = fma(sc[k], ld[t], v[t]);
          }
        }
        if (WHICH == COMB_RHS && rc) {
          double ld[CH];
#pragma unroll
          for (int t = 0; t < CH; ++t)
            if (t < cnt) ld[t] = rc[(unsigned)(lane + (t0 + t) * TM::LU)];
#pragma unroll
          for (int t = 0; t < CH; ++t)
            if (t < cnt) v[t] += ld[t];
        }
        if (WHICH == COMB_RHS && CCH) rhs_center_chain<M, CH>(v, A, sc, chain_ok, cc, wbase, lane, t0, cnt, nvalid);
#pragma unroll
        for (int t = 0; t < CH; ++t)
          if (t < cnt) *TM::elem(tl, r0, t0 + t) = v[t];
      } else {
        if constexpr (OVL) under_loads(t0 / CH);
#pragma unroll
        for (int k = 0; k < OMC_MAX_TERMS; ++k) {
          if (k >= nt) continue;
          const double* src = (WHICH == COMB_DIAG) ? A.T.diag[k] : (WHICH == COMB_OFF ? A.T.off[k] : A.T.rhs[k]);
          if (!src) {
            if (WHICH == COMB_DIAG) {
#pragma unroll
              for (int t = 0; t < CH; ++t) v[t] += sc[k];
            }
            continue;
          }
          const double* ps = src + wbase;
#pragma unroll
          for (int t = 0; t < CH; ++t) {
            const int idx = lane + (t0 + t) * TM::LU;
            if (t < cnt && idx < nvalid) v[t] = fma(sc[k], ps[(unsigned)idx], v[t]);
          }
        }
#pragma unroll
        for (int t = 0; t < CH; ++t) {
          const int idx = lane + (t0 + t) * TM::LU;
          if (t >= cnt) continue;
          if (WHICH == COMB_RHS && rc && idx < nvalid) v[t] += rc[(unsigned)idx];
        }
        if (WHICH == COMB_RHS && CCH) rhs_center_chain<M, CH>(v, A, sc, chain_ok, cc, wbase, lane, t0, cnt, nvalid);
#pragma unroll
        for (int t = 0; t < CH; ++t) {
          const int idx = lane + (t0 + t) * TM::LU;
          if (t >= cnt) continue;
          if (idx < 64 * M) *TM::elem(tl, r0, t0 + t) = (idx < nvalid) ? v[t] : fillv;
        }
      }
      __builtin_amdgcn_sched_barrier(0);  // keep the next batch's loads from being hoisted over this one
    }
  }
  wave_lds_fence();
}


// One coalesced vector of a wave straight into registers: element t of lane l is node 64 t + l of the wave's slice (zero beyond
// nvalid).
template <int M, bool FULLW>
__device__ __forceinline__ void coal_load(double (&v)[M], const double* base, int lane, int nvalid) {
#pragma unroll
  for (int t = 0; t < M; ++t) {
    const int idx = lane + 64 * t;
    v[t] = (FULLW || idx < nvalid) ? base[(unsigned)idx] : 0.0;
  }
}
template <int M>
__device__ __forceinline__ void coal_load(double (&v)[M], const double* base, int lane, int nvalid) {
  if (nvalid == 64 * M) coal_load<M, true>(v, base, lane, nvalid);
  else coal_load<M, false>(v, base, lane, nvalid);
}
// One pair of draws (Philox block `block` of the chain, Box-Muller) with the M loads of a coalesced vector
// issued one per Philox round: the loads drain while the wave computes (issued back to back in front of
// the arithmetic they also overlap, but less: a wave blocks at issue once the CU's vector-memory queue is
// full).
template <int M, bool FULLW>
__device__ __forceinline__ void draws_over_load(const omc_rng_key& key, int64_t gc, uint32_t block, double& z0, double& z1,
                                                double (&v)[M], const double* base, int lane, int nvalid) {
  constexpr int LPR = (M + 9) / 10;  // loads per round
  uint32_t c0 = block, c1 = key.c1, c2 = (uint32_t)gc;
  uint32_t c3 = key.c3_base | ((uint32_t)((uint64_t)gc >> 32) & 0xffu) << 16;
  uint32_t k0 = key.k0, k1 = key.k1;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
#pragma unroll
    for (int q = 0; q < LPR; ++q) {
      const int t = r * LPR + q;
      if (t < M) {
        const int idx = lane + 64 * t;
        v[t] = (FULLW || idx < nvalid) ? base[(unsigned)idx] : 0.0;
      }
    }
    omc_philox_round_r(r, c0, c1, c2, c3, k0, k1);
    __builtin_amdgcn_sched_barrier(0);
  }
  omc_normal_pair(make_uint4(c0, c1, c2, c3), z0, z1);
}

// Quadratic forms (x - m_k)' M_k (x - m_k) of one wave's 64*M nodes in the coalesced mapping: x comes
// back from the tile (x_{i+1} = the next tile element; the slot behind the tile's last row holds the
// first x of the next wave), the shared vectors straight from L2.
template <int M>
__device__ __forceinline__ void quad_wg(const double* tile, int lane, int wave_u, int lbase, const TriArgs& A,
                                        double (&acc)[OMC_MAX_TERMS], int64_t cc) {
  using TM = TileMap<M>;
  constexpr int CH = TM::CH;
  const int nt = A.T.n_terms, n32 = (int)A.n;
  const int wbase = wave_u * 64 * M;
  const int nrem = n32 - wbase;  // nodes of the chain from this wave's first one on (may exceed the tile)
  const int nvalid = nrem < 64 * M ? (nrem < 0 ? 0 : nrem) : 64 * M;
  const double* tl = tile + lbase;
  const int r0 = TM::lane_col(lane);
  {
#pragma unroll
    for (int t0 = 0; t0 < TM::NS; t0 += CH) {
      const int cnt = (TM::NS - t0 < CH) ? TM::NS - t0 : CH;
      double xv[CH], xn[CH];  // x_i and x_{i+1}
      if (TM::upto(t0 + cnt) < nrem) {  // wave-uniform: i + 1 < n for every node of the batch
#pragma unroll
        for (int t = 0; t < CH; ++t)
          if (t < cnt) {
            xv[t] = *TM::elem(tl, r0, t0 + t);
            xn[t] = *TM::succ(TM::elem(tl, r0, t0 + t), r0, t0 + t);
          }
#pragma unroll
        for (int k = 0; k < OMC_MAX_TERMS; ++k) {
          if (k >= nt || ((A.cc.quad_skip >> k) & 1)) continue;  // (wave-uniform)
          const double *ck = A.T.center[k], *dk = A.T.diag[k], *ok = A.T.off[k];
          const double* cck = (A.cc.v && A.cc.k == k) ? A.cc.v + cc * A.cc.ld : nullptr;
          double ri[CH], rn[CH], dv[CH], ov[CH];
#pragma unroll
          for (int t = 0; t < CH; ++t) {
            if (t >= cnt) continue;
            const unsigned off = (unsigned)(lane + (t0 + t) * TM::LU);
            ri[t] = ck ? (ck + wbase)[off] : 0.0;
            rn[t] = (ck && ok) ? (ck + wbase)[off + 1u] : 0.0;
            if (cck) {  // per-chain part of the centre
              ri[t] += (cck + wbase)[off];
              if (ok) rn[t] += (cck + wbase)[off + 1u];
            }
            dv[t] = dk ? (dk + wbase)[off] : 1.0;
            ov[t] = ok ? (ok + wbase)[off] : 0.0;
          }
          if (ok) {
#pragma unroll
            for (int t = 0; t < CH; ++t) {
              if (t >= cnt) continue;
              const double a = xv[t] - ri[t], bnx = xn[t] - rn[t];
              acc[k] = fma(fma(2.0 * ov[t], bnx, dv[t] * a), a, acc[k]);
            }
          } else {
#pragma unroll
            for (int t = 0; t < CH; ++t) {
              if (t >= cnt) continue;
              const double a = xv[t] - ri[t];
              acc[k] = fma(dv[t] * a, a, acc[k]);
            }
          }
        }
      } else if (t0 * TM::LU < nvalid) {  // the chain's boundary batch
#pragma unroll
        for (int t = 0; t < CH; ++t) {
          if (t >= cnt) continue;
          const int idx = lane + (t0 + t) * TM::LU;
          const bool in = idx < nvalid, in1 = in && idx + 1 < nrem;
          const double x0 = in ? *TM::elem(tl, r0, t0 + t) : 0.0, x1 = in1 ? *TM::succ(TM::elem(tl, r0, t0 + t), r0, t0 + t) : 0.0;
#pragma unroll
          for (int k = 0; k < OMC_MAX_TERMS; ++k) {
            if (k >= nt || ((A.cc.quad_skip >> k) & 1)) continue;
            const double *ck = A.T.center[k], *dk = A.T.diag[k], *ok = A.T.off[k];
            const double* cck = (A.cc.v && A.cc.k == k) ? A.cc.v + cc * A.cc.ld : nullptr;
            const double a = x0 - ((ck && in) ? (ck + wbase)[(unsigned)idx] : 0.0) - ((cck && in) ? (cck + wbase)[(unsigned)idx] : 0.0);
            const double bnx = x1 - ((ck && ok && in1) ? (ck + wbase)[(unsigned)idx + 1u] : 0.0)
                                  - ((cck && ok && in1) ? (cck + wbase)[(unsigned)idx + 1u] : 0.0);
            const double d = in ? (dk ? (dk + wbase)[(unsigned)idx] : 1.0) : 0.0;
            const double o = (ok && in1) ? (ok + wbase)[(unsigned)idx] : 0.0;
            acc[k] = fma(fma(2.0 * o, bnx, d * a), a, acc[k]);
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}
