// Scan machinery of k_tridiag_seg (omc_tridiag.hip): the Moebius and affine scan elements, exclusive scans over a sub-wave
// group (shuffles) and over a workgroup (DPP lane shifts, one LDS barrier), neighbour exchange, reductions, the LDS-only barrier.
#pragma once
#include "omc_common.h"

// ------------------------------------------------------------------------------------------
// segmented kernel: scan machinery
struct Mob { double a, b, c, d; };  // 2x2 matrix [[a,b],[c,d]] acting as D -> (aD+b)/(cD+d)
struct Aff { double p, q; };        // v -> p + q v

// later-after-earlier composition.  The Moebius product is left unscaled: a product of k matrices whose
// largest entries lie in [1, 2) has entries below 2^(2k-1) -- below 2^(k (s + 1) - 1) for entries below 2^s --, so the
// scans rescale (`renorm`, an exact power of two: the map is unchanged) once per 16-lane row pass, not once per product.
__device__ __forceinline__ Mob compose(const Mob& L, const Mob& E) {
  return Mob{fma(L.a, E.a, L.b * E.c), fma(L.a, E.b, L.b * E.d), fma(L.c, E.a, L.d * E.c), fma(L.c, E.b, L.d * E.d)};
}
__device__ __forceinline__ Aff compose(const Aff& L, const Aff& E) { return Aff{fma(L.q, E.p, L.p), L.q * E.q}; }
// The scans' rescaling: by the exponent of the LEADING entry alone (v_frexp_exp, a negation, four v_ldexp: 6 instructions in a
// dependent chain of three, against 15 in a chain of eight for the maximum over four entries, ilogb and four multiplies it
// replaces; the scan sits between two barriers, where every wave pays the chain's latency).  Any exact power of two serves:
// it cancels in (a D + b)/(c D + d), and fma and multiply commute with it, so the choice changes no bit of a start value as
// long as nothing leaves the normal range.
// The guard is the instruction's own: v_frexp_exp_i32_f64 returns 0 for an input that is 0, infinite or NaN, so such a
// matrix is left alone (ldexp by 0) -- the guard inside the local product (k_tridiag_seg) relies on the same.  A
// compare and a select in front of it were measured: 0.36 us per sweep of the headline for four instructions (A/B in
// profiles/r09_ab_headline.txt).
// Why the leading entry will do.  For a stretch of a positive definite chain with pivots D (started from an infinite
// incoming pivot) and D' (the same stretch without its first node), couplings b0 into it:
//   a = prod D,  c = a / D_last,  b = -b0^2 prod D',  d = b / D'_last,
// so every entry lies within 2^s of a, s = log2 of the largest of D, 1/D, b0^2/D, b0^2/(D D') over the chain (31 for a
// precision scale of 1e9 against a unit identity term, 54 for 1e-8: there a ~ 1, b ~ 1e-16); a is positive and never the
// small difference of large terms.  Rescaled: a in [1/2, 1), every entry below 2^s.
// A product of two rescaled factors has the leading entry a_L a_E (1 - b^2/(D D')) with the pivots on either side of the
// join: smaller than a_L a_E by up to 2^-sigma, sigma <= 53 (about log2 sqrt(lambda/tau) + 1 on the random-walk smoother:
// 16 at 1e9) -- that factor per product is what underflowed unscaled products of wave totals at lambda >= 1e6.
__device__ __forceinline__ Mob mob_rescale(const Mob& m) {
  const int ex = -__builtin_amdgcn_frexp_exp(m.a);
  return Mob{ldexp(m.a, ex), ldexp(m.b, ex), ldexp(m.c, ex), ldexp(m.d, ex)};
}
__device__ __forceinline__ Mob renorm(const Mob& m) { return mob_rescale(m); }
__device__ __forceinline__ Aff renorm(const Aff& f) { return f; }

__device__ __forceinline__ Mob shfl(const Mob& v, int d, int w, bool rev) {
  return rev ? Mob{__shfl_down(v.a, d, w), __shfl_down(v.b, d, w), __shfl_down(v.c, d, w), __shfl_down(v.d, d, w)}
             : Mob{__shfl_up(v.a, d, w), __shfl_up(v.b, d, w), __shfl_up(v.c, d, w), __shfl_up(v.d, d, w)};
}
__device__ __forceinline__ Aff shfl(const Aff& v, int d, int w, bool rev) {
  return rev ? Aff{__shfl_down(v.p, d, w), __shfl_down(v.q, d, w)} : Aff{__shfl_up(v.p, d, w), __shfl_up(v.q, d, w)};
}

// Exclusive scan of `v` over the lanes of one chain, in segment order (or reverse order).
// Wd = lanes of this chain inside one wave (power of two); for MULTI the chain spans nw waves
// and `lds` (>= nw entries) carries the wave totals.  Every lane of the block must call it.
template <class T, bool MULTI>
__device__ __forceinline__ T excl_scan(T v, const T ident, int pos, int Wd, bool rev, T* lds, int wave, int nw) {
  const int p = rev ? (Wd - 1 - pos) : pos;  // rank in scan order inside the wave
  for (int d = 1; d < Wd; d <<= 1) {
    T o = shfl(v, d, Wd, rev);
    if (p >= d) v = compose(v, o);
    if (d & 0x2a) v = renorm(v);  // every other doubling step
  }
  v = renorm(v);
  T e = shfl(v, 1, Wd, rev);
  if (p == 0) e = ident;
  if (MULTI) {
    if (p == Wd - 1) lds[wave] = v;
    __syncthreads();
    T pre = ident;
    if (!rev) {
      for (int w = 0; w < wave; ++w) pre = renorm(compose(lds[w], pre));
    } else {
      for (int w = nw - 1; w > wave; --w) pre = renorm(compose(lds[w], pre));
    }
    e = compose(e, pre);
    __syncthreads();
  }
  return e;
}

// value held by the previous segment's lane (identity for the first segment)
template <bool MULTI>
__device__ __forceinline__ void prev_lane2(double& v0, double& v1, double id0, double id1, int pos, int Wd,
                                           double* lds, int wave) {
  double a = __shfl_up(v0, 1, Wd), b = __shfl_up(v1, 1, Wd);
  if (MULTI) {
    if (pos == Wd - 1) { lds[2 * wave] = v0; lds[2 * wave + 1] = v1; }
    __syncthreads();
    if (pos == 0 && wave > 0) { a = lds[2 * (wave - 1)]; b = lds[2 * (wave - 1) + 1]; }
    if (pos == 0 && wave == 0) { a = id0; b = id1; }
    __syncthreads();
  } else if (pos == 0) {
    a = id0; b = id1;
  }
  v0 = a; v1 = b;
}

template <bool MULTI>
__device__ __forceinline__ double group_sum(double v, int Wd, double* lds, int wave, int nw) {
  for (int d = Wd >> 1; d >= 1; d >>= 1) v += __shfl_xor(v, d, Wd);
  if (MULTI) {
    if ((threadIdx.x & 63) == 0) lds[wave] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < nw; ++w) t += lds[w];
    __syncthreads();
    v = t;
  }
  return v;
}

// ------------------------------------------------------------------------------------------
// Full-wave (64 lanes = 64 consecutive segments of one chain) scans on DPP lane shifts: a shift is
// one v_mov_dpp per 32-bit word instead of a ds_bpermute round trip.  Lanes without a source
// receive the identity, so no lane needs a conditional.
#define DPP_ROW_SHR(n) (0x110 + (n))
#define DPP_ROW_SHL(n) (0x100 + (n))
#define DPP_WAVE_SHL1 0x130
#define DPP_WAVE_SHR1 0x138

// `fill` is always a compile-time identity element (0.0 or 1.0) at the call sites: a word of it that is zero
// is produced by the instruction's own bound_ctrl zero fill instead of a preloaded destination register
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v, double fill) {
  const int flo = __double2loint(fill), fhi = __double2hiint(fill);
  int lo, hi;
  if (__builtin_constant_p(flo) && flo == 0) lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
  else lo = __builtin_amdgcn_update_dpp(flo, __double2loint(v), CTRL, 0xf, 0xf, false);
  if (__builtin_constant_p(fhi) && fhi == 0) hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
  else hi = __builtin_amdgcn_update_dpp(fhi, __double2hiint(v), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
template <int CTRL> __device__ __forceinline__ Mob dpp_mov(const Mob& v, const Mob& f) {
  return Mob{dpp_mov<CTRL>(v.a, f.a), dpp_mov<CTRL>(v.b, f.b), dpp_mov<CTRL>(v.c, f.c), dpp_mov<CTRL>(v.d, f.d)};
}
template <int CTRL> __device__ __forceinline__ Aff dpp_mov(const Aff& v, const Aff& f) {
  return Aff{dpp_mov<CTRL>(v.p, f.p), dpp_mov<CTRL>(v.q, f.q)};
}
// row_bcast15 / row_bcast31 (GFX9 DPP): the last lane of a row -> every lane of the next row / lane 31 -> rows 2
// and 3.  Rows not selected by ROW_MASK keep `fill` (the identity), so composing with the result is a no-op there.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_bcast(double v, double fill) {
  int lo = __builtin_amdgcn_update_dpp(__double2loint(fill), __double2loint(v), CTRL, ROW_MASK, 0xf, false);
  int hi = __builtin_amdgcn_update_dpp(__double2hiint(fill), __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
  return __hiloint2double(hi, lo);
}
template <int CTRL, int ROW_MASK> __device__ __forceinline__ Mob dpp_bcast(const Mob& v, const Mob& f) {
  return Mob{dpp_bcast<CTRL, ROW_MASK>(v.a, f.a), dpp_bcast<CTRL, ROW_MASK>(v.b, f.b), dpp_bcast<CTRL, ROW_MASK>(v.c, f.c),
             dpp_bcast<CTRL, ROW_MASK>(v.d, f.d)};
}
template <int CTRL, int ROW_MASK> __device__ __forceinline__ Aff dpp_bcast(const Aff& v, const Aff& f) {
  return Aff{dpp_bcast<CTRL, ROW_MASK>(v.p, f.p), dpp_bcast<CTRL, ROW_MASK>(v.q, f.q)};
}
__device__ __forceinline__ double read_lane(double v, int l) {  // l must be wave-uniform
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ Mob read_lane(const Mob& v, int l) {
  return Mob{read_lane(v.a, l), read_lane(v.b, l), read_lane(v.c, l), read_lane(v.d, l)};
}
__device__ __forceinline__ Aff read_lane(const Aff& v, int l) { return Aff{read_lane(v.p, l), read_lane(v.q, l)}; }

// inclusive scan inside each row of 16 lanes, forward (REV = false) or from the high lane down
// NORM: rescale the result (mob_rescale; the bounds in its terms s and sigma).  Inside the pass the fifteen products are left
// unscaled either way: leading entry above 2^-(16 + 15 sigma), entries below 2^s of it.
//   NORM = true, the row pass inside a wave: three more products follow inside the wave (two folds, the shift's exclusive
//     prefix) and sixteen wave totals meet in wave 0 -- 2^-(64 sigma) per wave if nothing were rescaled on the way.  Rescaled
//     here: a wave total's leading entry stays above 2^-(4 + 3 sigma).
//   NORM = false, wave 0's pass over the (rescaled) wave totals.  ONE product with a wave's exclusive prefix (above
//     2^-(4 + 3 sigma)), the product with the lane's own factor and the quotient that forms the start pivot follow: nothing
//     below 2^-(22 + 20 sigma + 2 s) -- 2^-450 at sigma = 16, s = 54; the pass itself goes as low as 2^-(16 + 15 sigma) with
//     or without a rescaling behind it -- and nothing above 2^(2 s + 1).  Left as it is.
template <class T, bool REV, bool NORM = true>
__device__ __forceinline__ T row_scan(T v, const T& id) {
  if (!REV) {
    v = compose(v, dpp_mov<DPP_ROW_SHR(1)>(v, id));
    v = compose(v, dpp_mov<DPP_ROW_SHR(2)>(v, id));
    v = compose(v, dpp_mov<DPP_ROW_SHR(4)>(v, id));
    v = compose(v, dpp_mov<DPP_ROW_SHR(8)>(v, id));
  } else {
    v = compose(v, dpp_mov<DPP_ROW_SHL(1)>(v, id));
    v = compose(v, dpp_mov<DPP_ROW_SHL(2)>(v, id));
    v = compose(v, dpp_mov<DPP_ROW_SHL(4)>(v, id));
    v = compose(v, dpp_mov<DPP_ROW_SHL(8)>(v, id));
  }
  return NORM ? renorm(v) : v;
}

// Workgroup barrier that orders LDS traffic only.  `__syncthreads()` is a fence as well: it waits for every
// outstanding vector-memory operation of the wave (vmcnt(0)) -- here that would be the 80 KB of x stores and the
// LDS-DMA transfers, which no other wave ever reads; the hand-overs of the scans and reductions go through LDS.
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Exclusive scan over all lanes of the workgroup (one chain), in segment order or reversed.
// `lds` holds one entry per wave.  Every lane of the block must call it.
// ONE_WAVE: the scan over the wave totals is done by wave 0 alone and handed out through `lds2` behind a second
// barrier, instead of redundantly by every wave -- worth it for the Moebius elements, whose 16-lane row scan
// is ~140 vector-ALU instructions per wave (x 16 waves on 4 SIMDs) against a few hundred cycles of one wave.
template <class T, bool REV, bool ONE_WAVE = false>
__device__ __forceinline__ T excl_scan_wg(T v, const T id, T* lds, int lane, int wave, int nw, T* lds2 = nullptr) {
  v = row_scan<T, REV>(v, id);
  // row totals sit in the last (first) lane of each row; fold the preceding rows in
  const int row = lane >> 4;
  if (!REV) {
    // the classic wave64 pattern: lane 15 -> row 1 and lane 47 -> row 3, then lane 31 -> rows 2 and 3
    v = compose(v, dpp_bcast<0x142, 0xA>(v, id));
    v = compose(v, dpp_bcast<0x143, 0xC>(v, id));
  } else {  // no mirrored broadcast exists: fold through readlanes
    const T t3 = read_lane(v, 48), t2 = read_lane(v, 32), t1 = read_lane(v, 16);
    const T p1 = compose(t2, t3), p0 = compose(t1, p1);
    const T pre = row == 2 ? t3 : (row == 1 ? p1 : (row == 0 ? p0 : id));
    v = compose(v, pre);
  }
  T e = REV ? dpp_mov<DPP_WAVE_SHL1>(v, id) : dpp_mov<DPP_WAVE_SHR1>(v, id);
  if (nw > 1) {
    if (lane == (REV ? 0 : 63)) lds[wave] = v;  // wave total
    lds_barrier();
    const int w = __builtin_amdgcn_readfirstlane(wave);
    const int src = REV ? w + 1 : w - 1;
    if (ONE_WAVE) {
      if (w == 0) {
        // The wave totals arrive unscaled from two folds; products of Moebius matrices of a precision of magnitude
        // lambda shrink by ~1/lambda per factor, so sixteen of them in a row underflowed for lambda >= 1e6 on chains of
        // twelve and more waves (0/0 start values).  Rescaled here, the row pass sees leading entries in [1/2, 1) like the
        // one inside a wave (a wave total is a product of four rescaled rows: leading entry above 2^-(4 + 3 sigma)); its own
        // result needs no rescaling any more (row_scan, NORM = false).
        T t = (lane < nw) ? renorm(lds[lane]) : id;
        t = row_scan<T, REV, false>(t, id);
        if (lane < nw) lds2[lane] = t;
      }
      lds_barrier();
      if (src >= 0 && src < nw) e = compose(e, lds2[src]);
    } else {
      T t = (lane < nw) ? lds[lane] : id;        // nw <= 16: one row
      t = row_scan<T, REV>(t, id);
      if (src >= 0 && src < nw) e = compose(e, read_lane(t, src));
    }
    // no trailing barrier: consecutive calls must use different `lds` buffers (the barrier of
    // the next call then orders this call's reads before the buffer is written again)
  }
  return e;
}

// previous segment's (v0, v1); (id0, id1) for the first segment of the chain
__device__ __forceinline__ void prev_lane2_wg(double& v0, double& v1, double id0, double id1, double* lds, int lane,
                                              int wave, int nw) {
  double a = dpp_mov<DPP_WAVE_SHR1>(v0, id0), b = dpp_mov<DPP_WAVE_SHR1>(v1, id1);
  if (nw > 1) {
    if (lane == 63) { lds[2 * wave] = v0; lds[2 * wave + 1] = v1; }
    lds_barrier();
    if (lane == 0 && wave > 0) { a = lds[2 * (wave - 1)]; b = lds[2 * (wave - 1) + 1]; }
    // no trailing barrier: see excl_scan_wg
  }
  v0 = a; v1 = b;
}

// sums of the first nt accumulators over the workgroup with a single barrier; lds: [4][16]
__device__ __forceinline__ void sum4_wg(const double (&v)[OMC_MAX_TERMS], double (&out)[OMC_MAX_TERMS], int nt, double* lds,
                                        int lane, int wave, int nw) {
  double t[OMC_MAX_TERMS] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < OMC_MAX_TERMS; ++k) {
    if (k >= nt) continue;  // wave-uniform
    double x = v[k];
    x += dpp_mov<DPP_ROW_SHR(1)>(x, 0.0);
    x += dpp_mov<DPP_ROW_SHR(2)>(x, 0.0);
    x += dpp_mov<DPP_ROW_SHR(4)>(x, 0.0);
    x += dpp_mov<DPP_ROW_SHR(8)>(x, 0.0);
    t[k] = (read_lane(x, 15) + read_lane(x, 31)) + (read_lane(x, 47) + read_lane(x, 63));
  }
  if (nw > 1) {
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < OMC_MAX_TERMS; ++k)
        if (k < nt) lds[k * 16 + wave] = t[k];
    }
    lds_barrier();
    // lane 16 k + w holds wave w's partial sum of term k; one row reduction serves all terms
    double x = ((lane & 15) < nw && (lane >> 4) < nt) ? lds[lane] : 0.0;
    x += dpp_mov<DPP_ROW_SHR(1)>(x, 0.0);
    x += dpp_mov<DPP_ROW_SHR(2)>(x, 0.0);
    x += dpp_mov<DPP_ROW_SHR(4)>(x, 0.0);
    x += dpp_mov<DPP_ROW_SHR(8)>(x, 0.0);
    t[0] = read_lane(x, 15); t[1] = read_lane(x, 31); t[2] = read_lane(x, 47); t[3] = read_lane(x, 63);
  }
#pragma unroll
  for (int k = 0; k < OMC_MAX_TERMS; ++k) out[k] = t[k];
}

__device__ __forceinline__ double sum_wg(double v, double* lds, int lane, int wave, int nw) {
  v += dpp_mov<DPP_ROW_SHR(1)>(v, 0.0);
  v += dpp_mov<DPP_ROW_SHR(2)>(v, 0.0);
  v += dpp_mov<DPP_ROW_SHR(4)>(v, 0.0);
  v += dpp_mov<DPP_ROW_SHR(8)>(v, 0.0);
  double t = (read_lane(v, 15) + read_lane(v, 31)) + (read_lane(v, 47) + read_lane(v, 63));
  if (nw > 1) {
    if (lane == 0) lds[wave] = t;
    lds_barrier();
    double u = 0.0;
    for (int w = 0; w < nw; ++w) u += lds[w];
    t = u;  // no trailing barrier: every call site owns its 16-entry slot of `lds`
  }
  return t;
}

// Workgroup-wide OR of a per-lane flag with ONE LDS barrier: every wave leaves its ballot in its own word of `slot`, all
// read the row behind the barrier.  (`__syncthreads_or` is a library reduction of three `s_barrier`s -- clear, `ds_or`,
// read -- and a full `__syncthreads` fence each; the join test sits on every chain-update's critical path.)  No trailing
// barrier: the next call on the same `slot` must lie behind another barrier.
__device__ __forceinline__ bool any_wg(int need, int* slot, int lane, int wave, int nw) {
  const bool mine = __ballot(need) != 0ull;
  if (nw <= 1) return mine;
  if (lane == 0) slot[wave] = mine ? 1 : 0;
  lds_barrier();
  const int f = (lane < nw) ? slot[lane] : 0;
  return __ballot(f) != 0ull;
}
