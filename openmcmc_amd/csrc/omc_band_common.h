// What the band kernels of omc_band.hip and omc_bandwide.hip share: the terms of the precision as a kernel argument, its entries,
// and -- host arithmetic only, so that tests/native/band_layout_host.hip can enumerate it without a GPU -- the LDS images of the
// blocked kernel and the choice among its instantiations.  Not part of the ABI.
#pragma once
#include "omc_common.h"

struct BandTermsDev {
  int n_terms;
  const double* band[OMC_MAX_TERMS];  // [ (bw+1) x n ], band[d*n + i] = M[i+d, i]; NULL = identity
  int bw[OMC_MAX_TERMS];
  const double* rhs[OMC_MAX_TERMS];
  const double* scale[OMC_MAX_TERMS];
};

__device__ __forceinline__ double band_entry(const BandTermsDev& T, const double* s, int64_t n, int64_t col, int d) {
  // Q[col + d, col]; d >= 0, so the test covers col >= n as well
  if (col + d >= n) return 0.0;
  double v = 0.0;
#pragma unroll
  for (int k = 0; k < OMC_MAX_TERMS; ++k) {
    if (k < T.n_terms) {
      if (T.band[k]) {
        if (d <= T.bw[k]) v = fma(s[k], T.band[k][(int64_t)d * n + col], v);
      } else if (d == 0) {
        v += s[k];
      }
    }
  }
  return v;
}

__device__ __forceinline__ double band_rhs(const BandTermsDev& T, const double* s, int64_t n, int64_t col, const double* rc) {
  if (col >= n) return 0.0;
  double b = rc ? rc[col] : 0.0;
#pragma unroll
  for (int k = 0; k < OMC_MAX_TERMS; ++k)
    if (k < T.n_terms && T.rhs[k]) b = fma(s[k], T.rhs[k][col], b);
  return b;
}

// omc_bandwide.hip.  Lws: [C][n][w + 1] doubles.  Returns false if no form fits (the caller then takes k_band_sample).
bool omc_band_blocked_launch(omc_ctx* ctx, int64_t n, int w, const BandTermsDev& T, const double* rhs_chain, int64_t ld_rhs,
                             const double* z_inject, int64_t ld_z, omc_rng_key key, double* Lws, double* x, int64_t ld_x, double* mean,
                             int64_t ld_mean, double* logdet);

// ---- k_band_blocked<NB, NT>: its two LDS images at bandwidth w, offsets in doubles from the start of the allocation.  The kernel
// takes every pointer and offset from here and the host the size it launches with; tests/test_band_layout_host.py holds each region
// to what the kernel indexes.
struct BandBlockedLds {
  enum { FAIL = 0, ZERO = 1, DUMP = 2, COUNTER = 66, MISC_SLOTS = 68 };  // misc: a pivot was not positive, a zero to read, a slot
                                                                         // per lane to write to in vain, the item counter (an int)
  // forward pass (factorisation): W1 = w + 1, WS ring slots, WP panel rows (whole tiles), PS panel row stride
  int W1 = 0, WS = 0, WP = 0, PS = 0;
  int ring = 0;    // WS x W1: ring[slot(col) * W1 + d] = open entry Q[col + d, col]
  int rring = 0;   // WS: open right-hand side
  // a factorised block column, TWO copies (the block being applied and the one factorised ahead of it), FBS doubles apart:
  int Ld = 0;      // NB x PS: the diagonal block's factor (its strict lower triangle is what is read)
  int P = 0;       // WP x PS: the panel below it, right behind: row r of the block column = Ld[r * PS ..]
  int dv = 0;      // NB: 1 / L_jj of the block
  int Us = 0;      // NB: forward-substituted right-hand side of the block
  int FBS = 0, misc = 0, fwd_end = 0;
  // backward pass, laid over the same memory
  int WB = 0;      // slots of a solution ring: w + 2 NB, not w + NB (see the kernel)
  int xs = 0, ms = 0;  // WB each: the last solutions of the draw and of the mean, slot = column % WB
  int Sx = 0, Sm = 0;  // NB each: sum over the rows behind the block, per column
  int Lb = 0;      // NB x PS: the block's own triangle of the factor
  int Part = 0;    // [2][2][NB][QPC]: the far sums of the quads, for blocks of even and odd number, draw and mean
  int dump = 0;    // 64: a slot per lane to write to in vain
  int diag = 0;    // NB: the block's 1 / L_jj
  int bwd_end = 0;
  __host__ __device__ constexpr BandBlockedLds(int w, int NB, int NT) {
    W1 = w + 1; WS = w + NB; WP = (w + 15) & ~15; PS = NB + 1;
    rring = ring + WS * W1; Ld = rring + WS; P = Ld + NB * PS; dv = P + WP * PS; Us = dv + NB;
    FBS = Us + NB - Ld; misc = Ld + 2 * FBS; fwd_end = misc + MISC_SLOTS;
    WB = w + 2 * NB;
    ms = xs + WB; Sx = ms + WB; Sm = Sx + NB; Lb = Sm + NB; Part = Lb + NB * PS;
    dump = Part + 4 * NB * ((NT - 64) / NB / 4); diag = dump + 64; bwd_end = diag + NB;
  }
  __host__ __device__ constexpr size_t bytes() const { return (size_t)(fwd_end > bwd_end ? fwd_end : bwd_end) * sizeof(double); }
};

// ---- the instantiations of k_band_blocked and which of them a draw takes
#define BAND_BLOCKED_FORMS(X) /* (NB, NT, MT, WPE) */ \
  X(16, 256, 2, 4) X(16, 256, 2, 1) X(16, 256, OMC_MAX_TERMS, 1) X(8, 256, 2, 4) X(8, 512, 2, 4) X(16, 512, 2, 1) \
  X(16, 512, OMC_MAX_TERMS, 1) X(8, 512, 2, 1) X(8, 512, OMC_MAX_TERMS, 1)
#define BAND_WMAX_W 128
#define BAND_W16_MAX 115                 // 16 columns per step and eight waves up to here: beyond, the window does not fit the LDS
#define BAND_LDS_LIMIT (160 * 1024)
static_assert(BandBlockedLds(BAND_W16_MAX, 16, 512).bytes() <= BAND_LDS_LIMIT && BandBlockedLds(BAND_W16_MAX + 1, 16, 512).bytes() > BAND_LDS_LIMIT,
              "BAND_W16_MAX is where the 16-column image stops fitting");
struct BandBlockedForm {
  int NB, NT, MT, WPE;  // columns per step, threads, terms compiled for, waves per SIMD the registers leave room for; NB == 0: none
  // the widest band the form is launched for (it sizes the kernel's per-thread arrays; the four-wave forms: bands narrower than a
  // block, or four tiles a side) and the workgroups a CU is meant to hold (its LDS must take that many images)
  __host__ __device__ constexpr int wmax() const { return NT == 256 ? (NB == 16 ? 15 : 64) : (NB == 16 ? BAND_W16_MAX : BAND_WMAX_W); }
  __host__ __device__ constexpr int wgs_per_cu() const { return WPE == 4 ? 1024 / NT : (NT == 256 ? 3 : 1); }
  constexpr bool fits(int w) const { return w <= wmax() && (size_t)wgs_per_cu() * BandBlockedLds(w, NB, NT).bytes() <= BAND_LDS_LIMIT; }
  constexpr int key() const { return ((NB * 1024 + NT) * 8 + MT) * 8 + WPE; }
};
// Which form, by what fits a CU (measured on 10 000-node lattices, profiles/r04q_band.txt):
//  * bands narrower than a block take four waves per chain (one tile, one factorising wave); with more chains than three
//    workgroups per CU hold, the form compiled for 128 registers puts four there (1024 chains at w = 8: 8.0 -> 4.6 ms);
//  * bands up to ~64 on more chains than CUs: 8 columns per step at 128 registers -- four waves per chain and four workgroups
//    to a CU while their LDS fits (w <= 55: 1024 chains at w = 32 15.6 -> 6.2 ms, at w = 16 15.6 -> 5.6 ms), eight waves and
//    two to a CU beyond (w = 64: 16.4 -> 14.6 ms); slower where one workgroup per CU is all there is (3.9 -> 4.9 ms at 256
//    chains);
//  * otherwise 16 columns per step, eight waves, one workgroup per CU (8 columns where the window would not fit the LDS).
// forced ("band_blocked_threads"): 0 this choice; 512 eight waves and no register limit whatever the shape; 4 / 16 / 8 the
// 128-register forms wherever they apply (A/B runs and tests).  Only the forms compiled for two terms have the 128-register variants.
inline BandBlockedForm band_blocked_choose(int w, int n_terms, int64_t n_chains, int cus, int forced) {
  if (w < 1 || w > BAND_WMAX_W) return {0, 0, 0, 0};
  const bool few = n_terms <= 2;
  const int MT = few ? 2 : OMC_MAX_TERMS;
  if (w <= 15 && forced != 512 && forced != 8)
    return {16, 256, MT, (few && (forced == 4 || (forced == 0 && n_chains > 3 * (int64_t)cus))) ? 4 : 1};
  const bool many = forced == 0 && n_chains > (int64_t)cus;
  const BandBlockedForm four{8, 256, 2, 4}, two{8, 512, 2, 4}, wide{16, 512, MT, 1}, tall{8, 512, MT, 1};
  if (few && (forced == 16 || many) && four.fits(w)) return four;
  if (few && (forced == 8 || many) && two.fits(w)) return two;
  return wide.fits(w) ? wide : tall.fits(w) ? tall : BandBlockedForm{0, 0, 0, 0};
}
