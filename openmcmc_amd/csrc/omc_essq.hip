// The effective sample size of indicator series of the device-resident store -- ArviZ's ess(method="quantile" / "local") -- and
// order statistics at given positions, without moving the store off the GPU.  The contract is in include/omcmc_hip.h
// (omc_store_ess_indicator, omc_store_order_stats).
//
// store is [N][C][size]; every chain is split as omc_store_rhat_ess splits it: M = N / 2, J = 2 C series, S = J M split draws per
// element.  An indicator series is ONE BIT per draw, 64 draws per word, and every sum Geyer's sequence needs from it is an exact
// integer.  With b_j[0..M) the 0/1 series of one (element, interval):
//   n_j = sum_s b_j[s],  Nn = sum_j n_j,  Q = sum_j n_j^2,
//   A(t) = sum_j sum_{s < M - t} b_j[s] b_j[s + t]                      = sum of popcount(w & (w >> t)) over the words,
//   H(t) = sum_j n_j (sum_{s < M - t} b_j[s] + sum_{s >= t} b_j[s])     = 2 Q - sum_j n_j (ones among the first t + the last t draws),
//   Z(t) = M^2 A(t) - M H(t) + (M - t) Q                                = M^2 times the centred lag sum of omc_store_rhat_ess,
//   S(t) = (double)Z(t) / (M M),  B_M = (double)(J Q - Nn^2) / (M M J (J - 1)),
// and from there the rule of omc_geyer.h, the one omc_store_rhat_ess follows.  Nothing is rounded before the conversion of Z, so
// nothing depends on the order in which lanes, waves or chunks add: repeated calls, any "rank_tile", any "rank_chunk" and both
// forms of the lag kernel give the same bits.  No floating-point atomics, no host round trip per block of lags.
//
// Per chunk of Kc selected elements:
//   rank_gather_sort   k_rank_gather with the split geometry and the key-only bitonic sort of every column (omc_store_shared.hip),
//   k_essq_thresholds  q_lo, q_hi of every interval from the sorted column, numpy's interpolation (q_lerp of omc_quantile.h; the
//                      ranks and the weight come from the host),
//   k_essq_pack        one read of the chunk's columns: a thread per (word of 64 draws, series, element), the elements on
//                      consecutive lanes (a row load is a contiguous run where idx is), 64 independent strided loads, then one word
//                      per interval into bits [Kc][n_p][J][Wd], Wd = ceil(M / 64): every series starts on its own word, the
//                      bits past M are zero,
//   k_essq_lags        one workgroup per (element, interval) walks its own Geyer sequence to the end, 64 lags at a time: lane r
//                      of every wave owns lag t = 64 q + r, the waves share out the words, and a word pair costs one funnel
//                      shift, one AND and one popcount per lane with no reduction across lanes.  The bits are staged in LDS where they fit (form 1),
//                      else read where they lie (form 2: the addresses are wave-uniform).
#include <math.h>

#include "omc_common.h"
#include "omc_geyer.h"
#include "omc_quantile.h"
#include "omc_rank_sort.h"
#include "omc_store_view.h"

namespace {

constexpr int EQ_MAXP = 32;                        // intervals per call
constexpr int EQ_NW = 4;                           // waves of k_essq_lags
constexpr size_t EQ_LDS_MAX = (size_t)144 * 1024;  // bits and series counts of the LDS form at most (160 KiB less the reductions)

// the two order statistics and the weight of np.quantile's "linear" interpolation for the ends of every interval (end 0: the lower
// one, r0 < 0 where there is none), worked out on the host
struct EssqProbs { int64_t r0[2][EQ_MAXP], r1[2][EQ_MAXP]; double fr[2][EQ_MAXP]; };

// q_ranks of omc_quantile.h on the host: virtual index (n - 1) q, its floor, the next index and the fraction, every operation
// rounded on its own as numpy rounds it (no fused multiply-add may stand in for the product and the subtraction)
void essq_ranks(int64_t nv, double q, int64_t& lo, int64_t& hi, double& frac) {
#pragma clang fp contract(off)
  const volatile double h = (double)(nv - 1) * q;
  lo = (int64_t)floor(h);
  if (lo < 0) lo = 0;
  if (lo > nv - 1) lo = nv - 1;
  hi = lo + 1 < nv ? lo + 1 : nv - 1;
  if (h >= (double)(nv - 1)) lo = hi = nv - 1;
  frac = h < (double)(nv - 1) ? h - (double)lo : 0.0;
}

// One thread per element of the chunk: thr [Kc][n_p][2] = q_lo (NaN: no lower end), q_hi of every interval; q_out [n_p][n_idx][2]
__global__ void __launch_bounds__(64) k_essq_thresholds(int64_t Kc, int64_t k0, int64_t n_idx, int64_t P, int n_p, EssqProbs pr,
                                                        const uint64_t* __restrict__ keys, double* __restrict__ thr,
                                                        double* __restrict__ q_out) {
  const int64_t e = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (e >= Kc) return;
  const uint64_t* col = keys + e * P;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
  for (int p = 0; p < EQ_MAXP; ++p) {
    if (p < n_p) {
      double q[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const bool none = pr.r0[h][p] < 0;
        const double v = q_lerp(q_val(col[none ? 0 : pr.r0[h][p]]), q_val(col[none ? 0 : pr.r1[h][p]]), pr.fr[h][p]);
        q[h] = none ? nan : v;
      }
      thr[(e * n_p + p) * 2] = q[0];
      thr[(e * n_p + p) * 2 + 1] = q[1];
      if (q_out) {
        q_out[((int64_t)p * n_idx + k0 + e) * 2] = q[0];
        q_out[((int64_t)p * n_idx + k0 + e) * 2 + 1] = q[1];
      }
    }
  }
}

// One thread per (element e, word w, series j), e fastest: the 64 draws [64 w, 64 w + 64) of series j = 2 c + h of the element,
// loaded once, then bit i of the interval's word = (q_lo <= x_i && x_i <= q_hi) (a NaN q_lo: no lower end).  The loads past M go
// to the series' last draw and their bits are masked off.
__global__ void __launch_bounds__(256) k_essq_pack(const double* __restrict__ store, const int64_t* __restrict__ idx, int64_t k0, int64_t Kc,
                                                   int64_t size, int64_t N, int64_t M, int64_t C, int64_t Wd, int n_p,
                                                   const double* __restrict__ thr, uint64_t* __restrict__ bits) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t J = 2 * C;
  if (t >= Kc * Wd * J) return;
  const int64_t e = t % Kc, w = (t / Kc) % Wd, j = t / (Kc * Wd);
  const int64_t col = idx ? idx[k0 + e] : k0 + e;
  const int64_t it0 = ((j & 1) ? N - M : 0) + 64 * w;  // first iteration of the word
  const int64_t left = M - 64 * w;                    // draws of the series from there on, >= 1
  const int nv = left < 64 ? (int)left : 64;
  const int64_t stride = C * size;
  const double* p = store + (it0 * C + (j >> 1)) * size + col;
  double v[64];
#pragma unroll
  for (int i = 0; i < 64; ++i) v[i] = p[(int64_t)(i < nv ? i : nv - 1) * stride];
  const uint64_t mask = nv == 64 ? ~0ull : ((1ull << nv) - 1ull);
  for (int q = 0; q < n_p; ++q) {
    const double lo = thr[(e * n_p + q) * 2], hi = thr[(e * n_p + q) * 2 + 1];
    uint32_t w0 = 0, w1 = 0;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      w0 |= (uint32_t)((v[i] <= hi && !(v[i] < lo)) ? 1u : 0u) << i;
      w1 |= (uint32_t)((v[i + 32] <= hi && !(v[i + 32] < lo)) ? 1u : 0u) << i;
    }
    bits[((e * n_p + q) * J + j) * Wd + w] = (((uint64_t)w1 << 32) | w0) & mask;
  }
}

struct EssqLag {
  const uint64_t* bits;  // [Kc][n_p][J][Wd]
  int32_t* nj;           // [Kc][n_p][J] (the global form's series counts)
  const int32_t* flags;  // [Kc]
  int64_t k0, n_idx, J, M, Wd, n_cnt;
  int n_p;
  double* ess_out; int32_t* lag_out; int64_t* counts_out;
};

__device__ __forceinline__ unsigned long long essq_wave_sum(unsigned long long v) {
#pragma unroll
  for (int sh = 32; sh > 0; sh >>= 1) v += __shfl_xor(v, sh, 64);
  return v;
}

// One workgroup of EQ_NW waves per (element, interval).  A block of 64 lags t = 64 q + r, lane r of every wave on lag t:
//   A(t): the waves share out the J Wd words; for word i of a series the lane takes popc(w[i] & ((w[i+q] >> r) | (w[i+q+1] << (64 - r)))),
//         the words past the series' end being zero (the shift by 64 of r == 0 is written as two shifts);
//   H(t) = 2 Q - G(t), G(t + 1) = G(t) + sum_j n_j (b_j[t] + b_j[M - 1 - t]): the lane's increment, summed over the waves' series, then a
//         prefix sum over the lanes of wave 0 and the carry of the blocks before;
// the waves' integers are added through LDS, wave 0 forms Z(t) and S(t), and thread 0 advances the sequence (omc_geyer.h) and says
// whether another block is needed.  counts_out: Nn, Q, then (A(t), H(t)) for t < n_cnt, evaluated whatever the sequence needs.
template <bool LDS>
__global__ void __launch_bounds__(64 * EQ_NW) k_essq_lags(EssqLag a) {
  extern __shared__ uint64_t sm[];  // LDS form: the bits [J][Wd], then the series counts [J]
  __shared__ unsigned long long redA[EQ_NW][64], redH[EQ_NW][64];
  __shared__ double Sblk[64];
  __shared__ unsigned long long tot[2][EQ_NW];
  __shared__ int more;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t ep = blockIdx.x, e = ep / a.n_p, p = ep - e * a.n_p;
  const int64_t J = a.J, M = a.M, Wd = a.Wd, n_cnt = a.n_cnt;
  const int64_t o = p * a.n_idx + a.k0 + e;
  int64_t* cnt = a.counts_out ? a.counts_out + o * (2 + 2 * n_cnt) : nullptr;
  if (a.flags[e] != 0) {  // a non-finite draw somewhere in the element
    if (tid == 0) {
      if (a.ess_out) a.ess_out[o] = __longlong_as_double(0x7ff8000000000000LL);
      if (a.lag_out) a.lag_out[o] = 0;
    }
    if (cnt) for (int64_t i = tid; i < 2 + 2 * n_cnt; i += 64 * EQ_NW) cnt[i] = 0;
    return;
  }
  const int64_t total = J * Wd;
  const uint64_t* gw = a.bits + ep * total;
  const uint64_t* w;
  int32_t* nj;
  if (LDS) {
    for (int64_t i = tid; i < total; i += 64 * EQ_NW) sm[i] = gw[i];
    w = sm;
    nj = (int32_t*)(sm + total);
    __syncthreads();
  } else {
    w = gw;
    nj = a.nj + ep * J;
  }
  // the series counts, Nn and Q
  unsigned long long nn = 0, qq = 0;
  for (int64_t j = tid; j < J; j += 64 * EQ_NW) {
    unsigned long long c = 0;
    for (int64_t i = 0; i < Wd; ++i) c += (unsigned)__popcll(w[j * Wd + i]);
    nj[j] = (int32_t)c;
    nn += c;
    qq += c * c;
  }
  nn = essq_wave_sum(nn);
  qq = essq_wave_sum(qq);
  if (lane == 0) { tot[0][wave] = nn; tot[1][wave] = qq; }
  __syncthreads();
  int64_t Nn = 0, Q = 0;
#pragma unroll
  for (int u = 0; u < EQ_NW; ++u) { Nn += (int64_t)tot[0][u]; Q += (int64_t)tot[1][u]; }
  if (cnt && tid == 0) { cnt[0] = Nn; cnt[1] = Q; }

  const double JM = (double)J * (double)M, MM = (double)M * (double)M;
  GeyerState g = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool running = true;  // thread 0: the sequence goes on
  int64_t G = 0;        // wave 0: sum_j n_j (ones among the first and the last 64 q draws)
  // the words of a wave: [i_begin, i_end) of the J Wd, walked with the position within the series alongside
  const int64_t per = (total + EQ_NW - 1) / EQ_NW;
  const int64_t i_begin = per * wave < total ? per * wave : total, i_end = i_begin + per < total ? i_begin + per : total;
  const int64_t pos0 = i_begin % Wd;
  for (int64_t q = 0;; ++q) {
    const int64_t t0 = 64 * q, t = t0 + lane;
    uint32_t accA = 0;
    {
      int64_t pos = pos0;
      for (int64_t i = i_begin; i < i_end; ++i) {
        if (pos + q < Wd) {
          const uint64_t x = w[i], lo = w[i + q], hi = pos + q + 1 < Wd ? w[i + q + 1] : 0ull;
          accA += (uint32_t)__popcll(x & ((lo >> lane) | ((hi << 1) << (63 - lane))));
        }
        if (++pos == Wd) pos = 0;
      }
    }
    unsigned long long hinc = 0;
    if (t < M) {
      const int64_t back = M - 1 - t;
      for (int64_t j = wave; j < J; j += EQ_NW) {
        const uint64_t b = ((w[j * Wd + q] >> lane) & 1ull) + ((w[j * Wd + (back >> 6)] >> (back & 63)) & 1ull);
        hinc += (unsigned long long)nj[j] * b;
      }
    }
    redA[wave][lane] = accA;
    redH[wave][lane] = hinc;
    __syncthreads();
    if (wave == 0) {
      unsigned long long A = 0, inc = 0;
#pragma unroll
      for (int u = 0; u < EQ_NW; ++u) { A += redA[u][lane]; inc += redH[u][lane]; }
      unsigned long long scan = inc;  // inclusive prefix sum over the lanes
#pragma unroll
      for (int sh = 1; sh < 64; sh <<= 1) {
        const unsigned long long up = __shfl_up(scan, sh, 64);
        if (lane >= sh) scan += up;
      }
      const int64_t H = 2 * Q - (G + (int64_t)(scan - inc));
      G += (int64_t)__shfl(scan, 63, 64);
      const int64_t Z = M * M * (int64_t)A - M * H + (M - t) * Q;
      Sblk[lane] = t < M ? (double)Z / MM : 0.0;
      if (cnt && t < n_cnt) { cnt[2 + 2 * t] = (int64_t)A; cnt[3 + 2 * t] = H; }
    }
    __syncthreads();
    if (tid == 0) {
      auto S = [&](int64_t tt) { return Sblk[tt - t0]; };
      if (q == 0) {
        const double BM = (double)(J * Q - Nn * Nn) / (MM * (double)J * (double)(J - 1));
        if (geyer_start(g, Sblk[0], BM, J, M, S) != GEYER_GO) {  // every draw on one side of the interval
          if (a.ess_out) a.ess_out[o] = JM;
          if (a.lag_out) a.lag_out[o] = 0;
          running = false;
        }
      }
      if (running && geyer_advance(g, M, JM, t0 + 64, S)) {
        double ess;
        int32_t lags;
        geyer_finish(g, JM, ess, lags);
        if (a.ess_out) a.ess_out[o] = ess;
        if (a.lag_out) a.lag_out[o] = lags;
        running = false;
      }
      more = (t0 + 64 < M && (running || t0 + 64 < n_cnt)) ? 1 : 0;
    }
    __syncthreads();
    if (!more) break;
  }
}

// out [n_idx][n_pos] = the key at position pos[e][k] of the element's sorted column, NaN for an element with a NaN draw
__global__ void __launch_bounds__(256) k_essq_pick(int64_t Kc, int64_t k0, int64_t P, int64_t n_pos, const uint64_t* __restrict__ keys,
                                                   const int32_t* __restrict__ flags, const int64_t* __restrict__ pos,
                                                   double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= Kc * n_pos) return;
  const int64_t e = i / n_pos;
  const int64_t at = (k0 + e) * n_pos + (i - e * n_pos);
  out[at] = (flags[e] & 1) ? __longlong_as_double(0x7ff8000000000000LL) : q_val(keys[e * P + pos[at]]);
}

}  // namespace

extern "C" omc_status omc_store_ess_indicator(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx,
                                              int64_t n_idx, const double* prob_lo, const double* prob_hi, int32_t n_p, int32_t algo,
                                              double* ess_out, int32_t* lag_out, double* q_out, int64_t* counts_out, int64_t n_cnt) {
  if (!omc_selection_ok(ctx, n_iter, 4, size, store, idx, n_idx) || !prob_lo || !prob_hi || n_p < 1 || n_p > EQ_MAXP || algo < 0 || algo > 2 ||
      n_cnt < 0)
    return OMC_INVALID_ARG;
  const int64_t N = n_iter, C = ctx->n_chains, M = N / 2, J = 2 * C, Wd = (M + 63) / 64;
  if (n_cnt > M) return OMC_INVALID_ARG;
  const RankGeom g = rank_geom(N, C, true);
  EssqProbs pr;
  for (int p = 0; p < EQ_MAXP; ++p) {
    pr.r0[0][p] = -1;
    pr.r0[1][p] = pr.r1[0][p] = pr.r1[1][p] = 0;
    pr.fr[0][p] = pr.fr[1][p] = 0.0;
    if (p < n_p) {
      const double lo = prob_lo[p], hi = prob_hi[p];
      if (!(hi >= 0.0 && hi <= 1.0) || lo != lo || (lo >= 0.0 && !(lo <= hi))) return OMC_INVALID_ARG;
      if (lo >= 0.0) essq_ranks(g.S, lo, pr.r0[0][p], pr.r1[0][p], pr.fr[0][p]);
      essq_ranks(g.S, hi, pr.r0[1][p], pr.r1[1][p], pr.fr[1][p]);
    }
  }
  if ((N * C + 63) / 64 > 0x7fffffffLL) return OMC_INVALID_ARG;
  // Z(t) and J Q - Nn^2 must be exact in int64: J M^3 < 2^62 and J M < 2^31
  if (g.S >= ((int64_t)1 << 31) || (double)J * (double)M * (double)M * (double)M >= 4611686018427387904.0) return OMC_UNSUPPORTED;
  const size_t lds = (size_t)J * Wd * sizeof(uint64_t) + (size_t)J * sizeof(int32_t);
  if (algo == 1 && lds > EQ_LDS_MAX) return OMC_INVALID_ARG;
  const bool in_lds = algo == 1 || (algo == 0 && lds <= EQ_LDS_MAX);
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  // per element: keys [P], the thresholds [n_p][2], the bits [n_p][J][Wd], the series counts [n_p][J], the flag word
  RankCarve ws(ctx, (size_t)g.P * sizeof(uint64_t) + (size_t)n_p * (2 * sizeof(double) + lds) + sizeof(int32_t), n_idx);
  while (ws.Kc > 1 && ws.Kc * (int64_t)n_p > 0x7fffffffLL) ws.Kc /= 2;
  const int64_t Kc = ws.Kc;
  if (Kc * Wd * J / 256 > 0x7fffffffLL) return OMC_INVALID_ARG;
  uint64_t* keys = ws.take<uint64_t>((size_t)Kc * g.P);
  uint64_t* bits = ws.take<uint64_t>((size_t)Kc * n_p * J * Wd);
  double* thr = ws.take<double>((size_t)Kc * n_p * 2);
  int32_t* nj = ws.take<int32_t>((size_t)Kc * n_p * J);
  int32_t* flags = ws.take<int32_t>(Kc);
  omc_status st = ws.done();
  if (st == OMC_OK) st = omc_store_check_index(ctx, ws.head(), idx, n_idx, size);
  if (st != OMC_OK) return st;
  hipStream_t s = ctx->stream;
  if (in_lds) OMC_HIP_CHECK(hipFuncSetAttribute((const void*)k_essq_lags<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)EQ_LDS_MAX));
  EssqLag a;
  a.bits = bits; a.nj = nj; a.flags = flags; a.n_idx = n_idx; a.J = J; a.M = M; a.Wd = Wd; a.n_cnt = counts_out ? n_cnt : 0; a.n_p = n_p;
  a.ess_out = ess_out; a.lag_out = lag_out; a.counts_out = counts_out;
  for (int64_t k0 = 0; k0 < n_idx; k0 += Kc) {
    const int64_t kc = n_idx - k0 < Kc ? n_idx - k0 : Kc;
    st = rank_gather_sort(ctx, store, idx, k0, kc, size, g, nullptr, keys, flags);
    if (st != OMC_OK) return st;
    hipLaunchKernelGGL(k_essq_thresholds, dim3((unsigned)((kc + 63) / 64)), dim3(64), 0, s, kc, k0, n_idx, g.P, (int)n_p, pr, keys, thr,
                       q_out);
    hipLaunchKernelGGL(k_essq_pack, dim3((unsigned)((kc * Wd * J + 255) / 256)), dim3(256), 0, s, store, idx, k0, kc, size, N, M, C, Wd,
                       (int)n_p, thr, bits);
    a.k0 = k0;
    if (in_lds) hipLaunchKernelGGL(k_essq_lags<true>, dim3((unsigned)(kc * n_p)), dim3(64 * EQ_NW), lds, s, a);
    else hipLaunchKernelGGL(k_essq_lags<false>, dim3((unsigned)(kc * n_p)), dim3(64 * EQ_NW), 0, s, a);
    OMC_HIP_CHECK(hipGetLastError());
  }
  return OMC_OK;
}

extern "C" omc_status omc_store_order_stats(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx,
                                            int64_t n_idx, int32_t split, const int64_t* pos, int64_t n_pos, double* out) {
  if (!omc_selection_ok(ctx, n_iter, split ? 4 : 1, size, store, idx, n_idx) || !pos || n_pos < 1 || !out) return OMC_INVALID_ARG;
  const int64_t N = n_iter, C = ctx->n_chains;
  const RankGeom g = rank_geom(N, C, split != 0);
  if ((N * C + 63) / 64 > 0x7fffffffLL) return OMC_INVALID_ARG;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  RankCarve ws(ctx, (size_t)g.P * sizeof(uint64_t) + sizeof(int32_t), n_idx);
  const int64_t Kc = ws.Kc;
  if (Kc * n_pos / 256 > 0x7fffffffLL) return OMC_INVALID_ARG;
  uint64_t* keys = ws.take<uint64_t>((size_t)Kc * g.P);
  int32_t* flags = ws.take<int32_t>(Kc);
  omc_status st = ws.done();
  // the selection against [0, size) and the positions against [0, S): one read-back, before out is written
  if (st == OMC_OK) st = omc_store_check_index(ctx, ws.head(), idx, n_idx, size, pos, n_idx * n_pos, g.S);
  if (st != OMC_OK) return st;
  for (int64_t k0 = 0; k0 < n_idx; k0 += Kc) {
    const int64_t kc = n_idx - k0 < Kc ? n_idx - k0 : Kc;
    st = rank_gather_sort(ctx, store, idx, k0, kc, size, g, nullptr, keys, flags);
    if (st != OMC_OK) return st;
    hipLaunchKernelGGL(k_essq_pick, dim3((unsigned)((kc * n_pos + 255) / 256)), dim3(256), 0, ctx->stream, kc, k0, g.P, n_pos, keys, flags, pos,
                       out);
    OMC_HIP_CHECK(hipGetLastError());
  }
  return OMC_OK;
}
