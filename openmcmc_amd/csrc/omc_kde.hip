// Kernel density estimates from bin counts: bandwidth rules (Scott, Silverman, improved Sheather-Jones, their mean), the binned
// Gaussian convolution with reflection at a bound, and the mode.  The contract is in include/omcmc_hip.h (omc_kde_binned).
//
// What it replaces: scipy.stats.gaussian_kde / ArviZ's kde on a column of MCMC.store[param] moved to the host (host arrays in the
// reference: mcmc.py:105-111).  The counts come from omc_store_histogram over evenly spaced edges; everything here is a function
// of (counts, lo, hi) alone, so counts added over ranks give the estimate of all ranks' chains.
//
// k_kde: one workgroup per column -- one wave up to KDE_WAVE_BINS bins, four above; the choice depends on G alone and both give
// the same bits.  The LDS image is kde_layout()'s (omc_kde_layout.h).
//   kde_sum      every floating-point sum over the bins or over k: the elements in blocks of 64, a block added by an xor butterfly
//                over the lanes of one wave (every lane ends with the same bits), the block sums through LDS in ascending order by
//                every thread.  The order depends on the element count alone, not on the wave that owns a block; every thread holds
//                the same sum, so the scan, the bisection and the choice of a root need no broadcast.  One barrier per sum: the
//                block sums alternate between two buffers.
//   quantiles    an exact inclusive prefix sum of the counts by wave 0; the one bin whose prefix pair encloses u N writes q(u).
//   ISJ          thread k forms a_k over the bins in ascending order, the cosine from the quarter-wave table by the integer
//                k (2 j + 1) mod 4 G, kept by adding 2 k; a Phi(t) is six dependent kde_sums of G - 1 terms.
//   density      thread k adds c_j (T[|k - j|] + images) over the non-empty bins in ascending order.
// No atomics; nothing depends on the order in which workgroups or waves run.
#include <math.h>

#include "omc_common.h"
#include "omc_kde_layout.h"

namespace {

struct KdeArgs {
  const int64_t* counts;  // [n_cols][G]
  const double *lo, *hi;  // [n_cols]
  const double* bw_in;    // [n_cols], rule 0
  double* density;        // [n_cols][G] or NULL
  double* bw;             // [n_cols] or NULL
  int32_t* flag;
  double* mode;
  double bw_fct;
  int G, rule, reflect;
};

constexpr double KDE_PI2 = 9.869604401089358;          // pi^2
constexpr double KDE_SQRT_2PI = 2.5066282746310002;    // sqrt(2 pi)
constexpr double KDE_SQRT_PI = 1.7724538509055159;     // sqrt(pi)
constexpr double KDE_SQRT_HALF = 0.70710678118654752;  // 2^(-1/2)
constexpr int KDE_SCAN = 47, KDE_BISECT = 60;

__global__ void k_kde_check(const int64_t* __restrict__ counts, int64_t n, int32_t* __restrict__ word) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n && counts[t] < 0) word[0] = 1;
}

// sum of term(e), e < n, in the order that n alone fixes (see above).  red: KDE_RED doubles, not the buffer of the call before.
template <int NT, class F>
__device__ __forceinline__ double kde_sum(int n, double* red, F term) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nb = (n + 63) >> 6;
  for (int b = wave; b < nb; b += NT / 64) {
    const int e = 64 * b + lane;
    double v = e < n ? term(e) : 0.0;
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) v += __shfl_xor(v, sh, 64);
    if (lane == 0) red[b] = v;
  }
  __syncthreads();
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s += red[b];
  return s;
}

__device__ __forceinline__ bool kde_finite(double x) { return fabs(x) < __longlong_as_double(0x7ff0000000000000LL); }

template <int NT>
__global__ void __launch_bounds__(NT) k_kde(KdeArgs a) {
  extern __shared__ __attribute__((aligned(16))) char kde_lds[];
  const int G = a.G;
  const KdeLayout L = kde_layout(G);
  double* sC = (double*)(kde_lds + L.counts_off);
  double* sA = (double*)(kde_lds + L.a2_off);
  double* sT = (double*)(kde_lds + L.cos_off);
  double* sG = (double*)(kde_lds + L.gauss_off);
  double* sR = (double*)(kde_lds + L.red_off);
  double* sX = sR + 2 * KDE_RED;  // hand-over: [0], [1] the quartiles, [2..) the waves' maxima and their bins
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t col = blockIdx.x;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  int par = 0;  // which buffer of block sums the next kde_sum takes
  auto red = [&]() { par ^= 1; return sR + KDE_RED * par; };

  const int64_t* c = a.counts + col * G;
  for (int j = tid; j < G; j += NT) sC[j] = (double)c[j];
  __syncthreads();
  const double lo = a.lo[col], hi = a.hi[col];
  const double delta = (hi - lo) / (double)G;
  const double N = kde_sum<NT>(G, red(), [&](int j) { return sC[j]; });
  const double nz = kde_sum<NT>(G, red(), [&](int j) { return sC[j] > 0.0 ? 1.0 : 0.0; });
  const int rule = a.rule;
  const double given = rule == 0 ? a.bw_in[col] : 1.0;
  bool bad = !(kde_finite(lo) && kde_finite(hi) && hi > lo);
  if (rule == 0) bad = bad || N < 1.0 || !(given > 0.0 && kde_finite(given));
  else bad = bad || N < 2.0 || nz < 2.0;
  if (bad) {  // (the same in every thread)
    if (a.density) for (int j = tid; j < G; j += NT) a.density[col * G + j] = nan;
    if (tid == 0) {
      if (a.bw) a.bw[col] = nan;
      if (a.mode) a.mode[col] = nan;
      if (a.flag) a.flag[col] = 2;
    }
    return;
  }

  double h = given;
  int flag = 0;
  if (rule != 0) {
    // quartiles: inclusive prefix sums (integers below 2^53: exact in any order), then the bin with C_j < u N <= C_j + c_j
    if (wave == 0) {
      double carry = 0.0;
      for (int b = 0; b < (G + 63) >> 6; ++b) {
        const int e = 64 * b + lane;
        double v = e < G ? sC[e] : 0.0;
#pragma unroll
        for (int sh = 1; sh < 64; sh <<= 1) {
          const double up = __shfl_up(v, sh, 64);
          if (lane >= sh) v += up;
        }
        v += carry;
        if (e < G) sA[e] = v;
        carry = __shfl(v, 63, 64);
      }
    }
    __syncthreads();
    for (int j = tid; j < G; j += NT) {
      const double inc4 = 4.0 * sA[j], exc4 = j ? 4.0 * sA[j - 1] : 0.0;
#pragma unroll
      for (int u = 1; u <= 3; u += 2) {
        const double un4 = (double)u * N;
        if (exc4 < un4 && inc4 >= un4) sX[u >> 1] = lo + delta * ((double)j + 0.25 * (un4 - exc4) / sC[j]);
      }
    }
    __syncthreads();
    const double iqr = sX[1] - sX[0];
    const double m =kde_sum<NT>(G, red(), [&](int j) { return sC[j] / N * (lo + ((double)j + 0.5) * delta); });
    const double var = kde_sum<NT>(G, red(), [&](int j) {
      const double d = lo + ((double)j + 0.5) * delta - m;
      return sC[j] / N * d * d;
    });
    const double sd = sqrt(N / (N - 1.0) * var);
    const double n15 = pow(N, -0.2);
    const double scott = 1.06 * sd * n15;
    const double spread = (iqr == 0.0 || sd < iqr / 1.34) ? sd : iqr / 1.34;
    const double silver = 0.9 * spread * n15;
    h = rule == 1 ? scott : silver;
    if (rule >= 3) {
      for (int mI = tid; mI <= G; mI += NT)
        sT[mI] = 2 * mI <= G ? cospi((double)mI / (double)(2 * G)) : sinpi((double)(G - mI) / (double)(2 * G));
      for (int j = tid; j < G; j += NT) sG[j] = sC[j] / N;
      if (tid == 0) sA[0] = 0.0;
      __syncthreads();  // (also: the prefix sums in sA have been read)
      for (int k = tid + 1; k < G; k += NT) {
        double acc = 0.0;
        int idx = k;  // k (2 j + 1) mod 4 G
        for (int j = 0; j < G; ++j) {
          const double p = sG[j];
          if (p != 0.0) {
            const int q = idx <= 2 * G ? idx : 4 * G - idx;                // cos is even about 2 G
            const double cs = q <= G ? sT[q] : -sT[2 * G - q];            // ... and odd about G
            acc += p * cs;
          }
          idx += 2 * k;
          if (idx >= 4 * G) idx -= 4 * G;
        }
        sA[k] = acc * acc;
      }
      __syncthreads();
      auto phi = [&](double t) {
        double f = 0.0, ts = t;
#pragma unroll 1
        for (int s = 7; s >= 2; --s) {
          double pi2s = 1.0, kappa = 1.0;
          for (int i = 1; i <= s; ++i) { pi2s *= KDE_PI2; kappa *= (double)(2 * i - 1); }
          if (s < 7) {
            const double cs = (1.0 + ldexp(KDE_SQRT_HALF, -s)) / 3.0;
            ts = pow(2.0 * cs * (kappa / KDE_SQRT_2PI) / (N * f), 2.0 / (double)(3 + 2 * s));
          }
          const double tt = ts;
          f = 2.0 * pi2s * kde_sum<NT>(G - 1, red(), [&](int e) {
            const double K = (double)(e + 1) * (double)(e + 1);
            double pw = K;
            for (int i = 1; i < s; ++i) pw *= K;
            const double x = K * KDE_PI2 * tt;
            if (x > 746.0) return 0.0;  // exp(-x) rounds to zero from 745.14 on: the same term, and a block of such k skips its exp
            return pw * sA[e + 1] * exp(-x);
          });
        }
        return t - pow(2.0 * N * KDE_SQRT_PI * f, -0.4);
      };
      auto scan_t = [](int i) { return ldexp((i & 1) ? KDE_SQRT_HALF : 1.0, -3 - (i >> 1)); };
      double t_hi = 0.0, t_lo = 0.0, prev = phi(scan_t(0));
      bool found = false, lo_pos = false;
#pragma unroll 1
      for (int i = 1; i < KDE_SCAN; ++i) {
        const double cur = phi(scan_t(i));
        if (kde_finite(prev) && kde_finite(cur) && ((prev >= 0.0) != (cur >= 0.0))) {
          t_hi = scan_t(i - 1); t_lo = scan_t(i); lo_pos = cur >= 0.0; found = true;
          break;
        }
        prev = cur;
      }
      double isj = silver;
      if (found) {
#pragma unroll 1
        for (int it = 0; it < KDE_BISECT; ++it) {
          const double mid = 0.5 * (t_lo + t_hi);
          // the ends have met in fp64: Phi(mid) is the end's own value, the step changes nothing, and neither does any later one
          if (mid == t_lo || mid == t_hi) break;
          if ((phi(mid) >= 0.0) == lo_pos) t_lo = mid; else t_hi = mid;
        }
        isj = sqrt(0.5 * (t_lo + t_hi)) * (hi - lo);
      } else {
        flag = 1;
      }
      h = rule == 3 ? isj : 0.5 * (silver + isj);
    }
  }
  h *= a.bw_fct;
  if (tid == 0) {
    if (a.bw) a.bw[col] = h;
    if (a.flag) a.flag[col] = flag;
  }
  if (!a.density && !a.mode) return;

  __syncthreads();  // (the p_j in sG have been read)
  const double step = delta / h;
  for (int d = tid; d < 2 * G; d += NT) {
    const double z = (double)d * step;
    sG[d] = exp(-0.5 * z * z);
  }
  __syncthreads();
  const bool r_lo = (a.reflect & 1) != 0, r_hi = (a.reflect & 2) != 0;
  const double norm = 1.0 / (N * h * KDE_SQRT_2PI);
  double best = -1.0;
  int best_k = 0;
  for (int k = tid; k < G; k += NT) {
    double acc = 0.0;
    for (int j = 0; j < G; ++j) {
      const double cj = sC[j];
      if (cj != 0.0) {
        double w = sG[k >= j ? k - j : j - k];
        if (r_lo) w += sG[k + j + 1];
        if (r_hi) w += sG[2 * G - 1 - k - j];
        acc += cj * w;
      }
    }
    const double f = acc * norm;
    if (a.density) a.density[col * G + k] = f;
    if (f > best) { best = f; best_k = k; }  // (k ascends: the lowest bin of equal densities stays)
  }
  if (!a.mode) return;
#pragma unroll
  for (int sh = 32; sh > 0; sh >>= 1) {
    const double ob = __shfl_xor(best, sh, 64);
    const int ok = __shfl_xor(best_k, sh, 64);
    if (ob > best || (ob == best && ok < best_k)) { best = ob; best_k = ok; }
  }
  if (lane == 0) { sX[2 + 2 * wave] = best; sX[3 + 2 * wave] = (double)best_k; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 0; w < NT / 64; ++w) {
      const double ob = sX[2 + 2 * w];
      const int ok = (int)sX[3 + 2 * w];
      if (ob > best || (ob == best && ok < best_k)) { best = ob; best_k = ok; }
    }
    a.mode[col] = lo + ((double)best_k + 0.5) * delta;
  }
}

}  // namespace

extern "C" omc_status omc_kde_layout(int32_t G, int32_t* out) {
  if (G < KDE_MIN_BINS || G > KDE_MAX_BINS || !out) return OMC_INVALID_ARG;
  const KdeLayout l = kde_layout(G);
  const int32_t v[8] = {l.threads, l.counts_off, l.a2_off, l.cos_off, l.gauss_off, l.red_off, l.end, KDE_LDS_BUDGET};
  for (int i = 0; i < 8; ++i) out[i] = v[i];
  return OMC_OK;
}

extern "C" omc_status omc_kde_binned(omc_ctx* ctx, int64_t n_cols, int32_t G, const int64_t* counts, const double* lo, const double* hi,
                                     int32_t rule, const double* bw_in, double bw_fct, int32_t reflect, double* density_out,
                                     double* bw_out, int32_t* flag_out, double* mode_out) {
  if (!ctx || n_cols < 1 || n_cols > 0x7fffffffLL || G < KDE_MIN_BINS || G > KDE_MAX_BINS || !counts || !lo || !hi || rule < 0 || rule > 4 ||
      (rule == 0 && !bw_in) || !(bw_fct > 0.0 && bw_fct < HUGE_VAL) || reflect < 0 || reflect > 3)
    return OMC_INVALID_ARG;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  omc_status st = omc_ensure(ctx, ctx->store_ws, 64);
  if (st != OMC_OK) return st;
  // a negative count: one word read back before anything is written
  int32_t* word = (int32_t*)ctx->store_ws.p;
  int32_t got = 0;
  const int64_t n = n_cols * G;
  if ((n + 255) / 256 > 0x7fffffffLL) return OMC_INVALID_ARG;
  st = omc_words_zero(ctx, word, 1);
  if (st != OMC_OK) return st;
  hipLaunchKernelGGL(k_kde_check, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, counts, n, word);
  st = omc_words_read(ctx, word, 1, &got);
  if (st != OMC_OK) return st;
  if (got) return OMC_INVALID_ARG;
  KdeArgs a;
  a.counts = counts; a.lo = lo; a.hi = hi; a.bw_in = bw_in; a.density = density_out; a.bw = bw_out; a.flag = flag_out; a.mode = mode_out;
  a.bw_fct = bw_fct; a.G = G; a.rule = rule; a.reflect = reflect;
  const KdeLayout L = kde_layout(G);
  if (L.threads == 64) hipLaunchKernelGGL(k_kde<64>, dim3((unsigned)n_cols), dim3(64), (size_t)L.end, s, a);
  else hipLaunchKernelGGL(k_kde<256>, dim3((unsigned)n_cols), dim3(256), (size_t)L.end, s, a);
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}
