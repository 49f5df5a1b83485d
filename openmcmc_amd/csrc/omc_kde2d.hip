// Joint kernel density estimates of pairs of coordinates from their 2-D bin counts: the binned moments and the kernel covariance
// (given, or Scott's rule = Silverman's in two dimensions), the full-covariance binned Gaussian convolution, the joint mode and the
// density levels of the highest-density regions.  The contract is in include/omcmc_hip.h (omc_kde2d_binned).
//
// What it replaces: scipy.stats.gaussian_kde / az.plot_kde(x, y, hdi_probs=...) on two columns of MCMC.store[param] moved to the host
// (host arrays in the reference: mcmc.py:105-111).  The counts come from omc_store_histogram2d over evenly spaced edges; everything
// here is a function of (counts, grid) alone, so counts added over ranks give the estimate of all ranks' chains.
//
//   k_kde2d_check  a negative count, a prob outside (0, 1): two words, read back before anything is written.
//   k_kde2d_prep   one workgroup per grid: row and column sums (exact integers), the binned moments, H, the flag; hands A, B / A, 1 / h_yy,
//                  the bin widths and the norming constant to the passes behind it, and which rows hold a draw.  A floating-point
//                  sum over the rows or columns: blocks of 64 added by an xor butterfly, the block sums in ascending order; the cross
//                  moment: per row the same sum over its columns, then that sum over the rows.
//   k_kde2d_conv   the hot path, one workgroup of four waves per (grid, tile of TX x TY outputs); image: omc_kde2d_layout.h.  The
//                  count rows go through LDS as doubles in blocks of RB rows.  For a block and a tile the row offsets di = k - i
//                  that occur are dealt to the waves in turn; a wave makes the weights of its di over the column offset in its own
//                  LDS vector (one exp each) and then takes every pair (output row k, count row k - di) of the tile, four output
//                  rows at a time: per RY count columns the 4 RY counts (the same address in all lanes) and a window of 2 RY - 1
//                  weights feed 4 RY^2 FMAs.  A row without a draw is never loaded, and of a row's runs of RY cells only those
//                  that hold a draw in one of the four rows are walked, by the set bits of the rows' masks (a wave's ballot when
//                  the block comes in): adding +0 to a non-negative accumulator changes no bit.  An output is the sum of its four waves' partial sums, added
//                  in the order of the waves; which (i, j) a wave takes and in what order depends on (nx, ny) alone.
//   k_kde2d_mode   one workgroup per grid: the largest density (the lowest flat index of equals) and the sort keys, ~bits of the
//                  density: non-negative doubles order as unsigned integers, so an ascending sort of the keys is a descending
//                  sort of the densities; the all-ones key pads a column to a power of two and equals the key of a density +0.
//   rank_sort      the key-only bitonic sort of omc_store_shared.hip.
//   k_kde2d_level  one workgroup per grid: the running sums S_r of the sorted densities and the first r with S_r >= prob S.
// No atomics; nothing depends on the order in which workgroups or waves run.
#include <math.h>

#include "omc_common.h"
#include "omc_kde2d_layout.h"
#include "omc_rank_sort.h"

namespace {

struct Kde2dArgs {
  const int64_t* counts;                               // [n_grids][nx][ny]
  const double *lo_x, *hi_x, *lo_y, *hi_y;             // [n_grids]
  const double* bw_in;                                 // [n_grids][3], rule 0
  const double* probs;                                 // [n_probs]
  double *density, *bw, *mode, *level;                 // the caller's outputs or NULL
  int64_t* level_pos;
  int32_t* flag;
  double* dens;     // where the densities go: the caller's array (dens_g0 = 0) or the workspace of a chunk (dens_g0 = g0)
  double* prm;      // [n_grids][8]: A, B / A, 1 / h_yy, delta_x, delta_y, the norming constant, the flag
  uint64_t* rownz;  // [n_grids][KDE2D_MAX_BINS / 64]: bit i = count row i holds a draw
  uint64_t* keys;   // [chunk][P] or NULL: no levels wanted
  double bw_fct;
  int64_t g0, dens_g0, P;
  int nx, ny, rule, n_probs;
};

constexpr double KDE2D_2PI = 6.283185307179586;
constexpr double KDE2D_NEARLY_ONE = 1.0 - 1.0 / 1048576.0;  // 1 - 2^-20

__device__ __forceinline__ bool kde2d_finite(double x) { return fabs(x) < __longlong_as_double(0x7ff0000000000000LL); }
__device__ __forceinline__ double kde2d_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// the bin centre lo + (k + 1/2) delta with both roundings, as numpy forms it: no fused multiply-add
[[maybe_unused]] __device__ __noinline__ double kde2d_centre(double lo, double delta, int k) {
#pragma clang fp contract(off)
  const double step = ((double)k + 0.5) * delta;
  return lo + step;
}

__global__ void k_kde2d_check(const int64_t* __restrict__ counts, int64_t n, const double* __restrict__ probs, int n_probs,
                              int32_t* __restrict__ words) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n && counts[t] < 0) words[0] = 1;
  if (t < n_probs && !(probs[t] > 0.0 && probs[t] < 1.0)) words[1] = 1;
}

// sum of term(e), e < n <= 256, by 256 threads: a block of 64 by an xor butterfly, the block sums in ascending order; every thread
// holds the sum.  red: 4 doubles, not the buffer of the call before.
template <class F>
__device__ __forceinline__ double kde2d_sum(int n, double* red, F term) {
  const int tid = threadIdx.x;
  double v = tid < n ? term(tid) : 0.0;
#pragma unroll
  for (int sh = 32; sh > 0; sh >>= 1) v += __shfl_xor(v, sh, 64);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int b = 0; b < (n + 63) >> 6; ++b) s += red[b];
  return s;
}

__global__ void __launch_bounds__(KDE2D_THREADS) k_kde2d_prep(Kde2dArgs a) {
  __shared__ long long sRow[KDE2D_MAX_BINS], sCol[KDE2D_MAX_BINS], sColW[4][KDE2D_MAX_BINS];
  __shared__ double sT[KDE2D_MAX_BINS], sRed[2][4];
  __shared__ long long sInt[3][4];
  const int nx = a.nx, ny = a.ny, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t g = blockIdx.x;
  const int64_t* c = a.counts + g * nx * ny;
  int par = 0;
  auto red = [&]() { par ^= 1; return sRed[par]; };

  // row and column sums: exact integers, any order
  long long col[4] = {0, 0, 0, 0};
  for (int i = wave; i < nx; i += 4) {
    long long r = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = lane + 64 * q;
      const long long v = j < ny ? c[(int64_t)i * ny + j] : 0;
      col[q] += v;
      r += v;
    }
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) r += __shfl_xor(r, sh, 64);
    if (lane == 0) sRow[i] = r;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) sColW[wave][lane + 64 * q] = col[q];
  __syncthreads();
  if (tid < ny) sCol[tid] = sColW[0][tid] + sColW[1][tid] + sColW[2][tid] + sColW[3][tid];
  {
    long long n = tid < nx ? sRow[tid] : 0, zr = tid < nx && sRow[tid] > 0 ? 1 : 0;
    long long zc = tid < ny && sColW[0][tid] + sColW[1][tid] + sColW[2][tid] + sColW[3][tid] > 0 ? 1 : 0;
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) {
      n += __shfl_xor(n, sh, 64);
      zr += __shfl_xor(zr, sh, 64);
      zc += __shfl_xor(zc, sh, 64);
    }
    if (lane == 0) { sInt[0][wave] = n; sInt[1][wave] = zr; sInt[2][wave] = zc; }
  }
  {  // (KDE2D_THREADS == KDE2D_MAX_BINS: wave w answers for rows 64 w .. 64 w + 63)
    const uint64_t rows = __ballot(tid < nx && sRow[tid] > 0);
    if (lane == 0) a.rownz[g * (KDE2D_MAX_BINS / 64) + wave] = rows;
  }
  __syncthreads();
  const long long Ni = sInt[0][0] + sInt[0][1] + sInt[0][2] + sInt[0][3];
  const long long nzr = sInt[1][0] + sInt[1][1] + sInt[1][2] + sInt[1][3], nzc = sInt[2][0] + sInt[2][1] + sInt[2][2] + sInt[2][3];
  const double N = (double)Ni;
  const double lox = a.lo_x[g], hix = a.hi_x[g], loy = a.lo_y[g], hiy = a.hi_y[g];
  const double dx = (hix - lox) / (double)nx, dy = (hiy - loy) / (double)ny;
  const int rule = a.rule;
  bool bad = !(kde2d_finite(lox) && kde2d_finite(hix) && hix > lox && kde2d_finite(loy) && kde2d_finite(hiy) && hiy > loy);
  if (rule == 0) bad = bad || Ni < 1;
  else bad = bad || Ni < 2 || nzr < 2 || nzc < 2;
  double hxx = 0.0, hxy = 0.0, hyy = 0.0;
  if (!bad) {  // (the same in every thread)
    if (rule == 0) {
      hxx = a.bw_in[3 * g]; hxy = a.bw_in[3 * g + 1]; hyy = a.bw_in[3 * g + 2];
    } else {
      const double mx = kde2d_sum(nx, red(), [&](int i) { return (double)sRow[i] / N * (lox + ((double)i + 0.5) * dx); });
      const double my = kde2d_sum(ny, red(), [&](int j) { return (double)sCol[j] / N * (loy + ((double)j + 0.5) * dy); });
      const double vx = kde2d_sum(nx, red(), [&](int i) {
        const double d = lox + ((double)i + 0.5) * dx - mx;
        return (double)sRow[i] / N * d * d;
      });
      const double vy = kde2d_sum(ny, red(), [&](int j) {
        const double d = loy + ((double)j + 0.5) * dy - my;
        return (double)sCol[j] / N * d * d;
      });
      for (int i = wave; i < nx; i += 4) {
        double t = 0.0;
        if (sRow[i] > 0) {
          for (int q = 0; q < (ny + 63) >> 6; ++q) {
            const int j = lane + 64 * q;
            double v = j < ny ? (double)c[(int64_t)i * ny + j] / N * (loy + ((double)j + 0.5) * dy - my) : 0.0;
#pragma unroll
            for (int sh = 32; sh > 0; sh >>= 1) v += __shfl_xor(v, sh, 64);
            t += v;
          }
        }
        if (lane == 0) sT[i] = t * (lox + ((double)i + 0.5) * dx - mx);
      }
      __syncthreads();
      const double cxy = kde2d_sum(nx, red(), [&](int i) { return sT[i]; });
      const double corr = N / (N - 1.0), fac = pow(N, -1.0 / 3.0);
      hxx = fac * (corr * vx); hxy = fac * (corr * cxy); hyy = fac * (corr * vy);
    }
    const double f2 = a.bw_fct * a.bw_fct;
    hxx *= f2; hxy *= f2; hyy *= f2;
    bad = !(hxx > 0.0 && hyy > 0.0 && kde2d_finite(hxx) && kde2d_finite(hyy) && kde2d_finite(hxy)) ||
          !(hxy * hxy < KDE2D_NEARLY_ONE * (hxx * hyy));
  }
  if (tid != 0) return;
  double* prm = a.prm + 8 * g;
  const double nan = kde2d_nan();
  if (bad) {
    prm[6] = 1.0;
    if (a.bw) { a.bw[3 * g] = nan; a.bw[3 * g + 1] = nan; a.bw[3 * g + 2] = nan; }
    if (a.flag) a.flag[g] = 2;
    return;
  }
  const double det = hxx * hyy - hxy * hxy;
  // q = A u^2 + 2 B u v + C v^2 = A (u + (B / A) v)^2 + v^2 / h_yy: two non-negative terms, nothing cancels between them
  prm[0] = hyy / det; prm[1] = -hxy / hyy; prm[2] = 1.0 / hyy; prm[3] = dx; prm[4] = dy;
  prm[5] = 1.0 / (N * KDE2D_2PI * sqrt(det));
  prm[6] = 0.0;
  if (a.bw) { a.bw[3 * g] = hxx; a.bw[3 * g + 1] = hxy; a.bw[3 * g + 2] = hyy; }
  if (a.flag) a.flag[g] = 0;
}

template <int RY>
__global__ void __launch_bounds__(KDE2D_THREADS) k_kde2d_conv(Kde2dArgs a) {
  extern __shared__ __attribute__((aligned(16))) char kde2d_lds[];
  constexpr int TX = KDE2D_TX, NT = KDE2D_THREADS;
  const int nx = a.nx, ny = a.ny;
  const Kde2dLayout L = kde2d_layout(nx, ny);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  double* sC = (double*)(kde2d_lds + L.counts_off);
  int32_t* sNz = (int32_t*)(kde2d_lds + L.rownz_off);
  uint64_t* sM = (uint64_t*)(kde2d_lds + L.mask_off);
  double* sW = (double*)(kde2d_lds + L.weights_off + wave * L.wave_weights);
  const int tiles = L.tiles_x * L.tiles_y, tile = (int)(blockIdx.x % (unsigned)tiles);
  const int64_t g = a.g0 + blockIdx.x / (unsigned)tiles;
  const int k0 = (tile / L.tiles_y) * TX, lt = (tile % L.tiles_y) * L.ty;
  const int k_end = k0 + TX < nx ? k0 + TX : nx;
  const double* prm = a.prm + 8 * g;
  double* out = a.dens + (g - a.dens_g0) * nx * ny;
  if (prm[6] != 0.0) {  // a degenerate grid (the same in every thread)
    if (a.density)
      for (int idx = tid; idx < TX * L.ty; idx += NT) {
        const int k = k0 + idx / L.ty, l = lt + idx % L.ty;
        if (k < nx && l < ny) out[(int64_t)k * ny + l] = kde2d_nan();
      }
    return;
  }
  const double A = prm[0], beta = prm[1], ihyy = prm[2], dx = prm[3], dy = prm[4], norm = prm[5];
  const int nyp = L.nyp, cs = L.cs, PL = L.pl, njb = nyp / RY, rb = L.rb;
  const int64_t* c = a.counts + g * nx * ny;
  const uint64_t* nz = a.rownz + g * (KDE2D_MAX_BINS / 64);
  double acc[TX][RY];
#pragma unroll
  for (int rr = 0; rr < TX; ++rr)
#pragma unroll
    for (int r = 0; r < RY; ++r) acc[rr][r] = 0.0;
  for (int j = tid; j < cs; j += NT) sC[rb * cs + j] = 0.0;
  if (tid == 0) { sNz[rb] = 0; sM[2 * rb] = 0; sM[2 * rb + 1] = 0; }

  for (int i0 = 0; i0 < nx; i0 += rb) {
    const int rbn = rb < nx - i0 ? rb : nx - i0;
    __syncthreads();  // (the block before has been read)
    for (int r = tid; r < rbn; r += NT) sNz[r] = (int32_t)((nz[(i0 + r) >> 6] >> ((i0 + r) & 63)) & 1);
    __syncthreads();
    int any = 0;
    for (int r = 0; r < rbn; ++r) any |= sNz[r];
    if (!any) continue;  // (the same in every thread)
    for (int idx = tid; idx < rbn * cs; idx += NT) {
      const int r = idx / cs, j = idx - r * cs;
      if (sNz[r]) sC[idx] = j < ny ? (double)c[(int64_t)(i0 + r) * ny + j] : 0.0;
    }
    __syncthreads();
    for (int r = wave; r < rbn; r += NT / 64) {  // which runs of RY cells of row r hold a draw: lane b answers for runs b and 64 + b
      uint64_t m0 = 0, m1 = 0;
      if (sNz[r]) {  // (the same in every lane)
        bool a0 = false, a1 = false;
#pragma unroll
        for (int s = 0; s < RY; ++s) {
          if (lane < njb) a0 = a0 || sC[r * cs + RY * lane + s] != 0.0;
          if (lane + 64 < njb) a1 = a1 || sC[r * cs + RY * (lane + 64) + s] != 0.0;
        }
        m0 = __ballot(a0);
        m1 = __ballot(a1);
      }
      if (lane == 0) { sM[2 * r] = m0; sM[2 * r + 1] = m1; }
    }
    const int di_min = k0 - (i0 + rbn - 1), di_max = k_end - 1 - i0;
    for (int d0 = di_min; d0 <= di_max; d0 += NT / 64) {
      const int di = d0 + wave;
      const bool live = di <= di_max;
      __syncthreads();  // (the counts are in place; the weights of the step before have been read)
      if (live) {
        const double u = (double)di * dx;
        for (int idx = lane; idx < RY * PL; idx += 64) {
          const int p = idx / PL, s = idx - p * PL;
          const double v = (double)(RY * s + lt + p - nyp) * dy;
          const double t = u + beta * v;
          sW[idx] = exp(-0.5 * (A * t * t + v * v * ihyy));
        }
      }
      __syncthreads();
      if (!live) continue;
#pragma unroll
      for (int grp = 0; grp < TX / 4; ++grp) {
        int rp[4];
        uint64_t m[2] = {0, 0};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int k = k0 + 4 * grp + t, il = k - di - i0;
          const bool in = k < nx && il >= 0 && il < rbn;
          const int row = (in && sNz[in ? il : rb] != 0) ? il : rb;  // (row rb: all zero, no bit set; a row without a draw was not loaded)
          rp[t] = row * cs;
          m[0] |= sM[2 * row];
          m[1] |= sM[2 * row + 1];
        }
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          // (the masks are the same in every lane: a scalar loop over the set bits)
          uint64_t left = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m[half]) |
                          (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(m[half] >> 32)) << 32;
          while (left) {
            const int jb = 64 * half + __builtin_ctzll(left);
            left &= left - 1;
            double cc[4][RY];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
              for (int s = 0; s < RY; ++s) cc[t][s] = sC[rp[t] + RY * jb + s];
            const int M = lane - jb + njb;  // 1 .. PL - 1
            double win[2 * RY - 1];
#pragma unroll
            for (int d = -(RY - 1); d <= RY - 1; ++d) win[d + RY - 1] = d >= 0 ? sW[d * PL + M] : sW[(d + RY) * PL + M - 1];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
              for (int s = 0; s < RY; ++s)
#pragma unroll
                for (int r = 0; r < RY; ++r) acc[4 * grp + t][r] = fma(cc[t][s], win[r - s + RY - 1], acc[4 * grp + t][r]);
          }
        }
      }
    }
  }
  // the four waves' partial sums, added in the order of the waves; a lane meets its own slots only
  __syncthreads();
  for (int w = 0; w < NT / 64; ++w) {
    if (wave == w) {
#pragma unroll
      for (int rr = 0; rr < TX; ++rr)
#pragma unroll
        for (int r = 0; r < RY; ++r) {
          const int idx = rr * L.ty + RY * lane + r;
          sC[idx] = w ? sC[idx] + acc[rr][r] : acc[rr][r];
        }
    }
    __syncthreads();
  }
  for (int idx = tid; idx < TX * L.ty; idx += NT) {
    const int k = k0 + idx / L.ty, l = lt + idx % L.ty;
    if (k < nx && l < ny) out[(int64_t)k * ny + l] = sC[idx] * norm;
  }
}

__global__ void __launch_bounds__(256) k_kde2d_mode(Kde2dArgs a) {
  __shared__ double sB[4];
  __shared__ int sK[4];
  const int nx = a.nx, ny = a.ny, n = nx * ny, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t g = a.g0 + blockIdx.x;
  uint64_t* keys = a.keys ? a.keys + (g - a.g0) * a.P : nullptr;
  if (a.prm[8 * g + 6] != 0.0) {
    if (keys) for (int64_t e = tid; e < a.P; e += 256) keys[e] = ~0ull;
    if (a.mode && tid == 0) { a.mode[2 * g] = kde2d_nan(); a.mode[2 * g + 1] = kde2d_nan(); }
    return;
  }
  const double* f = a.dens + (g - a.dens_g0) * n;
  double best = -1.0;
  int best_k = 0;
  for (int e = tid; e < n; e += 256) {
    const double v = f[e];
    if (keys) keys[e] = ~(uint64_t)__double_as_longlong(v);
    if (v > best) { best = v; best_k = e; }  // (e ascends: the lowest index of equal densities stays)
  }
  if (keys) for (int64_t e = n + tid; e < a.P; e += 256) keys[e] = ~0ull;
  if (!a.mode) return;
#pragma unroll
  for (int sh = 32; sh > 0; sh >>= 1) {
    const double ob = __shfl_xor(best, sh, 64);
    const int ok = __shfl_xor(best_k, sh, 64);
    if (ob > best || (ob == best && ok < best_k)) { best = ob; best_k = ok; }
  }
  if (lane == 0) { sB[wave] = best; sK[wave] = best_k; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 0; w < 4; ++w)
      if (sB[w] > best || (sB[w] == best && sK[w] < best_k)) { best = sB[w]; best_k = sK[w]; }
    const double lox = a.lo_x[g], loy = a.lo_y[g];
    const double dx = (a.hi_x[g] - lox) / (double)nx, dy = (a.hi_y[g] - loy) / (double)ny;
    a.mode[2 * g] = kde2d_centre(lox, dx, best_k / ny);
    a.mode[2 * g + 1] = kde2d_centre(loy, dy, best_k % ny);
  }
}

// S_r: thread t owns the sorted densities [t len, (t + 1) len), len = ceil(n / 256); its running sum starts from the sum of the
// segment sums before it (each added up from zero in ascending order, the segments in ascending order) and takes its own
// densities in ascending order.  S is S_r at r = n - 1.
__global__ void __launch_bounds__(256) k_kde2d_level(Kde2dArgs a) {
  __shared__ double sSeg[256], sTot;
  __shared__ int sFirst[KDE2D_MAX_PROBS][256];
  const int n = a.nx * a.ny, tid = threadIdx.x, len = (n + 255) / 256;
  const int64_t g = a.g0 + blockIdx.x;
  if (a.prm[8 * g + 6] != 0.0) {
    if (tid < a.n_probs) {
      if (a.level) a.level[g * a.n_probs + tid] = kde2d_nan();
      if (a.level_pos) a.level_pos[g * a.n_probs + tid] = -1;
    }
    return;
  }
  const uint64_t* keys = a.keys + (g - a.g0) * a.P;
  const int r0 = tid * len < n ? tid * len : n, r1 = r0 + len < n ? r0 + len : n;
  double s = 0.0;
  for (int r = r0; r < r1; ++r) s += __longlong_as_double((long long)~keys[r]);
  sSeg[tid] = s;
  __syncthreads();
  double before = 0.0;
  for (int u = 0; u < tid; ++u) before += sSeg[u];
  if (r0 < n && r1 == n) {
    double run = before;
    for (int r = r0; r < r1; ++r) run += __longlong_as_double((long long)~keys[r]);
    sTot = run;
  }
  __syncthreads();
  const double S = sTot;
  for (int p = 0; p < a.n_probs; ++p) {
    const double target = a.probs[p] * S;
    double run = before;
    int first = 0x7fffffff;
    for (int r = r0; r < r1; ++r) {
      run += __longlong_as_double((long long)~keys[r]);
      if (run >= target && first == 0x7fffffff) first = r;
    }
    sFirst[p][tid] = first;
  }
  __syncthreads();
  if (tid < a.n_probs) {
    int r = n - 1;
    for (int u = 0; u < 256; ++u)
      if (sFirst[tid][u] != 0x7fffffff) { r = sFirst[tid][u]; break; }
    if (a.level) a.level[g * a.n_probs + tid] = __longlong_as_double((long long)~keys[r]);
    if (a.level_pos) a.level_pos[g * a.n_probs + tid] = r;
  }
}

}  // namespace

extern "C" omc_status omc_kde2d_layout(int32_t nx, int32_t ny, int32_t* out) {
  if (nx < KDE2D_MIN_BINS || nx > KDE2D_MAX_BINS || ny < KDE2D_MIN_BINS || ny > KDE2D_MAX_BINS || !out) return OMC_INVALID_ARG;
  const Kde2dLayout l = kde2d_layout(nx, ny);
  const int32_t v[16] = {l.tx, l.ty, l.ry, l.rb, l.threads, l.tiles_x, l.tiles_y, l.cs, l.pl, l.counts_off, l.rownz_off, l.mask_off,
                         l.weights_off, l.wave_weights, l.end, KDE2D_LDS_BUDGET};
  for (int i = 0; i < 16; ++i) out[i] = v[i];
  return OMC_OK;
}

extern "C" omc_status omc_kde2d_binned(omc_ctx* ctx, int64_t n_grids, int32_t nx, int32_t ny, const int64_t* counts, const double* lo_x,
                                       const double* hi_x, const double* lo_y, const double* hi_y, int32_t rule, const double* bw_in,
                                       double bw_fct, int32_t n_probs, const double* probs, double* density_out, double* bw_out,
                                       double* mode_out, double* level_out, int64_t* level_pos_out, int32_t* flag_out) {
  if (!ctx || n_grids < 1 || n_grids > 0x7fffffffLL || nx < KDE2D_MIN_BINS || nx > KDE2D_MAX_BINS || ny < KDE2D_MIN_BINS ||
      ny > KDE2D_MAX_BINS || !counts || !lo_x || !hi_x || !lo_y || !hi_y || rule < 0 || rule > 1 || (rule == 0 && !bw_in) ||
      !(bw_fct > 0.0 && bw_fct < HUGE_VAL) || n_probs < 0 || n_probs > KDE2D_MAX_PROBS || (n_probs > 0 && !probs))
    return OMC_INVALID_ARG;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int64_t cells = (int64_t)nx * ny, n = n_grids * cells;
  if ((n + 255) / 256 > 0x7fffffffLL) return OMC_INVALID_ARG;
  // store_ws: the two check words, then A, B / A, 1 / h_yy, the bin widths, the norming constant and the flag of every grid, then a
  // bit per count row of every grid
  const size_t prm_bytes = (size_t)n_grids * 8 * sizeof(double);
  omc_status st = omc_ensure(ctx, ctx->store_ws, 64 + prm_bytes + (size_t)n_grids * (KDE2D_MAX_BINS / 64) * sizeof(uint64_t));
  if (st != OMC_OK) return st;
  int32_t* words = (int32_t*)ctx->store_ws.p;
  int32_t got[2] = {0, 0};
  st = omc_words_zero(ctx, words, 2);
  if (st != OMC_OK) return st;
  hipLaunchKernelGGL(k_kde2d_check, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, counts, n, probs, (int)n_probs, words);
  st = omc_words_read(ctx, words, 2, got);
  if (st != OMC_OK) return st;
  if (got[0] || got[1]) return OMC_INVALID_ARG;

  Kde2dArgs a;
  a.counts = counts; a.lo_x = lo_x; a.hi_x = hi_x; a.lo_y = lo_y; a.hi_y = hi_y; a.bw_in = bw_in; a.probs = probs;
  a.density = density_out; a.bw = bw_out; a.mode = mode_out; a.level = level_out; a.level_pos = level_pos_out; a.flag = flag_out;
  a.dens = density_out;
  a.prm = (double*)((char*)ctx->store_ws.p + 64);
  a.rownz = (uint64_t*)((char*)ctx->store_ws.p + 64 + prm_bytes);
  a.keys = nullptr;
  a.bw_fct = bw_fct; a.g0 = 0; a.dens_g0 = 0; a.P = rank_pow2(cells); a.nx = nx; a.ny = ny; a.rule = rule; a.n_probs = n_probs;
  hipLaunchKernelGGL(k_kde2d_prep, dim3((unsigned)n_grids), dim3(KDE2D_THREADS), 0, s, a);
  OMC_HIP_CHECK(hipGetLastError());
  const bool levels = n_probs > 0 && (level_out || level_pos_out);
  if (!density_out && !mode_out && !levels) return OMC_OK;

  // rank_ws, a chunk of grids at a time (rank_chunk: what fits the budget, or option "rank_chunk"): the densities unless the caller
  // takes them, and the sort keys if levels are wanted
  const size_t per_grid = (density_out ? 0 : (size_t)cells * sizeof(double)) + (levels ? (size_t)a.P * sizeof(uint64_t) : 0);
  const int64_t Gc = rank_chunk(ctx, per_grid ? per_grid : sizeof(double), n_grids);
  if (per_grid) {
    st = omc_ensure(ctx, ctx->rank_ws, (size_t)Gc * per_grid);
    if (st != OMC_OK) return st;
  }
  const Kde2dLayout L = kde2d_layout(nx, ny);
  const int64_t tiles = (int64_t)L.tiles_x * L.tiles_y;
  for (int64_t g0 = 0; g0 < n_grids; g0 += Gc) {
    const int64_t gc = Gc < n_grids - g0 ? Gc : n_grids - g0;
    char* ws = (char*)ctx->rank_ws.p;
    a.g0 = g0;
    if (!density_out) {
      a.dens = (double*)ws;
      a.dens_g0 = g0;
      ws += (size_t)Gc * cells * sizeof(double);
    }
    a.keys = levels ? (uint64_t*)ws : nullptr;
    if (L.ry == 1) hipLaunchKernelGGL(k_kde2d_conv<1>, dim3((unsigned)(gc * tiles)), dim3(KDE2D_THREADS), (size_t)L.end, s, a);
    else hipLaunchKernelGGL(k_kde2d_conv<2>, dim3((unsigned)(gc * tiles)), dim3(KDE2D_THREADS), (size_t)L.end, s, a);
    if (mode_out || levels) hipLaunchKernelGGL(k_kde2d_mode, dim3((unsigned)gc), dim3(256), 0, s, a);
    OMC_HIP_CHECK(hipGetLastError());
    if (levels) {
      st = rank_sort(ctx, a.keys, gc, a.P);
      if (st != OMC_OK) return st;
      hipLaunchKernelGGL(k_kde2d_level, dim3((unsigned)gc), dim3(256), 0, s, a);
      OMC_HIP_CHECK(hipGetLastError());
    }
  }
  return OMC_OK;
}
