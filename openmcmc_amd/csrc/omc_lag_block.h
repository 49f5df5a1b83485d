// A block of L direct lag sums of one series kept in registers: L accumulators and an L-slot ring of lagged operands, one load of
// each operand per L FMAs.  Shared by omc_diag.hip (whole half-series) and omc_autocorr.hip (time slices of a column).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// L steps i = ib .. ib + L - 1 of the block, in batches of D_LAG_BATCH: the batch's 2 D_LAG_BATCH loads are issued back to back,
// then its FMAs run while the later loads are still on their way (the scheduling barrier keeps the compiler from sinking every load
// to its use, where each would be waited for alone: a memory round trip per step).  y(i) is the load alone; post(x), the centring,
// is applied behind the barrier, so that it does not make the batch wait load by load.  MASK: steps past i1 and lagged operands from e1
// on count as zero; their loads go to clamped indices and the zeros are selected afterwards, so that no load sits behind a branch.
constexpr int D_LAG_BATCH = 16;
template <int L, bool MASK, typename F, typename P>
__device__ __forceinline__ void d_lag_steps(int64_t t0, int64_t ib, int64_t i1, int64_t e1, F y, P post, double (&ring)[L], double (&acc)[L]) {
  constexpr int B = L < D_LAG_BATCH ? L : D_LAG_BATCH;
#pragma unroll
  for (int u0 = 0; u0 < L; u0 += B) {
    double a[B], b[B];
#pragma unroll
    for (int v = 0; v < B; ++v) {
      const int64_t i = ib + u0 + v;
      if (MASK) {
        a[v] = y(i < i1 ? i : i1 - 1);
        b[v] = y(i - t0 < e1 ? i - t0 : e1 - 1);
      } else {
        a[v] = y(i);
        b[v] = y(i - t0);  // (t0 == 0: the same address again, served by the cache, rather than a branch around the load)
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int v = 0; v < B; ++v) {
      const int u = u0 + v;
      const int64_t i = ib + u;
      const double av = (!MASK || i < i1) ? post(a[v]) : 0.0;
      ring[u] = (!MASK || (i < i1 && i - t0 < e1)) ? post(b[v]) : 0.0;
#pragma unroll
      for (int l = 0; l < L; ++l) acc[l] = fma(av, ring[(u - l + L) % L], acc[l]);
    }
  }
}

// With z(i) = post(y(i)):
// acc[l] += sum of z(i) z(i - t0 - l) over the steps i in [i0, i1) whose earlier factor e = i - t0 - l lies in [i0 - t0, e1), l < L:
// the lane's contribution to the lag sums t0 .. t0 + L - 1.  Ring slot u holds y(i - t0) of the step i = ib + u, or zero once
// i - t0 has reached e1; slots not yet written in this call are zero, which drops the terms with e < i0 - t0.  The loop is unrolled
// by L: every ring index is a compile-time constant.  y is called with i in [i0, i1) and with i - t0 in [i0 - t0, e1) only
// (i0 < i1 and i0 - t0 < e1, or nothing is done).
template <int L, typename F, typename P>
__device__ __forceinline__ void d_lag_block(int64_t t0, int64_t i0, int64_t i1, int64_t e1, F y, P post, double (&acc)[L]) {
  double ring[L];
#pragma unroll
  for (int l = 0; l < L; ++l) ring[l] = 0.0;
  if (i0 - t0 >= e1) return;
  for (int64_t ib = i0; ib < i1; ib += L) {
    if (ib + L <= i1 && ib + L - 1 - t0 < e1) d_lag_steps<L, false>(t0, ib, i1, e1, y, post, ring, acc);
    else d_lag_steps<L, true>(t0, ib, i1, e1, y, post, ring, acc);
  }
}

// the whole series of M values: acc[l] += sum_{i = t0 + l}^{M - 1} z(i) z(i - t0 - l)
template <int L, typename F, typename P>
__device__ __forceinline__ void d_lag_block(int64_t t0, int64_t M, F y, P post, double (&acc)[L]) {
  d_lag_block<L>(t0, t0, M, M, y, post, acc);
}
