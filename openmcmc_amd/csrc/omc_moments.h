// Running (count, mean, m2) of a series of doubles: Welford's update by one value and Chan's combination of two partial results.
// Exact for equal values: the mean stays and m2 stays 0.  The order of the updates and combinations fixes the bits.
// Non-finite values: m2 is NaN from the first of them on, and Welford's mean from the value after an infinity on (its own
// inf - inf).  Chan's combination keeps an infinite mean as a plain sum does -- until the opposite infinity or a NaN meets it --, so
// a caller that wants numpy's mean of such a series replaces a NaN mean by the series' plain sum before it combines.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void omc_welford(double& n, double& mean, double& m2, double v) {
  n += 1.0;
  const double d = v - mean;
  mean += d / n;
  m2 = fma(d, v - mean, m2);
}
// Welford's update by a value that is the n-th of its series, with inv_n = 1 / n supplied by a caller that updates several series of
// the same length side by side (one division for all of them); exact for equal values like omc_welford
__device__ __forceinline__ void omc_welford_nth(double inv_n, double& mean, double& m2, double v) {
  const double d = v - mean;
  mean = fma(d, inv_n, mean);
  m2 = fma(d, v - mean, m2);
}
__device__ __forceinline__ void omc_chan(double& n, double& mean, double& m2, double nb, double mb, double qb) {
  if (nb == 0.0) return;
  if (n == 0.0) {  // nothing yet: b as it is (d * d * 0 below is NaN once d * d overflows, from |mb| = 1.4e154 on)
    n = nb; mean = mb; m2 = qb;
    return;
  }
  const double tot = n + nb, d = mb - mean;
  // (the fma spelt out: next to the other branch the compiler no longer contracts mean + d * (nb / tot), and the bits would move)
  mean = isinf(mean) ? mean + mb : fma(d, nb / tot, mean);
  m2 += qb + d * d * (n * nb / tot);
  n = tot;
}
