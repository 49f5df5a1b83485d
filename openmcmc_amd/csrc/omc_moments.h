// Running (count, mean, m2) of a series of doubles: Welford's update by one value and Chan's combination of two partial results.
// Exact for equal values: the mean stays and m2 stays 0.  The order of the updates and combinations fixes the bits.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void omc_welford(double& n, double& mean, double& m2, double v) {
  n += 1.0;
  const double d = v - mean;
  mean += d / n;
  m2 = fma(d, v - mean, m2);
}
__device__ __forceinline__ void omc_chan(double& n, double& mean, double& m2, double nb, double mb, double qb) {
  if (nb == 0.0) return;
  const double tot = n + nb, d = mb - mean;
  mean += d * (nb / tot);
  m2 += qb + d * d * (n * nb / tot);
  n = tot;
}
