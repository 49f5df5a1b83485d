// The order-preserving 64-bit image of a double and numpy's quantile interpolation, shared by the store summaries that work on
// order statistics (omc_store.hip: omc_store_quantiles; omc_rank.hip: the rank-normalised diagnostics).
#pragma once
#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ uint64_t q_key(double v) {
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  if (v != v) return ~0ull;  // every NaN sorts last, like np.sort
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double q_val(uint64_t k) {
  const uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

// np.quantile, method "linear": virtual index (n - 1) q, its floor and the next index (lib/_function_base_impl.py:
// _get_indexes / _get_gamma) for a column with nv valid values -> the two ranks and the interpolation weight
__device__ __forceinline__ void q_ranks(int64_t nv, double q, int64_t& lo, int64_t& hi, double& frac) {
  const double h = (double)(nv - 1) * q;
  lo = (int64_t)floor(h);
  if (lo < 0) lo = 0;
  if (lo > nv - 1) lo = nv - 1;
  hi = lo + 1 < nv ? lo + 1 : nv - 1;
  if (h >= (double)(nv - 1)) lo = hi = nv - 1;
  if (nv <= 0) lo = hi = 0;
  frac = (nv > 0 && h < (double)(nv - 1)) ? h - (double)lo : 0.0;
}

// numpy's _lerp (lib/_function_base_impl.py), operation by operation: a + (b - a) t, and b - (b - a)(1 - t) where t >= 0.5.
// (HIP's __dmul_rn / __dadd_rn are plain operators the compiler may still fuse into an fma: contraction is switched off here)
[[maybe_unused]] __device__ __noinline__ double q_lerp(double a, double b, double t) {
#pragma clang fp contract(off)
  const double diff = b - a;
  const double up = a + diff * t, down = b - diff * (1.0 - t);
  return t >= 0.5 ? down : up;
}

}  // namespace
