// LDS image of k_kde (omc_kde.hip), as arithmetic that compiles for the host and the device alike: the kernel takes every offset
// from kde_layout() and the host the bytes it launches with, so the two cannot drift apart.  No HIP headers: omc_kde_layout hands
// the same numbers to the host-only test (tests/test_kde_layout_host.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define OMC_KDE_HD __host__ __device__
#else
#define OMC_KDE_HD
#endif

#define KDE_MIN_BINS 8
#define KDE_MAX_BINS 1024
#define KDE_WAVE_BINS 128           // up to here one wave owns the column, above four
#define KDE_RED 16                  // block sums of a reduction: ceil(KDE_MAX_BINS / 64)
#define KDE_LDS_BUDGET (48 * 1024)  // three workgroups per CU of 160 KiB at the largest grid
#define KDE_LDS_WORKGROUP (64 * 1024)

// One workgroup per column, G bins.  All regions are doubles, every offset a multiple of 16 bytes:
//   counts [G]      the counts as doubles (exact below 2^53)
//   a2     [G]      the inclusive prefix sums of the counts while the quantiles are taken, then A2_k = a_k^2 (index k, entry 0 unused)
//   cos    [G + 1]  the quarter wave cos(pi m / (2 G)), m = 0..G
//   gauss  [2 G]    p_j = c_j / N in its first G entries while the a_k are formed, then T[d] = exp(-(d delta / h)^2 / 2)
//   red    [64]     two buffers of KDE_RED block sums, taken in turn, then 32 words of hand-over (quantiles, the waves' maxima)
struct KdeLayout {
  int n_bins, threads;
  int counts_off, a2_off, cos_off, gauss_off, red_off, end;  // bytes
};

OMC_KDE_HD constexpr int kde_round16(int bytes) { return (bytes + 15) & ~15; }

OMC_KDE_HD constexpr KdeLayout kde_layout(int n_bins) {
  KdeLayout l{};
  l.n_bins = n_bins;
  l.threads = n_bins <= KDE_WAVE_BINS ? 64 : 256;
  l.counts_off = 0;
  l.a2_off = l.counts_off + kde_round16(8 * n_bins);
  l.cos_off = l.a2_off + kde_round16(8 * n_bins);
  l.gauss_off = l.cos_off + kde_round16(8 * (n_bins + 1));
  l.red_off = l.gauss_off + kde_round16(16 * n_bins);
  l.end = l.red_off + 8 * (2 * KDE_RED + 32);
  return l;
}

static_assert(kde_layout(KDE_MAX_BINS).end <= KDE_LDS_BUDGET, "the largest grid must fit the budget");
static_assert(KDE_LDS_BUDGET <= KDE_LDS_WORKGROUP, "a workgroup gets at most 64 KiB");
static_assert(KDE_RED * 64 >= KDE_MAX_BINS, "one block sum per 64 bins");
