// LDS image of k_hist_count (omc_hist.hip), as arithmetic that compiles for the host and the device alike: the kernel takes every
// offset and stride from hist_layout() and the host the bytes it launches with, so the two cannot drift apart.  No HIP headers:
// omc_store_histogram_layout hands the same numbers to the host-only test (tests/test_hist_layout_host.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define OMC_HIST_HD __host__ __device__
#else
#define OMC_HIST_HD
#endif

#define HIST_THREADS 256
#define HIST_MAX_BINS 1024
#define HIST_TE_MAX 64               // elements of a tile: 512 contiguous bytes of a store row
#define HIST_LDS_BUDGET (48 * 1024)  // three workgroups (twelve waves) per CU of 160 KiB
#define HIST_LDS_WORKGROUP (64 * 1024)

// One workgroup: a tile of TE consecutive selected elements x slices of RB rows.  Thread t: element t % TE, row lane t / TE.
//   edges   doubles: shared [n_bins + 1]; per element [TE][ES], ES odd so that lanes of one bin meet 32 different 8-byte banks
//   counts  uint32 [TE][CS], CS odd: lanes (elements) adding to one bin meet different banks, the flush reads a row in order
//   outside uint32 [TE][3]: below, above, NaN
struct HistLayout {
  int n_bins, per_element;
  int TE, RB;  // tile elements; rows of a slice
  int ES, CS;  // strides of an element's edges (doubles; 0 when shared) and counters (words)
  int edges_off, counts_off, outside_off, end;  // bytes
};

OMC_HIST_HD constexpr HistLayout hist_layout_te(int n_bins, int per_element, int te) {
  HistLayout l{};
  l.n_bins = n_bins;
  l.per_element = per_element;
  l.TE = te;
  // The flush costs n_bins 8-byte atomic adds per element and slice against RB 8-byte loads, and atomics run at about a fifth
  // of the load rate: sixteen rows per bin keep the flush under a third of the reading; 1024 rows keep a small index in
  // enough workgroups.
  l.RB = 1024;
  while (l.RB < 16 * n_bins) l.RB *= 2;
  l.ES = per_element ? ((n_bins + 1) | 1) : 0;
  l.CS = n_bins | 1;
  l.edges_off = 0;
  l.counts_off = 8 * (per_element ? te * l.ES : n_bins + 1);
  l.outside_off = l.counts_off + 4 * te * l.CS;
  l.end = (l.outside_off + 4 * te * 3 + 7) & ~7;
  return l;
}

// the largest power-of-two tile whose image fits the budget (TE = 1 fits at every n_bins <= HIST_MAX_BINS)
OMC_HIST_HD constexpr HistLayout hist_layout(int n_bins, int per_element) {
  int te = HIST_TE_MAX;
  while (te > 1 && hist_layout_te(n_bins, per_element, te).end > HIST_LDS_BUDGET) te /= 2;
  return hist_layout_te(n_bins, per_element, te);
}

static_assert(hist_layout(HIST_MAX_BINS, 1).end <= HIST_LDS_BUDGET && hist_layout(HIST_MAX_BINS, 0).end <= HIST_LDS_BUDGET,
              "the one-element tile must fit");
static_assert(HIST_LDS_BUDGET <= HIST_LDS_WORKGROUP, "a workgroup gets at most 64 KiB");

#if defined(__HIPCC__)
// The bin rule of the store histograms (omc_hist.hip, omc_hist2d.hip), the one that makes counts equal np.histogram's bit for bit:
// the last j in [0, nb) with E[j] <= v, np.searchsorted(E, v, 'right') - 1 with the last bin closed, by comparisons with the
// edges alone -- a bisection or, with evenly spaced edges (UNIFORM; scale = nb / (E[nb] - e0)), an arithmetic guess put right by
// the same comparisons.  e0 = E[0] <= v <= E[nb], v not NaN: what lies outside or is NaN is the caller's to count.
template <bool UNIFORM>
__device__ __forceinline__ int hist_bin(const double* E, int nb, double e0, double scale, double v) {
  if (UNIFORM) {
    const double t = (v - e0) * scale;
    int j = t >= (double)nb ? nb - 1 : (int)t;
    while (j > 0 && v < E[j]) --j;
    while (j < nb - 1 && v >= E[j + 1]) ++j;
    return j;
  }
  int lo = 0, hi = nb - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (E[mid] <= v) lo = mid; else hi = mid - 1;
  }
  return lo;
}
#endif
