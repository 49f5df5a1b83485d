// LDS images of k_hist2d_pair and k_hist2d_pool (omc_hist2d.hip), as arithmetic that compiles for the host and the device alike,
// as omc_hist_layout.h does for k_hist_count: the kernels take every offset and stride from hist2d_layout() and the host the
// bytes it launches with.  No HIP headers: omc_store_histogram2d_layout hands the same numbers to the host-only test
// (tests/test_hist2d_layout_host.py).  Threads, bin limit and LDS budget are those of the marginal histogram.
#pragma once
#include "omc_hist_layout.h"

#define HIST2D_PER_PAIR 0  // shapes: a grid per pair
#define HIST2D_POOLED 1    // ... one grid for all pairs
#define HIST2D_POOLED_OCC 2  // ... and a second one for the rows in which a cell is occupied
#define HIST2D_OCC_PAIRS 256  // occupancy keeps a row's cells in one wave: four per lane

// Per pair: one workgroup = a tile of TE consecutive pairs x slices of RB rows.  Thread t: pair t % TE, row lane t / TE.
// Pooled pairs: one workgroup = ONE grid (TE = 1) x slices of RB rows; the lanes of a wave lie along the pairs of a row.
//   edges x doubles: shared [nx + 1]; per pair [TE][EXS], EXS odd so that lanes at one edge meet different 8-byte banks
//   edges y doubles: likewise [ny + 1] / [TE][EYS]
//   counts  uint32 [TE][CS], cell jx * ny + jy of a pair; CS odd: lanes (pairs) adding to one cell meet different banks, and the
//           flush reads a pair's grid in order.  LDS form only: the direct form adds to the output itself (CS = 0)
//   occupied uint32 [nx ny], pooled pairs with occupancy, LDS form only
//   outside uint64 [TE][2]: pairs with a coordinate outside its range, pairs with a NaN coordinate (64 bits: the direct form has
//           no limit on the rows a workgroup walks)
// Every region starts on 8 bytes.
struct Hist2dLayout {
  int nx, ny, per_pair, shape;
  int direct;    // 1: the counters of one pair do not fit the budget -- 64-bit atomic adds straight to the output
  int TE, RB;    // tile pairs; rows of a slice
  int EXS, EYS;  // strides of a pair's edges (doubles; 0 when shared)
  int CS;        // stride of a pair's counters (words; 0 in the direct form)
  int ex_off, ey_off, counts_off, occ_off, outside_off, end;  // bytes
};

OMC_HIST_HD constexpr int hist2d_up8(int b) { return (b + 7) & ~7; }

OMC_HIST_HD constexpr Hist2dLayout hist2d_layout_te(int nx, int ny, int per_pair, int shape, int direct, int te) {
  Hist2dLayout l{};
  const int cells = nx * ny;
  l.nx = nx; l.ny = ny; l.per_pair = per_pair; l.shape = shape; l.direct = direct; l.TE = te;
  // The flush costs one 8-byte atomic add per non-zero cell, pair and slice, and atomics run at about a fifth of the load rate
  // (omc_hist_layout.h).  Per pair a row brings two 8-byte loads for a pair's grid: eight rows per cell keep the flush under a
  // third of the reading, as sixteen rows per bin do there.  Pooled, a row brings two loads for EVERY pair into the one grid
  // (tens of them in a ragged store) and the map of such a store is sparse, so one row per cell is enough and keeps a store of
  // a million rows in a few hundred workgroups.  The direct form has nothing to flush: the shortest slice.
  l.RB = 1024;
  if (!direct)
    while (l.RB < (shape == HIST2D_PER_PAIR ? 8 : 1) * cells) l.RB *= 2;
  l.EXS = per_pair ? ((nx + 1) | 1) : 0;
  l.EYS = per_pair ? ((ny + 1) | 1) : 0;
  l.CS = direct ? 0 : (cells | 1);
  l.ex_off = 0;
  l.ey_off = 8 * (per_pair ? te * l.EXS : nx + 1);
  l.counts_off = l.ey_off + 8 * (per_pair ? te * l.EYS : ny + 1);
  l.occ_off = hist2d_up8(l.counts_off + 4 * te * l.CS);
  l.outside_off = hist2d_up8(l.occ_off + ((shape == HIST2D_POOLED_OCC && !direct) ? 4 * cells : 0));
  l.end = l.outside_off + 8 * te * 2;
  return l;
}

// The largest power-of-two tile whose image fits the budget in the given form (in the LDS form TE = 1 may still not fit)
OMC_HIST_HD constexpr Hist2dLayout hist2d_layout_form(int nx, int ny, int per_pair, int shape, int direct) {
  int te = shape == HIST2D_PER_PAIR ? HIST_TE_MAX : 1;
  while (te > 1 && hist2d_layout_te(nx, ny, per_pair, shape, direct, te).end > HIST_LDS_BUDGET) te /= 2;
  return hist2d_layout_te(nx, ny, per_pair, shape, direct, te);
}

// The form a shape takes by itself: the LDS form, or, where not even one pair's counters fit, the direct form with the largest
// tile of edges that fits (TE = 1 fits at every nx, ny <= HIST_MAX_BINS: 16 KiB of edges).
OMC_HIST_HD constexpr Hist2dLayout hist2d_layout(int nx, int ny, int per_pair, int shape) {
  const Hist2dLayout l = hist2d_layout_form(nx, ny, per_pair, shape, 0);
  return l.end <= HIST_LDS_BUDGET ? l : hist2d_layout_form(nx, ny, per_pair, shape, 1);
}

// the smallest tile of the largest grid each form takes
static_assert(hist2d_layout(HIST_MAX_BINS, HIST_MAX_BINS, 1, HIST2D_PER_PAIR).end <= HIST_LDS_BUDGET &&
                  hist2d_layout(HIST_MAX_BINS, HIST_MAX_BINS, 0, HIST2D_PER_PAIR).end <= HIST_LDS_BUDGET &&
                  hist2d_layout(HIST_MAX_BINS, HIST_MAX_BINS, 0, HIST2D_POOLED_OCC).end <= HIST_LDS_BUDGET &&
                  hist2d_layout(HIST_MAX_BINS, HIST_MAX_BINS, 1, HIST2D_PER_PAIR).direct == 1,
              "the edges of one pair must fit in the direct form");
static_assert(hist2d_layout(HIST_MAX_BINS, 9, 0, HIST2D_PER_PAIR).direct == 0 && hist2d_layout(HIST_MAX_BINS, 9, 0, HIST2D_PER_PAIR).TE == 1 &&
                  hist2d_layout(HIST_MAX_BINS, 9, 0, HIST2D_PER_PAIR).end <= HIST_LDS_BUDGET &&
                  hist2d_layout(HIST_MAX_BINS, 10, 0, HIST2D_PER_PAIR).direct == 1 &&
                  hist2d_layout(9, HIST_MAX_BINS, 1, HIST2D_PER_PAIR).direct == 0 &&
                  hist2d_layout(9, HIST_MAX_BINS, 1, HIST2D_PER_PAIR).end <= HIST_LDS_BUDGET &&
                  hist2d_layout(10, HIST_MAX_BINS, 1, HIST2D_PER_PAIR).direct == 1,
              "the one-pair tile of the largest grid the LDS form takes must fit");
static_assert(hist2d_layout(64, 64, 0, HIST2D_POOLED_OCC).direct == 0 && hist2d_layout(64, 64, 0, HIST2D_POOLED_OCC).end <= HIST_LDS_BUDGET,
              "a 64 x 64 occupancy map is counted in LDS");
// 32-bit keys of the occupancy pass: (row of a wave's pass) * cells + cell, at most 4 x 64 rows
static_assert(256LL * HIST_MAX_BINS * HIST_MAX_BINS < (1LL << 31), "occupancy keys are ints");
