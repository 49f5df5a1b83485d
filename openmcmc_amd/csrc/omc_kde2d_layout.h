// Tiling and LDS image of k_kde2d_conv (omc_kde2d.hip), as arithmetic that compiles for the host and the device alike: the kernel
// takes every offset from kde2d_layout() and the host the bytes it launches with, so the two cannot drift apart.  No HIP headers:
// omc_kde2d_layout hands the same numbers to the host-only test (tests/test_kde2d_layout_host.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define OMC_KDE2D_HD __host__ __device__
#else
#define OMC_KDE2D_HD
#endif

#define KDE2D_MIN_BINS 8
#define KDE2D_MAX_BINS 256
#define KDE2D_MAX_PROBS 16
#define KDE2D_THREADS 256             // four waves
#define KDE2D_TX 8                    // output rows of a workgroup's tile
#define KDE2D_LDS_BUDGET (48 * 1024)  // three workgroups per CU of 160 KiB at the largest grid
#define KDE2D_LDS_WORKGROUP (64 * 1024)

// One workgroup per (grid, output tile of TX rows x TY columns).  A lane owns RY adjacent columns of every row of the tile, TY =
// 64 RY; RY, and with it everything below, depends on ny alone: 1 up to 64 columns, 2 above (two tiles along y above 128).
//   counts  [RB + 1][CS] doubles: a block of RB count rows (exact below 2^53), columns ny .. CS - 1 zero, and one all-zero row (index
//           RB) that stands in for a row outside the block or without a draw.  RB = 32 rows up to 128 columns, 16 above, at most nx.
//           The region is at least TX TY doubles: the four waves' partial tiles are added through it when the blocks are done.
//   rownz   [RB + 1] words: whether a row of the block holds a draw (entry RB: 0)
//   mask    [RB + 1][2] 64-bit words: bit b of a row's 128 = whether its run of RY cells from column RY b holds a draw (row RB: 0)
//   weights [4][RY][PL] doubles, a vector per wave: for the wave's row offset di the weights over the column offset dj, one exp
//           each, de-interleaved into RY planes: plane p, slot s holds dj = RY s + (tile's first column) + p - NYP, NYP = ny rounded
//           up to RY.  PL = 64 + NYP / RY slots.  The lanes of a wave read consecutive slots of one plane: no bank conflict.
struct Kde2dLayout {
  int nx, ny, ry, tx, ty, rb, nyp, cs, pl, threads, tiles_x, tiles_y;
  int counts_off, rownz_off, mask_off, weights_off, wave_weights, end;  // bytes
};

OMC_KDE2D_HD constexpr int kde2d_round16(int bytes) { return (bytes + 15) & ~15; }

OMC_KDE2D_HD constexpr Kde2dLayout kde2d_layout(int nx, int ny) {
  Kde2dLayout l{};
  l.nx = nx;
  l.ny = ny;
  l.ry = ny <= 64 ? 1 : 2;
  l.tx = KDE2D_TX;
  l.ty = 64 * l.ry;
  l.rb = ny <= 128 ? 32 : 16;
  if (l.rb > nx) l.rb = nx;
  l.nyp = (ny + l.ry - 1) / l.ry * l.ry;
  l.cs = l.nyp;
  l.pl = 64 + l.nyp / l.ry;
  l.threads = KDE2D_THREADS;
  l.tiles_x = (nx + l.tx - 1) / l.tx;
  l.tiles_y = (ny + l.ty - 1) / l.ty;
  const int counts = 8 * (l.rb + 1) * l.cs, tile = 8 * l.tx * l.ty;
  l.counts_off = 0;
  l.rownz_off = l.counts_off + kde2d_round16(counts > tile ? counts : tile);
  l.mask_off = l.rownz_off + kde2d_round16(4 * (l.rb + 1));
  l.weights_off = l.mask_off + 16 * (l.rb + 1);
  l.wave_weights = kde2d_round16(8 * l.ry * l.pl);
  l.end = l.weights_off + (KDE2D_THREADS / 64) * l.wave_weights;
  return l;
}

static_assert(kde2d_layout(KDE2D_MAX_BINS, KDE2D_MAX_BINS).end <= KDE2D_LDS_BUDGET, "the largest grid must fit the budget");
static_assert(kde2d_layout(KDE2D_MAX_BINS, 128).end <= KDE2D_LDS_BUDGET, "the tallest count block must fit the budget");
static_assert(kde2d_layout(KDE2D_MAX_BINS, 64).end <= KDE2D_LDS_BUDGET, "one column per lane must fit the budget");
static_assert(KDE2D_LDS_BUDGET <= KDE2D_LDS_WORKGROUP, "a workgroup gets at most 64 KiB");
static_assert(KDE2D_MAX_BINS / 2 <= 128 && 64 <= 128, "a row's runs of RY cells fit its 128 mask bits at either lane width");
static_assert(KDE2D_THREADS == KDE2D_MAX_BINS, "a thread per count row when the rows' flags are taken by ballot");
static_assert(KDE2D_TX % 4 == 0, "a wave takes the rows of a tile in groups of four");
