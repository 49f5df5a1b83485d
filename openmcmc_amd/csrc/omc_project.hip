// Linear maps and posterior-predictive draws of the device store on the fp64 matrix cores (gfx950: v_mfma_f64_16x16x4_f64).
// The contract is in include/omcmc_hip.h (omc_store_project).
//
// What it replaces: the loop over MCMC.store[...] of the reference that calls LinearCombination.predictor / Normal.rvs per stored
// draw (host arrays there).  store is [n_iter][C][size]; a ROW is the size contiguous doubles of one (iteration, chain), R = n_iter C
// rows.  Selection position k = 0 .. n_idx - 1 is element idx[k] of the row (k itself without an index) with value x[k]:
//   out[row][j] = base[row][j] + offset[j] + sum_k W[j][k] x[k] (+ z[row][j] / sqrt(prec[row][j or 0])),   j = 0 .. m - 1
// a tall product whose contraction runs ALONG the rows of the store (K contiguous in both operands), where omc_cov.hip and
// omc_gram.hip contract down them.
//
// k_project_mfma, one family (16-byte loads / 8-byte loads / 8-byte loads through the index, each in two tile shapes):
//   * a workgroup of 4 waves owns PJ_TR = 64 rows and PJ_TM = 128 output columns and walks the WHOLE contraction in slabs of
//     PJ_TK = 32 selection positions: no split of K over workgroups, no partial tiles, no atomics.  The waves sit 2 x 2, a wave
//     holds 32 rows x 64 columns = 2 x 4 MFMA tiles (64 accumulator registers).  grid x = row tiles, y = column tiles: with
//     m <= 128 the store is read exactly once.  With m <= 64 the right-hand pair of waves would idle: the tile is then
//     128 rows x 64 columns, the waves 4 x 1 (TALL), the same wave-level code and the same order of additions;
//   * the row slab goes to LDS as Xs[row][k], the W slab beside it as Ws[column][k], both at a row stride of PJ_TK + 2 doubles:
//     the 16 rows and 2 k values that half a wave reads for one MFMA operand (ds_read_b64, bank = double index mod 32) then lie
//     at 2 row + k mod 32, all different;
//   * loads run along the row: without an index, with an even size and a 16-byte aligned store, 16 lanes x 16 bytes per row of the
//     slab; otherwise 32 lanes x 8 bytes at the column the lane read once for the slab (idx[k], or k), so a contiguous index run
//     costs what no index costs.  The next slab is fetched into registers under the multiplications;
//   * omit_nan: a NaN draw is stored to LDS as 0, so its term is 0 whatever the weight (np.nansum of the terms).  Rows beyond R,
//     positions beyond n_idx and columns beyond m are stored as 0 and never loaded; an output element depends on its own row of
//     Xs and its own row of Ws only, and only real outputs are written: nothing that pads a tile reaches an output;
//   * blocks of 16 columns without a real output are skipped (wave-uniform), so m <= 16 costs one MFMA column per wave;
//   * the epilogue adds offset and base (read and written by the same thread: out may be base) and, with a precision, the
//     noise: one IEEE square root and one IEEE division per term, z from the chain's normal stream at draw index
//     (1 << 41) + it + (replicate << 44) (field map: omc_common.h), element j.
// Order of the additions of a row: the slabs in ascending k, inside a slab the MFMA steps of four positions in ascending k, each
// adding its four products to the accumulator as the instruction does.  The slabs hold the same values whichever load path
// filled them, and steps that lie wholly beyond n_idx add exact zeros where they are not skipped: the order depends on n_idx
// and PJ_TK only -- not on the row's position in its tile, on R, C, m, the tile shape, the index or the row's alignment.
// No scratch (tests/test_project_kernel_resources.py).
#include "omc_common.h"
#include "omc_store_view.h"

typedef double double4_t __attribute__((ext_vector_type(4)));

#define PJ_TR 64   // rows of a tile
#define PJ_TM 128  // output columns of a tile
#define PJ_TK 32   // selection positions of a slab
#define PJ_LD (PJ_TK + 2)

namespace {

struct ProjArgs {
  const double* store; const int64_t* idx; const double* W; const double* offset; const double* base; const double* prec;
  const double* z;
  double* out;
  int64_t R, size, n_idx, m, ld_w, prec_size, C, chain_offset;
  uint64_t seed, draw0;  // draw index of iteration 0: (1 << 41) + (replicate << 44)
  int32_t omit_nan;
};

// VEC: no index, even size, 16-byte aligned store (so n_idx == size is even and a pair never straddles n_idx)
// TALL: the tile is 128 rows x 64 columns, the waves 4 x 1 (m <= 64: no wave without a real column)
template <bool VEC, bool IDX, bool TALL>
__global__ void __launch_bounds__(256) k_project_mfma(ProjArgs g) {
  constexpr int TR = TALL ? 2 * PJ_TR : PJ_TR, TM = TALL ? PJ_TM / 2 : PJ_TM;
  __shared__ __attribute__((aligned(16))) double Xs[TR][PJ_LD];
  __shared__ __attribute__((aligned(16))) double Ws[TM][PJ_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = TALL ? wave : wave >> 1, wc = TALL ? 0 : wave & 1;
  const int64_t row0 = (int64_t)blockIdx.x * TR, col0 = (int64_t)blockIdx.y * TM;
  const bool omit = g.omit_nan != 0;
  // blocks of 16 columns of this wave that hold a real output
  const int64_t m_left = g.m - col0 - wc * 64;
  const int nq = m_left <= 0 ? 0 : (m_left >= 64 ? 4 : (int)((m_left + 15) >> 4));

  // slab element of a thread.  8-byte form: position kx, rows rx + 8 q (q < TR / 8; W: q < TM / 8).  16-byte form (rows only):
  // positions 2 px, 2 px + 1, rows rv + 16 q (q < TR / 16), the pair in xr[2 q], xr[2 q + 1]
  const int kx = tid & 31, rx = tid >> 5, px = tid & 15, rv = tid >> 4;
  double xr[TR / 8], wv[TM / 8];
  auto fetch = [&](int64_t k0) {
    if (VEC) {
      const int64_t k = k0 + 2 * px;
#pragma unroll
      for (int q = 0; q < TR / 16; ++q) {
        const int64_t r = row0 + rv + 16 * q;
        double2 v = make_double2(0.0, 0.0);
        if (k < g.n_idx && r < g.R) v = *(const double2*)(g.store + r * g.size + k);
        xr[2 * q] = v.x;
        xr[2 * q + 1] = v.y;
      }
    } else {
      const int64_t k = k0 + kx;
      const bool kok = k < g.n_idx;
      const int64_t col = kok ? (IDX ? g.idx[k] : k) : 0;  // 0 <= idx[k] < size: checked before the launch
#pragma unroll
      for (int q = 0; q < TR / 8; ++q) {
        const int64_t r = row0 + rx + 8 * q;
        xr[q] = (kok && r < g.R) ? g.store[r * g.size + col] : 0.0;
      }
    }
    const int64_t k = k0 + kx;
#pragma unroll
    for (int q = 0; q < TM / 8; ++q) {
      const int64_t j = col0 + rx + 8 * q;
      wv[q] = (k < g.n_idx && j < g.m) ? g.W[j * g.ld_w + k] : 0.0;
    }
  };
  // (the NaN test waits here: next to the load it would need the value at once, and the loads would no longer fly under the
  // multiplications)
  auto stage = [&]() {
    if (VEC) {
#pragma unroll
      for (int q = 0; q < TR / 16; ++q) {
        double2 v = make_double2(xr[2 * q], xr[2 * q + 1]);
        if (omit && v.x != v.x) v.x = 0.0;
        if (omit && v.y != v.y) v.y = 0.0;
        *(double2*)&Xs[rv + 16 * q][2 * px] = v;
      }
    } else {
#pragma unroll
      for (int q = 0; q < TR / 8; ++q) Xs[rx + 8 * q][kx] = (omit && xr[q] != xr[q]) ? 0.0 : xr[q];
    }
#pragma unroll
    for (int q = 0; q < TM / 8; ++q) Ws[rx + 8 * q][kx] = wv[q];
  };

  double4_t acc[2][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[a][q] = double4_t{0.0, 0.0, 0.0, 0.0};

  fetch(0);
  for (int64_t k0 = 0; k0 < g.n_idx; k0 += PJ_TK) {
    __syncthreads();  // the previous slab has been consumed
    stage();
    __syncthreads();
    if (k0 + PJ_TK < g.n_idx) fetch(k0 + PJ_TK);  // in flight under the multiplications below
    const int64_t left = g.n_idx - k0;
    const int steps = left >= PJ_TK ? PJ_TK / 4 : (int)((left + 3) >> 2);  // steps beyond n_idx would add zeros
    const int cl = lane & 15;
    for (int s = 0; s < steps; ++s) {
      const int kr = 4 * s + (lane >> 4);
      const double a0 = Xs[wr * 32 + cl][kr], a1 = Xs[wr * 32 + 16 + cl][kr];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q < nq) {
          const double b = Ws[wc * 64 + 16 * q + cl][kr];
          acc[0][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc[0][q], 0, 0, 0);
          acc[1][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc[1][q], 0, 0, 0);
        }
    }
  }

  // C/D of the f64 form: column = lane & 15, row = (lane >> 4) + 4 * register
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = row0 + wr * 32 + 16 * a + (lane >> 4) + 4 * r, col = col0 + wc * 64 + 16 * q + (lane & 15);
        if (q < nq && row < g.R && col < g.m) {
          const int64_t e = row * g.m + col;
          double v = acc[a][q][r];
          if (g.offset) v += g.offset[col];
          if (g.base) v += g.base[e];
          g.out[e] = v;
        }
      }
  if (g.prec_size == 0) return;
  // the noise, on the elements this thread has just written (one copy of the draw's code instead of 32)
#pragma unroll 1
  for (int t = 0; t < 32; ++t) {
    const int a = t >> 4, q = (t >> 2) & 3, r = t & 3;
    const int64_t row = row0 + wr * 32 + 16 * a + (lane >> 4) + 4 * r, col = col0 + wc * 64 + 16 * q + (lane & 15);
    if (row >= g.R || col >= g.m) continue;
    const int64_t e = row * g.m + col, it = row / g.C, c = row - it * g.C;
    const omc_rng_key key = omc_make_key(g.seed, g.draw0 + (uint64_t)it, OMC_RNG_NORMAL);
    const double z = omc_elem_normal(g.z, e, key, g.chain_offset + c, col);
    const double p = g.prec[row * g.prec_size + (g.prec_size == 1 ? 0 : col)];
    g.out[e] += __ddiv_rn(z, __dsqrt_rn(p));
  }
}

}  // namespace

extern "C" omc_status omc_store_project(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx,
                                        int64_t n_idx, int64_t m, const double* W, int64_t ld_w, const double* offset,
                                        const double* base, int32_t omit_nan, const double* prec, int64_t prec_size,
                                        const double* z_inject, uint64_t replicate, double* out) {
  if (!ctx) return omc_invalid("omc_store_project: no context");
  if (n_iter < 1) return omc_invalid("omc_store_project: n_iter < 1");
  if (size < 1) return omc_invalid("omc_store_project: size < 1");
  if (m < 1) return omc_invalid("omc_store_project: m < 1");
  if (!store || !W || !out) return omc_invalid("omc_store_project: store, W and out must not be NULL");
  if (n_idx < 1 || (!idx && n_idx != size)) return omc_invalid("omc_store_project: n_idx < 1, or no index and n_idx != size");
  if (ld_w < n_idx) return omc_invalid("omc_store_project: ld_w < n_idx");
  if (prec_size != 0 && prec_size != 1 && prec_size != m) return omc_invalid("omc_store_project: prec_size must be 0, 1 or m");
  if ((prec_size != 0) != (prec != nullptr)) return omc_invalid("omc_store_project: prec and prec_size must be given together");
  if (z_inject && !prec) return omc_invalid("omc_store_project: z_inject without prec");
  if (replicate > 15) return omc_invalid("omc_store_project: replicate > 15");
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  const omc_status st = omc_store_check_index(ctx, nullptr, idx, n_idx, size);
  if (st == OMC_INVALID_ARG) return omc_invalid("omc_store_project: an index outside [0, size)");  // (the helper's only use of that status)
  if (st != OMC_OK) return st;
  const StoreView v = omc_store_view(ctx, n_iter, size, true, store, idx, n_idx);  // pooled: R rows of row_stride = size doubles
  const bool tall = m <= PJ_TM / 2;  // 128 rows x 64 columns
  const int64_t row_tiles = tall ? (v.R + 2 * PJ_TR - 1) / (2 * PJ_TR) : (v.R + PJ_TR - 1) / PJ_TR, col_tiles = tall ? 1 : (m + PJ_TM - 1) / PJ_TM;
  if (row_tiles > 0x7fffffffLL || col_tiles > 65535) return omc_invalid("omc_store_project: more rows or outputs than one launch takes");
  ProjArgs g;
  g.store = v.data; g.idx = v.idx; g.W = W; g.offset = offset; g.base = base; g.prec = prec; g.z = z_inject; g.out = out;
  g.R = v.R; g.size = v.row_stride; g.n_idx = v.n; g.m = m; g.ld_w = ld_w; g.prec_size = prec_size;
  g.C = ctx->n_chains; g.chain_offset = ctx->chain_offset;
  g.seed = ctx->seed; g.draw0 = (1ULL << 41) + (replicate << 44);
  g.omit_nan = omit_nan != 0;
  const dim3 grid((unsigned)row_tiles, (unsigned)col_tiles), block(256);
  const bool vec = !idx && size % 2 == 0 && ((uintptr_t)store & 15) == 0;
  void (*kernel)(ProjArgs) = idx ? (tall ? k_project_mfma<false, true, true> : k_project_mfma<false, true, false>)
                             : vec ? (tall ? k_project_mfma<true, false, true> : k_project_mfma<true, false, false>)
                                   : (tall ? k_project_mfma<false, false, true> : k_project_mfma<false, false, false>);
  hipLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, g);
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}
