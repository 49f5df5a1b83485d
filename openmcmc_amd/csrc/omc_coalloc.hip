// Co-allocation (posterior similarity) matrix and least-squares partition of the allocation vectors in the device store, on the
// int8 matrix cores (gfx950: v_mfma_i32_16x16x64_i8).  The contract is in include/omcmc_hip.h (omc_store_coalloc,
// omc_store_partition_score).
//
// What it replaces: (Z[:, :, None] == Z[:, None, :]).sum(0) on the gathered labels Z of MCMC.store[param] (host arrays in the
// reference); here the store stays on the device.  store is [n_iter][C][size], seen through StoreView as omc_store_cov sees it.
//   1. k_coalloc_pack reads the selected fp64 columns once and turns every draw into one byte: its label 0 .. K - 1, or 0xFF for
//      a draw that carries none (NaN, or any other value that is not an integer in [0, K)); it counts both kinds per element.
//      The bytes lie as [batch][block of 16 rows][column][16 rows]: the 16 bytes a lane of the tile pass or of the score pass
//      wants are one aligned 16-byte load, and consecutive lanes (columns) read consecutive 16 bytes.  Rows past the end of the
//      last block are 0xFF.  Nothing after this pass is floating point.
//   2. k_coalloc_mfma: the tiling of k_cov_mfma (omc_cov.hip: 128 x 128 output tile per workgroup on or below the diagonal, 4
//      waves in 2 x 2 of 64 x 64 = 4 x 4 MFMA tiles; grid x = (batch, tile pair), y = slice of the rows).  The contraction index
//      is (row, label) flattened, the label padded to Kp = the next power of two: operand element (column i, row r, label k) is
//      [z_ir == k], one-hot int8, so that sum_k a_irk a_jrk = [z_ir == z_jr].  A lane's fragment of v_mfma_i32_16x16x64_i8 is
//      16 consecutive contraction positions of one column -- 16 / Kp rows, or a 16-label piece of one row --, expanded from the
//      label bytes on the way to LDS (onehot16); both operands are expanded by the same function from the same positions, so
//      whatever order the instruction gives the 64 positions of a step, it gives it to both.  per_label: one label at a time
//      (Kp = 1, the byte is [z == k]), the label a third coordinate of grid x.  A slab is 256 contraction positions = 256 / Kp
//      rows, 16 fragments per column and side in LDS; the next slab's label bytes are fetched into registers under the
//      multiplications.  Partial tiles are int32: every row adds at most 1 to an entry, and a slice is capped at C_SLICE_CAP
//      rows, below 2^31.
//   3. k_coalloc_join adds the slices' partial tiles in int64 and mirrors the lower triangle: out == out' bit for bit.
//      Row chunks (the packed bytes are kept within 1 GiB) add to what the chunks before them left.
//   4. k_partition_score: a workgroup holds a 64 x 64 tile of W = R - 2 counts (int64, zero on and above the diagonal and past
//      the selection) in LDS and walks a slice of rows, a lane per row: the row's 64 + 64 labels come from the packed bytes
//      through LDS, the 64 of the tile's columns then sit in registers.  Partial scores are added to the zeroed score_out with
//      64-bit integer atomics; k_partition_best finds the first minimum of a batch.  Vector ALU: W does not fit int8.
// Integer sums do not depend on their order: repeated calls are bit-equal.
// Workspace: the packed bytes in ctx->rank_ws (a chunk at a time), the partial tiles and the word of the index check in
// ctx->store_ws (no pass of this file calls a summary that uses either).
#include <string>

#include "omc_common.h"
#include "omc_store_view.h"

typedef int int4_t __attribute__((ext_vector_type(4)));

#define CA_TS 128     // output tile
#define CA_SLAB 256   // contraction positions of a slab (four steps of the 16x16x64 instruction)
#define CA_GROUPS 16  // 16-byte fragments of a column in a slab
#define PS_T 64       // tile of the score pass
#define PS_ROWS 256   // rows a workgroup of the score pass holds at a time (a lane each)

namespace {

constexpr int64_t C_CHUNK_BYTES = (int64_t)1 << 30;        // packed bytes kept at a time
constexpr int64_t C_SLICE_CAP = ((int64_t)1 << 31) - 256;  // rows of a slice: an int32 partial count holds them

// the packed label of a draw: v == k for an integer 0 <= k < K (-0.0 is 0), else 0xFF with bit 8 (NaN) or bit 9 (any other value)
__device__ __forceinline__ uint32_t coalloc_label(double v, int K) {
  if (v != v) return 0x1FFu;
  if (v >= 0.0 && v < (double)K) {
    const int k = (int)v;
    if ((double)k == v) return (uint32_t)k;
  }
  return 0x2FFu;
}

// packed [batch][blocks][n][16]: rows r0 .. r0 + rows - 1 of every batch of the view.  grid x = tiles of 64 columns, y = groups of
// 16 blocks (strided), z = batch; a wave takes a block at a time, a lane a column of it.
__global__ void __launch_bounds__(256) k_coalloc_pack(StoreView v, int64_t r0, int64_t rows, int64_t blocks, int K,
                                                      uint4* __restrict__ packed, unsigned long long* __restrict__ flags) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t batch = blockIdx.z, j = (int64_t)blockIdx.x * 64 + lane;
  if (j >= v.n) return;
  const double* col = v.column(batch, j) + r0 * v.row_stride;
  uint4* out = packed + batch * blocks * v.n + j;
  uint32_t nan = 0, bad = 0;
  for (int64_t grp = blockIdx.y; grp * 16 < blocks; grp += gridDim.y) {
    for (int64_t b = grp * 16 + wave; b < grp * 16 + 16 && b < blocks; b += 4) {
      const double* p = col + b * 16 * v.row_stride;
      const int left = (int)((rows - b * 16 < 16) ? rows - b * 16 : 16);  // rows of the block that exist: 16 but in the last
      double x[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) x[r] = p[(r < left ? r : 0) * v.row_stride];
      uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const uint32_t z = r < left ? coalloc_label(x[r], K) : 0xFFu;
        nan += (z >> 8) & 1u;
        bad += z >> 9;
        w[r >> 2] |= (z & 0xFFu) << (8 * (r & 3));
      }
      out[b * v.n] = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
  if (flags) {
    if (nan) atomicAdd(flags + (batch * v.n + j) * 2, (unsigned long long)nan);
    if (bad) atomicAdd(flags + (batch * v.n + j) * 2 + 1, (unsigned long long)bad);
  }
}

// The one-hot int8 image of 16 consecutive contraction positions of one column, from the label bytes that cover them.
// LOGK = log2 Kp.  Kp <= 16: the positions are 16 / Kp whole rows, raw holds their 16 / Kp label bytes (lowest byte first);
// Kp > 16: they are labels base .. base + 15 of one row, raw[0] its label byte.  Kp == 1: the byte is [z == target].
template <int LOGK>
__device__ __forceinline__ uint4 onehot16(const uint32_t* raw, uint32_t base, uint32_t target) {
  constexpr int KP = 1 << LOGK;
  uint32_t o[4] = {0u, 0u, 0u, 0u};
  if constexpr (LOGK == 0) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {  // 0x01 in every byte of raw[w] that equals target (the exact zero-byte test on the difference)
      const uint32_t t = raw[w] ^ (target * 0x01010101u);
      const uint32_t y = ((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t | 0x7f7f7f7fu;
      o[w] = (~y) >> 7;
    }
  } else if constexpr (LOGK <= 2) {  // a row is 2 or 4 positions: its word and its first byte in the word are known here
#pragma unroll
    for (int r = 0; r < 16 / KP; ++r) {
      const uint32_t z = (raw[r >> 2] >> (8 * (r & 3))) & 0xFFu;
      o[(r * KP) >> 2] |= (z < (uint32_t)KP) ? 1u << (8 * (((r * KP) & 3) + (z & 3u))) : 0u;
    }
  } else {  // a row is two words or more
#pragma unroll
    for (int r = 0; r < (LOGK == 3 ? 2 : 1); ++r) {
      const uint32_t z = (raw[0] >> (8 * r)) & 0xFFu;
      const uint32_t d = (z < (uint32_t)KP) ? (uint32_t)(r * KP) + z - base : 0xFFFFFFFFu;  // (z < base wraps: no position)
      const uint32_t bit = (d < 16u) ? 1u << (8 * (d & 3u)) : 0u;
#pragma unroll
      for (int w = 0; w < 4; ++w) o[w] |= ((d >> 2) == (uint32_t)w) ? bit : 0u;
    }
  }
  return make_uint4(o[0], o[1], o[2], o[3]);
}

struct CoallocArgs {
  const uint8_t* packed;  // [batches][blocks][n][16]
  int32_t* part;          // [slices][batches labels][n][n], entries i >= j
  int64_t rows16;         // rows of the chunk, rounded up to whole blocks
  int64_t blocks, kchunk;
  int n, pairs, labels;   // labels: 1, or K with per_label (LOGK == 0: grid x = ((batch, label), tile pair))
};

template <int LOGK>
__global__ void __launch_bounds__(256, 2) k_coalloc_mfma(CoallocArgs a) {
  constexpr int KP = 1 << LOGK;
  constexpr int NB = KP <= 16 ? 16 / KP : 1;  // label bytes behind a fragment
  constexpr int RW = NB >= 4 ? NB / 4 : 1;    // ... in words
  constexpr int RS = CA_SLAB / KP;            // rows of a slab
  __shared__ uint4 As[CA_GROUPS][CA_TS];
  __shared__ uint4 Bs[CA_GROUPS][CA_TS];
  const int64_t bl = blockIdx.x / a.pairs, bls = gridDim.x / a.pairs;
  int t = (int)(blockIdx.x - bl * a.pairs), bi = 0;
  while (t >= bi + 1) { t -= bi + 1; ++bi; }  // tile pair below or on the diagonal from the linear index: bi >= bj
  const int bj = t;
  const bool one_panel = bi == bj;
  const int64_t batch = bl / a.labels;
  const uint32_t target = (uint32_t)(bl - batch * a.labels);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int64_t kbeg = (int64_t)blockIdx.y * a.kchunk;
  const int64_t kend = (kbeg + a.kchunk < a.rows16) ? kbeg + a.kchunk : a.rows16;
  const int ci = bi * CA_TS, cj = bj * CA_TS;
  const bool wave_on = ci + wr * 64 < a.n && cj + wc * 64 < a.n && !(one_panel && wr < wc);

  // fragment e = q * 256 + tid of a slab: group 2 q + tid / 128, column tid % 128 for every q
  const int c = tid & 127, g_lo = tid >> 7;
  const bool oka = ci + c < a.n, okb = !one_panel && cj + c < a.n;
  const uint8_t* base = a.packed + batch * a.blocks * a.n * 16;
  const uint8_t* pa = base + (int64_t)(oka ? ci + c : 0) * 16;
  const uint8_t* pb = base + (int64_t)(okb ? cj + c : 0) * 16;

  int4_t acc[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[m][q] = int4_t{0, 0, 0, 0};

  // the label bytes behind group g of the slab at row k0: rows k0 + (16 g >> LOGK) .., NB of them, inside one block of 16
  uint32_t ra[8][RW], rb[8][RW];
  auto load = [&](const uint8_t* p, int64_t row, bool ok, uint32_t* r) {
    const uint8_t* src = p + ((row >> 4) * a.n * 16 + (row & 15));
    if (!(ok && row < kend)) {
#pragma unroll
      for (int w = 0; w < RW; ++w) r[w] = 0xFFFFFFFFu;
    } else if constexpr (NB == 16) {
      const uint4 x = *(const uint4*)src;
      r[0] = x.x; r[1] = x.y; r[2] = x.z; r[3] = x.w;
    } else if constexpr (NB == 8) {
      const uint2 x = *(const uint2*)src;
      r[0] = x.x; r[1] = x.y;
    } else if constexpr (NB == 4) {
      r[0] = *(const uint32_t*)src;
    } else if constexpr (NB == 2) {
      r[0] = *(const uint16_t*)src;
    } else {
      r[0] = *src;
    }
  };
  auto fetch = [&](int64_t k0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int64_t row = k0 + (((2 * q + g_lo) * 16) >> LOGK);
      load(pa, row, oka, ra[q]);
      if (!one_panel) load(pb, row, okb, rb[q]);
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int g = 2 * q + g_lo;
      const uint32_t lab0 = (uint32_t)(g * 16) & (uint32_t)(KP - 1);
      As[g][c] = onehot16<LOGK>(ra[q], lab0, target);
      if (!one_panel) Bs[g][c] = onehot16<LOGK>(rb[q], lab0, target);
    }
  };

  fetch(kbeg);
  for (int64_t k0 = kbeg; k0 < kend; k0 += RS) {
    __syncthreads();  // the previous slab has been consumed
    stage();
    __syncthreads();
    if (k0 + RS < kend) fetch(k0 + RS);  // in flight under the multiplications below
    if (!wave_on) continue;
    const uint4(*Bp)[CA_TS] = one_panel ? As : Bs;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int g = kk * 4 + (lane >> 4), cl = lane & 15;
      int4_t fa[4], fb[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const uint4 x = As[g][wr * 64 + m * 16 + cl];
        fa[m] = int4_t{(int)x.x, (int)x.y, (int)x.z, (int)x.w};
      }
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const uint4 x = Bp[g][wc * 64 + m * 16 + cl];
        fb[m] = int4_t{(int)x.x, (int)x.y, (int)x.z, (int)x.w};
      }
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[m][q] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[m], fb[q], acc[m][q], 0, 0, 0);
    }
  }
  if (!wave_on) return;
  // C/D of the 16 x 16 forms (every type but f64): column = lane & 15, row = 4 (lane >> 4) + register
  int32_t* out = a.part + ((int64_t)blockIdx.y * bls + bl) * a.n * a.n;
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = ci + wr * 64 + m * 16 + 4 * (lane >> 4) + r, j = cj + wc * 64 + q * 16 + (lane & 15);
        if (i < a.n && j <= i) out[(int64_t)i * a.n + j] = acc[m][q][r];
      }
}

// out[m][i][j] (+)= the slices' entries (max(i, j), min(i, j)), in int64; m over the batches (and labels)
__global__ void __launch_bounds__(256) k_coalloc_join(int64_t mats, int n, int slices, int accumulate, const int32_t* __restrict__ part,
                                                      int64_t* __restrict__ out) {
  const int64_t mat = (int64_t)n * n, total = mats * mat;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = e / mat, w = e - m * mat;
    const int i = (int)(w / n), j = (int)(w - (int64_t)i * n);
    const int64_t src = m * mat + (i < j ? (int64_t)j * n + i : w);
    int64_t s = accumulate ? out[e] : 0;
    for (int k = 0; k < slices; ++k) s += (int64_t)part[(int64_t)k * total + src];
    out[e] = s;
  }
}

struct ScoreArgs {
  const uint8_t* packed;      // [batches][blocks][n][16] of the chunk
  const int64_t* counts;      // [batches][n][n]
  unsigned long long* score;  // [n_iter][C], zeroed
  int64_t R, r0, rows, blocks, rows_per_slice;
  int64_t row_mul, row_add;   // place of row r of batch b in score: r * row_mul + b * row_add
  int n, pairs;
};

__global__ void __launch_bounds__(256) k_partition_score(ScoreArgs a) {
  __shared__ long long W[PS_T][PS_T];
  __shared__ uint4 Z[2 * PS_T][PS_ROWS / 16];  // label bytes [column of the i side, then of the j side][row]
  const int64_t batch = blockIdx.z;
  int t = blockIdx.x, bi = 0;
  while (t >= bi + 1) { t -= bi + 1; ++bi; }
  const int bj = t, ci = bi * PS_T, cj = bj * PS_T, tid = threadIdx.x;
  for (int e = tid; e < PS_T * PS_T; e += 256) {
    const int i = ci + e / PS_T, j = cj + e % PS_T;
    W[e / PS_T][e % PS_T] = (i < a.n && j < i) ? a.R - 2 * a.counts[(batch * a.n + i) * a.n + j] : 0;
  }
  const uint4* packed = (const uint4*)a.packed + batch * a.blocks * a.n;
  const uint8_t* Zb = (const uint8_t*)&Z[0][0];
  const int64_t s0 = (int64_t)blockIdx.y * a.rows_per_slice;
  const int64_t s1 = (s0 + a.rows_per_slice < a.rows) ? s0 + a.rows_per_slice : a.rows;
  for (int64_t r = s0; r < s1; r += PS_ROWS) {  // (r is a multiple of 16: rows_per_slice is one of PS_ROWS)
    __syncthreads();                           // W is written; the labels of the rows before these have been read
    for (int e = tid; e < 2 * PS_T * (PS_ROWS / 16); e += 256) {
      const int col = e & (2 * PS_T - 1), blk = e / (2 * PS_T);
      const int j = col < PS_T ? ci + col : cj + col - PS_T;
      const int64_t b = (r >> 4) + blk;
      Z[col][blk] = (j < a.n && b < a.blocks) ? packed[b * a.n + j] : make_uint4(~0u, ~0u, ~0u, ~0u);
    }
    __syncthreads();
    uint32_t zj[PS_T];
#pragma unroll
    for (int j = 0; j < PS_T; ++j) zj[j] = Zb[(PS_T + j) * PS_ROWS + tid];
    long long sum = 0;
    for (int i = 0; i < PS_T; ++i) {
      const uint32_t zi = Zb[i * PS_ROWS + tid];
      if (zi == 0xFFu) continue;  // (0xFF matches nothing, not even itself)
#pragma unroll
      for (int j = 0; j < PS_T; ++j) sum += (zj[j] == zi) ? W[i][j] : 0ll;
    }
    if (r + tid < s1 && sum != 0) atomicAdd(a.score + (a.r0 + r + tid) * a.row_mul + batch * a.row_add, (unsigned long long)sum);
  }
}

// best[b] = {row of the first minimum of the batch's scores, that score}
__global__ void __launch_bounds__(256) k_partition_best(const int64_t* __restrict__ score, int64_t R, int64_t row_mul, int64_t row_add,
                                                        int64_t* __restrict__ best) {
  __shared__ long long sv[256];
  __shared__ long long sr[256];
  const int64_t batch = blockIdx.x;
  long long bv = 0, br = -1;
  for (int64_t r = threadIdx.x; r < R; r += 256) {
    const long long v = score[r * row_mul + batch * row_add];
    if (br < 0 || v < bv) { bv = v; br = r; }  // (a thread's rows ascend: the first of equals stays)
  }
  sv[threadIdx.x] = bv; sr[threadIdx.x] = br;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      const long long ov = sv[threadIdx.x + w], orow = sr[threadIdx.x + w];
      const long long mv = sv[threadIdx.x], mrow = sr[threadIdx.x];
      if (orow >= 0 && (mrow < 0 || ov < mv || (ov == mv && orow < mrow))) { sv[threadIdx.x] = ov; sr[threadIdx.x] = orow; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { best[batch * 2] = sr[0]; best[batch * 2 + 1] = sv[0]; }
}

// what both entry points ask of their arguments; the text goes to omc_last_error
omc_status coalloc_check(const char* who, omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx,
                         int64_t n_idx, int32_t n_labels, const void* in_or_out) {
  const auto no = [who](const char* text) { return omc_invalid((std::string(who) + ": " + text).c_str()); };
  if (!ctx) return no("no context");
  if (n_iter < 1) return no("n_iter < 1");
  if (size < 1) return no("size < 1");
  if (!store || !in_or_out) return no("store and the counts must not be NULL");
  if (n_idx < 1 || (!idx && n_idx != size)) return no("n_idx < 1, or no index and n_idx != size");
  if (n_labels < 1) return no("n_labels < 1");
  if (n_labels > 64) {
    omc_set_error_text((std::string(who) + ": n_labels > 64").c_str());
    return OMC_UNSUPPORTED;
  }
  if (n_idx > 0x7fffffffLL / 16) return no("more selected elements than one launch takes");
  return OMC_OK;
}

// rows of a chunk: what keeps the packed bytes of all batches within C_CHUNK_BYTES, whole slabs of every Kp, at least one
int64_t coalloc_chunk_rows(const StoreView& v) {
  int64_t rows = C_CHUNK_BYTES / (v.batches * v.n) / CA_SLAB * CA_SLAB;
  if (rows < CA_SLAB) rows = CA_SLAB;
  return rows < v.R ? rows : (v.R + 15) / 16 * 16;
}

// packs rows r0 .. r0 + rows - 1 of the view into ctx->rank_ws (ensured by the caller); flags (zeroed) or NULL
omc_status coalloc_pack(omc_ctx* ctx, const StoreView& v, int64_t r0, int64_t rows, int K, unsigned long long* flags) {
  const int64_t blocks = (rows + 15) / 16, groups = (blocks + 15) / 16;
  const dim3 grid((unsigned)((v.n + 63) / 64), (unsigned)(groups < 65535 ? groups : 65535), (unsigned)v.batches);
  hipLaunchKernelGGL(k_coalloc_pack, grid, dim3(256), 0, ctx->stream, v, r0, rows, blocks, K, (uint4*)ctx->rank_ws.p, flags);
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}

template <int LOGK>
void launch_mfma(dim3 grid, hipStream_t s, const CoallocArgs& a) {
  hipLaunchKernelGGL(k_coalloc_mfma<LOGK>, grid, dim3(256), 0, s, a);
}

}  // namespace

extern "C" omc_status omc_store_coalloc(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx,
                                        int64_t n_idx, int32_t n_labels, int32_t pooled, int32_t per_label, int64_t* counts_out,
                                        int64_t* flags_out) {
  omc_status st = coalloc_check("omc_store_coalloc", ctx, n_iter, size, store, idx, n_idx, n_labels, counts_out);
  if (st != OMC_OK) return st;
  const StoreView v = omc_store_view(ctx, n_iter, size, pooled != 0, store, idx, n_idx);
  if (v.batches > 65535) return omc_invalid("omc_store_coalloc: more chains than one launch takes (65535)");
  const int64_t n = v.n, labels = per_label ? n_labels : 1, mats = v.batches * labels;
  const int64_t tiles = (n + CA_TS - 1) / CA_TS, pairs = tiles * (tiles + 1) / 2;
  if (pairs * mats > 0x7fffffffLL) return omc_invalid("omc_store_coalloc: more tiles than one launch takes");
  int logk = 0;
  if (!per_label)
    while ((1 << logk) < n_labels) ++logk;
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;

  // slices of the rows of a chunk: omc_row_slices over the (batch, label, tile pair) groups, whole slabs of every Kp, and never
  // more than C_SLICE_CAP rows -- every row adds at most 1 to an int32 partial count, so rows < 2^31 cannot overflow it
  const int64_t chunk_rows = coalloc_chunk_rows(v);
  int64_t kchunk;
  omc_row_slices(pairs * mats, chunk_rows, &kchunk);
  kchunk = (kchunk + CA_SLAB - 1) / CA_SLAB * CA_SLAB;
  if (kchunk > C_SLICE_CAP) kchunk = C_SLICE_CAP / CA_SLAB * CA_SLAB;
  const int64_t max_slices = (chunk_rows + kchunk - 1) / kchunk;
  if (max_slices > 65535) return omc_invalid("omc_store_coalloc: more slices than one launch takes");
  const size_t part_bytes = (size_t)max_slices * mats * n * n * sizeof(int32_t);
  st = omc_ensure(ctx, ctx->store_ws, 64 + part_bytes);
  if (st != OMC_OK) return st;
  st = omc_ensure(ctx, ctx->rank_ws, (size_t)v.batches * ((chunk_rows + 15) / 16) * n * 16);
  if (st != OMC_OK) return st;
  st = omc_store_check_index(ctx, (int32_t*)ctx->store_ws.p, idx, n_idx, size);
  if (st == OMC_INVALID_ARG) return omc_invalid("omc_store_coalloc: an index outside [0, size)");  // (the helper's only use of that status)
  if (st != OMC_OK) return st;
  if (flags_out) OMC_HIP_CHECK(hipMemsetAsync(flags_out, 0, (size_t)v.batches * n * 2 * sizeof(int64_t), s));

  CoallocArgs a;
  a.packed = (const uint8_t*)ctx->rank_ws.p;
  a.part = (int32_t*)((char*)ctx->store_ws.p + 64);
  a.kchunk = kchunk; a.n = (int)n; a.pairs = (int)pairs; a.labels = (int)labels;
  int64_t jgrid = (mats * n * n + 255) / 256;
  if (jgrid > 4096) jgrid = 4096;
  for (int64_t r0 = 0; r0 < v.R; r0 += chunk_rows) {
    const int64_t rows = (v.R - r0 < chunk_rows) ? v.R - r0 : chunk_rows;
    st = coalloc_pack(ctx, v, r0, rows, n_labels, (unsigned long long*)flags_out);
    if (st != OMC_OK) return st;
    a.blocks = (rows + 15) / 16;
    a.rows16 = a.blocks * 16;
    const int64_t slices = (a.rows16 + kchunk - 1) / kchunk;
    const dim3 grid((unsigned)(pairs * mats), (unsigned)slices);
    switch (logk) {
      case 0: launch_mfma<0>(grid, s, a); break;
      case 1: launch_mfma<1>(grid, s, a); break;
      case 2: launch_mfma<2>(grid, s, a); break;
      case 3: launch_mfma<3>(grid, s, a); break;
      case 4: launch_mfma<4>(grid, s, a); break;
      case 5: launch_mfma<5>(grid, s, a); break;
      default: launch_mfma<6>(grid, s, a); break;
    }
    OMC_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_coalloc_join, dim3((unsigned)jgrid), dim3(256), 0, s, mats, (int)n, (int)slices, (int)(r0 > 0), a.part, counts_out);
    OMC_HIP_CHECK(hipGetLastError());
  }
  return OMC_OK;
}

extern "C" omc_status omc_store_partition_score(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx,
                                                int64_t n_idx, int32_t n_labels, int32_t pooled, const int64_t* counts,
                                                int64_t* score_out, int64_t* best_out) {
  omc_status st = coalloc_check("omc_store_partition_score", ctx, n_iter, size, store, idx, n_idx, n_labels, counts);
  if (st != OMC_OK) return st;
  if (!score_out || !best_out) return omc_invalid("omc_store_partition_score: score_out and best_out must not be NULL");
  const StoreView v = omc_store_view(ctx, n_iter, size, pooled != 0, store, idx, n_idx);
  if (v.batches > 65535) return omc_invalid("omc_store_partition_score: more chains than one launch takes (65535)");
  const int64_t n = v.n, C = ctx->n_chains;
  // |score| <= pairs of positions x R: kept below 2^62
  if ((unsigned __int128)(n * (n - 1) / 2) * (unsigned __int128)v.R >= ((unsigned __int128)1 << 62)) {
    omc_set_error_text("omc_store_partition_score: n_idx (n_idx - 1) / 2 x rows >= 2^62");
    return OMC_UNSUPPORTED;
  }
  const int64_t tiles = (n + PS_T - 1) / PS_T, pairs = tiles * (tiles + 1) / 2;
  if (pairs > 0x7fffffffLL) return omc_invalid("omc_store_partition_score: more tiles than one launch takes");
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int64_t chunk_rows = coalloc_chunk_rows(v);
  st = omc_ensure(ctx, ctx->store_ws, 64);
  if (st != OMC_OK) return st;
  st = omc_ensure(ctx, ctx->rank_ws, (size_t)v.batches * ((chunk_rows + 15) / 16) * n * 16);
  if (st != OMC_OK) return st;
  st = omc_store_check_index(ctx, (int32_t*)ctx->store_ws.p, idx, n_idx, size);
  if (st == OMC_INVALID_ARG) return omc_invalid("omc_store_partition_score: an index outside [0, size)");  // (the helper's only use of that status)
  if (st != OMC_OK) return st;
  OMC_HIP_CHECK(hipMemsetAsync(score_out, 0, (size_t)n_iter * C * sizeof(int64_t), s));

  ScoreArgs a;
  a.packed = (const uint8_t*)ctx->rank_ws.p;
  a.counts = counts;
  a.score = (unsigned long long*)score_out;
  a.R = v.R; a.n = (int)n; a.pairs = (int)pairs;
  a.row_mul = pooled ? 1 : C;
  a.row_add = pooled ? 0 : 1;
  for (int64_t r0 = 0; r0 < v.R; r0 += chunk_rows) {
    const int64_t rows = (v.R - r0 < chunk_rows) ? v.R - r0 : chunk_rows;
    st = coalloc_pack(ctx, v, r0, rows, n_labels, nullptr);
    if (st != OMC_OK) return st;
    a.r0 = r0; a.rows = rows; a.blocks = (rows + 15) / 16;
    int64_t rps;
    int64_t slices = omc_row_slices(pairs * v.batches, rows, &rps);
    rps = (rps + PS_ROWS - 1) / PS_ROWS * PS_ROWS;
    slices = (rows + rps - 1) / rps;
    a.rows_per_slice = rps;
    hipLaunchKernelGGL(k_partition_score, dim3((unsigned)pairs, (unsigned)slices, (unsigned)v.batches), dim3(256), 0, s, a);
    OMC_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_partition_best, dim3((unsigned)v.batches), dim3(256), 0, s, score_out, v.R, a.row_mul, a.row_add, best_out);
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}
