// First failures of the stored states against up to eight slots of per-element sides: the counts behind joint excursion sets,
// contour-avoiding sets and the reliability of a contour map (Bolin and Lindgren 2015, 2017).
// The contract is in include/omcmc_hip.h (omc_store_first_failure).
//
// store is [n_iter][C][size]; a ROW is the size contiguous doubles of one (iteration, chain), R = n_iter C rows.  Selection
// position k = 0 .. n - 1 is element idx[k] (k itself without an index).  Slot l has lo[l][k], hi[l][k] (fp64) and pos[l][k] (int32):
// row s AGREES at k iff x == x && (lo == -inf || x > lo) && (hi == +inf || x < hi), and its first failure is
// r = min({pos[l][k] : s does not agree at k} u {n}).  h[l][j] counts the rows with r == j.  The store is read once for all slots.
//
// One state (FfMin) serves both forms: LT running int32 minima per lane, LT the number of slots rounded up to 1, 2, 4 or 8 (the
// slots beyond the call's are skipped by a uniform branch), joined over lanes by a butterfly of integer min.  An integer minimum
// does not depend on how the elements are cut over lanes, so both forms and every call give the same r, and h is added with
// integer atomics only: no floating point reaches a result.
//   k_ff_long    a workgroup owns FF_ROWS = 32 consecutive rows, a wave FF_ROWS / 4 of them one after the other (the four waves
//                walk four adjacent rows at a time).  Without an index a row is read with 16-byte loads, four in flight per lane:
//                a row that starts 8 bytes off a 16-byte boundary (every second row of an odd size) gives its first element to
//                lane 0, and a last element without a partner goes to lane 63.  With an index every lane reads idx[k] and gathers
//                8 bytes.
//   k_ff_short   a workgroup copies TR consecutive rows, one flat stream of TR size doubles, into LDS with coalesced 16-byte loads
//                (head and tail as above) at the row pitch of k_reduce_short (omc_reduce.hip), G lanes per row with at most 16
//                selected elements each.
// The slot tables (20 L bytes per selected element: 1.6 MB at n = 10 000, L = 8) are read through the caches in both forms, not
// staged in LDS.  A wave needs the tables of the WHOLE row, which no workgroup's LDS holds at that size; staging a column tile of
// them would turn the row's minimum into a join across workgroups.  As they are, the tables fit every XCD's 4 MiB L2 beside the
// streamed rows, the four waves of a workgroup walk the same k at about the same time (one L1 line serves them), and the short
// form's tables (at most a few KB) stay in L1.
// ff_flush     what both forms end a tile of rows with: the tile's r values lie in LDS as [row][LT]; thread (row, l) writes r where
//              asked for, and the FIRST of equal values within a group of 32 rows adds their number to h[l][r] with one integer
//              atomic (most rows of a real field share one value, n or a small one: one atomic per group and value, not one per
//              row).  The long form adds to the output.  The short form, where L (n + 1) <= FF_HIST_LDS, keeps the whole h in LDS
//              counters and adds the ones that are not zero to the output when it has walked its last tile, and it is launched
//              with at most eight workgroups per compute unit, each walking the tiles b, b + grid, ..: short rows have at most
//              n + 1 distinct values of r, and a million rows adding to the output queue on a handful of addresses (measured: five
//              times the kernel's time at 2000 x 512 x 20).  The long form gains nothing from either: as tile-walking workgroups it
//              took 4.26 ms instead of 3.68 ms on the 10 000-node store (profiles/store_excursion.txt).
// No scratch (tests/test_excursion_kernel_resources.py).
#include "omc_common.h"
#include "omc_store_view.h"

namespace {

constexpr int FF_THREADS = 256;
constexpr int FF_ROWS = 32;                // k_ff_long: rows of a workgroup; ff_flush: rows of a group
constexpr int FF_LDS_BUDGET = 40 * 1024;   // k_ff_short: bytes of a workgroup's tile at most (beside 8 KiB of r and 8 KiB of counters)
constexpr int FF_HIST_LDS = 2048;          // the counters of h that a workgroup keeps in LDS, at most
constexpr int64_t FF_SHORT_AUTO = 128;     // algo 0: rows of up to this many elements take the short form (omc_reduce.hip's crossover)
constexpr int FF_MAX_SLOTS = 8;

struct FfArgs {
  const double* store; const int64_t* idx; const double* lo; const double* hi; const int32_t* pos;
  unsigned long long* h; int32_t* rows_out;
  int64_t R, size, n, tiles;  // tiles: the short form's sets of TR rows
  int32_t L;
  int32_t G, TR, pitch;      // short form: lanes per row, rows of a tile, doubles between two rows in LDS
};

template <int LT>
struct FfMin {
  int32_t m[LT];

  __device__ __forceinline__ void init(int32_t n) {
#pragma unroll
    for (int l = 0; l < LT; ++l) m[l] = n;
  }

  // element x at selection position k < n
  __device__ __forceinline__ void add(const FfArgs& g, double x, int64_t k) {
    const double inf = __builtin_inf();
#pragma unroll
    for (int l = 0; l < LT; ++l) {
      if (l < g.L) {
        const int64_t j = l * g.n + k;
        const double lo = g.lo[j], hi = g.hi[j];
        const bool agree = x == x && (lo == -inf || x > lo) && (hi == inf || x < hi);
        if (!agree) {
          const int32_t p = g.pos[j];  // 0 <= p < n: checked before the launch
          m[l] = p < m[l] ? p : m[l];
        }
      }
    }
  }

  // the butterfly over aligned groups of `width` lanes (a power of two up to 64): every lane of a group ends with the group's minima
  __device__ __forceinline__ void combine(int width) {
    for (int j = width >> 1; j >= 1; j >>= 1) {
#pragma unroll
      for (int l = 0; l < LT; ++l) {
        const int32_t o = __shfl_xor(m[l], j, 64);
        m[l] = o < m[l] ? o : m[l];
      }
    }
  }

  __device__ __forceinline__ void put(int32_t* __restrict__ s) const {
#pragma unroll
    for (int l = 0; l < LT; ++l) s[l] = m[l];
  }
};

// sr [n_rows][LT] in LDS, complete (a barrier lies behind the caller's writes): row row0 + i, slot l < L; hl: the LDS counters or NULL
template <int LT>
__device__ __forceinline__ void ff_flush(const FfArgs& g, const int32_t* __restrict__ sr, unsigned* __restrict__ hl, int64_t row0, int n_rows) {
  const int L = g.L;
  for (int e = threadIdx.x; e < n_rows * L; e += FF_THREADS) {
    const int i = e / L, l = e - i * L;
    const int32_t v = sr[i * LT + l];  // 0 <= v <= n
    if (g.rows_out) g.rows_out[l * g.R + row0 + i] = v;
    const int i0 = i & ~(FF_ROWS - 1), i1 = i0 + FF_ROWS < n_rows ? i0 + FF_ROWS : n_rows;
    bool first = true;
    for (int q = i0; q < i; ++q) first = first && sr[q * LT + l] != v;
    if (first) {
      unsigned long long cnt = 1;
      for (int q = i + 1; q < i1; ++q) cnt += sr[q * LT + l] == v ? 1 : 0;
      if (hl) atomicAdd(hl + l * (int)(g.n + 1) + v, (unsigned)cnt);
      else atomicAdd(g.h + l * (g.n + 1) + v, cnt);
    }
  }
}

__device__ __forceinline__ bool ff_hist_in_lds(const FfArgs& g) { return (int64_t)g.L * (g.n + 1) <= FF_HIST_LDS; }

__device__ __forceinline__ void ff_hist_zero(const FfArgs& g, unsigned* __restrict__ hl) {
  for (int e = threadIdx.x; e < g.L * (int)(g.n + 1); e += FF_THREADS) hl[e] = 0;  // (the first flush lies behind a barrier)
}

// after the barrier behind the last flush: h is [L][n + 1], as the counters are
__device__ __forceinline__ void ff_hist_add(const FfArgs& g, const unsigned* __restrict__ hl) {
  for (int e = threadIdx.x; e < g.L * (int)(g.n + 1); e += FF_THREADS)
    if (hl[e]) atomicAdd(g.h + e, (unsigned long long)hl[e]);
}

// workgroup b: rows [b FF_ROWS, b FF_ROWS + FF_ROWS); wave w takes the rows w, w + 4, ..
template <int LT, bool IDX>
__global__ void __launch_bounds__(FF_THREADS) k_ff_long(FfArgs g) {
  __shared__ int32_t sr[FF_ROWS * LT];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t n = g.n;
  const int64_t row0 = (int64_t)blockIdx.x * FF_ROWS;
  const int n_rows = g.R - row0 < FF_ROWS ? (int)(g.R - row0) : FF_ROWS;
  for (int i = w; i < n_rows; i += FF_THREADS / 64) {
    const double* __restrict__ row = g.store + (row0 + i) * g.size;
    FfMin<LT> acc;
    acc.init((int32_t)n);
    if (IDX) {
      for (int64_t kb = 0; kb < n; kb += 4 * 64) {
        double x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int64_t k = kb + 64 * u + lane;
          x[u] = k < n ? row[g.idx[k]] : 0.0;  // 0 <= idx[k] < size: checked before the launch
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int64_t k = kb + 64 * u + lane;
          if (k < n) acc.add(g, x[u], k);
        }
      }
    } else {  // n == size: position k is element k
      const int64_t head = ((uintptr_t)row & 8) ? 1 : 0;
      if (head && lane == 0) acc.add(g, row[0], 0);
      const double2* __restrict__ q = (const double2*)(row + head);
      const int64_t n_pairs = (n - head) >> 1;
      for (int64_t jb = 0; jb < n_pairs; jb += 4 * 64) {
        double2 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int64_t j = jb + 64 * u + lane;
          x[u] = j < n_pairs ? q[j] : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int64_t j = jb + 64 * u + lane;
          if (j < n_pairs) {
            const int64_t k = head + 2 * j;  // k + 1 < n
            acc.add(g, x[u].x, k);
            acc.add(g, x[u].y, k + 1);
          }
        }
      }
      if (((n - head) & 1) && lane == 63) acc.add(g, row[n - 1], n - 1);
    }
    acc.combine(64);
    if (lane == 0) acc.put(sr + i * LT);
  }
  __syncthreads();
  ff_flush<LT>(g, sr, nullptr, row0, n_rows);
}

// tile t: rows [t TR, t TR + TR), TR <= FF_THREADS / G
template <int LT>
__global__ void __launch_bounds__(FF_THREADS) k_ff_short(FfArgs g) {
  extern __shared__ double ff_lds[];
  __shared__ int32_t sr[FF_THREADS * LT];
  __shared__ unsigned hist[FF_HIST_LDS];
  unsigned* hl = ff_hist_in_lds(g) ? hist : nullptr;
  if (hl) ff_hist_zero(g, hl);
  const int tid = threadIdx.x;
  const int size = (int)g.size, pitch = g.pitch;
  for (int64_t tile = blockIdx.x; tile < g.tiles; tile += gridDim.x) {
  const int64_t row0 = tile * g.TR;
  const int n_rows = g.R - row0 < g.TR ? (int)(g.R - row0) : g.TR;
  {  // the tile: n = n_rows size doubles from p (n <= FF_LDS_BUDGET / 8), flat element e to LDS row e / size
    const double* __restrict__ p = g.store + row0 * g.size;
    const int n = n_rows * size;
    const int head = ((uintptr_t)p & 8) ? 1 : 0;
    if (head && tid == 0) ff_lds[0] = p[0];
    const double2* __restrict__ q = (const double2*)(p + head);
    const int n_pairs = (n - head) >> 1;
    for (int j = tid; j < n_pairs; j += FF_THREADS) {
      const double2 x = q[j];
      const int e = head + 2 * j;  // e + 1 < n
      int rw = e / size, col = e - rw * size;
      ff_lds[rw * pitch + col] = x.x;
      if (++col == size) { col = 0; ++rw; }
      ff_lds[rw * pitch + col] = x.y;
    }
    if (((n - head) & 1) && tid == FF_THREADS - 1) ff_lds[(n_rows - 1) * pitch + size - 1] = p[n - 1];
  }
  __syncthreads();
  const int G = g.G, t = tid / G, sub = tid & (G - 1);
  FfMin<LT> acc;
  acc.init((int32_t)g.n);
  if (t < n_rows) {
    const double* s = ff_lds + t * pitch;
    for (int64_t k = sub; k < g.n; k += G) acc.add(g, s[g.idx ? g.idx[k] : k], k);
  }
  acc.combine(G);
  if (t < n_rows && sub == 0) acc.put(sr + t * LT);
  __syncthreads();
  ff_flush<LT>(g, sr, hl, row0, n_rows);
  __syncthreads();  // the tile and sr are written again
  }
  if (hl) ff_hist_add(g, hl);
}

// sets the word if an entry of pos [count] lies outside [0, n)
__global__ void k_ff_check_pos(const int32_t* __restrict__ pos, int64_t count, int64_t n, int32_t* __restrict__ word) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < count && (pos[j] < 0 || pos[j] >= n)) *word = 1;
}

template <int LT>
void ff_launch(omc_ctx* ctx, const FfArgs& g, bool short_form, int64_t blocks) {
  if (short_form)
    hipLaunchKernelGGL(k_ff_short<LT>, dim3((unsigned)blocks), dim3(FF_THREADS), (size_t)g.TR * g.pitch * sizeof(double), ctx->stream, g);
  else if (g.idx)
    hipLaunchKernelGGL((k_ff_long<LT, true>), dim3((unsigned)blocks), dim3(FF_THREADS), 0, ctx->stream, g);
  else
    hipLaunchKernelGGL((k_ff_long<LT, false>), dim3((unsigned)blocks), dim3(FF_THREADS), 0, ctx->stream, g);
}

}  // namespace

extern "C" omc_status omc_store_first_failure(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx,
                                              int64_t n_idx, int32_t n_slots, const double* lo, const double* hi, const int32_t* pos,
                                              int32_t algo, int64_t* h_out, int32_t* rows_out) {
  if (!ctx) return omc_invalid("omc_store_first_failure: no context");
  if (n_iter < 1) return omc_invalid("omc_store_first_failure: n_iter < 1");
  if (size < 1) return omc_invalid("omc_store_first_failure: size < 1");
  if (!store || !lo || !hi || !pos || !h_out) return omc_invalid("omc_store_first_failure: store, lo, hi, pos and h_out must not be NULL");
  if (n_idx < 1 || (!idx && n_idx != size)) return omc_invalid("omc_store_first_failure: n_idx < 1, or no index and n_idx != size");
  if (n_idx > 0x7ffffffeLL) return omc_invalid("omc_store_first_failure: more selected elements than an int32 position takes");
  if (n_slots < 1 || n_slots > FF_MAX_SLOTS) return omc_invalid("omc_store_first_failure: n_slots outside 1 .. 8");
  if (algo < 0 || algo > 2) return omc_invalid("omc_store_first_failure: algo outside 0 .. 2");
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  const StoreView v = omc_store_view(ctx, n_iter, size, true, store, idx, n_idx);  // pooled: R rows of row_stride = size doubles
  const int64_t R = v.R, n = v.n, count = (int64_t)n_slots * n;

  FfArgs g;
  g.store = v.data; g.idx = v.idx; g.lo = lo; g.hi = hi; g.pos = pos;
  g.h = (unsigned long long*)h_out; g.rows_out = rows_out;
  g.R = R; g.size = v.row_stride; g.n = n; g.L = n_slots;
  // short form: the geometry of k_reduce_short (omc_reduce.hip) -- G lanes per row, at most 16 selected elements each; the pitch is
  // the first p >= size with p = G (mod 2 G), so that the 32 / G rows of half a wave start on different multiples of G of the 32
  // eight-byte banks (from G = 32 on half a wave reads one row: any pitch)
  int64_t G = 1;
  while (G < 64 && G * 16 < n) G <<= 1;
  int64_t pitch = size;
  if (G < 32) pitch = size + ((G - size % (2 * G)) + 2 * G) % (2 * G);
  int64_t TR = FF_LDS_BUDGET / (pitch * (int64_t)sizeof(double));
  if (TR > FF_THREADS / G) TR = FF_THREADS / G;
  g.G = (int32_t)G; g.TR = (int32_t)TR; g.pitch = (int32_t)pitch;
  // rows beyond the LDS budget take the long form whatever algo says
  const bool short_form = TR >= 1 && (algo == 1 || (algo == 0 && size <= FF_SHORT_AUTO));
  g.tiles = short_form ? (R + TR - 1) / TR : (R + FF_ROWS - 1) / FF_ROWS;
  const int64_t most = 8 * (int64_t)(ctx->dev_cus > 0 ? ctx->dev_cus : 1);
  const int64_t blocks = short_form && g.tiles > most ? most : g.tiles;  // the short form walks its tiles
  if (blocks > 0x7fffffffLL || (count + 255) / 256 > 0x7fffffffLL) return omc_invalid("omc_store_first_failure: more rows than one launch takes");

  // one word, one read-back: the index and the positions, before anything is written
  omc_status st = omc_ensure(ctx, ctx->store_ws, 64);
  if (st != OMC_OK) return st;
  int32_t* word = (int32_t*)ctx->store_ws.p;
  st = omc_words_zero(ctx, word, 2);
  if (st != OMC_OK) return st;
  omc_store_check_index_launch(ctx, idx, n_idx, size, nullptr, 0, 0, word);
  hipLaunchKernelGGL(k_ff_check_pos, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, pos, count, n, word + 1);
  int32_t got[2] = {0, 0};
  st = omc_words_read(ctx, word, 2, got);
  if (st != OMC_OK) return st;
  if (got[0]) return omc_invalid("omc_store_first_failure: an index outside [0, size)");
  if (got[1]) return omc_invalid("omc_store_first_failure: a pos entry outside [0, n_idx)");

  OMC_HIP_CHECK(hipMemsetAsync(h_out, 0, (size_t)n_slots * (n + 1) * sizeof(int64_t), ctx->stream));
  if (n_slots == 1) ff_launch<1>(ctx, g, short_form, blocks);
  else if (n_slots == 2) ff_launch<2>(ctx, g, short_form, blocks);
  else if (n_slots <= 4) ff_launch<4>(ctx, g, short_form, blocks);
  else ff_launch<8>(ctx, g, short_form, blocks);
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}
