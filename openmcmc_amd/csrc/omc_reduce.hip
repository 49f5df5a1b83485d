// Per-draw reductions of the device store: one number per stored state (iteration, chain) over the selected elements of its row.
// The contract is in include/omcmc_hip.h (omc_store_reduce).
//
// What it replaces: np.nansum(store[param], axis=0) and kin on MCMC.store[param] of the reference (host arrays there:
// mcmc.py:105-111).  store is [n_iter][C][size]; a ROW is the size contiguous doubles of one (iteration, chain), R = n_iter C rows.
// The store is read once, 8 (16 with the count) bytes are written per row.  Selection position k = 0 .. n_idx - 1 is element
// idx[k] (k itself without an index); a and b are aligned with k.
//
// One accumulator (RedAcc) serves every op: a value, a position and the count of the terms that are not NaN.
//   SUM            value += term.  The only op whose result depends on the order of the operations.
//   COUNT_ABOVE    position += (x > a[k]): an integer count.
//   the others     (value, position) of the best term so far under a total order in which a NaN term -- only met with
//                  omit_nan == 0; otherwise it is dropped before the comparison -- beats every number, and of two equal terms (or
//                  two NaN) the lower position wins.  Positions are unique, so the best pair is the same in whatever order lanes,
//                  waves and forms combine theirs: MIN, MAX, ARGMIN, ARGMAX and SUPNORM are bit-equal between the forms.
// k_reduce_long  one wave per row; rows of RED_SPLIT_MIN selected elements or more are cut into four pieces, one per wave of the
//                workgroup, joined through LDS in piece order.  Without an index a piece is read with 16-byte loads, four in
//                flight per lane: a piece that starts 8 bytes off a 16-byte boundary (every second row of an odd size) gives its
//                first element to lane 0, and a last element without a partner goes to lane 63.  With an index every lane reads
//                idx[k] and gathers 8 bytes.  A lane adds its terms in ascending k, then the 64 lanes are combined by the
//                butterfly 32, 16 .. 1 (a + b == b + a: every lane ends with the same bits).
// k_reduce_short a workgroup copies TR consecutive rows, one flat stream of TR size doubles, into LDS with coalesced 16-byte loads
//                (head and tail as above) at a row pitch that keeps G lanes per row free of bank conflicts, G a power of two with
//                at most 16 selected elements per lane: lane g of a row takes k = g, g + G, .. in ascending order from LDS (under
//                an index at idx[k]), and the G lanes are combined by the butterfly G / 2 .. 1.
// The order of the additions of SUM therefore depends on the form, on (size, n_idx) -- through G, the pieces and the lane of
// every k -- and, in the long form without an index, on whether the row starts on a 16-byte boundary: on nothing that differs
// between two calls with the same arguments.  No atomics of any kind, no scratch.
#include "omc_common.h"
#include "omc_store_view.h"

namespace {

constexpr int RED_THREADS = 256;
constexpr int RED_LDS_BUDGET = 48 * 1024;   // k_reduce_short: bytes of a workgroup's tile at most
constexpr int64_t RED_SPLIT_MIN = 32768;    // k_reduce_long: selected elements from which a row is cut over the four waves
constexpr int64_t RED_SHORT_AUTO = 128;     // reduce_algo 0: rows of up to this many elements take the short form (profiles/store_derive.txt)
constexpr int64_t RED_NONE = 0x7fffffffffffffffLL;  // the position of "no term yet"

struct RedArgs {
  const double* store; const int64_t* idx; const double* a; const double* b;
  double* out; int64_t* count_out;
  int64_t R, size, n_idx;
  int32_t omit_nan, wpr;     // long form: waves per row, 1 or 4
  int32_t G, TR, pitch;      // short form: lanes per row, rows of a tile, doubles between two rows in LDS
};

template <int OP>
struct RedAcc {
  static constexpr bool kSum = OP == OMC_REDUCE_SUM, kCount = OP == OMC_REDUCE_COUNT_ABOVE, kExt = !kSum && !kCount;
  static constexpr bool kUp = OP == OMC_REDUCE_MAX || OP == OMC_REDUCE_ARGMAX || OP == OMC_REDUCE_SUPNORM;
  static constexpr bool kNeedA = kSum || kCount || OP == OMC_REDUCE_SUPNORM, kNeedB = OP == OMC_REDUCE_SUPNORM;
  double v;
  int64_t pos, cnt;

  __device__ __forceinline__ void init() { v = 0.0; pos = kExt ? RED_NONE : 0; cnt = 0; }

  // does (t2, p2) come before (t, p)?  p2 is a real position
  static __device__ __forceinline__ bool before(double t2, int64_t p2, double t, int64_t p) {
    if (p == RED_NONE) return true;
    const bool n2 = t2 != t2, n1 = t != t;
    if (n1 || n2) return n2 && (!n1 || p2 < p);
    return kUp ? (t2 > t || (t2 == t && p2 < p)) : (t2 < t || (t2 == t && p2 < p));
  }

  // element x at selection position k; a == NULL (SUM only): the term is x
  __device__ __forceinline__ void add(double x, int64_t k, const double* __restrict__ a, const double* __restrict__ b, bool omit) {
    double t = x;
    if (kSum && a) t = a[k] * x;
    if (OP == OMC_REDUCE_SUPNORM) t = __ddiv_rn(fabs(__dsub_rn(x, a[k])), b[k]);  // one rounded subtraction, one rounded division
    const bool ok = t == t;
    cnt += ok ? 1 : 0;
    if (kCount) {
      pos += (x > a[k]) ? 1 : 0;
    } else if (ok || !omit) {
      if (kSum) v += t;
      else if (before(t, k, v, pos)) { v = t; pos = k; }
    }
  }

  __device__ __forceinline__ void merge(double v2, int64_t p2, int64_t c2) {
    cnt += c2;
    if (kSum) v += v2;
    else if (kCount) pos += p2;
    else if (p2 != RED_NONE && before(v2, p2, v, pos)) { v = v2; pos = p2; }
  }

  // the butterfly over aligned groups of `width` lanes (a power of two up to 64): every lane of a group ends with the group's result
  __device__ __forceinline__ void combine(int width) {
    for (int j = width >> 1; j >= 1; j >>= 1) {
      const double v2 = __shfl_xor(v, j, 64);
      const int64_t p2 = (int64_t)__shfl_xor((unsigned long long)pos, j, 64);
      const int64_t c2 = (int64_t)__shfl_xor((unsigned long long)cnt, j, 64);
      merge(v2, p2, c2);
    }
  }

  __device__ __forceinline__ double result() const {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if (kSum) return v;
    if (kCount) return (double)pos;
    if (pos == RED_NONE) return nan;
    return (OP == OMC_REDUCE_ARGMIN || OP == OMC_REDUCE_ARGMAX) ? (double)pos : v;
  }
};

template <int OP>
__device__ __forceinline__ void red_write(const RedArgs& g, int64_t r, const RedAcc<OP>& acc) {
  g.out[r] = acc.result();
  if (g.count_out) g.count_out[r] = acc.cnt;
}

// workgroup b, wave w: piece (4 b + w) % wpr of row (4 b + w) / wpr
template <int OP, bool IDX>
__global__ void __launch_bounds__(RED_THREADS) k_reduce_long(RedArgs g) {
  __shared__ double sv[RED_THREADS / 64];
  __shared__ int64_t sp[RED_THREADS / 64], sc[RED_THREADS / 64];
  typedef RedAcc<OP> Acc;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t piece = (int64_t)blockIdx.x * (RED_THREADS / 64) + w;
  const int64_t r = piece / g.wpr;
  const int part = (int)(piece - r * g.wpr);
  const bool omit = g.omit_nan != 0;
  const double* __restrict__ a = Acc::kNeedA ? g.a : nullptr;
  const double* __restrict__ b = Acc::kNeedB ? g.b : nullptr;
  Acc acc;
  acc.init();
  if (r < g.R) {
    const int64_t per = ((g.n_idx + g.wpr - 1) / g.wpr + 1) & ~(int64_t)1;  // selected elements of a piece, even
    const int64_t k0 = part * per, k1 = k0 + per < g.n_idx ? k0 + per : g.n_idx;  // (k0 >= k1: nothing left for this piece)
    const double* __restrict__ row = g.store + r * g.size;
    if (IDX) {
      for (int64_t kb = k0; kb < k1; kb += 4 * 64) {
        double x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int64_t k = kb + 64 * u + lane;
          x[u] = k < k1 ? row[g.idx[k]] : 0.0;  // 0 <= idx[k] < size: checked before the launch
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int64_t k = kb + 64 * u + lane;
          if (k < k1) acc.add(x[u], k, a, b, omit);
        }
      }
    } else if (k0 < k1) {  // n_idx == size: position k is element k
      const double* p = row + k0;
      const int64_t n = k1 - k0;
      const int64_t head = ((uintptr_t)p & 8) ? 1 : 0;
      if (head && lane == 0) acc.add(p[0], k0, a, b, omit);
      const double2* __restrict__ q = (const double2*)(p + head);
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
            const int64_t k = k0 + head + 2 * j;
            acc.add(x[u].x, k, a, b, omit);
            acc.add(x[u].y, k + 1, a, b, omit);
          }
        }
      }
      if (((n - head) & 1) && lane == 63) acc.add(p[n - 1], k1 - 1, a, b, omit);
    }
  }
  acc.combine(64);
  if (g.wpr == 1) {
    if (r < g.R && lane == 0) red_write(g, r, acc);
    return;
  }
  // wpr == 4: the four waves of the workgroup hold the four pieces of one row
  if (lane == 0) { sv[w] = acc.v; sp[w] = acc.pos; sc[w] = acc.cnt; }
  __syncthreads();
  if (threadIdx.x == 0 && r < g.R) {
    for (int q = 1; q < RED_THREADS / 64; ++q) acc.merge(sv[q], sp[q], sc[q]);
    red_write(g, r, acc);
  }
}

// workgroup b: rows [b TR, b TR + TR)
template <int OP>
__global__ void __launch_bounds__(RED_THREADS) k_reduce_short(RedArgs g) {
  extern __shared__ double red_lds[];
  typedef RedAcc<OP> Acc;
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * g.TR;
  const int n_rows = g.R - row0 < g.TR ? (int)(g.R - row0) : g.TR;
  const int size = (int)g.size, pitch = g.pitch;
  const bool omit = g.omit_nan != 0;
  {  // the tile: n = n_rows size doubles from p (n <= RED_LDS_BUDGET / 8), flat element e to LDS row e / size
    const double* __restrict__ p = g.store + row0 * g.size;
    const int n = n_rows * size;
    const int head = ((uintptr_t)p & 8) ? 1 : 0;
    if (head && tid == 0) red_lds[0] = p[0];
    const double2* __restrict__ q = (const double2*)(p + head);
    const int n_pairs = (n - head) >> 1;
    for (int j = tid; j < n_pairs; j += RED_THREADS) {
      const double2 x = q[j];
      const int e = head + 2 * j;  // e + 1 < n
      int rw = e / size, col = e - rw * size;
      red_lds[rw * pitch + col] = x.x;
      if (++col == size) { col = 0; ++rw; }
      red_lds[rw * pitch + col] = x.y;
    }
    if (((n - head) & 1) && tid == RED_THREADS - 1) red_lds[(n_rows - 1) * pitch + size - 1] = p[n - 1];
  }
  __syncthreads();
  const int G = g.G, t = tid / G, sub = tid & (G - 1);
  const double* __restrict__ a = Acc::kNeedA ? g.a : nullptr;
  const double* __restrict__ b = Acc::kNeedB ? g.b : nullptr;
  Acc acc;
  acc.init();
  if (t < n_rows) {
    const double* s = red_lds + t * pitch;
    for (int64_t k = sub; k < g.n_idx; k += G) acc.add(s[g.idx ? g.idx[k] : k], k, a, b, omit);
  }
  acc.combine(G);
  if (t < n_rows && sub == 0) red_write(g, row0 + t, acc);
}

template <int OP>
void red_launch(omc_ctx* ctx, const RedArgs& g, bool short_form) {
  if (short_form) {
    const int64_t tiles = (g.R + g.TR - 1) / g.TR;
    hipLaunchKernelGGL(k_reduce_short<OP>, dim3((unsigned)tiles), dim3(RED_THREADS), (size_t)g.TR * g.pitch * sizeof(double), ctx->stream, g);
    return;
  }
  const int64_t blocks = (g.R * g.wpr + RED_THREADS / 64 - 1) / (RED_THREADS / 64);
  if (g.idx) hipLaunchKernelGGL((k_reduce_long<OP, true>), dim3((unsigned)blocks), dim3(RED_THREADS), 0, ctx->stream, g);
  else hipLaunchKernelGGL((k_reduce_long<OP, false>), dim3((unsigned)blocks), dim3(RED_THREADS), 0, ctx->stream, g);
}

}  // namespace

extern "C" omc_status omc_store_reduce(omc_ctx* ctx, int64_t n_iter, int64_t size, const double* store, const int64_t* idx, int64_t n_idx,
                                       int32_t op, int32_t omit_nan, const double* a, const double* b, double* out, int64_t* count_out) {
  if (!ctx) return omc_invalid("omc_store_reduce: no context");
  if (n_iter < 1) return omc_invalid("omc_store_reduce: n_iter < 1");
  if (size < 1) return omc_invalid("omc_store_reduce: size < 1");
  if (!store || !out) return omc_invalid("omc_store_reduce: store and out must not be NULL");
  if (n_idx < 1 || (!idx && n_idx != size)) return omc_invalid("omc_store_reduce: n_idx < 1, or no index and n_idx != size");
  if (op < OMC_REDUCE_SUM || op > OMC_REDUCE_SUPNORM) return omc_invalid("omc_store_reduce: unknown op");
  if (op == OMC_REDUCE_COUNT_ABOVE && !a) return omc_invalid("omc_store_reduce: COUNT_ABOVE needs the thresholds a");
  if (op == OMC_REDUCE_SUPNORM && (!a || !b)) return omc_invalid("omc_store_reduce: SUPNORM needs the centres a and the scales b");
  OMC_HIP_CHECK(hipSetDevice(ctx->device));
  const omc_status st = omc_store_check_index(ctx, nullptr, idx, n_idx, size);
  if (st == OMC_INVALID_ARG) return omc_invalid("omc_store_reduce: an index outside [0, size)");  // (the helper's only use of that status)
  if (st != OMC_OK) return st;
  const StoreView v = omc_store_view(ctx, n_iter, size, true, store, idx, n_idx);  // pooled: R rows of row_stride = size doubles
  const int64_t R = v.R;
  RedArgs g;
  g.store = v.data; g.idx = v.idx; g.a = a; g.b = b; g.out = out; g.count_out = count_out;
  g.R = R; g.size = v.row_stride; g.n_idx = v.n; g.omit_nan = omit_nan != 0;
  g.wpr = n_idx >= RED_SPLIT_MIN ? RED_THREADS / 64 : 1;
  // short form: G lanes per row, at most 16 selected elements each; the pitch is the first p >= size with p = G (mod 2 G), so
  // that the 32 / G rows of half a wave start on different multiples of G of the 32 eight-byte banks (from G = 32 on half a wave
  // reads one row: any pitch)
  int64_t G = 1;
  while (G < 64 && G * 16 < n_idx) G <<= 1;
  int64_t pitch = size;
  if (G < 32) pitch = size + ((G - size % (2 * G)) + 2 * G) % (2 * G);
  int64_t TR = RED_LDS_BUDGET / (pitch * (int64_t)sizeof(double));
  if (TR > RED_THREADS / G) TR = RED_THREADS / G;
  g.G = (int32_t)G; g.TR = (int32_t)TR; g.pitch = (int32_t)pitch;
  // rows beyond the LDS budget take the long form whatever the option says
  const bool short_form = TR >= 1 && (ctx->reduce_algo == 1 || (ctx->reduce_algo == 0 && size <= RED_SHORT_AUTO));
  const int64_t blocks = short_form ? (R + TR - 1) / TR : (R * g.wpr + RED_THREADS / 64 - 1) / (RED_THREADS / 64);
  if (blocks > 0x7fffffffLL) return omc_invalid("omc_store_reduce: more rows than one launch takes");
  switch (op) {
    case OMC_REDUCE_SUM: red_launch<OMC_REDUCE_SUM>(ctx, g, short_form); break;
    case OMC_REDUCE_MIN: red_launch<OMC_REDUCE_MIN>(ctx, g, short_form); break;
    case OMC_REDUCE_MAX: red_launch<OMC_REDUCE_MAX>(ctx, g, short_form); break;
    case OMC_REDUCE_ARGMIN: red_launch<OMC_REDUCE_ARGMIN>(ctx, g, short_form); break;
    case OMC_REDUCE_ARGMAX: red_launch<OMC_REDUCE_ARGMAX>(ctx, g, short_form); break;
    case OMC_REDUCE_COUNT_ABOVE: red_launch<OMC_REDUCE_COUNT_ABOVE>(ctx, g, short_form); break;
    default: red_launch<OMC_REDUCE_SUPNORM>(ctx, g, short_form); break;
  }
  OMC_HIP_CHECK(hipGetLastError());
  return OMC_OK;
}
