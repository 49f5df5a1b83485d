// What the store summaries that need every order statistic of a column share (omc_rank.hip: ranks and the rank-normalised
// diagnostics; omc_hdi.hip: highest-density intervals; omc_essq.hip: indicator ESS and order statistics; omc_psis.hip and
// omc_loo_expect.hip: the importance ratios).  Inline on the device: the key of a draw, the gather of a tile of draws into columns
// of keys, the bisection in a sorted column.  On the host: the geometry of a whole or split column (RankGeom) and the cursor that
// sizes and carves ctx->rank_ws for a chunk (RankCarve).  Compiled once, in omc_store_shared.hip: the gather of such columns
// (k_rank_gather behind rank_gather_sort) and the sort itself:
//
//   k_rank_sort_tile / k_rank_sort_global
//                  a bitonic network over every column, keys only.  Its addressing depends on P and the tile T alone, never on
//                  the data.  Stage k (k = 2, 4, .. P) compare-exchanges at strides j = k / 2 .. 1, ascending where the
//                  position within the column has bit k clear.  Strides inside a tile of T keys run in LDS, one workgroup per
//                  tile: the first launch sorts every tile (all stages up to T), and each later stage ends in one launch that
//                  does its strides T / 2 .. 1; strides of 64 and more go through LDS with a barrier per stride, the last six
//                  (32 .. 1) stay inside a wave, a key per lane exchanged by __shfl_xor.  Every stride >= T is one pass over
//                  global memory.  rank_schedule() lists the launches; rank_sort() walks that list and
//                  omc_store_rank_schedule hands it to the tests, which replay it in numpy.
//
// Kc: what fits RANK_BUDGET = 1 GiB (a choice, not a measurement: large enough for a few hundred elements of a store with a
// million pooled draws, small beside the store) at the caller's bytes per element, at least 1; option "rank_chunk" forces it.
#pragma once
#include <vector>

#include "omc_common.h"
#include "omc_quantile.h"

constexpr size_t RANK_BUDGET = (size_t)1 << 30;
constexpr int64_t RANK_KC_MAX = (int64_t)1 << 17;  // elements of a chunk at most (grid.y of k_rank_emit: Kc / 4)
constexpr int RANK_TILE_DEFAULT = 8192;            // keys of an LDS tile: 64 KiB
constexpr int RANK_G_TE = 16, RANK_G_TS = 64;      // rank_gather_tile: elements x draws of a workgroup's tile
constexpr size_t RANK_HEAD = 64;                   // bytes in front of the per-element arrays of ctx->rank_ws: the word of the index check

struct RankLaunch { int64_t kind, k, j; };  // kind 0: sort every tile (stages 2 .. k); 1: global pass (k, j); 2: tile strides j .. 1 of stage k

inline int64_t rank_pow2(int64_t S) {
  int64_t P = 1;
  while (P < S) P <<= 1;
  return P;
}

// The layout of a column's draws for k_rank_gather: draw s of a column (s < S) is row s of the store seen as [N C][size] when
// s < first, else row s + skip -- the two halves of a split store --, and the middle row of an odd N (rows [mid_row0, mid_row0 + C),
// mid_row0 < 0: none) is read for its NaN / inf only.
struct RankGeom { int64_t S, P, first, skip, mid_row0; };
inline RankGeom rank_geom(int64_t N, int64_t C, bool split) {
  RankGeom g;
  const int64_t M = N / 2;
  g.S = split ? 2 * C * M : N * C;
  g.P = rank_pow2(g.S);
  g.first = split ? M * C : g.S;
  g.skip = split ? (N - 2 * M) * C : 0;
  g.mid_row0 = (split && (N & 1)) ? M * C : -1;
  return g;
}

// omc_store_shared.hip
std::vector<RankLaunch> rank_schedule(int64_t P, int64_t T);              // the launches that sort columns of P keys with tiles of T
omc_status rank_sort(omc_ctx* ctx, uint64_t* keys, int64_t Kc, int64_t P);  // sorts the Kc columns of P keys
int64_t rank_chunk(const omc_ctx* ctx, size_t per_elem, int64_t n_idx);   // Kc (above)
// k_rank_gather and rank_sort: the draws of selected elements [k0, k0 + kc) as sorted columns keys [kc][g.P]; with stats the draws
// are folded, |x - stats[3 e]|.  flags (or NULL: left as they are) are zeroed first and then hold what the gather saw.
omc_status rank_gather_sort(omc_ctx* ctx, const double* store, const int64_t* idx, int64_t k0, int64_t kc, int64_t size, const RankGeom& g,
                            const double* stats, uint64_t* keys, int32_t* flags);

// A cursor over ctx->rank_ws behind RANK_HEAD, for a caller that works on chunks of Kc elements at per_elem bytes each.  Kc is
// rank_chunk's; a caller with a limit of its own lowers it before the first take().  The first take() asks omc_ensure for
// RANK_HEAD + Kc per_elem + 64 bytes; every take() hands out the next n objects of T where the cursor stands, so the arrays lie in
// the order they are taken, nothing between them.  done() is what the caller returns on failure: omc_ensure's status, or
// OMC_HIP_ERROR with a text if a take was misaligned or the cursor has passed the bytes asked for -- per_elem and the takes disagree,
// and nothing has been launched yet.
struct RankCarve {
  omc_ctx* ctx;
  size_t per_elem;
  int64_t Kc;
  char *at = nullptr, *end = nullptr;
  omc_status st = OMC_OK;
  bool aligned = true;

  RankCarve(omc_ctx* c, size_t per_elem_, int64_t n_idx) : ctx(c), per_elem(per_elem_), Kc(rank_chunk(c, per_elem_, n_idx)) {}

  template <typename T>
  T* take(size_t n) {
    if (!at && st == OMC_OK) {
      const size_t need = RANK_HEAD + (size_t)Kc * per_elem + 64;
      st = omc_ensure(ctx, ctx->rank_ws, need);
      if (st != OMC_OK) return nullptr;
      at = (char*)ctx->rank_ws.p + RANK_HEAD;
      end = (char*)ctx->rank_ws.p + need;
    }
    if (st != OMC_OK) return nullptr;
    T* p = (T*)at;
    aligned = aligned && (uintptr_t)at % alignof(T) == 0;
    at += n * sizeof(T);
    return p;
  }
  int32_t* head() const { return (int32_t*)ctx->rank_ws.p; }  // the check words in front of the arrays
  omc_status done() const {
    if (st != OMC_OK || (aligned && at <= end)) return st;
    omc_set_error_text(aligned ? "rank_ws: the arrays of a chunk pass the bytes their caller sized the workspace with"
                               : "rank_ws: an array of a chunk is not aligned for its type");
    return OMC_HIP_ERROR;
  }
};

__device__ __forceinline__ uint64_t rank_key(double v) {
  if (v == 0.0) v = 0.0;  // -0.0 and +0.0 are one value
  return q_key(v);
}

// what a column's flag word notes of a draw: bit 0 a NaN, bit 1 an infinity
__device__ __forceinline__ int32_t rank_flag_bits(double x) {
  return x != x ? 1 : (fabs(x) == __longlong_as_double(0x7ff0000000000000LL) ? 2 : 0);
}

// One workgroup of 256, one tile of RANK_G_TE selected elements (from e0 of the chunk's Kc, element k0 + e of the selection) x
// RANK_G_TS draws (from s0 of the S): reads the draws where they lie -- 16 adjacent elements of a row per 128 bytes, four loads in
// flight --, draw s of the column at row row_of(s) of the store seen as [N C][size]; turns value(x) into its key and writes the
// keys, transposed through LDS, into columns q0 + e of keys [..][P], the all-ones key behind the S draws.  flags (or NULL):
// the flag bits of the values and `bits`, the thread's own for element e0 + tid % 16, combined through LDS: one atomic per
// workgroup and element.  OR does not depend on the order.
template <typename RowOf, typename Value>
__device__ __forceinline__ void rank_gather_tile(const double* __restrict__ store, const int64_t* __restrict__ idx, int64_t k0, int64_t Kc,
                                                 int64_t size, int64_t S, int64_t P, int64_t e0, int64_t s0, int64_t q0, RowOf row_of,
                                                 Value value, int32_t bits, uint64_t* __restrict__ keys, int32_t* __restrict__ flags) {
  __shared__ uint64_t tile[RANK_G_TE][RANK_G_TS + 1];
  __shared__ int32_t seen[256 / RANK_G_TE][RANK_G_TE];
  const int tid = threadIdx.x, e_l = tid & (RANK_G_TE - 1), d_l = tid / RANK_G_TE;
  const int64_t e = e0 + e_l;
  const bool live = e < Kc;
  const int64_t col = live ? (idx ? idx[k0 + e] : k0 + e) : 0;
  double v[RANK_G_TS / (256 / RANK_G_TE)];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t s = s0 + d_l + 16 * u;
    v[u] = (live && s < S) ? store[row_of(s) * size + col] : 0.0;
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t s = s0 + d_l + 16 * u;
    uint64_t key = ~0ull;
    if (live && s < S) {
      const double x = value(v[u], s, e_l);
      bits |= rank_flag_bits(x);
      key = rank_key(x);
    }
    tile[e_l][d_l + 16 * u] = key;
  }
  seen[d_l][e_l] = bits;
  __syncthreads();
  if (flags && tid < RANK_G_TE && e0 + tid < Kc) {
    int32_t any = 0;
    for (int q = 0; q < 256 / RANK_G_TE; ++q) any |= seen[q][tid];
    if (any) atomicOr(&flags[q0 + e0 + tid], any);
  }
  const int s_l = tid & (RANK_G_TS - 1);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int el = (tid >> 6) + 4 * u;
    if (e0 + el < Kc && s0 + s_l < P) keys[(q0 + e0 + el) * P + s0 + s_l] = tile[el][s_l];
  }
}

// keys of a sorted column (P of them, a power of two) that are < key (upper == false) or <= key (upper == true): every read is at
// an index below P whatever the keys hold
__device__ __forceinline__ int64_t rank_bound(const uint64_t* __restrict__ col, int64_t P, uint64_t key, bool upper) {
  int64_t lo = 0;
  for (int64_t step = P >> 1; step >= 1; step >>= 1) {
    const uint64_t c = col[lo + step - 1];
    if (upper ? c <= key : c < key) lo += step;
  }
  const uint64_t c = col[lo];
  return lo + ((upper ? c <= key : c < key) ? 1 : 0);
}
