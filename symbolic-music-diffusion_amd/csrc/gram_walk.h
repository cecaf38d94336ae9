// The query-column walk over the Gram tile of gram_tile.h that the nearest-neighbour kernels share: k-NN radii and ball cover
// (nn_metrics.hip) run it as query_walk(); the nearest-neighbour search (nn_search.hip, section 24) has it
// written out for the reason given there.  With it the sorted k-list all three keep.  The n_q x n_x distance matrix is never
// written.
//
// Orientation: the rows whose answer is sought (queries) are the COLUMNS of the accumulator tile, so a lane owns two queries
// (lane & 31 of its wave's two 32-wide column blocks) and sees 32 candidates of each per tile in its registers: the running
// state is two small per-query states per lane.  The other side (candidates / centres) runs over the accumulator rows and is
// walked in chunks of CHUNK tiles per workgroup.  The four partial states of a query column (2 row halves of the tile x 2 lane
// halves) meet in LDS, and every workgroup writes one slot per (split, query): no atomics, a merge launch combines the slots.
//
// What differs between the kernels is an operation object, inlined into the walk:
//   Op::Shared                  its LDS: per-candidate side arrays beside the norm, and the four parked partials per query
//   op.init(n, j)               the lane's state for its query n in {0, 1}, global row j
//   op.stage(sh, il, i, ok)     thread MT + il: side values of candidate i = i0 + il of the coming tile (ok: i < nx)
//   op.visit(sh, n, e)          one accumulator element e (WalkElem) of query n
//   op.park(sh, p, n, jl)       the lane's state of query n, tile column jl, as partial p of 4
//   op.fold(sh, jl, slot)       thread jl: the four partials of column jl -> slot = split * nq + j of the workspace
// The operation forms d2 itself from e.g and the two norms: WHICH norm is added first is part of a kernel's contract (the row
// that owns a radius goes first, section 14), d2_of() keeps the rest in one place.
#pragma once
#include <type_traits>

#include "gram_tile.h"
#include "../../include/smd_hip.h"

namespace {

constexpr int CHUNK = 16;          // candidate / centre tiles per workgroup (2048 rows)
inline int64_t splits_of(int n) { return (tiles_of(n) + CHUNK - 1) / CHUNK; }

// f(std::integral_constant<int, k>) for the k in [1, SMD_KNN_MAX_K] of a call that has checked its range
static_assert(SMD_KNN_MAX_K == 8, "dispatch_k lists the list lengths one by one");
template <typename F>
int dispatch_k(int k, F&& f) {
  switch (k) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    default: return f(std::integral_constant<int, 8>{});
  }
}

// ---------------------------------------------------------------------------------------------------- sorted k-list
// An entry is a distance alone (float) or a (distance, index) pair in lexicographic order.  Candidate indices are distinct, so
// the pair order is total; an empty entry is (+inf, -1), above every candidate that can enter.
template <typename I>
struct DistIdx {
  float d2; I i;
};
template <typename I>
__device__ __forceinline__ bool pair_less(float a, I ia, float b, I ib) { return a < b || (a == b && ia < ib); }
template <typename I>
__device__ __forceinline__ bool operator<(const DistIdx<I>& a, const DistIdx<I>& b) { return pair_less(a.d2, a.i, b.d2, b.i); }

// a <- the lower, b <- the higher of the two.  Distances alone stay a min / max chain with no compare-select.
__device__ __forceinline__ void order2(float& a, float& b) {
  const float lo = fminf(a, b);
  b = fmaxf(a, b);
  a = lo;
}
template <typename I>
__device__ __forceinline__ void order2(DistIdx<I>& a, DistIdx<I>& b) {
  const bool c = b < a;
  const DistIdx<I> lo{c ? b.d2 : a.d2, c ? b.i : a.i}, hi{c ? a.d2 : b.d2, c ? a.i : b.i};   // selects of values, not of addresses
  a = lo;
  b = hi;
}

// sorted ascending l[0..K): put v in if it is below the largest
template <int K, typename E>
__device__ __forceinline__ void list_insert(E (&l)[K], E v) {
  if (v < l[K - 1]) {
#pragma unroll
    for (int t = 0; t < K; ++t) order2(l[t], v);
  }
}

// ---------------------------------------------------------------------------------------------------- the walk
struct Walk {
  const float* q; int64_t ldq; int nq; const float* nrm_q;      // queries: the tile's columns
  const float* x; int64_t ldx; int nx; const float* nrm_x;      // candidates / centres: the tile's rows
  int d, tiles_x, splits;
};

// one accumulator element: candidate i = i0 + il of nx (past them: a padded row) against query j = j0 + jl
struct WalkElem {
  float g, n_query, n_cand;      // <x_i, q_j>, |q_j|^2, |x_i|^2 (0 for padded rows)
  int i0, il, i, j0, jl, j, nx;
  __device__ __forceinline__ bool pad() const { return i >= nx; }
};

// (-2 g + first) + second clamped at 0; `first` is the norm of the row that owns the expression
__device__ __forceinline__ float d2_of(float g, float first, float second) { return fmaxf((-2.0f * g + first) + second, 0.0f); }

// grid: tiles_of(nq) * splits workgroups of NT threads, XCD-banded so that neighbours share the query tile and an L2
template <typename Op>
__device__ __forceinline__ void query_walk(const Walk& a, Op& op) {
  __shared__ float As[BK * LDP];
  __shared__ float Bs[BK * LDP];
  __shared__ float nc[MT], nq[MT];
  __shared__ typename Op::Shared sh;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wr = w >> 1, wc = w & 1;
  const int tile = smd_xcd_band(blockIdx.x, gridDim.x);
  const int qb = tile / a.splits, s = tile - qb * a.splits;
  const int j0 = qb * MT;
  const int c_end = min(a.tiles_x, (s + 1) * CHUNK);
  if (t < MT) nq[t] = (j0 + t < a.nq) ? a.nrm_q[j0 + t] : 0.0f;
#pragma unroll
  for (int n = 0; n < 2; ++n) op.init(n, j0 + wc * 64 + n * 32 + (lane & 31));

  f32x16_t acc[2][2];
  for (int cb = s * CHUNK; cb < c_end; ++cb) {
    const int i0 = cb * MT;
    __syncthreads();                                          // the previous tile's epilogue has read nc and the side arrays
    if (t >= MT) {
      const int il = t - MT, i = i0 + il;
      const bool ok = i < a.nx;
      nc[il] = ok ? a.nrm_x[i] : 0.0f;
      op.stage(sh, il, i, ok);
    }
    // The query tile is the same for every candidate tile, and the compiler would keep its eight row addresses and their masks
    // in registers next to the lanes' states for the whole walk (9 VGPRs spilled in the search at K = 8).  An opaque copy of j0
    // has them formed per tile instead, where the loader's registers are free anyway.
    int jq = j0;
    asm volatile("" : "+s"(jq));
    gram_tile(a.x, a.ldx, a.nx, i0, a.q, a.ldq, a.nq, jq, a.d, As, Bs, acc);   // rows: candidates, columns: queries
    float cn[2][16];                                          // the lane's 32 candidate norms, read once for both queries
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) cn[m][r] = nc[wr * 64 + m * 32 + cd_row(r, lane)];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      WalkElem e;
      e.i0 = i0; e.j0 = j0; e.nx = a.nx;
      e.jl = wc * 64 + n * 32 + (lane & 31); e.j = j0 + e.jl;
      e.n_query = nq[e.jl];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          e.il = wr * 64 + m * 32 + cd_row(r, lane); e.i = i0 + e.il;
          e.g = acc[m][n][r]; e.n_cand = cn[m][r];
          op.visit(sh, n, e);
        }
    }
  }
  // the four partial states of a query column (2 row halves of the tile x 2 lane halves) -> one
  const int p = wr * 2 + (lane >> 5);
#pragma unroll
  for (int n = 0; n < 2; ++n) op.park(sh, p, n, wc * 64 + n * 32 + (lane & 31));
  __syncthreads();
  if (t < MT && j0 + t < a.nq) op.fold(sh, t, (int64_t)s * a.nq + j0 + t);
}

}  // namespace
