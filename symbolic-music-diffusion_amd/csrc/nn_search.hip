// Nearest-neighbour SEARCH on the Gram tile of metrics.hip: for every query row the k candidates with the
// smallest (d2, global index) in lexicographic order, distances and indices both; the nq x nx distance matrix is never written.
// It is what --copy_metrics asks: which training row is a sample closest to, and is it closer than held-out data is.
//
// It follows the query-column walk of gram_walk.h (orientation, chunking, the four-partial fold and the slots are described there)
// with one sorted k-list of (d2, index) PAIRS per query.  d2 = (-2 <q, x> + |q|^2) + |x|^2 clamped at 0, the query owning the
// expression as in knn_radii; the bits of a pair's d2 depend on the two rows alone (one fmaf chain in k order per product and
// per norm), not on the tile the pair falls into.
//
// Order: (d2, index) pairs are compared as pairs EVERYWHERE -- in a lane's insertion, between the four partial lists of a query
// column, between the column splits and against the previous result of an accumulating call.  Candidate indices are distinct, so
// the order is total and the k smallest pairs of a union of candidate sets are one list whatever the sets, their tiles and the
// sequence of the calls were: one call on all of X and calls on any partition of X into slabs, in any order, give the same bits.
// An empty entry is (+inf, -1).  It compares above every candidate that can enter (a candidate of d2 = +inf never enters, as
// -1 is below its index), so lists shorter than k keep it as their tail.
//
// Determinism: no atomics.  Every workgroup writes its partial lists (tile-local 32-bit indices) to a slot of its own and a merge
// launch combines the slots, adds x_base and, in an accumulating call, the previous output.
#include <float.h>
#include <math.h>

#include "gram_walk.h"

namespace {

constexpr int KMAX = SMD_KNN_MAX_K;

struct SearchArgs {
  const float* q; const float* x; int64_t ldq, ldx;
  int nq, nx, d, tiles_x, splits;
  int64_t self_shift;     // q_base - x_base: query j is candidate j + self_shift
  int exclude_self;
  const float* nrm_q; const float* nrm_x;
  float* part_d2;         // [splits][nq][K]
  int32_t* part_idx;      // [splits][nq][K], indices into this call's x
};

// query_walk() of gram_walk.h written out, with (d2, index) pair lists: as an operation of the shared walk this kernel computes the
// same bits, but the compiler then schedules the MFMA stage loop with one LDS address register instead of two (the two reads of a
// k step no longer issue back to back) and the search measures 1 - 5 % slower at d >= 146.  Until that is
// understood, a change to the walk is made here as well.
template <int K>
__global__ __launch_bounds__(NT, 2) void nn_search_partial_kernel(SearchArgs a) {
  using Pair = DistIdx<int32_t>;
  __shared__ float As[BK * LDP];
  __shared__ float Bs[BK * LDP];
  __shared__ float nc[MT], nq[MT];
  __shared__ float lists[4][K][MT];
  __shared__ int32_t ilists[4][K][MT];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wr = w >> 1, wc = w & 1;
  const int tile = smd_xcd_band(blockIdx.x, gridDim.x);      // neighbours share the query tile and an L2
  const int qb = tile / a.splits, s = tile - qb * a.splits;
  const int j0 = qb * MT;
  const int c_end = min(a.tiles_x, (s + 1) * CHUNK);
  if (t < MT) nq[t] = (j0 + t < a.nq) ? a.nrm_q[j0 + t] : 0.0f;
  Pair best[2][K];
  int32_t self[2];        // the candidate that IS the query (by index), -1 when there is none in x
#pragma unroll
  for (int n = 0; n < 2; ++n) {
#pragma unroll
    for (int e = 0; e < K; ++e) best[n][e] = Pair{INFINITY, -1};
    const int64_t si = (int64_t)(j0 + wc * 64 + n * 32 + (lane & 31)) + a.self_shift;
    self[n] = (a.exclude_self && si >= 0 && si < a.nx) ? (int32_t)si : -1;
  }

  f32x16_t acc[2][2];
  for (int cb = s * CHUNK; cb < c_end; ++cb) {
    const int i0 = cb * MT;
    __syncthreads();                                          // the previous tile's epilogue has read nc
    if (t >= MT) nc[t - MT] = (i0 + t - MT < a.nx) ? a.nrm_x[i0 + t - MT] : 0.0f;
    int jq = j0;                                              // opaque: see query_walk()
    asm volatile("" : "+s"(jq));
    gram_tile(a.x, a.ldx, a.nx, i0, a.q, a.ldq, a.nq, jq, a.d, As, Bs, acc);   // rows: candidates, columns: queries
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const float nj = nq[wc * 64 + n * 32 + (lane & 31)];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int il = wr * 64 + m * 32 + cd_row(r, lane), i = i0 + il;
          float d2 = d2_of(acc[m][n][r], nj, nc[il]);
          if (i >= a.nx || i == self[n]) d2 = INFINITY;       // padding, and self by index: a duplicate of the query still counts
          list_insert<K>(best[n], Pair{d2, i});
        }
    }
  }
  // the four partial lists of a query column (2 row halves of the tile x 2 lane halves) -> one, pairs compared as pairs
  const int p = wr * 2 + (lane >> 5);
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int e = 0; e < K; ++e) {
      lists[p][e][wc * 64 + n * 32 + (lane & 31)] = best[n][e].d2;
      ilists[p][e][wc * 64 + n * 32 + (lane & 31)] = best[n][e].i;
    }
  __syncthreads();
  if (t < MT && j0 + t < a.nq) {
    Pair l[K];
#pragma unroll
    for (int e = 0; e < K; ++e) l[e] = Pair{lists[0][e][t], ilists[0][e][t]};
#pragma unroll
    for (int q = 1; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < K; ++e) list_insert<K>(l, Pair{lists[q][e][t], ilists[q][e][t]});
    const int64_t o = ((int64_t)s * a.nq + j0 + t) * K;
#pragma unroll
    for (int e = 0; e < K; ++e) {
      a.part_d2[o + e] = l[e].d2;
      a.part_idx[o + e] = l[e].i;
    }
  }
}

// the k smallest pairs of the splits' lists of query j and, accumulating, of what the outputs hold; indices become global here
template <int K>
__global__ __launch_bounds__(256) void nn_search_merge_kernel(const float* __restrict__ part_d2, const int32_t* __restrict__ part_idx,
                                                              int nq, int splits, int64_t x_base, int accumulate,
                                                              float* __restrict__ d2_out, int64_t* __restrict__ idx_out) {
  using Pair = DistIdx<int64_t>;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nq) return;
  Pair l[K];
#pragma unroll
  for (int e = 0; e < K; ++e) l[e] = accumulate ? Pair{d2_out[(int64_t)j * K + e], idx_out[(int64_t)j * K + e]} : Pair{INFINITY, -1};
  for (int s = 0; s < splits; ++s) {
    const int64_t o = ((int64_t)s * nq + j) * K;
#pragma unroll
    for (int e = 0; e < K; ++e) {
      const int32_t i = part_idx[o + e];
      list_insert<K>(l, Pair{part_d2[o + e], i < 0 ? (int64_t)-1 : x_base + i});
    }
  }
#pragma unroll
  for (int e = 0; e < K; ++e) {
    d2_out[(int64_t)j * K + e] = l[e].d2;
    idx_out[(int64_t)j * K + e] = l[e].i;
  }
}

template <int K>
int search_launch(const SearchArgs& a, int64_t x_base, int accumulate, float* d2_out, int64_t* idx_out, hipStream_t st) {
  nn_search_partial_kernel<K><<<(unsigned)(tiles_of(a.nq) * a.splits), NT, 0, st>>>(a);
  SMD_LAUNCH_CHECK();
  nn_search_merge_kernel<K><<<(a.nq + 255) / 256, 256, 0, st>>>(a.part_d2, a.part_idx, a.nq, a.splits, x_base, accumulate, d2_out, idx_out);
  SMD_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" {

int64_t smd_nn_search_workspace_bytes(int nq, int nx, int k) {
  if (k < 1 || k > KMAX || nq < 1 || nx < 1) return -1;
  return up8(((int64_t)nq + nx) * 4) + splits_of(nx) * nq * k * 8;
}

int smd_nn_search(const float* q, int64_t ldq, int nq, int64_t q_base, const float* x, int64_t ldx, int nx, int64_t x_base, int d, int k,
                  int exclude_self, int accumulate, void* workspace, int64_t workspace_bytes, float* d2_out, int64_t* idx_out,
                  void* stream) {
  SMD_ARG_CHECK(q && x && workspace && d2_out && idx_out, "smd_nn_search: null pointer");
  SMD_ARG_CHECK(k >= 1 && k <= KMAX, "smd_nn_search: k=%d must be in [1, %d]", k, KMAX);
  SMD_ARG_CHECK(nq >= 1 && nx >= 1 && d >= 1 && nq <= INT32_MAX - MT && nx <= INT32_MAX - MT,
                "smd_nn_search: nq=%d nx=%d d=%d must be >= 1 (nq, nx at most %d)", nq, nx, d, INT32_MAX - MT);
  SMD_ARG_CHECK(ldq >= d && ldx >= d, "smd_nn_search: row strides ldq=%lld ldx=%lld must be >= d=%d", (long long)ldq, (long long)ldx, d);
  SMD_ARG_CHECK(q_base >= 0 && x_base >= 0 && q_base <= INT64_MAX - nq && x_base <= INT64_MAX - nx,
                "smd_nn_search: q_base=%lld x_base=%lld must be >= 0 and leave room for the rows' global indices", (long long)q_base,
                (long long)x_base);
  SMD_ARG_CHECK(al4(q) && al4(x) && al4(d2_out) && al8(idx_out) && al8(workspace),
                "smd_nn_search: q, x, d2_out must be 4-byte and idx_out, workspace 8-byte aligned");
  const int64_t tiles_q = tiles_of(nq), tiles_x = tiles_of(nx), splits = splits_of(nx);
  SMD_ARG_CHECK(fits_one_launch(tiles_q * splits), "smd_nn_search: %lld query tiles x %lld candidate splits exceed one launch (at most %lld workgroups)",
                (long long)tiles_q, (long long)splits, (long long)MAX_WORKGROUPS);
  const int64_t need = smd_nn_search_workspace_bytes(nq, nx, k);
  SMD_ARG_CHECK(workspace_bytes >= need, "smd_nn_search: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* nrm_q = ws_at<float>(workspace, 0);
  float* nrm_x = nrm_q + nq;
  if (const int e = launch_row_norms(q, nq, ldq, nrm_q, x, nx, ldx, nrm_x, d, st)) return e;
  SearchArgs a;
  a.q = q; a.x = x; a.ldq = ldq; a.ldx = ldx; a.nq = nq; a.nx = nx; a.d = d; a.tiles_x = (int)tiles_x; a.splits = (int)splits;
  a.self_shift = q_base - x_base; a.exclude_self = exclude_self ? 1 : 0; a.nrm_q = nrm_q; a.nrm_x = nrm_x;
  a.part_d2 = ws_at<float>(workspace, up8(((int64_t)nq + nx) * 4));
  a.part_idx = reinterpret_cast<int32_t*>(a.part_d2 + splits * nq * k);
  const int acc = accumulate ? 1 : 0;
  return dispatch_k(k, [&](auto K) { return search_launch<decltype(K)::value>(a, x_base, acc, d2_out, idx_out, st); });
}

}  // extern "C"
