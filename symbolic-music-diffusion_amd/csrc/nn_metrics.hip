// Nearest-neighbour sample-quality metrics (Kynkaanniemi et al. 2019: improved precision / recall, realism; logged by the
// reference's sample_ncsn.py:148-157, defined in DESIGN.md section 14) on the Gram tile of metrics.hip: exact-fp32 MFMA, the
// n x n distance matrix is never written.
//
//   knn_radii    r2[i] = the k-th smallest d2 from row i of X to its other rows (self excluded by index).
//   ball_cover   for each query q: covered = OR_j (d2(q, x_j) <= r2[j]) and realism2 = max over kept j of r2[j] / max(d2, FLT_MIN).
//
// Orientation: the rows whose answer is sought (queries) are the COLUMNS of the accumulator tile, so a lane owns two queries
// (lane & 31 of its wave's two 32-wide column blocks) and sees 32 candidates of each per tile in its registers: the running
// state is two sorted k-lists (or two flags and two maxima) per lane.  The other side (candidates / centres) runs over the
// accumulator rows and is walked in chunks of CHUNK tiles per workgroup.
//
// d2 = (-2 <x, y> + |x|^2) + |y|^2 clamped at 0, as in metrics.hip; x is the row that OWNS the radius (the query of knn_radii,
// the centre of ball_cover), so the d2 that made a radius and the d2 that is compared with it are the same bits: a row that is
// exactly the k-th neighbour of a centre is covered by it (d2 == r2), on the GPU as in exact arithmetic.
//
// Determinism: no atomics.  Every workgroup writes its partial (k-list, flag, maximum) to a slot of its own and a merge launch
// combines the slots; smallest-k, OR and max do not depend on the order anyway.  Two calls give the same bits.
#include <float.h>
#include <math.h>

#include "gram_tile.h"
#include "../../include/smd_hip.h"

namespace {

constexpr int CHUNK = 16;          // candidate / centre tiles per workgroup (2048 rows)
constexpr int KMAX = SMD_KNN_MAX_K;

inline int64_t tiles_of(int n) { return ((int64_t)n + MT - 1) / MT; }
inline int64_t splits_of(int n) { return (tiles_of(n) + CHUNK - 1) / CHUNK; }

// sorted ascending l[0..K): put v in if it is below the largest
template <int K>
__device__ __forceinline__ void topk_insert(float (&l)[K], float v) {
  if (v < l[K - 1]) {
#pragma unroll
    for (int t = 0; t < K; ++t) {
      const float lo = fminf(l[t], v);
      v = fmaxf(l[t], v);
      l[t] = lo;
    }
  }
}

// ---------------------------------------------------------------------------------------------------- k-NN radii
struct KnnArgs {
  const float* x; int64_t ld;
  int n, d, tiles, splits;
  const float* nrm;
  float* part;            // [splits][n][K]
};

template <int K>
__global__ __launch_bounds__(NT, 2) void knn_partial_kernel(KnnArgs a) {
  __shared__ float As[BK * LDP];
  __shared__ float Bs[BK * LDP];
  __shared__ float nc[MT], nq[MT];
  __shared__ float lists[4][K][MT];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wr = w >> 1, wc = w & 1;
  const int tile = smd_xcd_band(blockIdx.x, gridDim.x);      // neighbours share the query tile and an L2
  const int qb = tile / a.splits, s = tile - qb * a.splits;
  const int j0 = qb * MT;
  const int c_end = min(a.tiles, (s + 1) * CHUNK);
  if (t < MT) nq[t] = (j0 + t < a.n) ? a.nrm[j0 + t] : 0.0f;
  float best[2][K];
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int e = 0; e < K; ++e) best[n][e] = INFINITY;

  f32x16_t acc[2][2];
  for (int cb = s * CHUNK; cb < c_end; ++cb) {
    const int i0 = cb * MT;
    __syncthreads();                                          // the previous tile's epilogue has read nc
    if (t >= MT) nc[t - MT] = (i0 + t - MT < a.n) ? a.nrm[i0 + t - MT] : 0.0f;
    gram_tile(a.x, a.ld, a.n, i0, a.x, a.ld, a.n, j0, a.d, As, Bs, acc);   // rows: candidates, columns: queries
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int jl = wc * 64 + n * 32 + (lane & 31), j = j0 + jl;
      const float nj = nq[jl];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int il = wr * 64 + m * 32 + cd_row(r, lane), i = i0 + il;
          float d2 = fmaxf((-2.0f * acc[m][n][r] + nj) + nc[il], 0.0f);
          if (i >= a.n || i == j) d2 = INFINITY;              // padding, and self by index: a duplicate of row j still counts
          topk_insert<K>(best[n], d2);
        }
    }
  }
  // the four partial lists of a query column (2 row halves of the tile x 2 lane halves) -> one
  const int p = wr * 2 + (lane >> 5);
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int e = 0; e < K; ++e) lists[p][e][wc * 64 + n * 32 + (lane & 31)] = best[n][e];
  __syncthreads();
  if (t < MT && j0 + t < a.n) {
    float l[K];
#pragma unroll
    for (int e = 0; e < K; ++e) l[e] = lists[0][e][t];
#pragma unroll
    for (int q = 1; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < K; ++e) topk_insert<K>(l, lists[q][e][t]);
    float* out = a.part + ((int64_t)s * a.n + j0 + t) * K;
#pragma unroll
    for (int e = 0; e < K; ++e) out[e] = l[e];
  }
}

// r2[i] = the k-th smallest of the splits' lists of row i
template <int K>
__global__ __launch_bounds__(256) void knn_merge_kernel(const float* __restrict__ part, int n, int splits, float* __restrict__ r2) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float l[K];
#pragma unroll
  for (int e = 0; e < K; ++e) l[e] = part[(int64_t)i * K + e];
  for (int s = 1; s < splits; ++s) {
    const float* p = part + ((int64_t)s * n + i) * K;
#pragma unroll
    for (int e = 0; e < K; ++e) topk_insert<K>(l, p[e]);
  }
  r2[i] = l[K - 1];
}

template <int K>
int knn_launch(const KnnArgs& a, float* r2, hipStream_t st) {
  knn_partial_kernel<K><<<(unsigned)((int64_t)a.tiles * a.splits), NT, 0, st>>>(a);
  SMD_LAUNCH_CHECK();
  knn_merge_kernel<K><<<(a.n + 255) / 256, 256, 0, st>>>(a.part, a.n, a.splits, r2);
  SMD_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------- ball cover
struct CoverArgs {
  const float* q; const float* x; int64_t ldq, ldx;
  int nq, nx, d, exclude_diagonal, tiles_x, splits;
  const float* nrm_q; const float* nrm_x;
  const float* r2; const uint8_t* keep;      // keep may be null: every centre is kept
  float* part_max;        // [splits][nq]
  uint8_t* part_cov;      // [splits][nq]
};

__global__ __launch_bounds__(NT, 2) void ball_cover_partial_kernel(CoverArgs a) {
  __shared__ float As[BK * LDP];
  __shared__ float Bs[BK * LDP];
  __shared__ float nc[MT], nq[MT];
  __shared__ float rc[MT], rk[MT];       // radius^2 of the tile's centres for coverage / for realism; -1 where it does not apply
  __shared__ float pmax[4][MT];
  __shared__ int pcov[4][MT];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wr = w >> 1, wc = w & 1;
  const int tile = smd_xcd_band(blockIdx.x, gridDim.x);
  const int qb = tile / a.splits, s = tile - qb * a.splits;
  const int j0 = qb * MT;
  const int c_end = min(a.tiles_x, (s + 1) * CHUNK);
  if (t < MT) nq[t] = (j0 + t < a.nq) ? a.nrm_q[j0 + t] : 0.0f;
  float mx[2] = {0.0f, 0.0f};
  int cov[2] = {0, 0};

  f32x16_t acc[2][2];
  for (int cb = s * CHUNK; cb < c_end; ++cb) {
    const int i0 = cb * MT;
    __syncthreads();                                          // the previous tile's epilogue has read nc, rc, rk
    if (t >= MT) {
      const int il = t - MT, i = i0 + il;
      const bool ok = i < a.nx;
      const float r = ok ? a.r2[i] : -1.0f;                   // d2 >= 0 is never <= -1: padded centres cover nothing
      nc[il] = ok ? a.nrm_x[i] : 0.0f;
      rc[il] = r;
      rk[il] = (ok && (!a.keep || a.keep[i])) ? r : -1.0f;
    }
    gram_tile(a.x, a.ldx, a.nx, i0, a.q, a.ldq, a.nq, j0, a.d, As, Bs, acc);   // rows: centres, columns: queries
    const bool diag = a.exclude_diagonal && i0 == j0;         // Q is X: pair (i, i) lies on the diagonal of the diagonal tiles
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int jl = wc * 64 + n * 32 + (lane & 31);
      const float nj = nq[jl];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int il = wr * 64 + m * 32 + cd_row(r, lane);
          const float d2 = fmaxf((-2.0f * acc[m][n][r] + nc[il]) + nj, 0.0f);   // x = the centre: the d2 its radius was taken from
          const bool self = diag && il == jl;
          const float c = self ? -1.0f : rc[il], k = self ? -1.0f : rk[il];
          cov[n] |= (d2 <= c) ? 1 : 0;
          const float dd = fmaxf(d2, FLT_MIN);
          // IEEE division only where the quotient can pass the running maximum: fl(k / dd) > mx needs k > mx dd (1 - 2^-24)
          if (k > 0.999f * mx[n] * dd) mx[n] = fmaxf(mx[n], fminf(k / dd, FLT_MAX));
        }
    }
  }
  const int p = wr * 2 + (lane >> 5);
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    pmax[p][wc * 64 + n * 32 + (lane & 31)] = mx[n];
    pcov[p][wc * 64 + n * 32 + (lane & 31)] = cov[n];
  }
  __syncthreads();
  if (t < MT && j0 + t < a.nq) {
    const float m = fmaxf(fmaxf(pmax[0][t], pmax[1][t]), fmaxf(pmax[2][t], pmax[3][t]));
    const int c = pcov[0][t] | pcov[1][t] | pcov[2][t] | pcov[3][t];
    a.part_max[(int64_t)s * a.nq + j0 + t] = m;
    a.part_cov[(int64_t)s * a.nq + j0 + t] = (uint8_t)c;
  }
}

__global__ __launch_bounds__(256) void ball_cover_merge_kernel(const float* __restrict__ part_max, const uint8_t* __restrict__ part_cov,
                                                               int nq, int splits, uint8_t* __restrict__ covered,
                                                               float* __restrict__ realism2) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nq) return;
  float m = 0.0f;
  int c = 0;
  for (int s = 0; s < splits; ++s) {
    m = fmaxf(m, part_max[(int64_t)s * nq + j]);
    c |= part_cov[(int64_t)s * nq + j];
  }
  covered[j] = (uint8_t)c;
  realism2[j] = m;
}

}  // namespace

extern "C" {

int64_t smd_knn_radii_workspace_bytes(int n, int k) {
  if (k < 1 || k > KMAX || n < k + 1) return -1;
  return up8((int64_t)n * 4) + splits_of(n) * n * k * 4;
}

int smd_knn_radii(const float* x, int64_t ld, int n, int d, int k, void* workspace, int64_t workspace_bytes, float* r2, void* stream) {
  SMD_ARG_CHECK(x && workspace && r2, "smd_knn_radii: null pointer");
  SMD_ARG_CHECK(k >= 1 && k <= KMAX, "smd_knn_radii: k=%d must be in [1, %d]", k, KMAX);
  SMD_ARG_CHECK(d >= 1 && n >= k + 1, "smd_knn_radii: n=%d d=%d: d must be >= 1 and a row needs k=%d other rows", n, d, k);
  SMD_ARG_CHECK(ld >= d, "smd_knn_radii: row stride ld=%lld must be >= d=%d", (long long)ld, d);
  SMD_ARG_CHECK(al4(x) && al4(r2) && al8(workspace), "smd_knn_radii: x, r2 must be 4-byte and workspace 8-byte aligned");
  const int64_t tiles = tiles_of(n), splits = splits_of(n);
  // HIP bounds a launch by gridDim.x * blockDim.x < 2^32 work-items: 2^24 - 1 workgroups of NT = 256 (n ~ 2.1 M)
  SMD_ARG_CHECK(tiles * splits * NT < ((int64_t)1 << 32), "smd_knn_radii: %lld tiles x %lld column splits exceed one launch (at most %lld workgroups)",
                (long long)tiles, (long long)splits, (long long)((((int64_t)1 << 32) - 1) / NT));
  const int64_t need = smd_knn_radii_workspace_bytes(n, k);
  SMD_ARG_CHECK(workspace_bytes >= need, "smd_knn_radii: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* nrm = reinterpret_cast<float*>(workspace);
  row_norms_kernel<<<(n + 255) / 256, 256, 0, st>>>(x, n, d, ld, nrm);
  SMD_LAUNCH_CHECK();
  KnnArgs a;
  a.x = x; a.ld = ld; a.n = n; a.d = d; a.tiles = (int)tiles; a.splits = (int)splits; a.nrm = nrm;
  a.part = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + up8((int64_t)n * 4));
  switch (k) {
    case 1: return knn_launch<1>(a, r2, st);
    case 2: return knn_launch<2>(a, r2, st);
    case 3: return knn_launch<3>(a, r2, st);
    case 4: return knn_launch<4>(a, r2, st);
    case 5: return knn_launch<5>(a, r2, st);
    case 6: return knn_launch<6>(a, r2, st);
    case 7: return knn_launch<7>(a, r2, st);
    default: return knn_launch<8>(a, r2, st);
  }
}

int64_t smd_ball_cover_workspace_bytes(int nq, int nx) {
  if (nq < 1 || nx < 1) return -1;
  return up8(((int64_t)nq + nx) * 4) + splits_of(nx) * nq * 4 + up8(splits_of(nx) * nq);
}

int smd_ball_cover(const float* q, int64_t ldq, int nq, const float* x, int64_t ldx, int nx, int d, const float* r2,
                   const uint8_t* keep, int exclude_diagonal, void* workspace, int64_t workspace_bytes, uint8_t* covered,
                   float* realism2, void* stream) {
  SMD_ARG_CHECK(q && x && r2 && workspace && covered && realism2, "smd_ball_cover: null pointer (only keep may be NULL)");
  SMD_ARG_CHECK(nq >= 1 && nx >= 1 && d >= 1, "smd_ball_cover: nq=%d nx=%d d=%d must be >= 1", nq, nx, d);
  SMD_ARG_CHECK(ldq >= d && ldx >= d, "smd_ball_cover: row strides ldq=%lld ldx=%lld must be >= d=%d", (long long)ldq, (long long)ldx, d);
  SMD_ARG_CHECK(!exclude_diagonal || nq == nx, "smd_ball_cover: exclude_diagonal needs nq == nx (got %d, %d)", nq, nx);
  SMD_ARG_CHECK(al4(q) && al4(x) && al4(r2) && al4(realism2) && al8(workspace),
                "smd_ball_cover: q, x, r2, realism2 must be 4-byte and workspace 8-byte aligned");
  const int64_t tiles_q = tiles_of(nq), tiles_x = tiles_of(nx), splits = splits_of(nx);
  SMD_ARG_CHECK(tiles_q * splits * NT < ((int64_t)1 << 32), "smd_ball_cover: %lld query tiles x %lld centre splits exceed one launch (at most %lld workgroups)",
                (long long)tiles_q, (long long)splits, (long long)((((int64_t)1 << 32) - 1) / NT));
  const int64_t need = smd_ball_cover_workspace_bytes(nq, nx);
  SMD_ARG_CHECK(workspace_bytes >= need, "smd_ball_cover: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* nrm_q = reinterpret_cast<float*>(workspace);
  float* nrm_x = nrm_q + nq;
  float* part_max = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + up8(((int64_t)nq + nx) * 4));
  uint8_t* part_cov = reinterpret_cast<uint8_t*>(part_max + splits * nq);
  row_norms_kernel<<<(nq + 255) / 256, 256, 0, st>>>(q, nq, d, ldq, nrm_q);
  SMD_LAUNCH_CHECK();
  row_norms_kernel<<<(nx + 255) / 256, 256, 0, st>>>(x, nx, d, ldx, nrm_x);
  SMD_LAUNCH_CHECK();
  CoverArgs a;
  a.q = q; a.x = x; a.ldq = ldq; a.ldx = ldx; a.nq = nq; a.nx = nx; a.d = d; a.exclude_diagonal = exclude_diagonal ? 1 : 0;
  a.tiles_x = (int)tiles_x; a.splits = (int)splits; a.nrm_q = nrm_q; a.nrm_x = nrm_x; a.r2 = r2; a.keep = keep;
  a.part_max = part_max; a.part_cov = part_cov;
  ball_cover_partial_kernel<<<(unsigned)(tiles_q * splits), NT, 0, st>>>(a);
  SMD_LAUNCH_CHECK();
  ball_cover_merge_kernel<<<(nq + 255) / 256, 256, 0, st>>>(part_max, part_cov, nq, (int)splits, covered, realism2);
  SMD_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
