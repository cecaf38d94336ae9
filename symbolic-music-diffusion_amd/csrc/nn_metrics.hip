// Nearest-neighbour sample-quality metrics (Kynkaanniemi et al. 2019: improved precision / recall, realism; logged by the
// reference's sample_ncsn.py:148-157, defined in DESIGN.md section 14) on the Gram tile of metrics.hip: exact-fp32 MFMA, the
// n x n distance matrix is never written.
//
//   knn_radii    r2[i] = the k-th smallest d2 from row i of X to its other rows (self excluded by index).
//   ball_cover   for each query q: covered = OR_j (d2(q, x_j) <= r2[j]) and realism2 = max over kept j of r2[j] / max(d2, FLT_MIN).
//
// Both are the query-column walk of gram_walk.h (orientation, chunking, the four-partial fold and the slots are described
// there) with an operation each: two sorted k-lists of distances per lane, or two flags and two maxima.
//
// d2 = (-2 <x, y> + |x|^2) + |y|^2 clamped at 0, as in metrics.hip; x is the row that OWNS the radius (the query of knn_radii,
// the centre of ball_cover), so the d2 that made a radius and the d2 that is compared with it are the same bits: a row that is
// exactly the k-th neighbour of a centre is covered by it (d2 == r2), on the GPU as in exact arithmetic.
//
// Determinism: no atomics.  Every workgroup writes its partial (k-list, flag, maximum) to a slot of its own and a merge launch
// combines the slots; smallest-k, OR and max do not depend on the order anyway.  Two calls give the same bits.
#include <float.h>
#include <math.h>

#include "gram_walk.h"

namespace {

constexpr int KMAX = SMD_KNN_MAX_K;

// ---------------------------------------------------------------------------------------------------- k-NN radii
struct KnnArgs {
  const float* x; int64_t ld;
  int n, d, tiles, splits;
  const float* nrm;
  float* part;            // [splits][n][K]
};

template <int K>
struct KnnOp {
  struct Shared { float lists[4][K][MT]; };
  float* part;
  float best[2][K];
  __device__ __forceinline__ void init(int n, int) {
#pragma unroll
    for (int e = 0; e < K; ++e) best[n][e] = INFINITY;
  }
  __device__ __forceinline__ void stage(Shared&, int, int, bool) {}
  __device__ __forceinline__ void visit(Shared&, int n, const WalkElem& e) {
    float d2 = d2_of(e.g, e.n_query, e.n_cand);
    if (e.pad() || e.i == e.j) d2 = INFINITY;                   // padding, and self by index: a duplicate of row j still counts
    list_insert<K>(best[n], d2);
  }
  __device__ __forceinline__ void park(Shared& sh, int p, int n, int jl) {
#pragma unroll
    for (int e = 0; e < K; ++e) sh.lists[p][e][jl] = best[n][e];
  }
  __device__ __forceinline__ void fold(Shared& sh, int jl, int64_t slot) {
    float l[K];
#pragma unroll
    for (int e = 0; e < K; ++e) l[e] = sh.lists[0][e][jl];
#pragma unroll
    for (int q = 1; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < K; ++e) list_insert<K>(l, sh.lists[q][e][jl]);
#pragma unroll
    for (int e = 0; e < K; ++e) part[slot * K + e] = l[e];
  }
};

template <int K>
__global__ __launch_bounds__(NT, 2) void knn_partial_kernel(KnnArgs a) {
  KnnOp<K> op;
  op.part = a.part;
  query_walk(Walk{a.x, a.ld, a.n, a.nrm, a.x, a.ld, a.n, a.nrm, a.d, a.tiles, a.splits}, op);
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
    for (int e = 0; e < K; ++e) list_insert<K>(l, p[e]);
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

struct CoverOp {
  struct Shared {
    float rc[MT], rk[MT];     // radius^2 of the tile's centres for coverage / for realism; -1 where it does not apply
    float pmax[4][MT];
    int pcov[4][MT];
  };
  const CoverArgs& a;
  float mx[2];
  int cov[2];
  __device__ __forceinline__ void init(int n, int) { mx[n] = 0.0f; cov[n] = 0; }
  __device__ __forceinline__ void stage(Shared& sh, int il, int i, bool ok) {
    const float r = ok ? a.r2[i] : -1.0f;                     // d2 >= 0 is never <= -1: padded centres cover nothing
    sh.rc[il] = r;
    sh.rk[il] = (ok && (!a.keep || a.keep[i])) ? r : -1.0f;
  }
  __device__ __forceinline__ void visit(Shared& sh, int n, const WalkElem& e) {
    const float d2 = d2_of(e.g, e.n_cand, e.n_query);         // x = the centre: the d2 its radius was taken from
    const bool diag = a.exclude_diagonal && e.i0 == e.j0;     // Q is X: pair (i, i) lies on the diagonal of the diagonal tiles
    const bool self = diag && e.il == e.jl;
    const float c = self ? -1.0f : sh.rc[e.il], k = self ? -1.0f : sh.rk[e.il];
    cov[n] |= (d2 <= c) ? 1 : 0;
    const float dd = fmaxf(d2, FLT_MIN);
    // IEEE division only where the quotient can pass the running maximum: fl(k / dd) > mx needs k > mx dd (1 - 2^-24)
    if (k > 0.999f * mx[n] * dd) mx[n] = fmaxf(mx[n], fminf(k / dd, FLT_MAX));
  }
  __device__ __forceinline__ void park(Shared& sh, int p, int n, int jl) {
    sh.pmax[p][jl] = mx[n];
    sh.pcov[p][jl] = cov[n];
  }
  __device__ __forceinline__ void fold(Shared& sh, int jl, int64_t slot) {
    a.part_max[slot] = fmaxf(fmaxf(sh.pmax[0][jl], sh.pmax[1][jl]), fmaxf(sh.pmax[2][jl], sh.pmax[3][jl]));
    a.part_cov[slot] = (uint8_t)(sh.pcov[0][jl] | sh.pcov[1][jl] | sh.pcov[2][jl] | sh.pcov[3][jl]);
  }
};

__global__ __launch_bounds__(NT, 2) void ball_cover_partial_kernel(CoverArgs a) {
  CoverOp op{a};
  query_walk(Walk{a.q, a.ldq, a.nq, a.nrm_q, a.x, a.ldx, a.nx, a.nrm_x, a.d, a.tiles_x, a.splits}, op);   // rows: centres
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
  SMD_ARG_CHECK(fits_one_launch(tiles * splits), "smd_knn_radii: %lld tiles x %lld column splits exceed one launch (at most %lld workgroups)",
                (long long)tiles, (long long)splits, (long long)MAX_WORKGROUPS);      // reached at n ~ 2.1 M
  const int64_t need = smd_knn_radii_workspace_bytes(n, k);
  SMD_ARG_CHECK(workspace_bytes >= need, "smd_knn_radii: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* nrm = ws_at<float>(workspace, 0);
  if (const int e = launch_row_norms(x, n, ld, nrm, nullptr, 0, 0, nullptr, d, st)) return e;
  KnnArgs a;
  a.x = x; a.ld = ld; a.n = n; a.d = d; a.tiles = (int)tiles; a.splits = (int)splits; a.nrm = nrm;
  a.part = ws_at<float>(workspace, up8((int64_t)n * 4));
  return dispatch_k(k, [&](auto K) { return knn_launch<decltype(K)::value>(a, r2, st); });
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
  SMD_ARG_CHECK(fits_one_launch(tiles_q * splits), "smd_ball_cover: %lld query tiles x %lld centre splits exceed one launch (at most %lld workgroups)",
                (long long)tiles_q, (long long)splits, (long long)MAX_WORKGROUPS);
  const int64_t need = smd_ball_cover_workspace_bytes(nq, nx);
  SMD_ARG_CHECK(workspace_bytes >= need, "smd_ball_cover: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* nrm_q = ws_at<float>(workspace, 0);
  float* nrm_x = nrm_q + nq;
  float* part_max = ws_at<float>(workspace, up8(((int64_t)nq + nx) * 4));
  uint8_t* part_cov = reinterpret_cast<uint8_t*>(part_max + splits * nq);
  if (const int e = launch_row_norms(q, nq, ldq, nrm_q, x, nx, ldx, nrm_x, d, st)) return e;
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
