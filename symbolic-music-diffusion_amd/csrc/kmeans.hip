// Full-batch Lloyd k-means over latent frames: the primitive of the PRD precision / recall histogram (Sajjadi et al. 2018) and
// of the NDB score (Richardson & Weiss 2018) that the reference's evaluate() logs (sample_ncsn.py:141-146,160; DESIGN.md
// section 15).
//
//   kmeans_assign   labels[i] = arg min_j s_ij,  s_ij = -2 <x_i, c_j> + |c_j|^2, ties to the lowest j;  min_d2, inertia, changed.
//   kmeans_update   counts[j] and the mean of every cluster's rows; a cluster without rows keeps its centre.
//
// Assignment is ONE pass of the Gram tile of gram_tile.h (exact-fp32 MFMA, every product an fp32 fma in k order).  Orientation
// as in nn_metrics.hip: the rows whose answer is sought (a 128-row slab of X) are the COLUMNS of the accumulator tile and the
// centres (at most 128: one tile) its rows, so a lane owns two rows of X and sees 32 centres of each in its registers; the
// four partial minima of a row (2 centre halves of the tile x 2 lane halves) meet in LDS.  |x_i|^2 is the same for every j and
// takes no part in the order; it enters min_d2 = max(s + |x_i|^2, 0) only.
//
// The update is a labelled segmented sum: a workgroup is one wave, a thread owns one column of a 64-column strip and walks a
// slab of rows in order, adding into acc[label][column] in LDS in fp64 (k x 64 doubles: consecutive lanes hit consecutive
// columns, no bank conflicts, and no two lanes share an address).  A second launch adds the slabs' partials in a fixed order,
// divides and writes.
//
// Determinism: no floating-point atomics and no integer ones either.  Every workgroup writes its partial (inertia, changed
// labels, cluster sums, cluster counts) to a slot of its own and a second launch adds the slots in a fixed order that depends on
// the launch geometry alone.  Two calls give the same bits.
#include <math.h>

#include "gram_tile.h"
#include "../../include/smd_hip.h"

namespace {

constexpr int KMAX = SMD_KMEANS_MAX_K;
static_assert(KMAX == MT && KMAX <= 2 * 64, "the centres are one tile of the Gram pass; a lane counts two clusters");
constexpr int UPD_ROWS = 256;      // rows per slab of the update
constexpr int UPD_COLS = 64;       // columns per strip: one per lane

inline int64_t slabs_of(int n) { return ((int64_t)n + UPD_ROWS - 1) / UPD_ROWS; }
inline int64_t strips_of(int d) { return ((int64_t)d + UPD_COLS - 1) / UPD_COLS; }

// ---------------------------------------------------------------------------------------------------- assignment
struct AssignArgs {
  const float* x; int64_t ld;
  const float* c;
  int n, d, k, has_prev;
  const float* nx; const float* nc;      // |x_i|^2 [n], |c_j|^2 [k]
  int32_t* labels; float* min_d2;        // min_d2 may be null
  double* part_inertia;                  // [tiles]
  int64_t* part_changed;                 // [tiles]
};

__global__ __launch_bounds__(NT, 2) void kmeans_assign_kernel(AssignArgs a) {
  __shared__ float As[BK * LDP];
  __shared__ float Bs[BK * LDP];
  __shared__ float ncs[MT];
  __shared__ float ps[4][MT];
  __shared__ int pj[4][MT];
  __shared__ double red[MT];
  __shared__ int chg[MT];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wr = w >> 1, wc = w & 1;
  const int i0 = blockIdx.x * MT;
  if (t < MT) ncs[t] = (t < a.k) ? a.nc[t] : INFINITY;         // a padded centre is never below a real one

  f32x16_t acc[2][2];
  gram_tile(a.c, a.d, a.k, 0, a.x, a.ld, a.n, i0, a.d, As, Bs, acc);   // rows: centres, columns: rows of X (its barriers publish ncs)
  const int p = wr * 2 + (lane >> 5);
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    float best = INFINITY;
    int bj = 0;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) {                           // ascending centre index: '<' keeps the lowest of equals
        const int jl = wr * 64 + m * 32 + cd_row(r, lane);
        const float s = fmaf(-2.0f, acc[m][n][r], ncs[jl]);    // -2 g is exact: one rounding, of the sum
        if (s < best) { best = s; bj = jl; }
      }
    ps[p][wc * 64 + n * 32 + (lane & 31)] = best;
    pj[p][wc * 64 + n * 32 + (lane & 31)] = bj;
  }
  __syncthreads();
  if (t < MT) {
    double d2 = 0.0;
    int ch = 0;
    const int i = i0 + t;
    if (i < a.n) {
      float bs = ps[0][t];
      int bj = pj[0][t];
#pragma unroll
      for (int q = 1; q < 4; ++q) {
        const float s = ps[q][t];
        const int j = pj[q][t];
        if (s < bs || (s == bs && j < bj)) { bs = s; bj = j; }
      }
      const float m2 = fmaxf(bs + a.nx[i], 0.0f);
      ch = a.has_prev ? (a.labels[i] != bj) : 1;
      a.labels[i] = bj;
      if (a.min_d2) a.min_d2[i] = m2;
      d2 = (double)m2;
    }
    red[t] = d2;
    chg[t] = ch;
  }
  for (int h = MT / 2; h > 0; h >>= 1) {                       // fixed tree over the slab's rows
    __syncthreads();
    if (t < h) { red[t] += red[t + h]; chg[t] += chg[t + h]; }
  }
  if (t == 0) {
    a.part_inertia[blockIdx.x] = red[0];
    a.part_changed[blockIdx.x] = chg[0];
  }
}

// fixed-order sums of the slabs' partials -> inertia, changed
__global__ __launch_bounds__(256) void kmeans_assign_reduce_kernel(const double* __restrict__ part_inertia,
                                                                   const int64_t* __restrict__ part_changed, int64_t tiles,
                                                                   double* __restrict__ inertia, int64_t* __restrict__ changed) {
  __shared__ double s0[256];
  __shared__ int64_t s1[256];
  const int t = threadIdx.x;
  double a0 = 0.0;
  int64_t a1 = 0;
  for (int64_t i = t; i < tiles; i += 256) { a0 += part_inertia[i]; a1 += part_changed[i]; }
  s0[t] = a0; s1[t] = a1;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) { s0[t] += s0[t + h]; s1[t] += s1[t + h]; }
    __syncthreads();
  }
  if (t == 0) { *inertia = s0[0]; *changed = s1[0]; }
}

// ---------------------------------------------------------------------------------------------------- update
// grid (slabs, strips), one wave: acc[j][lane] += x[r][c0 + lane] for the slab's rows r in order, j = labels[r]
__global__ __launch_bounds__(UPD_COLS) void kmeans_partial_sums_kernel(const float* __restrict__ x, int64_t ld, int n, int d, int k,
                                                                       const int32_t* __restrict__ labels, double* __restrict__ part,
                                                                       int32_t* __restrict__ part_cnt) {
  extern __shared__ double sacc[];                             // [k][UPD_COLS]; a lane reads and writes its own column only
  const int lane = threadIdx.x, slab = blockIdx.x, c = blockIdx.y * UPD_COLS + lane;
  for (int j = 0; j < k; ++j) sacc[j * UPD_COLS + lane] = 0.0;
  int cnt0 = 0, cnt1 = 0;                                      // rows of clusters lane and lane + 64
  const int r0 = slab * UPD_ROWS, r1 = min(n, r0 + UPD_ROWS);
  constexpr int U = 8;                                         // rows whose loads are in flight together
  for (int rb = r0; rb < r1; rb += U) {
    float v[U];
    int lab[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int r = rb + u;
      const bool ok = r < r1;
      lab[u] = ok ? labels[r] : -1;
      v[u] = (ok && c < d) ? x[(int64_t)r * ld + c] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = lab[u];
      if (j >= 0 && j < k) {                                   // wave-uniform; a label outside [0, k) is skipped, never an index
        sacc[j * UPD_COLS + lane] += (double)v[u];
        cnt0 += (j == lane);
        cnt1 += (j == lane + UPD_COLS);
      }
    }
  }
  if (c < d)
    for (int j = 0; j < k; ++j) part[((int64_t)slab * k + j) * d + c] = sacc[j * UPD_COLS + lane];
  if (blockIdx.y == 0) {                                       // the first strip counts the rows for all
    if (lane < k) part_cnt[(int64_t)slab * k + lane] = cnt0;
    if (lane + UPD_COLS < k) part_cnt[(int64_t)slab * k + lane + UPD_COLS] = cnt1;
  }
}

// element e = j d + c of 64 per workgroup; the slabs are cut into four runs of consecutive slabs, one per wave, each added in
// slab order, and the four run sums are added in run order: fixed by (slabs, k, d) alone.  Then the mean, or the previous centre
// for an empty cluster.
__global__ __launch_bounds__(256) void kmeans_means_kernel(const double* __restrict__ part, const int32_t* __restrict__ part_cnt,
                                                           int slabs, int k, int d, const float* __restrict__ prev,
                                                           float* __restrict__ centres, int64_t* __restrict__ counts) {
  __shared__ double ssum[4][64];
  __shared__ int64_t scnt[4][64];
  const int q = threadIdx.x >> 6, el = threadIdx.x & 63;
  const int e = blockIdx.x * 64 + el;
  const bool ok = e < k * d;
  const int j = ok ? e / d : 0;
  const int per = (slabs + 3) / 4, s0 = q * per, s1 = min(slabs, s0 + per);
  double s = 0.0;
  int64_t m = 0;
  if (ok) {
#pragma unroll 4
    for (int sl = s0; sl < s1; ++sl) {
      s += part[(int64_t)sl * k * d + e];
      m += part_cnt[(int64_t)sl * k + j];
    }
  }
  ssum[q][el] = s;
  scnt[q][el] = m;
  __syncthreads();
  if (q == 0 && ok) {
    s = ((ssum[0][el] + ssum[1][el]) + ssum[2][el]) + ssum[3][el];
    m = scnt[0][el] + scnt[1][el] + scnt[2][el] + scnt[3][el];
    const float old = prev[e];                                 // read first: centres may alias prev_centres
    centres[e] = m > 0 ? (float)(s / (double)m) : old;
    if (e - j * d == 0) counts[j] = m;
  }
}

}  // namespace

extern "C" {

int64_t smd_kmeans_assign_workspace_bytes(int n, int k) {
  if (n < 1 || k < 1 || k > KMAX) return -1;
  return up8((int64_t)n * 4) + up8((int64_t)KMAX * 4) + tiles_of(n) * 16;
}

int smd_kmeans_assign(const float* x, int64_t ld, int n, int d, const float* centres, int k, int prev, void* workspace,
                      int64_t workspace_bytes, int32_t* labels, float* min_d2, double* inertia, int64_t* changed, void* stream) {
  SMD_ARG_CHECK(x && centres && workspace && labels && inertia && changed, "smd_kmeans_assign: null pointer (only min_d2 may be NULL)");
  SMD_ARG_CHECK(k >= 1 && k <= KMAX, "smd_kmeans_assign: k=%d must be in [1, %d]", k, KMAX);
  SMD_ARG_CHECK(n >= 1 && n <= INT32_MAX - MT && d >= 1, "smd_kmeans_assign: n=%d d=%d must be >= 1 (n at most %d)", n, d, INT32_MAX - MT);
  SMD_ARG_CHECK(ld >= d, "smd_kmeans_assign: row stride ld=%lld must be >= d=%d", (long long)ld, d);
  SMD_ARG_CHECK(al4(x) && al4(centres) && al4(labels) && al4(min_d2) && al8(inertia) && al8(changed) && al8(workspace),
                "smd_kmeans_assign: x, centres, labels, min_d2 must be 4-byte and inertia, changed, workspace 8-byte aligned");
  const int64_t tiles = tiles_of(n);
  // any int n stays below the bound; the check keeps that true should the tile shrink
  SMD_ARG_CHECK(fits_one_launch(tiles), "smd_kmeans_assign: %lld row slabs exceed one launch (at most %lld workgroups)",
                (long long)tiles, (long long)MAX_WORKGROUPS);
  const int64_t need = smd_kmeans_assign_workspace_bytes(n, k);
  SMD_ARG_CHECK(workspace_bytes >= need, "smd_kmeans_assign: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* nx = ws_at<float>(workspace, 0);
  float* nc = ws_at<float>(workspace, up8((int64_t)n * 4));
  double* part_inertia = ws_at<double>(workspace, up8((int64_t)n * 4) + up8((int64_t)KMAX * 4));
  int64_t* part_changed = reinterpret_cast<int64_t*>(part_inertia + tiles);
  if (const int e = launch_row_norms(x, n, ld, nx, centres, k, (int64_t)d, nc, d, st)) return e;
  AssignArgs a;
  a.x = x; a.ld = ld; a.c = centres; a.n = n; a.d = d; a.k = k; a.has_prev = prev ? 1 : 0; a.nx = nx; a.nc = nc;
  a.labels = labels; a.min_d2 = min_d2; a.part_inertia = part_inertia; a.part_changed = part_changed;
  kmeans_assign_kernel<<<(unsigned)tiles, NT, 0, st>>>(a);
  SMD_LAUNCH_CHECK();
  kmeans_assign_reduce_kernel<<<1, 256, 0, st>>>(part_inertia, part_changed, tiles, inertia, changed);
  SMD_LAUNCH_CHECK();
  return 0;
}

int64_t smd_kmeans_update_workspace_bytes(int n, int d, int k) {
  if (n < 1 || d < 1 || k < 1 || k > KMAX) return -1;
  return slabs_of(n) * k * d * 8 + up8(slabs_of(n) * k * 4);
}

int smd_kmeans_update(const float* x, int64_t ld, int n, int d, const int32_t* labels, const float* prev_centres, int k,
                      void* workspace, int64_t workspace_bytes, float* centres, int64_t* counts, void* stream) {
  SMD_ARG_CHECK(x && labels && prev_centres && workspace && centres && counts, "smd_kmeans_update: null pointer");
  SMD_ARG_CHECK(k >= 1 && k <= KMAX, "smd_kmeans_update: k=%d must be in [1, %d]", k, KMAX);
  SMD_ARG_CHECK(n >= 1 && n <= INT32_MAX - UPD_ROWS && d >= 1, "smd_kmeans_update: n=%d d=%d must be >= 1 (n at most %d)", n, d, INT32_MAX - UPD_ROWS);
  SMD_ARG_CHECK(ld >= d, "smd_kmeans_update: row stride ld=%lld must be >= d=%d", (long long)ld, d);
  SMD_ARG_CHECK(al4(x) && al4(labels) && al4(prev_centres) && al4(centres) && al8(counts) && al8(workspace),
                "smd_kmeans_update: x, labels, prev_centres, centres must be 4-byte and counts, workspace 8-byte aligned");
  const int64_t slabs = slabs_of(n), strips = strips_of(d);
  SMD_ARG_CHECK(strips <= 65535 && slabs * strips * UPD_COLS < ((int64_t)1 << 32) && (int64_t)k * d < ((int64_t)1 << 31),
                "smd_kmeans_update: %lld row slabs x %lld column strips (k d = %lld) exceed one launch", (long long)slabs,
                (long long)strips, (long long)k * d);
  const int64_t need = smd_kmeans_update_workspace_bytes(n, d, k);
  SMD_ARG_CHECK(workspace_bytes >= need, "smd_kmeans_update: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  double* part = reinterpret_cast<double*>(workspace);
  int32_t* part_cnt = reinterpret_cast<int32_t*>(part + slabs * k * d);
  const size_t lds = (size_t)k * UPD_COLS * 8;                     // 64 KiB at k = 128
  kmeans_partial_sums_kernel<<<dim3((unsigned)slabs, (unsigned)strips), UPD_COLS, lds, st>>>(x, ld, n, d, k, labels, part, part_cnt);
  SMD_LAUNCH_CHECK();
  kmeans_means_kernel<<<(unsigned)(((int64_t)k * d + 63) / 64), 256, 0, st>>>(part, part_cnt, (int)slabs, k, d, prev_centres, centres, counts);
  SMD_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
