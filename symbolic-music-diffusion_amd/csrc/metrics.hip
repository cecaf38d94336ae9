// Sample-quality distances of the evaluation (reference utils/metrics.py:24-77, used by sample_ncsn.py:69-186) on exact-fp32
// MFMA (v_mfma_f32_32x32x2_f32): no bf16 anywhere, every product is an fp32 fma in k order.
//
//   pair_sums    sum_ij exp(-g_rbf max(d2_ij, 0)) and sum_ij (g_poly <x_i,y_j> + c0)^degree in ONE pass over X Y^T: the
//                Gram tile (gram_tile.h) stays in registers and both epilogues read it; the N x N kernel matrix is never written.
//                d2 = (-2 <x,y> + |x|^2) + |y|^2 in the order of sklearn 0.19's euclidean_distances (the pinned reference).
//   moments      fp64 column mean and ddof = 1 covariance: fp64 column sums, then the Gram of the centred fp32 rows on
//                the same MFMA, split over row slabs and reduced in fixed order in fp64 (frechet_distance's np.mean / np.cov).
//
// Determinism: every workgroup writes its fp64 partial to a slot of its own and a second launch sums the slots in a fixed
// order, so two calls on the same inputs give the same bits.  Nothing is allocated and nothing waits on the host.
#include "gram_tile.h"
#include "../../include/smd_hip.h"

namespace {

// ---------------------------------------------------------------------------------------------------- pair sums
struct PairArgs {
  const float* x; const float* y; int64_t ldx, ldy;
  int nx, ny, d, symmetric, degree, tiles_y;
  float g_rbf, g_poly, c0;
  const float* nrm_x; const float* nrm_y;
  double* partial;        // [gridDim.x][2]
};

__device__ __forceinline__ float powi_(float t, int degree) {
  float p = t;
  for (int e = 1; e < degree; ++e) p *= t;
  return p;
}

__global__ __launch_bounds__(NT) void pair_sums_kernel(PairArgs a) {
  __shared__ float As[BK * LDP];
  __shared__ float Bs[BK * LDP];
  __shared__ float na[MT], nb[MT];
  __shared__ double red[2][NT / SMD_WAVE];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wr = w >> 1, wc = w & 1;
  // tile of this workgroup: XCD-banded (smd_xcd_band) so that neighbouring tiles, which share operand rows, share an L2
  const int tile = smd_xcd_band(blockIdx.x, gridDim.x);
  int bi, bj;
  if (a.symmetric) {                       // upper triangle bi <= bj, row-major
    int rem = tile, T = a.tiles_y;
    bi = 0;
    while (rem >= T - bi) { rem -= T - bi; ++bi; }
    bj = bi + rem;
  } else {
    bi = tile / a.tiles_y;
    bj = tile - bi * a.tiles_y;
  }
  const int i0 = bi * MT, j0 = bj * MT;
  if (t < MT) na[t] = (i0 + t < a.nx) ? a.nrm_x[i0 + t] : 0.0f;
  else nb[t - MT] = (j0 + t - MT < a.ny) ? a.nrm_y[j0 + t - MT] : 0.0f;

  // Padded rows load zeros and are masked again in the epilogue: a zero row would still add exp(0) = 1.
  f32x16_t acc[2][2];
  gram_tile(a.x, a.ldx, a.nx, i0, a.y, a.ldy, a.ny, j0, a.d, As, Bs, acc);   // its barriers publish na, nb

  // epilogue: both kernels from the same Gram values; fp32 for the 16 values of one MFMA tile, then fp64
  const bool diag = a.symmetric && bi == bj;
  double sr = 0.0, sp = 0.0;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int jl = wc * 64 + n * 32 + (lane & 31), j = j0 + jl;
      const float nj = nb[jl];
      float tr = 0.0f, tp = 0.0f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int il = wr * 64 + m * 32 + cd_row(r, lane), i = i0 + il;
        const float g = acc[m][n][r];
        float d2 = fmaxf((-2.0f * g + na[il]) + nj, 0.0f);
        if (diag && i == j) d2 = 0.0f;     // sklearn: distances.flat[::n + 1] = 0 when X is Y
        const float kr = __expf(-a.g_rbf * d2);
        const float kp = powi_(a.g_poly * g + a.c0, a.degree);
        if (i < a.nx && j < a.ny) { tr += kr; tp += kp; }
      }
      sr += (double)tr;
      sp += (double)tp;
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sr += __shfl_xor(sr, o, 64);
    sp += __shfl_xor(sp, o, 64);
  }
  if (lane == 0) { red[0][w] = sr; red[1][w] = sp; }
  __syncthreads();
  if (t == 0) {
    const double wgt = (a.symmetric && bi != bj) ? 2.0 : 1.0;   // an off-diagonal tile stands for itself and its mirror
    double r0 = 0.0, r1 = 0.0;
    for (int q = 0; q < NT / SMD_WAVE; ++q) { r0 += red[0][q]; r1 += red[1][q]; }
    a.partial[2 * (int64_t)blockIdx.x] = wgt * r0;
    a.partial[2 * (int64_t)blockIdx.x + 1] = wgt * r1;
  }
}

// fixed-order sum of `n` interleaved pairs -> out[0], out[1]
__global__ __launch_bounds__(256) void reduce_pairs_kernel(const double* __restrict__ partial, int64_t n, double* __restrict__ out) {
  __shared__ double s0[256], s1[256];
  const int t = threadIdx.x;
  double a0 = 0.0, a1 = 0.0;
  for (int64_t i = t; i < n; i += 256) { a0 += partial[2 * i]; a1 += partial[2 * i + 1]; }
  s0[t] = a0; s1[t] = a1;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) { s0[t] += s0[t + h]; s1[t] += s1[t + h]; }
    __syncthreads();
  }
  if (t == 0) { out[0] = s0[0]; out[1] = s1[0]; }
}

// ---------------------------------------------------------------------------------------------------- moments
constexpr int MOM_SLAB_ROWS = 1024;    // rows per split before the split count is capped
constexpr int MOM_MAX_SPLITS = 16;

__host__ __device__ inline int mom_splits(int n) {
  const int s = (n + MOM_SLAB_ROWS - 1) / MOM_SLAB_ROWS;
  return s < 1 ? 1 : (s > MOM_MAX_SPLITS ? MOM_MAX_SPLITS : s);
}

// fp64 column sums of one row slab: part[split][c]
__global__ __launch_bounds__(256) void col_sums_kernel(const float* __restrict__ x, int n, int d, int64_t ld, int slab,
                                                       double* __restrict__ part) {
  const int c = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
  if (c >= d) return;
  const int r0 = s * slab, r1 = min(n, r0 + slab);
  double acc = 0.0;
  for (int r = r0; r < r1; ++r) acc += (double)x[(int64_t)r * ld + c];
  part[(int64_t)s * d + c] = acc;
}

__global__ __launch_bounds__(256) void col_mean_kernel(const double* __restrict__ part, int splits, int n, int d, double* __restrict__ mean) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= d) return;
  double acc = 0.0;
  for (int s = 0; s < splits; ++s) acc += part[(int64_t)s * d + c];
  mean[c] = acc / (double)n;
}

// Gram of the centred rows of one slab for one MT x MT tile of the d x d output: C[a][b] = sum_r xc[r][a] xc[r][b] with
// xc = fp32(x - mean).  The fp32 accumulators are added to fp64 ones every two stages (32 rows), so no fp32 sum runs
// longer than 32 terms.  Output: part[split][a][b] (fp64).
__global__ __launch_bounds__(NT) void centred_gram_kernel(const float* __restrict__ x, int n, int d, int64_t ld, int slab,
                                                          const double* __restrict__ mean, int tiles, double* __restrict__ part) {
  __shared__ float As[BK * LDP];
  __shared__ float Bs[BK * LDP];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wr = w >> 1, wc = w & 1;
  const int ta = blockIdx.x / tiles, tb = blockIdx.x - ta * tiles, s = blockIdx.y;
  const int a0 = ta * MT, b0 = tb * MT;
  const int r0 = s * slab, r1 = min(n, r0 + slab);
  // this thread always loads column t & 127 of the tile, rows (t >> 7) + 2 q of the stage: coalesced along the row
  const int col = t & (MT - 1), rq = t >> 7;
  const bool va = a0 + col < d, vb = b0 + col < d;
  const double ma = va ? mean[a0 + col] : 0.0, mb = vb ? mean[b0 + col] : 0.0;
  float ra[LOADS], rb[LOADS];
  auto load = [&](int k0) {
#pragma unroll
    for (int q = 0; q < LOADS; ++q) {
      const int r = k0 + rq + 2 * q;
      const bool vr = r < r1;
      ra[q] = (vr && va) ? (float)((double)x[(int64_t)r * ld + a0 + col] - ma) : 0.0f;
      rb[q] = (vr && vb) ? (float)((double)x[(int64_t)r * ld + b0 + col] - mb) : 0.0f;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int q = 0; q < LOADS; ++q) {
      As[(rq + 2 * q) * LDP + col] = ra[q];
      Bs[(rq + 2 * q) * LDP + col] = rb[q];
    }
  };
  f32x16_t acc[2][2];
  double acc64[2][2][16];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int nn = 0; nn < 2; ++nn)
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc[m][nn][r] = 0.0f; acc64[m][nn][r] = 0.0; }

  const int stages = r1 > r0 ? (r1 - r0 + BK - 1) / BK : 0;
  if (stages > 0) load(r0);
  for (int st = 0; st < stages; ++st) {
    __syncthreads();
    store();
    __syncthreads();
    if (st + 1 < stages) load(r0 + (st + 1) * BK);
    mfma_stage(As, Bs, wr, wc, lane, acc);
    if ((st & 1) || st + 1 == stages) {
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nn = 0; nn < 2; ++nn)
#pragma unroll
          for (int r = 0; r < 16; ++r) { acc64[m][nn][r] += (double)acc[m][nn][r]; acc[m][nn][r] = 0.0f; }
    }
  }
  double* out = part + (int64_t)s * d * d;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int nn = 0; nn < 2; ++nn) {
      const int b = b0 + wc * 64 + nn * 32 + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ai = a0 + wr * 64 + m * 32 + cd_row(r, lane);
        if (ai < d && b < d) out[(int64_t)ai * d + b] = acc64[m][nn][r];
      }
    }
}

__global__ __launch_bounds__(256) void cov_reduce_kernel(const double* __restrict__ part, int splits, int n, int64_t dd,
                                                         double* __restrict__ cov) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= dd) return;
  double acc = 0.0;
  for (int s = 0; s < splits; ++s) acc += part[(int64_t)s * dd + e];
  cov[e] = acc / (double)(n - 1);
}

int64_t pair_tiles(int nx, int ny, int symmetric) {
  const int64_t tx = tiles_of(nx), ty = tiles_of(ny);
  return symmetric ? tx * (tx + 1) / 2 : tx * ty;
}

}  // namespace

extern "C" {

int64_t smd_pair_kernel_sums_workspace_bytes(int nx, int ny, int symmetric) {
  if (nx < 1 || ny < 1 || (symmetric && nx != ny)) return -1;
  return up8((int64_t)(nx + (symmetric ? 0 : ny)) * 4) + pair_tiles(nx, ny, symmetric) * 16;
}

int smd_pair_kernel_sums(const float* x, int64_t ldx, int nx, const float* y, int64_t ldy, int ny, int d, int symmetric,
                         float gamma_rbf, float gamma_poly, float coef0, int degree, void* workspace, int64_t workspace_bytes,
                         double* out, void* stream) {
  SMD_ARG_CHECK(x && out && workspace, "smd_pair_kernel_sums: null pointer");
  SMD_ARG_CHECK(symmetric || y, "smd_pair_kernel_sums: null y (only symmetric mode takes y = NULL)");
  SMD_ARG_CHECK(nx >= 1 && ny >= 1 && d >= 1, "smd_pair_kernel_sums: nx=%d ny=%d d=%d must be >= 1", nx, ny, d);
  SMD_ARG_CHECK(ldx >= d && (symmetric || ldy >= d), "smd_pair_kernel_sums: row strides ldx=%lld ldy=%lld must be >= d=%d",
                (long long)ldx, (long long)ldy, d);
  SMD_ARG_CHECK(!symmetric || nx == ny, "smd_pair_kernel_sums: symmetric mode needs nx == ny (got %d, %d)", nx, ny);
  SMD_ARG_CHECK(degree >= 1, "smd_pair_kernel_sums: degree=%d must be >= 1", degree);
  SMD_ARG_CHECK(al4(x) && (!y || al4(y)) && al8(out) && al8(workspace), "smd_pair_kernel_sums: x, y must be 4-byte and out, workspace 8-byte aligned");
  const int64_t need = smd_pair_kernel_sums_workspace_bytes(nx, ny, symmetric);
  SMD_ARG_CHECK(workspace_bytes >= need, "smd_pair_kernel_sums: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)need);
  const int64_t tiles = pair_tiles(nx, ny, symmetric);
  SMD_ARG_CHECK(fits_one_launch(tiles), "smd_pair_kernel_sums: %lld tiles of %d x %d exceed one launch (at most %lld)",
                (long long)tiles, MT, MT, (long long)MAX_WORKGROUPS);      // reached at nx = ny ~ 524k, full mode
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* nrm_x = ws_at<float>(workspace, 0);
  float* nrm_y = symmetric ? nrm_x : nrm_x + nx;
  double* partial = ws_at<double>(workspace, up8((int64_t)(nx + (symmetric ? 0 : ny)) * 4));
  if (const int e = launch_row_norms(x, nx, ldx, nrm_x, symmetric ? nullptr : y, ny, ldy, nrm_y, d, st)) return e;
  if (symmetric) { y = x; ldy = ldx; }
  PairArgs a;
  a.x = x; a.y = y; a.ldx = ldx; a.ldy = ldy; a.nx = nx; a.ny = ny; a.d = d; a.symmetric = symmetric ? 1 : 0;
  a.degree = degree; a.tiles_y = (ny + MT - 1) / MT; a.g_rbf = gamma_rbf; a.g_poly = gamma_poly; a.c0 = coef0;
  a.nrm_x = nrm_x; a.nrm_y = nrm_y; a.partial = partial;
  pair_sums_kernel<<<(unsigned)tiles, NT, 0, st>>>(a);
  SMD_LAUNCH_CHECK();
  reduce_pairs_kernel<<<1, 256, 0, st>>>(partial, tiles, out);
  SMD_LAUNCH_CHECK();
  return 0;
}

int64_t smd_moments_workspace_bytes(int n, int d) {
  if (n < 2 || d < 1 || d > SMD_MOMENTS_MAX_D) return -1;
  const int64_t s = mom_splits(n);
  return s * d * 8 + s * (int64_t)d * d * 8;
}

int smd_moments(const float* x, int64_t ld, int n, int d, void* workspace, int64_t workspace_bytes, double* mean, double* cov,
                void* stream) {
  SMD_ARG_CHECK(x && workspace && mean && cov, "smd_moments: null pointer");
  SMD_ARG_CHECK(n >= 2, "smd_moments: n=%d rows; the ddof = 1 covariance needs at least 2", n);
  SMD_ARG_CHECK(d >= 1 && d <= SMD_MOMENTS_MAX_D, "smd_moments: d=%d must be in [1, %d]", d, SMD_MOMENTS_MAX_D);
  SMD_ARG_CHECK(ld >= d, "smd_moments: row stride ld=%lld must be >= d=%d", (long long)ld, d);
  SMD_ARG_CHECK(al4(x) && al8(workspace) && al8(mean) && al8(cov), "smd_moments: x must be 4-byte and workspace, mean, cov 8-byte aligned");
  const int64_t need = smd_moments_workspace_bytes(n, d);
  SMD_ARG_CHECK(workspace_bytes >= need, "smd_moments: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int splits = mom_splits(n), slab = (n + splits - 1) / splits, tiles = (d + MT - 1) / MT;
  double* sums = reinterpret_cast<double*>(workspace);
  double* part = sums + (int64_t)splits * d;
  col_sums_kernel<<<dim3((d + 255) / 256, splits), 256, 0, st>>>(x, n, d, ld, slab, sums);
  SMD_LAUNCH_CHECK();
  col_mean_kernel<<<(d + 255) / 256, 256, 0, st>>>(sums, splits, n, d, mean);
  SMD_LAUNCH_CHECK();
  centred_gram_kernel<<<dim3(tiles * tiles, splits), NT, 0, st>>>(x, n, d, ld, slab, mean, tiles, part);
  SMD_LAUNCH_CHECK();
  const int64_t dd = (int64_t)d * d;
  cov_reduce_kernel<<<(unsigned)((dd + 255) / 256), 256, 0, st>>>(part, splits, n, dd, cov);
  SMD_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
