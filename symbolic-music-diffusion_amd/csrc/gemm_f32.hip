// nn.Dense in reference precision: Y = epilogue(A W + b) on exact-fp32 MFMA (v_mfma_f32_32x32x2_f32), engine option "fp32".
//
//   A  fp32 [M][K] activations (row-major, k contiguous)
//   W  fp32 [K][N] the flax kernel, read IN PLACE from the master parameter buffer (n contiguous): the k-major layout is
//      exactly what the MFMA's B operand wants, so no copy, transpose or operand pack of the weights exists in this mode
//   epilogue: + bias[n]; tanh-GELU or swish; + fp32 residual (row m, or m % res_row_mod for the positional encoding)
//
// Operand map of the 32x32x2 MFMA as used (the same as metrics.hip): lane l supplies A[i = l & 31][k = l >> 5] and
// B[k = l >> 5][j = l & 31]; accumulator register r of lane l is C[(r & 3) + 8 (r >> 2) + 4 (l >> 5)][l & 31].
//
// Two tile forms, chosen from N alone:
//   128 x 128 (4 waves of 64 x 64 = 2 x 2 MFMA tiles)   N > 512: the 2048-wide Dense layers (DenseResBlocks, fc1, up, FiLM ss)
//    32 x 128 (4 waves of 32 x 32)                      N <= 512: the skinny outputs (128, 384, C), 4 x the workgroups
// Both stage BK = 16 of k through LDS ([k][row] with a pitch of rows + 4 floats: the transposing stores of the A loader and
// the MFMA reads are free of bank conflicts) with the next stage's global loads in flight under the MFMAs.
//
// Determinism / batch invariance: an output element is ONE accumulator that receives the k pairs (0,1), (2,3), ... in order,
// whatever M, N or the tile form (k past K and rows / columns past the edge load exact zeros).  No split over k, no atomics:
// a row of A gives the same bits in a problem of 256 rows and in one of 8192, and two calls give equal bits.
#include "f32_kernels.h"
#include "../../include/smd_hip.h"

namespace {

constexpr int BN = 128;
constexpr int BK = 16;
constexpr int NT = 256;
constexpr int LDB = BN + 4;

__device__ __forceinline__ int cd_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

__device__ __forceinline__ float act_f32(float v, int act) {
  if (act == SMD_F32_ACT_GELU) return geluf_(v);
  if (act == SMD_F32_ACT_SWISH) return swishf_(v);
  return v;
}

// MI x NI MFMA tiles per wave, WR x WC waves: workgroup tile (WR MI 32) x (WC NI 32), WC NI 32 == BN
template <int MI, int NI, int WR, int WC>
__global__ __launch_bounds__(NT) void gemm_f32_kernel(GemmF32Args a, int tiles_n, int vec_a, int vec_b) {
  constexpr int BM = WR * MI * 32;
  constexpr int LDA = BM + 4;
  constexpr int QA = (BM * BK + NT - 1) / NT;        // scalar A loads per thread and stage
  constexpr int QA4 = (BM * BK / 4 + NT - 1) / NT;   // 16-byte A loads
  constexpr int QB = BK * BN / NT;                   // 8
  constexpr int QB4 = QB / 4;                        // 2
  static_assert(WC * NI * 32 == BN && WR * WC == 4, "tile form");
  __shared__ __attribute__((aligned(16))) float As[BK * LDA];
  __shared__ __attribute__((aligned(16))) float Bs[BK * LDB];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wr = w / WC, wc = w % WC;
  const int tile = smd_xcd_band(blockIdx.x, gridDim.x);
  const int bm = tile / tiles_n, bn = tile - bm * tiles_n;
  const int m0 = bm * BM, n0 = bn * BN;

  float ra[QA4 * 4 > QA ? QA4 * 4 : QA];
  float rb[QB];
  auto load = [&](int k0) {
    if (vec_a) {      // lda % 4 == 0, K % 4 == 0, A 16-byte aligned: a group of four k is inside or outside as a whole
#pragma unroll
      for (int q = 0; q < QA4; ++q) {
        const int idx = t + NT * q, r = idx >> 2, k = k0 + 4 * (idx & 3);
        f32x4_t v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (idx < BM * BK / 4 && m0 + r < a.M && k < a.K) v = *reinterpret_cast<const f32x4_t*>(a.A + (size_t)(m0 + r) * a.lda + k);
        ra[4 * q] = v[0]; ra[4 * q + 1] = v[1]; ra[4 * q + 2] = v[2]; ra[4 * q + 3] = v[3];
      }
    } else {
#pragma unroll
      for (int q = 0; q < QA; ++q) {
        const int idx = t + NT * q, r = idx / BK, k = k0 + idx % BK;
        ra[q] = (idx < BM * BK && m0 + r < a.M && k < a.K) ? a.A[(size_t)(m0 + r) * a.lda + k] : 0.0f;
      }
    }
    if (vec_b) {      // ldw % 4 == 0, N % 4 == 0, W 16-byte aligned
#pragma unroll
      for (int q = 0; q < QB4; ++q) {
        const int idx = t + NT * q, k = k0 + (idx >> 5), n = n0 + 4 * (idx & 31);
        f32x4_t v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (k < a.K && n < a.N) v = *reinterpret_cast<const f32x4_t*>(a.W + (size_t)k * a.ldw + n);
        rb[4 * q] = v[0]; rb[4 * q + 1] = v[1]; rb[4 * q + 2] = v[2]; rb[4 * q + 3] = v[3];
      }
    } else {
#pragma unroll
      for (int q = 0; q < QB; ++q) {
        const int idx = t + NT * q, k = k0 + idx / BN, n = n0 + idx % BN;
        rb[q] = (k < a.K && n < a.N) ? a.W[(size_t)k * a.ldw + n] : 0.0f;
      }
    }
  };
  auto store = [&]() {
    if (vec_a) {
#pragma unroll
      for (int q = 0; q < QA4; ++q) {
        const int idx = t + NT * q, r = idx >> 2, kk = 4 * (idx & 3);
        if (idx < BM * BK / 4) {
#pragma unroll
          for (int j = 0; j < 4; ++j) As[(kk + j) * LDA + r] = ra[4 * q + j];
        }
      }
    } else {
#pragma unroll
      for (int q = 0; q < QA; ++q) {
        const int idx = t + NT * q, r = idx / BK, kk = idx % BK;
        if (idx < BM * BK) As[kk * LDA + r] = ra[q];
      }
    }
    if (vec_b) {
#pragma unroll
      for (int q = 0; q < QB4; ++q) {
        const int idx = t + NT * q;
        const f32x4_t v = {rb[4 * q], rb[4 * q + 1], rb[4 * q + 2], rb[4 * q + 3]};
        *reinterpret_cast<f32x4_t*>(&Bs[(idx >> 5) * LDB + 4 * (idx & 31)]) = v;
      }
    } else {
#pragma unroll
      for (int q = 0; q < QB; ++q) {
        const int idx = t + NT * q;
        Bs[(idx / BN) * LDB + idx % BN] = rb[q];
      }
    }
  };

  f32x16_t acc[MI][NI];
#pragma unroll
  for (int m = 0; m < MI; ++m)
#pragma unroll
    for (int n = 0; n < NI; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.0f;

  const int li = lane & 31, lk = lane >> 5;
  const int stages = (a.K + BK - 1) / BK;
  load(0);
  for (int s = 0; s < stages; ++s) {
    __syncthreads();                       // the previous stage's reads are done
    store();
    __syncthreads();
    if (s + 1 < stages) load((s + 1) * BK);
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      float av[MI], bv[NI];
#pragma unroll
      for (int m = 0; m < MI; ++m) av[m] = As[(kk + lk) * LDA + (wr * MI + m) * 32 + li];
#pragma unroll
      for (int n = 0; n < NI; ++n) bv[n] = Bs[(kk + lk) * LDB + (wc * NI + n) * 32 + li];
#pragma unroll
      for (int m = 0; m < MI; ++m)
#pragma unroll
        for (int n = 0; n < NI; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m], bv[n], acc[m][n], 0, 0, 0);
    }
  }

  // epilogue: 32 lanes write 32 consecutive columns of one row
#pragma unroll
  for (int n = 0; n < NI; ++n) {
    const int col = n0 + (wc * NI + n) * 32 + li;
    if (col >= a.N) continue;
    const float bias = a.bias ? a.bias[col] : 0.0f;
#pragma unroll
    for (int m = 0; m < MI; ++m) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + (wr * MI + m) * 32 + cd_row(r, lane);
        if (row >= a.M) continue;
        float v = act_f32(acc[m][n][r] + bias, a.act);
        if (a.res) v += a.res[(size_t)(a.res_row_mod > 0 ? row % a.res_row_mod : row) * a.ld_res + col];
        a.out[(size_t)row * a.ld_out + col] = v;
      }
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

int launch_gemm_f32(const GemmF32Args& a, hipStream_t st) {
  SMD_ARG_CHECK(a.A && a.W && a.out, "gemm_f32: null pointer");
  SMD_ARG_CHECK(a.M > 0 && a.N > 0 && a.K > 0, "gemm_f32: M=%d N=%d K=%d", a.M, a.N, a.K);
  SMD_ARG_CHECK(a.lda >= a.K && a.ldw >= a.N && a.ld_out >= a.N, "gemm_f32: leading dimension smaller than the row (lda=%d K=%d, ldw=%d ld_out=%d N=%d)",
                a.lda, a.K, a.ldw, a.ld_out, a.N);
  SMD_ARG_CHECK(!a.res || (a.ld_res >= a.N && a.res_row_mod >= 0), "gemm_f32: residual ld_res=%d N=%d row_mod=%d", a.ld_res, a.N, a.res_row_mod);
  SMD_ARG_CHECK(a.act >= SMD_F32_ACT_NONE && a.act <= SMD_F32_ACT_SWISH, "gemm_f32: act=%d", a.act);
  SMD_ARG_CHECK(((reinterpret_cast<uintptr_t>(a.A) | reinterpret_cast<uintptr_t>(a.W) | reinterpret_cast<uintptr_t>(a.out) |
                  reinterpret_cast<uintptr_t>(a.bias) | reinterpret_cast<uintptr_t>(a.res)) & 3u) == 0, "gemm_f32: pointers must be 4-byte aligned");
  const int vec_a = aligned16(a.A) && a.lda % 4 == 0 && a.K % 4 == 0;
  const int vec_b = aligned16(a.W) && a.ldw % 4 == 0 && a.N % 4 == 0;
  const int tiles_n = (a.N + BN - 1) / BN;
  if (a.N > 512) {
    const long tiles = (long)((a.M + 127) / 128) * tiles_n;
    SMD_ARG_CHECK(tiles < (1L << 30), "gemm_f32: problem too large");
    hipLaunchKernelGGL((gemm_f32_kernel<2, 2, 2, 2>), dim3((unsigned)tiles), dim3(NT), 0, st, a, tiles_n, vec_a, vec_b);
  } else {
    const long tiles = (long)((a.M + 31) / 32) * tiles_n;
    SMD_ARG_CHECK(tiles < (1L << 30), "gemm_f32: problem too large");
    hipLaunchKernelGGL((gemm_f32_kernel<1, 1, 1, 4>), dim3((unsigned)tiles), dim3(NT), 0, st, a, tiles_n, vec_a, vec_b);
  }
  SMD_LAUNCH_CHECK();
  return 0;
}

extern "C" int smd_gemm_f32(const float* A, int lda, const float* W, int ldw, int M, int N, int K, const float* bias, int act,
                            const float* residual, int ld_res, int res_row_mod, float* out, int ld_out, void* stream) {
  GemmF32Args a;
  a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.M = M; a.N = N; a.K = K; a.bias = bias; a.act = act;
  a.res = residual; a.ld_res = ld_res; a.res_row_mod = res_row_mod; a.out = out; a.ld_out = ld_out;
  return launch_gemm_f32(a, reinterpret_cast<hipStream_t>(stream));
}
