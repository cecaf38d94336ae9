// The 128 x 128 Gram tile on exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) that the evaluation kernels share: metrics.hip (pair
// sums, moments), kmeans.hip (assignment) and, through the query-column walk of gram_walk.h, nn_metrics.hip and nn_search.hip.
// Every product is an fp32 fma in k order.  The row norms and the host-side helpers of those files' entry points live here too.
#pragma once
#include "smd_common.h"

namespace {

constexpr int MT = 128;        // workgroup tile: MT x MT outputs, 4 waves of 64 x 64 (2 x 2 MFMA tiles of 32 x 32)
constexpr int BK = 16;         // k per LDS stage
constexpr int LDP = MT + 4;    // LDS pitch in floats: the transposing stores of the pair loader hit 64 distinct banks
constexpr int NT = 256;
constexpr int LOADS = MT * BK / NT;   // 8 floats per operand per thread and stage

// One LDS stage: As / Bs hold [BK][LDP] (k-major), wave (wr, wc) owns rows wr*64.. and columns wc*64.. of the tile.
// 32x32x2 operand map: lane l supplies A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31].
__device__ __forceinline__ void mfma_stage(const float* As, const float* Bs, int wr, int wc, int lane, f32x16_t (&acc)[2][2]) {
  const int li = lane & 31, lk = lane >> 5;
#pragma unroll
  for (int kk = 0; kk < BK; kk += 2) {
    float a[2], b[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) a[m] = As[(kk + lk) * LDP + wr * 64 + m * 32 + li];
#pragma unroll
    for (int n = 0; n < 2; ++n) b[n] = Bs[(kk + lk) * LDP + wc * 64 + n * 32 + li];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], b[n], acc[m][n], 0, 0, 0);
  }
}

// C/D map of the 32x32 MFMA: column lane & 31, row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
__device__ __forceinline__ int cd_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

// acc = X[i0 .. i0 + MT) Y[j0 .. j0 + MT)^T over all of d for one workgroup of NT threads: element q of a thread's stage is
// (row idx / BK, k idx % BK), idx = t + NT q -- 16 consecutive k of a row per 16 lanes.  Rows past nx / ny and k past d load
// zeros and nothing outside the operands is read; the caller masks the padded rows and columns of the result.  The first
// barrier also orders this call's LDS stores after whatever the workgroup read from As / Bs before it.
__device__ __forceinline__ void gram_tile(const float* __restrict__ x, int64_t ldx, int nx, int i0, const float* __restrict__ y,
                                          int64_t ldy, int ny, int j0, int d, float* As, float* Bs, f32x16_t (&acc)[2][2]) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wr = w >> 1, wc = w & 1;
  float ra[LOADS], rb[LOADS];
  auto load = [&](int k0) {
#pragma unroll
    for (int q = 0; q < LOADS; ++q) {
      const int idx = t + NT * q, r = idx / BK, k = k0 + idx % BK;
      ra[q] = (i0 + r < nx && k < d) ? x[(int64_t)(i0 + r) * ldx + k] : 0.0f;
      rb[q] = (j0 + r < ny && k < d) ? y[(int64_t)(j0 + r) * ldy + k] : 0.0f;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int q = 0; q < LOADS; ++q) {
      const int idx = t + NT * q, r = idx / BK, kk = idx % BK;
      As[kk * LDP + r] = ra[q];
      Bs[kk * LDP + r] = rb[q];
    }
  };
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.0f;
  const int stages = (d + BK - 1) / BK;
  load(0);
  for (int s = 0; s < stages; ++s) {
    __syncthreads();                       // the previous stage's reads are done
    store();
    __syncthreads();
    if (s + 1 < stages) load((s + 1) * BK);   // next stage's global reads in flight under this stage's MFMAs
    mfma_stage(As, Bs, wr, wc, lane, acc);
  }
}

// ---------------------------------------------------------------------------------------------------- row norms
// |x_i|^2 as ONE fmaf chain in k order from 0 -- the same chain the MFMA forms for <x_i, x_i> (zero padding adds exact
// zeros), so a row against itself or its duplicate gives d2 = (-2n + n) + n = 0 exactly.
__global__ __launch_bounds__(256) void row_norms_kernel(const float* __restrict__ x, int n, int d, int64_t ld, float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* r = x + (int64_t)i * ld;
  float s = 0.0f;
  for (int k = 0; k < d; ++k) s = fmaf(r[k], r[k], s);
  out[i] = s;
}

// |row|^2 of the n rows of x into nrm, and of the ny rows of y into nrm_y unless y is null
inline int launch_row_norms(const float* x, int n, int64_t ld, float* nrm, const float* y, int ny, int64_t ldy, float* nrm_y, int d,
                            hipStream_t st) {
  row_norms_kernel<<<(n + 255) / 256, 256, 0, st>>>(x, n, d, ld, nrm);
  SMD_LAUNCH_CHECK();
  if (y) {
    row_norms_kernel<<<(ny + 255) / 256, 256, 0, st>>>(y, ny, d, ldy, nrm_y);
    SMD_LAUNCH_CHECK();
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------- host side
inline int64_t tiles_of(int n) { return ((int64_t)n + MT - 1) / MT; }

// HIP bounds a launch by gridDim.x * blockDim.x < 2^32 work-items: 2^24 - 1 workgroups of NT = 256
constexpr int64_t MAX_WORKGROUPS = (((int64_t)1 << 32) - 1) / NT;
inline bool fits_one_launch(int64_t workgroups) { return workgroups * NT < ((int64_t)1 << 32); }

inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
inline bool al8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
inline int64_t up8(int64_t b) { return (b + 7) & ~(int64_t)7; }
// the part of a workspace that starts `bytes` into it
template <typename T>
inline T* ws_at(void* workspace, int64_t bytes) { return reinterpret_cast<T*>(reinterpret_cast<char*>(workspace) + bytes); }

}  // namespace
