// What the fused sampler updates -- reverse_step_kernel, strided_step_kernel, multistep_step_kernel (diffusion.hip; DESIGN.md
// sections 16, 18) -- and the variational bound's kernels (bound.hip, section 17) have in common, as helpers that are inlined
// into each kernel: element moves, the Philox quad-or-pick, a key-table row, the metrics' root and workgroup tail, the
// last-arriver store, and on the host the (VEC, RG) launch.  The kernels keep their row loops: one walk shared as a template
// changed the register allocation of the step kernels and cost speed (section 16, "Shared helpers").
//
// Work split of all of them: one workgroup per sample, 128 column threads x RG row groups (RG = 4 for sequence states: four rows
// of every column in flight instead of one), VEC = 4 columns per thread when C % 4 == 0.
#pragma once
#include "smd_kernels.h"
#include "rng_threefry.h"
#include "rng.h"

namespace {

// ---------------------------------------------------------------------------------------------------- element moves
template <int VEC>
__device__ __forceinline__ void ldv(const float* p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = *p;
  }
}
template <int VEC>
__device__ __forceinline__ void stv(float* p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}
// the bf16 re-cast: one 8-byte store of four, or one element
template <int VEC>
__device__ __forceinline__ void stv_bf16(bf16_t* p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    bf16x4_t o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = f2bf(v[i]);
    *reinterpret_cast<bf16x4_t*>(p) = o;
  } else {
    p[0] = f2bf(v[0]);
  }
}

// ---------------------------------------------------------------------------------------------------- draws
// element e .. e + VEC of a sample from the Philox quad that holds it (VEC = 4: e % 4 == 0, the whole quad)
template <int VEC>
__device__ __forceinline__ void philox_normals(float (&out)[VEC], int e, uint32_t bglob, uint32_t stream, uint32_t t,
                                               uint32_t key_lo, uint32_t key_hi) {
  const float4 n4 = philox_normal4((uint32_t)(e >> 2), bglob, stream, t, key_lo, key_hi);
  if constexpr (VEC == 4) { out[0] = n4.x; out[1] = n4.y; out[2] = n4.z; out[3] = n4.w; }
  else out[0] = pick4(n4, e & 3);
}

// row `row` of a jax.random key table [rows][2]; no table: a key that is never used
__device__ __forceinline__ TfKey tf_key_row(const uint32_t* table, int row) {
  TfKey k{0, 0};
  if (table) { k.k0 = table[2 * row]; k.k1 = table[2 * row + 1]; }
  return k;
}

// ---------------------------------------------------------------------------------------------------- sums
// sqrt(sum(v^2, axis=1) + 1e-10) of the reference's metrics (utils/ebm_utils.py:157-161, :381-383): axis 1 is the SEQUENCE
// axis for (B,S,C) states -- a root per column, summed over the columns -- and the channel axis for the 2-D (B,C) states of
// DenseDDPM (S == 1): the columns' squares are summed and the root is taken once, by the workgroup.
__device__ __forceinline__ float norm_of(float sum_sq) { return sqrtf(sum_sq + 1e-10f); }

// Three sums over the threads of the two column waves (row group 0: threads 0..127; the other waves' values are not used):
// thread i < 3 returns sum i.  One barrier.
__device__ __forceinline__ float column_waves_sum3(float s0, float s1, float s2) {
  __shared__ float red[2][3];
  s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0 && w < 2) { red[w][0] = s0; red[w][1] = s1; red[w][2] = s2; }
  __syncthreads();
  return threadIdx.x < 3 ? red[0][threadIdx.x] + red[1][threadIdx.x] : 0.f;
}

// metrics_partial[t][b][:] of a sample from its threads' three sums
__device__ __forceinline__ void store_metrics(float* metrics_partial, int t, int B, int b, int S, float m0, float m1, float m2) {
  float v = column_waves_sum3(m0, m1, m2);
  if (threadIdx.x < 3) {
    if (S == 1) v = norm_of(v);
    metrics_partial[((size_t)t * B + b) * 3 + threadIdx.x] = v;
  }
}

// True in the LAST workgroup of the grid to get here, called by one thread of every workgroup: that one stores the walk's next
// timestep, without a launch of its own (every workgroup read the old one at its top, i.e. before its own arrival).  `arrive`
// is zero between launches: the last arriver resets it with a device-scope atomic.
__device__ __forceinline__ bool last_arriver(unsigned* arrive) {
  const unsigned prev = __hip_atomic_fetch_add(arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (prev != gridDim.x - 1) return false;
  __hip_atomic_exchange(arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}
__device__ __forceinline__ void last_arriver_store(unsigned* arrive, int* dst, int value) {
  if (last_arriver(arrive)) __hip_atomic_store(dst, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------------- host side
// (the launchers of diffusion.hip and bound.hip: each translation unit gets its own copy in its anonymous namespace)
inline bool al16(uintptr_t p) { return (p & 15) == 0; }

// kernel<VEC, RG> on B workgroups of 128 * RG threads: VEC = 4 on the vector path, RG = 4 for states of at least four rows
#define SMD_LAUNCH_VEC_RG(kernel, vec, a, st)                                                       \
  do {                                                                                              \
    if ((a).S >= 4) {                                                                               \
      if (vec) hipLaunchKernelGGL((kernel<4, 4>), dim3((a).B), dim3(512), 0, st, a);                \
      else hipLaunchKernelGGL((kernel<1, 4>), dim3((a).B), dim3(512), 0, st, a);                    \
    } else {                                                                                        \
      if (vec) hipLaunchKernelGGL((kernel<4, 1>), dim3((a).B), dim3(128), 0, st, a);                \
      else hipLaunchKernelGGL((kernel<1, 1>), dim3((a).B), dim3(128), 0, st, a);                    \
    }                                                                                               \
  } while (0)

}  // namespace
