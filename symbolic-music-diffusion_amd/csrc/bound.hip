// HBM-bound elementwise kernels of the per-timestep variational bound (Ho et al. 2020, eq. 5).
//
//   bound_noise    x_t = sqrt(ap_t) x0 + sqrt(1-ap_t) eps on an example: fp32 + the engine's bf16 network input
//   bound_terms    the three per-example sums behind L_t: |x0 - x0_hat|^2, |eps - eps_hat|^2, |x0|^2
//
// The work split is reverse_step_kernel's (diffusion.hip): one workgroup per sample, 128 column threads x RG row groups,
// VEC = 4 columns per thread when C % 4 == 0.  The timestep is read from device memory and the walk's next timestep comes
// from a table, so one captured (noise, eps-net forward, terms) iteration replays for a whole walk.
#include "step_walk.h"

namespace {

// ------------------------------------------------------------------ forward noising of an example
template <int VEC, int RG>
__global__ __launch_bounds__(128 * RG) void bound_noise_kernel(BoundNoiseArgs a) {
  const int t = *a.t_ptr;
  if (t < 0 || t >= a.T) return;          // the walk's terminator (or a bad timestep): nothing is written
  const float4 row = *reinterpret_cast<const float4*>(a.table + (size_t)t * 4);
  const float sqrt_ap = row.x, sqrt_1m = row.y;
  const int b = blockIdx.x;
  const int ct = threadIdx.x & 127, rg = threadIdx.x >> 7;
  const uint32_t bglob = (uint32_t)b + a.sample_offset;
  const size_t sample_base = (size_t)b * a.S * a.C;
  const uint32_t key_lo = a.key_ptr ? a.key_ptr[0] : a.key.seed_lo, key_hi = a.key_ptr ? a.key_ptr[1] : a.key.seed_hi;
  for (int cb = 0; cb < a.C; cb += 128 * VEC) {
    const int col0 = cb + ct * VEC;
    if (col0 >= a.C) continue;
    for (int s = rg; s < a.S; s += RG) {
      const int e = s * a.C + col0;
      const size_t idx = sample_base + e;
      float x0[VEC], ep[VEC], xt[VEC];
      ldv<VEC>(a.x0 + idx, x0);
      if (a.draw) {                        // Philox keyed by (seed, global sample index, t) on the bound's own stream
        philox_normals<VEC>(ep, e, bglob, SMD_STREAM_BOUND, (uint32_t)t, key_lo, key_hi);
        stv<VEC>(a.eps + idx, ep);
      } else {
        ldv<VEC>(a.eps + idx, ep);
      }
#pragma unroll
      for (int v = 0; v < VEC; ++v) xt[v] = __builtin_fmaf(sqrt_1m, ep[v], sqrt_ap * x0[v]);
      stv<VEC>(a.x_t + idx, xt);
      if (a.xt_bf16) stv_bf16<VEC>(a.xt_bf16 + ((size_t)b * a.S + s) * a.Cp + col0, xt);
    }
  }
}

// ------------------------------------------------------------------ the three sums of one example at one timestep
// d = x0 - clamp(sqrt_recip x_t - sqrt_m1 eps_hat, -clip, clip).  Inside the clamp the difference is NOT taken: with
// x_t = sqrt_ap x0 + sqrt_1m eps it is, term by term,
//   d = sqrt_m1 (eps_hat - eps) + (1 - sqrt_recip sqrt_ap) x0 + (sqrt_m1 - sqrt_recip sqrt_1m) eps
// where the two bracketed constants are 0 for exact tables and ~1e-7 for the float32 ones (one FMA each gives them to full
// relative precision), so d keeps its own 24 bits at t <= 1 where it is 1e-3 of x0.  Outside it is x0 -/+ clip; the two
// forms agree at the boundary.  The sums are combined in a fixed order (per thread, then row groups through LDS, then the two
// column waves): a sample's result depends on nothing but its own rows.
template <int VEC, int RG>
__global__ __launch_bounds__(128 * RG) void bound_terms_kernel(BoundTermsArgs a) {
  __shared__ float part[RG][3][128];
  const int t = *a.t_ptr;
  if (t < 0 || t >= a.T) return;          // a no-op that advances nothing
  const float4 row = *reinterpret_cast<const float4*>(a.table + (size_t)t * 4);
  const float sqrt_ap = row.x, sqrt_1m = row.y, sqrt_recip = row.z, sqrt_m1 = row.w;
  const float c_x0 = __builtin_fmaf(-sqrt_recip, sqrt_ap, 1.0f);
  const float c_eps = __builtin_fmaf(-sqrt_recip, sqrt_1m, sqrt_m1);
  const float clip = a.clip;
  const int b = blockIdx.x;
  const int ct = threadIdx.x & 127, rg = threadIdx.x >> 7;
  const size_t sample_base = (size_t)b * a.S * a.C;
  float acc_q[VEC], acc_e[VEC], acc_n[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc_q[v] = acc_e[v] = acc_n[v] = 0.f;
  for (int cb = 0; cb < a.C; cb += 128 * VEC) {
    const int col0 = cb + ct * VEC;
    if (col0 >= a.C) continue;
    for (int s = rg; s < a.S; s += RG) {
      const size_t idx = sample_base + (size_t)s * a.C + col0;
      float x0[VEC], ep[VEC], eh[VEC];
      ldv<VEC>(a.x0 + idx, x0);
      ldv<VEC>(a.eps + idx, ep);
      ldv<VEC>(a.eps_hat + idx, eh);
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const float xt = __builtin_fmaf(sqrt_1m, ep[v], sqrt_ap * x0[v]);          // the noise kernel's own x_t
        const float raw = __builtin_fmaf(sqrt_recip, xt, -sqrt_m1 * eh[v]);
        const float de = eh[v] - ep[v];
        float d = __builtin_fmaf(sqrt_m1, de, __builtin_fmaf(c_x0, x0[v], c_eps * ep[v]));
        if (raw > clip) d = x0[v] - clip;
        else if (raw < -clip) d = x0[v] + clip;
        acc_q[v] = __builtin_fmaf(d, d, acc_q[v]);
        acc_e[v] = __builtin_fmaf(de, de, acc_e[v]);
        acc_n[v] = __builtin_fmaf(x0[v], x0[v], acc_n[v]);
      }
    }
  }
  float sq = acc_q[0], se = acc_e[0], sn = acc_n[0];
#pragma unroll
  for (int v = 1; v < VEC; ++v) { sq += acc_q[v]; se += acc_e[v]; sn += acc_n[v]; }
  if constexpr (RG > 1) {
    part[rg][0][ct] = sq; part[rg][1][ct] = se; part[rg][2][ct] = sn;
    __syncthreads();
    if (rg == 0) {
      sq = part[0][0][ct]; se = part[0][1][ct]; sn = part[0][2][ct];
#pragma unroll
      for (int g2 = 1; g2 < RG; ++g2) { sq += part[g2][0][ct]; se += part[g2][1][ct]; sn += part[g2][2][ct]; }
    }
  }
  const float sum = column_waves_sum3(sq, se, sn);
  if (threadIdx.x < 3) a.partial[((size_t)t * a.B + b) * 3 + threadIdx.x] = sum;
  if (a.next_t && threadIdx.x == 0 && last_arriver(a.arrive))
    __hip_atomic_store(a.t_ptr, a.next_t[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

int launch_bound_noise(const BoundNoiseArgs& a, hipStream_t st) {
  SMD_ARG_CHECK(a.x0 && a.eps && a.x_t && a.table && a.t_ptr, "bound_noise: null pointer");
  SMD_ARG_CHECK(a.B > 0 && a.S > 0 && a.C > 0 && (!a.xt_bf16 || a.Cp >= a.C), "bound_noise: bad shape");
  SMD_ARG_CHECK(a.T > 0, "bound_noise: T=%d (number of timesteps: bounds the table)", a.T);
  SMD_ARG_CHECK(al16((uintptr_t)a.table), "bound_noise: the table rows are read as 16-byte vectors");
  const bool vec = a.C % 4 == 0 && (!a.xt_bf16 || a.Cp % 4 == 0);
  if (vec)
    SMD_ARG_CHECK(al16((uintptr_t)a.x0 | (uintptr_t)a.eps | (uintptr_t)a.x_t) && ((uintptr_t)a.xt_bf16 & 7) == 0,
                  "bound_noise: C=%d takes 16-byte loads: x0, eps, x_t must be 16-byte and the bf16 copy 8-byte aligned", a.C);
  SMD_LAUNCH_VEC_RG(bound_noise_kernel, vec, a, st);
  SMD_LAUNCH_CHECK();
  return 0;
}

int launch_bound_terms(const BoundTermsArgs& a, hipStream_t st) {
  SMD_ARG_CHECK(a.x0 && a.eps && a.eps_hat && a.table && a.t_ptr && a.partial, "bound_terms: null pointer");
  SMD_ARG_CHECK(a.B > 0 && a.S > 0 && a.C > 0, "bound_terms: bad shape");
  SMD_ARG_CHECK(a.T > 0, "bound_terms: T=%d (number of timesteps: bounds the tables and the rows of partial)", a.T);
  SMD_ARG_CHECK(a.clip > 0.0f, "bound_terms: clip=%g must be positive (inf: no clamp)", (double)a.clip);
  SMD_ARG_CHECK(!a.next_t || a.arrive, "bound_terms: next_t needs the arrival counter");
  SMD_ARG_CHECK(al16((uintptr_t)a.table), "bound_terms: the table rows are read as 16-byte vectors");
  const bool vec = a.C % 4 == 0;
  if (vec)
    SMD_ARG_CHECK(al16((uintptr_t)a.x0 | (uintptr_t)a.eps | (uintptr_t)a.eps_hat),
                  "bound_terms: C=%d takes 16-byte loads: x0, eps, eps_hat must be 16-byte aligned", a.C);
  SMD_LAUNCH_VEC_RG(bound_terms_kernel, vec, a, st);
  SMD_LAUNCH_CHECK();
  return 0;
}
