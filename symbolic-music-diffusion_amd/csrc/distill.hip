// HBM-bound element-wise kernels of a progressive-distillation step (Salimans & Ho 2022): a student is
// trained so that ONE of its strided steps lands where TWO strided steps of a frozen teacher land.
//
//   distill_noise   z_t = alpha_t x0 + sigma_t eps at the sample's own level t
//   distill_mid     x1 = clamp(c0_t z_t - c1_t out1), z_m = a x1 + b z_t: the teacher's first step, t -> m
//   distill_loss    x2 = clamp(c0_m z_m - c1_m out2), x~ = w1 x1 + w2 x2, the student's target, loss and d loss / d pred,
//                   element by element in float64 registers
//
// The work split is that of the sampler steps (step_walk.h): one workgroup per sample, 128 column threads x RG row groups,
// VEC = 4 columns per thread when C % 4 == 0.  What is new against those kernels is a walk step PER SAMPLE: sample b reads row
// steps[b] of the [N][16] table (schedule.distill_tables).  A step outside [0, N) makes the sample a no-op that writes nothing;
// the branch is uniform in the workgroup, so the barriers of the loss reduction stay legal.
#include "step_walk.h"

namespace {

// the clamped x0 estimate of strided_step_kernel (diffusion.hip): the rounding of c1 * out is carried along, so the estimate is
// rounded once even where the two products cancel
__device__ __forceinline__ float x0_estimate(float c0, float c1, float clip, float z, float out) {
  const float p = c1 * out;
  const float perr = __builtin_fmaf(c1, out, -p);
  const float recon = __builtin_fmaf(c0, z, -p) - perr;
  return fminf(fmaxf(recon, -clip), clip);
}

template <int VEC, int RG>
__global__ __launch_bounds__(128 * RG) void distill_noise_kernel(DistillNoiseArgs a) {
  const int b = blockIdx.x;
  const int k = a.steps[b];
  if (k < 0 || k >= a.N) return;
  const float* row = a.table + (size_t)k * SMD_DISTILL_COLUMNS;
  const float alpha_t = row[5], sigma_t = row[6];
  const int ct = threadIdx.x & 127, rg = threadIdx.x >> 7;
  const uint32_t bglob = (uint32_t)b + a.sample_offset;
  const uint32_t step = a.step_ptr ? *a.step_ptr : a.step;
  const size_t sample_base = (size_t)b * a.S * a.C;
  for (int cb = 0; cb < a.C; cb += 128 * VEC) {
    const int col0 = cb + ct * VEC;
    if (col0 >= a.C) continue;
    for (int s = rg; s < a.S; s += RG) {
      const int e = s * a.C + col0;
      const size_t idx = sample_base + e;
      float x0[VEC], ep[VEC], zt[VEC];
      ldv<VEC>(a.x0 + idx, x0);
      if (a.draw) {
        philox_normals<VEC>(ep, e, bglob, SMD_STREAM_DISTILL, step, a.key.seed_lo, a.key.seed_hi);
        stv<VEC>(a.eps + idx, ep);
      } else {
        ldv<VEC>(a.eps + idx, ep);
      }
#pragma unroll
      for (int v = 0; v < VEC; ++v) zt[v] = __builtin_fmaf(alpha_t, x0[v], sigma_t * ep[v]);
      stv<VEC>(a.z_t + idx, zt);
    }
  }
  if (threadIdx.x == 0) a.level_out[b] = alpha_t;
}

template <int VEC, int RG>
__global__ __launch_bounds__(128 * RG) void distill_mid_kernel(DistillMidArgs a) {
  const int b = blockIdx.x;
  const int k = a.steps[b];
  if (k < 0 || k >= a.N) return;
  const float* row = a.table + (size_t)k * SMD_DISTILL_COLUMNS;
  const float c0 = row[0], c1 = row[1], ca = row[2], cb = row[3], clip = row[4], alpha_m = row[7];
  const int ct = threadIdx.x & 127, rg = threadIdx.x >> 7;
  const size_t sample_base = (size_t)b * a.S * a.C;
  for (int cb0 = 0; cb0 < a.C; cb0 += 128 * VEC) {
    const int col0 = cb0 + ct * VEC;
    if (col0 >= a.C) continue;
    for (int s = rg; s < a.S; s += RG) {
      const size_t idx = sample_base + (size_t)s * a.C + col0;
      float z[VEC], o[VEC], x1[VEC], zm[VEC];
      ldv<VEC>(a.z_t + idx, z);
      ldv<VEC>(a.out1 + idx, o);
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        x1[v] = x0_estimate(c0, c1, clip, z[v], o[v]);
        // b z_t as the strided step forms it at sigma = 0, fma(b, x, 0): the same bits, the sign of a zero included
        zm[v] = __builtin_fmaf(ca, x1[v], __builtin_fmaf(cb, z[v], 0.0f));
      }
      stv<VEC>(a.x1 + idx, x1);
      stv<VEC>(a.z_m + idx, zm);
    }
  }
  if (threadIdx.x == 0) a.level_out[b] = alpha_m;
}

// The target is formed in float64 registers from the fp32 inputs and rounded once.  The fp32 recipe (x~ = fmaf(w2, x2, w1 x1),
// eps: fmaf(-alpha_t, x~, z_t) / sigma_t) keeps the target within its own bound, but the eps and v targets are a cancelling
// difference divided by sigma_t, and d = pred - target then carries that error at the size of the TERMS, not of d: measured
// up to 9.2 x the bound 4 * 2^-24 * 2 w inv (|pred| + |target|) on dpred.  The kernel moves 24 bytes per
// element and has the float64 rate to spare.
// The squares are summed in a fixed order: per thread over its elements, the row groups through LDS, the two column waves.
// A sample's loss depends on its own rows only, and two calls agree bitwise; no atomics.
template <int VEC, int RG>
__global__ __launch_bounds__(128 * RG) void distill_loss_kernel(DistillLossArgs a) {
  __shared__ float part[RG][128];          // the row groups' partial sums; not touched when RG == 1 (512 bytes)
  const int b = blockIdx.x;
  const int k = a.steps[b];
  if (k < 0 || k >= a.N) return;
  const float* row = a.table + (size_t)k * SMD_DISTILL_COLUMNS;
  const double clip = row[4], alpha_t = row[5], c0 = row[8], c1 = row[9], w1 = row[10], w2 = row[11];
  const double inv_sigma_t = row[13];
  const double w = (double)(a.iw ? a.iw[b] : 1.0f) * (double)row[12];
  const double gscale = 2.0 * (double)a.inv_global_count * w;
  const int kind = a.kind;
  const int ct = threadIdx.x & 127, rg = threadIdx.x >> 7;
  const size_t sample_base = (size_t)b * a.S * a.C;
  float acc = 0.f;
  for (int cb0 = 0; cb0 < a.C; cb0 += 128 * VEC) {
    const int col0 = cb0 + ct * VEC;
    if (col0 >= a.C) continue;
    for (int s = rg; s < a.S; s += RG) {
      const size_t idx = sample_base + (size_t)s * a.C + col0;
      float x1[VEC], zm[VEC], o[VEC], zt[VEC], p[VEC], tg[VEC], g[VEC];
      ldv<VEC>(a.x1 + idx, x1);
      ldv<VEC>(a.z_m + idx, zm);
      ldv<VEC>(a.out2 + idx, o);
      ldv<VEC>(a.pred + idx, p);
      if (kind != 1) ldv<VEC>(a.z_t + idx, zt);
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const double x2 = fmin(fmax(c0 * (double)zm[v] - c1 * (double)o[v], -clip), clip);
        const double xs = w2 * x2 + w1 * (double)x1[v];               // convex: w1 + w2 = 1, both >= 0
        double t = xs;
        if (kind == 0) t = ((double)zt[v] - alpha_t * xs) * inv_sigma_t;
        else if (kind == 2) t = (alpha_t * (double)zt[v] - xs) * inv_sigma_t;
        const double dd = (double)p[v] - t;
        const float d = (float)dd;
        acc += d * d;
        tg[v] = (float)t;
        g[v] = (float)(dd * gscale);
      }
      stv<VEC>(a.dpred + idx, g);
      if (a.target_out) stv<VEC>(a.target_out + idx, tg);
    }
  }
  if constexpr (RG > 1) {
    part[rg][ct] = acc;
    __syncthreads();
    if (rg == 0) {
      acc = part[0][ct];
#pragma unroll
      for (int g2 = 1; g2 < RG; ++g2) acc += part[g2][ct];
    }
  }
  // column_waves_sum3 adds the values of waves 0 and 1 only, i.e. of threads 0 .. 127: exactly the rg == 0 threads, which hold
  // the combined sums (with RG == 1 they are the whole workgroup)
  const float sum = column_waves_sum3(acc, 0.f, 0.f);
  if (threadIdx.x == 0) {
    a.loss_per_sample[b] = sum / (float)(a.S * a.C);
    a.weight_per_sample[b] = (float)w;
  }
}

}  // namespace

#define SMD_DISTILL_SHAPE_CHECK(who, a)                                                                                   \
  SMD_ARG_CHECK((a).table && (a).steps, who ": null table or steps");                                                     \
  SMD_ARG_CHECK((a).B > 0 && (a).S > 0 && (a).C > 0, who ": bad shape");                                                  \
  SMD_ARG_CHECK((a).N > 0, who ": N=%d (number of student steps: bounds the table)", (a).N);                              \
  SMD_ARG_CHECK(al16((uintptr_t)(a).table), who ": the table rows are 64 bytes and must be 16-byte aligned")

int launch_distill_noise(const DistillNoiseArgs& a, hipStream_t st) {
  SMD_ARG_CHECK(a.x0 && a.eps && a.z_t && a.level_out, "distill_noise: null pointer");
  SMD_DISTILL_SHAPE_CHECK("distill_noise", a);
  const bool vec = a.C % 4 == 0;
  if (vec)
    SMD_ARG_CHECK(al16((uintptr_t)a.x0 | (uintptr_t)a.eps | (uintptr_t)a.z_t),
                  "distill_noise: C=%d takes 16-byte loads: x0, eps, z_t must be 16-byte aligned", a.C);
  SMD_LAUNCH_VEC_RG(distill_noise_kernel, vec, a, st);
  SMD_LAUNCH_CHECK();
  return 0;
}

int launch_distill_mid(const DistillMidArgs& a, hipStream_t st) {
  SMD_ARG_CHECK(a.z_t && a.out1 && a.x1 && a.z_m && a.level_out, "distill_mid: null pointer");
  SMD_DISTILL_SHAPE_CHECK("distill_mid", a);
  const bool vec = a.C % 4 == 0;
  if (vec)
    SMD_ARG_CHECK(al16((uintptr_t)a.z_t | (uintptr_t)a.out1 | (uintptr_t)a.x1 | (uintptr_t)a.z_m),
                  "distill_mid: C=%d takes 16-byte loads: z_t, out1, x1, z_m must be 16-byte aligned", a.C);
  SMD_LAUNCH_VEC_RG(distill_mid_kernel, vec, a, st);
  SMD_LAUNCH_CHECK();
  return 0;
}

int launch_distill_loss(const DistillLossArgs& a, hipStream_t st) {
  SMD_ARG_CHECK(a.kind >= 0 && a.kind <= 2, "distill_loss: kind=%d (0 eps, 1 x0, 2 v)", a.kind);
  SMD_ARG_CHECK(a.x1 && a.z_m && a.out2 && a.pred && a.loss_per_sample && a.weight_per_sample && a.dpred,
                "distill_loss: null pointer");
  SMD_ARG_CHECK(a.kind == 1 || a.z_t, "distill_loss: the eps and v targets need z_t");
  SMD_DISTILL_SHAPE_CHECK("distill_loss", a);
  const bool vec = a.C % 4 == 0;
  if (vec)
    SMD_ARG_CHECK(al16((uintptr_t)a.x1 | (uintptr_t)a.z_m | (uintptr_t)a.out2 | (uintptr_t)a.z_t | (uintptr_t)a.pred |
                       (uintptr_t)a.dpred | (uintptr_t)a.target_out),
                  "distill_loss: C=%d takes 16-byte loads: every [B][S][C] array must be 16-byte aligned", a.C);
  SMD_LAUNCH_VEC_RG(distill_loss_kernel, vec, a, st);
  SMD_LAUNCH_CHECK();
  return 0;
}
