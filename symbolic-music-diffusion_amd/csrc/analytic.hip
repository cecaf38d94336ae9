// Kernels of the analytic (optimal) reverse variance of Bao et al. 2022 (Analytic-DPM).
//
//   score_moments   sums[t][s][c] = sum over the batch of eps_hat^2, eps_hat = A_t x_t + B_t out (the network's output in eps
//                   units for any prediction kind): the statistic g_t = E[eps_hat^2] the optimal variance needs
//   analytic_step   the strided (DDIM) step of diffusion.hip with a PER-ELEMENT noise scale sig[iteration][s][c]
//
// score_moments reduces ACROSS the batch, so the samplers' one-workgroup-per-sample split does not fit: the element axis goes
// over threads (VEC = 4 when C % 4 == 0) and the batch over the second grid dimension in chunks of SMD_MOMENT_CHUNK rows; a
// second, tiny launch adds the chunk partials in chunk order.  No float atomics anywhere: two calls give the same bits.
// analytic_step keeps the strided step's work split and its own row loop (section 16, "Shared helpers").
#include "step_walk.h"

namespace {

constexpr int MOM_THREADS = 128;

// ------------------------------------------------------------------ chunk partials of sum_b eps_hat^2
template <int VEC>
__global__ __launch_bounds__(MOM_THREADS) void score_moments_kernel(ScoreMomentsArgs a) {
  const int t = *a.t_ptr;
  if (t < 0 || t >= a.T) return;          // the walk's terminator (or a bad timestep): nothing is written
  const float4 row = *reinterpret_cast<const float4*>(a.table + (size_t)t * 4);
  const float cA = row.x, cB = row.y;
  const int N = a.S * a.C;
  const int n0 = (blockIdx.x * MOM_THREADS + threadIdx.x) * VEC;
  if (n0 >= N) return;                    // the masked tail of the last element block (N % VEC == 0 on the vector path)
  const int b0 = blockIdx.y * SMD_MOMENT_CHUNK;
  const int b1 = min(b0 + SMD_MOMENT_CHUNK, a.B);
  float acc[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
  for (int b = b0; b < b1; ++b) {
    const size_t idx = (size_t)b * N + n0;
    float x[VEC], o[VEC];
    ldv<VEC>(a.x_t + idx, x);
    ldv<VEC>(a.out + idx, o);
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const float eh = __builtin_fmaf(cA, x[v], cB * o[v]);      // (A, B) = (0, 1): out itself
      acc[v] = __builtin_fmaf(eh, eh, acc[v]);
    }
  }
  stv<VEC>(a.partial + (size_t)blockIdx.y * N + n0, acc);
}

// sums[t][n] = partial[0][n] + partial[1][n] + ... in chunk order; the launch's last workgroup stores the walk's next timestep
template <int VEC>
__global__ __launch_bounds__(MOM_THREADS) void score_moments_combine_kernel(ScoreMomentsArgs a) {
  const int t = *a.t_ptr;
  if (t < 0 || t >= a.T) return;          // a no-op that advances nothing
  const int N = a.S * a.C;
  const int n0 = (blockIdx.x * MOM_THREADS + threadIdx.x) * VEC;
  if (n0 < N) {
    const int chunks = (a.B + SMD_MOMENT_CHUNK - 1) / SMD_MOMENT_CHUNK;
    float acc[VEC];
    ldv<VEC>(a.partial + n0, acc);
    for (int j = 1; j < chunks; ++j) {
      float p[VEC];
      ldv<VEC>(a.partial + (size_t)j * N + n0, p);
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] += p[v];
    }
    stv<VEC>(a.sums + (size_t)t * N + n0, acc);
  }
  if (a.next_t && threadIdx.x == 0 && last_arriver(a.arrive))
    __hip_atomic_store(a.t_ptr, a.next_t[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------ strided step with a per-element noise scale
// strided_step_kernel (diffusion.hip) with sigma read per element: coef[t] = (sqrt_recip, sqrt_m1, a, b, on, clip, sqrt_as,
// sqrt_1m_as), plan[t] = (next_t, iteration, slot, 0), sig [n_iter][S][C]:
//   x0 = clamp(sqrt_recip x - sqrt_m1 eps_hat, -clip, clip);  x' = a x0 + b x + on * sig[iteration][s][c] * z
// on == 0: neither z nor sig is read, z is not drawn.  The arithmetic is the strided step's statement for statement -- z * sig
// is one rounding, as its z * sigma, a zero sig gives the +0 its sigma == 0 branch gives, and on = 1 multiplies exactly -- so a
// table filled with one sigma reproduces its bits.  An iteration outside [0, n_iter) is off the walk: a no-op.
template <int VEC, int RG>
__global__ __launch_bounds__(128 * RG) void analytic_step_kernel(AnalyticStepArgs a) {
  __shared__ float part[RG > 1 ? RG : 1][3][128 * VEC];
  const int b = blockIdx.x;
  const int ct = threadIdx.x & 127, rg = threadIdx.x >> 7;
  const int t = *a.t_ptr;
  if (t < 0 || t >= a.T) return;          // the walk's terminator (or a bad timestep): a no-op, t is not advanced either
  const int4 pl = *reinterpret_cast<const int4*>(a.plan + (size_t)t * 4);
  const int next_t = pl.x, iter = pl.y;
  if (iter < 0 || iter >= a.n_iter) return;
  const float* cf = a.coef + (size_t)t * 8;
  const float sqrt_recip = cf[0], sqrt_m1 = cf[1], ca = cf[2], cb = cf[3], on = cf[4], clip = cf[5];
  const float sqrt_as = cf[6], sqrt_1m_as = cf[7];
  const bool noisy = on != 0.0f;
  const bool next_live = next_t >= 0 && next_t < a.T;       // the state being produced is still a noisy level
  int slot = a.collection ? pl.z : -1;
  if (slot > 40) slot = -1;               // the collection has 41 rows; out-of-range scatters are dropped
  const uint32_t bglob = (uint32_t)b + a.sample_offset;
  const size_t sample_base = (size_t)b * a.S * a.C;
  const float* sig = a.sig + (size_t)iter * a.S * a.C;       // this iteration's [S][C] scales: the same rows for every sample
  const uint64_t tf_base = (uint64_t)bglob * a.S * a.C;       // this sample's first element in the global jax array
  const uint32_t key_lo = a.key_ptr ? a.key_ptr[0] : a.key.seed_lo, key_hi = a.key_ptr ? a.key_ptr[1] : a.key.seed_hi;
  TfKey tf_nk{0, 0}, tf_ik{0, 0};
  tf_nk = tf_key_row(a.tf_noise_keys, iter);
  tf_ik = tf_key_row(a.tf_infill_keys, iter);
  float m_eps = 0.f, m_step = 0.f, m_z = 0.f;
  for (int cb0 = 0; cb0 < a.C; cb0 += 128 * VEC) {          // uniform trip count: the LDS combine below has barriers
    const int col0 = cb0 + ct * VEC;
    const bool live = col0 < a.C;
    float acc_e[VEC], acc_s[VEC], acc_z[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc_e[v] = acc_s[v] = acc_z[v] = 0.f;
    for (int s = rg; live && s < a.S; s += RG) {
      const int e = s * a.C + col0;
      const size_t idx = sample_base + e;
      float x[VEC], eh[VEC], z[VEC], nx[VEC];
      ldv<VEC>(a.x + idx, x);
      ldv<VEC>(a.eps_hat + idx, eh);
      if (noisy) {
        float sg[VEC];
        ldv<VEC>(sig + e, sg);
        if (a.z_in) {
          ldv<VEC>(a.z_in + idx, z);
        } else if (a.tf_noise_keys) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) z[v] = jax_normal_from_bits(jax_bits_at(tf_nk, tf_base + e + v, (uint64_t)a.tf_n_total));
        } else {
          philox_normals<VEC>(z, e, bglob, SMD_STREAM_Z, (uint32_t)t, key_lo, key_hi);
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) z[v] = sg[v] != 0.0f ? on * (z[v] * sg[v]) : 0.f;
      } else {
#pragma unroll
        for (int v = 0; v < VEC; ++v) z[v] = 0.f;
      }
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        // x0 rounded once, as in strided_step_kernel: p + perr is sqrt_m1 * eps_hat exactly
        const float p = sqrt_m1 * eh[v];
        const float perr = __builtin_fmaf(sqrt_m1, eh[v], -p);
        float recon = __builtin_fmaf(sqrt_recip, x[v], -p) - perr;
        recon = fminf(fmaxf(recon, -clip), clip);                 // clip = inf: no clamp
        nx[v] = __builtin_fmaf(ca, recon, __builtin_fmaf(cb, x[v], z[v]));
      }
      if (a.infill_masks) {
        float im[VEC], is[VEC], iz[VEC];
        ldv<VEC>(a.infill_masks + idx, im);
        ldv<VEC>(a.infill_samples + idx, is);
        if (next_live) {
          if (a.infill_z_in) {
            ldv<VEC>(a.infill_z_in + idx, iz);
          } else if (a.tf_infill_keys) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) iz[v] = jax_normal_from_bits(jax_bits_at(tf_ik, tf_base + e + v, (uint64_t)a.tf_n_total));
          } else {
            philox_normals<VEC>(iz, e, bglob, SMD_STREAM_INFILL, (uint32_t)t, key_lo, key_hi);
          }
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          // the known region at the noise level of the state being PRODUCED (next_t), the clean samples at the end
          const float y = next_live ? __builtin_fmaf(sqrt_as, is[v], sqrt_1m_as * iz[v]) : is[v];
          nx[v] = nx[v] * (1.0f - im[v]) + y * im[v];
        }
      }
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const float st = x[v] - nx[v];
        acc_e[v] += eh[v] * eh[v];
        acc_s[v] += st * st;
        acc_z[v] += z[v] * z[v];
      }
      stv<VEC>(a.x + idx, nx);
      if (slot >= 0) stv<VEC>(a.collection + ((size_t)slot * a.B) * a.S * a.C + idx, nx);
      if (a.x_bf16) stv_bf16<VEC>(a.x_bf16 + ((size_t)b * a.S + s) * a.Cp + col0, nx);
    }
    if constexpr (RG > 1) {
      __syncthreads();
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        part[rg][0][ct * VEC + v] = acc_e[v]; part[rg][1][ct * VEC + v] = acc_s[v]; part[rg][2][ct * VEC + v] = acc_z[v];
      }
      __syncthreads();
      if (rg == 0) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          float se = 0.f, ss = 0.f, sz = 0.f;
#pragma unroll
          for (int g2 = 0; g2 < RG; ++g2) {
            se += part[g2][0][ct * VEC + v]; ss += part[g2][1][ct * VEC + v]; sz += part[g2][2][ct * VEC + v];
          }
          acc_e[v] = se; acc_s[v] = ss; acc_z[v] = sz;
        }
      }
    }
    // sqrt(sum(v^2, axis=1) + 1e-10) as in reverse_step_kernel: axis 1 is the sequence axis, the channel axis for S == 1
    if (rg == 0 && live)
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      if (a.S > 1) {
        m_eps += norm_of(acc_e[v]);
        m_step += norm_of(acc_s[v]);
        m_z += norm_of(acc_z[v]);
      } else {
        m_eps += acc_e[v]; m_step += acc_s[v]; m_z += acc_z[v];
      }
    }
  }
  if (a.metrics_partial) store_metrics(a.metrics_partial, t, a.B, b, a.S, m_eps, m_step, m_z);
  // *t_advance = plan[t].next_t by the LAST workgroup to get here, as in strided_step_kernel
  if (a.t_advance && threadIdx.x == 0) last_arriver_store(a.arrive, a.t_advance, next_t);
}

}  // namespace

int launch_score_moments(const ScoreMomentsArgs& a, hipStream_t st) {
  SMD_ARG_CHECK(a.x_t && a.out && a.table && a.t_ptr && a.partial && a.sums, "score_moments: null pointer");
  SMD_ARG_CHECK(a.B > 0 && a.S > 0 && a.C > 0 && (int64_t)a.S * a.C < (1ll << 30), "score_moments: bad shape");
  SMD_ARG_CHECK(a.T > 0, "score_moments: T=%d (number of timesteps: bounds the table and the rows of sums)", a.T);
  SMD_ARG_CHECK(!a.next_t || a.arrive, "score_moments: next_t needs the arrival counter");
  SMD_ARG_CHECK(al16((uintptr_t)a.table), "score_moments: the table rows are read as 16-byte vectors");
  const bool vec = a.C % 4 == 0;
  if (vec)
    SMD_ARG_CHECK(al16((uintptr_t)a.x_t | (uintptr_t)a.out | (uintptr_t)a.partial | (uintptr_t)a.sums),
                  "score_moments: C=%d takes 16-byte loads: x_t, out, partial and sums must be 16-byte aligned", a.C);
  const int N = a.S * a.C, per_block = MOM_THREADS * (vec ? 4 : 1);
  const unsigned blocks = (unsigned)((N + per_block - 1) / per_block);
  const unsigned chunks = (unsigned)((a.B + SMD_MOMENT_CHUNK - 1) / SMD_MOMENT_CHUNK);
  SMD_ARG_CHECK(chunks <= 65535u, "score_moments: B=%d is more than 65535 chunks of %d rows", a.B, SMD_MOMENT_CHUNK);
  if (vec) hipLaunchKernelGGL(score_moments_kernel<4>, dim3(blocks, chunks), dim3(MOM_THREADS), 0, st, a);
  else hipLaunchKernelGGL(score_moments_kernel<1>, dim3(blocks, chunks), dim3(MOM_THREADS), 0, st, a);
  SMD_LAUNCH_CHECK();
  if (vec) hipLaunchKernelGGL(score_moments_combine_kernel<4>, dim3(blocks), dim3(MOM_THREADS), 0, st, a);
  else hipLaunchKernelGGL(score_moments_combine_kernel<1>, dim3(blocks), dim3(MOM_THREADS), 0, st, a);
  SMD_LAUNCH_CHECK();
  return 0;
}

int launch_analytic_step(const AnalyticStepArgs& a, hipStream_t st) {
  const bool threefry = a.tf_infill_keys || a.tf_noise_keys;
  const uintptr_t f32 = (uintptr_t)a.x | (uintptr_t)a.eps_hat | (uintptr_t)a.infill_samples | (uintptr_t)a.infill_masks |
                        (uintptr_t)a.infill_z_in | (uintptr_t)a.collection | (uintptr_t)a.z_in | (uintptr_t)a.sig;
  SMD_ARG_CHECK(a.x && a.eps_hat && a.coef && a.plan && a.t_ptr && a.sig, "analytic_step: null pointer");
  SMD_ARG_CHECK(a.B > 0 && a.S > 0 && a.C > 0 && (!a.x_bf16 || a.Cp >= a.C), "analytic_step: bad shape");
  SMD_ARG_CHECK(a.n_iter > 0, "analytic_step: n_iter=%d (iterations of the walk: bounds the rows of sig)", a.n_iter);
  SMD_ARG_CHECK((a.infill_masks != nullptr) == (a.infill_samples != nullptr), "analytic_step: infill needs samples and masks");
  SMD_ARG_CHECK(a.T > 0, "analytic_step: T=%d (number of timesteps: bounds the coefficient table and the plan)", a.T);
  SMD_ARG_CHECK(!a.t_advance || a.arrive, "analytic_step: t_advance needs the arrival counter");
  SMD_ARG_CHECK(al16((uintptr_t)a.plan), "analytic_step: the plan rows are read as 16-byte vectors");
  SMD_ARG_CHECK(!threefry || (a.tf_n_total >= (int64_t)(a.sample_offset + a.B) * a.S * a.C && a.tf_n_total <= (1ll << 32)),
                "analytic_step: tf_n_total=%lld must cover this rank's window and be <= 2^32", (long long)a.tf_n_total);
  const bool vec = a.C % 4 == 0 && (!a.x_bf16 || a.Cp % 4 == 0);
  if (vec)
    SMD_ARG_CHECK(al16(f32) && ((uintptr_t)a.x_bf16 & 7) == 0,
                  "analytic_step: C=%d takes 16-byte loads: state, eps_hat, draws, sig, infill arrays and collection must be 16-byte aligned",
                  a.C);
  SMD_LAUNCH_VEC_RG(analytic_step_kernel, vec, a, st);
  SMD_LAUNCH_CHECK();
  return 0;
}
