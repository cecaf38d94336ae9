// The loss-second-moment timestep resampler of Nichol & Dhariwal 2021 (no reference counterpart):
//
//   timestep_draw     labels ~ p by inverse-CDF lookup, importance weights 1 / (n p)
//   timestep_update   ten-deep ring of per-timestep losses -> p ~ sqrt(E[L_t^2]) mixed with uniform, and its inclusive cdf
//
// Both are deterministic and use no atomics: the draw is a pure function of (key, global sample index, step), the update is
// one workgroup that applies the batch in sample order and sums in a fixed order.
#include "smd_kernels.h"
#include "rng.h"

namespace {

constexpr int TS_THREADS = 1024;   // one workgroup; a power of two (timestep i's ring belongs to thread i % TS_THREADS)
constexpr int TS_CHUNK = 2048;     // samples staged in LDS per pass over the batch
constexpr int TS_DEPTH = 10;       // losses kept per timestep (the paper's history_per_term)

// ------------------------------------------------------------------ draw
__global__ __launch_bounds__(256) void timestep_draw_kernel(const float* __restrict__ cdf, const float* __restrict__ p, int n,
                                                            int label_base, int B, uint32_t seed_lo, uint32_t seed_hi,
                                                            uint32_t sample_offset, uint32_t step,
                                                            const uint32_t* __restrict__ step_ptr,
                                                            const float* __restrict__ u_in, int* __restrict__ labels_out,
                                                            float* __restrict__ iw_out) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  float u;
  if (u_in) {
    u = u_in[b];
  } else {
    // 24 bits in [0, 1): keyed by the GLOBAL sample index like every other stream (rng.h), so a shard draws the batch's labels
    const uint4 r = philox4x32_10(make_uint4(0u, (uint32_t)b + sample_offset, SMD_STREAM_TIMESTEP, step_ptr ? *step_ptr : step),
                                  seed_lo, seed_hi);
    u = (float)(r.x >> 8) * 5.9604644775390625e-8f;
  }
  // first i with cdf[i] > u; the search never leaves [0, n - 1], so a cdf that ends below 1 through rounding (or a NaN u)
  // lands on the last timestep
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cdf[mid] > u) hi = mid;
    else lo = mid + 1;
  }
  labels_out[b] = label_base + lo;
  iw_out[b] = (float)(1.0 / ((double)n * (double)p[lo]));      // one rounding: within half an ulp of 1 / (n p)
}

// ------------------------------------------------------------------ update
// Inclusive scan of one double per thread over the workgroup in a fixed order (wave scan by shuffles, then the wave totals
// added front to back); *total receives the sum of all of them.  Two barriers.
__device__ __forceinline__ double block_scan(double v, double* wsum, double* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double a = __shfl_up(v, o, 64);
    if (lane >= o) v += a;
  }
  __syncthreads();                                   // nobody still reads the wave totals of an earlier scan
  if (lane == 63) wsum[w] = v;
  __syncthreads();
  double pre = 0.0, tot = 0.0;
#pragma unroll
  for (int i = 0; i < TS_THREADS / 64; ++i) {
    const double x = wsum[i];
    if (i < w) pre += x;
    tot += x;
  }
  *total = tot;
  return pre + v;
}

__device__ __forceinline__ double ring_rms(const float* h) {
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < TS_DEPTH; ++j) s += (double)h[j] * (double)h[j];
  return sqrt(s / (double)TS_DEPTH);
}

__global__ __launch_bounds__(TS_THREADS) void timestep_update_kernel(const int* __restrict__ labels, const float* __restrict__ loss,
                                                                     int Bg, float* history, int* counts, int n, int label_base,
                                                                     float uniform_mix, float* __restrict__ p_out,
                                                                     float* __restrict__ cdf_out, int* __restrict__ warmed_out) {
  __shared__ int s_idx[TS_CHUNK];
  __shared__ float s_loss[TS_CHUNK];
  __shared__ double wsum[TS_THREADS / 64];
  __shared__ int s_cold;
  const int tid = threadIdx.x;
  if (tid == 0) s_cold = 0;
  // ---- the rings.  Every thread walks the whole batch in sample order and applies the samples of ITS timesteps: two samples of
  // one timestep are applied by one thread, in batch order, so the ring's content does not depend on scheduling.
  for (int c0 = 0; c0 < Bg; c0 += TS_CHUNK) {
    const int m = min(TS_CHUNK, Bg - c0);
    __syncthreads();                                 // the previous chunk has been walked by everyone
    for (int j = tid; j < m; j += TS_THREADS) {
      s_idx[j] = labels[c0 + j] - label_base;
      s_loss[j] = loss[c0 + j];
    }
    __syncthreads();
    for (int j = 0; j < m; ++j) {
      const int idx = s_idx[j];
      if ((idx & (TS_THREADS - 1)) != tid || idx < 0 || idx >= n) continue;      // labels outside the table are dropped
      float* h = history + (size_t)idx * TS_DEPTH;
      const int c = max(counts[idx], 0);
      if (c < TS_DEPTH) {                            // warm-up: fill the row front to back
        h[c] = s_loss[j];
        counts[idx] = c + 1;
      } else {                                       // full: shift left and append (the paper's code)
        for (int k = 0; k + 1 < TS_DEPTH; ++k) h[k] = h[k + 1];
        h[TS_DEPTH - 1] = s_loss[j];
      }
    }
  }
  __threadfence_block();
  __syncthreads();
  // ---- the tables.  Thread t now owns the CONTIGUOUS timesteps [t per, (t + 1) per): sums run front to back inside a thread
  // and through block_scan across threads, in double -- the terms are fp32 values, so every p is the float64 result rounded once.
  const int per = (n + TS_THREADS - 1) / TS_THREADS;
  const int i0 = min(tid * per, n), i1 = min(i0 + per, n);
  bool cold = false;
  double seg = 0.0;
  for (int i = i0; i < i1; ++i) {
    cold |= counts[i] < TS_DEPTH;
    seg += ring_rms(history + (size_t)i * TS_DEPTH);
  }
  if (cold) s_cold = 1;                              // (every writer stores the same value)
  double total;
  block_scan(seg, wsum, &total);                     // its barriers also publish s_cold
  const bool warmed = s_cold == 0;
  const bool uniform = !warmed || !(total > 0.0) || !(total < __builtin_inf());
  const double mix = (double)uniform_mix, inv_n = 1.0 / (double)n;
  seg = 0.0;
  for (int i = i0; i < i1; ++i) {
    const double q = uniform ? inv_n : ring_rms(history + (size_t)i * TS_DEPTH) / total * (1.0 - mix) + mix * inv_n;
    const float pf = (float)q;
    p_out[i] = pf;
    seg += (double)pf;
  }
  // cdf: prefix sums of the ROUNDED p in double, rounded once.  Rounding is monotone and every p is >= uniform_mix / n, far
  // above the 2^-52 relative error of the sums, so the cdf is non-decreasing and ends within 2^-24 of sum(p).
  double run = block_scan(seg, wsum, &total) - seg;
  for (int i = i0; i < i1; ++i) {
    run += (double)p_out[i];
    cdf_out[i] = (float)run;
  }
  if (tid == 0) *warmed_out = warmed ? 1 : 0;
}

}  // namespace

int launch_timestep_draw(const float* cdf, const float* p, int n, int label_base, int B, uint32_t seed_lo, uint32_t seed_hi,
                         uint32_t sample_offset, uint32_t step, const uint32_t* step_ptr, const float* u_in, int* labels_out,
                         float* iw_out, hipStream_t st) {
  SMD_ARG_CHECK(cdf && p && labels_out && iw_out && n > 0 && B > 0, "timestep_draw: bad arguments");
  hipLaunchKernelGGL(timestep_draw_kernel, dim3((B + 255) / 256), dim3(256), 0, st, cdf, p, n, label_base, B, seed_lo, seed_hi,
                     sample_offset, step, step_ptr, u_in, labels_out, iw_out);
  SMD_LAUNCH_CHECK();
  return 0;
}

int launch_timestep_update(const int* labels, const float* loss, int Bg, float* history, int* counts, int n, int label_base,
                           float uniform_mix, float* p_out, float* cdf_out, int* warmed_out, hipStream_t st) {
  SMD_ARG_CHECK(labels && loss && history && counts && p_out && cdf_out && warmed_out && Bg > 0 && n > 0,
                "timestep_update: bad arguments");
  SMD_ARG_CHECK(uniform_mix >= 0.0f && uniform_mix <= 1.0f, "timestep_update: uniform_mix=%g outside [0, 1]", (double)uniform_mix);
  hipLaunchKernelGGL(timestep_update_kernel, dim3(1), dim3(TS_THREADS), 0, st, labels, loss, Bg, history, counts, n, label_base,
                     uniform_mix, p_out, cdf_out, warmed_out);
  SMD_LAUNCH_CHECK();
  return 0;
}
