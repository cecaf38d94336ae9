// The non-GEMM kernels of the reference-precision (fp32 end to end) forward pass, engine option "fp32":
//
//   layernorm_f32     flax.nn.LayerNorm (+ FiLM scale * ln + shift, + swish), fp32 in, fp32 out   models/shared.py:61-70
//   attention_f32     softmax((q / sqrt(d)) k^T) v for S = 32, d in {8, 16, 32}                   models/ncsn.py:161
//   noise_embed_f32   NoiseEncoding.apply with fp32 output                                        models/ncsn.py:28-41
//
// Together under 1 % of the pass's arithmetic: plain VALU code, one wave per LayerNorm row, one workgroup per sample in
// the attention.  Every reduction runs in a fixed order, so two calls give equal bits and a row's result does not depend
// on the batch it sits in.
#include "f32_kernels.h"
#include "../../include/smd_hip.h"

namespace {

// ------------------------------------------------------------------ LayerNorm
// One wave per row, 4 rows per workgroup.  Two passes over the row: sums, then normalise (the second read hits the cache).
template <bool VEC4>
__global__ __launch_bounds__(256) void layernorm_f32_kernel(LnF32Args a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.rows) return;
  const float* x = a.x + (size_t)row * a.D;
  float s = 0.0f, s2 = 0.0f;
  if (VEC4) {
    for (int c = 4 * lane; c < a.D; c += 256) {
      const f32x4_t v = *reinterpret_cast<const f32x4_t*>(x + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) { s += v[j]; s2 = fmaf(v[j], v[j], s2); }
    }
  } else {
    for (int c = lane; c < a.D; c += 64) { const float v = x[c]; s += v; s2 = fmaf(v, v, s2); }
  }
  s = wave_sum(s);
  s2 = wave_sum(s2);
  const float inv_d = 1.0f / (float)a.D;
  const float mean = s * inv_d;
  const float var = s2 * inv_d - mean * mean;
  const float rstd = 1.0f / sqrtf(fmaxf(var + 1e-6f, 1e-6f));      // the one-pass variance can round below 0 (smd_ln_rstd, smd_common.h)
  const float* fs = nullptr;
  const float* fh = nullptr;
  if (a.film_scale) {
    const int fr = a.t_ptr ? smd_clamp_t(*a.t_ptr, a.film_rows) : row / a.rows_per_sample;
    fs = a.film_scale + (size_t)fr * a.ld_film;
    fh = a.film_shift + (size_t)fr * a.ld_film;
  }
  float* out = a.out + (size_t)row * a.D;
  auto one = [&](float v, int c) {
    float y = (v - mean) * rstd * a.gamma[c] + a.beta[c];
    if (fs) y = fs[c] * y + fh[c];
    return a.swish ? y / (1.0f + expf(-y)) : y;
  };
  if (VEC4) {
    for (int c = 4 * lane; c < a.D; c += 256) {
      const f32x4_t v = *reinterpret_cast<const f32x4_t*>(x + c);
      f32x4_t o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = one(v[j], c + j);
      *reinterpret_cast<f32x4_t*>(out + c) = o;
    }
  } else {
    for (int c = lane; c < a.D; c += 64) out[c] = one(x[c], c);
  }
}

// ------------------------------------------------------------------ attention
// One workgroup per sample: q | k | v of its 32 rows in LDS (row pitch 3E + 1 floats: the 32 lanes of a head read 32
// different rows of q from 32 different banks; k and v rows are read by all lanes of a head at once -- a broadcast).
// Thread (h, i) owns query row i of head h: 32 logits, softmax with max subtraction, P v.
template <int HD>
__global__ __launch_bounds__(256) void attention_f32_kernel(const float* __restrict__ qkv, float* __restrict__ out, int E, int H) {
  extern __shared__ float sm[];
  const int E3 = 3 * E, pitch = E3 + 1;
  const int b = blockIdx.x, t = threadIdx.x;
  const float* src = qkv + (size_t)b * 32 * E3;
  for (int idx = t; idx < 32 * E3; idx += 256) {
    const int r = idx / E3, c = idx - r * E3;
    sm[r * pitch + c] = src[idx];
  }
  __syncthreads();
  const float inv = 1.0f / sqrtf((float)HD);
  for (int p = t; p < H * 32; p += 256) {
    const int h = p >> 5, i = p & 31;
    float q[HD];
#pragma unroll
    for (int c = 0; c < HD; ++c) q[c] = sm[i * pitch + h * HD + c] * inv;
    float l[32];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const float* k = sm + j * pitch + E + h * HD;
      float acc = 0.0f;
#pragma unroll
      for (int c = 0; c < HD; ++c) acc = fmaf(q[c], k[c], acc);
      l[j] = acc;
      mx = fmaxf(mx, acc);
    }
    float den = 0.0f;
#pragma unroll
    for (int j = 0; j < 32; ++j) { l[j] = expf(l[j] - mx); den += l[j]; }
    const float rden = 1.0f / den;
    float o[HD];
#pragma unroll
    for (int c = 0; c < HD; ++c) o[c] = 0.0f;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const float* v = sm + j * pitch + 2 * E + h * HD;
      const float pj = l[j] * rden;
#pragma unroll
      for (int c = 0; c < HD; ++c) o[c] = fmaf(pj, v[c], o[c]);
    }
    float* dst = out + ((size_t)b * 32 + i) * E + h * HD;
#pragma unroll
    for (int c = 0; c < HD; ++c) dst[c] = o[c];
  }
}

// ------------------------------------------------------------------ noise embedding
// arguments reach 5000 rad: sincosf (with its full range reduction), never the fast hardware sine
__global__ __launch_bounds__(256) void noise_embed_f32_kernel(const float* __restrict__ s, int n, int channels,
                                                              float* __restrict__ out, int ld_out) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int half = channels >> 1;
  if (idx >= n * half) return;
  const int r = idx / half, i = idx - r * half;
  const float f = expf((float)i * -(9.210340371976184f / (float)(half - 1)));
  const float arg = (5000.0f * s[r]) * f;
  float sn, cs;
  sincosf(arg, &sn, &cs);
  out[(size_t)r * ld_out + i] = sn;
  out[(size_t)r * ld_out + half + i] = cs;
  if ((channels & 1) && i == 0) out[(size_t)r * ld_out + channels - 1] = 0.0f;
}

}  // namespace

int launch_layernorm_f32(const LnF32Args& a, hipStream_t st) {
  SMD_ARG_CHECK(a.x && a.gamma && a.beta && a.out, "layernorm_f32: null pointer");
  SMD_ARG_CHECK(a.rows > 0 && a.D > 0, "layernorm_f32: rows=%d D=%d", a.rows, a.D);
  SMD_ARG_CHECK(!a.film_scale || (a.film_shift && a.ld_film >= a.D && a.rows_per_sample > 0 && a.film_rows > 0),
                "layernorm_f32: FiLM arguments (ld_film=%d D=%d rows_per_sample=%d)", a.ld_film, a.D, a.rows_per_sample);
  SMD_ARG_CHECK(!a.t_ptr || a.film_scale, "layernorm_f32: t_ptr without a FiLM table");
  const bool vec = a.D % 4 == 0 && ((reinterpret_cast<uintptr_t>(a.x) | reinterpret_cast<uintptr_t>(a.out)) & 15u) == 0;
  const dim3 grid((a.rows + 3) / 4);
  if (vec) hipLaunchKernelGGL(layernorm_f32_kernel<true>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(layernorm_f32_kernel<false>, grid, dim3(256), 0, st, a);
  SMD_LAUNCH_CHECK();
  return 0;
}

int launch_attention_f32(const float* qkv, float* out, int B, int S, int E, int H, hipStream_t st) {
  SMD_ARG_CHECK(qkv && out && B > 0, "attention_f32: bad arguments");
  SMD_ARG_CHECK(S == 32 && H > 0 && E % H == 0 && E <= 1024, "attention_f32: S=%d E=%d H=%d (S must be 32)", S, E, H);
  const int d = E / H;
  const size_t lds = (size_t)32 * (3 * E + 1) * sizeof(float);
  SMD_ARG_CHECK(lds <= 64 * 1024, "attention_f32: E=%d does not fit the LDS tile", E);
  if (d == 8) hipLaunchKernelGGL(attention_f32_kernel<8>, dim3(B), dim3(256), lds, st, qkv, out, E, H);
  else if (d == 16) hipLaunchKernelGGL(attention_f32_kernel<16>, dim3(B), dim3(256), lds, st, qkv, out, E, H);
  else if (d == 32) hipLaunchKernelGGL(attention_f32_kernel<32>, dim3(B), dim3(256), lds, st, qkv, out, E, H);
  else { smd_set_error("attention_f32: head dimension %d (8, 16 or 32)", d); return -1; }
  SMD_LAUNCH_CHECK();
  return 0;
}

int launch_noise_embed_f32(const float* s, int n, int channels, float* out, int ld_out, hipStream_t st) {
  SMD_ARG_CHECK(s && out && n > 0 && channels >= 4 && ld_out >= channels, "noise_embed_f32: bad arguments");
  const int total = n * (channels / 2);
  hipLaunchKernelGGL(noise_embed_f32_kernel, dim3((total + 255) / 256), dim3(256), 0, st, s, n, channels, out, ld_out);
  SMD_LAUNCH_CHECK();
  return 0;
}

extern "C" {
int smd_layernorm_f32(const float* x, int rows, int D, const float* gamma, const float* beta, const float* film_scale,
                      const float* film_shift, int ld_film, int rows_per_sample, const int32_t* t_ptr, int film_rows, int swish,
                      float* out, void* stream) {
  LnF32Args a;
  a.x = x; a.rows = rows; a.D = D; a.gamma = gamma; a.beta = beta; a.film_scale = film_scale; a.film_shift = film_shift;
  a.ld_film = ld_film; a.rows_per_sample = rows_per_sample > 0 ? rows_per_sample : 1; a.t_ptr = t_ptr;
  a.film_rows = film_rows > 0 ? film_rows : (1 << 30); a.swish = swish; a.out = out;
  return launch_layernorm_f32(a, reinterpret_cast<hipStream_t>(stream));
}
int smd_attention_f32(const float* qkv, float* out, int B, int S, int E, int H, void* stream) {
  return launch_attention_f32(qkv, out, B, S, E, H, reinterpret_cast<hipStream_t>(stream));
}
int smd_noise_embed_f32(const float* s, int n, int channels, float* out, int ld_out, void* stream) {
  return launch_noise_embed_f32(s, n, channels, out, ld_out, reinterpret_cast<hipStream_t>(stream));
}
}
