// Reference-precision (fp32 end to end) inference kernels: gemm_f32.hip and net_f32.hip.  Engine option "fp32".
#pragma once
#include "smd_common.h"

// ------------------------------------------------------------------ Dense on exact-fp32 MFMA (gemm_f32.hip)
// out[m][n] = act(sum_k A[m][k] W[k][n] + bias[n]) + res[m or m % res_row_mod][n]
// A fp32 [M][K] (row pitch lda), W fp32 [K][N] (row pitch ldw: the flax kernel layout of the master parameters, read in
// place), v_mfma_f32_32x32x2_f32: every product an fp32 multiply, accumulation in k order from 0 in steps of two.  The
// value of an output element depends on its row of A, its column of W and K only -- not on M, N or the tile form.
#define SMD_F32_ACT_NONE 0
#define SMD_F32_ACT_GELU 1
#define SMD_F32_ACT_SWISH 2
struct GemmF32Args {
  const float* A = nullptr; int lda = 0;
  const float* W = nullptr; int ldw = 0;
  const float* bias = nullptr;        // [N] or null
  const float* res = nullptr;         // fp32 residual added after the activation, or null (may alias out)
  int ld_res = 0;
  int res_row_mod = 0;                // > 0: residual row = m % res_row_mod (positional encoding)
  float* out = nullptr; int ld_out = 0;
  int M = 0, N = 0, K = 0;
  int act = SMD_F32_ACT_NONE;
};
int launch_gemm_f32(const GemmF32Args& a, hipStream_t st);

// ------------------------------------------------------------------ LayerNorm, attention, noise embedding (net_f32.hip)
// out = LN(x) * gamma + beta, then optionally swish(scale * out + shift) with the FiLM row of the sample (row /
// rows_per_sample) or of the table row *t_ptr; variance as E[x^2] - mean^2, eps 1e-6 (the reference's flax LayerNorm)
struct LnF32Args {
  const float* x = nullptr;
  int rows = 0, D = 0;
  const float* gamma = nullptr;
  const float* beta = nullptr;
  const float* film_scale = nullptr;
  const float* film_shift = nullptr;
  int ld_film = 0;
  int rows_per_sample = 1;
  const int* t_ptr = nullptr;
  int film_rows = 1 << 30;
  int swish = 0;
  float* out = nullptr;               // [rows][D]
};
int launch_layernorm_f32(const LnF32Args& a, hipStream_t st);
// qkv fp32 [B*32][3E] ([q|k|v], head h at columns h*d..), out fp32 [B*32][E]; S == 32, d = E / H in {8, 16, 32}
int launch_attention_f32(const float* qkv, float* out, int B, int S, int E, int H, hipStream_t st);
// NoiseEncoding (models/ncsn.py:28-41) with fp32 output
int launch_noise_embed_f32(const float* s, int n, int channels, float* out, int ld_out, hipStream_t st);
