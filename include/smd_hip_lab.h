/* smd_hip_lab.h -- laboratory hooks of libsmd_hip.so: kernel-selection knobs for A/B runs, debug views of the engine's saved
 * activations, hardware probes.  Used by tests/ and tools/ of this repository only; NOT part of the stable surface (smd_hip.h), no
 * reference callable stands behind any of these, and they may change without an ABI version bump. */
#ifndef SMD_HIP_LAB_H_
#define SMD_HIP_LAB_H_

#include "smd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Debugging aid (tools/det_first_diff.py): with a buffer of smd_engine_debug_snapshot_bytes() bytes set, the encoder backward
 * copies the shared per-layer gradient buffers (da2 partial tiles, dh, dA_E, dh) behind each of its kernels into it, so two
 * identical steps can be compared kernel by kernel; behind those 34 * rows * E bytes per encoder layer follow 2 K + 1 copies of
 * the output stage's shared dX buffer (bf16 [rows][mlp_dims]; behind out_proj's dgrad, then for block K-1 .. 0 behind the dgrad
 * of its second and its first Dense).  NULL switches it off (the default). */
int64_t smd_engine_debug_snapshot_bytes(const smd_engine* e);
int smd_engine_debug_snapshots(smd_engine* e, void* buf, int64_t bytes);

/* Debugging aid (layer-by-layer parity): device pointer, shape and element type (0 fp32, 1 bf16) of an activation the training
 * forward pass saved in the bound workspace: "x_bf16", "h"/"h_mid"/"a1"/"qkv"/"o"/"a2" [encoder layer], "h_last", "af",
 * "y" [0..K], "ya1"/"o1"/"ya2"/"f1"/"p"/"ss" [block], "emb", "ao", "pred", "s", "ln_stats" [0..2K: the saved (mean, rstd) rows of
 * ln1 / ln2 of block k at 2k / 2k + 1 and of the output norm at 2K]; and of the last backward pass the operands of
 * every weight-gradient GEMM: "dpred", "dyb" [0..K], "do1"/"dss"/"dss_bf16"/"dp"/"df1"/"zf1" [block], "dhb" [0..2L], "dqkv"/"dz1"/"u" [encoder
 * layer].  Valid until the next call on the handle. */
int smd_engine_debug_tensor(const smd_engine* e, const char* name, int index, const void** ptr, int64_t* rows, int64_t* cols,
                            int32_t* dtype);

/* process-wide kernel-selection knob for benchmark A/B runs (defaults = fast paths).
 * "gemm_nt256": 1 = large Dense GEMMs use the 256x256 8-phase kernel (default), 0 = 128-wide tiles only,
 *               2 = every shape with M,N % 256 == 0 and K % 128 == 0 (tests);
 * "gemm_nt256_variant": schedule variant of that kernel, 0 (default) .. 3, all computing the same result; the
 *               ablation variants used by tools/kbench.py exist only in a -DSMD_ABLATIONS build;
 * "ln_bwd_narrow": 1 (default) = the 128-wide LayerNorm backward runs on the 16-lanes-per-row kernel, 0 = one row per wave;
 * "tn_exclusive_cu": which 128-wide weight-gradient kernel the side stream runs and whether its workgroups own their CU:
 *               2 (default) = the four-buffer kernel (+ loader waves), unpadded: small-LDS workgroups of the main stream may
 *               share its CU (bitwise repeatable: 0 of 1499 repeated steps differ); 1 = the same kernels
 *               padded to the CU's whole LDS so that nothing shares their CU (the round-2 default, 2 % slower);
 *               0 = the two-buffer kernel, unpadded: NOT IN THE SHIPPED LIBRARY (the launch fails) -- with it on their CU the
 *               128-wide LayerNorm backward kernels intermittently compute a wrong row statistic (tools/rsq_repro.hip); it and
 *               the other experiment instantiations exist in a -DSMD_TN_EXPERIMENTS build only;
 * "tn_mode":    0 (default) = as "tn_exclusive_cu" says; NS*100 + NW*10 + pad picks buffers / issuing waves / pad (0 none,
 *               1 whole CU, 2 96 KiB) of that kernel explicitly; anything but 48x needs the experiment build;
 * "gemm_tn256": 1 = 2048-wide weight gradients use the 256x256 8-phase kernel (default), 0 = 128-wide tiles,
 *               2 = also on small grids (tests);
 * "tn_split_model": 1 = split-K of the 128-wide weight gradients chosen for whole rounds of 256 workgroups;
 * "tn128_loader_waves": 1 = the 128-wide weight-gradient kernel runs four extra waves that only issue LDS-DMA (0 needs the
 *               experiment build);
 * "gemm_nt_form": 0 (default) = the 128-column kernel picks its tile form from the shape; 1 .. 6 force <64,2>, <128,2>,
 *               <128,2,two K-groups>, <64,2,two K-groups>, <128,3>, <64,3,two K-groups> (tools/gemm_nt_forms_ab.py);
 *               "gemm_nt_form_wk": the same forms for the wide-K, few-column shapes only (N <= 512, K >= 2048: out_proj);
 * further keys ("ln_bwd_wide", "ln_fwd_wide", "ln_bwd_narrow", "gemm_nt_deep", "gemm_nt_kg", "mlp_variant", ...) select
 * between equivalent kernels for A/B runs; unknown keys return < 0. */
int smd_set_tuning(const char* key, int value);

/* lab probe: a HIP stream (returned as void*) created with hipExtStreamCreateWithCUMask(mask_words[0 .. n_words), one bit per CU).
 * Measured on MI355X / ROCm 7.2 (tools/cumask_probe.hip, profiles/r5a_cumask_probe.txt): mask bit i belongs to XCC i % 8; an XCC
 * whose share of the mask is EMPTY is not masked at all (a single set bit leaves 7 x 32 + 1 = 225 CUs), so a stream cannot be kept
 * off an XCD -- only a fraction of EVERY XCC's CUs can be selected (bits 0..127 = half of each).  Graph launches honour the launch
 * stream's mask like plain launches.  tools/chain_phase.py used it to show that halving every XCC between the two sampling chains
 * buys nothing; the product does not use it. */
int smd_probe_stream_create_cu_mask(const uint32_t* mask_words, int n_words, void** stream_out);
int smd_probe_stream_destroy(void* stream);
/* lab probe: `blocks` one-wave workgroups spin for ~spin_us; out[8 * b + ..] = XCC id, HW_ID, shader-clock ticks (2 words),
 * 100 MHz ticks (2 words), start time in 100 MHz ticks (2 words) -- where a stream runs and at which clock */
int smd_probe_clock(uint32_t* out, int blocks, int spin_us, void* stream);

/* lab probe: every XCD reads all `bytes` of `p`, leaving it resident in all eight L2s (sink: one writable dword or NULL) */
int smd_probe_l2_warm(const void* p, int64_t bytes, uint32_t* sink, void* stream);

/* lane-level probe of ds_read_b64_tr_b16 (debug): out[64][4] = values read from a 2 KiB linear image */
int smd_probe_tr_read(const smd_bf16* image_1024, smd_bf16* out_256, void* stream);

/* lab entry: the engine's own multi-problem weight-gradient launchers on a caller's problem list (tests/test_gpu_wgrad_groups.py).
 * Problem i: dW_i[Kd][N] (row stride ldo) = X_i[Mrows][0:Kd]^T dY_i[Mrows][0:N], db_i[N] = column sums of dY_i (bias_out may be NULL);
 * X / dY bf16 with ldx / ldy multiples of 8, every problem of a call with the same Mrows.
 * kind 0: SmdEngine::flush_grouped_wgrads' launcher -- the 128x128-tile kernel, at most 8 problems per kernel launch (a longer list
 *         takes several), one split-K factor per launch, slabs carved from the start of `slab`, one slab reduce; needs ldo == N;
 * kind 1: SmdEngine::flush_pending256's launcher -- 1..4 problems the 256x256-tile kernel accepts (Kd, N multiples of 256, at least
 *         8 K-tiles of 64 rows, ldo a multiple of 4, 16-byte aligned outputs; knob "gemm_tn256" 2 admits small grids) in one launch.
 * zero_page: 128 zeroed bf16; slab / slab_elems: the split-K workspace (smd_gemm_tn_slab_elems() floats in the engine; a smaller
 * one bounds the split factor of kind 0 and is an error where kind 1 cannot fit its partials).
 * plan_out (may be NULL): plan_cap int32; for the j-th GEMM kernel launched, plan_out[3 j ..] = tiles (kind 1: of all problems),
 * nsplit, ktiles_per_split -- the grid and kernel argument of that launch as the launcher passed them.  *launches_out (may be
 * NULL) = number of GEMM kernel launches, also past plan_cap / 3.
 * Argument errors (n < 1, n > 64, a null or misaligned operand, differing Mrows, ldo != N for kind 0, an ineligible problem or
 * n > 4 or too small a slab for kind 1) return < 0 with smd_last_error() set and launch nothing. */
typedef struct smd_wgrad_problem {
  const smd_bf16* X;
  const smd_bf16* dY;
  float* out;
  float* bias_out;
  int32_t ldx, ldy, ldo, Mrows, Kd, N;
} smd_wgrad_problem;
int smd_wgrad_lab_launch(const smd_wgrad_problem* probs, int n, int kind, const smd_bf16* zero_page, float* slab, int64_t slab_elems,
                         int32_t* plan_out, int plan_cap, int32_t* launches_out, void* stream);

/* lab entry: launch_gemm_nt, the launcher of every Dense forward and dgrad, with a full epilogue (tests/test_gpu_gemm_nt_epilogue.py).
 * C[M][N] = A[M][0:K] Bt[N][0:K]^T on bf16 operands (K a multiple of 64, lda / ldb multiples of 8 and >= K, A / Bt 16-byte aligned),
 * then, per element and in this order (GemmEpilogue, csrc/smd_kernels.h):
 *   v = alpha * acc + bias[col];  pre_bf16 <- v;  v = act(v) (0 none, 1 tanh-GELU, 2 swish);  v *= act'(aux[row][col]) (aux_mode 0
 *   none, 1 GELU', 2 swish');  v += res_f32[res_row_mod > 0 ? row % res_row_mod : row][col];  v += res_bf16[row][col];
 *   out_f32 (accumulate ? += : =) v;  out_bf16 <- v.
 * Every pointer of the epilogue may be NULL (at least one of pre_bf16 / out_f32 / out_bf16 is needed); out_f32 may be res_f32.
 * min_tiles: grid size from which an eligible shape goes to the 256 x 256 kernel (<= 0: the library's default).
 * plan_out (may be NULL): 8 int32 = the smd_plan::NtPlan the launcher ran with, handed out by the launcher itself: kernel (128 /
 * 256), BM, NS, KG, grid, block, pk_epilogue, vec_epilogue.
 * Argument errors (act / aux_mode outside 0..2, aux_mode without aux, a non-null epilogue tensor with ld < N, res_row_mod < 0, the
 * launcher's own lda / ldb / K / no-output rules) return < 0 with smd_last_error() set; nothing is launched, plan_out is untouched. */
typedef struct smd_gemm_epilogue {
  float alpha;
  int32_t act;
  const float* bias;
  smd_bf16* pre_bf16;
  const smd_bf16* aux;
  const float* res_f32;
  const smd_bf16* res_bf16;
  float* out_f32;
  smd_bf16* out_bf16;
  int32_t ld_pre, ld_aux, aux_mode, ld_res, res_row_mod, ld_resb, ld_out, accumulate, ld_outb;
} smd_gemm_epilogue;
int smd_gemm_nt_lab(const smd_bf16* A, int lda, const smd_bf16* Bt, int ldb, int M, int N, int K, const smd_gemm_epilogue* ep,
                    int min_tiles, int32_t* plan_out, void* stream);
/* lab entry: launch_gemm_nt256_fp8, the launcher of the e4m3 DenseResBlock layers and dgrads, with the same full epilogue
 * (tests/test_gpu_e4m3_regimes.py): smd_gemm_e4m3_nt (smd_hip.h) reaches bias / fp32 residual / fp32 and bf16 outputs only, the
 * engine also runs bf16 residual -> bf16 output.  Operands and shape rules are those of smd_gemm_e4m3_nt (M, N, K multiples of 256,
 * lda / ldb multiples of 16 and >= K); the epilogue checks are those of smd_gemm_nt_lab; alpha must be 1 and accumulate 0.  No
 * arithmetic of its own.  Errors return < 0 with smd_last_error() set and launch nothing. */
int smd_gemm_e4m3_nt_lab(const uint8_t* A8, int lda, const uint32_t* scale_a, const uint8_t* Bt8, int ldb, const uint32_t* scale_b,
                         int M, int N, int K, const smd_gemm_epilogue* ep, void* stream);

/* lab entry: launch_layernorm_fwd with the sampler's table-driven FiLM row (tests/test_gpu_ln_regimes.py).  It is
 * smd_layernorm_fwd_stats (smd_hip.h) plus the two LnArgs fields that only the engine's sampler steps set: with t_ptr != NULL every
 * row of the launch reads FiLM row clamp(*t_ptr, 0, film_rows - 1) of the [film_rows][ld_film] tables film_scale / film_shift (*t_ptr
 * is read on the device when the kernel runs), rows_per_sample is ignored by the forward and rows need not be a multiple of it.
 * With t_ptr == NULL it is smd_layernorm_fwd_stats.  No arithmetic of its own; the argument checks are the launcher's (t_ptr needs
 * a FiLM table and film_rows > 0), errors return < 0 with smd_last_error() set and launch nothing. */
int smd_layernorm_fwd_lab(const float* x, const smd_bf16* x_bf16, int rows, int D, const float* gamma, const float* beta,
                          const float* film_scale, const float* film_shift, int ld_film, int rows_per_sample, int swish,
                          smd_bf16* out, uint8_t* out8, uint32_t* out_scale, float* stats_out, const int32_t* t_ptr, int film_rows,
                          void* stream);

/* lab entries: the launchers of csrc/diffusion.hip with EVERY field of their argument structs (tests/test_gpu_diffusion_regimes.py).
 * The stable entries smd_ddpm_reverse_step / smd_q_sample / smd_mse_fwd_bwd fix some of them (no infill arrays, no bf16 re-cast, no
 * t_advance hand-off, no score-matching form); the engine sets all of them.  The structs mirror ReverseStepArgs / QSampleArgs
 * (csrc/smd_kernels.h) field for field; a field left 0 / NULL means what it means there.  No arithmetic of their own.
 * form_out (may be NULL) receives the instantiation the LAUNCHER chose, handed out by the launcher itself, written only behind a launch:
 *   smd_reverse_step_lab  form_out[0..1] = (VEC, RG) of reverse_step_kernel<VEC, RG>: VEC 4 iff C % 4 == 0 (and Cp % 4 == 0 with x_bf16),
 *                         RG 4 iff S >= 4;
 *   smd_q_sample_lab      form_out[0] = 0 q_sample_quads_kernel<4>, 1 q_sample_quads_kernel<1>, 2 q_sample_kernel<true> (S*C % 4 == 0),
 *                         3 q_sample_kernel<false> (the scalar tail);
 *   smd_loss_grad_lab     form_out[0] = VEC of mse_loss_grad_kernel<VEC> (4 iff C % 4 == 0 and Cp % 4 == 0).
 * The vector forms move 16 bytes per lane: the launchers refuse fp32 arrays that are not 16-byte aligned and a bf16 array that is
 * not 8-byte aligned.  On top of the launchers' own checks the lab entries refuse what the launchers trust the engine for: a
 * pointer that is not aligned to its element, infill draws without masks, threefry key tables with tf_t0 outside [0, T), Cp < C.
 * Errors return < 0 with smd_last_error() set; nothing is launched and form_out is untouched. */
typedef struct smd_reverse_step_args {
  float* x;
  const float* eps_hat;
  int32_t B, S, C, Cp, T;
  const float* coef;
  const int32_t* t_ptr;
  int32_t* t_advance;
  uint32_t* arrive;
  const float* z_in;
  uint32_t seed_lo, seed_hi;
  const uint32_t* key_ptr;
  uint32_t sample_offset;
  const float* infill_samples;
  const float* infill_masks;
  const float* infill_z_in;
  const uint32_t* tf_noise_keys;
  const uint32_t* tf_infill_keys;
  int64_t tf_n_total;
  int32_t tf_t0;
  smd_bf16* x_bf16;
  float* metrics_partial;
  float* collection;
  const int32_t* slot_table;
} smd_reverse_step_args;
int smd_reverse_step_lab(const smd_reverse_step_args* a, int32_t* form_out, void* stream);

typedef struct smd_q_sample_args {
  const float* x0;
  int32_t B, S, C, Cp, T;
  const float* alphas_prod_ext;
  const int32_t* labels;
  int32_t label_min;
  const float* alpha_in;
  int32_t dsm;
  const float* eps_in;
  uint32_t seed_lo, seed_hi;
  const uint32_t* step_ptr;
  uint32_t sample_offset;
  smd_bf16* xt_bf16;
  float* eps_out;
  float* s_out;
} smd_q_sample_args;
int smd_q_sample_lab(const smd_q_sample_args* a, int32_t* form_out, void* stream);

/* launch_mse_loss_grad; dsm_sigma [B] (may be NULL) selects the score-matching form: d = sigma pred + eps, loss = 0.5 sum d^2,
 * dpred = d sigma inv_global_count S C */
int smd_loss_grad_lab(const float* pred, const float* eps, int B, int S, int C, int Cp, float inv_global_count, float* loss_per_sample,
                      smd_bf16* dpred_bf16, const float* dsm_sigma, int32_t* form_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SMD_HIP_LAB_H_ */
