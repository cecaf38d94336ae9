/* smd_hip.h -- C-ABI of libsmd_hip.so, the MI355X (gfx950) DDPM train + sample engine.
 *
 * The reference (magenta/symbolic-music-diffusion) has no FFI: its seam for this path is a set
 * of Python callables.  Each entry point below names the reference callable
 * (file:line under the reference repo root) whose arithmetic it replaces; INTEGRATION.md shows the
 * ctypes stub a maintainer would add on the reference side.
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch / C++ types.  All `void*`/`float*` data pointers are
 *     DEVICE pointers borrowed from the caller (never freed, never retained past the handle's
 *     bindings).  `stream` is a hipStream_t passed as void*.  Calls only enqueue work.
 *   - return value: 0 ok; < 0 argument / state error; > 0 a hipError_t.  smd_last_error() returns
 *     a thread-local message for the last non-zero return.
 *   - bf16 buffers are uint16 storage (`smd_bf16`).  GEMM operands are row-major with the
 *     contraction dimension padded to a multiple of 64 (zero filled).
 *   - entry points are re-entrant and stream-ordered.  The only process-wide mutable state is a thread-local error string
 *     (and the kernel-selection table behind smd_set_tuning() of smd_hip_lab.h: benchmark A/B knobs, the defaults are the
 *     shipped paths); everything else lives in the caller's buffers or in an smd_engine handle.
 *   - THIS header is the stable surface a maintainer binds.  What the repository's own laboratory uses --
 *     tuning knobs, debug views of saved activations, hardware probes -- is declared in smd_hip_lab.h and may change freely.
 */
#ifndef SMD_HIP_H_
#define SMD_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMD_ABI_VERSION 8   /* 8: engine option "fp32" (reference-precision inference), smd_gemm_f32, smd_layernorm_f32, smd_attention_f32, smd_noise_embed_f32; 7: smd_pair_kernel_sums, smd_moments (the evaluation distances of utils/metrics.py); 6: smd_attn_block_bwd_ln (the attention backward with both LayerNorm backwards in the launch), "fused_attn_bwd" 2; 2: smd_ddpm_reverse_step takes T; hidden-split MLP, fp8, loss-side and Langevin entries; 3: smd_langevin_io table mode, debug snapshots; 4: one-sweep optimiser, "opt_overlap", smd_engine_join_update; 5: smd_build_id, smd_engine_sample_step_part, smd_engine_forward_train / backward_from; the lab hooks (tuning knobs, debug tensors, probes) moved to smd_hip_lab.h -- this header is the stable surface */

typedef uint16_t smd_bf16;
typedef struct smd_engine smd_engine;

const char* smd_last_error(void);
int smd_abi_version(void);
/* 16 hex digits: a hash of the sources, headers and compiler flags this binary was built from (build.py source_id()).  The
 * host refuses to run a library whose id differs from its tree's (a stale .so next to edited sources). */
const char* smd_build_id(void);

/* ---- model description: the kwargs of train_ncsn.py:321-326 + data shape ---------------------- */
typedef struct smd_model_desc {
  int32_t arch;            /* 0 TransformerDDPM (models/ncsn.py:138-179), 1 DenseDDPM (:122-135) */
  int32_t data_channels;   /* C */
  int32_t seq_len;         /* S (32; 1 for DenseDDPM) */
  int32_t num_layers;      /* --num_layers       train_ncsn.py:69 */
  int32_t num_heads;       /* --num_heads        train_ncsn.py:70 */
  int32_t num_mlp_layers;  /* --num_mlp_layers   train_ncsn.py:71 */
  int32_t mlp_dims;        /* --mlp_dims         train_ncsn.py:72 */
  int32_t embed_channels;  /* 128, models/ncsn.py:151 */
  int32_t film_channels;   /* 128, models/ncsn.py:174 */
  int32_t num_timesteps;   /* --num_sigmas       train_ncsn.py:81 */
} smd_model_desc;

/* ---- engine handle ---------------------------------------------------------------------------- */
/* replaces train_ncsn.create_model (train_ncsn.py:193-203): builds the parameter layout only */
int smd_engine_create(const smd_model_desc* desc, smd_engine** out);
void smd_engine_destroy(smd_engine* e);

/* parameter pytree as a flat fp32 buffer: tensor i = (name, element offset, rows, cols[0 = 1-D]) */
int smd_engine_num_tensors(const smd_engine* e);
int smd_engine_tensor_info(const smd_engine* e, int i, const char** name, int64_t* offset, int32_t* rows,
                           int32_t* cols);
int64_t smd_engine_param_count(const smd_engine* e);
int64_t smd_engine_head_param_offset(const smd_engine* e);  /* first parameter of the output stage */
int64_t smd_engine_wpack_elems(const smd_engine* e);        /* bf16 elements of the GEMM operand pack */
int64_t smd_engine_workspace_bytes(const smd_engine* e, int batch, int training);
int64_t smd_engine_film_table_floats(const smd_engine* e);
int smd_engine_padded_channels(const smd_engine* e);
/* Per-handle options (set before the first bind unless noted; unknown keys return < 0).  Defaults are the shipped paths:
 *   "tr_path" 1          weight gradients with transposing LDS reads (0: explicit-transpose fallback)
 *   "side_wgrad" 0/1     weight-gradient GEMMs (and the gradient memset, FiLM chains) on the engine's low-priority side
 *                        stream, joined inside smd_engine_loss_backward; the Python host turns it on for training handles
 *   "group_wgrad" 2, "pair_wgrad" 1, "film_side" 1, "film_side_fwd" 1, "tail_on_main" 1   launch grouping of those GEMMs
 *   "fused_encoder" 1, "fused_attn_bwd" 2 (2: + both LayerNorm backwards in the launch, 1: attention only), "mlp_hs" 1   fused encoder half-layers / hidden-split MLP (0: separate launches)
 *   "resgrad_bf16" 1     DenseResBlock residual-gradient chain in bf16
 *   "trunk_bf16" 2       2048-wide residual stream in bf16 (2: inference + training, 1: inference only, 0: fp32)
 *   "fp8" 0/1            e4m3 DenseResBlock forward GEMMs (BASELINE config 5); "w8_dirty" 1: operand pack changed elsewhere
 *   "fp32" 0/1           reference precision, INFERENCE ONLY: every activation fp32, every Dense on the exact-fp32 MFMA reading
 *                        the fp32 master parameters in place (no operand pack, no bf16 state copy is read; "trunk_bf16" is
 *                        ignored).  Set before bind_workspace (the workspace grows).  Mutually exclusive with "fp8": setting
 *                        one while the other is on is an argument error.  smd_engine_forward, _forward_level,
 *                        _prepare_sampler and _sample_step work; smd_engine_sample_step_part with part 1 / 2 (the two-chain
 *                        pipeline) is an argument error, and so are a training workspace, smd_engine_bind_train,
 *                        _forward_train, _loss_backward, _backward_from and _optimizer_step ("fp32 is an inference precision
 *                        in this engine"): train in bf16, audit or publish samples in fp32 from the same parameter buffer.
 *   "label_min" 1/0      Philox labels in [1, T] (continuous_noise) or [0, T);  "loss_kind" 0/1  DDPM / score matching
 *   "prediction" 0       what the network's output means to smd_engine_loss_backward (any time; DDPM objective only: an
 *                        argument error together with "loss_kind" 1, and for values outside 0..2): 0 eps (the reference), 1 x0,
 *                        2 v = s eps - sqrt(1 - s^2) x0 (Salimans & Ho 2022).  See smd_engine_set_loss_weights for the targets
 *                        and weights.  Samplers and the bound take the kind through their coefficient tables, not from here.
 *   "grad_memset" 2      0 never / 1 always / 2 only with the tr_path = 0 fallback: zero the gradient buffer before a step
 *                        (every gradient element is written, not accumulated, by the default kernels)
 *   "nt256_min_tiles" 0  > 0: Dense layers take the 256x256 GEMM from this many output tiles up (default rule: 192)
 *   "fp8_dgrad" 1        fp8 mode, training: the DenseResBlock dgrad GEMMs on e4m3 operands too
 *   "dp_layer_events" 0  1: per-encoder-layer gradient-complete events in the stem backward (smd_engine_wait_grad_bucket)
 *   "opt_overlap" 0      smd_engine_optimizer_step placement (any time).  Bit 0: the update of the output-stage slice (parameters
 *                        >= smd_engine_head_param_offset, 86 % of the bytes) runs on the side stream and is NOT complete in
 *                        stream order when the call returns: the next smd_engine_loss_backward of the same handle waits for it
 *                        right before its first output-stage kernel; any other reader of params / m / v / ema / wpack (another
 *                        handle on the same buffers, a host copy) calls smd_engine_join_update(handle, its stream) first.
 *                        Bit 1: smd_engine_loss_backward(stage 0) reduces that slice's gradient-norm partials on the side
 *                        stream under the encoder backward; the caller must not change the gradient before the optimiser step
 *                        (leave it off around an all-reduce).  Opt-in (the Python host leaves 0 unless SMD_OPT_OVERLAP is set): +1 % at best on a
 *                        process's first training handle, and bit 0 halved the step rate of later handles of the same process
 *                        (DESIGN.md section 6). */
int smd_engine_set_option(smd_engine* e, const char* key, int value);

int smd_engine_bind_params(smd_engine* e, float* params, smd_bf16* wpack);
int smd_engine_bind_train(smd_engine* e, float* grads, float* adam_m, float* adam_v, float* ema /*nullable*/,
                          uint32_t* step_counter, float* metrics /*[4]: |g|, |g| clipped, lr, step*/);
int smd_engine_bind_workspace(smd_engine* e, void* workspace, int64_t bytes, int batch, int training,
                              void* stream);
/* coef [T][8] = (sqrt(1/ap), sqrt(1-ap)/sqrt(ap), mu1, mu2, sigma, ap, sqrt(ap), sqrt(1-ap)) per t
 * (utils/ebm_utils.py:332-358); sqrt_ap [T]; alphas_prod_ext [T+1] = [1, cumprod(1-beta)]
 * (utils/losses.py:277-281); film_tables: smd_engine_film_table_floats() floats or NULL.  smd_engine_prepare_sampler writes
 * the first blocks * T * 2 * mlp_dims of them (one [T][2 * mlp_dims] scale | shift table per DenseResBlock, every element); the
 * rest (T * 9 * film_channels bf16, fp32 with option "fp32", + 64 floats of slack) is scratch of the three generator GEMMs and
 * holds no defined values afterwards */
int smd_engine_bind_schedule(smd_engine* e, const float* coef, const float* sqrt_ap,
                             const float* alphas_prod_ext, float* film_tables);
int smd_engine_refresh_weights(smd_engine* e, void* stream);   /* fp32 master -> bf16 operand pack */

/* nn.Model.__call__: model(x:(B,S,C), noise_level:(B,)) -> eps_hat (models/ncsn.py:141-179, 125-135) */
int smd_engine_forward(smd_engine* e, const float* x, const float* noise_level, float* eps_out, void* stream);
/* model(x, level) for a BATCH-UNIFORM noise level given as a device-side row index into the FiLM tables built by
 * smd_engine_prepare_sampler (row r = noise level sqrt_ap[r] of the bound schedule): no FiLM-generator launches and nothing
 * step-dependent on the host, so an (eps-net forward + Langevin update) pair can be captured once and replayed
 * (utils/ebm_utils.py:140,242 -- the noise level is the same for the whole batch inside both Langevin samplers).  out may be
 * NULL: the result then stays in the engine's own buffer, smd_engine_pred(). */
int smd_engine_forward_level(smd_engine* e, const float* x, const int32_t* level_ptr, float* out, void* stream);

/* diffusion_loss + value_and_grad (utils/losses.py:250-308, train_ncsn.py:282-283).
 * labels/eps_in NULL -> on-device Philox draws keyed by (seed, global sample index, step).
 * inv_global_count = 1 / (global_batch * S * C).  stage 0 = everything, 1 = forward + output-stage
 * backward (gradients of parameters >= head offset are final), 2 = remaining backward. */
int smd_engine_loss_backward(smd_engine* e, const float* x0, const int32_t* labels, const float* eps_in,
                             uint32_t seed_lo, uint32_t seed_hi, uint32_t sample_offset,
                             float inv_global_count, int stage, void* stream);
/* jax.value_and_grad over an ARBITRARY objective (train_ncsn.py:279-283, `objective` is any callable of the model's output):
 * smd_engine_forward_train = model(x, noise_level) in the bound TRAINING workspace, every activation the backward needs saved
 * (eps_out [B][S][C] fp32, nullable: smd_engine_pred); smd_engine_backward_from = the backward pass of that forward from
 * dpred = d objective / d eps_hat ([B][S][C] fp32), parameter gradients WRITTEN to the bound gradient buffer.  stage as in
 * smd_engine_loss_backward (0 everything, 1 output stage, 2 the rest; dpred is read by stages 0 and 1).  The host binds the pair
 * to torch autograd (ops.py smd_amd::eps_forward_train), so train_step accepts objectives other than the two fused ones. */
int smd_engine_forward_train(smd_engine* e, const float* x, const float* noise_level, float* eps_out, void* stream);
int smd_engine_backward_from(smd_engine* e, const float* dpred, int stage, void* stream);
/* continuous_noise=False (utils/losses.py:272-286; option "label_min" = 0): labels are drawn in [0, T) and label 0 takes
 * a real uniform used_alpha in [alphas_prod[T], 1).  used_alphas ([B] device floats, or NULL) replaces the label -> alpha
 * lookup of the following smd_engine_loss_backward calls (parity mode: the reference's own jax.random.uniform draws). */
int smd_engine_set_used_alphas(smd_engine* e, const float* used_alphas);
/* Per-sample loss weights of the following smd_engine_loss_backward calls (DDPM objective only; no reference counterpart:
 * min-SNR-gamma weighting of Hang et al. 2023 and the importance weights of a non-uniform timestep draw).  With ap = the
 * squared noise level q-sample stored, w_b = iw_b min(1, min_snr_gamma (1 - ap) / ap) -- for eps-prediction min(SNR, gamma) / SNR
 * -- and the gradient of the step is that of mean_b(w_b loss_b); smd_engine_loss_per_sample stays the UNWEIGHTED loss and
 * smd_engine_weight_per_sample returns the w_b ([B] device floats, valid after a weighted call).  iw: [B] device floats or NULL
 * (= 1); min_snr_gamma <= 0 or +inf: no SNR factor.  (NULL, 0), the state of a new handle, runs the unweighted kernel.
 * With option "prediction" (s = the stored noise level, ap = s^2, sb = sqrt((1 - s)(1 + s)),
 * SNR = ap / (1 - ap)) the loss compares the network's output `out` with another target and the SNR factor changes with it:
 *   kind      target            x0 from out: c0 x_t - c1 out             SNR factor of w_b
 *   0 eps     eps               c0 = sqrt(1/ap), c1 = sqrt(1/ap - 1)     min(1, gamma / SNR)
 *   1 x0      x0                c0 = 0,          c1 = -1                 min(SNR, gamma)             ap = 1: gamma, ap = 0: 0
 *   2 v       s eps - sb x0     c0 = sqrt(ap),   c1 = sqrt(1 - ap)       min(SNR, gamma) / (SNR + 1) ap = 1: 0,     ap = 0: 0
 * (the v factor is evaluated as min(ap, gamma (1 - ap)): finite everywhere).  Kinds 1 and 2 always run the weighted form: with
 * (NULL, 0) every w_b is exactly 1 and smd_engine_weight_per_sample is valid all the same.  smd_engine_loss_per_sample is the
 * unweighted mean of (out - target)^2, in the output space of the kind; stage 3 (loss only) reports the same. */
int smd_engine_set_loss_weights(smd_engine* e, const float* iw, float min_snr_gamma);
const float* smd_engine_weight_per_sample(const smd_engine* e); /* [B] device pointer */
/* [B] device pointer: the noise level s_b = sqrt(used alpha) q-sample stored in the last smd_engine_loss_backward (what the
 * weights above are evaluated on; the host turns an x0 / v loss into eps units with it) */
const float* smd_engine_noise_level_per_sample(const smd_engine* e);
const float* smd_engine_loss_per_sample(const smd_engine* e);   /* [B] device pointer */
const float* smd_engine_pred(const smd_engine* e);              /* [B*S][C] device pointer */

/* clip_grads + Adam + stepped LR + EMA + bf16 re-cast (train_ncsn.py:284-287,340-342,364-365) */
typedef struct smd_train_hyper {
  float lr0, lr_gamma;
  int32_t lr_interval;
  float beta1, beta2, eps, grad_clip, mu;
  float grad_scale;        /* multiplies the gradients first (1/world_size after a SUM all-reduce) */
} smd_train_hyper;
int smd_engine_optimizer_step(smd_engine* e, const smd_train_hyper* h, void* stream);
/* Data-parallel gradient buckets of the stem slice [0, head offset) in BACKWARD order: bucket b = encoder layer L-1-b (the last
 * bucket also holds in_proj).  With option "dp_layer_events" = 1, smd_engine_loss_backward (stage 2 or 0) records an event per
 * bucket as soon as its gradients are final; smd_engine_wait_grad_bucket makes `stream` (the communication stream) wait for it,
 * so the collective of layer l starts while the layers below are still in their backward pass.  The last bucket is final when
 * the call returns (in the caller's stream order).  (The reference has no counterpart: jax.pmap's pmean at train_ncsn.py:282.) */
int smd_engine_num_grad_buckets(const smd_engine* e);
int smd_engine_grad_bucket(const smd_engine* e, int bucket, int64_t* offset, int64_t* length);
int smd_engine_wait_grad_bucket(smd_engine* e, int bucket, void* stream);
/* Makes `stream` wait for an output-stage update deferred by "opt_overlap" bit 0 (no-op when none is pending). */
int smd_engine_join_update(smd_engine* e, void* stream);

/* diffusion_dynamics (utils/ebm_utils.py:280-405), one sample_with_beta iteration per call */
typedef struct smd_sample_io {
  float* x;                        /* [B][S][C] state, in place */
  int32_t* t_ptr;                  /* device timestep; decremented by the call */
  const float* z_in;               /* explicit N(0,1) draw or NULL (Philox) */
  uint32_t seed_lo, seed_hi, sample_offset;
  const float* infill_samples;     /* NULL unless infilling */
  const float* infill_masks;
  const float* infill_z_in;
  float* metrics_partial;          /* [T][B][3] or NULL */
  float* collection;               /* [41][B][S][C] or NULL */
  const int32_t* slot_table;       /* [T] collection slot for timestep t, -1 = none */
  /* jax.random streams drawn inside the fused step (utils/ebm_utils.py:342-345,360-362): per-iteration key tables
   * [iterations][2] (uint32 pairs, row tf_t0 - t), NULL = Philox / explicit z.  The state is rows
   * [sample_offset, sample_offset + B) of a global (N, S, C) array of tf_n_total elements. */
  const uint32_t* tf_noise_keys;
  const uint32_t* tf_infill_keys;
  int64_t tf_n_total;
  int32_t tf_t0;
  /* Philox key in DEVICE memory ([2] words: seed_lo, seed_hi), NULL = the seed_lo / seed_hi fields above.  A captured
   * step that reads its key here (and its timestep from t_ptr) can be replayed for a later sampling run with another rng. */
  const uint32_t* key_ptr;
} smd_sample_io;
int smd_engine_prepare_sampler(smd_engine* e, void* stream);
int smd_engine_init_state(smd_engine* e, float* x, uint32_t seed_lo, uint32_t seed_hi, uint32_t sample_offset,
                          void* stream);
/* explicit initial state (parity mode / infill / interpolation): refreshes the bf16 network input */
int smd_engine_load_state(smd_engine* e, const float* x, void* stream);
int smd_engine_sample_step(smd_engine* e, const smd_sample_io* io, void* stream);
/* The two halves of that iteration, for a software pipeline over independent chains (the batch of diffusion_dynamics is a set of
 * independent samples): part 1 = the network's stem (models/ncsn.py:152-171: in_proj .. up projection; it reads the state left by
 * the previous reverse update and does not depend on t), part 2 = the output stage (models/ncsn.py:173-178) + the fused reverse
 * update (utils/ebm_utils.py:327-394), which advances *t_ptr.  part 1 then part 2 on one stream == smd_engine_sample_step.  The
 * host runs chain A as (2, 1) and chain B as (1, 2) on two streams inside one captured graph, so one chain's latency-bound
 * encoder kernels always sit beside the other's 2048-wide GEMMs (two free-running chains drift INTO phase: DESIGN.md section 5). */
int smd_engine_sample_step_part(smd_engine* e, const smd_sample_io* io, int part, void* stream);

/* One iteration of a STRIDED walk over the timesteps: the generalised non-Markovian sampler of Song et al. 2021 (DDIM; no
 * counterpart in the reference) going down a sub-sequence of [0, T), or, going up with sigma = 0, its inversion (a deterministic
 * encoder).  The eps-net is evaluated at t = *t_ptr as in smd_engine_sample_step; the fused update then reads everything that
 * depends on the walk from two device tables indexed by t:
 *   coef[t] = (sqrt(1/ap_t), sqrt(1-ap_t)/sqrt(ap_t), a, b, sigma, clip, sqrt(ap_s), sqrt(1-ap_s))   s = the next timestep
 *   plan[t] = (next_t, iteration, slot, 0)
 *   x0 = clamp(coef0 x - coef1 eps_hat, -clip, clip) (clip = inf: none);  x' = a x0 + b x + sigma z;
 *   (x0 is rounded ONCE: the rounding error of coef1 * eps_hat is carried through the subtraction with two FMAs, so it is the
 *   same formula as smd_engine_sample_step's but not its bits -- at low noise the two products cancel and b is ~0, and the plain
 *   form's error would be the whole error of x')
 *   with infill: x' = x' (1 - mask) + y mask,  y = sqrt(ap_s) samples + sqrt(1-ap_s) zi while next_t is in [0, T), else samples
 * (the known region at the level of the state being produced).  z is read / drawn only where sigma != 0 -- z_in, else
 * jax.random.normal of tf_noise_keys row `iteration`, else Philox keyed by t -- and zi likewise from infill_z_in /
 * tf_infill_keys / Philox.  The new state also goes to the engine's bf16 network input, to collection row `slot` (0..40,
 * anything else: not collected) and its norm partials to metrics_partial[t]; the launch's last workgroup stores next_t to
 * *t_ptr.  t outside [0, T), or a row whose iteration is < 0 (a timestep that is not on the walk), makes the update a no-op
 * that advances nothing, so a walk ends by itself at next_t = -1 (sampling) or T (inversion).  io->slot_table and io->tf_t0 are
 * not used.  part: 0 the whole iteration, 1 / 2 as in smd_engine_sample_step_part (argument error under option "fp32").
 * plan->T must be the engine's num_timesteps; the plan rows, and for data_channels % 4 == 0 every fp32 array, 16-byte aligned. */
typedef struct smd_stride_plan {
  const float* coef;               /* [T][8] */
  const int32_t* plan;             /* [T][4] */
  int32_t T;
} smd_stride_plan;
int smd_engine_strided_step(smd_engine* e, const smd_sample_io* io, const smd_stride_plan* plan, int part, void* stream);

/* One iteration of a MULTISTEP walk down a sub-sequence of the timesteps: DPM-Solver++(2M) of Lu et al. 2022 (Algorithm 2, data
 * prediction; no counterpart in the reference), the deterministic strided step with one more term from the chain's history:
 *   coef[t] = (sqrt(1/ap_t), sqrt(1-ap_t)/sqrt(ap_t), a0, b, unused, clip, sqrt(ap_s), sqrt(1-ap_s), a1, 0, 0, 0)
 *   plan[t] = (next_t, iteration, slot, 0)                                       as for smd_engine_strided_step
 *   x0 = clamp(coef0 x - coef1 eps_hat, -clip, clip) (rounded once, as there);  x' = a0 x0 + a1 x0_prev + b x;  infill as there;
 *   x0_prev = x0 (the clamped value just used, before the infill blend).
 * x0_prev is one fp32 array of the state's shape per chain, owned by the caller.  It is read only where a1 != 0 and always
 * written, so the first iteration of a walk (a1 = 0: no history yet) does not depend on what the array holds; a1 = 0 everywhere is
 * smd_engine_strided_step at sigma = 0, bit for bit.  There is no noise term: io->z_in and io->tf_noise_keys are not used and
 * the noise-norm partial is that of zeros.  Everything else -- the infill draws (infill_z_in, else tf_infill_keys row
 * `iteration`, else Philox keyed by t), the bf16 network input, the collection row, metrics_partial[t], the last workgroup's
 * store of next_t, the no-op for t outside [0, T) or off the walk, `part` and its refusal under option "fp32" -- is as for
 * smd_engine_strided_step.  plan->T must be the engine's num_timesteps; the plan rows, and for data_channels % 4 == 0 every
 * fp32 array, x0_prev included, 16-byte aligned. */
typedef struct smd_multistep_plan {
  const float* coef;               /* [T][12] */
  const int32_t* plan;             /* [T][4] */
  int32_t T;
} smd_multistep_plan;
int smd_engine_multistep_step(smd_engine* e, const smd_sample_io* io, const smd_multistep_plan* plan, float* x0_prev, int part,
                              void* stream);

/* One iteration of an EXPONENTIAL ADAMS walk down a sub-sequence of the timesteps: the third-order multistep predictor in
 * lambda = log(alpha / sigma) on the clamped data prediction, optionally with a corrector that costs no network evaluation (no
 * counterpart in the reference).  The multistep step with three history terms; the table keeps the row
 * layout of smd_multistep_plan and fills its spare columns:
 *   coef[t] = (sqrt(1/ap_t), sqrt(1-ap_t)/sqrt(ap_t), A0, b, unused, clip, sqrt(ap_s), sqrt(1-ap_s), A1, A2, A3, 0)
 *   x0 = clamp(coef0 x - coef1 eps_hat, -clip, clip) (rounded once);  x' = A0 x0 + A1 h1 + A2 h2 + A3 h3 + b x;  infill as there.
 * hist is one fp32 ring [3][B][S][C] per chain, owned by the caller: iteration j (plan[t].iteration) reads h_i, the x0 of iteration
 * j - i, from slot (j - i) mod 3, and stores its own x0 (before the infill blend) into slot j mod 3.  A history whose coefficient
 * is an exact 0 is not read, so a walk does not depend on what the ring held before it; with A2 = A3 = 0 the result is
 * smd_engine_multistep_step's, bit for bit.  The corrector is folded into A0 .. A3 on the host (schedule.adams_coefficient_table),
 * so predictor and predictor-corrector are this one call.  Everything else -- the infill draws, the bf16 network input, the
 * collection row, metrics_partial[t], the last workgroup's store of next_t, the no-op for t outside [0, T) or off the walk (the
 * ring untouched too), `part` and its refusal under option "fp32", the checks -- is as for smd_engine_multistep_step; hist must be
 * non-null and, for data_channels % 4 == 0, 16-byte aligned. */
int smd_engine_adams_step(smd_engine* e, const smd_sample_io* io, const smd_multistep_plan* plan, float* hist, int part, void* stream);

/* The fused update of smd_engine_adams_step alone, on a caller's state, network output, ring, tables and timestep (per-element
 * tests; a host that runs its own network).  The struct mirrors AdamsStepArgs (csrc/smd_kernels.h) field for field; a field left
 * 0 / NULL means what it means there: x_bf16 NULL = no bf16 copy, t_advance NULL = *t_ptr is not advanced (else arrive must be a
 * zeroed counter), collection NULL = nothing collected.  hist is the ring [3][B][S][C].  No arithmetic of its own.  The checks are
 * the launcher's (null state / eps_hat / tables / t_ptr / hist, T <= 0, infill samples without masks, t_advance without arrive,
 * for C % 4 == 0 every fp32 array 16-byte aligned, the ring included) plus: a pointer not aligned to its element, infill draws
 * without masks, Cp < C.  Errors return < 0 with smd_last_error() set and launch nothing. */
typedef struct smd_adams_step_args {
  float* x;
  float* hist;
  const float* eps_hat;
  int32_t B, S, C, Cp, T;
  const float* coef;
  const int32_t* plan;
  const int32_t* t_ptr;
  int32_t* t_advance;
  uint32_t* arrive;
  uint32_t seed_lo, seed_hi;
  const uint32_t* key_ptr;
  uint32_t sample_offset;
  const float* infill_samples;
  const float* infill_masks;
  const float* infill_z_in;
  const uint32_t* tf_infill_keys;
  int64_t tf_n_total;
  smd_bf16* x_bf16;
  float* metrics_partial;
  float* collection;
} smd_adams_step_args;
int smd_adams_step(const smd_adams_step_args* a, void* stream);

/* One iteration of a walk that evaluates the variational bound of Ho et al. 2020 (eq. 5) term by term on held-out examples (no
 * counterpart in the reference).  At t = *t_ptr:
 *   smd_bound_noise   x_t = sqrt(ap_t) x0 + sqrt(1-ap_t) eps  -> x_t (fp32) and the engine's bf16 network input
 *   eps-net           eps_hat = model(x_t, sqrt(ap_t)), FiLM-table row t as in smd_engine_forward_level
 *   smd_bound_terms   partial[t][b] = (sum (x0 - x0_hat)^2, sum (eps - eps_hat)^2, sum x0^2) over (s, c), fp32, with
 *                     x0_hat = clamp(sqrt(1/ap_t) x_t - sqrt(1/ap_t - 1) eps_hat, -clip, clip); the launch's last workgroup
 *                     stores next_t[t] to *t_ptr
 * Everything that depends on the timestep is read from device memory, so one captured iteration replays for a whole walk; the
 * host weights the sums (schedule.bound_tables) in float64.  eps: eps_source 0 = the caller put it into `eps`; 1 = the call
 * first fills `eps` with jax.random.normal(tf_keys[t], (N, S, C)) for this rank's rows [sample_offset, sample_offset + B)
 * (smd_threefry_normal with the key read on the device: tf_keys [T][2] uint32, tf_n_total = N S C; rows -1 and T of the key
 * table must be readable -- the draw of an iteration that turns out to be a no-op reads one of them and is discarded);
 * 2 = Philox keyed by (seed, b + sample_offset, t) on a stream id of its own (5: neither the sampler's nor the loss's draws),
 * written to `eps`.  t outside [0, T) makes both kernels no-ops that write and advance nothing (a host issues as many
 * iterations as its walk has timesteps, as for smd_engine_strided_step).  Needs smd_engine_prepare_sampler's FiLM tables and an inference
 * workspace; works for both architectures and under the options "fp8" and "fp32".  T must be the engine's num_timesteps; table
 * rows, and for data_channels % 4 == 0 every fp32 array, 16-byte aligned. */
typedef struct smd_bound_io {
  const float* x0;                 /* [B][S][C] examples (model space) */
  float* x_t;                      /* [B][S][C] scratch: the noised examples of the current timestep */
  float* eps;                      /* [B][S][C] the draw (read or written, see eps_source) */
  int32_t* t_ptr;                  /* device timestep; replaced by next_t[t] */
  const float* table;              /* [T][4] (sqrt(ap), sqrt(1-ap), sqrt(1/ap), sqrt(1/ap - 1)) */
  const int32_t* next_t;           /* [T] the walk: next timestep after t, -1 ends it */
  int32_t T;
  float clip;                      /* > 0; inf = no clamp */
  int32_t eps_source;              /* 0 explicit, 1 jax.random (threefry), 2 Philox */
  uint32_t seed_lo, seed_hi, sample_offset;
  const uint32_t* key_ptr;         /* Philox key in device memory ([2] words) or NULL = seed_lo / seed_hi */
  const uint32_t* tf_keys;         /* eps_source 1: [T][2] key table */
  int64_t tf_n_total;
  float* partial;                  /* [T][B][3] */
} smd_bound_io;
int smd_engine_bound_step(smd_engine* e, const smd_bound_io* io, void* stream);

/* One iteration of the walk that estimates the statistic of the analytic (optimal) reverse variance of Bao et al. 2022
 * (Analytic-DPM; no counterpart in the reference) on examples.  At t = *t_ptr:
 *   smd_bound_noise    x_t = sqrt(ap_t) x0 + sqrt(1-ap_t) eps  -> x_t (fp32) and the engine's bf16 network input, as above
 *   eps-net            out = model(x_t, sqrt(ap_t)), FiLM-table row t
 *   smd_score_moments  sums[t][s][c] = sum over the batch of (A_t x_t + B_t out)^2, (A_t, B_t) = moment_table[t][0..1]: the
 *                      network's output in eps units for any prediction kind; the last workgroup stores next_t[t] to *t_ptr
 * eps_source, the key fields, the no-op for t outside [0, T) and the requirements (FiLM tables, an inference workspace, both
 * architectures, options "fp8" and "fp32", T the engine's num_timesteps, 16-byte alignment of the table rows and, for
 * data_channels % 4 == 0, of every fp32 array) are those of smd_engine_bound_step.  Row t of sums is WRITTEN, every element of
 * it, never accumulated: the host adds batches and draws in float64.  partial is a workspace of
 * ceil(B / SMD_MOMENT_CHUNK) * S * C floats. */
#define SMD_MOMENT_CHUNK 8
typedef struct smd_moment_io {
  const float* x0;                 /* [B][S][C] examples (model space) */
  float* x_t;                      /* [B][S][C] scratch: the noised examples of the current timestep */
  float* eps;                      /* [B][S][C] the draw (read or written, see eps_source) */
  int32_t* t_ptr;                  /* device timestep; replaced by next_t[t] */
  const float* noise_table;        /* [T][4] (sqrt(ap), sqrt(1-ap), sqrt(1/ap), sqrt(1/ap - 1)): smd_bound_io's table */
  const float* moment_table;       /* [T][4] (A, B, 0, 0) */
  const int32_t* next_t;           /* [T] the walk: next timestep after t, -1 ends it */
  int32_t T;
  int32_t eps_source;              /* 0 explicit, 1 jax.random (threefry), 2 Philox */
  uint32_t seed_lo, seed_hi, sample_offset;
  const uint32_t* key_ptr;         /* Philox key in device memory ([2] words) or NULL = seed_lo / seed_hi */
  const uint32_t* tf_keys;         /* eps_source 1: [T][2] key table */
  int64_t tf_n_total;
  float* partial;                  /* [ceil(B / SMD_MOMENT_CHUNK)][S][C] workspace */
  float* sums;                     /* [T][S][C] */
} smd_moment_io;
int smd_engine_moment_step(smd_engine* e, const smd_moment_io* io, void* stream);

/* smd_engine_strided_step with a PER-ELEMENT noise scale (the diagonal form of the analytic variance):
 *   x' = a x0 + b x + coef4 * sig[iteration][s][c] * z
 * coef and plan are smd_stride_plan's tables; column 4 of coef is now a 0/1 switch, and z is read / drawn (and sig read) only
 * where it is not 0.  sig is one float32 [K][S][C] table shared by every sample, indexed by the plan's `iteration`; a row whose
 * iteration is outside [0, K) is off the walk (a no-op).  z * sig is rounded once and a zero sig contributes +0, so a table
 * filled with one constant sigma and coef4 = 1 gives the bits of smd_engine_strided_step with that sigma in column 4.  The
 * draws (z_in, else tf_noise_keys row `iteration`, else Philox keyed by t), the infill blend, the bf16 network input, the
 * collection row, metrics_partial[t], the last workgroup's store of next_t, the no-op for t outside [0, T) or off the walk,
 * `part` and its refusal under option "fp32" are as for smd_engine_strided_step.  plan->T must be the engine's num_timesteps;
 * the plan rows, and for data_channels % 4 == 0 every fp32 array, sig included, 16-byte aligned. */
typedef struct smd_sigma_table {
  const float* sig;                /* [K][S][C] */
  int32_t K;
} smd_sigma_table;
int smd_engine_analytic_step(smd_engine* e, const smd_sample_io* io, const smd_stride_plan* plan, const smd_sigma_table* sig, int part,
                             void* stream);

/* One Langevin update of annealed_langevin_dynamics / consistent_langevin_dynamics (utils/ebm_utils.py:131-164, 231-253):
 *   next = x + alpha * grad + noise_coef * z;  with infill: next = next (1 - mask) + (infill_samples + infill_sigma * zi) mask.
 * grad = model(state, sigma) comes from smd_engine_forward.  z / zi: explicit arrays, else jax.random.normal(step_rng) /
 * (infill_rng) from the two threefry keys (use_threefry; the state is rows [sample_offset, +B) of a global array of
 * tf_n_total elements), else Philox keyed by (seed, global sample index, step).  metrics_partial [B][3] receives the
 * per-sample sums behind grad_norm / step_norm / noise_norm (:157-161); collect_out a copy of the new state. */
typedef struct smd_langevin_io {
  float* x;
  const float* grad;
  float alpha, noise_coef;
  const float* z_in;
  uint32_t seed_lo, seed_hi, step, sample_offset;
  int32_t use_threefry;
  uint32_t tf_noise_key[2], tf_infill_key[2];
  int64_t tf_n_total;
  const float* infill_samples;
  const float* infill_masks;
  const float* infill_z_in;
  float infill_sigma;
  float* metrics_partial;
  float* collect_out;
  /* Table mode (graph-captured loops; ABI version 3): with k_ptr != NULL the update takes its step-dependent arguments from
   * device memory, indexed by the device-side update counter k = *k_ptr, so that ONE captured (forward + update) pair can be
   * replayed for a whole annealed / consistent run:  alpha, noise_coef, infill_sigma = step_table[k][0..2]; the Philox counter
   * word and (use_threefry) the two keys key_table[k][0..1 | 2..3] are those of update k; metrics_partial is the base of an
   * [n_steps][B][3] array (row k is written); the new state is copied to collection + slot_table[k] * B*S*C when that slot
   * is >= 0; sigma_out[b] receives step_table[k][3], the noise level of the NEXT forward pass (level_out its table row); the launch's last workgroup
   * stores k + 1 to k_ptr (arrive: one zeroed uint32).  k outside [0, n_steps) makes the launch a no-op. */
  const float* step_table;
  const int32_t* slot_table;
  const uint32_t* key_table;
  int32_t* k_ptr;
  uint32_t* arrive;
  float* collection;
  float* sigma_out;
  int32_t n_steps;
  int32_t* level_out;        /* one int32: receives min((k + 1) / steps_per_level, n_levels - 1), the FiLM-table row of the next forward */
  int32_t steps_per_level, n_levels;
} smd_langevin_io;
int smd_langevin_step(const smd_langevin_io* io, int B, int S, int C, void* stream);
/* *t_ptr = t on `stream`: restarts a reverse walk (the device-side timestep of smd_engine_sample_step) without a framework fill */
int smd_set_timestep(int32_t* t_ptr, int32_t t, void* stream);


/* ---- e4m3 (OCP fp8) path: BASELINE config 5.  Operands are e4m3 bytes with one power-of-two (E8M0) scale per row,
 * contracted by v_mfma_scale_f32_32x32x64_f8f6f4; engine option "fp8" = 1 (before bind_workspace) routes the
 * DenseResBlock forward GEMMs (models/shared.py:65,69) through it. ------------------------------------------------ */
/* rows of a bf16 matrix [rows][ld] (K used) -> out8 [rows][K] e4m3(v * 2^-e), scale[rows] = E8M0 byte e + 127.  Any rows >= 1;
 * K % 8 == 0, ld >= K and ld % 8 == 0 (16-byte loads); the columns K .. ld of a row are not read. */
int smd_quantize_rows_e4m3(const smd_bf16* in, int ld, int rows, int K, uint8_t* out8, uint32_t* scale, void* stream);
/* C[M,N] = (2^sa[m] A8[m,:]) . (2^sb[n] Bt8[n,:]) + bias (+ fp32 residual) -> fp32 and/or bf16; M, N, K % 256 == 0 */
int smd_gemm_e4m3_nt(const uint8_t* A8, int lda, const uint32_t* scale_a, const uint8_t* Bt8, int ldb,
                     const uint32_t* scale_b, int M, int N, int K, const float* bias, const float* residual, int ld_res,
                     float* out_f32, int ld_out, smd_bf16* out_bf16, int ld_outb, void* stream);
/* smd_layernorm_fwd (D = 1024 / 2048, FiLM + swish or neither) writing the e4m3 copy + row scales (and bf16 if non-NULL) */
int smd_layernorm_fwd_e4m3(const float* x, int rows, int D, const float* gamma, const float* beta, const float* film_scale,
                           const float* film_shift, int ld_film, int rows_per_sample, int swish, uint8_t* out8,
                           uint32_t* out_scale, smd_bf16* out_bf16 /*nullable*/, void* stream);

/* ---- single kernels (unit-testable ops) ------------------------------------------------------- */
enum { SMD_EPI_NONE = 0, SMD_EPI_GELU = 1, SMD_EPI_SWISH = 2 };
/* C[M,N] = act(A[M,K] Bt[N,K]^T + bias) (+ residual); nn.Dense, models/ncsn.py:155 etc.  K % 64 == 0; lda, ldb >= K and
 * multiples of 8 (16-byte rows; anything else returns < 0 unlaunched).  ld_res, ld_out, ld_outb >= N, any value: only the
 * columns < N of a row are read / written, whatever lies between N and the leading dimension is left alone. */
int smd_gemm_bf16_nt(const smd_bf16* A, int lda, const smd_bf16* Bt, int ldb, int M, int N, int K,
                     const float* bias, int act, const float* residual, int ld_res, float* out_f32, int ld_out,
                     smd_bf16* out_bf16, int ld_outb, void* stream);
/* Fused encoder MLP half-layer, models/ncsn.py:163-168: h_out = h_in + Dense(gelu(Dense(LN(h_in)))) for the
 * 128-wide residual stream, rows % 32 == 0.  W1t [hidden][128] and W2t [128][hidden] are bf16 with the contraction
 * index contiguous; save_* (optional) receive LN output, pre-GELU and post-GELU activations for the backward. */
int smd_mlp_block_fwd(const float* h_in, float* h_out, int rows, const float* gamma, const float* beta,
                      const smd_bf16* W1t, const float* b1, const smd_bf16* W2t, const float* b2, int hidden,
                      smd_bf16* save_a2, smd_bf16* save_z1, smd_bf16* save_u, void* stream);
/* MLP half-layer (models/ncsn.py:163-168) with the hidden dimension split over 4 workgroups per group of 4 / 2 / 1
 * samples: a quarter of the weight stream per CU.  a2 = ln2(h_mid) in bf16 (smd_attn_block_fwd_ex emits it);
 * output: four fp32 partial tiles part[k] = part + k*rows*128 with h_out = (p0 + p1) + (p2 + p3) -- quarter 0 carries
 * b2 + the residual h_res -- to be summed by the consumer (smd_attn_block_fwd_ex / smd_ln128_parts).  hidden % 512 == 0. */
int smd_mlp_block_fwd_hs(const smd_bf16* a2, const float* h_res, int rows, const smd_bf16* W1t, const float* b1,
                         const smd_bf16* W2t, const float* b2, int hidden, float* part, void* stream);
/* backward of that half-layer between ln2 and the residual add, hidden activations recomputed from a2:
 * u = gelu(a2 W1 + b1) and dz = (dh W2^T) gelu'(.) are written ([rows][hidden] bf16, the operands of the fc2 / fc1 weight
 * gradients), da2 = dz W1^T leaves as four fp32 partial tiles (summed by smd_ln128_bwd_parts).  W1t [hidden][128]: fc1
 * forward pack; W2 [hidden][128], W1 [128][hidden]: dgrad packs of fc2 / fc1.  rows % 128 == 0, hidden % 512 == 0. */
int smd_mlp_block_bwd_hs(const smd_bf16* a2, const smd_bf16* dh, int rows, const smd_bf16* W1t, const smd_bf16* W2,
                         const smd_bf16* W1, const float* b1, int hidden, smd_bf16* u, smd_bf16* dz, float* part, void* stream);
/* The four *_parts / *_ex / *_bwd_ln entries below read the partial tiles p_k = parts + k*part_stride as float2: part_stride
 * must be even and >= rows*128 (disjoint tiles), the fp32 row operands 8-byte aligned; anything else returns -1 unlaunched.
 * LayerNorm (D = 128) backward with dout = (p0 + p1) + (p2 + p3) (fp32 partial tiles): dx = LN-backward + dres (nullable)
 * -> dx_f32 (nullable, may alias dres) / dx_bf16 (nullable); partial [rows/32][2][128] = per-group dgamma / dbeta sums */
int smd_ln128_bwd_parts(const float* x, const float* parts, int64_t part_stride, int rows, const float* gamma,
                        const float* dres, float* dx_f32, smd_bf16* dx_bf16, float* partial, void* stream);
/* x = (p0 + p1) + (p2 + p3) per 128-wide row (parts + k*part_stride); x_out (nullable) <- x, ln_out (nullable) <-
 * LayerNorm(x) bf16: the encoder's final norm (models/ncsn.py:170) on a hidden-split MLP output */
int smd_ln128_parts(const float* parts, int64_t part_stride, int rows, const float* gamma, const float* beta, float* x_out,
                    smd_bf16* ln_out, void* stream);
/* smd_attn_block_fwd with (a) the input given as four partial tiles (h_parts != NULL: h_in unused; h_comb nullable
 * receives their sum) and (b) the LayerNorm of the OUTPUT rows (ln2 of the same layer) written as bf16 a2_out (nullable) */
int smd_attn_block_fwd_ex(const float* h_in, const float* h_parts, int64_t part_stride, float* h_comb, float* h_out, int rows,
                          const float* gamma, const float* beta, const smd_bf16* Wqkv_t, const float* b_qkv,
                          const smd_bf16* Wo_t, const float* b_o, int num_heads, const float* gamma2, const float* beta2,
                          smd_bf16* a2_out, smd_bf16* save_a1, smd_bf16* save_qkv, smd_bf16* save_o, void* stream);
/* Fused encoder attention half-layer, models/ncsn.py:159-162: h_out = h_in + out(softmax(q k^T / sqrt(d)) v) with
 * q,k,v = Dense(LN(h_in)); 32 tokens per sample, 128-wide stream, num_heads in {4, 8, 16}.  Wqkv_t [384][128]
 * (q | k | v rows), Wo_t [128][128], bf16, contraction contiguous; save_qkv receives the unscaled q. */
int smd_attn_block_fwd(const float* h_in, float* h_out, int rows, const float* gamma, const float* beta,
                       const smd_bf16* Wqkv_t, const float* b_qkv, const smd_bf16* Wo_t, const float* b_o, int num_heads,
                       smd_bf16* save_a1, smd_bf16* save_qkv, smd_bf16* save_o, void* stream);
/* Backward of that half-layer between its LayerNorms: dO = dh_mid Wo^T, attention backward (softmax recomputed
 * from the saved qkv), da1 = dqkv Wqkv^T.  Wo [128 in][128 out], Wqkv [128 in][384 out]: bf16, out index contiguous. */
int smd_attn_block_bwd(const smd_bf16* dh_mid, const smd_bf16* qkv, const smd_bf16* Wo, const smd_bf16* Wqkv,
                       smd_bf16* dqkv, smd_bf16* da1, int rows, int num_heads, void* stream);
/* The backward of models/ncsn.py:159-164 from the MLP's input gradient to the layer's input gradient in ONE launch: LayerNorm-2
 * backward on da2 given as four partial tiles (part_stride floats apart, summed (p0 + p1) + (p2 + p3)) + the residual gradient dh,
 * the attention half-layer backward (smd_attn_block_bwd), LayerNorm-1 backward + residual.  dh [rows][128] fp32 is read and then
 * overwritten IN PLACE with the gradient that leaves the layer; dh_mid_out / dh_out: its bf16 copies between the half-layers (the
 * operand of out_proj's weight gradient) and at the exit; partial1 / partial2 [rows/32][2][128]: dgamma | dbeta sums per sample
 * of LayerNorm 1 / 2 (reduce with smd_ln_bwd_reduce); da1 optional. */
int smd_attn_block_bwd_ln(const smd_bf16* qkv, const smd_bf16* Wo, const smd_bf16* Wqkv, smd_bf16* dqkv, smd_bf16* da1,
                          const float* h_mid, const float* da2_parts, int64_t part_stride, const float* gamma2, float* dh,
                          smd_bf16* dh_mid_out, float* partial2, const float* h, const float* gamma1, smd_bf16* dh_out,
                          float* partial1, int rows, int num_heads, void* stream);
/* dW[Kd,N] = X[M,Kd]^T dY[M,N] and db[N] = colsum(dY) (weight + bias gradient of nn.Dense).
 * tr_path 1: zero_page = 128 zeroed bf16, slab = smd_gemm_tn_slab_elems() floats (split-K partials);
 * tr_path 0: scratch = (Kd+N)*roundup(M,64) bf16 for explicit transposes (+ slab for the bias). */
int smd_gemm_bf16_tn(const smd_bf16* X, int ldx, const smd_bf16* dY, int ldy, int M, int Kd, int N, float* out,
                     int ldo, float* bias_out, const smd_bf16* zero_page, float* slab, int64_t slab_elems,
                     smd_bf16* scratch, int64_t scratch_elems, int tr_path, void* stream);
int64_t smd_gemm_tn_slab_elems(void);
/* flax.nn.LayerNorm (+ FiLM + swish), models/shared.py:62-68 */
int smd_layernorm_fwd(const float* x, int rows, int D, const float* gamma, const float* beta,
                      const float* film_scale, const float* film_shift, int ld_film, int rows_per_sample,
                      int swish, smd_bf16* out, void* stream);
/* the engine's form: the input row as fp32 (x) or bf16 (x_bf16: the 2048-wide trunk), exactly one of them non-NULL */
int smd_layernorm_fwd_ex(const float* x, const smd_bf16* x_bf16, int rows, int D, const float* gamma, const float* beta,
                         const float* film_scale, const float* film_shift, int ld_film, int rows_per_sample, int swish,
                         smd_bf16* out, void* stream);
int smd_layernorm_bwd(const float* x, int rows, int D, const float* gamma, const float* beta,
                      const float* film_scale, const float* film_shift, int ld_film, int rows_per_sample,
                      int swish, const smd_bf16* dout, float* dx, float* dgamma, float* dbeta, float* dscale,
                      float* dshift, float* partial, int64_t partial_elems, void* stream);
/* flax.nn.SelfAttention core, models/ncsn.py:161 */
/* (every LayerNorm backward WRITES dgamma / dbeta -- the sum over its row groups -- it does not accumulate into them;
 * partial is scratch of partial_elems >= ngroups * 2 * D floats, ngroups = ceil(rows / g) with g = rows_per_sample when FiLM
 * is given and 32 otherwise: less returns < 0 unlaunched)
 * the engine's form of the LayerNorm backward: optional fp32 residual gradient `dres` added to dx (may alias dx: the
 * in-place residual-gradient stream), optional bf16 copy of dx, bf16 or fp32 input */
int smd_layernorm_bwd_ex(const float* x, const smd_bf16* x_bf16, int rows, int D, const float* gamma, const float* beta,
                         const smd_bf16* dout, const float* dres, float* dx, smd_bf16* dx_bf16, float* dgamma, float* dbeta,
                         float* partial, int64_t partial_elems, void* stream);
/* ... and the ResBlock form (models/shared.py:62-68): FiLM + swish, bf16 or fp32 input, the residual gradient in fp32
 * (`dres`) or bf16 (`dres_bf16`, D in {1024, 2048}), fp32 and/or bf16 dx; dfilm_accumulate: dscale/dshift += */
int smd_layernorm_bwd_film(const float* x, const smd_bf16* x_bf16, int rows, int D, const float* gamma, const float* beta,
                           const float* film_scale, const float* film_shift, int ld_film, int rows_per_sample, int swish,
                           const smd_bf16* dout, const float* dres, const smd_bf16* dres_bf16, float* dx,
                           smd_bf16* dx_bf16, float* dgamma, float* dbeta, float* dscale, float* dshift,
                           int dfilm_accumulate, float* partial, int64_t partial_elems, void* stream);
/* ... and with saved row statistics, as the engine's training step runs its output-stage LayerNorms: smd_layernorm_fwd_stats is smd_layernorm_fwd_ex / _fwd_e4m3 in one call (out and/or out8 + out_scale)
 * that also writes (mean, rstd) of every row to stats_out, fp32 [rows][2], when it is non-NULL; smd_layernorm_bwd_stats is
 * smd_layernorm_bwd_film reading those statistics instead of recomputing them (D = 2048 8-wave kernel; every other kernel and a
 * NULL pointer recompute them from x). */
int smd_layernorm_fwd_stats(const float* x, const smd_bf16* x_bf16, int rows, int D, const float* gamma, const float* beta,
                            const float* film_scale, const float* film_shift, int ld_film, int rows_per_sample, int swish,
                            smd_bf16* out, uint8_t* out8, uint32_t* out_scale, float* stats_out, void* stream);
int smd_layernorm_bwd_stats(const float* x, const smd_bf16* x_bf16, int rows, int D, const float* gamma, const float* beta,
                            const float* film_scale, const float* film_shift, int ld_film, int rows_per_sample, int swish,
                            const smd_bf16* dout, const float* dres, const smd_bf16* dres_bf16, float* dx,
                            smd_bf16* dx_bf16, float* dgamma, float* dbeta, float* dscale, float* dshift,
                            int dfilm_accumulate, float* partial, int64_t partial_elems, const float* stats, void* stream);
int smd_attention_fwd(const smd_bf16* qkv, smd_bf16* out, int B, int S, int E, int H, void* stream);
int smd_attention_bwd(const smd_bf16* qkv, const smd_bf16* dout, smd_bf16* dqkv, int B, int S, int E, int H,
                      void* stream);
/* NoiseEncoding.apply, models/ncsn.py:28-41 */
int smd_noise_embed(const float* noise_level, int n, int channels, smd_bf16* out, int ld_out, void* stream);
/* The loss-side and optimiser kernels without an engine handle (the engine calls the same launchers).
 * smd_q_sample: utils/losses.py:271-296.  x0 [B][S][C] fp32 -> xt_bf16 [B*S][Cp] (the columns >= C are not written),
 *   eps_out [B][S][C], noise_level_out [B] = sqrt(used_alpha).  labels NULL -> Philox labels in
 *   [label_min, label_min + T) keyed by (seed, b + sample_offset, *step_ptr); used_alphas NULL -> alphas_prod_ext[label - 1]
 *   (label 0: a uniform draw in [alphas_prod_ext[T], 1)); eps_in NULL -> Philox normals.  S*C need not be a multiple of 4.
 * smd_mse_fwd_bwd: :304-305 and d(mean loss)/d pred: loss_per_sample [B], dpred_bf16 [B*S][Cp] = 2 (pred - eps) *
 *   inv_global_count (the columns >= C are not written, as in smd_q_sample: the caller zeroes them once).
 * smd_adam_clip_ema: train_ncsn.py:284-287,340-342,364-365 on flat fp32 buffers of n elements: gradient norm -> clip ->
 *   Adam with the stepped LR evaluated from *step_ptr (incremented by the kernel) -> EMA (ema may be NULL).
 *   norm_partial: >= 1024 floats of scratch; metrics_out [4] = norm before clip, after clip, lr, step.
 * Alignment: where S*C % 4 == 0 (smd_q_sample) or C % 4 == 0 and Cp % 4 == 0 (smd_mse_fwd_bwd, smd_ddpm_reverse_step with Cp = C) the
 *   fp32 arrays must be 16-byte aligned and the bf16 array 8-byte aligned (16-byte loads); anything else is refused before the launch. */
int smd_q_sample(const float* x0, int B, int S, int C, int Cp, int T, const float* alphas_prod_ext, const int32_t* labels,
                 int label_min, const float* used_alphas, const float* eps_in, uint32_t seed_lo, uint32_t seed_hi,
                 const uint32_t* step_ptr, uint32_t sample_offset, smd_bf16* xt_bf16, float* eps_out,
                 float* noise_level_out, void* stream);
int smd_mse_fwd_bwd(const float* pred, const float* eps, int B, int S, int C, int Cp, float inv_global_count,
                    float* loss_per_sample, smd_bf16* dpred_bf16, void* stream);
int smd_adam_clip_ema(float* params, const float* grads, float* m, float* v, float* ema, int64_t n,
                      const smd_train_hyper* h, uint32_t* step_ptr, float* norm_partial, float* metrics_out, void* stream);
/* Weighted training (no reference counterpart).
 * smd_weighted_mse_fwd_bwd: smd_mse_fwd_bwd with a weight per sample, w_b = iw_b min(1, min_snr_gamma (1 - s_b^2) / s_b^2) with
 *   s = noise_level [B] (what smd_q_sample stored); iw NULL = 1; min_snr_gamma <= 0 or +inf: no SNR factor (noise_level may then
 *   be NULL); s = 1 gives w = 0, not a NaN.  dpred_bf16 = 2 w_b (pred - eps) * inv_global_count (columns >= C not written),
 *   loss_per_sample [B] the UNWEIGHTED mean -- the bits smd_mse_fwd_bwd writes -- and weight_per_sample [B] = w_b.  Alignment as
 *   for smd_mse_fwd_bwd.
 * smd_timestep_draw: B timesteps from the table p [n] by its inclusive cdf [n]: labels_out[b] = label_base + (first i with
 *   cdf[i] > u_b, the last index when there is none), iw_out[b] = 1 / (n p[i]) (the weight that keeps the objective unbiased).
 *   u_b = u_in[b], or with u_in NULL 24 Philox bits in [0, 1) keyed by (seed, b + sample_offset, step) on a stream of their own;
 *   step_ptr (device, NULL-able) replaces `step`, as in smd_q_sample.
 * smd_timestep_update: the loss-second-moment resampler of Nichol & Dhariwal 2021.  history [n][10] and counts [n] are updated
 *   in place with the Bg pairs (labels[j] - label_base, loss[j]) IN ORDER (a row fills front to back, a full row shifts left and
 *   appends; labels outside the table are dropped); then, once every count is 10, p_out[i] = sqrt(mean_j history[i][j]^2)
 *   normalised to sum 1, times (1 - uniform_mix), plus uniform_mix / n -- before that p_out = 1 / n -- cdf_out = its inclusive
 *   prefix sums and *warmed_out = 1 / 0.  One workgroup, fixed summation order, no atomics: the same input gives the same bits. */
int smd_weighted_mse_fwd_bwd(const float* pred, const float* eps, const float* noise_level, const float* iw, float min_snr_gamma,
                             int B, int S, int C, int Cp, float inv_global_count, float* loss_per_sample,
                             float* weight_per_sample, smd_bf16* dpred_bf16, void* stream);
/* smd_weighted_mse_fwd_bwd for a network that predicts x0 (kind 1) or v (kind 2): target and w_b as tabulated at
 * smd_engine_set_loss_weights, x0 [B][S][C] fp32 (16-byte aligned like pred when C and Cp are multiples of 4).  eps may be NULL for
 * kind 1; noise_level may be NULL for kind 1 without an SNR factor.  kind 0 forwards to smd_weighted_mse_fwd_bwd (x0 unused). */
int smd_param_mse_fwd_bwd(const float* pred, const float* eps, const float* x0, const float* noise_level, const float* iw,
                          float min_snr_gamma, int kind, int B, int S, int C, int Cp, float inv_global_count,
                          float* loss_per_sample, float* weight_per_sample, smd_bf16* dpred_bf16, void* stream);
int smd_timestep_draw(const float* cdf, const float* p, int n, int label_base, int B, uint32_t seed_lo, uint32_t seed_hi,
                      uint32_t sample_offset, uint32_t step, const uint32_t* step_ptr, const float* u_in, int32_t* labels_out,
                      float* iw_out, void* stream);
int smd_timestep_update(const int32_t* labels, const float* loss, int Bg, float* history, int32_t* counts, int n, int label_base,
                        float uniform_mix, float* p_out, float* cdf_out, int32_t* warmed_out, void* stream);
/* Philox4x32-10 normals: out[b][e], counter (e/4, b + sample_offset, stream_id, 0) */
int smd_rng_normal(float* out, int B, int per_sample, uint32_t seed_lo, uint32_t seed_hi, uint32_t stream_id,
                   uint32_t sample_offset, void* stream);
/* jax.random-compatible draws (jax 0.2.8 threefry2x32 conventions; replaces jax.random.{randint,uniform,normal} at
 * utils/losses.py:272-294, utils/ebm_utils.py:343-345,361-362, train_ncsn.py:539-540).  Each call fills the window
 * [offset, offset+count) of a logical array of n_total <= 2^32 elements with exactly the values
 * jax.random.X(key=(k0,k1), shape=(n_total,)) holds there, so sharded callers reproduce the single-process stream.
 * smd_threefry_normal: key_table != NULL takes the key from key_table[idx_add + idx_mul * *idx_ptr] on device
 * (uint32 pairs), which keeps a captured reverse-sampling step replayable. */
int smd_threefry_bits(uint32_t* out, int64_t n_total, int64_t offset, int64_t count, uint32_t k0, uint32_t k1, void* stream);
int smd_threefry_uniform(float* out, int64_t n_total, int64_t offset, int64_t count, uint32_t k0, uint32_t k1,
                         float minval, float maxval, void* stream);
int smd_threefry_normal(float* out, int64_t n_total, int64_t offset, int64_t count, uint32_t k0, uint32_t k1,
                        const uint32_t* key_table, const int32_t* idx_ptr, int idx_mul, int idx_add, void* stream);
int smd_threefry_randint(int32_t* out, int64_t n_total, int64_t offset, int64_t count, uint32_t k0, uint32_t k1,
                         int32_t minval, int32_t maxval, void* stream);
/* in [rows][cols] fp32 -> out [rows][ld_out] bf16: the columns cols .. ld_out of every row are WRITTEN as +0 (the zero padding
 * the GEMMs contract over); nothing behind row rows - 1 is touched */
int smd_cast_pad_bf16(const float* in, int rows, int cols, smd_bf16* out, int ld_out, void* stream);
/* one reverse step on explicit eps_hat (the elementwise part of utils/ebm_utils.py:327-394); coef is the [T][8]
 * table, *t_ptr outside [0, T) makes the call a no-op */
int smd_ddpm_reverse_step(float* x, const float* eps_hat, int B, int S, int C, const float* coef, int T,
                          const int32_t* t_ptr, const float* z_in, uint32_t seed_lo, uint32_t seed_hi,
                          uint32_t sample_offset, float* metrics_partial, float* collection,
                          const int32_t* slot_table, void* stream);
/* The two kernels of smd_engine_bound_step on explicit arrays.  table is the [T][4] table of smd_bound_io (16-byte aligned);
 * *t_ptr outside [0, T) makes either call a no-op that writes nothing.
 * smd_bound_noise: x_t [B][S][C] = sqrt(ap_t) x0 + sqrt(1-ap_t) eps (one FMA per element) and, with xt_bf16 != NULL, its bf16
 *   rounding at [B*S][Cp] (the columns >= C are not written).  draw 0: eps is read; draw != 0: eps is WRITTEN with Philox
 *   normals, counter (e/4, b + sample_offset, 5, t), key = key_ptr[0..1] if key_ptr != NULL else (seed_lo, seed_hi).
 * smd_bound_terms: partial[t][b][0..2] = (sum (x0 - x0_hat)^2, sum (eps - eps_hat)^2, sum x0^2), partial [T][B][3] fp32, only row
 *   t is written.  x0 - x0_hat is sqrt_m1 (eps_hat - eps) plus the two O(1e-7) terms the rounding of the table rows leaves
 *   where the reconstruction is inside [-clip, clip], x0 -/+ clip elsewhere.  No atomics on floats, a fixed summation order:
 *   a sample's sums depend on its own rows only (not on B or the other samples), and two calls agree bitwise.  next_t != NULL:
 *   the launch's last workgroup stores next_t[t] to *t_ptr (arrive: one zeroed uint32, reset by the kernel). */
int smd_bound_noise(const float* x0, int B, int S, int C, int Cp, const float* table, int T, const int32_t* t_ptr, float* eps,
                    int draw, uint32_t seed_lo, uint32_t seed_hi, const uint32_t* key_ptr, uint32_t sample_offset, float* x_t,
                    smd_bf16* xt_bf16, void* stream);
int smd_bound_terms(const float* x0, const float* eps, const float* eps_hat, int B, int S, int C, const float* table, int T,
                    float clip, int32_t* t_ptr, const int32_t* next_t, uint32_t* arrive, float* partial, void* stream);
/* The reduction of smd_engine_moment_step on explicit arrays: sums[t][s][c] = sum over b of (A x_t[b][s][c] + B out[b][s][c])^2
 * with (A, B) = table[t][0..1] (table [T][4] fp32, 16-byte aligned), one FMA for eps_hat and one for its square, fp32.  The
 * batch is summed in chunks of SMD_MOMENT_CHUNK rows into partial [ceil(B / SMD_MOMENT_CHUNK)][S][C] and a second launch
 * adds the chunks in chunk order: no atomics on floats, two calls agree bitwise.  Only row t of sums [T][S][C] is written,
 * every element of it; x_t and out are contiguous [B][S][C] (no padding columns are read); *t_ptr outside [0, T) makes the
 * call a no-op that writes nothing.  next_t != NULL: the second launch's last workgroup stores next_t[t] to *t_ptr (arrive:
 * one zeroed uint32, reset by the kernel).  For C % 4 == 0 all four arrays must be 16-byte aligned. */
int smd_score_moments(const float* x_t, const float* out, int B, int S, int C, const float* table, int T, int32_t* t_ptr,
                      const int32_t* next_t, uint32_t* arrive, float* partial, float* sums, void* stream);
/* The three element-wise kernels of a progressive-distillation step (Salimans & Ho 2022) on explicit
 * arrays.  Every sample has a walk step of its own: steps [B] int32 in [0, N) picks its row of table [N][16] fp32 (16-byte
 * aligned; columns c0_t, c1_t, a, b, clip, alpha_t, sigma_t, alpha_m, c0_m, c1_m, w1, w2, weight, 1/sigma_t, 0, 0).  A step outside
 * [0, N) makes that sample a no-op: none of its outputs is written.  All arrays [B][S][C] fp32, contiguous; when C is a
 * multiple of 4 they must be 16-byte aligned (anything else is refused before the launch).  Nothing but the outputs named
 * here is written.
 * smd_distill_noise: z_t = fmaf(alpha_t, x0, sigma_t * eps), level_out[b] = alpha_t.  draw 0: eps is read; draw != 0: eps is
 *   WRITTEN with Philox normals, counter (e/4, b + sample_offset, 7, step), step_ptr (device, NULL-able) replacing `step`.
 * smd_distill_mid: x1 = clamp(c0_t z_t - c1_t out1, -clip, clip) (rounded once, as the strided sampler forms it),
 *   z_m = fmaf(a, x1, b * z_t), level_out[b] = alpha_m.  z_m has the bits the strided sampler step writes at sigma = 0 from
 *   the same table entries.
 * smd_distill_loss: x2 = clamp(c0_m z_m - c1_m out2, -clip, clip), x~ = w1 x1 + w2 x2, the student's target by its kind
 *   (0 eps: (z_t - alpha_t x~) * (1/sigma_t), 1 x0: x~, 2 v: (alpha_t z_t - x~) * (1/sigma_t), 1/sigma_t the table's column; z_t may
 *   be NULL for kind 1), evaluated per element in float64 from the fp32 inputs and rounded once: the eps and v targets are a
 *   cancelling difference over sigma_t, which fp32 arithmetic would carry into pred - target.
 *   loss_per_sample [B] the UNWEIGHTED mean of (pred - target)^2 (fp32, fixed summation order, no atomics: a sample's value
 *   depends on its own rows only and two calls agree bitwise), weight_per_sample [B] = iw_b * weight (iw NULL = 1),
 *   dpred = 2 w_b (pred - target) * inv_global_count in fp32, the layout smd_engine_backward_from takes, and, with
 *   target_out != NULL, the target itself. */
int smd_distill_noise(const float* x0, int B, int S, int C, const float* table, int N, const int32_t* steps, float* eps, int draw,
                      uint32_t seed_lo, uint32_t seed_hi, uint32_t sample_offset, uint32_t step, const uint32_t* step_ptr,
                      float* z_t, float* level_out, void* stream);
int smd_distill_mid(const float* z_t, const float* out1, int B, int S, int C, const float* table, int N, const int32_t* steps,
                    float* x1, float* z_m, float* level_out, void* stream);
int smd_distill_loss(const float* x1, const float* z_m, const float* out2, const float* z_t, const float* pred, int kind, int B,
                     int S, int C, const float* table, int N, const int32_t* steps, const float* iw, float inv_global_count,
                     float* loss_per_sample, float* weight_per_sample, float* dpred, float* target_out, void* stream);

/* ---- reference-precision (fp32) kernels of the engine option "fp32" -----------------------------------------------------
 * smd_gemm_f32: out[m][n] = act(sum_k A[m][k] W[k][n] + bias[n]) + residual[m or m % res_row_mod][n], nn.Dense with A
 *   (M x K, row stride lda) and W (K x N, row stride ldw: the flax kernel layout, read in place) fp32, on
 *   v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulation in k order.  act: SMD_EPI_*; bias and residual may be NULL;
 *   residual may alias out; res_row_mod > 0 indexes the residual by m % res_row_mod (positional encoding).  Any M, N, K >= 1
 *   (edges are masked; no padding is read or written).  All pointers 4-byte aligned (16-byte aligned operands with lda / ldw
 *   and K / N multiples of 4 take vector loads).  An output element's bits depend on its row of A, its column of W and K only:
 *   not on M, and two calls agree bitwise. */
int smd_gemm_f32(const float* A, int lda, const float* W, int ldw, int M, int N, int K, const float* bias, int act,
                 const float* residual, int ld_res, int res_row_mod, float* out, int ld_out, void* stream);
/* flax LayerNorm (variance E[x^2] - mean^2, eps 1e-6) fp32 -> fp32, optional FiLM scale * ln + shift (row of the sample, or
 * table row *t_ptr clamped to film_rows when t_ptr != NULL) and swish; any D >= 1 */
int smd_layernorm_f32(const float* x, int rows, int D, const float* gamma, const float* beta, const float* film_scale,
                      const float* film_shift, int ld_film, int rows_per_sample, const int32_t* t_ptr, int film_rows, int swish,
                      float* out, void* stream);
/* softmax((q / sqrt(d)) k^T) v in fp32: qkv [B*32][3E] = [q | k | v], out [B*32][E]; S == 32, d = E / H in {8, 16, 32} */
int smd_attention_f32(const float* qkv, float* out, int B, int S, int E, int H, void* stream);
/* NoiseEncoding (models/ncsn.py:28-41), fp32 rows: [sin | cos]((5000 s) f_i) with full range reduction */
int smd_noise_embed_f32(const float* s, int n, int channels, float* out, int ld_out, void* stream);

/* ---- sample-quality distances (utils/metrics.py:24-77, called by sample_ncsn.py:69-186 evaluate()) on exact-fp32 MFMA ----
 * smd_pair_kernel_sums: utils/metrics.py:57-77 (mmd_rbf, mmd_polynomial through sklearn 0.19 rbf_kernel / polynomial_kernel).
 *   X (nx x d) and Y (ny x d) are row-major fp32 with row strides ldx, ldy (in floats).  ONE pass over X Y^T writes
 *   out[0] = sum_ij exp(-gamma_rbf * max(d2_ij, 0)),  d2_ij = (-2 <x_i,y_j> + |x_i|^2) + |y_j|^2 (euclidean_distances' order)
 *   out[1] = sum_ij (gamma_poly * <x_i,y_j> + coef0)^degree
 *   as fp64 (device pointer, 2 doubles); the nx x ny kernel matrix is never formed.  symmetric != 0: Y is X (y and ldy are
 *   ignored, nx == ny), only the upper triangle of tiles runs and d2 is 0 on the diagonal (sklearn's `X is Y`).  Any d >= 1,
 *   integer degree >= 1.  Deterministic: a second call on the same inputs gives the same bits.  workspace: >=
 *   smd_pair_kernel_sums_workspace_bytes(nx, ny, symmetric) bytes, 8-byte aligned; x, y 4-byte aligned. */
int64_t smd_pair_kernel_sums_workspace_bytes(int nx, int ny, int symmetric);
int smd_pair_kernel_sums(const float* x, int64_t ldx, int nx, const float* y, int64_t ldy, int ny, int d, int symmetric,
                         float gamma_rbf, float gamma_poly, float coef0, int degree, void* workspace, int64_t workspace_bytes,
                         double* out, void* stream);
/* smd_moments: utils/metrics.py:29-30 (np.mean(x, axis=0), np.cov(x, rowvar=False)) for X (n x d, row stride ld): mean [d]
 *   and the ddof = 1 covariance cov [d][d] row-major, both fp64 (device pointers, 8-byte aligned).  The rows are centred in
 *   fp64 and rounded to fp32 before their Gram is taken on the MFMA; n >= 2, 1 <= d <= SMD_MOMENTS_MAX_D.  workspace: >=
 *   smd_moments_workspace_bytes(n, d) bytes, 8-byte aligned. */
#define SMD_MOMENTS_MAX_D 1024
int64_t smd_moments_workspace_bytes(int n, int d);
int smd_moments(const float* x, int64_t ld, int n, int d, void* workspace, int64_t workspace_bytes, double* mean, double* cov,
                void* stream);

/* ---- nearest-neighbour metrics (improved precision / recall and realism, Kynkaanniemi et al. 2019; the reference's
 * sample_ncsn.py:148-157 logs them, DESIGN.md section 14 defines them) on the same Gram tile, the n x n distances never written ----
 * smd_knn_radii: r2[i] (fp32, device) = the k-th smallest d2 from row i of X (n x d, row stride ld) to its OTHER rows -- self
 *   is excluded by index, a duplicated row counts (and gives 0).  d2 = (-2 <x,y> + |x|^2) + |y|^2 clamped at 0, x = row i.
 *   1 <= k <= SMD_KNN_MAX_K, n >= k + 1, any d >= 1.  No atomics: two calls give the same bits.  workspace: >=
 *   smd_knn_radii_workspace_bytes(n, k) bytes, 8-byte aligned; x, r2 4-byte aligned. */
#define SMD_KNN_MAX_K 8
int64_t smd_knn_radii_workspace_bytes(int n, int k);
int smd_knn_radii(const float* x, int64_t ld, int n, int d, int k, void* workspace, int64_t workspace_bytes, float* r2, void* stream);
/* smd_ball_cover: for queries Q (nq x d) against centres X (nx x d) with squared radii r2[nx], ONE Gram pass writes
 *   covered[j]  = 1 if some centre i has d2(q_j, x_i) <= r2[i], else 0 (uint8)
 *   realism2[j] = max over the centres with keep[i] != 0 of min(r2[i] / max(d2(q_j, x_i), FLT_MIN), FLT_MAX), 0 if there is none
 *   with d2 = (-2 <q,x> + |x_i|^2) + |q_j|^2 clamped at 0: the bits smd_knn_radii took r2[i] from when Q is X.  keep (nx bytes)
 *   may be NULL: every centre is kept; coverage ignores it.  exclude_diagonal != 0 (nq == nx, Q is X): the pair (i, i) takes
 *   part in neither output (leave-one-out).  OR and max do not depend on order: two calls give the same bits.  workspace: >=
 *   smd_ball_cover_workspace_bytes(nq, nx) bytes, 8-byte aligned; q, x, r2, realism2 4-byte aligned. */
int64_t smd_ball_cover_workspace_bytes(int nq, int nx);
int smd_ball_cover(const float* q, int64_t ldq, int nq, const float* x, int64_t ldx, int nx, int d, const float* r2,
                   const uint8_t* keep, int exclude_diagonal, void* workspace, int64_t workspace_bytes, uint8_t* covered,
                   float* realism2, void* stream);
/* smd_nn_search: for every row q_j of Q (nq x d, row stride ldq) the k candidates of X (nx x d, row
 *   stride ldx) with the smallest (d2, global index) in lexicographic order, the global index of candidate i being x_base + i:
 *   d2_out[j][0..k) ascending (fp32) and idx_out[j][0..k) (int64), both [nq][k] contiguous.  d2 = (-2 <q,x> + |q|^2) + |x|^2
 *   clamped at 0, the query owning the expression (smd_knn_radii's bits when Q is X).  Equal d2 bits are ordered by the lower
 *   global index, in every comparison the kernels make.  exclude_self != 0: the pair with q_base + j == x_base + i takes part
 *   in nothing (by index: a duplicate of the query still counts, with its own d2).  accumulate == 0: the lists start as
 *   (+inf, -1), which stays as the tail where fewer than k candidates exist (no error).  accumulate != 0: d2_out / idx_out hold
 *   the valid result of earlier calls (possibly padded with (+inf, -1)) and the new candidates are merged into it under the same
 *   order -- one call on all of X and calls on any partition of X into slabs, in any order, give the same bits in both outputs.
 *   1 <= k <= SMD_KNN_MAX_K, any nq, nx, d >= 1, q_base, x_base >= 0.  No atomics: two calls give the same bits.  workspace: >=
 *   smd_nn_search_workspace_bytes(nq, nx, k) bytes, 8-byte aligned; q, x, d2_out 4-byte and idx_out 8-byte aligned. */
int64_t smd_nn_search_workspace_bytes(int nq, int nx, int k);
int smd_nn_search(const float* q, int64_t ldq, int nq, int64_t q_base, const float* x, int64_t ldx, int nx, int64_t x_base, int d, int k,
                  int exclude_self, int accumulate, void* workspace, int64_t workspace_bytes, float* d2_out, int64_t* idx_out,
                  void* stream);

/* ---- k-means over latent frames (the primitive of the PRD precision / recall histogram, Sajjadi et al. 2018, and of the NDB
 * score, Richardson & Weiss 2018; the reference's sample_ncsn.py:141-146,160 logs them, DESIGN.md section 15 defines them) ----
 * smd_kmeans_assign: ONE Gram pass of X (n x d, row stride ld) against centres (k x d, contiguous), 1 <= k <= SMD_KMEANS_MAX_K:
 *   labels[i]  = arg min_j s_ij,  s_ij = -2 <x_i, c_j> + |c_j|^2 (dot product on the MFMA in k order, |c_j|^2 one fmaf chain),
 *                ties to the lowest j (int32); |x_i|^2 takes no part in the order
 *   min_d2[i]  = max(s_i,label + |x_i|^2, 0) (fp32; may be NULL).  A row whose bits are a centre's gives exactly 0.
 *   *inertia   = sum_i min_d2[i] as fp64 (device pointer), per-workgroup fp64 partials added in a fixed order
 *   *changed   = prev != 0: how many labels differ from what the labels buffer held before the call; prev == 0: n (int64, device)
 *   No atomics: two calls give the same bits.  Any n, d >= 1.  workspace: >= smd_kmeans_assign_workspace_bytes(n, k) bytes,
 *   8-byte aligned; x, centres, labels, min_d2 4-byte and inertia, changed 8-byte aligned. */
#define SMD_KMEANS_MAX_K 128
int64_t smd_kmeans_assign_workspace_bytes(int n, int k);
int smd_kmeans_assign(const float* x, int64_t ld, int n, int d, const float* centres, int k, int prev, void* workspace,
                      int64_t workspace_bytes, int32_t* labels, float* min_d2, double* inertia, int64_t* changed, void* stream);
/* smd_kmeans_update: counts[j] (int64) = the rows of X with labels[i] == j, centres[j] (k x d fp32, contiguous) = their mean,
 *   or prev_centres[j] bit for bit when there are none (centres may alias prev_centres).  Sums in fp64: 256-row slab partials
 *   in the workspace, each a row-ordered sum, added in an order fixed by (n, d, k), then one division and one rounding to fp32; no atomics, two
 *   calls give the same bits.  A label outside [0, k) is counted nowhere.  workspace: >=
 *   smd_kmeans_update_workspace_bytes(n, d, k) bytes, 8-byte aligned; counts 8-byte, the other pointers 4-byte aligned. */
int64_t smd_kmeans_update_workspace_bytes(int n, int d, int k);
int smd_kmeans_update(const float* x, int64_t ld, int n, int d, const int32_t* labels, const float* prev_centres, int k,
                      void* workspace, int64_t workspace_bytes, float* centres, int64_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SMD_HIP_H_ */
