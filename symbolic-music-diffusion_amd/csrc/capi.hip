// extern "C" surface of libsmd_hip.so -- see include/smd_hip.h for the contract.
#include "../../include/smd_hip.h"
#include "../../include/smd_hip_lab.h"

#include <new>

#include "engine.h"

const char* smd_get_error();

struct smd_engine {
  SmdEngine impl;
  explicit smd_engine(const SmdModelDesc& d) : impl(d) {}
};

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
static inline const bf16_t* B(const smd_bf16* p) { return reinterpret_cast<const bf16_t*>(p); }
static inline bf16_t* B(smd_bf16* p) { return reinterpret_cast<bf16_t*>(p); }
// the LayerNorm-128 kernels move fp32 rows as float2: 8-byte aligned operands (nullptr passes; the launcher checks presence)
static inline bool al8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
// four partial tiles of `rows` x 128 floats, `part_stride` floats apart, read as float2: disjoint tiles, 8-byte aligned ones
#define PART_STRIDE_CHECK(fn, parts, part_stride, rows)                                                                       \
  SMD_ARG_CHECK((part_stride) >= (int64_t)(rows) * 128 && (part_stride) % 2 == 0 && al8(parts),                             \
                fn ": part_stride=%lld must be even and >= rows*128 = %lld, parts 8-byte aligned", (long long)(part_stride), \
                (long long)(rows) * 128)

#define NEED(e)                                        \
  do {                                                 \
    if (!(e)) {                                        \
      smd_set_error("%s: null engine handle", __func__); \
      return -1;                                       \
    }                                                  \
  } while (0)

extern "C" {

const char* smd_last_error(void) { return smd_get_error(); }
int smd_abi_version(void) { return SMD_ABI_VERSION; }

int smd_engine_create(const smd_model_desc* d, smd_engine** out) {
  SMD_ARG_CHECK(d && out, "smd_engine_create: null argument");
  SMD_ARG_CHECK(d->arch == 0 || d->arch == 1, "smd_engine_create: arch=%d (0 TransformerDDPM, 1 DenseDDPM)", d->arch);
  SMD_ARG_CHECK(d->data_channels > 0 && d->num_layers > 0 && d->mlp_dims > 0 && d->num_timesteps > 0,
                "smd_engine_create: non-positive dimension");
  SMD_ARG_CHECK(d->embed_channels == 128 && d->film_channels == 128,
                "smd_engine_create: embed/film channels are fixed at 128 (models/ncsn.py:151,174)");
  SMD_ARG_CHECK(d->mlp_dims % 256 == 0 && d->mlp_dims <= 4096, "smd_engine_create: mlp_dims=%d must be a multiple of 256 <= 4096", d->mlp_dims);
  if (d->arch == 0) {
    SMD_ARG_CHECK(d->seq_len == 32, "smd_engine_create: TransformerDDPM kernels are specialised for seq_len 32 (got %d)", d->seq_len);
    SMD_ARG_CHECK(d->num_heads > 0 && 128 % d->num_heads == 0 && (128 / d->num_heads == 8 || 128 / d->num_heads == 16 || 128 / d->num_heads == 32),
                  "smd_engine_create: num_heads=%d unsupported (4, 8, 16)", d->num_heads);
    SMD_ARG_CHECK(d->num_mlp_layers > 0, "smd_engine_create: num_mlp_layers must be positive");
  } else {
    SMD_ARG_CHECK(d->seq_len == 1, "smd_engine_create: DenseDDPM takes (B, C) inputs: seq_len must be 1");
  }
  SmdModelDesc m;
  m.arch = d->arch; m.data_channels = d->data_channels; m.seq_len = d->seq_len; m.num_layers = d->num_layers;
  m.num_heads = d->num_heads; m.num_mlp_layers = d->num_mlp_layers; m.mlp_dims = d->mlp_dims;
  m.embed_channels = d->embed_channels; m.film_channels = d->film_channels; m.num_timesteps = d->num_timesteps;
  smd_engine* e = new (std::nothrow) smd_engine(m);
  SMD_ARG_CHECK(e, "smd_engine_create: out of host memory");
  *out = e;
  return 0;
}
void smd_engine_destroy(smd_engine* e) { delete e; }

int smd_engine_num_tensors(const smd_engine* e) { return e ? (int)e->impl.tensors().size() : -1; }
int smd_engine_tensor_info(const smd_engine* e, int i, const char** name, int64_t* offset, int32_t* rows,
                           int32_t* cols) {
  NEED(e);
  SMD_ARG_CHECK(i >= 0 && i < (int)e->impl.tensors().size(), "tensor_info: index %d out of range", i);
  const TensorInfo& t = e->impl.tensors()[i];
  if (name) *name = t.name.c_str();
  if (offset) *offset = t.offset;
  if (rows) *rows = t.rows;
  if (cols) *cols = t.cols;
  return 0;
}
int64_t smd_engine_param_count(const smd_engine* e) { return e ? e->impl.param_count() : -1; }
int64_t smd_engine_head_param_offset(const smd_engine* e) { return e ? e->impl.head_param_offset() : -1; }
int64_t smd_engine_wpack_elems(const smd_engine* e) { return e ? e->impl.wpack_elems() : -1; }
int64_t smd_engine_workspace_bytes(const smd_engine* e, int batch, int training) {
  return (e && batch > 0) ? e->impl.workspace_bytes(batch, training) : -1;
}
int64_t smd_engine_film_table_floats(const smd_engine* e) { return e ? e->impl.film_table_floats() : -1; }
int smd_engine_padded_channels(const smd_engine* e) { return e ? e->impl.padded_channels() : -1; }
int smd_engine_set_option(smd_engine* e, const char* key, int value) {
  NEED(e);
  SMD_ARG_CHECK(key, "set_option: null key");
  if (std::string(key) == "tr_path") { e->impl.tr_path = value ? 1 : 0; return 0; }
  if (std::string(key) == "side_wgrad") return e->impl.set_side_stream(value);
  if (std::string(key) == "fused_attn_bwd") { e->impl.fused_attn_bwd = value < 0 ? 0 : (value > 2 ? 2 : value); return 0; }
  if (std::string(key) == "resgrad_bf16") { e->impl.resgrad_bf16 = value ? 1 : 0; return 0; }
  if (std::string(key) == "ln_saved_stats") { e->impl.ln_saved_stats = value ? 1 : 0; return 0; }
  if (std::string(key) == "film_side") { e->impl.film_side = value; return 0; }
  if (std::string(key) == "pair_wgrad") { e->impl.pair_wgrad = value ? 1 : 0; return 0; }
  if (std::string(key) == "wgrad256_group") { e->impl.wgrad256_group = value < 1 ? 1 : (value > 4 ? 4 : value); return 0; }
  if (std::string(key) == "group_wgrad") { e->impl.group_wgrad = value; return 0; }
  if (std::string(key) == "fused_encoder") { e->impl.fused_encoder = value; return 0; }
  if (std::string(key) == "trunk_bf16") { e->impl.trunk_bf16 = value; return 0; }
  if (std::string(key) == "sample_split") { e->impl.sample_split = value < 0 ? 0 : value; return 0; }
  if (std::string(key) == "nt256_min_tiles") { e->impl.nt256_min_tiles = value; return 0; }
  if (std::string(key) == "grad_memset") { e->impl.grad_memset = value; return 0; }
  if (std::string(key) == "tail_on_main") { e->impl.tail_on_main = value ? 1 : 0; return 0; }
  if (std::string(key) == "film_side_fwd") { e->impl.film_side_fwd = value ? 1 : 0; return 0; }
  if (std::string(key) == "loss_kind") {
    SMD_ARG_CHECK(!value || e->impl.prediction == 0, "set_option: loss_kind=1 (score matching) with prediction=%d: x0 / v "
                  "prediction is defined for the DDPM objective only", e->impl.prediction);
    e->impl.loss_kind = value ? 1 : 0;
    return 0;
  }
  if (std::string(key) == "prediction") {      // 0 eps, 1 x0, 2 v; settable at any time
    SMD_ARG_CHECK(value >= 0 && value <= 2, "set_option: prediction=%d (0 eps, 1 x0, 2 v)", value);
    SMD_ARG_CHECK(value == 0 || !e->impl.loss_kind, "set_option: prediction=%d with loss_kind=1 (score matching): x0 / v "
                  "prediction is defined for the DDPM objective only", value);
    e->impl.prediction = value;
    return 0;
  }
  if (std::string(key) == "label_min") { e->impl.label_min = value ? 1 : 0; return 0; }
  if (std::string(key) == "mlp_hs") { e->impl.mlp_hs = value ? 1 : 0; return 0; }
  if (std::string(key) == "fp8" || std::string(key) == "fp32") return e->impl.set_precision_option(key, value);
  if (std::string(key) == "fp8_dgrad") { e->impl.fp8_dgrad = value ? 1 : 0; return 0; }
  if (std::string(key) == "opt_overlap") { e->impl.opt_overlap = value & 3; return 0; }
  if (std::string(key) == "dp_layer_events") { e->impl.dp_layer_events = value ? 1 : 0; return 0; }
  if (std::string(key) == "opt_fused") { e->impl.set_opt_fused(value != 0); return 0; }     // 0: norm / update / re-cast as three passes (A/B)
  if (std::string(key) == "opt_side_blocks") { e->impl.opt_side_blocks = value < 0 ? 0 : value; return 0; }
  if (std::string(key) == "w8_dirty") { e->impl.mark_w8_dirty(); return 0; }   // the bf16 operand pack changed under another handle
  smd_set_error("set_option: unknown key '%s'", key);
  return -1;
}

int smd_engine_bind_params(smd_engine* e, float* params, smd_bf16* wpack) { NEED(e); return e->impl.bind_params(params, B(wpack)); }
int smd_engine_bind_train(smd_engine* e, float* grads, float* m, float* v, float* ema, uint32_t* step, float* metrics) {
  NEED(e);
  return e->impl.bind_train(grads, m, v, ema, step, metrics);
}
int smd_engine_bind_workspace(smd_engine* e, void* ws, int64_t bytes, int batch, int training, void* stream) {
  NEED(e);
  return e->impl.bind_workspace(ws, bytes, batch, training, S(stream));
}
int smd_engine_bind_schedule(smd_engine* e, const float* coef, const float* sqrt_ap, const float* ape, float* tables) {
  NEED(e);
  return e->impl.bind_schedule(coef, sqrt_ap, ape, tables);
}
int smd_engine_refresh_weights(smd_engine* e, void* stream) { NEED(e); return e->impl.refresh_weights(S(stream)); }
int smd_engine_forward(smd_engine* e, const float* x, const float* s, float* out, void* stream) {
  NEED(e);
  return e->impl.forward(x, s, out, S(stream));
}
int smd_engine_forward_level(smd_engine* e, const float* x, const int32_t* level_ptr, float* out, void* stream) {
  NEED(e);
  return e->impl.forward_level(x, level_ptr, out, S(stream));
}
int smd_engine_loss_backward(smd_engine* e, const float* x0, const int32_t* labels, const float* eps_in,
                             uint32_t seed_lo, uint32_t seed_hi, uint32_t sample_offset, float inv_global_count,
                             int stage, void* stream) {
  NEED(e);
  return e->impl.loss_backward(x0, labels, eps_in, seed_lo, seed_hi, sample_offset, inv_global_count, stage, S(stream));
}
int smd_engine_forward_train(smd_engine* e, const float* x, const float* noise_level, float* eps_out, void* stream) {
  NEED(e);
  return e->impl.forward_train(x, noise_level, eps_out, S(stream));
}
int smd_engine_backward_from(smd_engine* e, const float* dpred, int stage, void* stream) {
  NEED(e);
  return e->impl.backward_from(dpred, stage, S(stream));
}
int smd_engine_set_used_alphas(smd_engine* e, const float* used_alphas) {
  NEED(e);
  e->impl.set_used_alphas(used_alphas);
  return 0;
}
int smd_engine_set_loss_weights(smd_engine* e, const float* iw, float min_snr_gamma) {
  NEED(e);
  SMD_ARG_CHECK(!(min_snr_gamma != min_snr_gamma), "smd_engine_set_loss_weights: min_snr_gamma is NaN");
  e->impl.set_loss_weights(iw, min_snr_gamma);
  return 0;
}
const float* smd_engine_weight_per_sample(const smd_engine* e) { return e ? e->impl.weight_per_sample() : nullptr; }
const float* smd_engine_noise_level_per_sample(const smd_engine* e) { return e ? e->impl.noise_levels() : nullptr; }
int64_t smd_engine_debug_snapshot_bytes(const smd_engine* e) { return e ? e->impl.debug_snapshot_bytes() : -1; }
int smd_engine_debug_snapshots(smd_engine* e, void* buf, int64_t bytes) {
  NEED(e);
  return e->impl.set_debug_snapshots(buf, bytes);
}
int smd_engine_debug_tensor(const smd_engine* e, const char* name, int index, const void** ptr, int64_t* rows, int64_t* cols,
                            int32_t* dtype) {
  NEED(e);
  int dt = 0;
  const int rc = e->impl.debug_tensor(name, index, ptr, rows, cols, &dt);
  if (rc == 0 && dtype) *dtype = dt;
  return rc;
}
const float* smd_engine_loss_per_sample(const smd_engine* e) { return e ? e->impl.loss_per_sample() : nullptr; }
const float* smd_engine_pred(const smd_engine* e) { return e ? e->impl.pred() : nullptr; }

int smd_engine_num_grad_buckets(const smd_engine* e) { return e ? e->impl.num_grad_buckets() : -1; }
int smd_engine_grad_bucket(const smd_engine* e, int bucket, int64_t* offset, int64_t* length) {
  NEED(e);
  return e->impl.grad_bucket(bucket, offset, length);
}
int smd_engine_wait_grad_bucket(smd_engine* e, int bucket, void* stream) { NEED(e); return e->impl.wait_grad_bucket(bucket, S(stream)); }
int smd_engine_join_update(smd_engine* e, void* stream) { NEED(e); return e->impl.join_update(S(stream)); }
int smd_engine_optimizer_step(smd_engine* e, const smd_train_hyper* h, void* stream) {
  NEED(e);
  SMD_ARG_CHECK(h, "optimizer_step: null hyper-parameters");
  TrainHyper t;
  t.lr0 = h->lr0; t.lr_gamma = h->lr_gamma; t.lr_interval = h->lr_interval; t.beta1 = h->beta1; t.beta2 = h->beta2;
  t.eps = h->eps; t.grad_clip = h->grad_clip; t.mu = h->mu; t.grad_scale = h->grad_scale;
  return e->impl.optimizer_step(t, S(stream));
}
int smd_engine_prepare_sampler(smd_engine* e, void* stream) { NEED(e); return e->impl.prepare_sampler(S(stream)); }
int smd_engine_init_state(smd_engine* e, float* x, uint32_t lo, uint32_t hi, uint32_t off, void* stream) {
  NEED(e);
  return e->impl.init_state(x, lo, hi, off, S(stream));
}
int smd_engine_load_state(smd_engine* e, const float* x, void* stream) {
  NEED(e);
  return e->impl.load_state(x, S(stream));
}
static SampleStepIO sample_io(const smd_sample_io* io) {
  SampleStepIO s;
  s.x = io->x; s.t_ptr = io->t_ptr; s.z_in = io->z_in; s.seed_lo = io->seed_lo; s.seed_hi = io->seed_hi;
  s.sample_offset = io->sample_offset; s.infill_samples = io->infill_samples; s.infill_masks = io->infill_masks;
  s.infill_z_in = io->infill_z_in; s.metrics_partial = io->metrics_partial; s.collection = io->collection;
  s.slot_table = io->slot_table;
  s.tf_noise_keys = io->tf_noise_keys; s.tf_infill_keys = io->tf_infill_keys; s.tf_n_total = io->tf_n_total; s.tf_t0 = io->tf_t0;
  s.key_ptr = io->key_ptr;
  return s;
}
static int sample_step_part(smd_engine* e, const smd_sample_io* io, int part, void* stream) {
  NEED(e);
  SMD_ARG_CHECK(io, "sample_step: null io");
  return e->impl.sample_step(sample_io(io), S(stream), part);
}
int smd_engine_sample_step(smd_engine* e, const smd_sample_io* io, void* stream) { return sample_step_part(e, io, 0, stream); }
int smd_engine_sample_step_part(smd_engine* e, const smd_sample_io* io, int part, void* stream) {
  SMD_ARG_CHECK(part == 1 || part == 2, "smd_engine_sample_step_part: part=%d (1 stem, 2 output stage + reverse update)", part);
  return sample_step_part(e, io, part, stream);
}
int smd_engine_strided_step(smd_engine* e, const smd_sample_io* io, const smd_stride_plan* plan, int part, void* stream) {
  NEED(e);
  SMD_ARG_CHECK(io && plan, "strided_step: null io / plan");
  StridePlan p;
  p.coef = plan->coef; p.plan = plan->plan; p.T = plan->T;
  return e->impl.strided_step(sample_io(io), p, S(stream), part);
}
int smd_engine_multistep_step(smd_engine* e, const smd_sample_io* io, const smd_multistep_plan* plan, float* x0_prev, int part,
                              void* stream) {
  NEED(e);
  SMD_ARG_CHECK(io && plan, "multistep_step: null io / plan");
  MultistepPlan p;
  p.coef = plan->coef; p.plan = plan->plan; p.T = plan->T;
  return e->impl.multistep_step(sample_io(io), p, x0_prev, S(stream), part);
}
int smd_engine_adams_step(smd_engine* e, const smd_sample_io* io, const smd_multistep_plan* plan, float* hist, int part, void* stream) {
  NEED(e);
  SMD_ARG_CHECK(io && plan, "adams_step: null io / plan");
  MultistepPlan p;
  p.coef = plan->coef; p.plan = plan->plan; p.T = plan->T;
  return e->impl.adams_step(sample_io(io), p, hist, S(stream), part);
}
int smd_engine_bound_step(smd_engine* e, const smd_bound_io* io, void* stream) {
  NEED(e);
  SMD_ARG_CHECK(io, "bound_step: null io");
  BoundStepIO b;
  b.x0 = io->x0; b.x_t = io->x_t; b.eps = io->eps; b.t_ptr = io->t_ptr; b.table = io->table; b.next_t = io->next_t; b.T = io->T;
  b.clip = io->clip; b.eps_source = io->eps_source; b.seed_lo = io->seed_lo; b.seed_hi = io->seed_hi;
  b.sample_offset = io->sample_offset; b.key_ptr = io->key_ptr; b.tf_keys = io->tf_keys; b.tf_n_total = io->tf_n_total;
  b.partial = io->partial;
  return e->impl.bound_step(b, S(stream));
}
int smd_engine_moment_step(smd_engine* e, const smd_moment_io* io, void* stream) {
  NEED(e);
  SMD_ARG_CHECK(io, "moment_step: null io");
  MomentStepIO m;
  m.x0 = io->x0; m.x_t = io->x_t; m.eps = io->eps; m.t_ptr = io->t_ptr; m.noise_table = io->noise_table;
  m.moment_table = io->moment_table; m.next_t = io->next_t; m.T = io->T; m.eps_source = io->eps_source; m.seed_lo = io->seed_lo;
  m.seed_hi = io->seed_hi; m.sample_offset = io->sample_offset; m.key_ptr = io->key_ptr; m.tf_keys = io->tf_keys;
  m.tf_n_total = io->tf_n_total; m.partial = io->partial; m.sums = io->sums;
  return e->impl.moment_step(m, S(stream));
}
int smd_engine_analytic_step(smd_engine* e, const smd_sample_io* io, const smd_stride_plan* plan, const smd_sigma_table* sig, int part,
                             void* stream) {
  NEED(e);
  SMD_ARG_CHECK(io && plan && sig, "analytic_step: null io / plan / sig");
  StridePlan p;
  p.coef = plan->coef; p.plan = plan->plan; p.T = plan->T;
  return e->impl.analytic_step(sample_io(io), p, sig->sig, sig->K, S(stream), part);
}
int smd_score_moments(const float* x_t, const float* out, int B, int S_, int C, const float* table, int T, int32_t* t_ptr,
                      const int32_t* next_t, uint32_t* arrive, float* partial, float* sums, void* stream) {
  ScoreMomentsArgs a;
  a.x_t = x_t; a.out = out; a.B = B; a.S = S_; a.C = C; a.T = T; a.table = table; a.t_ptr = t_ptr; a.next_t = next_t;
  a.arrive = arrive; a.partial = partial; a.sums = sums;
  return launch_score_moments(a, S(stream));
}

// ------------------------------------------------------------------ single kernels
int smd_set_tuning(const char* key, int value) { return smd_tuning_set(key, value); }
int smd_gemm_bf16_nt(const smd_bf16* A, int lda, const smd_bf16* Bt, int ldb, int M, int N, int K, const float* bias,
                     int act, const float* residual, int ld_res, float* out_f32, int ld_out, smd_bf16* out_bf16,
                     int ld_outb, void* stream) {
  GemmEpilogue ep;
  ep.bias = bias; ep.act = act; ep.res_f32 = residual; ep.ld_res = ld_res;
  ep.out_f32 = out_f32; ep.ld_out = ld_out; ep.out_bf16 = B(out_bf16); ep.ld_outb = ld_outb;
  return launch_gemm_nt(B(A), lda, B(Bt), ldb, M, N, K, ep, S(stream));
}
int smd_quantize_rows_e4m3(const smd_bf16* in, int ld, int rows, int K, uint8_t* out8, uint32_t* scale, void* stream) {
  return launch_quantize_rows_e4m3(B(in), ld, rows, K, out8, scale, S(stream));
}
int smd_gemm_e4m3_nt(const uint8_t* A8, int lda, const uint32_t* scale_a, const uint8_t* Bt8, int ldb, const uint32_t* scale_b, int M,
                     int N, int K, const float* bias, const float* residual, int ld_res, float* out_f32, int ld_out,
                     smd_bf16* out_bf16, int ld_outb, void* stream) {
  GemmEpilogue ep;
  ep.bias = bias; ep.res_f32 = residual; ep.ld_res = ld_res; ep.out_f32 = out_f32; ep.ld_out = ld_out; ep.out_bf16 = B(out_bf16);
  ep.ld_outb = ld_outb;
  return launch_gemm_nt256_fp8(A8, lda, scale_a, Bt8, ldb, scale_b, M, N, K, ep, S(stream));
}
int smd_layernorm_fwd_e4m3(const float* x, int rows, int D, const float* gamma, const float* beta, const float* film_scale,
                           const float* film_shift, int ld_film, int rows_per_sample, int swish, uint8_t* out8, uint32_t* out_scale,
                           smd_bf16* out_bf16, void* stream) {
  LnArgs a;
  a.x = x; a.rows = rows; a.D = D; a.gamma = gamma; a.beta = beta; a.film_scale = film_scale; a.film_shift = film_shift;
  a.ld_film = ld_film; a.rows_per_sample = rows_per_sample > 0 ? rows_per_sample : 1; a.swish = swish; a.out = B(out_bf16);
  a.out_f8 = out8; a.out_scale = out_scale;
  return launch_layernorm_fwd(a, S(stream));
}
int smd_mlp_block_fwd(const float* h_in, float* h_out, int rows, const float* gamma, const float* beta, const smd_bf16* W1t,
                      const float* b1, const smd_bf16* W2t, const float* b2, int hidden, smd_bf16* save_a2, smd_bf16* save_z1,
                      smd_bf16* save_u, void* stream) {
  return launch_mlp_block_fwd(h_in, h_out, rows, gamma, beta, B(W1t), b1, B(W2t), b2, hidden, B(save_a2), B(save_z1), B(save_u),
                              S(stream));
}
int smd_mlp_block_fwd_hs(const smd_bf16* a2, const float* h_res, int rows, const smd_bf16* W1t, const float* b1,
                         const smd_bf16* W2t, const float* b2, int hidden, float* part, void* stream) {
  return launch_mlp_block_fwd_hs(B(a2), h_res, rows, B(W1t), b1, B(W2t), b2, hidden, part, S(stream));
}
int smd_mlp_block_bwd_hs(const smd_bf16* a2, const smd_bf16* dh, int rows, const smd_bf16* W1t, const smd_bf16* W2, const smd_bf16* W1,
                         const float* b1, int hidden, smd_bf16* u, smd_bf16* dz, float* part, void* stream) {
  return launch_mlp_block_bwd_hs(B(a2), B(dh), rows, B(W1t), B(W2), B(W1), b1, hidden, B(u), B(dz), part, S(stream));
}
int smd_ln128_bwd_parts(const float* x, const float* parts, int64_t part_stride, int rows, const float* gamma, const float* dres,
                        float* dx_f32, smd_bf16* dx_bf16, float* partial, void* stream) {
  PART_STRIDE_CHECK("smd_ln128_bwd_parts", parts, part_stride, rows);
  SMD_ARG_CHECK(al8(x) && al8(gamma) && al8(dres) && al8(dx_f32), "smd_ln128_bwd_parts: x, gamma, dres, dx_f32 must be 8-byte aligned");
  return launch_ln128_bwd_parts(x, parts, (size_t)part_stride, rows, gamma, dres, dx_f32, B(dx_bf16), partial, S(stream));
}
int smd_ln128_parts(const float* parts, int64_t part_stride, int rows, const float* gamma, const float* beta, float* x_out,
                    smd_bf16* ln_out, void* stream) {
  PART_STRIDE_CHECK("smd_ln128_parts", parts, part_stride, rows);
  SMD_ARG_CHECK(al8(gamma) && al8(beta) && al8(x_out), "smd_ln128_parts: gamma, beta, x_out must be 8-byte aligned");
  return launch_ln128_parts(parts, (size_t)part_stride, rows, gamma, beta, x_out, B(ln_out), S(stream));
}
int smd_attn_block_fwd_ex(const float* h_in, const float* h_parts, int64_t part_stride, float* h_comb, float* h_out, int rows,
                          const float* gamma, const float* beta, const smd_bf16* Wqkv_t, const float* b_qkv,
                          const smd_bf16* Wo_t, const float* b_o, int num_heads, const float* gamma2, const float* beta2,
                          smd_bf16* a2_out, smd_bf16* save_a1, smd_bf16* save_qkv, smd_bf16* save_o, void* stream) {
  if (h_parts) PART_STRIDE_CHECK("smd_attn_block_fwd_ex", h_parts, part_stride, rows);
  SMD_ARG_CHECK(al8(h_in) && al8(h_comb) && al8(gamma) && al8(beta) && al8(gamma2) && al8(beta2),
                "smd_attn_block_fwd_ex: h_in, h_comb, gamma, beta, gamma2, beta2 must be 8-byte aligned");
  AttnBlockExtra ex;
  ex.h_parts = h_parts; ex.part_stride = (size_t)part_stride; ex.h_comb = h_comb; ex.gamma2 = gamma2; ex.beta2 = beta2;
  ex.a2_out = B(a2_out);
  return launch_attn_block_fwd(h_in, h_out, rows, gamma, beta, B(Wqkv_t), b_qkv, B(Wo_t), b_o, num_heads, B(save_a1), B(save_qkv),
                               B(save_o), S(stream), &ex);
}
int smd_attn_block_fwd(const float* h_in, float* h_out, int rows, const float* gamma, const float* beta, const smd_bf16* Wqkv_t,
                       const float* b_qkv, const smd_bf16* Wo_t, const float* b_o, int num_heads, smd_bf16* save_a1,
                       smd_bf16* save_qkv, smd_bf16* save_o, void* stream) {
  return launch_attn_block_fwd(h_in, h_out, rows, gamma, beta, B(Wqkv_t), b_qkv, B(Wo_t), b_o, num_heads, B(save_a1), B(save_qkv),
                               B(save_o), S(stream));
}
int smd_attn_block_bwd(const smd_bf16* dh_mid, const smd_bf16* qkv, const smd_bf16* Wo, const smd_bf16* Wqkv, smd_bf16* dqkv,
                       smd_bf16* da1, int rows, int num_heads, void* stream) {
  return launch_attn_block_bwd(B(dh_mid), B(qkv), B(Wo), B(Wqkv), B(dqkv), B(da1), rows, num_heads, S(stream));
}
int smd_attn_block_bwd_ln(const smd_bf16* qkv, const smd_bf16* Wo, const smd_bf16* Wqkv, smd_bf16* dqkv, smd_bf16* da1,
                          const float* h_mid, const float* da2_parts, int64_t part_stride, const float* gamma2, float* dh,
                          smd_bf16* dh_mid_out, float* partial2, const float* h, const float* gamma1, smd_bf16* dh_out,
                          float* partial1, int rows, int num_heads, void* stream) {
  PART_STRIDE_CHECK("smd_attn_block_bwd_ln", da2_parts, part_stride, rows);
  SMD_ARG_CHECK(al8(h_mid) && al8(gamma2) && al8(dh) && al8(h) && al8(gamma1),
                "smd_attn_block_bwd_ln: h_mid, gamma2, dh, h, gamma1 must be 8-byte aligned");
  AttnBwdLnArgs a;
  a.qkv = B(qkv); a.Wo = B(Wo); a.Wqkv = B(Wqkv); a.dqkv = B(dqkv); a.da1 = B(da1);
  a.h_mid = h_mid; a.da2_parts = da2_parts; a.part_stride = (size_t)part_stride; a.gamma2 = gamma2; a.dh = dh;
  a.dh_mid_out = B(dh_mid_out); a.partial2 = partial2; a.h = h; a.gamma1 = gamma1; a.dh_out = B(dh_out); a.partial1 = partial1;
  return launch_attn_block_bwd_ln(a, rows, num_heads, S(stream));
}
int smd_gemm_bf16_tn(const smd_bf16* X, int ldx, const smd_bf16* dY, int ldy, int M, int Kd, int N, float* out, int ldo,
                     float* bias_out, const smd_bf16* zero_page, float* slab, int64_t slab_elems, smd_bf16* scratch,
                     int64_t scratch_elems, int tr_path, void* stream) {
  TnLaunch t;
  t.X = B(X); t.ldx = ldx; t.dY = B(dY); t.ldy = ldy; t.Mrows = M; t.Kd = Kd; t.N = N; t.out = out; t.ldo = ldo;
  t.bias_out = bias_out; t.zero_page = B(zero_page); t.slab = slab; t.slab_elems = (size_t)slab_elems;
  t.scratch = B(scratch); t.scratch_elems = (size_t)scratch_elems; t.tr_path = tr_path;
  return launch_gemm_tn(t, S(stream));
}
int64_t smd_gemm_tn_slab_elems(void) { return (int64_t)gemm_tn_slab_elems(); }
int smd_layernorm_fwd(const float* x, int rows, int D, const float* gamma, const float* beta, const float* film_scale,
                      const float* film_shift, int ld_film, int rows_per_sample, int swish, smd_bf16* out, void* stream) {
  LnArgs a;
  a.x = x; a.rows = rows; a.D = D; a.gamma = gamma; a.beta = beta; a.film_scale = film_scale; a.film_shift = film_shift;
  a.ld_film = ld_film; a.rows_per_sample = rows_per_sample > 0 ? rows_per_sample : 1; a.swish = swish; a.out = B(out);
  return launch_layernorm_fwd(a, S(stream));
}
int smd_layernorm_fwd_ex(const float* x, const smd_bf16* x_bf16, int rows, int D, const float* gamma, const float* beta,
                         const float* film_scale, const float* film_shift, int ld_film, int rows_per_sample, int swish, smd_bf16* out,
                         void* stream) {
  LnArgs a;
  a.x = x; a.x_bf16 = B(x_bf16); a.rows = rows; a.D = D; a.gamma = gamma; a.beta = beta; a.film_scale = film_scale;
  a.film_shift = film_shift; a.ld_film = ld_film; a.rows_per_sample = rows_per_sample > 0 ? rows_per_sample : 1; a.swish = swish;
  a.out = B(out);
  return launch_layernorm_fwd(a, S(stream));
}
int smd_layernorm_bwd(const float* x, int rows, int D, const float* gamma, const float* beta, const float* film_scale,
                      const float* film_shift, int ld_film, int rows_per_sample, int swish, const smd_bf16* dout,
                      float* dx, float* dgamma, float* dbeta, float* dscale, float* dshift, float* partial,
                      int64_t partial_elems, void* stream) {
  LnBwdArgs b;
  b.f.x = x; b.f.rows = rows; b.f.D = D; b.f.gamma = gamma; b.f.beta = beta; b.f.film_scale = film_scale;
  b.f.film_shift = film_shift; b.f.ld_film = ld_film; b.f.rows_per_sample = rows_per_sample > 0 ? rows_per_sample : 1;
  b.f.swish = swish;
  b.dout = B(dout); b.dx = dx; b.dgamma = dgamma; b.dbeta = dbeta; b.dscale = dscale; b.dshift = dshift;
  b.partial = partial; b.partial_elems = (size_t)partial_elems;
  return launch_layernorm_bwd(b, S(stream));
}
int smd_layernorm_bwd_ex(const float* x, const smd_bf16* x_bf16, int rows, int D, const float* gamma, const float* beta,
                         const smd_bf16* dout, const float* dres, float* dx, smd_bf16* dx_bf16, float* dgamma, float* dbeta,
                         float* partial, int64_t partial_elems, void* stream) {
  LnBwdArgs b;
  b.f.x = x; b.f.x_bf16 = B(x_bf16); b.f.rows = rows; b.f.D = D; b.f.gamma = gamma; b.f.beta = beta;
  b.dout = B(dout); b.dres = dres; b.dx = dx; b.dx_bf16 = B(dx_bf16); b.dgamma = dgamma; b.dbeta = dbeta;
  b.partial = partial; b.partial_elems = (size_t)partial_elems;
  return launch_layernorm_bwd(b, S(stream));
}
int smd_layernorm_bwd_film(const float* x, const smd_bf16* x_bf16, int rows, int D, const float* gamma, const float* beta,
                           const float* film_scale, const float* film_shift, int ld_film, int rows_per_sample, int swish,
                           const smd_bf16* dout, const float* dres, const smd_bf16* dres_bf16, float* dx,
                           smd_bf16* dx_bf16, float* dgamma, float* dbeta, float* dscale, float* dshift,
                           int dfilm_accumulate, float* partial, int64_t partial_elems, void* stream) {
  LnBwdArgs b;
  b.f.x = x; b.f.x_bf16 = B(x_bf16); b.f.rows = rows; b.f.D = D; b.f.gamma = gamma; b.f.beta = beta;
  b.f.film_scale = film_scale; b.f.film_shift = film_shift; b.f.ld_film = ld_film; b.f.rows_per_sample = rows_per_sample;
  b.f.swish = swish;
  b.dout = B(dout); b.dres = dres; b.dres_bf16 = B(dres_bf16); b.dx = dx; b.dx_bf16 = B(dx_bf16);
  b.dgamma = dgamma; b.dbeta = dbeta; b.dscale = dscale; b.dshift = dshift; b.dfilm_accumulate = dfilm_accumulate;
  b.partial = partial; b.partial_elems = (size_t)partial_elems;
  return launch_layernorm_bwd(b, S(stream));
}
int smd_layernorm_fwd_stats(const float* x, const smd_bf16* x_bf16, int rows, int D, const float* gamma, const float* beta,
                            const float* film_scale, const float* film_shift, int ld_film, int rows_per_sample, int swish,
                            smd_bf16* out, uint8_t* out8, uint32_t* out_scale, float* stats_out, void* stream) {
  LnArgs a;
  a.x = x; a.x_bf16 = B(x_bf16); a.rows = rows; a.D = D; a.gamma = gamma; a.beta = beta; a.film_scale = film_scale;
  a.film_shift = film_shift; a.ld_film = ld_film; a.rows_per_sample = rows_per_sample > 0 ? rows_per_sample : 1; a.swish = swish;
  a.out = B(out); a.out_f8 = out8; a.out_scale = out_scale; a.stats_out = stats_out;
  return launch_layernorm_fwd(a, S(stream));
}
int smd_layernorm_fwd_lab(const float* x, const smd_bf16* x_bf16, int rows, int D, const float* gamma, const float* beta,
                          const float* film_scale, const float* film_shift, int ld_film, int rows_per_sample, int swish,
                          smd_bf16* out, uint8_t* out8, uint32_t* out_scale, float* stats_out, const int32_t* t_ptr, int film_rows,
                          void* stream) {
  LnArgs a;
  a.x = x; a.x_bf16 = B(x_bf16); a.rows = rows; a.D = D; a.gamma = gamma; a.beta = beta; a.film_scale = film_scale;
  a.film_shift = film_shift; a.ld_film = ld_film; a.rows_per_sample = rows_per_sample; a.swish = swish;
  a.out = B(out); a.out_f8 = out8; a.out_scale = out_scale; a.stats_out = stats_out; a.t_ptr = t_ptr; a.film_rows = film_rows;
  return launch_layernorm_fwd(a, S(stream));
}
int smd_layernorm_bwd_stats(const float* x, const smd_bf16* x_bf16, int rows, int D, const float* gamma, const float* beta,
                            const float* film_scale, const float* film_shift, int ld_film, int rows_per_sample, int swish,
                            const smd_bf16* dout, const float* dres, const smd_bf16* dres_bf16, float* dx,
                            smd_bf16* dx_bf16, float* dgamma, float* dbeta, float* dscale, float* dshift,
                            int dfilm_accumulate, float* partial, int64_t partial_elems, const float* stats, void* stream) {
  LnBwdArgs b;
  b.f.x = x; b.f.x_bf16 = B(x_bf16); b.f.rows = rows; b.f.D = D; b.f.gamma = gamma; b.f.beta = beta;
  b.f.film_scale = film_scale; b.f.film_shift = film_shift; b.f.ld_film = ld_film; b.f.rows_per_sample = rows_per_sample;
  b.f.swish = swish;
  b.dout = B(dout); b.dres = dres; b.dres_bf16 = B(dres_bf16); b.dx = dx; b.dx_bf16 = B(dx_bf16);
  b.dgamma = dgamma; b.dbeta = dbeta; b.dscale = dscale; b.dshift = dshift; b.dfilm_accumulate = dfilm_accumulate;
  b.partial = partial; b.partial_elems = (size_t)partial_elems; b.stats = stats;
  return launch_layernorm_bwd(b, S(stream));
}
int smd_attention_fwd(const smd_bf16* qkv, smd_bf16* out, int Bn, int Sn, int E, int H, void* stream) {
  return launch_attention_fwd(B(qkv), B(out), Bn, Sn, E, H, S(stream));
}
int smd_attention_bwd(const smd_bf16* qkv, const smd_bf16* dout, smd_bf16* dqkv, int Bn, int Sn, int E, int H, void* stream) {
  return launch_attention_bwd(B(qkv), B(dout), B(dqkv), Bn, Sn, E, H, S(stream));
}
int smd_noise_embed(const float* s, int n, int channels, smd_bf16* out, int ld_out, void* stream) {
  return launch_noise_embed(s, n, channels, B(out), ld_out, S(stream));
}
int smd_q_sample(const float* x0, int Bn, int Sn, int C, int Cp, int T, const float* alphas_prod_ext, const int32_t* labels,
                 int label_min, const float* used_alphas, const float* eps_in, uint32_t seed_lo, uint32_t seed_hi,
                 const uint32_t* step_ptr, uint32_t sample_offset, smd_bf16* xt_bf16, float* eps_out, float* noise_level_out,
                 void* stream) {
  QSampleArgs q;
  q.x0 = x0; q.B = Bn; q.S = Sn; q.C = C; q.Cp = Cp; q.T = T; q.alphas_prod_ext = alphas_prod_ext;
  q.labels = labels; q.label_min = label_min; q.alpha_in = used_alphas; q.eps_in = eps_in;
  q.key = RngKey{seed_lo, seed_hi}; q.step_ptr = step_ptr; q.sample_offset = sample_offset;
  q.xt_bf16 = B(xt_bf16); q.eps_out = eps_out; q.s_out = noise_level_out;
  return launch_q_sample(q, S(stream));
}
int smd_mse_fwd_bwd(const float* pred, const float* eps, int Bn, int Sn, int C, int Cp, float inv_global_count,
                    float* loss_per_sample, smd_bf16* dpred_bf16, void* stream) {
  return launch_mse_loss_grad(pred, eps, Bn, Sn, C, Cp, inv_global_count, loss_per_sample, B(dpred_bf16), S(stream));
}
int smd_adam_clip_ema(float* params, const float* grads, float* m, float* v, float* ema, int64_t n, const smd_train_hyper* h,
                      uint32_t* step_ptr, float* norm_partial, float* metrics_out, void* stream) {
  SMD_ARG_CHECK(h && n > 0, "adam_clip_ema: bad arguments");
  AdamArgs a;
  a.params = params; a.grads = grads; a.m = m; a.v = v; a.ema = ema; a.n = (size_t)n;
  a.lr0 = h->lr0; a.lr_gamma = h->lr_gamma; a.lr_interval = h->lr_interval; a.beta1 = h->beta1; a.beta2 = h->beta2;
  a.eps = h->eps; a.grad_clip = h->grad_clip; a.mu = h->mu; a.grad_scale = h->grad_scale;
  a.step_ptr = step_ptr; a.norm_partial = norm_partial; a.metrics_out = metrics_out;
  int rc = launch_grad_sumsq(a, S(stream));
  return rc ? rc : launch_adam_clip_ema(a, S(stream));
}
int smd_set_timestep(int32_t* t_ptr, int32_t t, void* stream) { return launch_set_t(t_ptr, t, S(stream)); }
int smd_langevin_step(const smd_langevin_io* io, int Bn, int Sn, int C, void* stream) {
  SMD_ARG_CHECK(io, "langevin_step: null io");
  LangevinStepArgs a;
  a.x = io->x; a.grad = io->grad; a.B = Bn; a.S = Sn; a.C = C; a.alpha = io->alpha; a.noise_coef = io->noise_coef;
  a.z_in = io->z_in; a.key = RngKey{io->seed_lo, io->seed_hi}; a.step = io->step; a.sample_offset = io->sample_offset;
  a.use_threefry = io->use_threefry;
  a.tf_noise_key[0] = io->tf_noise_key[0]; a.tf_noise_key[1] = io->tf_noise_key[1];
  a.tf_infill_key[0] = io->tf_infill_key[0]; a.tf_infill_key[1] = io->tf_infill_key[1];
  a.tf_n_total = io->tf_n_total;
  a.infill_samples = io->infill_samples; a.infill_masks = io->infill_masks; a.infill_z_in = io->infill_z_in;
  a.infill_sigma = io->infill_sigma; a.metrics_partial = io->metrics_partial; a.collect_out = io->collect_out;
  a.step_table = io->step_table; a.slot_table = io->slot_table; a.key_table = io->key_table; a.k_ptr = io->k_ptr;
  a.arrive = io->arrive; a.collection = io->collection; a.sigma_out = io->sigma_out; a.n_steps = io->n_steps;
  a.level_out = io->level_out; a.steps_per_level = io->steps_per_level; a.n_levels = io->n_levels;
  return launch_langevin_step(a, S(stream));
}
int smd_rng_normal(float* out, int Bn, int per_sample, uint32_t lo, uint32_t hi, uint32_t stream_id, uint32_t off, void* stream) {
  return launch_fill_normal(out, Bn, per_sample, RngKey{lo, hi}, stream_id, off, S(stream));
}
int smd_threefry_bits(uint32_t* out, int64_t n_total, int64_t offset, int64_t count, uint32_t k0, uint32_t k1, void* stream) {
  return launch_threefry_bits(out, n_total, offset, count, k0, k1, S(stream));
}
int smd_threefry_uniform(float* out, int64_t n_total, int64_t offset, int64_t count, uint32_t k0, uint32_t k1, float minval,
                         float maxval, void* stream) {
  return launch_threefry_uniform(out, n_total, offset, count, k0, k1, minval, maxval, S(stream));
}
int smd_threefry_normal(float* out, int64_t n_total, int64_t offset, int64_t count, uint32_t k0, uint32_t k1,
                        const uint32_t* key_table, const int32_t* idx_ptr, int idx_mul, int idx_add, void* stream) {
  return launch_threefry_normal(out, n_total, offset, count, k0, k1, key_table, idx_ptr, idx_mul, idx_add, S(stream));
}
int smd_threefry_randint(int32_t* out, int64_t n_total, int64_t offset, int64_t count, uint32_t k0, uint32_t k1,
                         int32_t minval, int32_t maxval, void* stream) {
  return launch_threefry_randint(out, n_total, offset, count, k0, k1, minval, maxval, S(stream));
}
int smd_cast_pad_bf16(const float* in, int rows, int cols, smd_bf16* out, int ld_out, void* stream) {
  return launch_cast_pad_bf16(in, rows, cols, B(out), ld_out, S(stream));
}
int smd_ddpm_reverse_step(float* x, const float* eps_hat, int Bn, int Sn, int C, const float* coef, int T, const int32_t* t_ptr,
                          const float* z_in, uint32_t lo, uint32_t hi, uint32_t off, float* metrics_partial,
                          float* collection, const int32_t* slot_table, void* stream) {
  ReverseStepArgs a;
  a.x = x; a.eps_hat = eps_hat; a.B = Bn; a.S = Sn; a.C = C; a.Cp = C; a.coef = coef; a.T = T; a.t_ptr = t_ptr; a.z_in = z_in;
  a.key = RngKey{lo, hi}; a.sample_offset = off; a.metrics_partial = metrics_partial; a.collection = collection;
  a.slot_table = slot_table;
  return launch_reverse_step(a, S(stream));
}

int smd_bound_noise(const float* x0, int Bn, int Sn, int C, int Cp, const float* table, int T, const int32_t* t_ptr, float* eps,
                    int draw, uint32_t lo, uint32_t hi, const uint32_t* key_ptr, uint32_t off, float* x_t, smd_bf16* xt_bf16,
                    void* stream) {
  BoundNoiseArgs a;
  a.x0 = x0; a.eps = eps; a.draw = draw ? 1 : 0; a.B = Bn; a.S = Sn; a.C = C; a.Cp = Cp; a.T = T; a.table = table; a.t_ptr = t_ptr;
  a.key = RngKey{lo, hi}; a.key_ptr = key_ptr; a.sample_offset = off; a.x_t = x_t; a.xt_bf16 = B(xt_bf16);
  return launch_bound_noise(a, S(stream));
}
int smd_bound_terms(const float* x0, const float* eps, const float* eps_hat, int Bn, int Sn, int C, const float* table, int T,
                    float clip, int32_t* t_ptr, const int32_t* next_t, uint32_t* arrive, float* partial, void* stream) {
  BoundTermsArgs a;
  a.x0 = x0; a.eps = eps; a.eps_hat = eps_hat; a.B = Bn; a.S = Sn; a.C = C; a.T = T; a.table = table; a.clip = clip;
  a.t_ptr = t_ptr; a.next_t = next_t; a.arrive = arrive; a.partial = partial;
  return launch_bound_terms(a, S(stream));
}

int smd_distill_noise(const float* x0, int Bn, int Sn, int C, const float* table, int N, const int32_t* steps, float* eps, int draw,
                      uint32_t lo, uint32_t hi, uint32_t off, uint32_t step, const uint32_t* step_ptr, float* z_t, float* level_out,
                      void* stream) {
  DistillNoiseArgs a;
  a.x0 = x0; a.eps = eps; a.draw = draw ? 1 : 0; a.B = Bn; a.S = Sn; a.C = C; a.N = N; a.table = table; a.steps = steps;
  a.key = RngKey{lo, hi}; a.sample_offset = off; a.step = step; a.step_ptr = step_ptr; a.z_t = z_t; a.level_out = level_out;
  return launch_distill_noise(a, S(stream));
}
int smd_distill_mid(const float* z_t, const float* out1, int Bn, int Sn, int C, const float* table, int N, const int32_t* steps,
                    float* x1, float* z_m, float* level_out, void* stream) {
  DistillMidArgs a;
  a.z_t = z_t; a.out1 = out1; a.B = Bn; a.S = Sn; a.C = C; a.N = N; a.table = table; a.steps = steps; a.x1 = x1; a.z_m = z_m;
  a.level_out = level_out;
  return launch_distill_mid(a, S(stream));
}
int smd_distill_loss(const float* x1, const float* z_m, const float* out2, const float* z_t, const float* pred, int kind, int Bn,
                     int Sn, int C, const float* table, int N, const int32_t* steps, const float* iw, float inv_global_count,
                     float* loss_per_sample, float* weight_per_sample, float* dpred, float* target_out, void* stream) {
  DistillLossArgs a;
  a.x1 = x1; a.z_m = z_m; a.out2 = out2; a.z_t = z_t; a.pred = pred; a.kind = kind; a.B = Bn; a.S = Sn; a.C = C; a.N = N;
  a.table = table; a.steps = steps; a.iw = iw; a.inv_global_count = inv_global_count; a.loss_per_sample = loss_per_sample;
  a.weight_per_sample = weight_per_sample; a.dpred = dpred; a.target_out = target_out;
  return launch_distill_loss(a, S(stream));
}

int smd_probe_tr_read(const smd_bf16* image, smd_bf16* out, void* stream) { return launch_probe_tr_read(B(image), B(out), S(stream)); }

// ---- lab entry: launch_gemm_tn_grouped / launch_gemm_tn256_multi on a caller's problem list (include/smd_hip_lab.h).  Everything
// launch_tn128 checks per problem is checked here for the WHOLE list first: a list of more than 8 problems is several launches,
// and a refusal must come before the first of them.  launch_gemm_tn256_multi makes all of its checks in front of its one launch.
int smd_wgrad_lab_launch(const smd_wgrad_problem* probs, int n, int kind, const smd_bf16* zero_page, float* slab, int64_t slab_elems,
                         int32_t* plan_out, int plan_cap, int32_t* launches_out, void* stream) {
  constexpr int MAXP = 64;
  if (launches_out) *launches_out = 0;
  SMD_ARG_CHECK(probs && n >= 1 && n <= MAXP, "smd_wgrad_lab_launch: 1..%d problems", MAXP);
  SMD_ARG_CHECK(kind == 0 || kind == 1, "smd_wgrad_lab_launch: kind must be 0 (grouped 128-wide) or 1 (256-wide multi)");
  SMD_ARG_CHECK(zero_page && slab && slab_elems >= 0 && plan_cap >= 0, "smd_wgrad_lab_launch: needs a zero page and a slab workspace");
  SMD_ARG_CHECK((reinterpret_cast<uintptr_t>(slab) & 15) == 0 && (reinterpret_cast<uintptr_t>(zero_page) & 15) == 0,
                "smd_wgrad_lab_launch: slab and zero page must be 16-byte aligned");
  TnLaunch ts[MAXP];
  for (int i = 0; i < n; ++i) {
    const smd_wgrad_problem& p = probs[i];
    SMD_ARG_CHECK(p.X && p.dY && p.out, "smd_wgrad_lab_launch: problem %d: null operand", i);
    SMD_ARG_CHECK(p.Mrows > 0 && p.Kd > 0 && p.N > 0, "smd_wgrad_lab_launch: problem %d: bad shape", i);
    SMD_ARG_CHECK(p.Mrows == probs[0].Mrows, "smd_wgrad_lab_launch: problem %d: different contraction length (%d, problem 0 has %d)", i,
                  p.Mrows, probs[0].Mrows);
    SMD_ARG_CHECK(p.ldx % 8 == 0 && p.ldy % 8 == 0 && p.ldx >= p.Kd && p.ldy >= p.N && p.ldo >= p.N,
                  "smd_wgrad_lab_launch: problem %d: ldx / ldy must be multiples of 8 and cover Kd / N, ldo >= N", i);
    SMD_ARG_CHECK((reinterpret_cast<uintptr_t>(p.X) & 15) == 0 && (reinterpret_cast<uintptr_t>(p.dY) & 15) == 0 &&
                      (reinterpret_cast<uintptr_t>(p.out) & 3) == 0 && (reinterpret_cast<uintptr_t>(p.bias_out) & 3) == 0,
                  "smd_wgrad_lab_launch: problem %d: X / dY must be 16-byte aligned", i);
    SMD_ARG_CHECK(kind != 0 || p.ldo == p.N, "smd_wgrad_lab_launch: problem %d: the grouped launch needs ldo == N", i);
    TnLaunch& t = ts[i];
    t.X = B(p.X); t.ldx = p.ldx; t.dY = B(p.dY); t.ldy = p.ldy; t.Mrows = p.Mrows; t.Kd = p.Kd; t.N = p.N;
    t.out = p.out; t.ldo = p.ldo; t.bias_out = p.bias_out;
    t.zero_page = B(zero_page); t.slab = slab; t.slab_elems = (size_t)slab_elems; t.tr_path = 1;
  }
  TnPlanLog log = {plan_out, plan_out ? plan_cap : 0, 0};
  smd_tn_plan_log_install(&log);
  const int rc = kind == 0 ? launch_gemm_tn_grouped(ts, n, S(stream)) : launch_gemm_tn256_multi(ts, n, S(stream));
  smd_tn_plan_log_install(nullptr);
  if (launches_out) *launches_out = log.launches;
  return rc;
}

// ---- lab entry: launch_gemm_nt with every field of GemmEpilogue (include/smd_hip_lab.h).  The checks the launcher cannot make (it
// trusts the engine's leading dimensions) come first; the plan is the launcher's own, written only behind a launch.
static int lab_epilogue(const char* who, const smd_gemm_epilogue* e, int N, GemmEpilogue& ep) {
  SMD_ARG_CHECK(e, "%s: null epilogue", who);
  SMD_ARG_CHECK(e->act >= 0 && e->act <= 2 && e->aux_mode >= 0 && e->aux_mode <= 2, "%s: act=%d aux_mode=%d must be 0..2", who,
                e->act, e->aux_mode);
  SMD_ARG_CHECK(e->aux_mode == SMD_AUX_NONE || e->aux, "%s: aux_mode without aux", who);
  SMD_ARG_CHECK(e->res_row_mod >= 0, "%s: res_row_mod=%d must be >= 0", who, e->res_row_mod);
  SMD_ARG_CHECK((!e->pre_bf16 || e->ld_pre >= N) && (!e->aux || e->ld_aux >= N) && (!e->res_f32 || e->ld_res >= N) &&
                    (!e->res_bf16 || e->ld_resb >= N) && (!e->out_f32 || e->ld_out >= N) && (!e->out_bf16 || e->ld_outb >= N),
                "%s: a leading dimension is below N=%d (ld_pre=%d ld_aux=%d ld_res=%d ld_resb=%d ld_out=%d ld_outb=%d)", who, N,
                e->ld_pre, e->ld_aux, e->ld_res, e->ld_resb, e->ld_out, e->ld_outb);
  ep.alpha = e->alpha; ep.bias = e->bias; ep.act = e->act; ep.pre_bf16 = B(e->pre_bf16); ep.ld_pre = e->ld_pre;
  ep.aux = B(e->aux); ep.ld_aux = e->ld_aux; ep.aux_mode = e->aux_mode; ep.res_f32 = e->res_f32; ep.ld_res = e->ld_res;
  ep.res_row_mod = e->res_row_mod; ep.res_bf16 = B(e->res_bf16); ep.ld_resb = e->ld_resb; ep.out_f32 = e->out_f32; ep.ld_out = e->ld_out;
  ep.accumulate = e->accumulate; ep.out_bf16 = B(e->out_bf16); ep.ld_outb = e->ld_outb;
  return 0;
}
int smd_gemm_nt_lab(const smd_bf16* A, int lda, const smd_bf16* Bt, int ldb, int M, int N, int K, const smd_gemm_epilogue* e,
                    int min_tiles, int32_t* plan_out, void* stream) {
  SMD_ARG_CHECK(e, "smd_gemm_nt_lab: null epilogue");
  SMD_ARG_CHECK(A && Bt && (reinterpret_cast<uintptr_t>(A) & 15) == 0 && (reinterpret_cast<uintptr_t>(Bt) & 15) == 0,
                "smd_gemm_nt_lab: A / Bt must be non-null and 16-byte aligned");
  GemmEpilogue ep;
  if (lab_epilogue("smd_gemm_nt_lab", e, N, ep) != 0) return -1;
  smd_plan::NtPlan p = {};
  const int rc = launch_gemm_nt(B(A), lda, B(Bt), ldb, M, N, K, ep, S(stream), min_tiles > 0 ? min_tiles : smd_plan::NT256_MIN_TILES, &p);
  if (rc == 0 && plan_out) {
    const int v[8] = {p.kernel, p.BM, p.NS, p.KG, p.grid, p.block, p.pk_epilogue, p.vec_epilogue};
    for (int i = 0; i < 8; ++i) plan_out[i] = v[i];
  }
  return rc;
}

// ---- lab entry: launch_gemm_nt256_fp8 with every field of GemmEpilogue (the forms the engine's e4m3 layers and dgrads run)
int smd_gemm_e4m3_nt_lab(const uint8_t* A8, int lda, const uint32_t* scale_a, const uint8_t* Bt8, int ldb, const uint32_t* scale_b,
                         int M, int N, int K, const smd_gemm_epilogue* e, void* stream) {
  SMD_ARG_CHECK(e, "smd_gemm_e4m3_nt_lab: null epilogue");
  SMD_ARG_CHECK(A8 && Bt8 && (reinterpret_cast<uintptr_t>(A8) & 15) == 0 && (reinterpret_cast<uintptr_t>(Bt8) & 15) == 0,
                "smd_gemm_e4m3_nt_lab: A8 / Bt8 must be non-null and 16-byte aligned");
  GemmEpilogue ep;
  if (lab_epilogue("smd_gemm_e4m3_nt_lab", e, N, ep) != 0) return -1;
  return launch_gemm_nt256_fp8(A8, lda, scale_a, Bt8, ldb, scale_b, M, N, K, ep, S(stream));
}

// ---- lab entries: the launchers of diffusion.hip with every field of their argument structs (include/smd_hip_lab.h).  What the
// launchers trust the engine for is checked here; the alignment of the vector forms is the launchers' own check.  The reported
// form is the launcher's, written only behind a launch.
static inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
static inline bool al2(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 1) == 0; }

int smd_reverse_step_lab(const smd_reverse_step_args* p, int32_t* form_out, void* stream) {
  SMD_ARG_CHECK(p, "smd_reverse_step_lab: null arguments");
  SMD_ARG_CHECK(al4(p->x) && al4(p->eps_hat) && al4(p->coef) && al4(p->t_ptr) && al4(p->t_advance) && al4(p->arrive) && al4(p->z_in) &&
                    al4(p->key_ptr) && al4(p->infill_samples) && al4(p->infill_masks) && al4(p->infill_z_in) && al4(p->tf_noise_keys) &&
                    al4(p->tf_infill_keys) && al4(p->metrics_partial) && al4(p->collection) && al4(p->slot_table) && al2(p->x_bf16),
                "smd_reverse_step_lab: a pointer is not aligned to its element");
  SMD_ARG_CHECK(p->Cp >= p->C, "smd_reverse_step_lab: Cp=%d is below C=%d", p->Cp, p->C);
  SMD_ARG_CHECK(p->infill_masks || !(p->infill_z_in || p->tf_infill_keys), "smd_reverse_step_lab: infill draws without infill masks");
  SMD_ARG_CHECK(!(p->tf_noise_keys || p->tf_infill_keys) || (p->tf_t0 >= 0 && p->tf_t0 < p->T),
                "smd_reverse_step_lab: tf_t0=%d must be in [0, T): the key tables are indexed by tf_t0 - t", p->tf_t0);
  ReverseStepArgs a;
  a.x = p->x; a.eps_hat = p->eps_hat; a.B = p->B; a.S = p->S; a.C = p->C; a.Cp = p->Cp; a.T = p->T; a.coef = p->coef;
  a.t_ptr = p->t_ptr; a.t_advance = p->t_advance; a.arrive = p->arrive; a.z_in = p->z_in; a.key = RngKey{p->seed_lo, p->seed_hi};
  a.key_ptr = p->key_ptr; a.sample_offset = p->sample_offset; a.infill_samples = p->infill_samples; a.infill_masks = p->infill_masks;
  a.infill_z_in = p->infill_z_in; a.tf_noise_keys = p->tf_noise_keys; a.tf_infill_keys = p->tf_infill_keys;
  a.tf_n_total = p->tf_n_total; a.tf_t0 = p->tf_t0; a.x_bf16 = B(p->x_bf16); a.metrics_partial = p->metrics_partial;
  a.collection = p->collection; a.slot_table = p->slot_table;
  int form[2] = {0, 0};
  const int rc = launch_reverse_step(a, S(stream), form);
  if (rc == 0 && form_out) { form_out[0] = form[0]; form_out[1] = form[1]; }
  return rc;
}

int smd_adams_step(const smd_adams_step_args* p, void* stream) {
  SMD_ARG_CHECK(p, "smd_adams_step: null arguments");
  SMD_ARG_CHECK(al4(p->x) && al4(p->hist) && al4(p->eps_hat) && al4(p->coef) && al4(p->plan) && al4(p->t_ptr) && al4(p->t_advance) &&
                    al4(p->arrive) && al4(p->key_ptr) && al4(p->infill_samples) && al4(p->infill_masks) && al4(p->infill_z_in) &&
                    al4(p->tf_infill_keys) && al4(p->metrics_partial) && al4(p->collection) && al2(p->x_bf16),
                "smd_adams_step: a pointer is not aligned to its element");
  SMD_ARG_CHECK(p->Cp >= p->C, "smd_adams_step: Cp=%d is below C=%d", p->Cp, p->C);
  SMD_ARG_CHECK(p->infill_masks || !(p->infill_z_in || p->tf_infill_keys), "smd_adams_step: infill draws without infill masks");
  AdamsStepArgs a;
  a.x = p->x; a.hist = p->hist; a.eps_hat = p->eps_hat; a.B = p->B; a.S = p->S; a.C = p->C; a.Cp = p->Cp; a.T = p->T;
  a.coef = p->coef; a.plan = p->plan; a.t_ptr = p->t_ptr; a.t_advance = p->t_advance; a.arrive = p->arrive;
  a.key = RngKey{p->seed_lo, p->seed_hi}; a.key_ptr = p->key_ptr; a.sample_offset = p->sample_offset;
  a.infill_samples = p->infill_samples; a.infill_masks = p->infill_masks; a.infill_z_in = p->infill_z_in;
  a.tf_infill_keys = p->tf_infill_keys; a.tf_n_total = p->tf_n_total; a.x_bf16 = B(p->x_bf16);
  a.metrics_partial = p->metrics_partial; a.collection = p->collection;
  return launch_adams_step(a, S(stream));
}

int smd_q_sample_lab(const smd_q_sample_args* p, int32_t* form_out, void* stream) {
  SMD_ARG_CHECK(p, "smd_q_sample_lab: null arguments");
  SMD_ARG_CHECK(al4(p->x0) && al4(p->alphas_prod_ext) && al4(p->labels) && al4(p->alpha_in) && al4(p->eps_in) && al4(p->step_ptr) &&
                    al4(p->eps_out) && al4(p->s_out) && al2(p->xt_bf16),
                "smd_q_sample_lab: a pointer is not aligned to its element");
  SMD_ARG_CHECK(p->dsm == 0 || p->dsm == 1, "smd_q_sample_lab: dsm=%d must be 0 or 1", p->dsm);
  SMD_ARG_CHECK((int64_t)p->S * p->C < (1ll << 31), "smd_q_sample_lab: S*C must fit an int");
  QSampleArgs q;
  q.x0 = p->x0; q.B = p->B; q.S = p->S; q.C = p->C; q.Cp = p->Cp; q.T = p->T; q.alphas_prod_ext = p->alphas_prod_ext;
  q.labels = p->labels; q.label_min = p->label_min; q.alpha_in = p->alpha_in; q.dsm = p->dsm; q.eps_in = p->eps_in;
  q.key = RngKey{p->seed_lo, p->seed_hi}; q.step_ptr = p->step_ptr; q.sample_offset = p->sample_offset;
  q.xt_bf16 = B(p->xt_bf16); q.eps_out = p->eps_out; q.s_out = p->s_out;
  int form = -1;
  const int rc = launch_q_sample(q, S(stream), &form);
  if (rc == 0 && form_out) *form_out = form;
  return rc;
}

int smd_weighted_mse_fwd_bwd(const float* pred, const float* eps, const float* noise_level, const float* iw, float min_snr_gamma,
                             int Bn, int Sn, int C, int Cp, float inv_global_count, float* loss_per_sample,
                             float* weight_per_sample, smd_bf16* dpred_bf16, void* stream) {
  return launch_weighted_mse_loss_grad(pred, eps, noise_level, iw, min_snr_gamma, Bn, Sn, C, Cp, inv_global_count, loss_per_sample,
                                       weight_per_sample, B(dpred_bf16), S(stream));
}
int smd_param_mse_fwd_bwd(const float* pred, const float* eps, const float* x0, const float* noise_level, const float* iw,
                          float min_snr_gamma, int kind, int Bn, int Sn, int C, int Cp, float inv_global_count,
                          float* loss_per_sample, float* weight_per_sample, smd_bf16* dpred_bf16, void* stream) {
  return launch_param_mse_loss_grad(pred, eps, x0, noise_level, iw, min_snr_gamma, kind, Bn, Sn, C, Cp, inv_global_count,
                                    loss_per_sample, weight_per_sample, B(dpred_bf16), S(stream));
}
int smd_timestep_draw(const float* cdf, const float* p, int n, int label_base, int Bn, uint32_t seed_lo, uint32_t seed_hi,
                      uint32_t sample_offset, uint32_t step, const uint32_t* step_ptr, const float* u_in, int32_t* labels_out,
                      float* iw_out, void* stream) {
  return launch_timestep_draw(cdf, p, n, label_base, Bn, seed_lo, seed_hi, sample_offset, step, step_ptr, u_in, labels_out, iw_out,
                              S(stream));
}
int smd_timestep_update(const int32_t* labels, const float* loss, int Bg, float* history, int32_t* counts, int n, int label_base,
                        float uniform_mix, float* p_out, float* cdf_out, int32_t* warmed_out, void* stream) {
  return launch_timestep_update(labels, loss, Bg, history, counts, n, label_base, uniform_mix, p_out, cdf_out, warmed_out,
                                S(stream));
}
int smd_loss_grad_lab(const float* pred, const float* eps, int Bn, int Sn, int C, int Cp, float inv_global_count, float* loss_per_sample,
                      smd_bf16* dpred_bf16, const float* dsm_sigma, int32_t* form_out, void* stream) {
  SMD_ARG_CHECK(al4(pred) && al4(eps) && al4(loss_per_sample) && al4(dsm_sigma) && al2(dpred_bf16),
                "smd_loss_grad_lab: a pointer is not aligned to its element");
  SMD_ARG_CHECK(Sn > 0 && C > 0 && (int64_t)Sn * C < (1ll << 31), "smd_loss_grad_lab: S*C must fit an int");
  int vec = 0;
  const int rc = launch_mse_loss_grad(pred, eps, Bn, Sn, C, Cp, inv_global_count, loss_per_sample, B(dpred_bf16), S(stream), dsm_sigma, &vec);
  if (rc == 0 && form_out) *form_out = vec;
  return rc;
}

// ---- lab probe: a stream restricted by a raw CU mask (hipExtStreamCreateWithCUMask).  What the mask can express on this part is
// documented in include/smd_hip_lab.h (tools/cumask_probe.hip: bit i belongs to XCC i % 8; an XCC whose share is empty is NOT masked).
int smd_probe_stream_create_cu_mask(const uint32_t* mask_words, int n_words, void** stream_out) {
  SMD_ARG_CHECK(mask_words && stream_out && n_words >= 1 && n_words <= 8, "smd_probe_stream_create_cu_mask: bad argument");
  hipStream_t st = nullptr;
  const hipError_t err = hipExtStreamCreateWithCUMask(&st, (uint32_t)n_words, mask_words);
  if (err != hipSuccess) { smd_set_error("hipExtStreamCreateWithCUMask: %s", hipGetErrorString(err)); return (int)err; }
  *stream_out = reinterpret_cast<void*>(st);
  return 0;
}
int smd_probe_stream_destroy(void* stream) {
  SMD_ARG_CHECK(stream, "smd_probe_stream_destroy: null stream");
  const hipError_t err = hipStreamDestroy(S(stream));
  if (err != hipSuccess) { smd_set_error("hipStreamDestroy: %s", hipGetErrorString(err)); return (int)err; }
  return 0;
}

// lab probe: where a one-wave kernel runs and the shader clock it sees.  out[0] = XCC id, out[1] = HW_ID, out[2..3] = s_memtime
// ticks (shader cycles) and out[4..5] = s_memrealtime ticks (100 MHz) spent spinning for ~spin_us
__global__ __launch_bounds__(64) void probe_clock_kernel(uint32_t* __restrict__ out, int spin_us) {
  const uint32_t xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);       // HW_REG_XCC_ID
  const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);         // HW_REG_HW_ID
  const uint64_t r0 = __builtin_amdgcn_s_memrealtime();
  const uint64_t c0 = __builtin_amdgcn_s_memtime();
  uint64_t r1 = r0;
  while (r1 - r0 < (uint64_t)spin_us * 100) { __builtin_amdgcn_s_sleep(4); r1 = __builtin_amdgcn_s_memrealtime(); }
  const uint64_t c1 = __builtin_amdgcn_s_memtime();
  if (threadIdx.x == 0) {
    uint32_t* o = out + 8 * blockIdx.x;
    o[0] = xcc; o[1] = hw;
    o[2] = (uint32_t)(c1 - c0); o[3] = (uint32_t)((c1 - c0) >> 32);
    o[4] = (uint32_t)(r1 - r0); o[5] = (uint32_t)((r1 - r0) >> 32);
    o[6] = (uint32_t)r0; o[7] = (uint32_t)(r0 >> 32);
  }
}
// lab probe: every XCD reads all `bytes` of `p` (workgroup b runs on XCD b % 8 and reads slice b / 8): the buffer is then
// resident in all eight L2s -- what a weight prefetch ahead of a latency-bound kernel would achieve
__global__ __launch_bounds__(256) void l2_warm_kernel(const uint4* __restrict__ p, size_t n16, int slices, uint32_t* __restrict__ sink) {
  const int slice = blockIdx.x >> 3;
  const size_t per = (n16 + slices - 1) / slices;
  const size_t lo = (size_t)slice * per, hi = lo + per < n16 ? lo + per : n16;
  uint32_t acc = 0;
  for (size_t i = lo + threadIdx.x; i < hi; i += 256) { const uint4 v = p[i]; acc ^= v.x ^ v.y ^ v.z ^ v.w; }
  if (acc == 0x9E3779B9u && sink) *sink = acc;     // never true in practice: keeps the loads
}
int smd_probe_l2_warm(const void* p, int64_t bytes, uint32_t* sink, void* stream) {
  SMD_ARG_CHECK(p && bytes >= 16 && bytes % 16 == 0, "smd_probe_l2_warm: bad argument");
  const size_t n16 = (size_t)bytes / 16;
  int slices = (int)((n16 + 2047) / 2048);          // <= 32 KiB per workgroup
  if (slices > 256) slices = 256;
  hipLaunchKernelGGL(l2_warm_kernel, dim3(8 * slices), dim3(256), 0, S(stream), reinterpret_cast<const uint4*>(p), n16, slices, sink);
  SMD_LAUNCH_CHECK();
  return 0;
}
int smd_probe_clock(uint32_t* out, int blocks, int spin_us, void* stream) {
  SMD_ARG_CHECK(out && blocks > 0 && spin_us >= 0, "smd_probe_clock: bad argument");
  hipLaunchKernelGGL(probe_clock_kernel, dim3(blocks), dim3(64), 0, S(stream), out, spin_us);
  SMD_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
