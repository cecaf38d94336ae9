// Process-wide kernel-selection knobs (smd_set_tuning in the C-ABI): benchmark A/B and tests; the defaults are the fast paths.
// The launchers read them with smd_tuning_get; the GEMM launchers pass the values on to the planners of gemm_plan.h.
#include "smd_kernels.h"
#include <string.h>

namespace {
struct Knob { const char* key; int value; };
Knob g_knobs[] = {
    {"gemm_nt256", 1},           // 256x256 NT kernel: 0 off, 1 for eligible shapes of >= min_tiles tiles, 2 for every eligible shape (tests)
    {"gemm_nt256_variant", 0},   // its schedule variant: 1..3 compute the same result (A/B); ablations 4.. need -DSMD_ABLATIONS
    {"gemm_nt256_pk", 1},        // its packed-bf16 epilogue for (bias ->) bf16 outputs; 0 off (A/B, tests)
    {"gemm_tn256", 1},           // 256x256 weight-gradient kernel: 0 off, 1 where eligible, 2 also for many-split / tiny grids (tests)
    {"ln_bwd_wide", 2},          // LayerNorm backward, D 1024..2048: 0 register kernel, 1 LDS-parameter kernel, 2 row-group kernel at D = 2048
    {"ln_bwd_narrow", 1},        // LayerNorm backward, D = 128: the 32-row-group kernel; 0 the generic one
    {"gemm_nt_deep", 1},         // 128-wide NT kernel, 32-row tiles, K >= 512: four LDS buffers instead of two
    {"mlp_variant", 0},          // encoder MLP kernels: 0 default forms; 5 eight-wave hidden-split forward, 9 backward re-reading fragments (A/B)
    {"tn128_target_wgs", 512},   // 128-wide weight gradient, single launch: split-K only below this many workgroups (256 at <= 16 tiles)
    {"gemm_tn_deep", 0},         // the same launch without tn_exclusive_cu: four-buffer kernel from 6 K-tiles per split up
    {"ln_fwd_wide", 3},          // LayerNorm forward, D 1024 / 2048: 0 row kernel, 1..3 its row-group kernels (3: the current form)
    {"gemm_nt_kg", 1},           // 128-wide NT kernel: two K-groups of four waves for long-K, few-workgroup shapes
    {"mlp_hs_dbg", 0},           // hidden-split MLP kernels: debug bits (64 / 128: phase stamps instead of the result)
    {"ln_excl", 0},              // ln128 backward: KiB of dynamic-LDS pad that keeps 64-KiB workgroups off its CU (experiment)
    {"tn_exclusive_cu", 2},      // weight-gradient kernels: 2 four-buffer kernels, 1 the same padded to the CU's 160 KiB, 0 two-buffer kernel (A/B build)
    {"tn_split_model", 1},       // 128-wide weight gradient: split-K factor from the round / slab cost model; 0 the "about 512 workgroups" rule
    {"tn128_loader_waves", 1},   // 128-wide weight gradient: four extra waves that only issue the LDS-DMA
    {"tn_mode", 0},              // 128-wide weight gradient: force NS*100 + NW*10 + pad (variants other than 48x need -DSMD_TN_EXPERIMENTS)
    {"gemm_nt_form", 0},         // 128-wide NT kernel, M > 64: force tile form 1..6 (tools/gemm_nt_forms_ab.py)
    {"gemm_nt_form_wk", 0},      // the same for the wide-K, few-column shapes only (N <= 512, K >= 2048: out_proj)
};
}  // namespace
int smd_tuning_set(const char* key, int value) {
  for (Knob& k : g_knobs)
    if (key && !strcmp(key, k.key)) { k.value = value; return 0; }
  smd_set_error("smd_set_tuning: unknown key '%s'", key ? key : "(null)");
  return -1;
}
int smd_tuning_get(const char* key) {
  for (const Knob& k : g_knobs)
    if (key && !strcmp(key, k.key)) return k.value;
  return -1;
}
