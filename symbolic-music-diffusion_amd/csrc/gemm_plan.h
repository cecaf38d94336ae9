// Which GEMM kernel, tile form and split-K factor a launch gets: every decision of the GEMM launchers, and nothing else.
// Plain C++17 without a HIP include: shapes, epilogue flags and knob VALUES go in (the launchers read the knobs and see the
// pointers), a small POD plan comes out.  tests/test_gemm_plan_host.py checks every function against tests/golden/gemm_dispatch.json.
#pragma once
#include <stddef.h>

namespace smd_plan {
// ------------------------------------------------------------------ NT GEMMs (gemm_nt.hip / gemm_nt256.hip)
constexpr int NT_BN = 128, NT_BK = 64;        // 128-wide kernel: BM x 128 x 64 tiles
constexpr int NT256_T = 256, NT256_TK = 64;   // 256 x 256 x 64 tiles
// at least ~3/4 of the 256 CUs busy (192 tiles): smaller grids are better served by 128-wide tiles -- unless the caller runs
// two such streams side by side (concurrent sampling chains ask for 128)
constexpr int NT256_MIN_TILES = 192;
// what the decision needs from the epilogue (smd_epi::plan_flags in gemm_epilogue.h fills it)
struct NtEpiFlags {
  int oct_ok, vec_ok;                                   // the 8-column / 4-column vector epilogues apply (alignment, alpha, accumulate)
  int out_bf16, out_f32, pre_bf16, act, aux, res;       // which outputs and stages the epilogue has
};
struct NtKnobs { int nt256, nt256_pk, deep, kg, form, form_wk; };   // gemm_nt256, gemm_nt256_pk, gemm_nt_deep, gemm_nt_kg, gemm_nt_form, gemm_nt_form_wk
enum NtKernel { NT128 = 128, NT256 = 256 };
struct NtPlan {
  int kernel;                       // NT128: gemm_nt_kernel<BM, NS, KG>, NT256: gemm_nt256_kernel
  int BM, NS, KG;                   // tile height, LDS K-tile buffers, K-groups of four waves
  int grid, block;
  int pk_epilogue, vec_epilogue;    // NT256: packed-bf16 epilogue; NT128: 4-column vector epilogue
};

// the packed-bf16 epilogue applies: (bias ->) bf16 output and nothing else (knob "gemm_nt256_pk" 0 switches it off: A/B, tests)
inline int nt256_pk_epilogue(const NtEpiFlags& f, int knob_pk) {
  return (knob_pk != 0 && f.out_bf16 && !f.out_f32 && !f.pre_bf16 && !f.act && !f.aux && !f.res) ? 1 : 0;
}
inline bool nt256_eligible(int M, int N, int K, const NtEpiFlags& f, int min_tiles, int knob_nt256) {
  if (!f.oct_ok || knob_nt256 == 0 || M % NT256_T || N % NT256_T || K % (2 * NT256_TK) || K < 2 * NT256_TK) return false;
  if (knob_nt256 == 2) return true;                  // forced (tests)
  return (long)(M / NT256_T) * (N / NT256_T) >= min_tiles;
}

inline NtPlan nt_plan(int M, int N, int K, const NtEpiFlags& f, int min_tiles, const NtKnobs& k) {
  NtPlan p = {NT128, 0, 2, 1, 0, 0, 0, 0};
  if (nt256_eligible(M, N, K, f, min_tiles, k.nt256)) {
    p.kernel = NT256; p.BM = NT256_T; p.grid = (M / NT256_T) * (N / NT256_T); p.block = 512;
    p.pk_epilogue = nt256_pk_epilogue(f, k.nt256_pk);
    return p;
  }
  auto form = [&p](int bm, int ns, int kg) { p.BM = bm; p.NS = ns; p.KG = kg; };
  const int BK = NT_BK;
  // tile height: keep >= ~256 workgroups on the chip when the output is skinny
  const int tiles_n = (N + NT_BN - 1) / NT_BN;
  const long wg128 = (long)((M + 127) / 128) * tiles_n;
  const long wg64 = (long)((M + 63) / 64) * tiles_n;
  const bool deep = K >= 8 * BK && k.deep;
  const bool k2 = K % (2 * BK) == 0;                // two K-groups need an even number of K-tiles
  // measurement knob (tools/gemm_nt_forms_ab.py): force one tile form for the shapes that have a choice
  // ("gemm_nt_form_wk": the same for the wide-K, few-column shapes only -- out_proj: N <= 512, K >= 2048 -- so that an in-step A/B
  // of that one GEMM leaves every other launch on its default form); a two-K-group form falls through to the default when K % 128 != 0
  const int form_wk = (M > 64 && N <= 512 && K >= 2048) ? k.form_wk : 0;
  const int forced = form_wk ? form_wk : (M > 64 ? k.form : 0);
  static const int FORMS[7][3] = {{0, 0, 0}, {64, 2, 1}, {128, 2, 1}, {128, 2, 2}, {64, 2, 2}, {128, 3, 1}, {64, 3, 2}};
  if (forced >= 1 && forced <= 6 && (FORMS[forced][2] == 1 || k2)) form(FORMS[forced][0], FORMS[forced][1], FORMS[forced][2]);
  else if (N <= 512 && K >= 2048 && k2 && M >= 2048 && k.kg) {
    // out_proj (models/ncsn.py:177-178: rows x 2048 -> 512): 128-row tiles with two K-groups of four waves -- half the operand
    // traffic per flop of the 64-row form and two waves per SIMD on one tile.  In-step A/B (profiles/r6d_schedule_and_out_proj_form_ab.txt):
    // sample step +2 ... +3 % (1849 / 1855 -> 1914 / 1885 steps/s), train step unchanged
    form(128, 2, 2);
  } else if (M <= 32 || !(wg128 >= 512 || wg64 >= 256 || M <= 64)) {
    // K >= 1024: two K-groups of four waves per workgroup (A/B: 8-18 % over one group with a 4-deep ring; deeper rings
    // -- 7 stages, or 2 groups x 4 stages -- gain nothing: the step time follows the LDS-DMA landing cadence)
    if (deep && K >= 16 * BK && k2 && k.kg) form(32, 3, 2);
    else if (deep) form(32, 4, 1);
    else form(32, 2, 1);
  } else if (wg128 >= 512) {
    form(128, 2, 1);
  } else if (wg64 <= 256 && K >= 16 * BK && k2 && k.kg) {
    // exactly one 64-row workgroup per CU and a long K (out_proj of one sampler chain, 4096 x 2048 -> 512; out_proj of the
    // C = 146 network): two K-groups of four waves = two waves per SIMD on the same tile, 19.6 -> 16.5 us and 18.9 -> 15.8 us
    // (profiles/r4w_gemm_nt_forms.txt); with two workgroups per CU (8192 x 2048 -> 512) the one-group form is the faster one
    form(64, 2, 2);
  } else {
    form(64, 2, 1);   // 4 stages = 96 KiB: 1 workgroup per CU instead of 3, slower (A/B)
  }
  p.grid = ((M + p.BM - 1) / p.BM) * tiles_n;
  p.block = 256 * p.KG;
  p.vec_epilogue = f.vec_ok;
  return p;
}

// ------------------------------------------------------------------ 128-wide weight-gradient kernel (gemm_tn.hip)
constexpr int TN128_T = 128, TN128_KM = 64;               // output tile edge, m rows per K-tile
constexpr int TN128_BUF_BYTES = 2 * TN128_KM * TN128_T * 2;   // one K-tile buffer: X tile + dY tile, 16 KiB each
constexpr int TN128_MAX_SPLIT = 32;
// tn128_target_wgs, tn_split_model, tn_exclusive_cu, gemm_tn_deep, tn128_loader_waves, tn_mode
struct TnKnobs { int target_wgs, split_model, exclusive_cu, deep, loader_waves, mode; };
struct TnSplit { int nsplit, ktiles_per_split; };
enum TnSite { TN_GROUPED = 0, TN_SINGLE = 1 };

// Split-K factor of a 128x128-tile launch.  With CU-exclusive workgroups (tn_exclusive_cu) a launch runs in whole rounds of
// 256 workgroups, so 36 tiles x 15 splits = 540 workgroups (the old "about 512" rule) took THREE rounds of 9 K-tiles;
// 7 splits = 252 workgroups take one round of 19.  Cost in K-tile units: rounds x (K-tiles per split + a fixed prologue /
// slab-epilogue share) + the slab traffic the split adds; the smallest wins, ties go to fewer splits.
inline int tn128_pick_split(int tiles, int total_kt, int max_split, const TnKnobs& k) {
  if (!k.split_model) {
    const int ns = (512 + tiles - 1) / tiles;
    return ns < 1 ? 1 : (ns > max_split ? max_split : ns);
  }
  const int per_round = k.exclusive_cu ? 256 : 512;
  int best = 1;
  float best_cost = 1e30f;
  for (int ns = 1; ns <= max_split && ns <= total_kt; ++ns) {
    const int per = (total_kt + ns - 1) / ns;
    const int rounds = (tiles * ns + per_round - 1) / per_round;
    const float cost = (float)rounds * ((float)per + 5.0f) + (ns > 1 ? 0.35f * (float)ns : 0.0f);
    if (cost < best_cost - 1e-3f) { best_cost = cost; best = ns; }
  }
  return best;
}

// One split planner for both launch sites.  `cap_splits`: how many splits' partials fit the slab workspace (0: the launch runs
// unsplit).  TN_SINGLE (launch_gemm_tn) splits only below its target of workgroups on the chip -- 512 (two per CU); 256 for
// the 128-wide weights (tiles <= 16), where the slab traffic of 32 splits costs more than the second workgroup per CU gains
// (kbench --tn128) -- and with tn_split_model 0 aims at that target; TN_GROUPED always asks tn128_pick_split.
inline TnSplit tn128_split(int tiles, int total_kt, size_t cap_splits, TnSite site, const TnKnobs& k) {
  int nsplit;
  if (site == TN_SINGLE) {
    int target = k.target_wgs;
    if (target == 512 && tiles <= 16) target = 256;
    if (tiles >= target) nsplit = 1;
    else nsplit = k.split_model ? tn128_pick_split(tiles, total_kt, TN128_MAX_SPLIT, k) : (target + tiles - 1) / tiles;
  } else {
    nsplit = tn128_pick_split(tiles, total_kt, TN128_MAX_SPLIT, k);
  }
  if (nsplit > TN128_MAX_SPLIT) nsplit = TN128_MAX_SPLIT;
  if (nsplit > total_kt) nsplit = total_kt;
  if ((size_t)nsplit > cap_splits) nsplit = (int)cap_splits;
  if (nsplit < 1) nsplit = 1;            // one split writes the gradients directly, no slab needed
  const int per = (total_kt + nsplit - 1) / nsplit;
  return TnSplit{(total_kt + per - 1) / per, per};
}

// Kernel variant of the 128-wide launch: NS LDS K-tile buffers, NW waves that issue the LDS-DMA, dynamic-LDS pad in bytes.
// CU-exclusive launch: four MFMA waves + four loader waves (tn128_loader_waves = 0: the four MFMA waves load themselves).
// Knob "tn_mode" (A/B experiments) overrides the choice: NS*100 + NW*10 + pad, pad 0 = none, 1 = fill the
// CU's 160 KiB, 2 = pad the workgroup to 96 KiB (one wgrad workgroup per CU, small-LDS workgroups may still share it).
// tn_exclusive_cu != 0 (default 2): the four-buffer instantiation (1: padded to the CU's whole LDS, see smd_tn_pad_bytes()); the
// single launch also takes it for long splits under gemm_tn_deep.
struct TnMode { int mode, ns, nw, pad_bytes; };
inline TnMode tn128_mode(int ktiles_per_split, TnSite site, const TnKnobs& k) {
  int mode = k.mode;
  if (!mode) {
    const bool exclusive = k.exclusive_cu != 0 || (site == TN_SINGLE && ktiles_per_split >= 6 && k.deep);
    mode = exclusive ? 400 + (k.loader_waves ? 80 : 40) + (k.exclusive_cu == 1 ? 1 : 0) : 240;
  }
  TnMode m = {mode, mode / 100, (mode / 10) % 10, 0};
  const int padc = mode % 10, lds = m.ns * TN128_BUF_BYTES;
  if (padc == 1) m.pad_bytes = 160 * 1024 - lds;
  else if (padc == 2) m.pad_bytes = 96 * 1024 - lds;
  if (m.pad_bytes < 0) m.pad_bytes = 0;
  return m;
}

// ------------------------------------------------------------------ 256-wide weight-gradient kernel (gemm_tn256.hip)
constexpr int TN256_T = 256, TN256_KM = 64;
// `nsplit` capped so that a block walks at least 4 K-tiles, K-tiles per split rounded up to even (the pipeline consumes them
// in pairs), `nsplit` recomputed
inline TnSplit tn256_round(int total_kt, int nsplit) {
  if (nsplit * 4 > total_kt) nsplit = total_kt / 4;
  if (nsplit < 1) nsplit = 1;
  int per = (total_kt + nsplit - 1) / nsplit;
  per = (per + 1) & ~1;
  return TnSplit{(total_kt + per - 1) / per, per};
}
// Shape part of the eligibility + split choice of a lone problem (gemm_tn256_plan adds the pointer / stride checks);
// nsplit == 0: not eligible, the 128-wide kernel takes it.  knob = "gemm_tn256" (0 off, 2 forced: tests).
inline TnSplit tn256_plan(int Mrows, int Kd, int N, size_t slab_elems, int knob) {
  const TnSplit no = {0, 0};
  if (knob == 0 || Kd % TN256_T || N % TN256_T) return no;
  const int tiles = (Kd / TN256_T) * (N / TN256_T);
  const int total_kt = (Mrows + TN256_KM - 1) / TN256_KM;
  if (total_kt < 8) return no;
  const int want = (256 + tiles - 1) / tiles;           // one workgroup per CU (128 KiB LDS each)
  if (want > 4 && knob != 2) return no;                 // slab traffic would dominate: 128-wide kernel
  const TnSplit s = tn256_round(total_kt, want);
  const size_t need = (size_t)s.nsplit * Kd * N + (size_t)s.nsplit * (Kd / TN256_T) * N;
  if (need > slab_elems) return no;
  if ((long)tiles * s.nsplit < 96 && knob != 2) return no;   // tiny grids: 128-wide kernel
  return s;
}
inline TnSplit tn256_multi_split(int total_kt, int tiles_all) { return tn256_round(total_kt, 256 / tiles_all); }   // n problems, one launch: one workgroup per CU

}  // namespace smd_plan
