"""absl-compatible command-line / flagfile parser (absl is not installed on the target image).

Keeps the flag surface of the reference: the 41 flags of train_ncsn.py:48-128 and the 9 of
sample_ncsn.py:51-66 with the same names, types and defaults, nested ``--flagfile=`` (later flags
win, configs/ddpm-mel-32seq-512-large.cfg:1), ``--flag`` / ``--noflag`` / ``--flag=False`` booleans
(configs/ddpm-base.cfg:8-10,14), comma lists (``--data_shape=32,512``), enums, ``None`` integers.
Engine-only flags (``--dtype``, ``--synthetic``, ...) are added on top and do not collide.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence


@dataclass
class FlagDef:
    name: str
    kind: str            # int | float | bool | string | enum | list
    default: Any
    help: str = ""
    choices: Optional[Sequence[str]] = None


class FlagError(ValueError):
    pass


class FlagValues:
    """Attribute access like absl's FLAGS; ``flags_into_string()`` like train_ncsn.py:557."""

    def __init__(self, defs: Sequence[FlagDef]):
        object.__setattr__(self, "_defs", {d.name: d for d in defs})
        object.__setattr__(self, "_values", {d.name: d.default for d in defs})
        object.__setattr__(self, "_present", set())
        object.__setattr__(self, "_flagfile_dirs", [])

    def __getattr__(self, name):
        try:
            return self._values[name]
        except KeyError:
            raise AttributeError(f"Unknown flag {name}") from None

    def __setattr__(self, name, value):
        if name not in self._defs:
            raise AttributeError(f"Unknown flag {name}")
        self._values[name] = value

    def is_present(self, name: str) -> bool:
        return name in self._present

    def flag_values_dict(self) -> Dict[str, Any]:
        return dict(self._values)

    def flags_into_string(self) -> str:
        out = []
        for k, v in self._values.items():
            d = self._defs[k]
            if d.kind == "bool":
                out.append(f"--{k}" if v else f"--no{k}")
            elif d.kind == "list":
                out.append(f"--{k}={','.join(str(x) for x in v)}")
            elif v is not None:
                out.append(f"--{k}={v}")
        return "\n".join(out)

    # ---- parsing
    def _convert(self, d: FlagDef, text: str):
        try:
            if d.kind == "int":
                return None if text in ("None", "") else int(text)
            if d.kind == "float":
                return float(text)
            if d.kind == "bool":
                t = text.strip().lower()
                if t in ("true", "t", "1", "yes", "y"):
                    return True
                if t in ("false", "f", "0", "no", "n"):
                    return False
                raise ValueError(text)
            if d.kind == "enum":
                if text not in d.choices:
                    raise FlagError(f"flag --{d.name}={text}: value should be one of <{'|'.join(d.choices)}>")
                return text
            if d.kind == "list":
                return [t for t in text.split(",")] if text != "" else []
            return text
        except FlagError:
            raise
        except ValueError:
            raise FlagError(f"flag --{d.name}={text}: invalid {d.kind} value") from None

    def _set(self, name: str, value):
        self._values[name] = value
        self._present.add(name)

    def read_flagfile(self, path: str, _depth: int = 0) -> List[str]:
        if _depth > 16:
            raise FlagError(f"flagfile nesting too deep at {path}")
        if not os.path.exists(path):
            # absl resolves nested flagfiles against the CWD (the reference is run from its repo
            # root); additionally try the directories of the including flagfiles.
            for base in reversed(self._flagfile_dirs):
                for cand in (os.path.join(base, path), os.path.join(os.path.dirname(base), path)):
                    if os.path.exists(cand):
                        path = cand
                        break
                else:
                    continue
                break
        if not os.path.exists(path):
            raise FlagError(f"Can't open flagfile {path}")
        self._flagfile_dirs.append(os.path.dirname(os.path.abspath(path)))
        args: List[str] = []
        with open(path) as f:
            for line in f:
                line = line.strip()
                if not line or line.startswith("#") or line.startswith("//"):
                    continue
                args.append(line)
        return args

    def parse(self, argv: Sequence[str], _depth: int = 0) -> List[str]:
        """Parses ``argv`` (without the program name); returns positional leftovers."""
        rest: List[str] = []
        i = 0
        argv = list(argv)
        while i < len(argv):
            a = argv[i]
            i += 1
            if a == "--":
                rest.extend(argv[i:])
                break
            if not a.startswith("-") or a == "-":
                rest.append(a)
                continue
            body = a.lstrip("-")
            name, eq, val = body.partition("=")
            if name == "flagfile":
                if not eq:
                    if i >= len(argv):
                        raise FlagError("--flagfile needs a path")
                    val = argv[i]
                    i += 1
                rest.extend(self.parse(self.read_flagfile(val.strip(), _depth), _depth + 1))
                continue
            d = self._defs.get(name)
            if d is None and name.startswith("no") and name[2:] in self._defs and \
                    self._defs[name[2:]].kind == "bool":
                if eq:
                    raise FlagError(f"--{name} does not take a value")
                self._set(name[2:], False)
                continue
            if d is None:
                raise FlagError(f"Unknown command line flag '{name}'")
            if d.kind == "bool":
                self._set(name, self._convert(d, val) if eq else True)
                continue
            if not eq:
                if i >= len(argv):
                    raise FlagError(f"Missing value for flag --{name}")
                val = argv[i]
                i += 1
            self._set(name, self._convert(d, val.strip()))
        return rest


def _D(name, kind, default, help="", choices=None):
    return FlagDef(name, kind, default, help, choices)


# train_ncsn.py:48-128 (same order)
TRAIN_FLAGS: List[FlagDef] = [
    _D("seed", "int", 0, "Random seed for network initialization."),
    _D("loss", "enum", "dsm", "Loss function.", ("dsm", "ssm", "ddpm")),
    _D("continuous_noise", "bool", True, "Continuous noise conditioning."),
    _D("learning_rate", "float", 3e-4, "Learning rate for optimizer."),
    _D("batch_size", "int", 128, "Batch size for training."),
    _D("epochs", "int", 10, "Number of training epochs."),
    _D("max_steps", "int", None, "Maximum number of training steps."),
    _D("early_stopping", "bool", False, "Use early stopping to prevent overfitting."),
    _D("grad_clip", "float", 1.0, "Max gradient norm for training."),
    _D("lr_gamma", "float", 0.98, "Gamma for learning rate scheduler."),
    _D("lr_schedule_interval", "int", 10000, "Number of steps between LR changes."),
    _D("architecture", "string", "TransformerDDPM", "Class name of model architecture."),
    _D("num_layers", "int", 6, "Number of encoder layers."),
    _D("num_heads", "int", 8, "Number of attention heads."),
    _D("num_mlp_layers", "int", 2, "Number of MLP layers."),
    _D("mlp_dims", "int", 2048, "Number of channels per MLP layer."),
    _D("sigma_begin", "float", 1.0, "Starting variance for noise schedule."),
    _D("sigma_end", "float", 1e-2, "Ending variance for noise schedule."),
    _D("schedule_type", "enum", "geometric", "Noise schedule configuration.", ("geometric", "linear", "fibonacci")),
    _D("num_sigmas", "int", 15, "Number of sigma values (L) in noise schedule."),
    _D("ld_steps", "int", 100, "Number of steps for annealed Langevin dynamics."),
    _D("ld_epsilon", "float", 2e-6, "Step size for annealed Langevin dynamics."),
    _D("sampling", "enum", "ald", "Sampling algorithm to use.", ("ald", "cas", "ddpm")),
    _D("ema", "bool", True, "Exponential moving average smoothing."),
    _D("mu", "float", 0.999, "Momentum parameter for EMA."),
    _D("denoise", "bool", True, "Add additional denoising step during sampling (Song et al., 2020)."),
    _D("data_shape", "list", ["2"], "Shape of data."),
    _D("problem", "enum", "toy", "Problem to solve.", ("toy", "mnist", "vae")),
    _D("dataset", "string", "./output/mix2d", "Path to directory containing data as train/eval tfrecord files."),
    _D("pca_ckpt", "string", "", "PCA transform."),
    _D("slice_ckpt", "string", "", "Slice transform."),
    _D("dim_weights_ckpt", "string", "", "Dimension scale transform."),
    _D("normalize", "bool", True, "Normalize dataset to [-1, 1]."),
    _D("logging_freq", "int", 100, "Logging frequency."),
    _D("snapshot_freq", "int", 5000, "Evaluation and checkpoint frequency."),
    _D("snapshot_sampling", "bool", True, "Sample from score network during evaluation."),
    _D("eval_samples", "int", 3000, "Number of samples to generate."),
    _D("checkpoints_to_keep", "int", 50, "Number of checkpoints to keep."),
    _D("save_ckpt", "bool", True, "Save model checkpoints at each evaluation step."),
    _D("model_dir", "string", "./save/ncsn", "Directory to store model data."),
    _D("verbose", "bool", True, "Toggle logging to stdout."),
]

# sample_ncsn.py:51-66
SAMPLE_FLAGS: List[FlagDef] = [
    _D("sample_seed", "int", 1, "Random number generator seed for sampling."),
    _D("sampling_dir", "string", "samples", "Sampling directory."),
    _D("sample_size", "int", 1000, "Number of samples."),
    _D("compute_metrics", "bool", False, "Compute evaluation metrics for generated samples."),
    _D("compute_final_only", "bool", False, "Do not include metrics for intermediate samples."),
    _D("flush", "bool", True, "Flush generated samples to disk."),
    _D("animate", "bool", False, "Generate animation of samples."),
    _D("infill", "bool", False, "Infill."),
    _D("interpolate", "bool", False, "Interpolate."),
]

# engine-only additions (no collision with the reference surface)
ENGINE_FLAGS: List[FlagDef] = [
    _D("dtype", "enum", "bf16", "GEMM operand precision of the HIP path: bf16, or fp8 = OCP e4m3 operands with per-row "
       "E8M0 scales for the DenseResBlock forward GEMMs and (training, --fp8_dgrad) their input-gradient GEMMs "
       "(BASELINE config 5); weight gradients and everything 128-wide stay bf16.  fp32 (sample_ncsn.py only): reference "
       "precision -- fp32 activations end to end and every Dense on the exact-fp32 MFMA from the fp32 master parameters; "
       "a checkpoint trained in bf16 / fp8 loads unchanged.  fp32 is an inference precision: train_ncsn.py refuses it.",
       ("bf16", "fp8", "fp32")),
    _D("fp8_dgrad", "bool", True, "--dtype=fp8 training: the four DenseResBlock dgrad GEMMs (dX = dY W^T) on e4m3 operands too "
       "(gradient parity 1.6e-2 vs 1.4e-2 with bf16 dgrads; recorded in the checkpoint metadata).  --nofp8_dgrad: bf16 dgrads."),
    _D("trunk_dtype", "enum", "bf16", "Storage type of the 2048-wide residual trunk between the DenseResBlocks DURING TRAINING: "
       "bf16 (default: +2 % train throughput; eps_hat parity 5.7e-3 -> 6.3e-3, loss curves indistinguishable over 400 steps, "
       "profiles/r3_trunk_dtype_curves.txt) or fp32 as the reference keeps it.  Logged at start-up and recorded in the "
       "checkpoint metadata; inference always uses bf16.", ("bf16", "fp32")),
    _D("dp_algorithm", "enum", "all_reduce", "Data-parallel gradient reduction (more than one rank): one all_reduce per bucket, or "
       "rs_ag = reduce_scatter + all_gather (one direct hop per phase on the 8-GPU xGMI mesh).", ("all_reduce", "rs_ag")),
    _D("dp_layer_buckets", "bool", False, "Data-parallel: reduce the encoder-stem gradients per layer in backward order, each "
       "collective started by the engine's per-layer gradient event instead of at the end of the backward pass."),
    _D("synthetic", "bool", False, "Use synthetic latents clip(0.25*N(0,1),-1,1) instead of --dataset."),
    _D("synthetic_examples", "int", 4096, "Synthetic examples per epoch."),
    _D("sample_ema", "bool", False, "sample_ncsn: sample from the EMA weights (reference uses raw weights)."),
    _D("nn_metrics", "bool", False, "sample_ncsn --compute_metrics: also compute the nearest-neighbour metrics improved_precision, "
       "improved_recall, improved_f1 and ipr_realism (Kynkaanniemi et al. 2019, DESIGN.md section 14)."),
    _D("nn_k", "int", 3, "--nn_metrics: the neighbour whose distance is a row's radius (1..8)."),
    _D("cluster_metrics", "bool", False, "sample_ncsn --compute_metrics: also compute the k-means metrics precision, recall, f1 (the "
       "PRD histogram of Sajjadi et al. 2018) and ndb (Richardson & Weiss 2018), DESIGN.md section 15."),
    _D("prd_clusters", "int", 20, "--cluster_metrics: clusters of the PRD histogram (2..128)."),
    _D("prd_runs", "int", 10, "--cluster_metrics: k-means runs the PRD curve is averaged over (1..100)."),
    _D("ndb_bins", "int", 50, "--cluster_metrics: bins of the NDB score (2..128)."),
    _D("copy_metrics", "bool", False, "sample_ncsn: search the training set for the nearest neighbours of every generated example "
       "and write {sampling_dir}/ncsn/copy_report.json (authenticity of Alaa et al. 2022, nearest-training distances against "
       "those of the eval examples, exact copies; frames and whole sequences) and nearest_train.pkl (DESIGN.md section 24)."),
    _D("copy_k", "int", 1, "--copy_metrics: training neighbours kept per generated row (1..8)."),
    _D("copy_train_examples", "int", 0, "--copy_metrics: search the first N training examples; 0 = all of them (--synthetic: as "
       "many as --sample_size)."),
    _D("graph", "bool", True, "Capture the sampling step in a hipGraph."),
    _D("ddim_steps", "int", 0, "sample_ncsn --sampling=ddpm: walk this many evenly spaced timesteps of the schedule with the strided "
       "(DDIM, Song et al. 2021) sampler instead of all --num_sigmas of them: 0 (off) or 2..num_sigmas network evaluations per "
       "sample from the same checkpoint (DESIGN.md section 16)."),
    _D("ddim_eta", "float", 0.0, "--ddim_steps: noise scale of the strided sampler, 0 = deterministic, 1 = the DDPM posterior's variance."),
    _D("ddim_encode", "bool", False, "--interpolate with --ddim_steps: encode starts and goals with the deterministic inversion of the "
       "strided sampler instead of the reference's single re-noising."),
    _D("compute_bound", "bool", False, "sample_ncsn --sampling=ddpm: evaluate the variational bound of Ho et al. 2020 on the eval "
       "examples, term by term, and write {sampling_dir}/ncsn/bound.json and bound_terms.pkl (DESIGN.md section 17)."),
    _D("bound_steps", "int", 0, "--compute_bound: 0 = every timestep (the bound itself, in bits/dim), else the per-timestep terms at "
       "2..num_sigmas evenly spaced timesteps only (the curve; no total)."),
    _D("bound_only", "bool", False, "--compute_bound: stop after writing the bound (no sampling run)."),
    _D("ddim_order", "int", 1, "--ddim_steps: order of the solver, 1 = the strided (DDIM) update, 2 = the second-order multistep "
       "update DPM-Solver++(2M) of Lu et al. 2022 (deterministic: --ddim_eta=0; DESIGN.md section 18)."),
    _D("ddim_spacing", "enum", "uniform", "--ddim_steps: the timesteps are evenly spaced in t (uniform) or in "
       "lambda = log(sqrt(ap) / sqrt(1 - ap)) snapped to timesteps (logsnr: at most --ddim_steps of them).", ("uniform", "logsnr")),
    _D("ddim_solver", "enum", "default", "--ddim_steps: default = the update --ddim_order names; adams3 = the third-order exponential "
       "Adams predictor in lambda on the clamped x0; adams3_pc = the same with a corrector that reuses every network evaluation "
       "to redo the previous step (no extra evaluations).  Deterministic (--ddim_eta=0), --ddim_order=1 left alone, meant for "
       "--ddim_spacing=logsnr (DESIGN.md section 29).", ("default", "adams3", "adams3_pc")),
    _D("analytic_variance", "enum", "none", "sample_ncsn --ddim_steps: give the noise of every iteration the optimal reverse variance of "
       "Bao et al. 2022 (Analytic-DPM) instead of sigma_eta^2, from an estimate of E[eps_hat^2] per timestep: none, scalar (one "
       "variance per iteration) or element (one per latent element; DESIGN.md section 28).  With --compute_bound (scalar only) "
       "bound.json gains the bound of the K-step chain.  Single process, --sampling=ddpm, --ddim_order=1.", ("none", "scalar", "element")),
    _D("analytic_examples", "int", 256, "--analytic_variance: examples the statistic is estimated on (the training split, else the eval "
       "examples; --synthetic: synthetic ones)."),
    _D("analytic_draws", "int", 1, "--analytic_variance: noise draws per example and timestep."),
    _D("analytic_moments", "string", "", "--analytic_variance: load the estimate from this file (a "
       "{sampling_dir}/ncsn/analytic_moments.safetensors of an earlier run) instead of estimating; a file whose metadata "
       "contradicts the run or whose timesteps do not cover the walk is refused."),
    _D("loss_weighting", "enum", "none", "train_ncsn --loss=ddpm: weight of every timestep in the loss, none (the reference) or "
       "min_snr = min(SNR, --min_snr_gamma) / SNR (Hang et al. 2023; DESIGN.md section 25).  Works on any number of ranks.",
       ("none", "min_snr")),
    _D("min_snr_gamma", "float", 5.0, "--loss_weighting=min_snr: the SNR above which a timestep's weight falls as gamma / SNR."),
    _D("timestep_sampler", "enum", "uniform", "train_ncsn --loss=ddpm: how training timesteps are drawn, uniform (the reference) "
       "or loss_second_moment = p_t ~ sqrt(E[L_t^2]) from a ten-deep loss history with the loss re-weighted by 1 / (n p_t) "
       "(Nichol & Dhariwal 2021; single process only; DESIGN.md section 25).", ("uniform", "loss_second_moment")),
    _D("distill_from", "string", "", "train_ncsn --loss=ddpm: progressive distillation (Salimans & Ho 2022; DESIGN.md section 27).  A "
       "safetensors checkpoint file, or a directory whose newest checkpoint is taken: the frozen teacher.  The student starts from "
       "its parameters and is trained so that one strided step lands where two of the teacher's land; its walk of --distill_steps "
       "timesteps is recorded in the checkpoint and sample_ncsn.py walks it.  The teacher's kind and walk come from its metadata; "
       "--prediction is the student's kind.  Single process, bf16, uniform timestep draw, --loss_weighting=none."),
    _D("distill_steps", "int", 0, "--distill_from: N, the student's number of sampler steps.  The teacher's walk must have 2N "
       "timesteps: evenly spaced ones for a teacher that was not distilled itself, else the walk its checkpoint records."),
    _D("distill_weighting", "enum", "truncated_snr", "--distill_from: loss weight of a student step, truncated_snr = max(SNR, 1) on "
       "the x-space error written in the student's output space, or none.", ("truncated_snr", "none")),
    _D("resume", "bool", False, "train_ncsn: start from the newest checkpoint under --model_dir (parameters, optimiser state, EMA, "
       "early stopping and, from a safetensors checkpoint, the timestep sampler's tables) instead of a fresh initialisation."),
    _D("ckpt_format", "enum", "safetensors", "Checkpoint file format written by train_ncsn: safetensors, or the "
       "reference's flax-0.3.0 msgpack state dict (both are recognised when restoring).", ("safetensors", "flax")),
    _D("rng_impl", "enum", "philox", "Random streams: the engine's fused Philox draws, or jax.random-compatible "
       "threefry2x32 streams (same --seed / --sample_seed => the reference's noise).", ("philox", "threefry")),
]


_PREDICTION_HELP = ("--loss=ddpm / --sampling=ddpm: what the network's output means, eps (the reference), x0, or "
                    "v = sqrt(ap) eps - sqrt(1 - ap) x0 (Salimans & Ho 2022; DESIGN.md section 26).  train_ncsn trains towards that "
                    "target (with --loss_weighting=min_snr: that kind's weight) and records the kind in a safetensors checkpoint; "
                    "--resume refuses another kind.  sample_ncsn: empty = what the checkpoint says, else eps; a value that "
                    "contradicts the checkpoint is refused.  --ckpt_format=flax has no place for the kind: the flag is then "
                    "REQUIRED to sample an x0 or v model.  The training log of an x0 / v run adds loss_eps, its unweighted loss in eps "
                    "units: compare it with an eps run's loss_unweighted (without --loss_weighting: its loss).")


def prediction_flag(include_sample: bool) -> FlagDef:
    """--prediction: an enum over eps, x0, v whose default is eps for train_ncsn and empty for sample_ncsn."""
    return _D("prediction", "enum", "" if include_sample else "eps", _PREDICTION_HELP,
              ("", "eps", "x0", "v") if include_sample else ("eps", "x0", "v"))


def make_flags(include_sample: bool = False) -> FlagValues:
    defs = list(TRAIN_FLAGS) + (list(SAMPLE_FLAGS) if include_sample else []) + list(ENGINE_FLAGS) + [prediction_flag(include_sample)]
    return FlagValues(defs)
