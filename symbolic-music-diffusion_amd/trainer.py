"""Optimisation step and data-parallel training for the DDPM path.

Mirrors train_ncsn.py:187-190 (create_optimizer), :206-257 (eval_step / evaluate), :260-288
(train_step) on top of the HIP engine, and adds what the reference does not have:
data-parallel training, one process per GPU, gradients summed with RCCL all-reduce over xGMI
(torch.distributed backend "nccl") in two buckets overlapped with the stem backward.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

from .engine import Engine
from .jax_random import ThreefryKey, diffusion_loss_draws, diffusion_loss_used_alphas
from .ncsn import (Model, PRNGKey, _dsm_draws, _ensure_any_schedule, _ensure_schedule, denoising_score_matching_loss,
                   diffusion_loss)


@dataclass
class Hyper:
    """Flags that shape the update (train_ncsn.py:53,61-63,94-96)."""
    learning_rate: float = 3e-4
    grad_clip: float = 1.0
    lr_gamma: float = 0.98
    lr_schedule_interval: int = 10000
    ema: bool = True
    mu: float = 0.999


class Optimizer:
    """flax.optim.Optimizer stand-in (train_ncsn.py:187-190): ``target`` is the model, the Adam
    moments / step counter / EMA live in the training engine's flat buffers."""

    def __init__(self, model: Model, learning_rate: float, ema: bool = False):
        self.target = model
        self.learning_rate = learning_rate
        self.engine: Engine = model.train_engine(ema)
        if ema and self.engine.ema is None:
            self.engine.ema = self.engine.params.clone()      # engine was created without EMA: rebind
            from . import lib as _lib
            e = self.engine
            _lib.check(e.L.smd_engine_bind_train(e.h, e.grads.data_ptr(), e.m.data_ptr(), e.v.data_ptr(),
                                                 e.ema.data_ptr(), e.step_counter.data_ptr(), e.metrics.data_ptr()))

    @property
    def step(self) -> int:
        return int(self.engine.step_counter.item())

    def state_dict(self) -> Dict[str, torch.Tensor]:
        e = self.engine
        return {"params": e.params, "adam_m": e.m, "adam_v": e.v, "step": e.step_counter,
                **({"ema": e.ema} if e.ema is not None else {})}


def create_optimizer(model: Model, learning_rate: float, ema: bool = False) -> Optimizer:
    """train_ncsn.py:187-190 (optim.Adam(learning_rate).create(model))."""
    return Optimizer(model, learning_rate, ema)


class LazyMetrics(dict):
    """Metrics stay on the device until somebody formats them (no per-step host sync)."""

    def resolve(self) -> Dict[str, float]:
        return {k: (float(v) if torch.is_tensor(v) else v) for k, v in self.items()}


LOSS_WEIGHTINGS = ("none", "min_snr")
PREDICTIONS = ("eps", "x0", "v")           # schedule.PREDICTIONS: what the network's output means
TIMESTEP_SAMPLERS = ("uniform", "loss_second_moment")


def validate_training_options(loss: str = "ddpm", loss_weighting: str = "none", timestep_sampler: str = "uniform",
                              world_size: int = 1, prediction: str = "eps", sampling: str = "ddpm") -> None:
    """The combinations of --loss / --loss_weighting / --timestep_sampler / --prediction / --sampling this engine trains (DESIGN.md
    sections 25, 26); anything else raises a ValueError that says what is refused.  train_ncsn.py calls this before it touches a
    device."""
    if prediction not in PREDICTIONS:
        raise ValueError(f"--prediction must be one of {PREDICTIONS}, got {prediction!r}")
    if prediction != "eps" and loss != "ddpm":
        raise ValueError(f"--prediction={prediction} applies to --loss=ddpm only (got --loss={loss}): x0- and v-prediction are "
                         "parameterisations of the DDPM network; the score-matching losses (--loss=dsm, --loss=ssm) train a score")
    if prediction != "eps" and sampling != "ddpm":
        raise ValueError(f"--prediction={prediction} needs --sampling=ddpm (got --sampling={sampling}): the Langevin samplers "
                         "(--sampling=ald, --sampling=cas) take the network's output as a score")
    if loss_weighting not in LOSS_WEIGHTINGS:
        raise ValueError(f"--loss_weighting must be one of {LOSS_WEIGHTINGS}, got {loss_weighting!r}")
    if timestep_sampler not in TIMESTEP_SAMPLERS:
        raise ValueError(f"--timestep_sampler must be one of {TIMESTEP_SAMPLERS}, got {timestep_sampler!r}")
    if loss != "ddpm" and (loss_weighting != "none" or timestep_sampler != "uniform"):
        raise ValueError(f"--loss_weighting={loss_weighting} / --timestep_sampler={timestep_sampler} apply to --loss=ddpm only "
                         f"(got --loss={loss}): the weights are defined for the DDPM loss (of any --prediction)")
    if timestep_sampler == "loss_second_moment" and world_size > 1:
        raise ValueError(f"--timestep_sampler=loss_second_moment is single-process only (world size {world_size}): every rank "
                         "would need the labels and losses of the whole batch (an all-gather per step) to keep the tables "
                         "equal; run one process, or --timestep_sampler=uniform (--loss_weighting=min_snr works on any "
                         "number of ranks)")


class TimestepSampler:
    """The loss-second-moment timestep resampler of Nichol & Dhariwal 2021 on the device: timesteps are
    drawn with p_t ~ sqrt(E[L_t^2]) from a ten-deep history of per-timestep losses (uniform until every timestep has ten), and
    the loss is re-weighted by 1 / (n p_t) so that the objective stays the uniform one in expectation.

    ``n`` timesteps starting at ``label_base``: the range of the run's uniform label draw -- ``for_schedule`` takes it from
    (len(sigmas), continuous_noise) exactly as q-sample does (labels in [label_min, label_min + T), utils/losses.py:272-275).
    The tables (history [n][10], counts [n], p [n], cdf [n]) live on the device and are touched by two kernels only
    (include/smd_hip.h smd_timestep_draw / smd_timestep_update): no host synchronisation per step."""

    DEPTH = 10
    STATE_KEYS = ("history", "counts", "p", "cdf")

    def __init__(self, n: int, label_base: int, device, uniform_mix: float = 1e-3):
        if n <= 0:
            raise ValueError(f"TimestepSampler: n={n}")
        self.n, self.label_base, self.uniform_mix = int(n), int(label_base), float(uniform_mix)
        self.device = torch.device(device)
        self.history = torch.zeros(self.n, self.DEPTH, dtype=torch.float32, device=self.device)
        self.counts = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        self.p = torch.full((self.n,), 1.0 / self.n, dtype=torch.float32, device=self.device)
        self.cdf = torch.cumsum(self.p.double(), 0).float()
        self._warmed = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.last_labels: Optional[torch.Tensor] = None      # what the last draw() returned (tests, logging)
        self.last_iw: Optional[torch.Tensor] = None

    @classmethod
    def for_schedule(cls, sigmas, continuous_noise: bool, device, uniform_mix: float = 1e-3) -> "TimestepSampler":
        # the engine's label draw: label_min + r % T with T = len(sigmas), label_min = 1 with continuous noise else 0
        # (csrc/diffusion.hip q_sample; jax_random.diffusion_loss_draws: randint(cn, T + cn))
        return cls(len(sigmas), 1 if continuous_noise else 0, device, uniform_mix)

    @property
    def warmed(self) -> bool:
        """Every timestep has ten losses (reads one int back: synchronises)."""
        return bool(self._warmed.item())

    def draw(self, B: int, rng, step: Optional[int] = None, sample_offset: int = 0, *, global_batch: Optional[int] = None,
             u: Optional[torch.Tensor] = None, step_ptr: Optional[torch.Tensor] = None):
        """(labels int32 [B], iw float32 [B]) for the samples [sample_offset, sample_offset + B) of the global batch: keyed by the
        global sample index, so a shard draws what the whole batch would.  Philox keys: the uniforms come from the engine's
        stream SMD_STREAM_TIMESTEP at (seed, sample, step); ``step_ptr`` (a device uint32, e.g. the optimiser's step counter)
        replaces ``step``.  A ThreefryKey: u = jax.random.uniform(split(rng, 4)[3], (global_batch,)) -- the reference has no such
        draw; its loss uses split(rng, 3).  ``u`` passes the uniforms explicitly."""
        from . import jax_random as _jr
        from . import lib as _lib
        labels = torch.empty(B, dtype=torch.int32, device=self.device)
        iw = torch.empty(B, dtype=torch.float32, device=self.device)
        seed = 0
        if u is not None:
            u = torch.as_tensor(u).to(self.device, torch.float32).contiguous()
            if u.numel() != B:
                raise ValueError(f"TimestepSampler.draw: u has {u.numel()} entries for batch {B}")
        elif isinstance(rng, ThreefryKey):
            gb = B if global_batch is None else int(global_batch)
            u = _jr.uniform(_jr.split(rng, 4)[3], (B,), self.device, n_total=gb, offset=sample_offset)
        else:
            seed = int(rng.seed)
        with torch.cuda.device(self.device):
            _lib.check(_lib.get_lib().smd_timestep_draw(
                self.cdf.data_ptr(), self.p.data_ptr(), self.n, self.label_base, B, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF,
                int(sample_offset), int(step or 0) & 0xFFFFFFFF, None if step_ptr is None else step_ptr.data_ptr(),
                None if u is None else u.data_ptr(), labels.data_ptr(), iw.data_ptr(),
                torch.cuda.current_stream().cuda_stream), "timestep_draw")
        self.last_labels, self.last_iw = labels, iw
        return labels, iw

    def update(self, labels: torch.Tensor, loss: torch.Tensor) -> None:
        """Feeds the (label, unweighted per-sample loss) pairs of a WHOLE batch, in sample order, into the history and
        refreshes p and cdf."""
        from . import lib as _lib
        labels = torch.as_tensor(labels).to(self.device, torch.int32).contiguous()
        loss = torch.as_tensor(loss).to(self.device, torch.float32).contiguous()
        if labels.numel() != loss.numel() or labels.numel() == 0:
            raise ValueError(f"TimestepSampler.update: {labels.numel()} labels for {loss.numel()} losses")
        with torch.cuda.device(self.device):
            _lib.check(_lib.get_lib().smd_timestep_update(
                labels.data_ptr(), loss.data_ptr(), labels.numel(), self.history.data_ptr(), self.counts.data_ptr(), self.n,
                self.label_base, self.uniform_mix, self.p.data_ptr(), self.cdf.data_ptr(), self._warmed.data_ptr(),
                torch.cuda.current_stream().cuda_stream), "timestep_update")

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {k: getattr(self, k).detach().cpu().clone() for k in self.STATE_KEYS}

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        for k in self.STATE_KEYS:
            dst, src = getattr(self, k), torch.as_tensor(sd[k])
            if tuple(src.shape) != tuple(dst.shape):
                raise ValueError(f"TimestepSampler.load_state_dict: {k} has shape {tuple(src.shape)}, this sampler {tuple(dst.shape)} "
                                 "(another --num_sigmas?)")
            dst.copy_(src.to(dst.dtype))
        self._warmed.copy_((self.counts >= self.DEPTH).all().to(torch.int32).reshape(1))


def loss_in_eps_units(loss_per_sample: torch.Tensor, noise_level: torch.Tensor, prediction: str = "eps") -> torch.Tensor:
    """The batch mean of f_b loss_b: the unweighted per-sample loss of an x0- / v-predicting network in the units of an eps loss,
    so runs of different kinds can be compared.  With ap = noise_level^2, at fixed x_t:
    x0_hat - x0 = -(sqrt(1 - ap) / sqrt(ap)) (eps_hat - eps) and v_hat - v = (eps_hat - eps) / sqrt(ap), so f = 1 for eps,
    ap / (1 - ap) for x0 and ap for v.  Samples with ap = 1 (label 1: x_t is x0 itself, an x0 estimate says nothing about eps) are
    left out of the x0 mean; a mean over no sample is 0.  Computed on the device in float64 from [B] values: no kernel of its own."""
    if prediction not in PREDICTIONS:
        raise ValueError(f"prediction must be one of {PREDICTIONS}, got {prediction!r}")
    loss = loss_per_sample.double()
    if prediction == "eps":
        return loss.mean().float()
    ap = noise_level.double() ** 2
    if prediction == "v":
        return (ap * loss).mean().float()
    keep = ap < 1.0
    f = torch.where(keep, ap / torch.where(keep, 1.0 - ap, torch.ones_like(ap)), torch.zeros_like(ap))
    return ((f * loss).sum() / keep.sum().clamp(min=1)).float()


def train_step(objective, batch, optimizer: Optimizer, sigmas, rng: PRNGKey, learning_rate: float, *,
               grad_clip: float = 1.0, mu: float = 0.999, labels=None, eps=None, comm: "Optional[GradComm]" = None,
               lr_gamma: float = 1.0, lr_interval: int = 1, sample_offset: int = 0,
               global_batch: Optional[int] = None, continuous_noise: bool = True, used_alphas=None,
               loss_weighting: str = "none", min_snr_gamma: float = 5.0,
               timestep_sampler: "Optional[TimestepSampler]" = None, loss_weights=None, prediction: str = "eps"):
    """train_ncsn.py:260-288: value_and_grad(mean diffusion_loss) -> clip_grads -> Adam
    (+ EMA, fused).  ``learning_rate`` is the step's LR as in the reference; pass ``lr_gamma`` /
    ``lr_interval`` instead to let the kernel evaluate the stepped schedule from its own step
    counter (learning_rate is then lr0).  ``continuous_noise`` is FLAGS.continuous_noise (:278): False draws the labels
    in [0, T) and gives label 0 its real uniform noise level (utils/losses.py:272-286).  Returns (optimizer, metrics{'loss','grad','lr'}).

    ``objective``: ``diffusion_loss`` / ``denoising_score_matching_loss`` of this package run fused (q-sample, forward, loss and
    backward as one engine call).  ANY other callable ``objective(batch, model, sigmas, rng, continuous_noise, 'mean')`` written in
    torch is differentiated as the reference differentiates it (jax.value_and_grad, :279-283): ``model`` is then a
    ``DifferentiableModel`` whose ``model(x, cond)`` runs the engine's forward and whose autograd backward is the engine's backward
    pass from d objective / d eps_hat (one model call per objective; second-order objectives like 'ssm' are not supported).

    Weighted training (``objective is diffusion_loss`` only): ``loss_weighting="min_snr"`` weights every
    sample by min(SNR, min_snr_gamma) / SNR of its noise level, ``timestep_sampler`` (a TimestepSampler) draws the labels from
    its loss-aware table, weights the samples by 1 / (n p) and is fed the step's per-sample losses; ``loss_weights`` ([B]) passes
    importance weights explicitly.  metrics['loss'] is then the weighted objective that is optimised, mean(w loss), and
    metrics['loss_unweighted'] the plain mean.  With the defaults nothing changes.

    ``prediction`` "x0" / "v" (``objective is diffusion_loss`` only): the network's output is compared with
    x0 / v = s eps - sqrt(1 - s^2) x0 and min_snr weights by min(SNR, gamma) / min(SNR, gamma) / (SNR + 1).  metrics['loss'] and
    ['loss_unweighted'] are then in that output's space, and metrics['loss_eps'] is the unweighted loss in eps units
    (``loss_in_eps_units``): what an eps run reports as its unweighted loss, so runs of different kinds can be compared."""
    if prediction not in PREDICTIONS:
        raise ValueError(f"train_step: prediction must be one of {PREDICTIONS}, got {prediction!r}")
    if prediction != "eps" and objective is not diffusion_loss:
        raise ValueError(f"train_step: prediction={prediction!r} applies to objective=diffusion_loss (the DDPM loss) only, got "
                         f"{getattr(objective, '__name__', objective)!r}")
    if loss_weighting not in LOSS_WEIGHTINGS:
        raise ValueError(f"train_step: loss_weighting must be one of {LOSS_WEIGHTINGS}, got {loss_weighting!r}")
    weighted = loss_weighting != "none" or timestep_sampler is not None or loss_weights is not None
    if weighted and objective is not diffusion_loss:
        raise ValueError("train_step: loss_weighting / timestep_sampler / loss_weights apply to objective=diffusion_loss (the DDPM "
                         f"loss) only, got {getattr(objective, '__name__', objective)!r}")
    if timestep_sampler is not None and comm is not None and comm.world_size > 1:
        raise ValueError(f"train_step: a timestep_sampler is single-process only (world size {comm.world_size}): its tables need "
                         "the labels and losses of the whole batch")
    eng = optimizer.engine
    batch = torch.as_tensor(batch).to(eng.device, torch.float32).contiguous()
    if objective is not diffusion_loss and objective is not denoising_score_matching_loss:
        return _train_step_generic(objective, batch, optimizer, sigmas, rng, learning_rate, grad_clip=grad_clip, mu=mu, comm=comm,
                                   lr_gamma=lr_gamma, lr_interval=lr_interval, continuous_noise=continuous_noise)
    dsm = objective is denoising_score_matching_loss
    if dsm:
        eng.set_prediction("eps")
        _ensure_any_schedule(eng)
    else:
        _ensure_schedule(eng, sigmas, with_sampler=False, prediction=prediction)
    eng.bind(batch.shape[0], training=True)
    lab = None if labels is None else torch.as_tensor(labels).to(eng.device, torch.int32).contiguous()
    e = None if eps is None else torch.as_tensor(eps).to(eng.device, torch.float32).contiguous()
    world = 1 if comm is None else comm.world_size
    gb = batch.shape[0] * world if global_batch is None else global_batch
    ua = None if used_alphas is None else torch.as_tensor(used_alphas).to(eng.device, torch.float32).contiguous()
    iw = None
    if dsm:
        # utils/losses.py:149-164: the noise level travels per sample (used_alphas carries the used_sigmas)
        sig = torch.as_tensor(np.asarray(sigmas, dtype=np.float32)).to(eng.device)
        if ua is None and lab is not None:
            ua = (sig[(lab.long() - 1) % len(sig)] if continuous_noise else sig[lab.long()]).contiguous()
        elif ua is None:
            _lab, ua, e2 = _dsm_draws(rng, tuple(batch.shape), sig, bool(continuous_noise), sample_offset, gb)
            e = e if e is not None else e2
        lab = None
    elif isinstance(rng, ThreefryKey) and lab is None and e is None:
        # the reference's own draws (utils/losses.py:271-294) for this rank's rows of the global batch
        lab, e = diffusion_loss_draws(rng, tuple(batch.shape), len(sigmas), eng.device, sample_offset=sample_offset,
                                      global_batch=gb, continuous_noise=continuous_noise)
        if timestep_sampler is not None:
            # the sampler's labels replace the uniform ones (eps stays the reference's draw); the step key is the step: no counter
            lab, iw = timestep_sampler.draw(batch.shape[0], rng, sample_offset=sample_offset, global_batch=gb)
        if not continuous_noise and ua is None:
            ua = diffusion_loss_used_alphas(rng, lab, eng._sched_tensors["ape"], sample_offset=sample_offset,
                                            global_batch=gb)
    elif timestep_sampler is not None and lab is None:
        # keyed like q-sample's own label draw: (seed, global sample index, the optimiser's step counter read on the device)
        lab, iw = timestep_sampler.draw(batch.shape[0], rng, sample_offset=sample_offset, global_batch=gb,
                                        step_ptr=None if isinstance(rng, ThreefryKey) else eng.step_counter)
    kw = dict(seed=rng.seed, sample_offset=sample_offset, global_batch=gb, used_alphas=ua, continuous_noise=continuous_noise,
              objective="dsm" if dsm else "ddpm")
    if weighted:
        if loss_weights is not None:
            iw = torch.as_tensor(loss_weights).to(eng.device, torch.float32).contiguous()
            if iw.numel() != batch.shape[0]:
                raise ValueError(f"train_step: loss_weights has {iw.numel()} entries for batch {batch.shape[0]}")
        kw.update(loss_weights=iw, min_snr_gamma=float(min_snr_gamma) if loss_weighting == "min_snr" else 0.0)
        if iw is None and not kw["min_snr_gamma"] > 0.0:
            raise ValueError(f"train_step: loss_weighting='min_snr' needs min_snr_gamma > 0 (inf: no SNR factor), got {min_snr_gamma}")
    # optimiser placement (engine option "opt_overlap"): 0 = the whole sweep on this stream.  Deferring the
    # output-stage slice to the side stream (bit 0) measured +1 % at best on a process's FIRST training engine and HALVED the
    # step rate of every second later engine of the same process (profiles/r4q_extras_opt_overlap.txt: the per-step
    # main-waits-on-side / side-waits-on-main pattern on whatever hardware queue the new side stream is mapped to), so it is
    # opt-in: SMD_OPT_OVERLAP=3 (1 with a communicator).
    eng.set_opt_overlap(0)
    if comm is None:
        eng.loss_backward(batch, lab, e, stage=0, **kw)
    else:
        layered = comm.layer_buckets and batch.is_cuda and eng.head_offset > 0
        if layered != getattr(eng, "_dp_layer_events", False):
            eng.set_option("dp_layer_events", int(layered))
            eng._dp_layer_events = layered
        eng.loss_backward(batch, lab, e, stage=1, **kw)
        comm.reduce_async(eng.grads[eng.head_offset:])          # output-stage gradients are final
        eng.loss_backward(None, None, None, stage=2, **kw)
        if layered:
            # the stem slice in backward order, one collective per encoder layer: layer l's starts behind the event the engine
            # recorded when ITS gradients became final, not behind the whole stem backward; the last bucket (in_proj + layer 0)
            # waits for the stream as before
            g = eng.grads
            buckets = eng.grad_buckets()
            for b, (off, ln) in enumerate(buckets):
                early = b + 1 < len(buckets)
                comm.reduce_async(g[off:off + ln], after=(lambda s, b=b: eng.wait_grad_bucket(b, s)) if early else None)
        else:
            comm.reduce_async(eng.grads[:eng.head_offset])
        comm.wait()
    # gradients were scaled by 1/(global_batch*S*C) at the loss, so the all-reduce SUM is the global mean
    eng.optimizer_step(learning_rate, lr_gamma, lr_interval, grad_clip, mu, 1.0)
    per_sample = eng.loss_per_sample()
    loss = per_sample.mean()
    metrics = LazyMetrics(loss=loss, grad=eng.metrics[1], lr=eng.metrics[2])
    if weighted or prediction != "eps":
        # the objective that was optimised, from the weights the loss kernel wrote; the plain mean stays comparable between runs
        # (an x0 / v step always runs the weighted kernel: unweighted, every weight is exactly 1)
        metrics["loss"] = (eng.weight_per_sample() * per_sample).mean()
        metrics["loss_unweighted"] = loss
        if prediction != "eps":        # (an eps run's loss_unweighted -- unweighted: its loss -- is already in eps units)
            metrics["loss_eps"] = loss_in_eps_units(per_sample, eng.noise_level_per_sample(), prediction)
        if timestep_sampler is not None:
            timestep_sampler.update(lab, per_sample)         # the UNWEIGHTED per-sample losses, in sample order
    return optimizer, metrics


def _train_step_generic(objective, batch, optimizer: Optimizer, sigmas, rng, learning_rate, *, grad_clip, mu, comm, lr_gamma,
                        lr_interval, continuous_noise):
    """train_ncsn.py:279-287 for an arbitrary objective: torch autograd over ``objective`` with the engine's forward / backward
    underneath (ops.py smd_amd::eps_forward_train), then the same fused clip + Adam (+ EMA) sweep as the fused objectives."""
    eng = optimizer.engine
    dm = getattr(optimizer, "_differentiable", None)
    if dm is None:
        dm = optimizer._differentiable = optimizer.target.differentiable(ema=eng.ema is not None)
    eng.set_opt_overlap(0)
    dm.params.grad = None
    with torch.enable_grad():
        loss = objective(batch, dm, sigmas, rng, continuous_noise, "mean")
    if not (torch.is_tensor(loss) and loss.requires_grad and loss.numel() == 1):
        raise ValueError("train_step: objective(batch, model, sigmas, rng, continuous_noise, 'mean') must return a scalar tensor "
                         "computed from model(x, cond)")
    eng._grad_alias_ok = True               # params.grad is None and is consumed below: eps_backward may hand autograd the buffer itself
    try:
        loss.backward()
    finally:
        eng._grad_alias_ok = False
    if dm.params.grad is None:
        raise ValueError("train_step: the objective did not reach the model's parameters")
    # the engine's gradient buffer holds the last backward pass; autograd's accumulated leaf gradient is the authoritative one
    # (it may BE the engine's buffer: under _grad_alias_ok eps_backward returns an alias that autograd can adopt)
    if dm.params.grad.data_ptr() != eng.grads.data_ptr():
        eng.grads.copy_(dm.params.grad)
    dm.params.grad = None
    world = 1
    if comm is not None:
        world = comm.world_size
        comm.reduce_async(eng.grads)
        comm.wait()
    eng.optimizer_step(learning_rate, lr_gamma, lr_interval, grad_clip, mu, 1.0 / world)     # the objective's mean is per rank
    return optimizer, LazyMetrics(loss=loss.detach(), grad=eng.metrics[1], lr=eng.metrics[2])


# ------------------------------------------------------------------ progressive distillation
from .schedule import DISTILL_WEIGHTINGS  # noqa: E402  (one list: the flag's enum, the tables' check)


def validate_distill_options(loss: str = "ddpm", loss_weighting: str = "none", timestep_sampler: str = "uniform",
                             world_size: int = 1, dtype: str = "bf16", ckpt_format: str = "safetensors",
                             distill_weighting: str = "truncated_snr", distill_steps: int = 0) -> None:
    """The combinations --distill_from is trained with; anything else raises a ValueError that says what is refused.
    train_ncsn.py calls this before it touches a device."""
    if loss != "ddpm":
        raise ValueError(f"--distill_from applies to --loss=ddpm only (got --loss={loss}): the teacher's two strided steps are "
                         "steps of the DDPM sampler")
    if timestep_sampler != "uniform":
        raise ValueError(f"--distill_from draws the student's steps uniformly: --timestep_sampler={timestep_sampler} is refused")
    if loss_weighting != "none":
        raise ValueError(f"--distill_from takes its loss weight from --distill_weighting: --loss_weighting={loss_weighting} is "
                         "refused")
    if ckpt_format == "flax":
        raise ValueError("--distill_from needs --ckpt_format=safetensors: the student's walk is recorded in the safetensors "
                         "metadata, which a flax checkpoint does not have")
    if world_size > 1:
        raise ValueError(f"--distill_from is single-process only (world size {world_size}): the distillation step has no "
                         "gradient all-reduce")
    if dtype != "bf16":
        raise ValueError(f"--distill_from trains the student in bf16 (got --dtype={dtype})")
    if distill_weighting not in DISTILL_WEIGHTINGS:
        raise ValueError(f"--distill_weighting must be one of {DISTILL_WEIGHTINGS}, got {distill_weighting!r}")
    if int(distill_steps) < 1:
        raise ValueError(f"--distill_from needs --distill_steps=N with N >= 1 (the student's number of sampler steps), got "
                         f"{distill_steps}")


class DistillTables:
    """What one round of progressive distillation needs from the schedule, on the device: the [N][16] table of
    ``schedule.distill_tables`` and a uniform (p, cdf) over the student's N steps for ``smd_timestep_draw``.  ``teacher_walk``
    (2N timesteps) and ``student_walk`` (N) are the host lists; ``ref`` holds the table's float64 originals."""

    def __init__(self, betas, teacher_walk, teacher_prediction: str, student_prediction: str, weighting: str = "truncated_snr",
                 device="cuda:0", clip: float = 1.0):
        from . import schedule as _sched
        self.betas = np.asarray(betas, dtype=np.float32)
        if len(teacher_walk) % 2:
            raise ValueError(f"DistillTables: a teacher walk has an even number of timesteps, got {len(teacher_walk)}")
        tw, sw = _sched.distill_walk(len(self.betas), len(teacher_walk) // 2, teacher_walk)
        self.teacher_walk, self.student_walk = [int(t) for t in tw], [int(t) for t in sw]
        self.teacher_prediction = _sched.PREDICTIONS[_sched.prediction_kind(teacher_prediction)]
        self.student_prediction = _sched.PREDICTIONS[_sched.prediction_kind(student_prediction)]
        self.weighting = weighting
        self.host, self.ref = _sched.distill_tables(self.betas, tw, self.teacher_prediction, self.student_prediction, weighting, clip)
        self.N = len(sw)
        self.device = torch.device(device)
        self.table = torch.from_numpy(self.host).to(self.device)
        self.p = torch.full((self.N,), 1.0 / self.N, dtype=torch.float32, device=self.device)
        self.cdf = torch.cumsum(self.p.double(), 0).float()

    def draw(self, B: int, seed: int, sample_offset: int = 0, step_ptr: Optional[torch.Tensor] = None) -> torch.Tensor:
        """int32 [B] steps in [0, N), uniform: Philox keyed by (seed, b + sample_offset, *step_ptr) on the timestep stream"""
        from . import lib as _lib
        steps = torch.empty(B, dtype=torch.int32, device=self.device)
        if getattr(self, "_iw", None) is None or self._iw.numel() != B:       # the entry point always writes the weights: all 1 here
            self._iw = torch.empty(B, dtype=torch.float32, device=self.device)
        iw = self._iw
        with torch.cuda.device(self.device):
            _lib.check(_lib.get_lib().smd_timestep_draw(
                self.cdf.data_ptr(), self.p.data_ptr(), self.N, 0, B, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF,
                int(sample_offset), 0, None if step_ptr is None else step_ptr.data_ptr(), None, steps.data_ptr(), iw.data_ptr(),
                torch.cuda.current_stream().cuda_stream), "timestep_draw")
        return steps


def distill_step(batch, optimizer: Optimizer, teacher: Model, tables: DistillTables, rng: PRNGKey, learning_rate: float, *,
                 steps=None, eps=None, loss_weights=None, prediction: Optional[str] = None, grad_clip: float = 1.0,
                 mu: float = 0.999, lr_gamma: float = 1.0, lr_interval: int = 1):
    """One optimisation step of progressive distillation (Salimans & Ho 2022): the student
    (``optimizer.target``) is trained so that ONE strided step from z_t at level t = walk[2k] lands where the frozen ``teacher``'s
    TWO strided steps t -> m -> u land.  On one stream: draw the steps k (unless ``steps`` int32 [B] is given), noise the batch to
    z_t (``eps`` given or Philox), teacher(z_t), the teacher's first step, teacher(z_m), student(z_t) in the training workspace,
    target + loss + d loss / d pred, the student's backward pass, the fused clip + Adam (+ EMA) sweep.  ``teacher`` is an inference
    model with parameters of its own; it is read only.  ``prediction`` is the student's kind (default: the tables').
    ``loss_weights`` [B] multiplies the tables' per-step weight.  Returns (optimizer, metrics {'loss' (weighted),
    'loss_unweighted', 'grad', 'lr'}) as LazyMetrics: nothing synchronises with the host."""
    from . import engine as _eng
    from . import schedule as _sched
    eng = optimizer.engine
    kind = tables.student_prediction if prediction is None else _sched.PREDICTIONS[_sched.prediction_kind(prediction)]
    if kind != tables.student_prediction:
        raise ValueError(f"distill_step: prediction={kind!r}, but the tables carry the loss weights of a {tables.student_prediction!r} "
                         "student")
    if eng.cfg.dtype != "bf16":
        raise ValueError(f"distill_step: the student trains in bf16, got dtype={eng.cfg.dtype!r}")
    if teacher.engine.params.data_ptr() == eng.params.data_ptr():
        raise ValueError("distill_step: the teacher shares the student's parameter buffer; it needs a frozen copy of its own")
    if tuple(teacher.cfg.sample_shape) != tuple(eng.cfg.sample_shape):
        raise ValueError(f"distill_step: teacher samples {teacher.cfg.sample_shape}, student samples {eng.cfg.sample_shape}")
    batch = torch.as_tensor(batch).to(eng.device, torch.float32).contiguous()
    B = batch.shape[0]
    eng.set_prediction(kind)
    eng.set_opt_overlap(0)
    if steps is None:
        k = tables.draw(B, int(rng.seed), step_ptr=eng.step_counter)
    else:
        k = torch.as_tensor(steps).to(eng.device, torch.int32).contiguous()
    e = None if eps is None else torch.as_tensor(eps).to(eng.device, torch.float32).contiguous()
    iw = None if loss_weights is None else torch.as_tensor(loss_weights).to(eng.device, torch.float32).contiguous()
    z_t, level_t, _ = _eng.distill_noise(batch, tables.table, k, e, seed=int(rng.seed), step_ptr=eng.step_counter)
    out1 = teacher.engine.forward(z_t, level_t)
    x1, z_m, level_m = _eng.distill_mid(z_t, out1, tables.table, k)
    out2 = teacher.engine.forward(z_m, level_m)
    pred = eng.forward_train(z_t, level_t)
    inv = 1.0 / (B * float(np.prod(eng.cfg.sample_shape)))
    per_sample, weight, dpred, _ = _eng.distill_loss(x1, z_m, out2, z_t, pred, tables.table, k, kind, inv, iw)
    eng.backward_from(dpred)
    eng.optimizer_step(learning_rate, lr_gamma, lr_interval, grad_clip, mu, 1.0)
    return optimizer, LazyMetrics(loss=(weight * per_sample).mean(), loss_unweighted=per_sample.mean(), grad=eng.metrics[1],
                                  lr=eng.metrics[2])


def eval_step(objective, batch, model: Model, sigmas, rng: PRNGKey, continuous_noise: bool = True):
    """train_ncsn.py:206-221: summed loss of one batch."""
    return objective(batch, model, sigmas, rng, continuous_noise, "sum")


def evaluate(dataset, model: Model, sigmas, rng: PRNGKey, continuous_noise: bool = True, objective=diffusion_loss):
    """train_ncsn.py:224-257: mean per-example loss over the dataset (iterable of batches)."""
    from .ncsn import split
    count, total = 0, 0.0
    for inputs in dataset:
        count += inputs.shape[0]
        rng, eval_rng = split(rng)
        total += float(eval_step(objective, inputs, model, sigmas, eval_rng, continuous_noise))
    return {"loss": total / max(count, 1)}


class GradComm:
    """Gradient reduction on a side stream (RCCL when the tensors are on GPUs, gloo in the CPU tests); SUM (the loss
    already carries 1/global_count).  Every rank ends with bitwise the same reduced gradient in every mode.

    ``buckets``: every reduce_async(flat) is cut into this many contiguous chunks, each its own collective, so the ring
    starts moving the first chunk while later ones are still queued (xGMI is point-to-point: a ring all-reduce is
    per-link bound, ~153 GB/s, and a 100 MB fp32 gradient is ~1.3 ms of wire time at 8 ranks however it is cut; smaller
    chunks only shorten the pipeline fill).  ``payload="bf16"``: the chunk is rounded to bf16 into a persistent staging
    buffer, reduced in bf16 and widened back in place -- half the bytes on the links for ~2^-9 relative rounding per
    addend; off by default because the reference reduces fp32 (jax.lax.pmean, train_ncsn.py:282).
    ``algorithm="rs_ag"``: reduce_scatter + all_gather instead of all_reduce -- on the 8-GPU xGMI mesh every GPU has a direct
    link to every other, so each of the two phases is ONE hop of n/8 per peer over 7 links in parallel
    where a ring makes 2 x 7 dependent hops; which one RCCL's own all_reduce picks is its tuning, this makes it a choice.
    ``layer_buckets``: the stem slice is reduced per encoder layer in backward order, each collective gated by the engine's
    per-layer gradient event (train_step; engine option dp_layer_events) instead of by the end of the stem backward.  OFF by
    default: six extra 2.4 MB collectives per step are latency-bound on a real communicator (a launch + >= 20 us each on a
    stream that competes with the stem backward for CUs) and have not been measured to win on RCCL.
    ``measure_exposed``: HIP events around the point where the compute stream waits for the communication stream;
    ``exposed_comm_us()`` returns the mean stall per step (what the overlap did NOT hide).
    ``emulate_load`` (dry runs on one GPU over gloo): every reduction first runs a copy + add of the chunk's size on the
    communication stream -- kernels of a collective's shape sharing the CUs with the backward pass, which gloo's host-side
    reduction would not provide."""

    def __init__(self, group=None, buckets: int = 1, payload: str = "fp32", algorithm: str = "all_reduce",
                 layer_buckets: bool = False, measure_exposed: bool = False, emulate_load: bool = False):
        import torch.distributed as dist
        if payload not in ("fp32", "bf16"):
            raise ValueError(f"payload must be 'fp32' or 'bf16', got {payload!r}")
        if algorithm not in ("all_reduce", "rs_ag"):
            raise ValueError(f"algorithm must be 'all_reduce' or 'rs_ag', got {algorithm!r}")
        self.dist = dist
        self.group = group
        self.world_size = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self.buckets = max(1, int(buckets))
        self.payload = payload
        self.algorithm = algorithm
        self.layer_buckets = bool(layer_buckets)
        self.measure_exposed = bool(measure_exposed)
        self.emulate_load = bool(emulate_load)
        self.collectives = 0                # issued since construction (the bench line reports collectives per step)
        self._exposed = []                  # (event before the stall, event after it) per wait()
        self._load = {}                     # numel -> two scratch buffers of the emulated collective
        self._works = []
        self._stream = None
        self._stage = {}                    # (data_ptr, numel) -> bf16 staging buffer
        self._shard = {}                    # (data_ptr, numel, dtype) -> reduce_scatter output shard
        self._pending = []                  # (fp32 chunk, bf16 buffer) to widen after the collective

    def _chunks(self, flat: torch.Tensor):
        n = flat.numel()
        step = -(-n // self.buckets)
        step = -(-step // 1024) * 1024      # 4 KiB-aligned chunk starts
        return [flat[i:min(i + step, n)] for i in range(0, n, step)]

    def _collective(self, buf: torch.Tensor) -> None:
        """SUM over the ranks of ``buf`` in place, asynchronously (the works are collected in self._works)."""
        d, W = self.dist, self.world_size
        self.collectives += 1
        if self.emulate_load and buf.is_cuda:
            sc = self._load.get(buf.numel())
            if sc is None:
                sc = self._load[buf.numel()] = (torch.empty_like(buf), torch.ones_like(buf))
            sc[0].copy_(buf)                # the receive copy ...
            sc[0].add_(sc[1])               # ... and the reduction of a ring step, on the communication stream
        if self.algorithm == "all_reduce" or buf.numel() < 2 * W:
            self._works.append(d.all_reduce(buf, op=d.ReduceOp.SUM, group=self.group, async_op=True))
            return
        main = buf.numel() - buf.numel() % W
        key = (buf.data_ptr(), buf.numel(), buf.dtype)
        shard = self._shard.get(key)
        if shard is None:
            shard = self._shard[key] = torch.empty(main // W, dtype=buf.dtype, device=buf.device)
        # phase 1: rank r ends with the sum of slice r; phase 2: every rank collects the W reduced slices (identical bytes
        # everywhere by construction).  The all_gather reads what the reduce_scatter wrote: wait() orders the two (on
        # GPUs it orders the communication stream, it does not block the host).
        d.reduce_scatter_tensor(shard, buf[:main], op=d.ReduceOp.SUM, group=self.group, async_op=True).wait()
        self._works.append(d.all_gather_into_tensor(buf[:main], shard, group=self.group, async_op=True))
        if main < buf.numel():
            self._works.append(d.all_reduce(buf[main:], op=d.ReduceOp.SUM, group=self.group, async_op=True))

    def _reduce(self, chunk: torch.Tensor) -> None:
        if self.payload == "bf16":
            key = (chunk.data_ptr(), chunk.numel())
            buf = self._stage.get(key)
            if buf is None:
                buf = self._stage[key] = torch.empty(chunk.numel(), dtype=torch.bfloat16, device=chunk.device)
            buf.copy_(chunk)
            self._collective(buf)
            self._pending.append((chunk, buf))
        else:
            self._collective(chunk)

    def reduce_async(self, flat: torch.Tensor, after=None) -> None:
        """Start the reduction of ``flat`` on the communication stream.  ``after(stream)``: a callable that makes that stream
        wait for exactly what ``flat`` depends on (an engine gradient-bucket event); default: everything enqueued on the
        current stream so far."""
        if self.world_size == 1:
            return
        if flat.is_cuda:
            if self._stream is None:
                self._stream = torch.cuda.Stream(device=flat.device)
            if after is not None:
                after(self._stream)
            else:
                self._stream.wait_stream(torch.cuda.current_stream(flat.device))
            with torch.cuda.stream(self._stream):
                for c in self._chunks(flat):
                    self._reduce(c)
        else:
            for c in self._chunks(flat):
                self._reduce(c)

    def wait(self) -> None:
        import contextlib
        cuda = self._stream is not None
        with (torch.cuda.stream(self._stream) if cuda else contextlib.nullcontext()):
            for w in self._works:
                w.wait()                    # on GPUs: orders the comm stream after the collective, no host block
            for chunk, buf in self._pending:
                chunk.copy_(buf)            # widen bf16 -> fp32 in place
        self._works.clear()
        self._pending.clear()
        if cuda:
            cur = torch.cuda.current_stream()
            if self.measure_exposed:
                e0 = torch.cuda.Event(enable_timing=True)
                e0.record(cur)
            cur.wait_stream(self._stream)
            if self.measure_exposed:
                e1 = torch.cuda.Event(enable_timing=True)
                e1.record(cur)
                self._exposed.append((e0, e1))

    def exposed_comm_us(self) -> Optional[float]:
        """Mean time per step the compute stream stood waiting for the communication stream since the last call (needs
        ``measure_exposed``); blocks until the recorded events have completed."""
        if not self._exposed:
            return None
        self._exposed[-1][1].synchronize()
        v = sum(a.elapsed_time(b) for a, b in self._exposed) * 1e3 / len(self._exposed)
        self._exposed.clear()
        return v

    def describe(self) -> Dict[str, object]:
        """What ran: backend, library version, world size and the shape of the exchange (for the bench line)."""
        d = self.dist
        backend = d.get_backend(self.group)
        ver = None
        if backend == "nccl":
            try:
                ver = ".".join(str(v) for v in torch.cuda.nccl.version())
            except Exception:
                ver = "unknown"
        return {"backend": backend, "library": "RCCL" if backend == "nccl" else backend, "version": ver,
                "world_size": self.world_size, "algorithm": self.algorithm, "buckets_per_stage": self.buckets,
                "payload": self.payload, "layer_buckets": self.layer_buckets, "emulated_load": self.emulate_load}

    def broadcast_params(self, flat: torch.Tensor, src: int = 0) -> None:
        if self.world_size > 1:
            self.dist.broadcast(flat, src=src, group=self.group)


def device_identity(index: Optional[int] = None) -> str:
    """A string that names the PHYSICAL device behind ``cuda:index`` of this process: its UUID and its PCI domain:bus:device as far as
    the runtime reports them, else the ordinal -- what the bench line lists per rank so that N ranks can be seen to sit on N distinct
    GPUs (a CPU-only process reports ``cpu:<hostname>:<pid>``)."""
    if not torch.cuda.is_available():
        import socket
        return f"cpu:{socket.gethostname()}:{os.getpid()}"
    i = torch.cuda.current_device() if index is None else int(index)
    pr = torch.cuda.get_device_properties(i)
    parts = []
    uuid = getattr(pr, "uuid", None)
    if uuid is not None and str(uuid).strip("0-") != "":
        parts.append(f"uuid:{uuid}")
    bus = getattr(pr, "pci_bus_id", None)
    if bus is not None:
        parts.append(f"pci:{getattr(pr, 'pci_domain_id', 0):04x}:{bus:02x}:{getattr(pr, 'pci_device_id', 0):02x}")
    # (both when both exist: two ranks count as sharing a device only if EVERY identifier the runtime gives agrees)
    return "|".join(parts) if parts else f"ordinal:{i}"


def gather_device_identities(dist=None, group=None, mine: Optional[str] = None) -> List[str]:
    """Every rank's ``device_identity()`` in rank order (all_gather_object over the job's process group; one entry without
    torch.distributed).  ``assert_distinct_devices`` is the check on top of it."""
    mine = device_identity() if mine is None else mine
    if dist is None or not dist.is_initialized() or dist.get_world_size(group) == 1:
        return [mine]
    out: List[Optional[str]] = [None] * dist.get_world_size(group)
    dist.all_gather_object(out, mine, group=group)
    return [str(o) for o in out]


def assert_distinct_devices(ids: List[str], allow_shared: bool = False) -> None:
    """A data-parallel job whose ranks share a GPU measures nothing: refuse (``allow_shared``: the one-GPU test hook)."""
    if len(set(ids)) != len(ids) and not allow_shared:
        raise RuntimeError(f"data-parallel ranks share a device: {ids}")


def shard_bounds(num_items: int, world_size: int, rank: int):
    """Contiguous shard [lo, hi) of ``num_items`` independent units (samples) for ``rank``."""
    base, rem = divmod(num_items, world_size)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)
