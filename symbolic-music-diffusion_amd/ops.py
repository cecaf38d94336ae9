"""PyTorch custom ops (``torch.ops.smd_amd.*``) over the C-ABI -- the "PyTorch-ROCm custom ops" seam of the north star.

Each op is a thin, shape-checked registration of one C entry point of ``include/smd_hip.h``: device tensors in, device
tensors out, launched on torch's current HIP stream; fake-tensor (meta) rules are registered so the ops trace under
``torch.compile`` / ``torch.export`` without running.  There is no CPU implementation: a CPU tensor raises.

  smd_amd::eps_forward(x, noise_level, engine)          model(x, cond), models/ncsn.py:141-179 / 125-135
  smd_amd::eps_forward_train(x, noise_level, params, engine)   the same, DIFFERENTIABLE with respect to the flat parameter
                                                        buffer: forward in the training workspace, backward =
                                                        the engine's own backward pass from d/d eps_hat (autograd formula
                                                        registered with torch.library.register_autograd)
  smd_amd::gemm_bf16_nt(a, bt, bias)                    nn.Dense, bf16 operands, fp32 accumulate -> bf16
  smd_amd::ddpm_reverse_step_(x, eps_hat, coef, t, ...) utils/ebm_utils.py:327-394, in place
  smd_amd::q_sample(x0, alphas_prod_ext, labels, eps)   utils/losses.py:271-296
  smd_amd::bound_noise(x0, eps, table, t)               x_t of the variational bound at the device timestep t
  smd_amd::bound_terms(x0, eps, eps_hat, table, t, clip)   its three per-example sums [B][3]
  smd_amd::timestep_draw(cdf, p, u, label_base)         loss-aware timestep labels and importance weights
  smd_amd::weighted_mse(pred, eps, s, iw, gamma, inv)   the weighted DDPM loss and its gradient w.r.t. pred
  smd_amd::param_mse(pred, eps, x0, s, iw, gamma, kind, inv)   the same for an x0- / v-predicting network

``engine`` is the integer id of a live ``smd_amd.engine.Engine`` (``register_engine``); custom-op schemas carry tensors
and scalars only.
"""
from __future__ import annotations

import weakref
from typing import Tuple

import torch

from . import lib as _lib

_ENGINES: "weakref.WeakValueDictionary[int, object]" = weakref.WeakValueDictionary()


def register_engine(engine) -> int:
    """Id under which ``engine`` is reachable from ``torch.ops.smd_amd.eps_forward`` (weakly held)."""
    _ENGINES[id(engine)] = engine
    return id(engine)


def _need_gpu(*ts: torch.Tensor) -> None:
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError("smd_amd ops run on the GPU only (no CPU fallback): got a tensor on " + str(t.device))


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


@torch.library.custom_op("smd_amd::eps_forward", mutates_args=())
def eps_forward(x: torch.Tensor, noise_level: torch.Tensor, engine: int) -> torch.Tensor:
    _need_gpu(x, noise_level)
    eng = _ENGINES.get(engine)
    if eng is None:
        raise RuntimeError(f"smd_amd::eps_forward: no live engine with id {engine} (ops.register_engine)")
    return eng.forward(x, noise_level)


@eps_forward.register_fake
def _(x, noise_level, engine):
    return torch.empty_like(x, dtype=torch.float32)


# ---- model(x, cond), differentiable w.r.t. the parameters: jax.value_and_grad(loss_fn)(optimizer.target), train_ncsn.py:279-283
@torch.library.custom_op("smd_amd::eps_forward_train", mutates_args=())
def eps_forward_train(x: torch.Tensor, noise_level: torch.Tensor, params: torch.Tensor, engine: int) -> torch.Tensor:
    """``engine`` is a TRAINING handle; ``params`` must be (an alias of) its flat fp32 parameter buffer -- it is an argument so
    that autograd has an edge to hang the parameter gradient on, the kernels read the engine's own operand pack."""
    _need_gpu(x, noise_level, params)
    eng = _ENGINES.get(engine)
    if eng is None:
        raise RuntimeError(f"smd_amd::eps_forward_train: no live engine with id {engine} (ops.register_engine)")
    if eng.cfg.dtype == "fp32":
        from .engine import FP32_REFUSAL
        raise ValueError(FP32_REFUSAL)
    if params.data_ptr() != eng.params.data_ptr() or params.numel() != eng.params.numel():
        raise ValueError("smd_amd::eps_forward_train: `params` is not the engine's parameter buffer")
    return eng.forward_train(x, noise_level)


@eps_forward_train.register_fake
def _(x, noise_level, params, engine):
    return torch.empty_like(x, dtype=torch.float32)


@torch.library.custom_op("smd_amd::eps_backward", mutates_args=())
def eps_backward(dpred: torch.Tensor, engine: int, generation: int) -> torch.Tensor:
    """The engine's backward pass from d objective / d eps_hat; returns the flat parameter gradient as a FRESH tensor (a copy of
    the engine's gradient buffer, which the handle's next backward pass overwrites): autograd may adopt it as ``params.grad``
    and accumulate later passes into it, and a ``.grad`` reference kept across steps stays what it was.
    trainer._train_step_generic alone skips the 100 MB copy: it sets ``engine._grad_alias_ok`` around its own backward pass,
    clears ``params.grad`` before it and consumes the gradient before the next one; only then is the buffer itself returned."""
    _need_gpu(dpred)
    eng = _ENGINES.get(engine)
    if eng is None:
        raise RuntimeError(f"smd_amd::eps_backward: no live engine with id {engine}")
    if getattr(eng, "_fwd_generation", 0) != generation:
        raise RuntimeError("smd_amd::eps_backward: the engine has run another training forward pass since this one (one "
                           "workspace per handle: call backward() before the next model(x, cond), or use a second handle)")
    eng.backward_from(dpred)
    return eng.grads.detach() if getattr(eng, "_grad_alias_ok", False) else eng.grads.clone()


@eps_backward.register_fake
def _(dpred, engine, generation):
    eng = _ENGINES.get(engine)
    return dpred.new_empty((eng.n_params if eng is not None else 0,), dtype=torch.float32)


def _eps_train_setup(ctx, inputs, output):
    _x, _s, _params, engine = inputs
    eng = _ENGINES.get(engine)
    ctx.engine = engine
    ctx.generation = getattr(eng, "_fwd_generation", 0)


def _eps_train_backward(ctx, grad_out):
    # d/dx is not produced (the reference never differentiates the objective w.r.t. the data either)
    return None, None, torch.ops.smd_amd.eps_backward(grad_out.contiguous(), ctx.engine, ctx.generation), None


torch.library.register_autograd("smd_amd::eps_forward_train", _eps_train_backward, setup_context=_eps_train_setup)


@torch.library.custom_op("smd_amd::gemm_bf16_nt", mutates_args=())
def gemm_bf16_nt(a: torch.Tensor, bt: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """C[M,N] = A[M,K] Bt[N,K]^T + bias (bf16 operands with K % 64 == 0, fp32 bias, bf16 result)."""
    _need_gpu(a, bt, bias)
    if a.dtype != torch.bfloat16 or bt.dtype != torch.bfloat16 or bias.dtype != torch.float32:
        raise TypeError("gemm_bf16_nt: a, bt bf16 and bias fp32")
    if a.dim() != 2 or bt.dim() != 2 or a.shape[1] != bt.shape[1] or bias.numel() != bt.shape[0]:
        raise ValueError(f"gemm_bf16_nt: shapes {tuple(a.shape)} x {tuple(bt.shape)}^T + {tuple(bias.shape)}")
    a, bt, bias = a.contiguous(), bt.contiguous(), bias.contiguous()
    M, K = a.shape
    N = bt.shape[0]
    out = torch.empty((M, N), dtype=torch.bfloat16, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(_lib.get_lib().smd_gemm_bf16_nt(a.data_ptr(), K, bt.data_ptr(), K, M, N, K, bias.data_ptr(), 0, None, 0,
                                                   None, 0, out.data_ptr(), N, _stream()), "gemm_bf16_nt")
    return out


@gemm_bf16_nt.register_fake
def _(a, bt, bias):
    return a.new_empty((a.shape[0], bt.shape[0]), dtype=torch.bfloat16)


@torch.library.custom_op("smd_amd::ddpm_reverse_step_", mutates_args=("x",))
def ddpm_reverse_step_(x: torch.Tensor, eps_hat: torch.Tensor, coef: torch.Tensor, t: torch.Tensor, z: torch.Tensor) -> None:
    """x <- one sample_with_beta iteration at the device timestep ``t`` (int32[1]) with the explicit draw ``z``."""
    _need_gpu(x, eps_hat, coef, t, z)
    if x.dtype != torch.float32 or not x.is_contiguous() or x.shape != eps_hat.shape or x.shape != z.shape:
        raise ValueError("ddpm_reverse_step_: x, eps_hat, z are contiguous fp32 tensors of one shape")
    B = x.shape[0]
    S, Cn = (1, x.shape[1]) if x.dim() == 2 else (x.shape[1], x.shape[2])
    with torch.cuda.device(x.device):
        _lib.check(_lib.get_lib().smd_ddpm_reverse_step(x.data_ptr(), eps_hat.contiguous().data_ptr(), B, S, Cn, coef.data_ptr(),
                                                        coef.shape[0], t.data_ptr(), z.contiguous().data_ptr(), 0, 0, 0, None,
                                                        None, None, _stream()), "ddpm_reverse_step")


@torch.library.custom_op("smd_amd::q_sample", mutates_args=())
def q_sample(x0: torch.Tensor, alphas_prod_ext: torch.Tensor, labels: torch.Tensor,
             eps: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(x_t as bf16 [B*S][C], noise level sqrt(alpha) [B]) for explicit labels in [1, T] and eps."""
    _need_gpu(x0, alphas_prod_ext, labels, eps)
    if x0.dtype != torch.float32 or eps.shape != x0.shape or labels.dtype != torch.int32:
        raise ValueError("q_sample: x0, eps fp32 of one shape, labels int32")
    x0, eps = x0.contiguous(), eps.contiguous()
    B = x0.shape[0]
    S, Cn = (1, x0.shape[1]) if x0.dim() == 2 else (x0.shape[1], x0.shape[2])
    xt = torch.empty((B * S, Cn), dtype=torch.bfloat16, device=x0.device)
    eo = torch.empty_like(x0)
    s = torch.empty((B,), dtype=torch.float32, device=x0.device)
    with torch.cuda.device(x0.device):
        _lib.check(_lib.get_lib().smd_q_sample(x0.data_ptr(), B, S, Cn, Cn, alphas_prod_ext.numel() - 1, alphas_prod_ext.data_ptr(),
                                               labels.data_ptr(), 1, None, eps.data_ptr(), 0, 0, None, 0, xt.data_ptr(),
                                               eo.data_ptr(), s.data_ptr(), _stream()), "q_sample")
    return xt, s


@q_sample.register_fake
def _(x0, alphas_prod_ext, labels, eps):
    B = x0.shape[0]
    rows = B if x0.dim() == 2 else B * x0.shape[1]
    return x0.new_empty((rows, x0.shape[-1]), dtype=torch.bfloat16), x0.new_empty((B,), dtype=torch.float32)


def _bsc(x: torch.Tensor):
    return (x.shape[0], 1, x.shape[1]) if x.dim() == 2 else tuple(x.shape)


@torch.library.custom_op("smd_amd::bound_noise", mutates_args=())
def bound_noise(x0: torch.Tensor, eps: torch.Tensor, table: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """x_t = sqrt(ap_t) x0 + sqrt(1-ap_t) eps at the device timestep ``t`` (int32[1]); ``table`` is schedule.bound_tables' [T][4]
    float32 table.  ``t`` outside [0, T) leaves the result zero."""
    _need_gpu(x0, eps, table, t)
    if x0.dtype != torch.float32 or eps.dtype != torch.float32 or eps.shape != x0.shape or x0.dim() not in (2, 3):
        raise ValueError("bound_noise: x0, eps fp32 (B, S, C) or (B, C) tensors of one shape")
    if table.dtype != torch.float32 or table.dim() != 2 or table.shape[1] != 4 or t.dtype != torch.int32:
        raise ValueError("bound_noise: table fp32 [T][4], t int32[1]")
    x0, eps, table = x0.contiguous(), eps.contiguous(), table.contiguous()
    B, S, Cn = _bsc(x0)
    xt = torch.zeros_like(x0)
    with torch.cuda.device(x0.device):
        _lib.check(_lib.get_lib().smd_bound_noise(x0.data_ptr(), B, S, Cn, Cn, table.data_ptr(), table.shape[0], t.data_ptr(),
                                                  eps.data_ptr(), 0, 0, 0, None, 0, xt.data_ptr(), None, _stream()), "bound_noise")
    return xt


@bound_noise.register_fake
def _(x0, eps, table, t):
    return torch.empty_like(x0)


@torch.library.custom_op("smd_amd::bound_terms", mutates_args=())
def bound_terms(x0: torch.Tensor, eps: torch.Tensor, eps_hat: torch.Tensor, table: torch.Tensor, t: torch.Tensor,
                clip: float) -> torch.Tensor:
    """[B][3] = per-example (sum (x0 - x0_hat)^2, sum (eps - eps_hat)^2, sum x0^2) at the device timestep ``t`` (int32[1], left
    as it is); ``t`` outside [0, T) leaves the result zero."""
    _need_gpu(x0, eps, eps_hat, table, t)
    if x0.dtype != torch.float32 or eps.shape != x0.shape or eps_hat.shape != x0.shape or x0.dim() not in (2, 3):
        raise ValueError("bound_terms: x0, eps, eps_hat fp32 (B, S, C) or (B, C) tensors of one shape")
    if eps.dtype != torch.float32 or eps_hat.dtype != torch.float32:
        raise ValueError("bound_terms: eps, eps_hat fp32")
    if table.dtype != torch.float32 or table.dim() != 2 or table.shape[1] != 4 or t.dtype != torch.int32:
        raise ValueError("bound_terms: table fp32 [T][4], t int32[1]")
    x0, eps, eps_hat, table = x0.contiguous(), eps.contiguous(), eps_hat.contiguous(), table.contiguous()
    B, S, Cn = _bsc(x0)
    T = table.shape[0]
    partial = torch.zeros((T, B, 3), dtype=torch.float32, device=x0.device)
    with torch.cuda.device(x0.device):
        _lib.check(_lib.get_lib().smd_bound_terms(x0.data_ptr(), eps.data_ptr(), eps_hat.data_ptr(), B, S, Cn, table.data_ptr(), T,
                                                  float(clip), t.data_ptr(), None, None, partial.data_ptr(), _stream()), "bound_terms")
    return partial.sum(dim=0)


@bound_terms.register_fake
def _(x0, eps, eps_hat, table, t, clip):
    return x0.new_empty((x0.shape[0], 3), dtype=torch.float32)


# ---- weighted training
@torch.library.custom_op("smd_amd::timestep_draw", mutates_args=())
def timestep_draw(cdf: torch.Tensor, p: torch.Tensor, u: torch.Tensor, label_base: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(labels int32 [B], iw fp32 [B]) from the uniforms ``u`` [B]: label_base + (first i with cdf[i] > u), iw = 1 / (n p[i])
    (include/smd_hip.h smd_timestep_draw; trainer.TimestepSampler.draw also makes the uniforms)."""
    _need_gpu(cdf, p, u)
    if cdf.dtype != torch.float32 or p.dtype != torch.float32 or u.dtype != torch.float32 or cdf.dim() != 1 or p.shape != cdf.shape or u.dim() != 1:
        raise ValueError("timestep_draw: cdf, p fp32 [n], u fp32 [B]")
    cdf, p, u = cdf.contiguous(), p.contiguous(), u.contiguous()
    B = u.shape[0]
    labels = torch.empty((B,), dtype=torch.int32, device=u.device)
    iw = torch.empty((B,), dtype=torch.float32, device=u.device)
    with torch.cuda.device(u.device):
        _lib.check(_lib.get_lib().smd_timestep_draw(cdf.data_ptr(), p.data_ptr(), cdf.shape[0], int(label_base), B, 0, 0, 0, 0, None,
                                                    u.data_ptr(), labels.data_ptr(), iw.data_ptr(), _stream()), "timestep_draw")
    return labels, iw


@timestep_draw.register_fake
def _(cdf, p, u, label_base):
    return u.new_empty(u.shape, dtype=torch.int32), u.new_empty(u.shape, dtype=torch.float32)


@torch.library.custom_op("smd_amd::weighted_mse", mutates_args=())
def weighted_mse(pred: torch.Tensor, eps: torch.Tensor, noise_level: torch.Tensor, iw: torch.Tensor, min_snr_gamma: float,
                 inv_global_count: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(loss_per_sample [B] unweighted, weight_per_sample [B], dpred bf16 [B*S][C]) of the weighted DDPM loss: w = iw min(1,
    gamma (1 - s^2) / s^2), dpred = 2 w (pred - eps) inv_global_count (include/smd_hip.h smd_weighted_mse_fwd_bwd)."""
    _need_gpu(pred, eps, noise_level, iw)
    if pred.dtype != torch.float32 or eps.dtype != torch.float32 or eps.shape != pred.shape or pred.dim() not in (2, 3):
        raise ValueError("weighted_mse: pred, eps fp32 (B, S, C) or (B, C) tensors of one shape")
    B, S, Cn = _bsc(pred)
    if noise_level.dtype != torch.float32 or iw.dtype != torch.float32 or noise_level.numel() != B or iw.numel() != B:
        raise ValueError("weighted_mse: noise_level, iw fp32 [B]")
    pred, eps, noise_level, iw = pred.contiguous(), eps.contiguous(), noise_level.contiguous(), iw.contiguous()
    loss = torch.empty((B,), dtype=torch.float32, device=pred.device)
    w = torch.empty_like(loss)
    dpred = torch.empty((B * S, Cn), dtype=torch.bfloat16, device=pred.device)
    with torch.cuda.device(pred.device):
        _lib.check(_lib.get_lib().smd_weighted_mse_fwd_bwd(pred.data_ptr(), eps.data_ptr(), noise_level.data_ptr(), iw.data_ptr(),
                                                           float(min_snr_gamma), B, S, Cn, Cn, float(inv_global_count), loss.data_ptr(),
                                                           w.data_ptr(), dpred.data_ptr(), _stream()), "weighted_mse")
    return loss, w, dpred


@weighted_mse.register_fake
def _(pred, eps, noise_level, iw, min_snr_gamma, inv_global_count):
    B = pred.shape[0]
    rows = B if pred.dim() == 2 else B * pred.shape[1]
    return (pred.new_empty((B,), dtype=torch.float32), pred.new_empty((B,), dtype=torch.float32),
            pred.new_empty((rows, pred.shape[-1]), dtype=torch.bfloat16))


# ---- x0- / v-parameterised training
@torch.library.custom_op("smd_amd::param_mse", mutates_args=())
def param_mse(pred: torch.Tensor, eps: torch.Tensor, x0: torch.Tensor, noise_level: torch.Tensor, iw: torch.Tensor,
              min_snr_gamma: float, kind: int, inv_global_count: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(loss_per_sample [B] unweighted, weight_per_sample [B], dpred bf16 [B*S][C]) of the weighted DDPM loss of a network that
    predicts eps (kind 0), x0 (1) or v = s eps - sqrt(1 - s^2) x0 (2): dpred = 2 w (pred - target) inv_global_count with the
    targets and weights of include/smd_hip.h smd_engine_set_loss_weights (smd_param_mse_fwd_bwd)."""
    _need_gpu(pred, eps, x0, noise_level, iw)
    if pred.dtype != torch.float32 or eps.dtype != torch.float32 or x0.dtype != torch.float32 or eps.shape != pred.shape \
            or x0.shape != pred.shape or pred.dim() not in (2, 3):
        raise ValueError("param_mse: pred, eps, x0 fp32 (B, S, C) or (B, C) tensors of one shape")
    if int(kind) not in (0, 1, 2):
        raise ValueError(f"param_mse: kind={kind} (0 eps, 1 x0, 2 v)")
    B, S, Cn = _bsc(pred)
    if noise_level.dtype != torch.float32 or iw.dtype != torch.float32 or noise_level.numel() != B or iw.numel() != B:
        raise ValueError("param_mse: noise_level, iw fp32 [B]")
    pred, eps, x0, noise_level, iw = pred.contiguous(), eps.contiguous(), x0.contiguous(), noise_level.contiguous(), iw.contiguous()
    loss = torch.empty((B,), dtype=torch.float32, device=pred.device)
    w = torch.empty_like(loss)
    dpred = torch.empty((B * S, Cn), dtype=torch.bfloat16, device=pred.device)
    with torch.cuda.device(pred.device):
        _lib.check(_lib.get_lib().smd_param_mse_fwd_bwd(pred.data_ptr(), eps.data_ptr(), x0.data_ptr(), noise_level.data_ptr(),
                                                        iw.data_ptr(), float(min_snr_gamma), int(kind), B, S, Cn, Cn,
                                                        float(inv_global_count), loss.data_ptr(), w.data_ptr(), dpred.data_ptr(),
                                                        _stream()), "param_mse")
    return loss, w, dpred


@param_mse.register_fake
def _(pred, eps, x0, noise_level, iw, min_snr_gamma, kind, inv_global_count):
    B = pred.shape[0]
    rows = B if pred.dim() == 2 else B * pred.shape[1]
    return (pred.new_empty((B,), dtype=torch.float32), pred.new_empty((B,), dtype=torch.float32),
            pred.new_empty((rows, pred.shape[-1]), dtype=torch.bfloat16))
