"""The sidecar of --analytic_variance: the estimated statistic g_t = E[eps_hat^2] of Bao et al. 2022 with
what it was estimated for, as {sampling_dir}/ncsn/analytic_moments.safetensors, and the checks a run makes before it trusts one."""
from __future__ import annotations

import os
from typing import Dict, Optional, Tuple

import numpy as np

MOMENTS_FILE = "analytic_moments.safetensors"
# what a loaded file must agree on with the run; "examples" / "draws" / "example_source" are recorded too, for the reader
META_KEYS = ("prediction", "num_sigmas", "sigma_begin", "sigma_end", "schedule_type", "dtype", "checkpoint", "weights", "data_shape")


def weights_digest(engine) -> str:
    """sha256 of the network's float32 parameters as the engine holds them: two checkpoints of one name, or freshly initialised
    weights of another seed, are different networks"""
    import hashlib
    return hashlib.sha256(engine.params.detach().cpu().numpy().tobytes()).hexdigest()


def run_metadata(FLAGS, prediction: str, engine=None) -> Dict[str, str]:
    """What an estimate depends on besides the examples: the network (its checkpoint file, a digest of its weights, its kind, the
    engine's dtype) and the schedule (length and end points).  Strings, as safetensors metadata is."""
    from . import checkpoint
    path = FLAGS.model_dir if os.path.isfile(FLAGS.model_dir) else checkpoint.latest_checkpoint(FLAGS.model_dir)
    return dict(prediction=str(prediction), num_sigmas=str(int(FLAGS.num_sigmas)), sigma_begin=repr(float(FLAGS.sigma_begin)),
                sigma_end=repr(float(FLAGS.sigma_end)), schedule_type=str(FLAGS.schedule_type), dtype=str(FLAGS.dtype),
                checkpoint=os.path.abspath(path) if path else "", weights=weights_digest(engine) if engine is not None else "",
                data_shape=",".join(str(int(v)) for v in FLAGS.data_shape))


def save_moments(path: str, g: np.ndarray, timesteps, count: int, meta: Dict[str, str]) -> None:
    """g [K][...sample shape] float64 for the ascending ``timesteps`` [K], from ``count`` (example, draw) pairs."""
    import torch
    from safetensors.torch import save_file
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    save_file({"g": torch.from_numpy(np.ascontiguousarray(g, dtype=np.float64)),
               "timesteps": torch.from_numpy(np.asarray(timesteps, dtype=np.int64)),
               "count": torch.tensor([int(count)], dtype=torch.int64)}, path, metadata={k: str(v) for k, v in meta.items()})


def load_moments(path: str) -> Tuple[np.ndarray, np.ndarray, int, Dict[str, str]]:
    from safetensors import safe_open
    from safetensors.torch import load_file
    t = load_file(path)
    for name in ("g", "timesteps", "count"):
        if name not in t:
            raise ValueError(f"--analytic_moments={path}: no tensor {name!r}; not a file written by --analytic_variance")
    with safe_open(path, framework="pt") as f:
        meta = dict(f.metadata() or {})
    return t["g"].double().numpy(), t["timesteps"].long().numpy(), int(t["count"][0]), meta


def check_moments(path: str, g: np.ndarray, timesteps: np.ndarray, meta: Dict[str, str], want: Dict[str, str], walk,
                  sample_shape) -> np.ndarray:
    """Refuses (ValueError naming --analytic_moments) a file whose metadata contradicts the run or whose timesteps do not cover
    ``walk``; returns g's rows in the order of ``walk`` (iteration order)."""
    for k in META_KEYS:
        if k not in meta:
            raise ValueError(f"--analytic_moments={path}: the file does not record {k}")
        if meta[k] != want[k]:
            raise ValueError(f"--analytic_moments={path}: estimated with {k}={meta[k]}, this run has {k}={want[k]}")
    if tuple(g.shape[1:]) != tuple(sample_shape) or g.shape[0] != len(timesteps):
        raise ValueError(f"--analytic_moments={path}: g of shape {tuple(g.shape)} for {len(timesteps)} timesteps of samples {tuple(sample_shape)}")
    walk = np.asarray(walk, dtype=np.int64)
    pos = np.searchsorted(timesteps, walk)
    ok = (pos < len(timesteps)) & (timesteps[np.minimum(pos, len(timesteps) - 1)] == walk)
    if not ok.all():
        raise ValueError(f"--analytic_moments={path}: its {len(timesteps)} timesteps do not cover the walk: "
                         f"{[int(t) for t in walk[~ok]][:8]} are missing")
    return g[pos]


def resolve_walk(FLAGS, betas, walk: Optional[list]) -> np.ndarray:
    """The descending walk --ddim_steps (or a distilled checkpoint's record) samples on."""
    from . import schedule
    if walk is not None:
        return np.asarray(walk, dtype=np.int64)
    T = len(betas)
    return np.asarray(schedule.stride_timesteps(T, FLAGS.ddim_steps) if FLAGS.ddim_spacing == "uniform"
                      else schedule.logsnr_timesteps(T, FLAGS.ddim_steps, betas), dtype=np.int64)
