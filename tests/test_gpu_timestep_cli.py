"""train_ncsn.py with --loss_weighting=min_snr --timestep_sampler=loss_second_moment end to end: it runs,
logs both loss values, writes a checkpoint whose metadata names the options and whose tensors include the sampler's tables, and a
resumed run loads them; without the flags the checkpoint holds no such tensors.  Model flags: those of tests/test_gpu_cli.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = ["timestep_sampler/cdf", "timestep_sampler/counts", "timestep_sampler/history", "timestep_sampler/p"]


def run(*flags, ok=True, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_ncsn.py"), *flags], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert (r.returncode == 0) == ok, f"train_ncsn.py returned {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r.stdout + r.stderr


def common(model_dir):
    return ["--flagfile=configs/ddpm-mel-32seq-512.cfg", "--synthetic", "--synthetic_examples=512", "--slice_ckpt=", f"--model_dir={model_dir}",
            "--loss=ddpm", "--num_layers=2", "--mlp_dims=256", "--num_mlp_layers=1", "--batch_size=8", "--num_sigmas=15",
            "--logging_freq=5", "--snapshot_freq=10", "--snapshot_sampling=false"]


def newest(model_dir):
    from safetensors import safe_open
    from smd_amd import checkpoint
    path = checkpoint.latest_checkpoint(str(model_dir))
    assert path is not None, os.listdir(model_dir)
    with safe_open(path, framework="pt") as f:
        return {k: f.get_tensor(k) for k in f.keys() if not k.startswith(("target/", "ema/", "state/param_states/"))}, f.metadata()


def test_weighted_training_checkpoints_and_resumes(tmp_path):
    d = tmp_path / "model"
    out = run(*common(d), "--max_steps=30", "--loss_weighting=min_snr", "--timestep_sampler=loss_second_moment")
    assert "loss weighting: min_snr (min_snr_gamma 5); timestep sampler: loss_second_moment" in out
    assert "loss_unweighted" in out                                                   # both loss values on the log line
    rows = [json.loads(l) for l in open(d / "train" / "scalars.jsonl")]
    lw, lu = ([r["value"] for r in rows if r["tag"] == t] for t in ("loss", "loss_unweighted"))
    assert len(lw) == len(lu) == 7 and np.isfinite(lw).all() and np.isfinite(lu).all() and lw != lu
    tensors, meta = newest(d)
    assert (meta["loss_weighting"], float(meta["min_snr_gamma"]), meta["timestep_sampler"]) == ("min_snr", 5.0, "loss_second_moment")
    assert sorted(k for k in tensors if k.startswith("timestep_sampler/")) == TABLES
    counts, hist = tensors["timestep_sampler/counts"].numpy(), tensors["timestep_sampler/history"].numpy()
    assert hist.shape == (15, 10) and counts.min() >= 0 and counts.max() == 10
    assert abs(float(tensors["timestep_sampler/cdf"][-1]) - 1.0) <= 15 * 2.0 ** -24
    step0 = int(tensors["state/step"])
    assert step0 == 31                                                                # steps 0 .. 30
    # a resumed run loads the tables and goes on from the optimiser state
    out = run(*common(d), "--max_steps=10", "--resume", "--loss_weighting=min_snr", "--timestep_sampler=loss_second_moment")
    assert "resumed from" in out and "timestep sampler: tables restored from the checkpoint" in out
    tensors2, _ = newest(d)
    assert int(tensors2["state/step"]) == step0 + 11
    filled = np.minimum(counts, 10).sum()
    assert np.minimum(tensors2["timestep_sampler/counts"].numpy(), 10).sum() >= filled     # the history went on, it did not restart
    assert (tensors2["timestep_sampler/counts"].numpy() >= counts).all()
    # the refusals of the command line
    assert "--loss=ddpm only" in run(*[f for f in common(d) if f != "--loss=ddpm"], "--loss=dsm", "--sampling=ald",
                                     "--loss_weighting=min_snr", ok=False)


def test_default_run_has_no_sampler_tensors(tmp_path):
    d = tmp_path / "model"
    out = run(*common(d), "--max_steps=10")
    assert "loss weighting: none" in out and "loss_unweighted" not in out
    tensors, meta = newest(d)
    assert not [k for k in tensors if k.startswith("timestep_sampler/")]
    assert (meta["loss_weighting"], meta["timestep_sampler"]) == ("none", "uniform")
