"""train_ncsn.py --prediction={v,x0} and sample_ncsn.py on its checkpoint, end to end: the run logs
loss, loss_unweighted and loss_eps, the checkpoint's metadata names the kind, sampling takes the kind from the checkpoint -- every
timestep, eight DPM-Solver++(2M) steps on the logSNR grid, the variational bound -- and refuses a --prediction that contradicts
it.  Model flags: those of tests/test_gpu_timestep_cli.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = ["--flagfile=configs/ddpm-mel-32seq-512.cfg", "--synthetic", "--slice_ckpt=", "--num_layers=2", "--mlp_dims=256",
         "--num_mlp_layers=1", "--num_sigmas=15"]


def run(script, *flags, ok=True, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), *flags], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert (r.returncode == 0) == ok, f"{script} returned {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r.stdout + r.stderr


@pytest.mark.parametrize("kind", ["v", "x0"])
def test_train_then_sample(tmp_path, kind):
    from safetensors import safe_open
    from smd_amd import checkpoint
    d = tmp_path / "model"
    out = run("train_ncsn.py", *MODEL, f"--model_dir={d}", "--synthetic_examples=512", "--loss=ddpm", "--batch_size=8",
              "--logging_freq=5", "--snapshot_freq=10", "--snapshot_sampling=false", "--max_steps=30", f"--prediction={kind}",
              "--loss_weighting=min_snr")
    assert f"prediction: {kind}" in out
    rows = [json.loads(l) for l in open(d / "train" / "scalars.jsonl")]
    vals = {t: [r["value"] for r in rows if r["tag"] == t] for t in ("loss", "loss_unweighted", "loss_eps")}
    for t, v in vals.items():
        assert len(v) == 7 and np.isfinite(v).all(), (t, v)
    assert vals["loss"] != vals["loss_unweighted"] and vals["loss_eps"] != vals["loss_unweighted"]
    path = checkpoint.latest_checkpoint(str(d))
    with safe_open(path, framework="pt") as f:
        assert f.metadata()["prediction"] == kind
    assert checkpoint.checkpoint_prediction(str(d)) == kind
    # --resume with another kind is refused at start-up
    other = "eps" if kind == "v" else "v"
    msg = run("train_ncsn.py", *MODEL, f"--model_dir={d}", "--synthetic_examples=512", "--loss=ddpm", "--batch_size=8", "--max_steps=2",
              "--resume", f"--prediction={other}", ok=False)
    assert "--resume" in msg and f"--prediction={kind}" in msg
    # sampling: no flag (the checkpoint says), the second-order solver on the logSNR grid, the bound, and the mismatch
    sample = [*MODEL, f"--model_dir={d}", "--sample_size=8", "--sampling=ddpm"]
    s1 = tmp_path / "full"
    out = run("sample_ncsn.py", *sample, f"--sampling_dir={s1}")
    assert f"prediction: {kind}" in out
    s2 = tmp_path / "dpm"
    run("sample_ncsn.py", *sample, f"--sampling_dir={s2}", "--ddim_steps=8", "--ddim_order=2", "--ddim_spacing=logsnr")
    from smd_amd import data
    for s in (s1, s2):
        g = np.asarray(data.load(str(s / "ncsn" / "generated.pkl")))
        assert g.shape[0] == 8 and np.isfinite(g).all()
    s3 = tmp_path / "bound"
    run("sample_ncsn.py", *sample, f"--sampling_dir={s3}", "--compute_bound", "--bound_steps=4", "--bound_only")
    js = json.load(open(s3 / "ncsn" / "bound.json"))
    assert js["prediction"] == kind and js["eps_mse"] is None and len(js["terms"]) == 4 and np.isfinite(js["terms"]).all()
    assert np.isfinite(js["prior"])
    msg = run("sample_ncsn.py", *sample, f"--sampling_dir={tmp_path / 'no'}", f"--prediction={other}", ok=False)
    assert f"--prediction={other} contradicts" in msg and f"--prediction={kind}" in msg
    # the refusals of the training command line name the flags
    msg = run("train_ncsn.py", *MODEL, f"--model_dir={tmp_path / 'm2'}", "--loss=dsm", "--sampling=ald", f"--prediction={kind}", ok=False)
    assert f"--prediction={kind}" in msg and "--loss=ddpm only" in msg
    msg = run("train_ncsn.py", *MODEL, f"--model_dir={tmp_path / 'm3'}", "--loss=ddpm", "--sampling=ald", f"--prediction={kind}", ok=False)
    assert "--sampling=ddpm" in msg
