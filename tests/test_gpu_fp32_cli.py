"""sample_ncsn.py --dtype=fp32 end to end on the GPU: unconditional, --infill, --interpolate, --compute_metrics, a checkpoint
written by a bf16 training run, and train_ncsn.py's refusal."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_cli import ROOT, common, run, workdir  # noqa: F401  (the fixture and helpers of the bf16 CLI test, by import)

pytestmark = pytest.mark.gpu
SYN = ["--flagfile=configs/ddpm-mel-32seq-512.cfg", "--slice_ckpt=", "--synthetic", "--dtype=fp32", "--sample_size=8", "--num_sigmas=50", "--num_layers=2", "--mlp_dims=256", "--num_mlp_layers=1"]


def test_synthetic_sampling_writes_the_reference_files_and_repeats(tmp_path):
    import smd_amd.data as D
    outs = []
    for i in range(2):
        d = tmp_path / f"s{i}"
        run("sample_ncsn.py", *SYN, f"--model_dir={tmp_path / 'none'}", f"--sampling_dir={d}", "--sample_seed=3")
        outs.append({n: open(d / "ncsn" / f"{n}.pkl", "rb").read() for n in ("generated", "collection", "real")})
    gen = D.load(str(tmp_path / "s0" / "ncsn" / "generated.pkl"))
    coll = D.load(str(tmp_path / "s0" / "ncsn" / "collection.pkl"))
    real = D.load(str(tmp_path / "s0" / "ncsn" / "real.pkl"))
    assert gen.shape == (8, 32, 512) and np.isfinite(gen).all()              # sample_ncsn.py:452-471 (synthetic: min / max are scalars)
    assert coll.shape == (41, 8, 32, 512) and real.shape == (8, 32, 512)
    assert outs[0]["generated"] == outs[1]["generated"]                    # same seed: identical bytes (no slice: every dim is the model's)


def test_infill_interpolate_and_metrics_run(tmp_path):
    import smd_amd.data as D
    base = [*SYN, f"--model_dir={tmp_path / 'none'}"]
    run("sample_ncsn.py", *base, f"--sampling_dir={tmp_path / 'inf'}", "--infill=true")
    g = D.load(str(tmp_path / "inf" / "ncsn" / "generated.pkl"))
    assert g.shape == (8, 32, 512) and np.isfinite(g).all()
    run("sample_ncsn.py", *base, f"--sampling_dir={tmp_path / 'itp'}", "--interpolate=true")
    gi = D.load(str(tmp_path / "itp" / "ncsn" / "generated.pkl"))
    assert gi.shape == (9, 8, 32, 512) and np.isfinite(gi).all()
    run("sample_ncsn.py", *base, f"--sampling_dir={tmp_path / 'met'}", "--compute_metrics=true", "--compute_final_only=true")
    assert os.path.exists(tmp_path / "met" / "scalars.jsonl")


def test_a_bf16_checkpoint_samples_under_fp32(workdir):  # noqa: F811
    import smd_amd.data as D
    run("train_ncsn.py", *common(workdir), "--epochs=1", "--logging_freq=1", "--snapshot_freq=100", "--snapshot_sampling=false")
    assert any(f.startswith("checkpoint_") for f in os.listdir(workdir / "model"))
    sl = D.load(str(workdir / "slice.pkl"))
    gens = {}
    for dt in ("fp32", "bf16"):
        out = run("sample_ncsn.py", *common(workdir), "--sample_size=4", f"--sampling_dir={workdir / dt}", "--sample_seed=3", f"--dtype={dt}")
        assert "no checkpoint" not in out
        gens[dt] = D.load(str(workdir / dt / "ncsn" / "generated.pkl"))[..., sl]
    assert gens["fp32"].shape == (4, 32, 42) and np.isfinite(gens["fp32"]).all()
    d = float(np.linalg.norm(gens["fp32"] - gens["bf16"]) / np.linalg.norm(gens["fp32"]))
    print(f"same checkpoint, same jax.random streams, 50 steps: bf16 samples against fp32 samples rel-L2 {d:.3e}")
    assert 0 < d < 5e-2           # the same weights were loaded (an unrelated model would be O(1) away); not the same arithmetic


def test_train_cli_refuses_fp32(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_ncsn.py"), "--slice_ckpt=", "--synthetic", "--dtype=fp32", f"--model_dir={tmp_path}"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "fp32 is an inference precision in this engine" in r.stderr
    assert not os.listdir(tmp_path)
