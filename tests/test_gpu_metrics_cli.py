"""sample_ncsn.py --compute_metrics end to end on the GPU: a tiny model trained as in test_gpu_cli.py (C = 42 slice, 2 layers),
then the distance scalars of evaluate() in <sampling_dir>/scalars.jsonl (reference sample_ncsn.py:69-186, :473-476)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("frechet_distance", "mmd_rbf", "mmd_polynomial")


def run(script, *flags, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), *flags], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, f"{script} failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r.stdout + r.stderr


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    import smd_amd.data as D
    import smd_amd.tfrecord as T
    d = tmp_path_factory.mktemp("metrics_cli")
    rng = np.random.default_rng(0)
    D.save(np.sort(rng.choice(512, 42, replace=False)), str(d / "slice.pkl"))
    for name, n in (("train-00000-of-00001", 24), ("eval-00000-of-00001", 16)):
        T.write_latents(str(d / "ds" / f"{name}.tfrecord"), (rng.standard_normal((n, 32, 512)) * 2).astype(np.float32))
    flags = ["--flagfile=configs/ddpm-mel-32seq-512.cfg", f"--dataset={d / 'ds'}", f"--slice_ckpt={d / 'slice.pkl'}",
             f"--model_dir={d / 'model'}", "--num_layers=2", "--mlp_dims=256", "--num_mlp_layers=1", "--batch_size=8",
             "--num_sigmas=50"]
    run("train_ncsn.py", *flags, "--epochs=1", "--snapshot_freq=100", "--snapshot_sampling=false")
    return d, flags


def scalars(path):
    with open(os.path.join(path, "scalars.jsonl")) as f:
        return [json.loads(line) for line in f]


def test_sample_compute_metrics_writes_the_distances(trained):
    d, flags = trained
    out = d / "samples"
    log = run("sample_ncsn.py", *flags, "--sample_size=8", f"--sampling_dir={out}", "--compute_metrics=true", "--flush=false")
    rows = scalars(out)
    got = {(r["tag"], r["step"]): r["value"] for r in rows}
    assert len(got) == len(rows) == 3 * 22
    assert set(got) == ({(f"ncsn/{m}", i) for m in NAMES for i in range(20)} | {(f"random/{m}", 0) for m in NAMES}
                        | {(f"real/{m}", 0) for m in NAMES})
    assert all(np.isfinite(v) for v in got.values())
    assert abs(got[("real/mmd_rbf", 0)]) <= 1e-7 and abs(got[("real/mmd_polynomial", 0)]) <= 1e-7
    # |real/frechet_distance| <= 1e-6 * 2 tr S; the eval set is normalised to [-1, 1]^42, so tr S <= 42
    assert abs(got[("real/frechet_distance", 0)]) <= 1e-6 * 2 * 42
    assert "frechet_dist" in log and "ipr_realism" in log                  # log_metrics line; the not-upstream warning
    assert os.path.isdir(out / "sampling_epoch0")                          # the sampler scalars, as before
    assert not os.path.exists(out / "ncsn" / "generated.pkl")              # --noflush: metrics only


def test_compute_final_only_logs_one_point(trained):
    d, flags = trained
    out = d / "final_only"
    run("sample_ncsn.py", *flags, "--sample_size=8", f"--sampling_dir={out}", "--compute_metrics=true",
        "--compute_final_only=true")
    steps = sorted(r["step"] for r in scalars(out) if r["tag"] == "ncsn/mmd_rbf")
    assert steps == [0]
    assert {r["tag"].split("/")[0] for r in scalars(out)} == {"ncsn", "random", "real"}
    assert os.path.exists(out / "ncsn" / "generated.pkl")
