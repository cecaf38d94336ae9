"""sample_ncsn.py --compute_metrics --nn_metrics end to end on the GPU: the tiny model of test_gpu_metrics_cli.py, then the seven
scalars per point of evaluate() in <sampling_dir>/scalars.jsonl and the refusals of the flag check."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _nn_metrics_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIST = ("frechet_distance", "mmd_rbf", "mmd_polynomial")
NN = ("improved_precision", "improved_recall", "improved_f1", "ipr_realism")


def run(script, *flags, timeout=600, ok=True):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), *flags], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=timeout)
    if ok:
        assert r.returncode == 0, f"{script} failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    import smd_amd.data as D
    import smd_amd.tfrecord as T
    d = tmp_path_factory.mktemp("nn_metrics_cli")
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


def eval_examples(flags, n, monkeypatch):
    """the eval examples sample_ncsn.py compares with, loaded as it loads them"""
    import smd_amd.data as D
    import smd_amd.flags as F
    import train_ncsn
    monkeypatch.chdir(ROOT)
    fl = F.make_flags(include_sample=True)
    fl.parse(list(flags))
    shape = train_ncsn.model_shape(fl, D.load(fl.slice_ckpt))
    _, eval_ds, _, _ = train_ncsn.build_datasets(fl, shape, None, 0, 1)
    return eval_ds.take_examples(n)


def test_nn_metrics_writes_seven_scalars_per_point(trained, monkeypatch):
    d, flags = trained
    out = d / "samples"
    r = run("sample_ncsn.py", *flags, "--sample_size=8", f"--sampling_dir={out}", "--compute_metrics=true", "--nn_metrics=true",
            "--flush=false")
    log = r.stdout + r.stderr
    rows = scalars(out)
    got = {(r_["tag"], r_["step"]): r_["value"] for r_ in rows}
    names = DIST + NN
    assert len(got) == len(rows) == 7 * 22
    assert set(got) == ({(f"ncsn/{m}", i) for m in names for i in range(20)} | {(f"random/{m}", 0) for m in names}
                        | {(f"real/{m}", 0) for m in names})
    assert all(np.isfinite(v) for v in got.values())
    for (tag, step), v in got.items():
        model, name = tag.split("/")
        if name in ("improved_precision", "improved_recall", "improved_f1"):
            assert 0.0 <= v <= 1.0, (tag, step, v)
        if name == "ipr_realism":
            assert v >= 0.0
        if name == "improved_f1":
            p, q = got[(f"{model}/improved_precision", step)], got[(f"{model}/improved_recall", step)]
            assert v == (2.0 * p * q / (p + q) if p + q > 0 else 0.0), (tag, step)
    # the real control: the leave-one-out scores of the eval examples (8 x 32 frames of 42), against float64
    x = eval_examples(flags, 8, monkeypatch).reshape(-1, 42)
    assert x.shape == (256, 42)
    k = 3
    m = R.d2_error_bound(42, x, x)
    dxx = R.sqdist(x)
    r2 = R.knn_radii2(x, k, dxx)
    s, certain = R.loo_certain(dxx, r2, k, m)
    und = int((~certain).sum())
    loo = float((s >= 0).mean())
    print(f"  real control: precision {got[('real/improved_precision', 0)]:.6f}, float64 leave-one-out {loo:.6f}, undecidable rows {und} of 256")
    assert und <= 0.005 * 256, "the float64 reference alone exceeds the cap: a bad test input"
    assert abs(got[("real/improved_precision", 0)] - loo) <= und / 256
    assert got[("real/improved_recall", 0)] == got[("real/improved_precision", 0)]
    # realism of the control: every kept pair distance is far above 2m here, so each row's squared score lies between
    # max_j (r2_j - m) / (d2 + m) and max_j (r2_j + m) / (d2 - m); when no radius is within 2 m / r of the median the kept set is float64's
    r = np.sqrt(r2)
    keep = R.keep_mask(r2)
    if not (np.abs(r - np.median(r)) <= 2 * (m / r).max()).any():
        dk = np.where(keep[None, :], dxx, np.inf)
        np.fill_diagonal(dk, np.inf)
        assert dk.min() > 2 * m
        lo = np.sqrt(((r2[None, :] - m) / (dk + m)).max(1)).mean()
        hi = np.sqrt(((r2[None, :] + m) / (dk - m)).max(1)).mean()
        print(f"  real control: ipr_realism {got[('real/ipr_realism', 0)]:.6f} in [{lo:.6f}, {hi:.6f}]")
        assert lo * (1 - 2.0 ** -22) <= got[("real/ipr_realism", 0)] <= hi * (1 + 2.0 ** -22)
    # the stats line has the four keys; the warning names only the k-means metrics as not computed
    assert all(n in log for n in NN) and "frechet_dist" in log
    warning = [ln for ln in log.splitlines() if "utils/metrics.py does not define" in ln]
    assert len(warning) == 1 and "precision, recall, f1, ndb of the reference" in warning[0]
    assert "are computed as DESIGN.md section 14 defines them (k = 3)" in warning[0]
    assert not os.path.exists(out / "ncsn" / "generated.pkl")


def test_compute_final_only_leaves_one_ncsn_point(trained):
    d, flags = trained
    out = d / "final_only"
    run("sample_ncsn.py", *flags, "--sample_size=8", f"--sampling_dir={out}", "--compute_metrics=true", "--nn_metrics=true",
        "--nn_k=2", "--compute_final_only=true")
    rows = scalars(out)
    assert len(rows) == 7 * 3
    for name in NN:
        assert sorted(r["step"] for r in rows if r["tag"] == f"ncsn/{name}") == [0]
    assert {r["tag"].split("/")[0] for r in rows} == {"ncsn", "random", "real"}


def test_without_nn_metrics_nothing_changes(trained):
    d, flags = trained
    out = d / "plain"
    r = run("sample_ncsn.py", *flags, "--sample_size=8", f"--sampling_dir={out}", "--compute_metrics=true", "--compute_final_only=true",
            "--flush=false")
    assert {row["tag"].split("/")[1] for row in scalars(out)} == set(DIST)
    assert "ipr_realism" in r.stderr + r.stdout and "only frechet_distance, mmd_rbf and mmd_polynomial are computed" in r.stderr + r.stdout


def test_refusals_exit_with_their_sentence(trained):
    d, flags = trained
    r = run("sample_ncsn.py", *flags, "--sample_size=8", f"--sampling_dir={d / 'refused'}", "--nn_metrics=true", ok=False)
    assert r.returncode != 0 and "it needs --compute_metrics" in r.stderr
    r = run("sample_ncsn.py", *flags, "--sample_size=8", f"--sampling_dir={d / 'refused'}", "--nn_metrics=true", "--interpolate=true", ok=False)
    assert r.returncode != 0 and "--nn_metrics does not apply to --interpolate" in r.stderr
    assert not os.path.exists(d / "refused")
