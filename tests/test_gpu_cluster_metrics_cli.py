"""sample_ncsn.py --compute_metrics --cluster_metrics end to end on the GPU: the tiny model of test_gpu_nn_metrics_cli.py, then
the four k-means scalars per point of evaluate() in <sampling_dir>/scalars.jsonl, the warning texts of every flag combination
and the refusals of the flag check."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIST = ("frechet_distance", "mmd_rbf", "mmd_polynomial")
NN = ("improved_precision", "improved_recall", "improved_f1", "ipr_realism")
KM = ("precision", "recall", "f1", "ndb")


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
    d = tmp_path_factory.mktemp("cluster_metrics_cli")
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


def warnings_of(r):
    return [ln for ln in (r.stdout + r.stderr).splitlines() if "utils/metrics.py does not define" in ln]


def test_cluster_metrics_writes_four_more_scalars_per_point(trained):
    d, flags = trained
    out = d / "samples"
    r = run("sample_ncsn.py", *flags, "--sample_size=8", f"--sampling_dir={out}", "--compute_metrics=true", "--cluster_metrics=true",
            "--prd_runs=2", "--flush=false")
    log = r.stdout + r.stderr
    rows = scalars(out)
    got = {(r_["tag"], r_["step"]): r_["value"] for r_ in rows}
    names = DIST + KM
    assert len(got) == len(rows) == 7 * 22
    assert set(got) == ({(f"ncsn/{m}", i) for m in names for i in range(20)} | {(f"random/{m}", 0) for m in names}
                        | {(f"real/{m}", 0) for m in names})
    assert all(np.isfinite(v) for v in got.values())
    for (tag, step), v in got.items():
        model, name = tag.split("/")
        if name in KM:
            assert 0.0 <= v <= 1.0, (tag, step, v)
        if name == "f1":
            p, q = got[(f"{model}/precision", step)], got[(f"{model}/recall", step)]
            assert v == (2.0 * p * q / (p + q) if p + q > 0 else 0.0), (tag, step)
        if name == "ndb":
            assert abs(v * 50 - round(v * 50)) <= 1e-9              # a count of the 50 bins
    # the real control: equal histograms and no different bin
    assert abs(got[("real/precision", 0)] - 1.0) <= 1e-6 and abs(got[("real/recall", 0)] - 1.0) <= 1e-6 and got[("real/ndb", 0)] == 0.0
    print(f"  random control: precision {got[('random/precision', 0)]:.4f} recall {got[('random/recall', 0)]:.4f} ndb {got[('random/ndb', 0)]:.2f}")
    # the stats line has the four keys; the warning names the nearest-neighbour metrics as what is still not computed
    stats = [ln for ln in log.splitlines() if "frechet_dist" in ln]
    assert stats and all(f"| {n} " in stats[-1] for n in KM)
    w = warnings_of(r)
    assert len(w) == 1 and "improved_precision, improved_recall, improved_f1, ipr_realism of the reference" in w[0]
    assert "precision, recall, f1, ndb are computed as DESIGN.md section 15 defines them (20 clusters x 2 runs, 50 bins)" in w[0]


def test_every_metric_flag_on_leaves_nothing_to_warn_about(trained):
    d, flags = trained
    out = d / "all"
    r = run("sample_ncsn.py", *flags, "--sample_size=8", f"--sampling_dir={out}", "--compute_metrics=true", "--cluster_metrics=true",
            "--nn_metrics=true", "--prd_runs=1", "--prd_clusters=8", "--ndb_bins=16", "--compute_final_only=true", "--flush=false")
    rows = scalars(out)
    assert len(rows) == 11 * 3 and {row["tag"].split("/")[1] for row in rows} == set(DIST + NN + KM)
    # per point: the three distances, then the nearest-neighbour four, then the k-means four
    assert [row["tag"] for row in rows[:11]] == [f"ncsn/{m}" for m in DIST + NN + KM]
    assert warnings_of(r) == []


def test_without_the_flag_nothing_changes(trained):
    d, flags = trained
    r = run("sample_ncsn.py", *flags, "--sample_size=8", f"--sampling_dir={d / 'plain'}", "--compute_metrics=true",
            "--compute_final_only=true", "--flush=false")
    assert [row["tag"] for row in scalars(d / "plain")] == [f"{m}/{n}" for m in ("ncsn", "random", "real") for n in DIST]
    w = warnings_of(r)
    assert len(w) == 1 and w[0].endswith(
        "--compute_metrics: precision, recall, f1, improved_precision, improved_recall, improved_f1, ipr_realism, ndb of the reference's "
        "evaluate() call functions that utils/metrics.py does not define; only frechet_distance, mmd_rbf and mmd_polynomial are computed")
    r = run("sample_ncsn.py", *flags, "--sample_size=8", f"--sampling_dir={d / 'nn'}", "--compute_metrics=true", "--nn_metrics=true",
            "--compute_final_only=true", "--flush=false")
    assert [row["tag"] for row in scalars(d / "nn")] == [f"{m}/{n}" for m in ("ncsn", "random", "real") for n in DIST + NN]
    w = warnings_of(r)
    assert len(w) == 1 and w[0].endswith(
        "--compute_metrics: precision, recall, f1, ndb of the reference's evaluate() call functions that utils/metrics.py does not define "
        "and are not computed; improved_precision, improved_recall, improved_f1, ipr_realism are computed as DESIGN.md section 14 defines "
        "them (k = 3)")


def test_refusals_exit_with_their_sentence(trained):
    d, flags = trained
    common = ["--sample_size=8", f"--sampling_dir={d / 'refused'}"]
    r = run("sample_ncsn.py", *flags, *common, "--cluster_metrics=true", ok=False)
    assert r.returncode != 0 and "it needs --compute_metrics" in r.stderr
    r = run("sample_ncsn.py", *flags, *common, "--cluster_metrics=true", "--interpolate=true", ok=False)
    assert r.returncode != 0 and "--cluster_metrics does not apply to --interpolate" in r.stderr
    r = run("sample_ncsn.py", *flags, "--sample_size=1", f"--sampling_dir={d / 'refused'}", "--compute_metrics=true",
            "--cluster_metrics=true", ok=False)
    assert r.returncode != 0 and "are 32 frames, fewer than the 50 clusters" in r.stderr
    assert not os.path.exists(d / "refused")
