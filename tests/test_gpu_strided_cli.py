"""sample_ncsn.py --ddim_steps end to end on the GPU: freshly initialised tiny weights (synthetic (32, 512) latents, 2 layers, T = 50), 8 samples,
8 of the 50 timesteps -- generation, --infill, --interpolate with and without --ddim_encode, --compute_metrics and --dtype=fp32
write the reference's files in the reference's shapes.  The driver runs in this process: what is under test is its routing."""
import importlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("strided_cli")
    sl = np.arange(512)                    # synthetic latents are not sliced: every dimension is the model's
    flags = [f"--flagfile={ROOT}/configs/ddpm-mel-32seq-512.cfg", "--synthetic", "--slice_ckpt=", f"--model_dir={d / 'no_model'}", "--num_layers=2", "--mlp_dims=256", "--num_mlp_layers=1", "--num_sigmas=50",
             "--sample_size=8", "--ddim_steps=8"]
    return d, flags, sl


def sample(work, name, *extra):
    import smd_amd.data as D
    d, flags, _ = work
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    sm = importlib.import_module("sample_ncsn")
    out = d / name
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        sm.main(["sample_ncsn.py", *flags, f"--sampling_dir={out}", *extra])
    finally:
        os.chdir(cwd)
    load = lambda f: D.load(str(out / "ncsn" / f)) if os.path.exists(out / "ncsn" / f) else None
    return out, load("generated.pkl"), load("collection.pkl"), load("real.pkl")


def test_generation_is_repeatable_at_eta_zero(work):
    _, _, sl = work
    _, gen, coll, real = sample(work, "gen")
    assert gen.shape == (8, 32, 512) and coll.shape == (41, 8, 32, 512) and real.shape == (8, 32, 512)
    assert np.isfinite(gen).all() and np.abs(coll[40][..., sl]).max() > 0 and np.abs(coll[1][..., sl]).max() == 0
    _, gen2, _, _ = sample(work, "gen2")
    assert np.array_equal(gen[..., sl], gen2[..., sl])
    _, gen3, _, _ = sample(work, "gen3", "--ddim_eta=1.0")
    assert not np.allclose(gen[..., sl], gen3[..., sl])


def test_infill_keeps_the_context_rows(work):
    _, _, sl = work
    _, gen, coll, real = sample(work, "infill", "--infill=true", "--ddim_eta=0.5")
    fixed, free = list(range(8)) + list(range(24, 32)), list(range(8, 24))
    assert gen.shape == (8, 32, 512) and coll.shape == (41, 8, 32, 512)
    assert np.array_equal(gen[:, fixed][..., sl], real[:, fixed][..., sl])
    assert not np.allclose(gen[:, free][..., sl], real[:, free][..., sl])


@pytest.mark.parametrize("encode", [False, True])
def test_interpolate(work, encode):
    out, gen, coll, _ = sample(work, f"interp{int(encode)}", "--interpolate=true", *(["--ddim_encode=true"] if encode else []))
    assert gen.shape == (9, 8, 32, 512) and np.isfinite(gen).all() and coll is None


def test_compute_metrics_on_the_collection(work):
    out, gen, _, _ = sample(work, "metrics", "--compute_metrics=true", "--compute_final_only=true")
    with open(out / "scalars.jsonl") as f:
        rows = [json.loads(line) for line in f]
    got = {r["tag"]: r["value"] for r in rows if r["step"] == 0}
    assert all(np.isfinite(got[f"ncsn/{m}"]) for m in ("frechet_distance", "mmd_rbf", "mmd_polynomial"))
    assert gen.shape == (8, 32, 512)


def test_fp32(work):
    _, gen, coll, _ = sample(work, "fp32", "--dtype=fp32")
    assert gen.shape == (8, 32, 512) and coll.shape == (41, 8, 32, 512) and np.isfinite(gen).all()
