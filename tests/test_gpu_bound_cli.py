"""sample_ncsn.py --compute_bound end to end on the GPU: freshly initialised tiny weights (synthetic (32, 512) latents, 2 layers,
T = 40), 8 examples.  --bound_only writes bound.json and bound_terms.pkl and no samples; --bound_steps writes the curve without a
total; without --compute_bound neither file appears.  The driver runs in this process: what is under test is its routing."""
import importlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"nats_per_dim", "bits_per_dim", "total", "prior", "timesteps", "terms", "eps_mse", "dtype", "num_examples", "clip", "var_0", "exact"}


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("bound_cli")
    flags = [f"--flagfile={ROOT}/configs/ddpm-mel-32seq-512.cfg", "--synthetic", "--slice_ckpt=", f"--model_dir={d / 'no_model'}", "--num_layers=2",
             "--mlp_dims=256", "--num_mlp_layers=1", "--num_sigmas=40", "--sample_size=8"]
    return d, flags


def run(work, name, *extra):
    import smd_amd.data as D
    d, flags = work
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
    js = json.load(open(out / "ncsn" / "bound.json")) if os.path.exists(out / "ncsn" / "bound.json") else None
    pk = D.load(str(out / "ncsn" / "bound_terms.pkl")) if os.path.exists(out / "ncsn" / "bound_terms.pkl") else None
    return out, js, pk


def test_bound_only_writes_the_bound_and_no_samples(work):
    out, js, pk = run(work, "exact", "--compute_bound", "--bound_only")
    assert set(js) == KEYS and js["exact"] is True and js["dtype"] == "bf16" and js["num_examples"] == 8 and js["clip"] == 1.0
    assert js["timesteps"] == list(range(40)) and len(js["terms"]) == 40 and len(js["eps_mse"]) == 40
    D = 32 * 512
    assert np.isfinite(js["bits_per_dim"]) and abs(js["bits_per_dim"] - js["total"] / (D * np.log(2))) < 1e-9 * abs(js["bits_per_dim"])
    assert abs(js["nats_per_dim"] - js["total"] / D) < 1e-9 * abs(js["nats_per_dim"]) and js["var_0"] > 0
    assert pk["terms"].shape == (40, 8) and pk["eps_mse"].shape == (40, 8) and pk["prior"].shape == (8,) and pk["total"].shape == (8,)
    assert np.array_equal(pk["timesteps"], np.arange(40))
    assert np.allclose(pk["terms"].mean(axis=1), js["terms"], rtol=1e-12) and abs(pk["total"].mean() - js["total"]) <= 1e-9 * abs(js["total"])
    for f in ("generated.pkl", "collection.pkl", "real.pkl"):
        assert not os.path.exists(out / "ncsn" / f), f
    _, js2, pk2 = run(work, "exact2", "--compute_bound", "--bound_only")               # --sample_seed keys the draws
    assert js2 == js and np.array_equal(pk2["terms"], pk["terms"])


def test_bound_steps_writes_the_curve_without_a_total(work):
    _, js, pk = run(work, "stride", "--compute_bound", "--bound_only", "--bound_steps=8")
    assert set(js) == KEYS and js["exact"] is False
    assert js["total"] is None and js["bits_per_dim"] is None and js["nats_per_dim"] is None
    assert len(js["timesteps"]) == 8 and js["timesteps"][0] == 0 and js["timesteps"][-1] == 39
    assert pk["terms"].shape == (8, 8) and pk["total"] is None


def test_without_the_flag_nothing_changes(work):
    out, js, pk = run(work, "plain", "--ddim_steps=4")
    assert js is None and pk is None
    assert os.path.exists(out / "ncsn" / "generated.pkl")
    out, js, _ = run(work, "both", "--compute_bound", "--ddim_steps=4")               # the bound, then the usual sampling run
    assert js["exact"] is True and os.path.exists(out / "ncsn" / "generated.pkl")
    import smd_amd.data as D
    a, b = D.load(str(work[0] / "plain" / "ncsn" / "generated.pkl")), D.load(str(out / "ncsn" / "generated.pkl"))
    assert np.array_equal(a, b)                                                       # the sampler's draws are not disturbed
