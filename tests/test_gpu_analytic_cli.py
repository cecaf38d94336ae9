"""sample_ncsn.py --analytic_variance end to end on the GPU: freshly initialised tiny weights (synthetic (32, 512) latents, 2
layers, T = 50), 8 samples, --ddim_steps=8 --ddim_eta=1.  The driver runs in this process: what is under test is its routing,
the moments sidecar and the bound's new fields."""
import importlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ("generated.pkl", "collection.pkl", "real.pkl")
EX = "--analytic_examples=16"


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("analytic_cli")
    flags = [f"--flagfile={ROOT}/configs/ddpm-mel-32seq-512.cfg", "--synthetic", "--slice_ckpt=", f"--model_dir={d / 'no_model'}", "--num_layers=2",
             "--mlp_dims=256", "--num_mlp_layers=1", "--num_sigmas=50", "--sample_size=8", "--sampling=ddpm", "--ddim_steps=8",
             "--ddim_eta=1"]
    return d, flags


def sample(work, name, *extra):
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
    load = lambda f: D.load(str(out / "ncsn" / f)) if os.path.exists(out / "ncsn" / f) else None
    return out, [load(f) for f in FILES]


def file_bytes(out, names=FILES):
    return {f: open(out / "ncsn" / f, "rb").read() for f in names}


def test_element_generation_writes_the_sidecar_and_a_second_run_loads_it(work, monkeypatch):
    import smd_amd.analytic as AN
    import smd_amd.ncsn as N
    out, (gen, coll, real) = sample(work, "gen", "--analytic_variance=element", EX)
    assert gen.shape == (8, 32, 512) and coll.shape == (41, 8, 32, 512) and np.isfinite(gen).all() and np.isfinite(coll).all()
    side = out / "ncsn" / AN.MOMENTS_FILE
    g, ts, count, meta = AN.load_moments(str(side))
    assert g.shape == (8, 32, 512) and len(ts) == 8 and count == 16 and meta["prediction"] == "eps" and meta["num_sigmas"] == "50"
    assert (g > 0).all() and np.isfinite(g).all()
    _, (plain, _, _) = sample(work, "plain", "--analytic_variance=none")
    assert not np.array_equal(gen, plain)                              # the variance is in the walk
    # the second run must not estimate
    def refuse(*a, **k):
        raise AssertionError("--analytic_moments re-estimated")
    monkeypatch.setattr(N, "estimate_score_moments", refuse)
    out2, _ = sample(work, "gen2", "--analytic_variance=element", f"--analytic_moments={side}")
    assert file_bytes(out) == file_bytes(out2)
    assert not os.path.exists(out2 / "ncsn" / AN.MOMENTS_FILE)
    # a file that contradicts the run, or does not cover the walk, is refused with the flag's name
    with pytest.raises(SystemExit, match="--analytic_moments=.*num_sigmas=50, this run has num_sigmas=40"):
        sample(work, "bad", "--analytic_variance=element", f"--analytic_moments={side}", "--num_sigmas=40")
    with pytest.raises(SystemExit, match="--analytic_moments=.*do not cover the walk"):
        sample(work, "bad2", "--analytic_variance=element", f"--analytic_moments={side}", "--ddim_steps=12")


@pytest.mark.parametrize("mode", ["--infill=true", "--interpolate=true"])
def test_infill_and_interpolate_walk_with_the_variance(work, mode):
    out, (gen, coll, real) = sample(work, "m" + mode[2:6], mode, "--analytic_variance=scalar", EX)
    assert np.isfinite(gen).all() and gen.shape[-2:] == (32, 512)
    if "infill" in mode:
        fixed = list(range(8)) + list(range(24, 32))
        assert np.allclose(gen[:, fixed], real[:, fixed], atol=1e-6)


def test_bound_of_the_k_step_chain_is_a_number(work):
    out, _ = sample(work, "bound", "--compute_bound", "--bound_only", "--bound_steps=8", "--analytic_variance=scalar", EX)
    rep = json.load(open(out / "ncsn" / "bound.json"))
    assert rep["total"] is None and rep["exact"] is False              # the fixed-variance fields are as they were
    assert np.isfinite(rep["analytic_total"]) and np.isfinite(rep["analytic_bits_per_dim"])
    assert len(rep["analytic_terms"]) == len(rep["sigma2_ratio"]) == len(rep["timesteps"]) == 8
    assert all(r >= 1 - 1e-9 for r in rep["sigma2_ratio"])
    plain, _ = sample(work, "bound_plain", "--compute_bound", "--bound_only", "--bound_steps=8")
    rep0 = json.load(open(plain / "ncsn" / "bound.json"))
    assert not any(k.startswith("analytic") or k == "sigma2_ratio" for k in rep0)
    assert {k: rep[k] for k in rep0} == rep0


@pytest.mark.parametrize("extra,msg", [
    (["--ddim_steps=0", "--ddim_eta=0"], "--analytic_variance=element belongs to the strided sampler: give --ddim_steps"),
    (["--ddim_order=2", "--ddim_spacing=logsnr", "--ddim_eta=0"], "with --ddim_order=2"),
    (["--compute_bound"], "--analytic_variance=element with --compute_bound"),
])
def test_refusals_exit_with_their_message(work, extra, msg):
    with pytest.raises(SystemExit, match=msg):
        sample(work, "refused", "--analytic_variance=element", *extra)


def test_other_samplers_and_ranks_are_refused(work, monkeypatch):
    with pytest.raises(SystemExit, match="--analytic_variance=scalar.*needs --sampling=ddpm"):
        sample(work, "refused", "--analytic_variance=scalar", "--sampling=ald", "--ddim_steps=0", "--ddim_eta=0")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="single process"):
        sample(work, "refused", "--analytic_variance=scalar")
