"""train_ncsn.py --distill_from and sample_ncsn.py on its checkpoints, end to end, --synthetic at T = 16 on
the two-layer network of tests/test_gpu_prediction_cli.py: a v teacher trained for a few steps, a student of 4 steps distilled
from it, sampling on the recorded walk (asserted on the alpha row of the sampler's ld_metrics), a second round to 2 steps that
takes its teacher walk from the checkpoint, and the refusals that need a real checkpoint.  Both commands run in-process through
their main()."""
import importlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = [f"--flagfile={ROOT}/configs/ddpm-mel-32seq-512.cfg", "--synthetic", "--slice_ckpt=", "--num_layers=2", "--mlp_dims=256",
         "--num_mlp_layers=1", "--num_sigmas=16"]
TRAIN = ["--synthetic_examples=256", "--loss=ddpm", "--batch_size=8", "--logging_freq=2", "--snapshot_freq=4",
         "--snapshot_sampling=false", "--max_steps=8", "--prediction=v"]


def _main(script, *flags):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    mod = importlib.import_module(script)
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        mod.main([script + ".py", *MODEL, *flags])
    finally:
        os.chdir(cwd)
    return mod


def _meta(d):
    from safetensors import safe_open
    from smd_amd import checkpoint
    with safe_open(checkpoint.latest_checkpoint(str(d)), framework="pt") as f:
        return dict(f.metadata())


def _alphas():
    """the cumulative alphas of the run's schedule, from the same flags"""
    from smd_amd import flags as F
    from smd_amd import schedule
    FL = F.make_flags(include_sample=True)
    FL.parse(MODEL)
    betas = schedule.create_noise_schedule(FL.sigma_begin, FL.sigma_end, FL.num_sigmas, schedule=FL.schedule_type)
    return schedule.alphas_cumprod(betas)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """teacher -> student of 4 steps -> student of 2 steps, trained once"""
    d = tmp_path_factory.mktemp("distill_cli")
    teacher, s4, s2 = d / "teacher", d / "s4", d / "s2"
    _main("train_ncsn", *TRAIN, f"--model_dir={teacher}")
    _main("train_ncsn", *TRAIN, f"--model_dir={s4}", f"--distill_from={teacher}", "--distill_steps=4")
    _main("train_ncsn", *TRAIN, f"--model_dir={s2}", f"--distill_from={s4}", "--distill_steps=2", "--distill_weighting=none")
    return d, teacher, s4, s2


def test_checkpoints_record_the_walks(runs):
    _, teacher, s4, s2 = runs
    mt, m4, m2 = _meta(teacher), _meta(s4), _meta(s2)
    assert mt["prediction"] == "v" and "distill_timesteps" not in mt and "distill_teacher_steps" not in mt
    assert m4["distill_timesteps"] == "15,11,6,2" and m4["distill_teacher_steps"] == "8" and m4["prediction"] == "v"
    assert m2["distill_timesteps"] == "15,6" and m2["distill_teacher_steps"] == "4"       # the teacher walk came from s4's checkpoint
    rows = [json.loads(line) for line in open(s4 / "train" / "scalars.jsonl")]
    for tag in ("loss", "loss_unweighted", "grad", "lr"):
        v = [r["value"] for r in rows if r["tag"] == tag]
        assert len(v) >= 4 and np.isfinite(v).all(), (tag, v)


def test_the_student_starts_from_the_teacher_and_moves(runs):
    import torch
    from safetensors.torch import load_file
    from smd_amd import checkpoint
    _, teacher, s4, _ = runs
    t = load_file(checkpoint.latest_checkpoint(str(teacher)))
    s = load_file(checkpoint.latest_checkpoint(str(s4)))
    keys = [k for k in t if k.startswith("target/params/")]
    assert keys and all(t[k].shape == s[k].shape for k in keys)
    num = sum(float((t[k].double() - s[k].double()).pow(2).sum()) for k in keys) ** 0.5
    den = sum(float(t[k].double().pow(2).sum()) for k in keys) ** 0.5
    assert 0 < num / den < 0.1, num / den                  # 8 Adam steps from the teacher's parameters, not a fresh initialisation
    assert torch.isfinite(torch.cat([s[k].flatten() for k in keys])).all()


def test_sampling_walks_the_recorded_walk(runs, monkeypatch):
    from smd_amd import data
    d, _, s4, s2 = runs
    ap = _alphas()
    sm = importlib.import_module("sample_ncsn")
    seen = []
    real = sm.generate_samples

    def spy(*a, **kw):
        out = real(*a, **kw)
        seen.append(out[2])
        return out

    monkeypatch.setattr(sm, "generate_samples", spy)
    for name, model, walk, extra in (("a", s4, [15, 11, 6, 2], []), ("b", s4, [15, 11, 6, 2], ["--ddim_steps=4", "--ddim_order=2"]),
                                     ("c", s2, [15, 6], [])):
        out = d / f"sample_{name}"
        _main("sample_ncsn", f"--model_dir={model}", "--sample_size=8", "--sampling=ddpm", f"--sampling_dir={out}", *extra)
        ld = seen.pop()
        assert len(ld) == len(walk), "one row of ld_metrics per timestep of the recorded walk"
        assert [float(row[0]["alpha"]) for row in ld] == [float(a) for a in ap[walk]]
        g = np.asarray(data.load(str(out / "ncsn" / "generated.pkl")))
        assert g.shape[0] == 8 and np.isfinite(g).all()
    monkeypatch.undo()
    out = d / "sample_infill"
    _main("sample_ncsn", f"--model_dir={s4}", "--sample_size=8", "--sampling=ddpm", f"--sampling_dir={out}", "--infill=true")
    assert np.isfinite(np.asarray(data.load(str(out / "ncsn" / "generated.pkl")))).all()


def test_refusals_on_real_checkpoints(runs):
    d, teacher, s4, _ = runs
    tm = importlib.import_module("train_ncsn")
    sm = importlib.import_module("sample_ncsn")
    with pytest.raises(SystemExit, match="--distill_steps=3: .*needs a teacher walk of 6 timesteps, got 4"):
        tm.main(["train_ncsn.py", *MODEL, *TRAIN, f"--model_dir={d / 'no3'}", f"--distill_from={s4}", "--distill_steps=3"])
    with pytest.raises(SystemExit, match="--resume: .* the distillation walk 15,11,6,2, this run asks for no distillation walk"):
        tm.main(["train_ncsn.py", *MODEL, *TRAIN, f"--model_dir={s4}", "--resume"])
    with pytest.raises(SystemExit, match="--resume: .* the distillation walk 15,11,6,2, this run asks for the distillation walk 15,6"):
        tm.main(["train_ncsn.py", *MODEL, *TRAIN, f"--model_dir={s4}", "--resume", f"--distill_from={s4}", "--distill_steps=2"])
    with pytest.raises(SystemExit, match="--ddim_steps=3: .* was distilled to the 4 timesteps 15,11,6,2"):
        sm.main(["sample_ncsn.py", *MODEL, f"--model_dir={s4}", "--sample_size=8", "--sampling=ddpm", "--ddim_steps=3",
                 f"--sampling_dir={d / 'no'}"])
    assert not os.path.exists(d / "no3") or not os.listdir(d / "no3")
