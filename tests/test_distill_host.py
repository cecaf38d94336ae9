"""Host side of progressive distillation: the walks, the [N][16] table and its convex target weights, the
loss weights, the float64 reference of the kernels (tests/_distill_ref.py) and the refusals.  No GPU needed."""
import numpy as np
import pytest

import _distill_ref as R

KINDS = ("eps", "x0", "v")


def real_betas():
    import smd_amd.schedule as S
    return S.create_noise_schedule(1e-6, 0.01, 1000, "linear")


def small_betas(T=16):
    return np.linspace(1e-3, 0.2, T).astype(np.float32)


@pytest.mark.parametrize("N", [1, 2, 4, 128, 500])
def test_target_weights_are_convex_on_the_real_schedule(N):
    import smd_amd.schedule as S
    betas = real_betas()
    tw, sw = S.distill_walk(len(betas), N)
    assert len(tw) == 2 * N and list(sw) == list(tw[0::2]) and tw[0] == len(betas) - 1 and tw[-1] == 0
    table, ref = S.distill_tables(betas, tw, "v", "v", "truncated_snr")
    assert table.shape == (N, 16) and table.dtype == np.float32 and table.flags["C_CONTIGUOUS"]
    assert np.max(np.abs(ref["w1"] + ref["w2"] - 1.0)) <= 1e-15
    assert (ref["w1"] >= 0).all() and (ref["w2"] >= 0).all()
    assert ref["w1"][-1] == 0.0 and ref["w2"][-1] == 1.0                 # the clean step
    # D, formed as a' + a b', is the D of the definition, alpha_u - r alpha_t; and b' b = r: the cancellation of the z_t terms
    D_def = ref["alpha_u"] - ref["r"] * ref["alpha_t"]
    assert np.max(np.abs(ref["D"] - D_def)) <= 1e-14
    assert np.max(np.abs(ref["b2"] * ref["b"] - ref["r"])) <= 1e-15
    assert (ref["D"] > 0).all()


@pytest.mark.parametrize("N", [1, 2, 4, 128, 500])
def test_convex_form_agrees_with_the_quotient_form(N):
    import smd_amd.schedule as S
    betas = real_betas()
    tw, _ = S.distill_walk(len(betas), N)
    _, ref = S.distill_tables(betas, tw, "x0", "x0", "none")
    g = np.random.default_rng(27 + N)
    x1, x2, z_t = g.uniform(-1, 1, (3, N, 64))
    col = lambda k: ref[k][:, None]
    z_m = col("a") * x1 + col("b") * z_t
    z_u = col("a2") * x2 + col("b2") * z_m
    quot = R.quotient_target(z_t, z_u, col("alpha_t"), col("sigma_t"), col("alpha_u"), col("sigma_u"))
    conv = col("w1") * x1 + col("w2") * x2
    assert (np.abs(quot - conv) <= 1e-9 / col("D")).all(), float(np.max(np.abs(quot - conv) * col("D")))


@pytest.mark.parametrize("student", KINDS)
@pytest.mark.parametrize("teacher", KINDS)
def test_an_exact_teacher_gives_the_exact_target(teacher, student):
    """teacher outputs = the kind-targets of a fixed x*: x~ == x*, the student's target == the kind-target of x* at t"""
    import smd_amd.schedule as S
    betas = real_betas()
    ap = S.alphas_cumprod(betas).astype(np.float64)
    tw, _ = S.distill_walk(len(betas), 8)
    _, ref = S.distill_tables(betas, tw, teacher, student, "none")
    tk, sk = S.prediction_kind(teacher), S.prediction_kind(student)
    g = np.random.default_rng(5)
    xs = g.uniform(-0.9, 0.9, (8, 48))
    eps = g.standard_normal((8, 48))
    col = lambda k: ref[k][:, None]
    z_t = col("alpha_t") * xs + col("sigma_t") * eps
    out1 = R.exact_output(tk, xs, z_t, ap[ref["t"]][:, None])
    x1 = R.x_hat(z_t, out1, col("c0_t"), col("c1_t"), 1.0)
    z_m = col("a") * x1 + col("b") * z_t
    out2 = R.exact_output(tk, xs, z_m, ap[ref["m"]][:, None])
    x2 = R.x_hat(z_m, out2, col("c0_m"), col("c1_m"), 1.0)
    xt = col("w1") * x1 + col("w2") * x2
    np.testing.assert_allclose(x1, xs, atol=1e-12, rtol=0)
    np.testing.assert_allclose(xt, xs, atol=1e-12, rtol=0)
    want = R.exact_output(sk, xs, z_t, ap[ref["t"]][:, None])
    got = R.kind_target(sk, xt, z_t, col("alpha_t"), col("inv_sigma_t"))
    np.testing.assert_allclose(got, want, atol=1e-10, rtol=0)
    # z_m IS the forward-noised x* with the same eps: the deterministic step keeps the noise
    np.testing.assert_allclose(z_m, np.sqrt(ap[ref["m"]])[:, None] * xs + ref["sigma_m"][:, None] * eps, atol=1e-12, rtol=0)


def test_the_float64_kernel_reference_on_an_exact_teacher():
    """tests/_distill_ref.py, from the fp32 table: the same identity to the table's rounding; a no-op sample comes back NaN"""
    import smd_amd.schedule as S
    betas = small_betas()
    ap = S.alphas_cumprod(betas).astype(np.float64)
    tw, sw = S.distill_walk(16, 4)
    table, ref = S.distill_tables(betas, tw, "v", "x0", "none")
    steps = np.array([0, 3, 1, 7, 1])
    g = np.random.default_rng(9)
    xs = g.uniform(-0.9, 0.9, (5, 6)).astype(np.float32)
    eps = g.standard_normal((5, 6)).astype(np.float32)
    z_t, level = R.noise(xs, eps, table, steps)
    assert np.isnan(z_t[3]).all() and np.isnan(level[3])
    live = steps < 4
    k = steps[live]
    out1 = R.exact_output(2, xs[live], z_t[live], ap[ref["t"][k]][:, None])
    x1, z_m, level_m, _ = R.mid(z_t[live], out1, table, k)
    out2 = R.exact_output(2, xs[live], z_m, ap[ref["m"][k]][:, None])
    res = R.loss(x1, z_m, out2, z_t[live], xs[live], 1, table, k, None, 1.0 / xs[live].size)
    np.testing.assert_allclose(res["target"], xs[live], atol=2e-6, rtol=0)
    assert (res["loss"] < 1e-11).all() and (res["weight"] == 1.0).all()
    assert level_m.tolist() == table[k, 7].astype(np.float64).tolist()


def test_table_is_rounded_once_from_float64_and_padded():
    import smd_amd.schedule as S
    betas = small_betas()
    tw, sw = S.distill_walk(16, 4)
    assert list(tw) == list(S.stride_timesteps(16, 8))
    table, ref = S.distill_tables(betas, tw, "eps", "v", "truncated_snr", clip=1.0)
    for j, name in enumerate(S.DISTILL_COLUMN_NAMES):
        assert table[:, j].tolist() == ref[name].astype(np.float32).tolist(), name
    assert (table[:, 14:] == 0).all() and (table[:, 4] == 1.0).all()
    co = S.strided_coefficients(betas, tw, 0.0)
    assert ref["a"].tolist() == co["a"][0::2].tolist() and ref["b"].tolist() == co["b"][0::2].tolist()
    c0, c1 = S.x0_coefficients(S.alphas_cumprod(betas).astype(np.float64)[tw], "eps")
    assert ref["c0_t"].tolist() == c0[0::2].tolist() and ref["c1_m"].tolist() == c1[1::2].tolist()
    assert ref["u"].tolist() == [int(t) for t in tw[2::2]] + [-1]


def test_distill_weights_closed_forms():
    import smd_amd.schedule as S
    betas = real_betas()
    ap = S.alphas_cumprod(betas).astype(np.float64)
    walk = S.stride_timesteps(1000, 8)
    snr = ap[walk] / (1 - ap[walk])
    assert snr.min() < 1 < snr.max()                                   # both branches of every max
    for kind in KINDS:
        assert S.distill_weights(ap, walk, kind, "none").tolist() == [1.0] * 8
    np.testing.assert_allclose(S.distill_weights(ap, walk, "x0", "truncated_snr"), np.maximum(snr, 1), rtol=1e-15)
    np.testing.assert_allclose(S.distill_weights(ap, walk, "eps", "truncated_snr"), np.maximum(1, 1 / snr), rtol=1e-15)
    np.testing.assert_allclose(S.distill_weights(ap, walk, "v", "truncated_snr"), np.maximum(snr, 1) / (snr + 1), rtol=1e-15)
    # one x-space weight in three output spaces: w_eps SNR = w_x0 = w_v (SNR + 1)
    np.testing.assert_allclose(S.distill_weights(ap, walk, "eps") * snr, S.distill_weights(ap, walk, "x0"), rtol=1e-14)
    np.testing.assert_allclose(S.distill_weights(ap, walk, "v") * (snr + 1), S.distill_weights(ap, walk, "x0"), rtol=1e-14)
    with pytest.raises(ValueError, match="weighting must be one of"):
        S.distill_weights(ap, walk, "v", "min_snr")


def test_distill_walk_refusals_and_the_second_round():
    import smd_amd.schedule as S
    with pytest.raises(ValueError, match="N >= 1"):
        S.distill_walk(16, 0)
    with pytest.raises(ValueError, match="needs a teacher walk of 18 timesteps, the schedule has 16"):
        S.distill_walk(16, 9)
    with pytest.raises(ValueError, match="needs a teacher walk of 6 timesteps, got 4"):
        S.distill_walk(16, 3, [15, 10, 5, 0])
    for bad in ([15, 10, 10, 0], [0, 5, 10, 15], [16, 10, 5, 0], [15, 10, 5, -1]):
        with pytest.raises(ValueError, match="strictly descending within"):
            S.distill_walk(16, 2, bad)
    tw1, sw1 = S.distill_walk(16, 4)                                   # round 1: 8 -> 4
    tw2, sw2 = S.distill_walk(16, 2, sw1)                              # round 2 takes the recorded walk: 4 -> 2
    assert list(tw2) == list(sw1) and list(sw2) == list(tw1[0::4])
    tw3, sw3 = S.distill_walk(16, 1, sw2)
    assert list(sw3) == [15]
    with pytest.raises(ValueError, match="needs a teacher walk of 6 timesteps, got 4"):
        S.distill_walk(16, 3, sw1)
    table, ref = S.distill_tables(small_betas(), tw3, "v", "v")
    assert table.shape == (1, 16) and ref["w1"][0] == 0.0 and ref["m"][0] == sw2[1]


def _fake_checkpoint(d, **meta):
    """a safetensors file that holds nothing but metadata: what the refusals read before any device is touched"""
    import torch
    from safetensors.torch import save_file
    d.mkdir(parents=True, exist_ok=True)
    save_file({"x": torch.zeros(1)}, str(d / "checkpoint_1"), metadata={k: str(v) for k, v in meta.items()})
    return str(d)


def test_train_flag_refusals_through_main(tmp_path, monkeypatch):
    """every refusal of train_ncsn.py --distill_from is one sentence from main(), before a device is touched"""
    import importlib
    tm = importlib.import_module("train_ncsn")
    plain = _fake_checkpoint(tmp_path / "plain", prediction="v")
    student4 = _fake_checkpoint(tmp_path / "s4", prediction="v", distill_timesteps="15,11,6,2", distill_teacher_steps=8)
    base = ["train_ncsn.py", "--synthetic", "--num_sigmas=16", "--sampling=ddpm", f"--model_dir={tmp_path / 'out'}"]
    on = base + [f"--distill_from={plain}", "--distill_steps=4", "--loss=ddpm", "--prediction=v"]

    def refused(argv, match):
        with pytest.raises(SystemExit, match=match):
            tm.main(argv)

    refused(base + [f"--distill_from={plain}", "--distill_steps=4", "--loss=dsm"], "--distill_from applies to --loss=ddpm only")
    refused(base + [f"--distill_from={plain}", "--distill_steps=4", "--loss=ssm"], "--loss=ddpm")
    refused(on + ["--timestep_sampler=loss_second_moment"], "--timestep_sampler=loss_second_moment is refused")
    refused(on + ["--loss_weighting=min_snr"], "--loss_weighting=min_snr is refused")
    refused(on + ["--ckpt_format=flax"], "--distill_from needs --ckpt_format=safetensors")
    refused(on + ["--dtype=fp8"], "trains the student in bf16")
    refused(base + [f"--distill_from={plain}", "--loss=ddpm"], "--distill_steps=N with N >= 1")
    refused(base + ["--loss=ddpm", "--distill_steps=4"], "--distill_steps: options of progressive distillation, give --distill_from")
    refused(base + ["--loss=ddpm", f"--distill_from={tmp_path / 'nothing'}", "--distill_steps=4"], "no checkpoint there")
    # a teacher walk whose length is not 2N: the recorded walk of 4 timesteps serves N = 2 only; an undistilled teacher on T = 16
    # has no walk of 18 timesteps
    refused(base + ["--loss=ddpm", f"--distill_from={student4}", "--distill_steps=3"],
            "--distill_steps=3: .*needs a teacher walk of 6 timesteps, got 4.*records a walk of 4 timesteps")
    refused(base + ["--loss=ddpm", f"--distill_from={plain}", "--distill_steps=9"], "needs a teacher walk of 18 timesteps")
    # --resume refuses a changed walk: another N, and a distilled run resumed as a plain one
    resumed = _fake_checkpoint(tmp_path / "resumed", prediction="v", distill_timesteps="15,6", distill_teacher_steps=4)
    rbase = ["train_ncsn.py", "--synthetic", "--num_sigmas=16", "--sampling=ddpm", f"--model_dir={resumed}", "--resume", "--loss=ddpm",
             "--prediction=v"]
    refused(rbase + [f"--distill_from={plain}", "--distill_steps=4"],
            "--resume: .* was trained on the distillation walk 15,6, this run asks for the distillation walk 15,11,6,2")
    refused(rbase, "--resume: .* was trained on the distillation walk 15,6, this run asks for no distillation walk")
    monkeypatch.setenv("WORLD_SIZE", "2")
    refused(on, "single-process only .world size 2.")


def test_sample_flag_refusals_through_main(tmp_path):
    import importlib
    sm = importlib.import_module("sample_ncsn")
    student4 = _fake_checkpoint(tmp_path / "s4", prediction="v", distill_timesteps="15,11,6,2", distill_teacher_steps=8)
    base = ["sample_ncsn.py", "--synthetic", "--num_sigmas=16", "--sampling=ddpm", "--loss=ddpm", f"--model_dir={student4}"]
    with pytest.raises(SystemExit, match="--ddim_steps=5: .* was distilled to the 4 timesteps 15,11,6,2; drop the flag or pass --ddim_steps=4"):
        sm.main(base + ["--ddim_steps=5"])
    with pytest.raises(SystemExit, match="--ddim_spacing=logsnr chooses the timesteps itself"):
        sm.main(base + ["--ddim_spacing=logsnr"])
    with pytest.raises(SystemExit, match="--ddim_encode inverts an evenly spaced walk"):
        sm.main(base + ["--interpolate", "--ddim_encode"])
    with pytest.raises(SystemExit, match="--num_sigmas=8: .* was distilled to the 4 timesteps"):
        sm.main(["sample_ncsn.py", "--synthetic", "--num_sigmas=8", "--sampling=ddpm", "--loss=ddpm", f"--model_dir={student4}"])


def test_checkpoint_walk_helpers(tmp_path):
    from smd_amd import checkpoint
    plain = _fake_checkpoint(tmp_path / "plain", prediction="v")
    s4 = _fake_checkpoint(tmp_path / "s4", distill_timesteps="15,11,6,2")
    assert checkpoint.checkpoint_distill_walk(plain) is None and checkpoint.checkpoint_distill_walk(str(tmp_path / "none")) is None
    assert checkpoint.checkpoint_distill_walk(s4) == [15, 11, 6, 2] and checkpoint.format_walk([15, 6]) == "15,6"
    checkpoint.check_resume_distill(plain, None)
    checkpoint.check_resume_distill(s4, [15, 11, 6, 2])
    checkpoint.check_resume_distill(str(tmp_path / "none"), [3, 1])
    with pytest.raises(ValueError, match="no distillation walk, this run asks for the distillation walk 3,1"):
        checkpoint.check_resume_distill(plain, [3, 1])


def test_training_option_helper():
    import smd_amd.schedule as S
    import smd_amd.trainer as T
    assert T.DISTILL_WEIGHTINGS is S.DISTILL_WEIGHTINGS
    T.validate_distill_options(distill_steps=4)
    with pytest.raises(ValueError, match="--distill_weighting must be one of"):
        T.validate_distill_options(distill_steps=4, distill_weighting="min_snr")


def test_the_exports_are_declared_and_bound():
    import smd_amd.lib as lib
    import smd_amd.build as build
    for name in ("smd_distill_noise", "smd_distill_mid", "smd_distill_loss"):
        assert name in lib.declared_symbols(lab=False) and name in lib._SIGS
    assert "distill.hip" in build.SOURCES
