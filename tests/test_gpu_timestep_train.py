"""Weighted training through trainer.train_step: the default path stays the unweighted one bit for bit,
the fused weighted step against the generic autograd path, the timestep sampler's state against tests/_timestep_ref.py, and
the refusals.  Network: the smallest the CLI tests train (2 encoder layers, one DenseResBlock pair of width 256, C = 42)."""
import numpy as np
import pytest
import torch

import _timestep_ref as R
import ddpm_oracle as O

pytestmark = pytest.mark.gpu

BETAS = O.create_noise_schedule(1e-6, 0.01, 1000, "linear")
KW = dict(num_layers=2, num_heads=8, num_mlp_layers=1, mlp_dims=256)
SHAPE = (32, 42)

# ||g_fused - g_generic|| / ||g_generic|| of the UNWEIGHTED diffusion loss at these shapes (B = 8, fixed labels / eps), measured
# on the parent commit: exactly 0, twice in a row -- both paths round the same fp32 x_t and the same fp32 dpred = (pred - eps) *
# (2 / (B S C)) to bf16, so the gradient buffers agree bit for bit.  The weighted step may differ by twice that: it must be
# bit-identical too.  The generic objective is written so that autograd forms the fused kernel's products,
# fl(fl(w * fl(1 / (B S C))) * 2 d), from the weights the fused kernel reports (which tests/test_gpu_timestep.py checks per element
# against float64).
PARENT_FUSED_VS_GENERIC = 0.0


def make_model(T=1000, seed=0):
    import smd_amd.ncsn as N
    return N.create_model(N.PRNGKey(seed), SHAPE, KW, architecture="TransformerDDPM", num_timesteps=T)


def draws(B, T, seed=5):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.clamp(0.25 * torch.randn(B, *SHAPE, generator=g), -1, 1)
    labels = torch.randint(1, T + 1, (B,), generator=g).int()
    eps = torch.randn(B, *SHAPE, generator=g)
    return x0, labels, eps


def test_default_path_is_unchanged_bit_for_bit():
    """three steps with loss_weighting='min_snr', min_snr_gamma=inf (the weighted kernel with every weight exactly 1) leave the
    parameters byte-equal to three default steps, and report the same loss"""
    import smd_amd.ncsn as N
    from smd_amd.trainer import create_optimizer, train_step
    x0, labels, eps = draws(8, 1000)
    out = []
    for kw in ({}, dict(loss_weighting="min_snr", min_snr_gamma=float("inf"))):
        model = make_model()
        opt = create_optimizer(model, 1e-3, ema=True)
        ms = []
        for it in range(3):
            _, m = train_step(N.diffusion_loss, x0, opt, BETAS, N.PRNGKey(it), 1e-3, labels=labels, eps=eps, **kw)
            ms.append(m.resolve())
        torch.cuda.synchronize()
        out.append((opt.engine.params.clone(), opt.engine.ema.clone(), ms))
    (p0, e0, m0), (p1, e1, m1) = out
    assert torch.equal(p0.view(torch.int32), p1.view(torch.int32)) and torch.equal(e0.view(torch.int32), e1.view(torch.int32))
    assert set(m0[0]) == {"loss", "grad", "lr"} and set(m1[0]) == {"loss", "grad", "lr", "loss_unweighted"}
    for a, b in zip(m0, m1):
        assert a["loss"] == b["loss"] == b["loss_unweighted"] and a["grad"] == b["grad"]


def _fused_vs_generic(weighted):
    """(relative difference of the two gradient buffers, fused metrics, generic loss) for one step from the same parameters"""
    import smd_amd.ncsn as N
    from smd_amd import schedule
    from smd_amd.trainer import _train_step_generic, create_optimizer, train_step
    B, gamma = 8, 5.0
    x0, labels, eps = draws(B, 1000)
    iw = (0.5 + 1.5 * torch.rand(B, generator=torch.Generator().manual_seed(9))) if weighted else None
    model = make_model()
    opt = create_optimizer(model, 1e-3, ema=False)
    eng = opt.engine
    params0 = eng.params.clone()
    kw = dict(loss_weighting="min_snr", min_snr_gamma=gamma, loss_weights=iw) if weighted else {}
    _, m = train_step(N.diffusion_loss, x0, opt, BETAS, N.PRNGKey(0), 1e-3, grad_clip=1e9, labels=labels, eps=eps, **kw)
    m = m.resolve()
    g_fused = eng.grads.clone()
    eng.params.copy_(params0)
    eng.refresh_weights()
    alpha = torch.from_numpy(O.used_alphas_from_labels(BETAS, labels.numpy()).astype(np.float32))
    w = torch.ones(B)
    if weighted:
        w = eng.weight_per_sample().cpu().clone()                  # the fused kernel's own weights ...
        s = eng.debug_tensor("s").flatten().float().cpu().numpy()  # the noise levels q-sample stored: sqrt(used_alpha)
        np.testing.assert_allclose(s.astype(np.float64) ** 2, alpha.double().numpy(), rtol=8 * R.U)
        want = schedule.min_snr_weight(s.astype(np.float64) ** 2, gamma) * iw.double().numpy()
        np.testing.assert_allclose(w.double().numpy(), want, rtol=R.FP32_ROUNDINGS * R.U)      # ... which are the formula's

    def objective(batch, mdl, sigmas, rng, continuous_noise, reduction):
        dev = batch.device
        a = alpha.to(dev).view(B, 1, 1)
        e = eps.to(dev)
        xt = a.sqrt() * batch + (1 - a).sqrt() * e
        return (w.to(dev).view(B, 1, 1) * (mdl(xt, a.sqrt()) - e).pow(2)).mean()      # = mean_b(w_b mean_sc(d^2))

    _, mg = _train_step_generic(objective, x0.to(eng.device), opt, BETAS, N.PRNGKey(0), 1e-3, grad_clip=1e9, mu=0.999, comm=None,
                                lr_gamma=1.0, lr_interval=1, continuous_noise=True)
    g_gen = eng.grads.clone()
    rel = float((g_fused.double() - g_gen.double()).norm() / g_gen.double().norm())
    return rel, m, float(mg.resolve()["loss"])


def test_fused_weighted_step_against_the_generic_path():
    """The fused weighted step's gradient buffer against _train_step_generic with the same weighted MSE written in torch over
    eps_forward_train.  Tolerance: twice the difference of the same two paths for the UNWEIGHTED loss on the parent commit at
    these shapes, PARENT_FUSED_VS_GENERIC -- measured there as exactly 0 (see the constant and DESIGN.md section 25), so the
    weighted gradient buffers must agree bit for bit."""
    base, _, _ = _fused_vs_generic(False)
    rel, m, loss_generic = _fused_vs_generic(True)
    print(f"fused vs generic gradient: unweighted {base:.3e} (parent: {PARENT_FUSED_VS_GENERIC:.3e}), weighted {rel:.3e}; "
          f"loss {m['loss']:.6f} vs {loss_generic:.6f}, unweighted {m['loss_unweighted']:.6f}")
    assert rel <= 2 * PARENT_FUSED_VS_GENERIC
    assert abs(m["loss"] - loss_generic) <= 2e-3 * abs(loss_generic)             # 'loss' is the weighted objective that is optimised
    assert m["loss"] != m["loss_unweighted"]


def test_sampler_state_follows_the_reference_and_survives_a_state_dict():
    import smd_amd.ncsn as N
    from smd_amd import schedule
    from smd_amd.trainer import TimestepSampler, create_optimizer, train_step
    T, B, steps = 15, 64, 20
    sig = schedule.create_noise_schedule(1e-6, 0.01, T, schedule="linear")
    model = make_model(T)
    opt = create_optimizer(model, 1e-3, ema=False)
    sampler = TimestepSampler.for_schedule(sig, True, opt.engine.device)
    assert (sampler.n, sampler.label_base) == (T, 1)                            # the range of the uniform draw with continuous noise
    assert TimestepSampler.for_schedule(sig, False, opt.engine.device).label_base == 0
    g = torch.Generator().manual_seed(3)
    rh, rc = np.zeros((T, R.DEPTH), np.float32), np.zeros(T, np.int32)
    key = N.PRNGKey(17)
    for it in range(steps):
        x0 = torch.clamp(0.25 * torch.randn(B, *SHAPE, generator=g), -1, 1)
        key, sub = N.split(key)
        _, m = train_step(N.diffusion_loss, x0, opt, sig, sub, 1e-3, loss_weighting="min_snr", timestep_sampler=sampler)
        labels, iw = sampler.last_labels.cpu().numpy(), sampler.last_iw.cpu().numpy()
        loss = opt.engine.loss_per_sample().cpu().numpy()
        assert labels.min() >= 1 and labels.max() <= T
        if it == 0:
            assert (np.abs(iw - 1.0) <= 2.0 ** -23).all()                       # warm-up: p = fp32(1 / n), iw = 1 to rounding
        rh, rc = R.ring_update(rh, rc, labels, loss, 1)
        assert np.isfinite(m.resolve()["loss"])
    torch.cuda.synchronize()
    assert sampler.warmed and (rc == R.DEPTH).all()
    assert sampler.history.cpu().numpy().tobytes() == rh.tobytes() and sampler.counts.cpu().numpy().tobytes() == rc.tobytes()
    assert R.check_tables(sampler.p.cpu().numpy(), sampler.cdf.cpu().numpy(), rh, rc) == []
    assert float(sampler.p.max()) > float(sampler.p.min())
    # state_dict -> a new sampler -> load_state_dict: byte-equal draws from then on
    other = TimestepSampler.for_schedule(sig, True, opt.engine.device)
    other.load_state_dict(sampler.state_dict())
    assert other.warmed
    for step in (0, 7):
        a, b = sampler.draw(B, N.PRNGKey(99), step), other.draw(B, N.PRNGKey(99), step)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert not torch.equal(sampler.draw(B, N.PRNGKey(99), 0)[0], sampler.draw(B, N.PRNGKey(99), 1)[0])
    with pytest.raises(ValueError, match="shape"):
        TimestepSampler(T + 1, 1, opt.engine.device).load_state_dict(sampler.state_dict())


def test_refusals():
    import smd_amd.ncsn as N
    from smd_amd.trainer import TimestepSampler, create_optimizer, train_step, validate_training_options
    x0, labels, eps = draws(4, 1000)
    model = make_model()
    opt = create_optimizer(model, 1e-3, ema=False)

    def custom(batch, mdl, sigmas, rng, continuous_noise, reduction):
        return mdl(batch, torch.ones(4, 1, 1, device=batch.device)).pow(2).mean()

    for objective in (custom, N.denoising_score_matching_loss):
        with pytest.raises(ValueError, match="diffusion_loss"):
            train_step(objective, x0, opt, BETAS, N.PRNGKey(0), 1e-3, loss_weighting="min_snr")
        with pytest.raises(ValueError, match="diffusion_loss"):
            train_step(objective, x0, opt, BETAS, N.PRNGKey(0), 1e-3,
                       timestep_sampler=TimestepSampler.for_schedule(BETAS, True, opt.engine.device))
    with pytest.raises(ValueError, match="loss_weighting"):
        train_step(N.diffusion_loss, x0, opt, BETAS, N.PRNGKey(0), 1e-3, loss_weighting="snr")
    # the engine refuses weights on the score-matching loss itself, too
    with pytest.raises(ValueError, match="DDPM objective only"):
        opt.engine.loss_backward(x0.to(opt.engine.device), None, eps.to(opt.engine.device), objective="dsm", min_snr_gamma=5.0,
                                 used_alphas=torch.ones(4, device=opt.engine.device))
    # --dtype=fp32 stays an inference precision, as today
    fp32 = N.create_model(N.PRNGKey(0), SHAPE, KW, architecture="TransformerDDPM", num_timesteps=1000, dtype="fp32")
    with pytest.raises(ValueError, match="inference precision"):
        create_optimizer(fp32, 1e-3)
    # more than one rank with the resampler: refused by the flag validation, without starting ranks
    with pytest.raises(ValueError, match="single-process only"):
        validate_training_options("ddpm", "min_snr", "loss_second_moment", 2)
    validate_training_options("ddpm", "min_snr", "uniform", 2)
    # and evaluation stays unit-weight after weighted steps on the same handle
    train_step(N.diffusion_loss, x0, opt, BETAS, N.PRNGKey(0), 1e-3, labels=labels, eps=eps, loss_weighting="min_snr")
    got = N.diffusion_loss(x0, model, BETAS, N.PRNGKey(0), True, "none", labels=labels, eps=eps)
    model2 = make_model()
    model2.engine.params.copy_(model.engine.params)
    model2.engine.refresh_weights()
    want = N.diffusion_loss(x0, model2, BETAS, N.PRNGKey(0), True, "none", labels=labels, eps=eps)
    assert torch.equal(got, want)
