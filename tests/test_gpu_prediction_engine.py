"""x0- / v-parameterised training through the engine on the smallest networks the suite trains: a
TransformerDDPM of 2 encoder layers (C = 42, B = 8) and a DenseDDPM (C = 42).

(a) With ``prediction`` left at its default -- or set to eps explicitly, or set to v and back -- loss, gradient buffer and
    parameters after one step are bitwise those of a handle that never heard of the option.
(b) For x0 and v, the gradient of the fused step (loss_backward on explicit labels / eps) against the arbitrary-objective route
    (smd_engine_forward_train + smd_engine_backward_from) fed dpred computed on the host from the float64 reference
    tests/_prediction_ref.py.  Both routes feed the network the SAME bf16 x_t: the second route reads the fused step's own
    (smd_engine_debug_tensor "x_bf16", checked against the float64 x_t), so the comparison isolates dpred and the backward pass.
    When the second route formed x_t itself in float64, one element of x_t rounding to the other bf16 neighbour moved the whole
    forward pass and the routes differed by up to 1.8e-3 for every kind alike (seed 9 below); with the same x_t that seed gives
    exactly 0 for all three kinds.
    The bound is twice the LARGEST difference the same two routes show for EPS, whose fused path is the parent commit's code
    unchanged ((a) asserts the bits): EPS_ROUTE_DIFFERENCE below, measured on the draws of seeds 5 .. 12, unweighted and with
    min-SNR weights (16 runs per kind and architecture).  DenseDDPM: 0 in all 48 runs.  TransformerDDPM:
    eps 0 in 14 runs, 1.562e-4 and 2.618e-4 on seed 10; x0 0 in all 16; v 0 in 12, 5.3e-10, 3.4e-9 and (seed 10, unweighted)
    1.978e-4.  What remains is dpred: fp32 kernel arithmetic against float64 rounded once, so single bf16 elements of dpred
    differ; why seed 10's are worth 2e-4 of the gradient was not established.  The bound is asserted on seeds 5, 9 and 10, both
    weightings.
"""
import numpy as np
import pytest
import torch

import _prediction_ref as R
import ddpm_oracle as O

pytestmark = pytest.mark.gpu

BETAS = O.create_noise_schedule(1e-6, 0.01, 1000, "linear")
KW = dict(num_layers=2, num_heads=8, num_mlp_layers=1, mlp_dims=256)
ARCH = {"TransformerDDPM": (32, 42), "DenseDDPM": (42,)}
B, GAMMA = 8, 5.0

# ||g_fused - g_routes|| / ||g_routes|| for eps at these shapes (B = 8, fixed labels / eps, the same bf16 x_t in both routes): the
# largest value the eps routes showed over seeds 5 .. 12, unweighted and min-SNR weighted, per architecture; the x0 / v routes
# may differ by twice that.
EPS_ROUTE_DIFFERENCE = {"TransformerDDPM": 2.618e-4, "DenseDDPM": 0.0}
ROUTE_SEEDS = (5, 9, 10)


def make_model(arch, seed=0):
    import smd_amd.ncsn as N
    return N.create_model(N.PRNGKey(seed), ARCH[arch], KW, architecture=arch, num_timesteps=1000)


def draws(arch, seed=5):
    g = torch.Generator().manual_seed(seed)
    shape = ARCH[arch]
    x0 = torch.clamp(0.25 * torch.randn(B, *shape, generator=g), -1, 1)
    labels = torch.randint(1, 1001, (B,), generator=g).int()
    labels[0], labels[1] = 1, 1000                                    # ap = 1 exactly, and the last timestep
    eps = torch.randn(B, *shape, generator=g)
    return x0, labels, eps


@pytest.mark.parametrize("arch", list(ARCH))
def test_default_step_is_unchanged_bit_for_bit(arch):
    import smd_amd.ncsn as N
    from smd_amd.trainer import create_optimizer, train_step
    x0, labels, eps = draws(arch)
    out = []
    for how in ("never", "default kw", "eps", "v and back"):
        model = make_model(arch)
        opt = create_optimizer(model, 1e-3, ema=True)
        eng = opt.engine
        kw = {}
        if how == "eps":
            eng.set_prediction("eps")
            kw = dict(prediction="eps")
        elif how == "v and back":
            train_step(N.diffusion_loss, x0, opt, BETAS, N.PRNGKey(0), 0.0, labels=labels, eps=eps, prediction="v", mu=1.0)
            assert eng.prediction == "v"
            model = make_model(arch)                                  # fresh parameters and optimiser state, then back to eps on
            opt = create_optimizer(model, 1e-3, ema=True)             # a handle that has been through the option
            eng = opt.engine
            eng.set_prediction("v")
            eng.set_prediction("eps")
        _, m = train_step(N.diffusion_loss, x0, opt, BETAS, N.PRNGKey(0), 1e-3, labels=labels, eps=eps, **kw)
        torch.cuda.synchronize()
        assert eng.prediction == "eps"
        out.append((m.resolve(), eng.loss_per_sample().clone(), eng.grads.clone(), eng.params.clone(), eng.ema.clone()))
    m0, l0, g0, p0, e0 = out[0]
    assert set(m0) == {"loss", "grad", "lr"}
    for m, l, g, p, e in out[1:]:
        assert m == m0
        for a, b in ((l, l0), (g, g0), (p, p0), (e, e0)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _routes(arch, kind, seed=5, gamma=GAMMA):
    """(relative difference of the two gradient buffers, fused metrics) for one step of ``kind`` (min-SNR weights unless gamma is
    0) on the draws of ``seed``"""
    import smd_amd.ncsn as N
    from smd_amd.trainer import create_optimizer, train_step
    name = ("eps", "x0", "v")[kind]
    x0, labels, eps = draws(arch, seed)
    model = make_model(arch)
    opt = create_optimizer(model, 1e-3, ema=False)
    eng = opt.engine
    params0 = eng.params.clone()
    wkw = dict(loss_weighting="min_snr", min_snr_gamma=gamma) if gamma else {}
    _, m = train_step(N.diffusion_loss, x0, opt, BETAS, N.PRNGKey(0), 1e-3, grad_clip=1e9, labels=labels, eps=eps,
                      prediction=name, **wkw)
    m = m.resolve()
    g_fused = eng.grads.clone()
    s = eng.noise_level_per_sample().cpu().numpy().copy()
    x_bf16 = eng.debug_tensor("x_bf16")[:, :ARCH[arch][-1]].float().reshape(B, *ARCH[arch]).clone()    # the x_t the fused step fed its network
    w_fused = eng.weight_per_sample().cpu().numpy().astype(np.float64) if (gamma or kind) else np.ones(B)
    loss_fused = eng.loss_per_sample().cpu().numpy().astype(np.float64)
    eng.params.copy_(params0)
    eng.refresh_weights()
    # the other route: the engine's forward in its training workspace on the SAME bf16 x_t (checked against float64 below),
    # dpred from the float64 reference on the prediction it returns, the engine's backward from it
    s64, sb64 = R.levels(s)
    shp = (B,) + (1,) * (x0.dim() - 1)
    alpha = O.used_alphas_from_labels(BETAS, labels.numpy()).astype(np.float64).reshape(shp)     # q-sample's own sb is sqrt(1 - alpha)
    t1, t2 = np.sqrt(alpha) * x0.double().numpy(), np.sqrt(1.0 - alpha) * eps.double().numpy()
    # it is the float64 x_t up to q-sample's fp32 roundings of the two terms and one bf16 rounding of the sum
    assert (np.abs(x_bf16.cpu().double().numpy() - (t1 + t2)) <= 2.0 ** -8 * np.abs(t1 + t2) + 2.0 ** -22 * (np.abs(t1) + np.abs(t2))).all()
    pred = eng.forward_train(x_bf16, torch.from_numpy(s))
    inv = np.float32(1.0 / (B * int(np.prod(ARCH[arch]))))
    g64, loss64, w64 = R.param_grad(kind, pred.cpu().numpy(), eps.numpy(), x0.numpy(), s, None, gamma, inv)
    eng.backward_from(torch.from_numpy(g64.astype(np.float32)))
    torch.cuda.synchronize()
    g_ref = eng.grads.clone()
    rel = float((g_fused.double() - g_ref.double()).norm() / g_ref.double().norm())
    assert np.isfinite(w_fused).all() and np.allclose(w_fused, w64, rtol=16 * R.U, atol=0)
    np.testing.assert_allclose(loss_fused, loss64, rtol=1e-5)          # the same forward pass twice: the kernel test's bound
    if kind:
        assert w_fused[0] == ((GAMMA if kind == 1 else 0.0) if gamma else 1.0)          # label 1: ap = 1
        assert m["loss_eps"] == pytest.approx(R.loss_in_eps_units(kind, loss_fused, s), rel=1e-5)
        assert m["loss"] == pytest.approx(float((w_fused * loss_fused).mean()), rel=1e-5)
    return rel, m


@pytest.mark.parametrize("arch", list(ARCH))
def test_fused_step_against_the_arbitrary_objective_route(arch):
    for seed in ROUTE_SEEDS:
        for gamma in (0.0, GAMMA):
            for kind in (1, 2):
                rel, m = _routes(arch, kind, seed, gamma)
                print(f"{arch} kind {kind} seed {seed} gamma {gamma}: fused vs forward_train + backward_from gradient {rel:.3e} (eps "
                      f"recorded {EPS_ROUTE_DIFFERENCE[arch]:.3e}); loss {m['loss']:.5f} unweighted {m['loss_unweighted']:.5f} "
                      f"eps units {m['loss_eps']:.5f}")
                assert set(m) == {"loss", "grad", "lr", "loss_unweighted", "loss_eps"} and all(np.isfinite(v) for v in m.values())
                assert rel <= 2 * EPS_ROUTE_DIFFERENCE[arch], (seed, gamma, kind, rel)


def test_engine_refusals_and_eval_loss():
    import smd_amd.ncsn as N
    from smd_amd.trainer import create_optimizer
    arch = "TransformerDDPM"
    x0, labels, eps = draws(arch)
    model = make_model(arch)
    opt = create_optimizer(model, 1e-3, ema=False)
    eng = opt.engine
    with pytest.raises(ValueError, match="prediction"):
        eng.set_option("prediction", 3)
    with pytest.raises(ValueError, match="prediction=3"):            # the library's own check, under the Python handle
        import smd_amd.lib as lib
        lib.check(eng.L.smd_engine_set_option(eng.h, b"prediction", 3), "set_option")
    with pytest.raises(ValueError, match="prediction"):
        eng.set_prediction("score")
    eng.set_option("prediction", 2)                                   # the option goes through set_prediction: the handle's tables,
    assert eng.prediction == "v"                                      # cache keys and this attribute follow it
    eng.set_prediction("v")
    assert eng.prediction == "v"
    with pytest.raises(ValueError, match="loss_kind"):
        eng.set_option("loss_kind", 1)                                # score matching with v: an argument error, either order
    eng.set_option("prediction", 0)
    eng.set_option("loss_kind", 1)
    with pytest.raises(ValueError, match="score matching"):
        eng.set_option("prediction", 1)
    eng.set_option("loss_kind", 0)
    with pytest.raises(ValueError, match="objective='ddpm'"):
        eng.loss_backward(x0.to(eng.device), None, eps.to(eng.device), objective="dsm", prediction="v",
                          used_alphas=torch.ones(B, device=eng.device))
    # stage 3 (loss only): the output-space loss of the kind, against the float64 reference on the engine's own prediction
    for kind, name in ((1, "x0"), (2, "v")):
        got = N.diffusion_loss(x0, model, BETAS, N.PRNGKey(0), True, "none", labels=labels, eps=eps, prediction=name)
        s = eng.noise_level_per_sample().cpu().numpy()
        pred = eng.last_pred().cpu().numpy()
        _, loss64, _ = R.param_grad(kind, pred, eps.numpy(), x0.numpy(), s, None, 0.0, np.float32(1.0))
        np.testing.assert_allclose(got.cpu().numpy(), loss64, rtol=1e-5)
    back = N.diffusion_loss(x0, model, BETAS, N.PRNGKey(0), True, "none", labels=labels, eps=eps)
    assert eng.prediction == "eps"
    pred = eng.last_pred().cpu().numpy()
    np.testing.assert_allclose(back.cpu().numpy(), ((pred - eps.numpy()).astype(np.float64) ** 2).reshape(B, -1).mean(1), rtol=1e-5)


# ---------------------------------------------------------------------------------------------------- (c) the float64 oracle
def _oracle_loss(kind, x0, model, labels, eps):
    """oracle/ddpm_oracle.py diffusion_loss (utils/losses.py:250-308) with the target of ``kind`` in place of eps: float64
    autograd through the oracle network; per-sample losses"""
    Bn = x0.shape[0]
    a = torch.from_numpy(O.used_alphas_from_labels(BETAS, labels.numpy())).to(x0.dtype).reshape(Bn, *([1] * (x0.dim() - 1)))
    sa, sb = torch.sqrt(a), torch.sqrt(1 - a)
    out = model(sa * x0 + sb * eps, sa)
    target = x0 if kind == 1 else sa * eps - sb * x0
    d = (target - out) ** 2
    return d.mean(dim=tuple(range(1, d.dim())))


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "min_snr"])
@pytest.mark.parametrize("name", ["x0", "v"])
@pytest.mark.parametrize("arch,L,K,Bn", [("TransformerDDPM", 2, 1, 8), ("DenseDDPM", 2, 2, 64)])
def test_loss_and_gradient_against_the_float64_oracle(arch, L, K, Bn, name, weighted):
    """(c) The engine's loss and parameter gradient under the kind's loss against float64 autograd through the oracle network
    (imported read-only from oracle/), on identical weights, labels and eps.  Bounds: those of
    tests/test_gpu_engine.py::test_loss_and_gradient_parity, the eps parity test at this size -- mean loss 5e-3 relative,
    whole-vector gradient rel-L2 1e-2, worst tensor 6e-2.  min_snr: the oracle's objective is mean_b(w_b loss_b) with
    schedule.min_snr_weight of the kind on the float32 used alphas."""
    import smd_amd.schedule as S
    from test_gpu_engine import data, make, rel
    kind = S.prediction_kind(name)
    ocfg, p, model = make(arch, 42, L, 8, K, M=256)
    shape = ARCH[arch]
    x0, g = data(Bn, shape)
    labels = torch.randint(1, 1001, (Bn,), generator=g)
    labels[0], labels[1] = 1, 1000                                    # ap = 1 exactly (w_x0 = gamma, w_v = 0), and t = T - 1
    eps = torch.randn(Bn, *shape, generator=g)
    leaf = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    loss_ref = _oracle_loss(kind, x0.double(), O.make_model(leaf, ocfg), labels, eps.double())
    alpha = O.used_alphas_from_labels(BETAS, labels.numpy()).astype(np.float64)
    w = torch.from_numpy(S.min_snr_weight(alpha, GAMMA, name)) if weighted else torch.ones(Bn, dtype=torch.float64)
    (w * loss_ref).mean().backward()

    eng = model.train_engine(ema=True)
    eng.set_prediction(name)
    eng.set_schedule(BETAS, with_sampler=False)
    eng.bind(Bn, training=True)
    eng.loss_backward(x0.cuda(), labels.int().cuda(), eps.cuda(), stage=0, min_snr_gamma=GAMMA if weighted else 0.0)
    torch.cuda.synchronize()
    got, want = float(eng.loss_per_sample().mean()), float(loss_ref.mean())
    wg = eng.weight_per_sample().double().cpu()
    # the kernel's weight is evaluated on the stored fp32 s, the oracle's on alpha: at labels 2, 3, ... 1 - s^2 carries s's rounding
    print(f"{arch} {name} {'min_snr' if weighted else 'unweighted'}: loss {got:.6f} vs {want:.6f}; weights rel {rel(wg, w):.2e}")
    assert abs(got - want) / want < 5e-3
    gv = eng.named_views(eng.grads)
    worst, num, den = 0.0, 0.0, 0.0
    for k, v in leaf.items():
        r = rel(gv[k], v.grad)
        worst = max(worst, r)
        num += float((gv[k].double().cpu() - v.grad).pow(2).sum())
        den += float(v.grad.pow(2).sum())
    total = (num / den) ** 0.5
    print(f"gradient {arch} {name}: whole-vector rel-L2 {total:.3e}, worst tensor {worst:.3e}")
    assert total < 1e-2
    assert worst < 6e-2
