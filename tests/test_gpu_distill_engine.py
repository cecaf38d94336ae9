"""trainer.distill_step on the smallest networks the suite trains: a TransformerDDPM of 2 encoder layers
and a DenseDDPM, C = 42, B = 8, T = 16 (the sizes of tests/test_gpu_prediction_engine.py), teacher walk of 8 timesteps, student
of N = 4 steps.

(a) The step's gradient buffer against a second route on the same z_t and the same teacher outputs: the engine-free kernels
    (bitwise repeatable) up to the teacher's second output, the student's forward_train, d loss / d pred computed on the host
    in float64 by tests/_distill_ref.py and rounded once to fp32, backward_from.  Bound on ||g_step - g_route|| / ||g_route||:
    twice 2.618e-4, the bound DESIGN.md section 26 derived for the same comparison of the fused x0 / v step -- inherited, not
    re-measured here.
(b) The teacher's parameter buffer is bitwise unchanged after 3 steps; two runs from one seed give bitwise equal students.
(c) 100 steps of a DenseDDPM student at B = 64 lower its unweighted distillation loss on a fixed evaluation set (strictly).
"""
import numpy as np
import pytest
import torch

import _distill_ref as R

pytestmark = pytest.mark.gpu

T, N, B = 16, 4, 8
BETAS = np.linspace(1e-3, 0.2, T).astype(np.float32)
KW = dict(num_layers=2, num_heads=8, num_mlp_layers=1, mlp_dims=256)
ARCH = {"TransformerDDPM": (32, 42), "DenseDDPM": (42,)}
ROUTE_BOUND = 2 * 2.618e-4
STEPS = [0, 3, 1, 1, 2, 0, 3, 2]


def make_model(arch, seed):
    import smd_amd.ncsn as Nn
    return Nn.create_model(Nn.PRNGKey(seed), ARCH[arch], KW, architecture=arch, num_timesteps=T)


def make_pair(arch, teacher_kind, student_kind, weighting="truncated_snr", ema=False):
    """(teacher, student, optimizer, tables): the student starts from the teacher's parameters, in a buffer of its own"""
    import smd_amd.schedule as S
    from smd_amd.trainer import DistillTables, create_optimizer
    teacher, student = make_model(arch, 1), make_model(arch, 2)
    student.engine.params.copy_(teacher.engine.params)
    student.engine.refresh_weights()
    opt = create_optimizer(student, 1e-3, ema=ema)
    tw, _ = S.distill_walk(T, N)
    return teacher, student, opt, DistillTables(BETAS, tw, teacher_kind, student_kind, weighting, device=student.engine.device)


def draws(arch, seed=5, batch=B):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.clamp(0.25 * torch.randn(batch, *ARCH[arch], generator=g), -1, 1)
    eps = torch.randn(batch, *ARCH[arch], generator=g)
    return x0, eps


@pytest.mark.parametrize("student_kind", ["x0", "v"])
@pytest.mark.parametrize("teacher_kind", ["eps", "v"])
@pytest.mark.parametrize("arch", list(ARCH))
def test_step_gradient_against_the_float64_dpred_route(arch, teacher_kind, student_kind):
    import smd_amd.engine as E
    import smd_amd.ncsn as Nn
    import smd_amd.schedule as S
    from smd_amd.trainer import distill_step
    teacher, student, opt, tab = make_pair(arch, teacher_kind, student_kind)
    eng = opt.engine
    dev = eng.device
    x0, eps = draws(arch)
    params0 = eng.params.clone()
    steps = torch.tensor(STEPS, dtype=torch.int32)
    _, m = distill_step(x0, opt, teacher, tab, Nn.PRNGKey(0), 1e-3, steps=steps, eps=eps, grad_clip=1e9)
    m = m.resolve()
    g_step = eng.grads.clone()
    assert set(m) == {"loss", "loss_unweighted", "grad", "lr"} and all(np.isfinite(v) for v in m.values())
    eng.params.copy_(params0)
    eng.refresh_weights()
    # the second route
    k = steps.to(dev)
    z_t, lt, _ = E.distill_noise(x0.to(dev), tab.table, k, eps.to(dev))
    out1 = teacher.engine.forward(z_t, lt)
    x1, z_m, lm = E.distill_mid(z_t, out1, tab.table, k)
    out2 = teacher.engine.forward(z_m, lm)
    pred = eng.forward_train(z_t, lt)
    inv = np.float32(1.0 / (B * int(np.prod(ARCH[arch]))))
    n = lambda t: t.cpu().numpy()
    kind = S.prediction_kind(student_kind)
    ref = R.loss(n(x1), n(z_m), n(out2), n(z_t), n(pred), kind, tab.host, np.asarray(STEPS), None, inv)
    eng.backward_from(torch.from_numpy(ref["dpred"].astype(np.float32)))
    torch.cuda.synchronize()
    g_ref = eng.grads.clone()
    rel = float((g_step.double() - g_ref.double()).norm() / g_ref.double().norm())
    print(f"{arch} teacher {teacher_kind} student {student_kind}: distill_step vs forward_train + float64 dpred + backward_from "
          f"gradient {rel:.3e} (bound {ROUTE_BOUND:.3e}); loss {m['loss']:.5f} unweighted {m['loss_unweighted']:.5f}")
    assert float(g_ref.double().norm()) > 0
    assert m["loss_unweighted"] == pytest.approx(float(ref["loss"].mean()), rel=1e-4)
    assert m["loss"] == pytest.approx(float((ref["weight"] * ref["loss"]).mean()), rel=1e-4)
    assert rel <= ROUTE_BOUND, rel


def _three_steps(arch, seed):
    import smd_amd.ncsn as Nn
    from smd_amd.trainer import distill_step
    teacher, student, opt, tab = make_pair(arch, "v", "v", ema=True)
    t0 = teacher.engine.params.clone()
    rng = Nn.PRNGKey(seed)
    for i in range(3):
        x0, _ = draws(arch, 40 + i)
        distill_step(x0, opt, teacher, tab, rng, 1e-3, lr_gamma=0.98, lr_interval=10000)
    torch.cuda.synchronize()
    assert torch.equal(teacher.engine.params.view(torch.int32), t0.view(torch.int32)), "the teacher is read only"
    assert not torch.equal(opt.engine.params, t0), "the student moved"
    assert opt.step == 3
    return opt.engine.params.clone(), opt.engine.ema.clone()


@pytest.mark.parametrize("arch", list(ARCH))
def test_teacher_is_frozen_and_the_step_is_reproducible(arch):
    p1, e1 = _three_steps(arch, 11)
    p2, e2 = _three_steps(arch, 11)
    p3, _ = _three_steps(arch, 12)
    assert torch.equal(p1.view(torch.int32), p2.view(torch.int32)) and torch.equal(e1.view(torch.int32), e2.view(torch.int32))
    assert not torch.equal(p1, p3), "another seed draws other steps and noise"


def test_refusals():
    import smd_amd.ncsn as Nn
    from smd_amd.trainer import distill_step
    teacher, student, opt, tab = make_pair("DenseDDPM", "v", "v")
    x0, _ = draws("DenseDDPM")
    with pytest.raises(ValueError, match="the tables carry the loss weights of a 'v' student"):
        distill_step(x0, opt, teacher, tab, Nn.PRNGKey(0), 1e-3, prediction="x0")
    with pytest.raises(ValueError, match="shares the student's parameter buffer"):
        distill_step(x0, opt, student, tab, Nn.PRNGKey(0), 1e-3)


def test_sampler_walks_an_explicit_walk():
    """strided_dynamics(timesteps=walk): the student's 4 timesteps, read back from ld_metrics' alpha row; the evenly spaced walk
    given explicitly has the bits of steps=K; a bad walk and a contradicting step count are refused"""
    import smd_amd.ncsn as Nn
    import smd_amd.schedule as S
    model = make_model("DenseDDPM", 1)
    ap = S.alphas_cumprod(BETAS)
    _, sw = S.distill_walk(T, N)
    init = torch.randn(6, 42, generator=torch.Generator().manual_seed(1))
    for order in (1, 2):
        x, _, ld = Nn.strided_dynamics(Nn.PRNGKey(0), model, BETAS, init, None, timesteps=sw, order=order, prediction="v")
        assert torch.isfinite(x).all() and ld.shape == (4, N, 1)
        assert ld[2, :, 0].cpu().numpy().tolist() == ap[sw].tolist()
    a, _, lda = Nn.strided_dynamics(Nn.PRNGKey(0), model, BETAS, init, 4, prediction="v")
    b, _, ldb = Nn.strided_dynamics(Nn.PRNGKey(0), model, BETAS, init, 4, timesteps=S.stride_timesteps(T, 4), prediction="v")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(lda, ldb)
    assert ldb[2, :, 0].cpu().numpy().tolist() != ap[sw].tolist()                  # another walk of the same length, another key
    c, _, ldc = Nn.strided_dynamics(Nn.PRNGKey(0), model, BETAS, init, None, timesteps=sw, prediction="v")
    assert ldc[2, :, 0].cpu().numpy().tolist() == ap[sw].tolist() and not torch.equal(c, b)
    with pytest.raises(ValueError, match="strictly descending"):
        Nn.strided_dynamics(Nn.PRNGKey(0), model, BETAS, init, None, timesteps=[3, 7])
    with pytest.raises(ValueError, match="contradicts the explicit walk"):
        Nn.strided_dynamics(Nn.PRNGKey(0), model, BETAS, init, 3, timesteps=sw)


def test_training_lowers_the_distillation_loss():
    import smd_amd.engine as E
    import smd_amd.ncsn as Nn
    from smd_amd.trainer import distill_step
    arch, Bt = "DenseDDPM", 64
    teacher, student, opt, tab = make_pair(arch, "v", "v")
    dev = opt.engine.device
    g = torch.Generator().manual_seed(77)
    ev_x, ev_eps = draws(arch, 900, 256)
    ev_k = torch.randint(0, N, (256,), generator=g).int().to(dev)

    def eval_loss():
        z_t, lt, _ = E.distill_noise(ev_x.to(dev), tab.table, ev_k, ev_eps.to(dev))
        x1, z_m, lm = E.distill_mid(z_t, teacher.engine.forward(z_t, lt), tab.table, ev_k)
        out2 = teacher.engine.forward(z_m, lm)
        pred = student.engine.forward(z_t, lt)
        per, _, _, _ = E.distill_loss(x1, z_m, out2, z_t, pred, tab.table, ev_k, "v", 1.0 / ev_x.numel())
        return float(per.double().mean())

    before = eval_loss()
    rng = Nn.PRNGKey(3)
    for i in range(100):
        x0, _ = draws(arch, 1000 + i % 8, Bt)
        distill_step(x0, opt, teacher, tab, rng, 1e-3)
    after = eval_loss()
    print(f"unweighted distillation loss on the fixed set: {before:.6f} before, {after:.6f} after 100 steps")
    assert np.isfinite(before) and np.isfinite(after) and after < before
