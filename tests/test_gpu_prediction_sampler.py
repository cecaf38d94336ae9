"""The sampler kernels fed the output of an x0- / v-predicting network with that kind's tables: no sampler
kernel changed, so what is under test is that the first two table columns alone carry the parameterisation on the GPU.

For each of smd_ddpm_reverse_step, one strided iteration (smd_engine_strided_step) and one multistep iteration
(smd_engine_multistep_step) the output `out` is turned into the EQUIVALENT eps_hat in float64 with the exact coefficients of the
kind (tests/_prediction_ref.py eps_of: written independently of the tables), and the update is recomputed in float64 in its
eps form -- x0 = clamp(x / sqrt(ap) - sqrt(1/ap - 1) eps_hat) with exact float64 coefficients, the remaining columns as the
float32 table holds them.  A wrong sign of c1, swapped columns or a clamp that misbehaves at c0 = 0 all show per element.
Timesteps include t = T - 1 and t = 0.

Bounds per element, those of tests/test_gpu_strided.py / tests/test_gpu_multistep.py for the update alone,
    |err| <= 4 * 2^-23 * (|g x0| + |b x| + |sigma z| + |a1 x0_prev|) + 1e-12        (g = a, a0 or mu1; b = b or mu2)
plus the one thing those tests do not meet, because they recompute from the float32 columns the kernel read: here the reference
uses EXACT c0, c1, and the table's are rounded once to float32, so x0 may differ by 2^-24 (|c0 x| + |c1 out|) before the gain g:
    + |g| * 2^-24 * (|c0 x| + |c1 out|)          (zero for the x0 kind: its 0 and -1 are exact)
"""
import numpy as np
import pytest
import torch

import _multistep_ref as MR
import _prediction_ref as R
import _strided_ref as SR
from test_gpu_full_walk import BETAS
from test_gpu_multistep import logsnr_taus, plan_struct
from test_gpu_strided import dense_model, transformer_model

pytestmark = pytest.mark.gpu
T, K = 1000, 20
AP = SR.alphas_prod(BETAS)
KINDS = {"x0": 1, "v": 2}
d = lambda v: v.double().cpu()


def exact_eps_row(t):
    """(sqrt(1/ap), sqrt(1/ap - 1)) in float64, the latter without the cancellation of 1/ap - 1 near ap = 1"""
    return 1.0 / np.sqrt(AP[t]), np.sqrt(1.0 - AP[t]) / np.sqrt(AP[t])


def table_slack(kind, gain, t, x, out):
    c0, c1 = R.x0_coefficients(kind, AP[t])
    return abs(gain) * 2.0 ** -24 * ((float(c0) * x).abs() + (float(c1) * out).abs()) if kind == 2 else 0.0


@pytest.mark.parametrize("name", list(KINDS))
@pytest.mark.parametrize("C", [512, 42])
def test_reverse_step_on_the_kinds_output(dev, C, name):
    import smd_amd.lib as lib
    import smd_amd.schedule as S
    kind = KINDS[name]
    L = lib.get_lib()
    B, Sq = 3, 32
    coef = S.reverse_coefficient_table(BETAS, name)
    coefd = torch.from_numpy(coef).to(dev)
    slotd = torch.from_numpy(S.collection_slot_table(T)).to(dev)
    g = torch.Generator().manual_seed(C + kind)
    worst = 0.0
    for t in (T - 1, 975, 1, 0):
        x = torch.randn(B, Sq, C, generator=g)
        eh = torch.randn(B, Sq, C, generator=g)               # the network's belief about the noise ...
        z = torch.randn(B, Sq, C, generator=g)
        out = torch.from_numpy(R.output_of(kind, x.double().numpy(), eh.double().numpy(), AP[t]).astype(np.float32))   # ... as this kind emits it
        eq = torch.from_numpy(R.eps_of(kind, x.double().numpy(), out.double().numpy(), AP[t]))      # what the ROUNDED output is equivalent to
        c0, c1 = exact_eps_row(t)
        mu1, mu2, sigma = (float(coef[t, k]) for k in (2, 3, 4))
        x0 = torch.clamp(c0 * d(x) - c1 * eq, -1.0, 1.0)
        if t == 0:
            sigma = 0.0                                       # the last step adds no noise (utils/ebm_utils.py: noise only where t > 0)
        ref = mu1 * x0 + mu2 * d(x) + sigma * d(z)
        xd, tp = x.clone().to(dev), torch.tensor([t], dtype=torch.int32, device=dev)
        mp = torch.zeros(T, B, 3, device=dev)
        cl = torch.zeros(41, B, Sq, C, device=dev)
        outd, zd = out.to(dev), z.to(dev)
        lib.check(L.smd_ddpm_reverse_step(xd.data_ptr(), outd.data_ptr(), B, Sq, C, coefd.data_ptr(), T, tp.data_ptr(), zd.data_ptr(), 0, 0, 0,
                                          mp.data_ptr(), cl.data_ptr(), slotd.data_ptr(), torch.cuda.current_stream().cuda_stream), "reverse_step")
        torch.cuda.synchronize()
        mag = (mu1 * x0).abs() + (mu2 * d(x)).abs() + (sigma * d(z)).abs()
        bound = 4 * 2.0 ** -23 * mag + table_slack(kind, mu1, t, d(x), d(out)) + 1e-12
        ratio = float(((d(xd) - ref).abs() / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (name, t, ratio)
        assert float((x0.abs() == 1.0).double().mean()) < 1.0 and float((d(xd) - d(x)).abs().max()) > 0
    print(f"[reverse {name} C={C}] worst |err| / bound = {worst:.3f}")


def _engine(arch, C, B, name):
    model = transformer_model(C) if arch == "transformer" else dense_model(C)
    eng = model.engine
    eng.set_prediction(name)
    eng.set_schedule(BETAS, with_sampler=True)
    eng.bind(B, training=False)
    eng.prepare_sampler()
    return model, eng


@pytest.mark.parametrize("name", list(KINDS))
@pytest.mark.parametrize("arch,B,C", [("transformer", 3, 42), ("dense", 5, 512)])
def test_strided_iteration_on_the_kinds_output(arch, B, C, name):
    import smd_amd.lib as lib
    import smd_amd.schedule as S
    kind = KINDS[name]
    model, eng = _engine(arch, C, B, name)
    Sq, dev = eng.S, eng.device
    shape = (B, Sq, C) if Sq > 1 else (B, C)
    taus = S.stride_timesteps(T, K)
    g = torch.Generator().manual_seed(21 + kind)
    worst = 0.0
    for eta in (0.0, 0.7):
        for clip in (1.0, float("inf")):
            coef, plan = S.strided_coefficient_table(BETAS, taus, eta, clip, prediction=name)
            coef_d, plan_d = torch.from_numpy(coef).to(dev), torch.from_numpy(plan).to(dev)
            sp = lib.StridePlan()
            sp.coef, sp.plan, sp.T = coef_d.data_ptr(), plan_d.data_ptr(), T
            for j in (0, K // 2, K - 1):                               # t = T - 1, the middle, t = 0
                t = int(taus[j])
                x = (torch.randn(*shape, generator=g) * (1.0 if j < K - 1 else 0.5)).to(dev)
                z = torch.randn(*shape, generator=g).to(dev)
                x_in = x.clone()
                t_ptr = torch.tensor([t], dtype=torch.int32, device=dev)
                mp = torch.zeros((T, B, 3), device=dev)
                coll = torch.full((41, *shape), 7.0, device=dev)
                io = lib.SampleIO()
                io.x, io.t_ptr, io.z_in = x.data_ptr(), t_ptr.data_ptr(), z.data_ptr()
                io.metrics_partial, io.collection = mp.data_ptr(), coll.data_ptr()
                eng.load_state(x)
                eng.strided_step(io, sp)
                torch.cuda.synchronize()
                out = eng.last_pred().clone()
                eq = torch.from_numpy(R.eps_of(kind, d(x_in).numpy(), d(out).numpy(), AP[t]))
                row = dict(zip(("sqrt_recip", "sqrt_m1", "a", "b", "sigma", "clip", "sqrt_as", "sqrt_1m_as"), (float(v) for v in coef[t])))
                row["sqrt_recip"], row["sqrt_m1"] = exact_eps_row(t)
                row.update(t=t, next_t=int(plan[t, 0]))
                ref, x0, _ = SR.update(d(x_in), eq, d(z), row, T)
                mag = (row["a"] * x0).abs() + (row["b"] * d(x_in)).abs() + (row["sigma"] * d(z)).abs()
                bound = 4 * 2.0 ** -23 * mag + table_slack(kind, row["a"], t, d(x_in), d(out)) + 1e-12
                ratio = float(((d(x) - ref).abs() / bound).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (name, eta, clip, t, ratio)
                assert int(t_ptr.item()) == int(plan[t, 0])
    print(f"[strided {name} {arch} B={B} C={C}] worst |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("name", list(KINDS))
@pytest.mark.parametrize("arch,B,C", [("transformer", 3, 42), ("dense", 5, 512)])
def test_multistep_iteration_on_the_kinds_output(arch, B, C, name):
    import smd_amd.schedule as S
    import smd_amd.lib as lib
    kind = KINDS[name]
    model, eng = _engine(arch, C, B, name)
    Sq, dev = eng.S, eng.device
    shape = (B, Sq, C) if Sq > 1 else (B, C)
    taus = logsnr_taus()
    n = len(taus)
    g = torch.Generator().manual_seed(22 + kind)
    worst = worst_h = 0.0
    for clip in (1.0, float("inf")):
        coef, plan = S.multistep_coefficient_table(BETAS, taus, 2, clip, prediction=name)
        sp, keep = plan_struct(coef, plan, dev)
        rows = MR.table_rows(coef, plan, taus, BETAS)
        for j in (0, 1, n // 2, n - 1):                                # t = T - 1 (no history), with history, t = 0
            t = int(taus[j])
            x = (torch.randn(*shape, generator=g) * (1.0 if j < n - 1 else 0.5)).to(dev)
            hist = torch.clamp(0.5 * torch.randn(*shape, generator=g), -1, 1).to(dev)
            x_in, hist_in = x.clone(), hist.clone()
            t_ptr = torch.tensor([t], dtype=torch.int32, device=dev)
            mp = torch.zeros((T, B, 3), device=dev)
            coll = torch.full((41, *shape), 7.0, device=dev)
            io = lib.SampleIO()
            io.x, io.t_ptr = x.data_ptr(), t_ptr.data_ptr()
            io.metrics_partial, io.collection = mp.data_ptr(), coll.data_ptr()
            eng.load_state(x)
            eng.multistep_step(io, sp, hist)
            torch.cuda.synchronize()
            out = eng.last_pred().clone()
            eq = torch.from_numpy(R.eps_of(kind, d(x_in).numpy(), d(out).numpy(), AP[t]))
            a0, a1, cb = (float(coef[t, k]) for k in (2, 8, 3))
            row = {k: (int(v[j]) if k in ("t", "next_t") else float(v[j])) for k, v in rows.items()}
            row["sqrt_recip"], row["sqrt_m1"] = exact_eps_row(t)
            ref, x0, _ = MR.update(d(x_in), eq, d(hist_in), row, T)
            mag = (a0 * x0).abs() + (a1 * d(hist_in)).abs() + (cb * d(x_in)).abs()
            bound = 4 * 2.0 ** -23 * mag + table_slack(kind, a0, t, d(x_in), d(out)) + 1e-12
            ratio = float(((d(x) - ref).abs() / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (name, clip, t, ratio)
            # the stored history: the clamped x0 this kind's columns recover
            c0, c1 = (float(v) for v in R.x0_coefficients(kind, AP[t]))
            mag_h = (c0 * d(x_in)).abs() + (c1 * d(out)).abs()
            ratio_h = float(((d(hist) - x0).abs() / (4 * 2.0 ** -23 * mag_h + table_slack(kind, 1.0, t, d(x_in), d(out)) + 1e-12)).max())
            worst_h = max(worst_h, ratio_h)
            assert ratio_h <= 1.0, (name, clip, t, ratio_h)
            assert float(hist.abs().max()) <= clip
    print(f"[multistep {name} {arch} B={B} C={C}] worst |err| / bound = {worst:.3f}, history {worst_h:.3f}")
