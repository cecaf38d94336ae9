"""Footprint of the fused exponential Adams update (smd_adams_step), in the style of
tests/test_gpu_footprint.py: every buffer in a guarded arena (tests/_footprint.py).  The kernel writes the state, ITS slot of the
ring, the planned collection row, the logical columns of the bf16 copy, its metric row and the timestep (and leaves the arrival
counter zero); the other two ring slots, every other collection and metric row, the bf16 padding columns, the tables and the infill
arrays keep their bytes, and no sentinel byte around any of them changes -- under both sentinels, with the same result."""
import ctypes

import pytest
import torch

import _adams_ref as A
import _footprint as F
from test_gpu_full_walk import BETAS

pytestmark = pytest.mark.gpu
T = 1000


@pytest.mark.parametrize("shape,Cp", [((3, 32, 42), 48), ((2, 5, 516), 528)])
def test_adams_step_writes_only_its_outputs(shape, Cp):
    import smd_amd.lib as lib
    import smd_amd.schedule as S
    B, Sq, C = shape
    dev = torch.device("cuda:0")
    P = lambda t: t.data_ptr()
    taus = A.logsnr_timesteps(T, 20, BETAS)
    coef_np, plan_np = S.adams_coefficient_table(BETAS, taus, True)
    j = 4
    t = int(taus[j])
    slot = int(plan_np[t, 2])
    assert all(coef_np[t, c] != 0 for c in (2, 8, 9, 10)) and 0 < slot <= 40
    g = torch.Generator().manual_seed(4)
    x0, eh0, iz = (torch.randn(*shape, generator=g) for _ in range(3))
    ring0 = torch.clamp(0.5 * torch.randn(3, *shape, generator=g), -1, 1)
    samples, masks = torch.clamp(0.25 * torch.randn(*shape, generator=g), -1, 1), (torch.rand(*shape, generator=g) < 0.5).float()
    results = []
    for fill in F.PATTERNS:
        guard = lambda src: F.guarded_like(src, dev, fill=fill)
        ins = [guard(v) for v in (torch.from_numpy(coef_np), torch.from_numpy(plan_np), eh0, iz, samples, masks)]
        (coef, _), (plan, _), (eh, _), (izd, _), (sd, _), (md, _) = ins
        snaps = [h.snapshot() for _, h in ins]
        x, x_h = guard(x0)
        ring, ring_h = guard(ring0)
        t_ptr, t_h = guard(torch.tensor([t], dtype=torch.int32))
        arrive, a_h = guard(torch.zeros(1, dtype=torch.int32))
        mp, mp_h = F.guarded((T, B, 3), torch.float32, dev, fill=fill)
        coll, coll_h = F.guarded((41, *shape), torch.float32, dev, fill=fill)
        xb, xb_h = F.guarded((B * Sq, C), torch.bfloat16, dev, ld=Cp, fill=fill)          # the padding columns are sentinel
        a = lib.AdamsStepArgs()
        a.x, a.hist, a.eps_hat = P(x), P(ring), P(eh)
        a.B, a.S, a.C, a.Cp, a.T = B, Sq, C, Cp, T
        a.coef, a.plan, a.t_ptr, a.t_advance, a.arrive = P(coef), P(plan), P(t_ptr), P(t_ptr), P(arrive)
        a.infill_samples, a.infill_masks, a.infill_z_in = P(sd), P(md), P(izd)
        a.x_bf16, a.metrics_partial, a.collection = P(xb), P(mp), P(coll)
        lib.check(lib.get_lib().smd_adams_step(ctypes.byref(a), torch.cuda.current_stream().cuda_stream), "adams_step")
        torch.cuda.synchronize()
        for name, h in (("x", x_h), ("ring", ring_h), ("t", t_h), ("arrive", a_h), ("metrics_partial", mp_h), ("collection", coll_h),
                        ("x_bf16", xb_h)):
            h.assert_untouched(name)
        for (_, h), snap in zip(ins, snaps):
            h.assert_same(snap, "input")
        word = torch.tensor([fill | fill << 16], dtype=torch.int64).to(torch.int32).to(dev)
        poison = lambda v: bool((v.contiguous().view(torch.int32) == word).all())
        assert int(t_ptr.item()) == int(plan_np[t, 0]) and int(arrive.item()) == 0
        rows_poison = (mp.contiguous().view(torch.int32).view(T, -1) == word).all(dim=1)
        assert bool(rows_poison[:t].all()) and bool(rows_poison[t + 1:].all()) and bool(torch.isfinite(mp[t]).all())
        assert all(poison(coll[k]) for k in range(41) if k != slot) and torch.equal(coll[slot], x)
        own = j % 3
        for k in range(3):
            if k != own:
                assert torch.equal(ring[k].cpu().view(torch.int32), ring0[k].view(torch.int32)), k
        assert bool(torch.isfinite(ring[own]).all()) and float(ring[own].abs().max()) <= 1.0 and not torch.equal(ring[own].cpu(), ring0[own])
        assert torch.equal(xb, x.reshape(-1, C).to(torch.bfloat16))
        results.append((x.clone().cpu(), ring.clone().cpu(), mp[t].clone().cpu()))
    assert all(torch.equal(u, v) for u, v in zip(results[0], results[1]))
    assert bool(torch.isfinite(results[0][0]).all())
