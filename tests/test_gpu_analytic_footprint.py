"""Footprints of the analytic-variance entry points with the guarded arenas of tests/_footprint.py:
smd_score_moments and smd_engine_analytic_step write only their documented outputs, leave their inputs alone and do not depend
on what lies around them."""
import numpy as np
import pytest
import torch

import _footprint as F
from test_gpu_full_walk import BETAS
from test_gpu_strided import transformer_model

pytestmark = pytest.mark.gpu
T = 1000
K = 20
DEV = "cuda:0"


@pytest.mark.parametrize("B,S,C", [(3, 32, 42), (19, 32, 512), (5, 1, 42)])
def test_score_moments_footprint(B, S, C):
    import smd_amd.lib as lib
    import smd_amd.schedule as Sch
    L = lib.get_lib()
    table, next_t = Sch.analytic_moment_tables(BETAS, np.arange(T), "v")
    g = torch.Generator().manual_seed(B + C)
    x_c, o_c = torch.randn(B, S, C, generator=g), torch.randn(B, S, C, generator=g)
    chunks = (B + lib.MOMENT_CHUNK - 1) // lib.MOMENT_CHUNK
    results = []
    for fill in F.PATTERNS:
        x, hx = F.guarded_like(x_c, DEV, fill=fill)
        o, ho = F.guarded_like(o_c, DEV, fill=fill)
        tab, ht = F.guarded_like(torch.from_numpy(table), DEV, fill=fill)
        nt, hn = F.guarded_like(torch.from_numpy(next_t), DEV, fill=fill)
        part, hp = F.guarded((chunks, S * C), torch.float32, DEV, fill=fill)
        sums, hs = F.guarded((T, S * C), torch.float32, DEV, fill=fill)
        tp, htp = F.guarded((1,), torch.int32, DEV, fill=fill)
        ar, har = F.guarded((1,), torch.int32, DEV, fill=fill)
        t = 500
        tp.fill_(t)
        ar.zero_()
        before = sums.clone()
        with F.unchanged(hx, ho, ht, hn):
            lib.check(L.smd_score_moments(x.data_ptr(), o.data_ptr(), B, S, C, tab.data_ptr(), T, tp.data_ptr(), nt.data_ptr(),
                                          ar.data_ptr(), part.data_ptr(), sums.data_ptr(), None), "score_moments")
            torch.cuda.synchronize()
        for name, h in (("x_t", hx), ("out", ho), ("table", ht), ("next_t", hn), ("partial", hp), ("sums", hs), ("t_ptr", htp), ("arrive", har)):
            h.assert_untouched(name)
        assert int(tp.item()) == t + 1 and int(ar.item()) == 0
        rest = torch.ones(T, dtype=torch.bool)
        rest[t] = False
        assert torch.equal(sums[rest].view(torch.int32), before[rest].view(torch.int32))      # the other rows keep their sentinel bits
        assert bool(torch.isfinite(sums[t]).all()) and bool(torch.isfinite(part).all())          # every element of row t and of the partials
        results.append(sums[t].clone())
    assert torch.equal(results[0], results[1])


@pytest.mark.parametrize("C", [42, 512])
def test_analytic_step_footprint(C):
    import smd_amd.lib as lib
    import smd_amd.schedule as Sch
    model = transformer_model(C)
    eng = model.engine
    B, S = 3, eng.S
    eng.set_schedule(BETAS, with_sampler=True)
    eng.bind(B, training=False)
    eng.prepare_sampler()
    taus = Sch.stride_timesteps(T, K)
    coef, plan = Sch.strided_coefficient_table(BETAS, taus, 1.0)
    coef[taus, 4] = 1.0
    g = torch.Generator().manual_seed(C)
    x_c, z_c = torch.randn(B, S, C, generator=g), torch.randn(B, S, C, generator=g)
    sig_c = 0.05 + torch.rand(K, S, C, generator=g)
    j = 4
    t = int(taus[j])
    results = []
    for fill in F.PATTERNS:
        x, hx = F.guarded_like(x_c, DEV, fill=fill)
        z, hz = F.guarded_like(z_c, DEV, fill=fill)
        sig, hsg = F.guarded_like(sig_c, DEV, fill=fill)
        cf, hc = F.guarded_like(torch.from_numpy(coef), DEV, fill=fill)
        pl, hpl = F.guarded_like(torch.from_numpy(plan), DEV, fill=fill)
        mp, hm = F.guarded((T, B * 3), torch.float32, DEV, fill=fill)
        coll, hco = F.guarded((41, B * S * C), torch.float32, DEV, fill=fill)
        tp, htp = F.guarded((1,), torch.int32, DEV, fill=fill)
        tp.fill_(t)
        sp = lib.StridePlan()
        sp.coef, sp.plan, sp.T = cf.data_ptr(), pl.data_ptr(), T
        st = lib.SigmaTable()
        st.sig, st.K = sig.data_ptr(), K
        io = lib.SampleIO()
        io.x, io.t_ptr, io.z_in = x.data_ptr(), tp.data_ptr(), z.data_ptr()
        io.metrics_partial, io.collection = mp.data_ptr(), coll.data_ptr()
        eng.load_state(x)
        mp_before, coll_before = mp.clone(), coll.clone()
        with F.unchanged(hz, hsg, hc, hpl):
            eng.analytic_step(io, sp, st)
            torch.cuda.synchronize()
        for name, h in (("state", hx), ("z", hz), ("sig", hsg), ("coef", hc), ("plan", hpl), ("metrics", hm), ("collection", hco), ("t_ptr", htp)):
            h.assert_untouched(name)
        assert int(tp.item()) == int(plan[t, 0])
        slot = int(plan[t, 2])
        for k in range(41):
            if k == slot:
                assert torch.equal(coll[k], x.reshape(-1))
            else:
                assert torch.equal(coll[k].view(torch.int32), coll_before[k].view(torch.int32))
        rest = torch.ones(T, dtype=torch.bool)
        rest[t] = False
        assert torch.equal(mp[rest].view(torch.int32), mp_before[rest].view(torch.int32)) and bool(torch.isfinite(mp[t]).all())
        assert bool(torch.isfinite(x).all())
        results.append((x.clone(), mp[t].clone()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
