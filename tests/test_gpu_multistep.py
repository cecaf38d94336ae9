"""The second-order multistep sampler (DPM-Solver++(2M)) on the GPU: the fused update alone against float64, the history that is
not read where a1 = 0, the kernel at w = 0 against the strided kernel, fp32 and bf16 walks against the float64 walk of
tests/_multistep_ref.py, the graph / two-chain arrangements, the "multistep" cache slot, infill and the footprint of
smd_engine_multistep_step.

Bounds.  The update alone: |err| <= 4 * 2^-23 * (|a0 x0| + |a1 x0_prev| + |b x| + |y|) + 1e-12 per element, the stored history
|err| <= 4 * 2^-23 * (|sqrt_recip x| + |sqrt_m1 eps_hat|) + 1e-12.  fp32 walks: 4 x g32, the float32 CPU walk of _multistep_ref
against its float64 walk (DESIGN.md section 13's rule).  bf16 walks: measured on an MI355X x 1.5 (BF16_MEASURED below, DESIGN.md
section 18), which must stay under the 5e-2 SURVEY 8(c) allows bf16 samplers.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _footprint as F
import _multistep_ref as R
import ddpm_oracle as O
from test_gpu_full_walk import BETAS, make, rel
from test_gpu_strided import dense_model, find_bf16_input, partials64, transformer_model, worst_rel

pytestmark = pytest.mark.gpu
T = 1000
K = 20                                                                 # the logsnr grid snaps it to 18 iterations
# bf16 walks (order 2, logsnr, K = 20) against float64, rel-L2, worst of final state and snapshots, measured on an MI355X:
# plain walks (small B = 4, base B = 2) and the small network's infill walk with explicit draws
BF16_MEASURED = {"small": 8.27e-3, "base": 8.25e-3, "small_infill": 5.94e-3}
NETS = {"small": (42, 2, 8, 1, 4), "base": (512, 6, 8, 2, 2)}          # C, L, H, mlp layers, B


def logsnr_taus():
    return R.logsnr_timesteps(T, K, BETAS)


def tables(order, taus, clip=1.0):
    import smd_amd.schedule as S
    return S.multistep_coefficient_table(BETAS, taus, order, clip)


def plan_struct(coef, plan, dev):
    import smd_amd.lib as lib
    coef_d, plan_d = torch.from_numpy(coef).to(dev), torch.from_numpy(plan).to(dev)
    sp = lib.MultistepPlan()
    sp.coef, sp.plan, sp.T = coef_d.data_ptr(), plan_d.data_ptr(), T
    return sp, (coef_d, plan_d)


def noise(shape, t, stream=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(200_000 + 7919 * stream + t))


# ------------------------------------------------------------------ the update alone
# the last three rows: VEC = 1 with one row group; two trips of the column loop, the last with 18 live threads (VEC = 1) and
# with one live thread (VEC = 4)
@pytest.mark.parametrize("arch,B,C", [("transformer", 3, 42), ("transformer", 3, 512), ("dense", 5, 512),
                                      ("dense", 5, 42), ("transformer", 3, 146), ("dense", 3, 1028)])
def test_fused_update_alone_against_float64(arch, B, C):
    """One launch at a time on random x, history, masks: the network's own eps_hat is read back and the update is recomputed in
    float64 from the float32 tables the kernel read.  C = 42: VEC = 1 and a masked last column block; C = 512: VEC = 4;
    DenseDDPM: one row group and channel-axis norms.  Iterations 0 (a1 = 0), 1, the middle and the last (a1 = 0, b = 0)."""
    import smd_amd.lib as lib
    model = transformer_model(C) if arch == "transformer" else dense_model(C)
    eng = model.engine
    Sq = eng.S
    shape = (B, Sq, C) if Sq > 1 else (B, C)
    dev = eng.device
    eng.set_schedule(BETAS, with_sampler=True)
    eng.bind(B, training=False)
    eng.prepare_sampler()
    taus = logsnr_taus()
    n = len(taus)
    g = torch.Generator().manual_seed(12)
    samples = torch.clamp(0.25 * torch.randn(*shape, generator=g), -1, 1).to(dev)
    masks = (torch.rand(*shape, generator=g) < 0.5).float().to(dev)
    located = None
    worst = worst_h = 0.0
    d = lambda v: v.double().cpu()
    for clip in (1.0, float("inf")):
        coef, plan = tables(2, taus, clip)
        sp, keep = plan_struct(coef, plan, dev)
        rows = R.table_rows(coef, plan, taus, BETAS)
        for j in (0, 1, n // 2, n - 1):
            t = int(taus[j])
            for infill in (False, True):
                x = (torch.randn(*shape, generator=g) * (1.0 if j < n - 1 else 0.5)).to(dev)
                hist = torch.clamp(0.5 * torch.randn(*shape, generator=g), -1, 1).to(dev)
                iz = torch.randn(*shape, generator=g).to(dev)
                x_in, hist_in = x.clone(), hist.clone()
                t_ptr = torch.tensor([t], dtype=torch.int32, device=dev)
                mp = torch.zeros((T, B, 3), device=dev)
                coll = torch.full((41, *shape), 7.0, device=dev)
                io = lib.SampleIO()
                io.x, io.t_ptr = x.data_ptr(), t_ptr.data_ptr()
                io.metrics_partial, io.collection = mp.data_ptr(), coll.data_ptr()
                if infill:
                    io.infill_samples, io.infill_masks, io.infill_z_in = samples.data_ptr(), masks.data_ptr(), iz.data_ptr()
                eng.load_state(x)
                if located is None:
                    torch.cuda.synchronize()
                    located = find_bf16_input(eng, x)
                eng.multistep_step(io, sp, hist)
                torch.cuda.synchronize()
                eh = eng.last_pred().clone()
                a0, a1, cb = (float(coef[t, k]) for k in (2, 8, 3))
                assert (a1 == 0) == (j in (0, n - 1))
                row = {k: (int(v[j]) if k in ("t", "next_t") else float(v[j])) for k, v in rows.items()}
                ref, x0, y = R.update(d(x_in), d(eh), d(hist_in), row, T, d(masks) if infill else None, d(samples), d(iz))
                mag = (a0 * x0).abs() + (a1 * d(hist_in)).abs() + (cb * d(x_in)).abs() + (y.abs() if infill else 0)
                ratio = float(((d(x) - ref).abs() / (4 * 2.0 ** -23 * mag + 1e-12)).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (clip, t, infill, ratio)
                # the stored history: the clamped x0 the update used, before the infill blend
                mag_h = (float(coef[t, 0]) * d(x_in)).abs() + (float(coef[t, 1]) * d(eh)).abs()
                ratio_h = float(((d(hist) - x0).abs() / (4 * 2.0 ** -23 * mag_h + 1e-12)).max())
                worst_h = max(worst_h, ratio_h)
                assert ratio_h <= 1.0, (clip, t, infill, ratio_h)
                assert float(hist.abs().max()) <= clip
                # bf16 copy: round-to-nearest of the fp32 state, padding zero
                off, nbytes, (nrows, Cp) = located
                xb = eng.workspace[off:off + nbytes].view(torch.bfloat16).view(nrows, Cp)
                assert torch.equal(xb[:, :C], x.reshape(nrows, C).to(torch.bfloat16)) and not bool(xb[:, C:].any())
                assert int(t_ptr.item()) == int(plan[t, 0])
                # metric partials: row t only; the noise norm is that of zeros
                want = torch.stack([partials64(d(eh), Sq), partials64(d(x_in) - ref, Sq), partials64(torch.zeros_like(ref), Sq)], dim=1)
                got = mp[t].double().cpu()
                assert float(((got - want).abs() / want.abs()).max()) <= 1e-5, (got, want)
                mp[t] = 0
                assert not bool(mp.any())
                # collection: the planned slot only
                slot = int(plan[t, 2])
                for k in range(41):
                    if k == slot:
                        assert torch.equal(coll[k], x)
                    else:
                        assert bool((coll[k] == 7.0).all()), (k, slot)
        # the terminators (and a timestep that is not on the walk): nothing changes, bit for bit
        for t_end in (-1, T, int(taus[0]) - 1):
            t_ptr.fill_(t_end)
            mp.zero_()
            before = [v.clone() for v in (x, hist, mp, coll, eng.workspace[off:off + nbytes])]
            eng.multistep_step(io, sp, hist)
            torch.cuda.synchronize()
            for u, v in zip(before, (x, hist, mp, coll, eng.workspace[off:off + nbytes])):
                assert torch.equal(u.view(torch.uint8), v.view(torch.uint8))
            assert int(t_ptr.item()) == t_end
    print(f"[{arch} B={B} C={C}] fused multistep update: worst |err| / bound = {worst:.3f} (state), {worst_h:.3f} (history)")
    t_ptr.fill_(int(taus[0]))
    if C % 4 == 0:                                                     # 16-byte loads: a history 4 bytes off is refused
        with pytest.raises(ValueError, match="16-byte aligned"):
            lib.check(eng.L.smd_engine_multistep_step(eng.h, ctypes.byref(io), ctypes.byref(sp), hist.data_ptr() + 4, 0,
                                                      torch.cuda.current_stream().cuda_stream), "multistep_step")
    with pytest.raises(ValueError, match="null history"):
        lib.check(eng.L.smd_engine_multistep_step(eng.h, ctypes.byref(io), ctypes.byref(sp), None, 0,
                                                  torch.cuda.current_stream().cuda_stream), "multistep_step")
    torch.cuda.synchronize()
    assert int(t_ptr.item()) == int(taus[0])


@pytest.mark.parametrize("C", [42, 512])
def test_history_is_not_read_when_a1_is_zero(C):
    """the first and the last iteration with a history of NaNs: the new state is finite and bitwise the run with a zero history,
    and the history comes out overwritten"""
    import smd_amd.lib as lib
    model = transformer_model(C)
    eng = model.engine
    dev = eng.device
    B = 3
    eng.set_schedule(BETAS, with_sampler=True)
    eng.bind(B, training=False)
    eng.prepare_sampler()
    taus = logsnr_taus()
    coef, plan = tables(2, taus)
    sp, keep = plan_struct(coef, plan, dev)
    x_in = torch.randn(B, 32, C, generator=torch.Generator().manual_seed(13)).to(dev)
    for t in (taus[0], taus[-1]):
        assert coef[t, 8] == 0
        out = []
        for fill in (float("nan"), 0.0):
            x = x_in.clone()
            hist = torch.full_like(x, fill)
            t_ptr = torch.tensor([t], dtype=torch.int32, device=dev)
            io = lib.SampleIO()
            io.x, io.t_ptr = x.data_ptr(), t_ptr.data_ptr()
            eng.load_state(x)
            eng.multistep_step(io, sp, hist)
            torch.cuda.synchronize()
            out.append((x, hist))
        assert bool(torch.isfinite(out[0][0]).all()) and bool(torch.isfinite(out[0][1]).all())
        assert torch.equal(out[0][0].view(torch.int32), out[1][0].view(torch.int32))
        assert torch.equal(out[0][1].view(torch.int32), out[1][1].view(torch.int32))


@pytest.mark.parametrize("infill", [False, True])
def test_the_kernel_at_w_zero_is_the_strided_kernel(infill):
    """order-1 tables through smd_engine_multistep_step on the uniform grid: final state, collection and ld_metrics are those of
    strided_dynamics(eta = 0), bit for bit"""
    import smd_amd.ncsn as N
    import smd_amd.schedule as S
    _, _, model = make(42, 2, 8, 1)
    B = 4
    g = torch.Generator().manual_seed(14)
    init = torch.randn(B, 32, 42, generator=g)
    kw = {}
    if infill:
        mask = torch.zeros(B, 32, 42)
        mask[:, 8:24] = 1.0
        kw = dict(infill=True, infill_samples=torch.clamp(0.25 * torch.randn(B, 32, 42, generator=g), -1, 1), infill_masks=mask)
    want = N.strided_dynamics(N.PRNGKey(3), model, BETAS, init, K, 0.0, **kw)
    taus = S.stride_timesteps(T, K)
    coef, plan = S.multistep_coefficient_table(BETAS, taus, 1)
    for use_graph in (True, False):
        x, coll, mp = N._strided_walk("multistep", N.PRNGKey(3), model, BETAS, init, [int(t) for t in taus], coef, plan,
                                      ("multistep", K, 1, "uniform"), collect=True, use_graph=use_graph, multistep=True, **kw)
        got = (x, coll, N._walk_ld_metrics(model, BETAS, taus, mp))
        assert all(torch.equal(u, v) for u, v in zip(got, want)), use_graph
    assert bool(torch.isfinite(want[0]).all()) and float((want[0].cpu() - init).abs().max()) > 0


# ------------------------------------------------------------------ walks
@functools.lru_cache(maxsize=None)
def reference(name):
    """the float64 and the float32 walk of _multistep_ref on the CPU oracle's network, computed once: order 2, logsnr, K = 20"""
    C, L, H, Km, B = NETS[name]
    ocfg, p, _ = make(C, L, H, Km, dtype="fp32")
    init = torch.randn(B, 32, C, generator=torch.Generator().manual_seed(34))
    taus = logsnr_taus()
    co = R.coefficients(BETAS, taus, 2)
    out = []
    with torch.no_grad():
        for dt in (torch.float64, torch.float32):
            m = O.make_model({k: v.to(dt) for k, v in p.items()}, ocfg)
            out.append(R.walk(m, co, init.to(dt), T, collect=R.slots(len(taus))))
    (rx, rc, rm), (fx, fc, fm) = out
    return p, init, taus, (rx, rc, rm), worst_rel(fx, fc, rx, rc), max(rel(fm[i], rm[i]) for i in (0, 1))


@pytest.mark.parametrize("name", ["small", "base"])
def test_fp32_walk_against_the_float64_walk(name):
    import smd_amd.ncsn as N
    C, L, H, Km, B = NETS[name]
    p, init, taus, (rx, rc, rm), g_state, g_met = reference(name)
    _, _, model = make(C, L, H, Km, dtype="fp32")
    n = len(taus)
    x, coll, met = N.strided_dynamics(N.PRNGKey(0), model, BETAS, init, K, 0.0, order=2, spacing="logsnr")
    assert model.sampler_arrangement["walk"] == "multistep" and model.sampler_arrangement["iterations"] == n == 18
    assert tuple(coll.shape) == (41, B, 32, C) and tuple(met.shape) == (4, n, 1)
    written = sorted(k for k in range(1, 41) if float(coll[k].abs().max()) > 0)
    assert written == sorted(rc) and torch.equal(coll[0].cpu(), init)
    e_state = worst_rel(x, coll, rx, rc)
    m = met[:, :, 0].cpu().double()
    e_met = max(rel(m[i], rm[i]) for i in (0, 1))
    print(f"[fp32 multistep walk {name} K={K} ({n} iterations)] g32: state {g_state:.3e} metrics {g_met:.3e} | GPU: state + snapshots "
          f"{e_state:.3e} (ratio {e_state / g_state:.2f}), metric rows {e_met:.3e} (ratio {e_met / g_met:.2f})")
    assert e_state <= 4 * g_state
    assert e_met <= 4 * g_met
    assert rel(m[2], rm[2]) < 1e-6                                     # the alpha row is table data
    assert float(m[3].max()) == pytest.approx(1e-5, rel=1e-3)          # no noise: the norm of zeros
    assert float(x.abs().max()) <= 1.0                                 # the last iteration returns the clamped x0


@pytest.mark.parametrize("name", ["small", "base"])
def test_bf16_walk_against_the_float64_walk(name):
    import smd_amd.ncsn as N
    C, L, H, Km, B = NETS[name]
    p, init, taus, (rx, rc, _), _, _ = reference(name)
    _, _, model = make(C, L, H, Km)
    x, coll, _ = N.strided_dynamics(N.PRNGKey(0), model, BETAS, init, K, 0.0, order=2, spacing="logsnr", use_graph=False)
    e = worst_rel(x, coll, rx, rc)
    print(f"[bf16 multistep walk {name} K={K} B={B}] worst rel-L2 of state + snapshots against float64: {e:.3e}")
    tol = 1.5 * BF16_MEASURED[name]
    assert tol < 5e-2
    assert e < tol


# ------------------------------------------------------------------ arrangements
def test_graph_replay_equals_eager_bitwise():
    import smd_amd.ncsn as N
    _, _, model = make(42, 2, 8, 1)
    init = torch.randn(4, 32, 42, generator=torch.Generator().manual_seed(5))
    a = N.strided_dynamics(N.PRNGKey(9), model, BETAS, init, K, order=2, spacing="logsnr", use_graph=True)
    assert model.sampler_arrangement["graphed"] and model.sampler_arrangement["chains"] == 1
    b = N.strided_dynamics(N.PRNGKey(9), model, BETAS, init, K, order=2, spacing="logsnr", use_graph=False)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    c = N.strided_dynamics(N.PRNGKey(9), model, BETAS, init, K, order=1, spacing="logsnr")
    assert rel(c[0], a[0]) > 1e-3                                      # the history term is really there
    with pytest.raises(ValueError, match="eta must be 0"):
        N.strided_dynamics(N.PRNGKey(9), model, BETAS, init, K, 0.5, order=2)
    with pytest.raises(ValueError, match="order"):
        N.strided_dynamics(N.PRNGKey(9), model, BETAS, init, K, order=3)


@pytest.mark.parametrize("infill", [False, True])
def test_two_chain_walk_equals_one_chain_and_eager(infill, monkeypatch):
    """B = 136 walks as 72 + 64 pipelined chains, each with its own history: 18 iterations are 17 replays, two graphs of 8
    iterations and one as plain launches.  The comparison and tolerance of tests/test_gpu_strided.py's."""
    import smd_amd.ncsn as N
    _, _, model = make(C=512, L=2, H=8, K=1)
    B = 136
    g = torch.Generator().manual_seed(77)
    init = torch.randn(B, 32, 512, generator=g)
    kw = {}
    if infill:
        mask = torch.zeros(B, 32, 512)
        mask[:, 8:24] = 1.0
        kw = dict(infill=True, infill_samples=torch.clamp(0.25 * torch.randn(B, 32, 512, generator=g), -1, 1), infill_masks=mask)

    def walk(chains, graph):
        monkeypatch.setenv("SMD_SAMPLER_CHAINS", str(chains))
        out = N.strided_dynamics(N.PRNGKey(5), model, BETAS, init, K, 0.0, use_graph=graph, order=2, spacing="logsnr", **kw)
        return out, dict(model.sampler_arrangement)

    (x2, c2, m2), arr = walk(2, True)
    assert arr["chain_sizes"] == [72, 64] and arr["pipelined_unroll"] == 8 and arr["padded"] == 0 and arr["walk"] == "multistep"
    (x1, c1, m1), arr1 = walk(1, True)
    (xe, ce, me), _ = walk(1, False)
    assert arr1["chains"] == 1
    assert torch.equal(x1, xe) and torch.equal(c1, ce) and torch.equal(m1, me)      # one chain: replay == eager, bitwise
    slots = [s for s in R.slots(len(logsnr_taus())) if s >= 0]
    assert torch.equal(c2[0], c1[0]) and all(float(c2[s].abs().max()) > 0 for s in slots)
    assert rel(x2, x1) < 5e-3, rel(x2, x1)
    assert all(rel(c2[s], c1[s]) < 5e-3 for s in slots)
    assert rel(m2[0], m1[0]) < 5e-3 and rel(m2[1], m1[1]) < 5e-3
    assert torch.equal(m2[2], m1[2])
    assert float((x2[72:] - init[72:].cuda()).abs().max()) > 0
    if infill:
        m = kw["infill_masks"].cuda().bool()
        assert torch.equal(x2[m], kw["infill_samples"].cuda()[m])                    # the last iteration returns the template


# ------------------------------------------------------------------ cache
def test_cache_reuse_other_starts_and_slots():
    import smd_amd.ncsn as N
    g = torch.Generator().manual_seed(6)
    init, other = torch.randn(4, 32, 42, generator=g), torch.randn(4, 32, 42, generator=g)
    ms = lambda m, start: N.strided_dynamics(N.PRNGKey(1), m, BETAS, start, K, order=2, spacing="logsnr")
    _, _, model = make(42, 2, 8, 1)
    first = ms(model, init)
    entry = model._sampler_graphs["multistep"]
    second = ms(model, init)                                           # reused graphs, a history left by the first walk
    assert model._sampler_graphs["multistep"] is entry
    assert all(torch.equal(u, v) for u, v in zip(first, second))
    third = ms(model, other)
    assert model._sampler_graphs["multistep"] is entry
    _, _, fresh = make(42, 2, 8, 1)
    assert all(torch.equal(u, v) for u, v in zip(third, ms(fresh, other)))
    # another (iterations, order, spacing) replaces the slot; the other walks keep theirs
    N.strided_dynamics(N.PRNGKey(1), model, BETAS, init, K, order=2, spacing="uniform")
    assert model._sampler_graphs["multistep"] is not entry
    N.diffusion_dynamics(N.PRNGKey(1), model, BETAS, init, t_stop=985)
    sd = N.strided_dynamics(N.PRNGKey(1), model, BETAS, init, K, order=1)
    ms(model, init)
    N.ddim_encode(model, BETAS, torch.clamp(0.25 * init, -1, 1), K)
    assert set(model._sampler_graphs) == {"entry", "strided", "multistep", "encode"}
    kept = model._sampler_graphs["strided"]
    ms(model, other)
    assert model._sampler_graphs["strided"] is kept
    assert all(torch.equal(u, v) for u, v in zip(sd, N.strided_dynamics(N.PRNGKey(1), model, BETAS, init, K, order=1)))
    model.drop_sampler_cache()
    assert "_sampler_graphs" not in model.__dict__


@pytest.mark.parametrize("order", [2, 1])
def test_steps_that_snap_to_the_same_number_of_iterations_do_not_share_graphs(order):
    """on the lambda grid K = 19 and K = 20 are both 18 iterations, on different timesteps: the cached entry of one must not
    serve the other (its device tables are the first call's).  Order 2 in the "multistep" slot, order 1 in "strided"."""
    import smd_amd.ncsn as N
    import smd_amd.schedule as S
    t19, t20 = (list(S.logsnr_timesteps(T, k, BETAS)) for k in (19, 20))
    assert len(t19) == len(t20) == 18 and t19 != t20
    init = torch.randn(4, 32, 42, generator=torch.Generator().manual_seed(10))
    walk = lambda m, k: N.strided_dynamics(N.PRNGKey(1), m, BETAS, init, k, order=order, spacing="logsnr")
    slot = "multistep" if order == 2 else "strided"
    _, _, model = make(42, 2, 8, 1)
    a19 = walk(model, 19)
    entry = model._sampler_graphs[slot]
    a20 = walk(model, 20)
    assert model._sampler_graphs[slot] is not entry
    _, _, fresh = make(42, 2, 8, 1)
    want = walk(fresh, 20)
    assert all(torch.equal(u, v) for u, v in zip(a20, want))
    assert not torch.equal(a19[0], a20[0])
    assert float(a20[2][0].min()) > 0                                  # every metric row of the K = 20 walk was written
    entry = model._sampler_graphs[slot]
    assert all(torch.equal(u, v) for u, v in zip(walk(model, 20), want)) and model._sampler_graphs[slot] is entry


def test_engine_refuses_a_history_that_is_not_the_states_twin():
    import smd_amd.lib as lib
    model = transformer_model(42)
    eng = model.engine
    eng.set_schedule(BETAS, with_sampler=True)
    eng.bind(3, training=False)
    eng.prepare_sampler()
    sp, keep = plan_struct(*tables(2, logsnr_taus()), eng.device)
    x = torch.randn(3, 32, 42, device=eng.device)
    t_ptr = torch.tensor([T - 1], dtype=torch.int32, device=eng.device)
    io = lib.SampleIO()
    io.x, io.t_ptr = x.data_ptr(), t_ptr.data_ptr()
    before = x.clone()
    for bad in (torch.zeros(3, 32, 42, dtype=torch.bfloat16, device=eng.device), torch.zeros(2, 32, 42, device=eng.device),
                torch.zeros(3, 32, 84, device=eng.device)[:, :, ::2], torch.zeros(3, 32, 42)):
        with pytest.raises(ValueError, match="x0_prev must be"):
            eng.multistep_step(io, sp, bad)
    torch.cuda.synchronize()
    assert torch.equal(x, before) and int(t_ptr.item()) == T - 1


# ------------------------------------------------------------------ infill
@pytest.mark.parametrize("rng", ["philox", "threefry"])
def test_infill_returns_the_known_region_exactly(rng):
    import smd_amd.jax_random as J
    import smd_amd.ncsn as N
    _, _, model = make(42, 2, 8, 1)
    B = 4
    g = torch.Generator().manual_seed(8)
    init = torch.randn(B, 32, 42, generator=g)
    samples = torch.clamp(0.25 * torch.randn(B, 32, 42, generator=g), -1, 1)
    mask = torch.zeros(B, 32, 42)
    mask[:, 8:24] = 1.0
    key = J.PRNGKey(3) if rng == "threefry" else N.PRNGKey(3)
    x, coll, _ = N.strided_dynamics(key, model, BETAS, init, K, 0.0, True, samples, mask, order=2, spacing="logsnr")
    assert model.sampler_arrangement["rng"] == rng
    m = mask.cuda().bool()
    assert torch.equal(x[m], samples.cuda()[m])
    assert bool(torch.isfinite(x).all()) and float((x[~m] - samples.cuda()[~m]).abs().max()) > 0
    assert float((coll[40][m] - samples.cuda()[m]).abs().max()) > 0    # the snapshots hold the known region at its noise level
    x2, _, _ = N.strided_dynamics(key, model, BETAS, init, K, 0.0, True, samples, mask, order=2, spacing="logsnr")
    assert torch.equal(x, x2)


def test_bf16_infill_walk_with_explicit_draws_against_the_float64_walk():
    import smd_amd.ncsn as N
    C, L, H, Km, B = NETS["small"]
    p, init, taus, _, _, _ = reference("small")
    ocfg, _, model = make(C, L, H, Km)
    g = torch.Generator().manual_seed(9)
    samples = torch.clamp(0.25 * torch.randn(B, 32, C, generator=g), -1, 1)
    mask = (torch.rand(B, 32, C, generator=g) < 0.5).float()
    nz = lambda t: noise((B, 32, C), t, 1)
    with torch.no_grad():
        rx, rc, _ = R.walk(O.make_model(p, ocfg), R.coefficients(BETAS, taus, 2), init.double(), T, mask.double(), samples.double(), nz,
                           collect=R.slots(len(taus)))
    x, coll, _ = N.strided_dynamics(N.PRNGKey(0), model, BETAS, init, K, 0.0, True, samples, mask, infill_noises=nz, order=2,
                                    spacing="logsnr")
    assert model.sampler_arrangement["rng"] == "explicit"
    e = worst_rel(x, coll, rx, rc)
    print(f"[bf16 multistep infill walk small K={K} B={B}] worst rel-L2 of state + snapshots against float64: {e:.3e}")
    tol = 1.5 * BF16_MEASURED["small_infill"]
    assert tol < 5e-2
    assert e < tol
    assert torch.equal(x[mask.cuda().bool()], samples.cuda()[mask.bool()])


# ------------------------------------------------------------------ footprint
def test_multistep_step_writes_only_its_outputs():
    """smd_engine_multistep_step with every caller-side buffer in a guarded arena: it writes the state, the history, the planned
    collection slot, its metric row and the timestep (the bf16 copy with its padding columns at C = 42 and the arrival counter
    live in the workspace, an arena of exactly smd_engine_workspace_bytes()); tables and infill arrays are read only, under both
    sentinels."""
    import smd_amd.lib as lib
    from smd_amd.engine import Engine, NetConfig
    B, C = 3, 42
    L = lib.get_lib()
    P = lambda t: t.data_ptr()
    st = lambda: torch.cuda.current_stream().cuda_stream
    dev = torch.device("cuda:0")
    eng = Engine(NetConfig(data_channels=C, num_layers=2, num_heads=8, num_mlp_layers=1, num_timesteps=T), "cuda:0")
    eng.init_params(0)
    eng.set_schedule(BETAS, with_sampler=True)
    h = eng.h
    taus = logsnr_taus()
    coef_np, plan_np = tables(2, taus)
    g = torch.Generator().manual_seed(4)
    x0, iz = (torch.randn(B, 32, C, generator=g) for _ in range(2))
    hist0 = torch.clamp(0.5 * torch.randn(B, 32, C, generator=g), -1, 1)
    samples, masks = torch.clamp(0.25 * torch.randn(B, 32, C, generator=g), -1, 1), (torch.rand(B, 32, C, generator=g) < 0.5).float()
    t = int(taus[2])
    slot = int(plan_np[t, 2])
    assert 0 < slot <= 40 and coef_np[t, 8] != 0
    results = []
    for fill in F.PATTERNS:
        guard = lambda src: F.guarded_like(src, dev, fill=fill)
        ins = [guard(v) for v in (torch.from_numpy(coef_np), torch.from_numpy(plan_np), iz, samples, masks)]
        (coef, _), (plan, _), (izd, _), (sd, _), (md, _) = ins
        snaps = [hh.snapshot() for _, hh in ins]
        ws_bytes = int(L.smd_engine_workspace_bytes(h, B, 0))
        ws, ws_h = F.guarded((ws_bytes,), torch.uint8, dev, fill=fill)
        lib.check(L.smd_engine_bind_workspace(h, P(ws), ws_bytes, B, 0, st()), "bind_workspace")
        lib.check(L.smd_engine_prepare_sampler(h, st()), "prepare_sampler")
        x, x_h = guard(x0)
        hist, hist_h = guard(hist0)
        t_ptr, t_h = guard(torch.tensor([t], dtype=torch.int32))
        mp, mp_h = F.guarded((T, B, 3), torch.float32, dev, fill=fill)
        coll, coll_h = F.guarded((41, B, 32, C), torch.float32, dev, fill=fill)
        io = lib.SampleIO()
        io.x, io.t_ptr = P(x), P(t_ptr)
        io.infill_samples, io.infill_masks, io.infill_z_in = P(sd), P(md), P(izd)
        io.metrics_partial, io.collection = P(mp), P(coll)
        sp = lib.MultistepPlan()
        sp.coef, sp.plan, sp.T = P(coef), P(plan), T
        lib.check(L.smd_engine_load_state(h, P(x), st()), "load_state")
        lib.check(L.smd_engine_multistep_step(h, ctypes.byref(io), ctypes.byref(sp), P(hist), 0, st()), "multistep_step")
        torch.cuda.synchronize()
        for name, hh in (("workspace", ws_h), ("x", x_h), ("history", hist_h), ("t", t_h), ("metrics_partial", mp_h), ("collection", coll_h)):
            hh.assert_untouched(name)
        for (_, hh), snap in zip(ins, snaps):
            hh.assert_same(snap, "input")
        word = torch.from_numpy(np.array([fill | fill << 16], np.uint32).view(np.int32)).to(dev)
        poison = lambda v: bool((v.contiguous().view(torch.int32) == word).all())
        assert int(t_ptr.item()) == int(plan_np[t, 0])
        rows_poison = (mp.contiguous().view(torch.int32).view(T, -1) == word).all(dim=1)
        assert bool(rows_poison[:t].all()) and bool(rows_poison[t + 1:].all()) and bool(torch.isfinite(mp[t]).all())
        assert all(poison(coll[k]) for k in range(41) if k != slot) and torch.equal(coll[slot], x)
        assert bool(torch.isfinite(hist).all()) and float(hist.abs().max()) <= 1.0 and not torch.equal(hist.cpu(), hist0)
        results.append((x.clone().cpu(), hist.clone().cpu(), mp[t].clone().cpu()))
    assert all(torch.equal(u, v) for u, v in zip(results[0], results[1]))
    assert bool(torch.isfinite(results[0][0]).all())
    # argument checks: the plan's T, null tables, null history, the part
    bad = lib.MultistepPlan()
    bad.coef, bad.plan, bad.T = P(coef), P(plan), T - 1
    call = lambda pl, hp, part: lib.check(L.smd_engine_multistep_step(h, ctypes.byref(io), ctypes.byref(pl), hp, part, st()), "multistep_step")
    with pytest.raises(ValueError, match="timesteps"):
        call(bad, P(hist), 0)
    bad.T, bad.plan = T, None
    with pytest.raises(ValueError, match="null"):
        call(bad, P(hist), 0)
    with pytest.raises(ValueError, match="null history"):
        call(sp, None, 0)
    with pytest.raises(ValueError, match="part"):
        call(sp, P(hist), 3)
    del eng
