"""The strided (DDIM) sampler and its inversion on the GPU: the fused update alone against float64, fp32 and bf16 walks against
the float64 walks of tests/_strided_ref.py, the graph / two-chain arrangements, the graph cache next to diffusion_dynamics',
jax.random streams and the footprint of smd_engine_strided_step.

Bounds.  The update alone: |err| <= 4 * 2^-23 * (|a x0| + |b x| + |sigma z| + |y|) + 1e-12 per element.  fp32 walks: 4 x g32, the
float32 CPU walk of _strided_ref against its float64 walk (DESIGN.md section 13's rule).  bf16 walks, eta = 1: the 1.5e-2 of
tests/test_gpu_full_walk.py; eta = 0: measured on an MI355X x 1.5 (ETA0_TOL below).
"""
import ctypes

import numpy as np
import pytest
import torch

import _footprint as F
import _strided_ref as R
import ddpm_oracle as O
from test_gpu_full_walk import BETAS, make, rel

pytestmark = pytest.mark.gpu
T = 1000
K = 20
# bf16 walks at eta = 0 against float64, rel-L2, worst of final state and snapshots: measured (small, base) x 1.5
ETA0_MEASURED = {"small": 6.81e-3, "base": 6.69e-3}      # (eta = 1 on the same walks: 6.15e-3, 7.38e-3)


def noise(shape, t, stream=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(100_000 + 7919 * stream + t))


def dense_model(C=512):
    import smd_amd.ncsn as N
    from smd_amd.engine import NetConfig
    return N.Model(NetConfig(architecture="DenseDDPM", data_channels=C, num_layers=3, num_heads=8, num_mlp_layers=2, num_timesteps=T),
                   "cuda:0", seed=0)


def transformer_model(C):
    import smd_amd.ncsn as N
    from smd_amd.engine import NetConfig
    return N.Model(NetConfig(data_channels=C, num_layers=2, num_heads=8, num_mlp_layers=1, num_timesteps=T), "cuda:0", seed=0)


def find_bf16_input(eng, x):
    """byte offset in the handle's workspace of its bf16 network input: where load_state(x) left bf16(x), zero padded"""
    C, Cp = eng.C, int(eng.L.smd_engine_padded_channels(eng.h))
    rows = x.reshape(-1, C)
    img = torch.zeros((rows.shape[0], Cp), dtype=torch.bfloat16, device=x.device)
    img[:, :C] = rows.to(torch.bfloat16)
    want = img.view(torch.uint8).reshape(-1)
    ws = eng.workspace
    base = (-ws.data_ptr()) % 256
    n = (ws.numel() - base - want.numel()) // 256 + 1
    head = ws[base:base + n * 256].view(n, 256)[:, :64]
    cand = torch.nonzero((head == want[:64]).all(dim=1)).flatten().tolist()
    hits = [base + 256 * i for i in cand if torch.equal(ws[base + 256 * i:base + 256 * i + want.numel()], want)]
    assert len(hits) == 1, hits
    return hits[0], want.numel(), (rows.shape[0], Cp)


def partials64(v, S):
    """metrics_partial of one launch for v (B, S, C) or (B, C) in float64: (B,)"""
    sq = torch.sqrt((v.double() ** 2).sum(dim=1) + 1e-10)
    return sq.sum(dim=1) if S > 1 else sq


# the last three rows: VEC = 1 with one row group; two trips of the column loop, the last with 18 live threads (VEC = 1) and
# with one live thread (VEC = 4)
@pytest.mark.parametrize("arch,B,C", [("transformer", 3, 42), ("transformer", 3, 512), ("dense", 5, 512),
                                      ("dense", 5, 42), ("transformer", 3, 146), ("dense", 3, 1028)])
def test_fused_update_alone_against_float64(arch, B, C):
    """One launch at a time on random x, z, masks: the network's own eps_hat is read back and the update is recomputed in
    float64 from the float32 tables the kernel read.  C = 42: VEC = 1 and a masked last column block; C = 512: VEC = 4;
    DenseDDPM: one row group and channel-axis norms."""
    import smd_amd.lib as lib
    import smd_amd.schedule as S
    model = transformer_model(C) if arch == "transformer" else dense_model(C)
    eng = model.engine
    Sq = eng.S
    shape = (B, Sq, C) if Sq > 1 else (B, C)
    dev = eng.device
    eng.set_schedule(BETAS, with_sampler=True)
    eng.bind(B, training=False)
    eng.prepare_sampler()
    taus = S.stride_timesteps(T, K)
    g = torch.Generator().manual_seed(11)
    samples = torch.clamp(0.25 * torch.randn(*shape, generator=g), -1, 1).to(dev)
    masks = (torch.rand(*shape, generator=g) < 0.5).float().to(dev)
    located = None
    worst = 0.0
    for eta in (0.0, 0.7):
        for clip in (1.0, float("inf")):
            coef, plan = S.strided_coefficient_table(BETAS, taus, eta, clip)
            coef_d, plan_d = torch.from_numpy(coef).to(dev), torch.from_numpy(plan).to(dev)
            sp = lib.StridePlan()
            sp.coef, sp.plan, sp.T = coef_d.data_ptr(), plan_d.data_ptr(), T
            for j in (0, K // 2, K - 1):
                t = int(taus[j])
                for infill in (False, True):
                    x = (torch.randn(*shape, generator=g) * (1.0 if j < K - 1 else 0.5)).to(dev)
                    z, iz = torch.randn(*shape, generator=g).to(dev), torch.randn(*shape, generator=g).to(dev)
                    x_in = x.clone()
                    t_ptr = torch.tensor([t], dtype=torch.int32, device=dev)
                    mp = torch.zeros((T, B, 3), device=dev)
                    coll = torch.full((41, *shape), 7.0, device=dev)
                    io = lib.SampleIO()
                    io.x, io.t_ptr, io.z_in = x.data_ptr(), t_ptr.data_ptr(), z.data_ptr()
                    io.metrics_partial, io.collection = mp.data_ptr(), coll.data_ptr()
                    if infill:
                        io.infill_samples, io.infill_masks, io.infill_z_in = samples.data_ptr(), masks.data_ptr(), iz.data_ptr()
                    eng.load_state(x)
                    if located is None:
                        torch.cuda.synchronize()
                        located = find_bf16_input(eng, x)
                    eng.strided_step(io, sp)
                    torch.cuda.synchronize()
                    eh = eng.last_pred().clone()
                    row = dict(zip(("sqrt_recip", "sqrt_m1", "a", "b", "sigma", "clip", "sqrt_as", "sqrt_1m_as"), (float(v) for v in coef[t])))
                    row.update(t=t, next_t=int(plan[t, 0]))
                    d = lambda v: v.double().cpu()
                    ref, x0, y = R.update(d(x_in), d(eh), d(z), row, T, d(masks) if infill else None, d(samples), d(iz))
                    mag = (row["a"] * x0).abs() + (row["b"] * d(x_in)).abs() + (row["sigma"] * d(z)).abs() + (y.abs() if infill else 0)
                    err = (d(x) - ref).abs()
                    ratio = float((err / (4 * 2.0 ** -23 * mag + 1e-12)).max())
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, (eta, clip, t, infill, ratio)
                    # bf16 copy: round-to-nearest of the fp32 state, padding zero
                    off, nbytes, (rows, Cp) = located
                    xb = eng.workspace[off:off + nbytes].view(torch.bfloat16).view(rows, Cp)
                    assert torch.equal(xb[:, :C], x.reshape(rows, C).to(torch.bfloat16)) and not bool(xb[:, C:].any())
                    assert int(t_ptr.item()) == int(plan[t, 0])
                    # metric partials: row t only
                    want = torch.stack([partials64(d(eh), Sq), partials64(d(x_in) - ref, Sq), partials64(row["sigma"] * d(z), Sq)], dim=1)
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
                before = [v.clone() for v in (x, mp, coll, eng.workspace[off:off + nbytes])]
                eng.strided_step(io, sp)
                torch.cuda.synchronize()
                for u, v in zip(before, (x, mp, coll, eng.workspace[off:off + nbytes])):
                    assert torch.equal(u.view(torch.uint8), v.view(torch.uint8))
                assert int(t_ptr.item()) == t_end
    print(f"[{arch} B={B} C={C}] fused strided update: worst |err| / bound = {worst:.3f}")
    if C % 4 == 0:                                                     # 16-byte loads: a state 4 bytes off is refused
        io.x = x.data_ptr() + 4
        t_ptr.fill_(int(taus[0]))
        with pytest.raises(ValueError, match="16-byte aligned"):
            eng.strided_step(io, sp)
        torch.cuda.synchronize()
        assert int(t_ptr.item()) == int(taus[0])


# ------------------------------------------------------------------ walks
def reference_walks(p, ocfg, co, init, noises, collect=None, masks=None, samples=None, infill_noises=None):
    """(float64 walk, float32 walk) of _strided_ref on the CPU oracle's network"""
    out = []
    with torch.no_grad():
        for dt in (torch.float64, torch.float32):
            m = O.make_model({k: v.to(dt) for k, v in p.items()}, ocfg)
            out.append(R.walk(m, co, init.to(dt), T, noises, masks, samples, infill_noises, collect))
    return out


def worst_rel(x, coll, rx, rcoll):
    return max([rel(x, rx)] + [rel(coll[k], v) for k, v in rcoll.items()])


@pytest.fixture(scope="module")
def small32():
    return make(42, 2, 8, 1, dtype="fp32")


@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_fp32_walk_against_the_float64_walk(small32, eta):
    import smd_amd.ncsn as N
    ocfg, p, model = small32
    B, C = 5, 42
    init = torch.randn(B, 32, C, generator=torch.Generator().manual_seed(31))
    nz = lambda t: noise((B, 32, C), t)
    co = R.descending(BETAS, R.timesteps(T, K), eta)
    (rx, rc, rm), (fx, fc, fm) = reference_walks(p, ocfg, co, init, nz, collect=R.slots(K))
    g_state, g_met = worst_rel(fx, fc, rx, rc), max(rel(fm[i], rm[i]) for i in (0, 1, 3))
    x, coll, met = N.strided_dynamics(N.PRNGKey(0), model, BETAS, init, K, eta, noises=nz)
    assert tuple(coll.shape) == (41, B, 32, C) and tuple(met.shape) == (4, K, 1)
    written = sorted(k for k in range(1, 41) if float(coll[k].abs().max()) > 0)
    assert written == sorted(rc) and torch.equal(coll[0].cpu(), init)
    e_state = worst_rel(x, coll, rx, rc)
    m = met[:, :, 0].cpu().double()
    e_met = max(rel(m[i], rm[i]) for i in (0, 1, 3))
    print(f"[fp32 strided walk K={K} eta={eta}] g32: state {g_state:.3e} metrics {g_met:.3e} | GPU: state + snapshots {e_state:.3e} "
          f"(ratio {e_state / g_state:.2f}), metric rows {e_met:.3e} (ratio {e_met / g_met:.2f})")
    assert e_state <= 4 * g_state
    assert e_met <= 4 * g_met
    assert rel(m[2], rm[2]) < 1e-6                                     # the alpha row is table data
    # batch invariance: the first three rows walked alone
    x3, c3, _ = N.strided_dynamics(N.PRNGKey(0), model, BETAS, init[:3], K, eta, noises=lambda t: nz(t)[:3])
    assert torch.equal(x3, x[:3]) and torch.equal(c3, coll[:, :3])
    if eta == 0.0:                                                     # deterministic: the key is never used
        a = N.strided_dynamics(N.PRNGKey(1), model, BETAS, init, K, 0.0)
        b = N.strided_dynamics(N.PRNGKey(2), model, BETAS, init, K, 0.0)
        assert all(torch.equal(u, v) for u, v in zip(a, b))
        assert float(b[2][3].max()) == pytest.approx(1e-5, rel=1e-3)   # no noise was drawn: the norm of zeros


def test_fp32_ddim_encode_against_the_float64_walk(small32):
    import smd_amd.ncsn as N
    ocfg, p, model = small32
    B, C = 3, 42
    x0 = torch.clamp(0.25 * torch.randn(B, 32, C, generator=torch.Generator().manual_seed(32)), -1, 1)
    co = R.ascending(BETAS, R.timesteps(T, K))
    (rx, _, _), (fx, _, _) = reference_walks(p, ocfg, co, x0, None)
    g32 = rel(fx, rx)
    z = N.ddim_encode(model, BETAS, x0, K)
    e = rel(z, rx)
    back, _, _ = N.strided_dynamics(N.PRNGKey(0), model, BETAS, z, K, 0.0)
    print(f"[fp32 ddim_encode K={K}] g32 {g32:.3e} | GPU {e:.3e} (ratio {e / g32:.2f}); latent std {float(z.std()):.3f}; "
          f"encode -> decode round trip rel-L2 {rel(back, x0):.3e} (a property of the model, not asserted)")
    assert e <= 4 * g32
    assert torch.equal(z, N.ddim_encode(model, BETAS, x0, K, use_graph=False))
    assert model.sampler_arrangement["chains"] == 1 and model.sampler_arrangement["iterations"] == K - 1


@pytest.mark.parametrize("name,C,L,H,Km,B", [("small", 42, 2, 8, 1, 4), ("base", 512, 6, 8, 2, 2)])
def test_bf16_walks_against_the_float64_walk(name, C, L, H, Km, B):
    import smd_amd.ncsn as N
    ocfg, p, model = make(C, L, H, Km)
    init = torch.randn(B, 32, C, generator=torch.Generator().manual_seed(33))
    nz = lambda t: noise((B, 32, C), t)
    res = {}
    for eta in (1.0, 0.0):
        co = R.descending(BETAS, R.timesteps(T, K), eta)
        with torch.no_grad():
            rx, rc, _ = R.walk(O.make_model(p, ocfg), co, init.double(), T, nz, collect=R.slots(K))
        x, coll, _ = N.strided_dynamics(N.PRNGKey(0), model, BETAS, init, K, eta, noises=nz if eta else None, use_graph=False)
        res[eta] = worst_rel(x, coll, rx, rc)
    print(f"[bf16 strided walk {name} K={K} B={B}] worst rel-L2 of state + snapshots against float64: eta=1 {res[1.0]:.3e}, eta=0 {res[0.0]:.3e}")
    assert res[1.0] < 1.5e-2
    tol0 = 1.5 * ETA0_MEASURED[name]
    assert tol0 < 5e-2
    assert res[0.0] < tol0


# ------------------------------------------------------------------ arrangements
def test_graph_replay_equals_eager_bitwise():
    import smd_amd.ncsn as N
    _, _, model = make(42, 2, 8, 1)
    init = torch.randn(4, 32, 42, generator=torch.Generator().manual_seed(5))
    a = N.strided_dynamics(N.PRNGKey(9), model, BETAS, init, K, 0.5, use_graph=True)
    assert model.sampler_arrangement["graphed"] and model.sampler_arrangement["chains"] == 1
    b = N.strided_dynamics(N.PRNGKey(9), model, BETAS, init, K, 0.5, use_graph=False)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert float(a[2][3, :-1].min()) > 1e-3                            # noise was drawn on every iteration but the last


@pytest.mark.parametrize("infill", [False, True])
def test_two_chain_walk_equals_one_chain_and_eager(infill, monkeypatch):
    """B = 136 walks as 72 + 64 pipelined chains: K = 20 is 19 replays, two graphs of 8 iterations and 3 as plain launches.
    The comparison and tolerance of tests/test_gpu_engine.py test_two_chain_sampler_equals_one_chain_and_eager."""
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
        out = N.strided_dynamics(N.PRNGKey(5), model, BETAS, init, K, 1.0, use_graph=graph, **kw)
        return out, dict(model.sampler_arrangement)

    (x2, c2, m2), arr = walk(2, True)
    assert arr["chain_sizes"] == [72, 64] and arr["pipelined_unroll"] == 8 and arr["padded"] == 0
    (x1, c1, m1), arr1 = walk(1, True)
    (xe, ce, me), _ = walk(1, False)
    assert arr1["chains"] == 1
    assert torch.equal(x1, xe) and torch.equal(c1, ce) and torch.equal(m1, me)      # one chain: replay == eager, bitwise
    slots = [s for s in R.slots(K) if s >= 0]
    assert torch.equal(c2[0], c1[0]) and all(float(c2[s].abs().max()) > 0 for s in slots)
    assert rel(x2, x1) < 5e-3, rel(x2, x1)
    assert all(rel(c2[s], c1[s]) < 5e-3 for s in slots)
    assert rel(m2[0], m1[0]) < 5e-3 and rel(m2[1], m1[1]) < 5e-3 and rel(m2[3], m1[3]) < 5e-3
    assert torch.equal(m2[2], m1[2])
    assert float((x2[72:] - init[72:].cuda()).abs().max()) > 0
    if infill:
        m = kw["infill_masks"].cuda().bool()
        assert torch.equal(x2[m], kw["infill_samples"].cuda()[m])                    # the last iteration returns the template


def test_graph_cache_across_seeds_steps_and_eta():
    import smd_amd.ncsn as N
    init = torch.randn(4, 32, 42, generator=torch.Generator().manual_seed(6))
    calls = [(1, K, 0.0), (2, 12, 0.5), (3, 12, 0.5), (4, K, 0.5)]
    _, _, model = make(42, 2, 8, 1)
    got, reused = [], []
    for seed, k, eta in calls:
        before = model.__dict__.get("_sampler_graphs", {}).get("strided")
        got.append(N.strided_dynamics(N.PRNGKey(seed), model, BETAS, init, k, eta))
        reused.append(model._sampler_graphs["strided"] is before)
    assert reused == [False, False, True, False]                      # the key carries (K, eta); another seed reuses the graphs
    for (seed, k, eta), out in zip(calls[1:], got[1:]):
        _, _, fresh = make(42, 2, 8, 1)
        want = N.strided_dynamics(N.PRNGKey(seed), fresh, BETAS, init, k, eta)
        assert all(torch.equal(u, v) for u, v in zip(out, want)), (seed, k, eta)


def test_strided_and_every_step_walks_do_not_disturb_each_other():
    import smd_amd.ncsn as N
    init = torch.randn(4, 32, 42, generator=torch.Generator().manual_seed(7))
    dd = lambda m, seed: N.diffusion_dynamics(N.PRNGKey(seed), m, BETAS, init, t_stop=985)
    sd = lambda m, seed: N.strided_dynamics(N.PRNGKey(seed), m, BETAS, init, K, 1.0)
    _, _, alone = make(42, 2, 8, 1)
    want_dd = [dd(alone, 1), dd(alone, 2)]
    _, _, alone = make(42, 2, 8, 1)
    want_sd = [sd(alone, 1), sd(alone, 2)]
    _, _, model = make(42, 2, 8, 1)
    got = [sd(model, 1), dd(model, 1), sd(model, 2), dd(model, 2)]
    assert set(model._sampler_graphs) == {"entry", "strided"}
    for out, want in zip(got, (want_sd[0], want_dd[0], want_sd[1], want_dd[1])):
        assert all(torch.equal(u, v) for u, v in zip(out, want))


def test_threefry_noise_of_iteration_j_is_normal_of_key_row_j():
    """jax.random streams: the update of iteration j draws jax.random.normal(noise key row j) for its rows of the global array;
    here the rows come from jax_random.normal on the host side and go in as explicit draws."""
    import smd_amd.jax_random as J
    import smd_amd.ncsn as N
    import smd_amd.schedule as S
    _, _, model = make(42, 2, 8, 1)
    B, k = 4, 4
    init = torch.randn(B, 32, 42, generator=torch.Generator().manual_seed(8))
    key = J.PRNGKey(3)
    a = N.strided_dynamics(key, model, BETAS, init, k, 1.0)
    assert model.sampler_arrangement["rng"] == "threefry"
    _, nk = J.sampler_key_tables(key, k)
    taus = [int(t) for t in S.stride_timesteps(T, k)]
    draws = {t: J.normal(J.ThreefryKey(int(nk[j][0]), int(nk[j][1])), (B, 32, 42), "cuda:0") for j, t in enumerate(taus)}
    b = N.strided_dynamics(N.PRNGKey(0), model, BETAS, init, k, 1.0, noises=lambda t: draws[t])
    assert rel(a[2][3], b[2][3]) < 1e-6          # the noise norm of iteration j depends on nothing but sigma_j z_j: row j's key
    # ... and the state after one iteration (K = 2 collects it in row 40), to the rounding of one normal
    a2 = N.strided_dynamics(key, model, BETAS, init, 2, 1.0)
    _, nk2 = J.sampler_key_tables(key, 2)
    z0 = J.normal(J.ThreefryKey(int(nk2[0][0]), int(nk2[0][1])), (B, 32, 42), "cuda:0")
    b2 = N.strided_dynamics(N.PRNGKey(0), model, BETAS, init, 2, 1.0, noises=lambda t: z0)
    assert float(a2[1][40].abs().max()) > 0 and float((a2[1][40] - b2[1][40]).abs().max()) <= 1e-6


# ------------------------------------------------------------------ footprint
def test_strided_step_writes_only_its_outputs():
    """smd_engine_strided_step with every caller-side buffer in a guarded arena: it writes the state, the planned collection
    slot, its metric row and the timestep (the bf16 copy and the arrival counter live in the workspace, an arena of exactly
    smd_engine_workspace_bytes()); tables, draws and infill arrays are read only, under both sentinels."""
    import smd_amd.lib as lib
    import smd_amd.schedule as S
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
    taus = S.stride_timesteps(T, K)
    coef_np, plan_np = S.strided_coefficient_table(BETAS, taus, 0.7)
    g = torch.Generator().manual_seed(4)
    x0, z, iz = (torch.randn(B, 32, C, generator=g) for _ in range(3))
    samples, masks = torch.clamp(0.25 * torch.randn(B, 32, C, generator=g), -1, 1), (torch.rand(B, 32, C, generator=g) < 0.5).float()
    t = int(taus[1])
    slot = int(plan_np[t, 2])
    assert 0 < slot <= 40
    results = []
    for fill in F.PATTERNS:
        guard = lambda src: F.guarded_like(src, dev, fill=fill)
        ins = [guard(v) for v in (torch.from_numpy(coef_np), torch.from_numpy(plan_np), z, iz, samples, masks)]
        (coef, _), (plan, _), (zd, _), (izd, _), (sd, _), (md, _) = ins
        snaps = [hh.snapshot() for _, hh in ins]
        ws_bytes = int(L.smd_engine_workspace_bytes(h, B, 0))
        ws, ws_h = F.guarded((ws_bytes,), torch.uint8, dev, fill=fill)
        lib.check(L.smd_engine_bind_workspace(h, P(ws), ws_bytes, B, 0, st()), "bind_workspace")
        lib.check(L.smd_engine_prepare_sampler(h, st()), "prepare_sampler")
        x, x_h = guard(x0)
        t_ptr, t_h = guard(torch.tensor([t], dtype=torch.int32))
        mp, mp_h = F.guarded((T, B, 3), torch.float32, dev, fill=fill)
        coll, coll_h = F.guarded((41, B, 32, C), torch.float32, dev, fill=fill)
        io = lib.SampleIO()
        io.x, io.t_ptr, io.z_in = P(x), P(t_ptr), P(zd)
        io.infill_samples, io.infill_masks, io.infill_z_in = P(sd), P(md), P(izd)
        io.metrics_partial, io.collection = P(mp), P(coll)
        sp = lib.StridePlan()
        sp.coef, sp.plan, sp.T = P(coef), P(plan), T
        lib.check(L.smd_engine_load_state(h, P(x), st()), "load_state")
        lib.check(L.smd_engine_strided_step(h, ctypes.byref(io), ctypes.byref(sp), 0, st()), "strided_step")
        torch.cuda.synchronize()
        for name, hh in (("workspace", ws_h), ("x", x_h), ("t", t_h), ("metrics_partial", mp_h), ("collection", coll_h)):
            hh.assert_untouched(name)
        for (_, hh), snap in zip(ins, snaps):
            hh.assert_same(snap, "input")
        word = torch.from_numpy(np.array([fill | fill << 16], np.uint32).view(np.int32)).to(dev)
        poison = lambda v: bool((v.contiguous().view(torch.int32) == word).all())
        assert int(t_ptr.item()) == int(plan_np[t, 0])
        rows_poison = (mp.contiguous().view(torch.int32).view(T, -1) == word).all(dim=1)
        assert bool(rows_poison[:t].all()) and bool(rows_poison[t + 1:].all()) and bool(torch.isfinite(mp[t]).all())
        assert all(poison(coll[k]) for k in range(41) if k != slot) and torch.equal(coll[slot], x)
        results.append((x.clone().cpu(), mp[t].clone().cpu()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    assert bool(torch.isfinite(results[0][0]).all())
    # argument checks: the plan's T, null tables, the part
    bad = lib.StridePlan()
    bad.coef, bad.plan, bad.T = P(coef), P(plan), T - 1
    with pytest.raises(ValueError, match="timesteps"):
        lib.check(L.smd_engine_strided_step(h, ctypes.byref(io), ctypes.byref(bad), 0, st()), "strided_step")
    bad.T, bad.plan = T, None
    with pytest.raises(ValueError, match="null"):
        lib.check(L.smd_engine_strided_step(h, ctypes.byref(io), ctypes.byref(bad), 0, st()), "strided_step")
    with pytest.raises(ValueError, match="part"):
        lib.check(L.smd_engine_strided_step(h, ctypes.byref(io), ctypes.byref(sp), 3, st()), "strided_step")
    del eng
