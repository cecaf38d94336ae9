"""The walks of the analytic reverse variance on the GPU: the estimator of E[eps_hat^2] and the
element-mode sampler against the float64 restatements of tests/_analytic_ref.py on the CPU oracle's network, and the graph
arrangements.

Bounds.  fp32: 4 x g32, the float32 CPU computation against its float64 twin (section 13's rule).  bf16: measured on an MI355X
against the float64 reference, asserted at 1.5 x the measured value (sections 16 and 17's convention); the figures are the
named constants below.
"""
import numpy as np
import pytest
import torch

import _analytic_ref as A
import _strided_ref as R
import ddpm_oracle as O
from test_gpu_full_walk import BETAS, make, rel
from test_gpu_strided import noise

pytestmark = pytest.mark.gpu
T = 1000
K = 20
# bf16 against float64, measured on an MI355X (small transformer L = 2; DenseDDPM L = 3, C = 512):
G_BF16_MEASURED = {"transformer": 5.80e-3, "dense": 6.94e-3}      # worst rel-L2 over the timesteps of g_t
G_FP8_MEASURED = 5.80e-3           # the small transformer under "fp8": the bf16 figure (its 64-row GEMMs take no e4m3 tile)
WALK_BF16_MEASURED = 5.92e-3                                      # element-mode walk K = 20: rel-L2 of the final state and snapshots


def _examples(shape, seed):
    return torch.clamp(0.25 * torch.randn(*shape, generator=torch.Generator().manual_seed(seed)), -1, 1)


def _worst_rel(g, ref):
    return max(rel(g[k], ref[k]) for k in range(len(ref)))


def _reference_g(p, ocfg, x0, ts, eps_of):
    m64 = O.make_model(p, ocfg)
    m32 = O.make_model({k: v.float() for k, v in p.items()}, ocfg)
    return A.estimate(m64, BETAS, x0, ts, eps_of, torch.float64), A.estimate(m32, BETAS, x0, ts, eps_of, torch.float32)


def _dense(dtype):
    """DenseDDPM (L = 3, C = 512) of tests/test_gpu_strided.py in the engine dtype ``dtype`` with its oracle twin"""
    import smd_amd.ncsn as N
    from smd_amd.engine import NetConfig
    model = N.Model(NetConfig(architecture="DenseDDPM", data_channels=512, num_layers=3, num_heads=8, num_mlp_layers=2, num_timesteps=T,
                              dtype=dtype), "cuda:0", seed=0)
    ocfg = O.NetConfig(architecture="DenseDDPM", data_channels=512, num_layers=3, num_heads=8, num_mlp_layers=2)
    p = {k: v.double().cpu() for k, v in model.engine.named_views().items()}
    return ocfg, p, model


@pytest.mark.parametrize("arch", ["transformer", "dense"])
def test_estimator_fp32_against_float64(arch):
    import smd_amd.ncsn as N
    if arch == "transformer":
        ocfg, p, model = make(42, 2, 8, 1, dtype="fp32")
        shape = (5, 32, 42)
    else:
        ocfg, p, model = _dense("fp32")
        shape = (5, 512)
    x0 = _examples(shape, 41)
    ts = sorted(R.timesteps(T, 8))
    eps_of = lambda t: noise(shape, t, stream=3)
    g64, g32 = _reference_g(p, ocfg, x0, ts, eps_of)
    g, count = N.estimate_score_moments(model, BETAS, x0, ts, eps_in=lambda r, t: eps_of(t))
    assert g.shape == (8, *shape[1:]) and g.dtype == np.float64 and count == 5
    e, e32 = _worst_rel(g, g64), _worst_rel(g32, g64)
    print(f"[estimator fp32 {arch}] g32 {e32:.3e} | GPU {e:.3e} (ratio {e / e32:.2f})")
    assert e <= 4 * e32
    # batches of 2 + 2 + 1 add up to the same estimate (float64 accumulation of fp32 sums over other chunkings: not bitwise)
    gb, _ = N.estimate_score_moments(model, BETAS, x0, ts, eps_in=lambda r, t: eps_of(t), batch=2)
    assert _worst_rel(gb, g) <= 1e-6


def test_estimator_fp8_against_float64():
    """the estimator walk under the engine option "fp8" (e4m3 operands in the wide GEMMs): measured, asserted at 1.5 x"""
    import smd_amd.ncsn as N
    ocfg, p, model = make(42, 2, 8, 1, dtype="fp8")
    shape = (4, 32, 42)
    x0 = _examples(shape, 43)
    ts = sorted(R.timesteps(T, 8))
    eps_of = lambda t: noise(shape, t, stream=4)
    g64 = A.estimate(O.make_model(p, ocfg), BETAS, x0, ts, eps_of, torch.float64)
    g, _ = N.estimate_score_moments(model, BETAS, x0, ts, eps_in=lambda r, t: eps_of(t))
    e = _worst_rel(g, g64)
    print(f"[estimator fp8 transformer] worst rel-L2 of g_t against float64: {e:.3e} (asserted at 1.5 x {G_FP8_MEASURED:.2e})")
    assert e <= 1.5 * G_FP8_MEASURED
    a, _ = N.estimate_score_moments(model, BETAS, x0, ts, rng=N.PRNGKey(7))
    b, _ = N.estimate_score_moments(model, BETAS, x0, ts, rng=N.PRNGKey(7))
    assert np.array_equal(a, b)                                         # the graph-replayed walk, twice


@pytest.mark.parametrize("arch", ["transformer", "dense"])
def test_estimator_bf16_against_float64(arch):
    import smd_amd.ncsn as N
    if arch == "transformer":
        ocfg, p, model = make(42, 2, 8, 1)
        shape = (4, 32, 42)
    else:
        ocfg, p, model = _dense("bf16")
        shape = (4, 512)
    x0 = _examples(shape, 43)
    ts = sorted(R.timesteps(T, 8))
    eps_of = lambda t: noise(shape, t, stream=4)
    g64 = A.estimate(O.make_model(p, ocfg), BETAS, x0, ts, eps_of, torch.float64)
    g, count = N.estimate_score_moments(model, BETAS, x0, ts, eps_in=lambda r, t: eps_of(t))
    e = _worst_rel(g, g64)
    print(f"[estimator bf16 {arch}] worst rel-L2 of g_t against float64: {e:.3e} (asserted at 1.5 x {G_BF16_MEASURED[arch]:.2e})")
    assert e <= 1.5 * G_BF16_MEASURED[arch]


def test_estimator_is_repeatable_and_graph_equals_eager():
    import smd_amd.ncsn as N
    _, _, model = make(42, 2, 8, 1)
    x0 = _examples((19, 32, 42), 45)
    ts = R.timesteps(T, 8)
    a, ca = N.estimate_score_moments(model, BETAS, x0, ts, draws=2, rng=N.PRNGKey(7), batch=19)
    b, _ = N.estimate_score_moments(model, BETAS, x0, ts, draws=2, rng=N.PRNGKey(7), batch=19)
    c, _ = N.estimate_score_moments(model, BETAS, x0, ts, draws=2, rng=N.PRNGKey(7), batch=19, use_graph=False)
    d, _ = N.estimate_score_moments(model, BETAS, x0, ts, draws=2, rng=N.PRNGKey(8), batch=19)
    assert ca == 38 and np.array_equal(a, b) and np.array_equal(a, c) and not np.array_equal(a, d)
    assert 0.0 < float(a.min()) and np.isfinite(a).all()


def _sig_table(shape, taus, eta, seed):
    import smd_amd.schedule as S
    g = np.random.default_rng(seed).uniform(0.2, 0.95, (len(taus), *shape[1:]))
    return g, S.analytic_sigma_table(BETAS, taus, eta, g)


def test_element_walk_fp32_against_the_float64_walk():
    import smd_amd.ncsn as N
    ocfg, p, model = make(42, 2, 8, 1, dtype="fp32")
    B, C = 5, 42
    init = torch.randn(B, 32, C, generator=torch.Generator().manual_seed(31))
    nz = lambda t: noise((B, 32, C), t)
    taus = R.timesteps(T, K)
    g, sig = _sig_table((B, 32, C), taus, 1.0, 51)
    with torch.no_grad():
        rx, rc = A.walk(O.make_model(p, ocfg), BETAS, taus, 1.0, sig, init.double(), nz, T, collect=R.slots(K))
        fx, fc = A.walk(O.make_model({k: v.float() for k, v in p.items()}, ocfg), BETAS, taus, 1.0, sig, init.float(), nz, T, collect=R.slots(K))
    g32 = max([rel(fx, rx)] + [rel(fc[k], rc[k]) for k in rc])
    x, coll, met = N.strided_dynamics(N.PRNGKey(0), model, BETAS, init, K, 1.0, noises=nz, analytic=("element", g))
    e = max([rel(x, rx)] + [rel(coll[k], v) for k, v in rc.items()])
    print(f"[element walk fp32 K={K}] g32 {g32:.3e} | GPU {e:.3e} (ratio {e / g32:.2f})")
    assert e <= 4 * g32
    assert tuple(met.shape) == (4, K, 1) and float(met[3, :-1].min()) > 1e-3 and model.sampler_arrangement["walk"] == "analytic"


def test_element_walk_bf16_against_the_float64_walk():
    import smd_amd.ncsn as N
    ocfg, p, model = make(42, 2, 8, 1)
    B, C = 4, 42
    init = torch.randn(B, 32, C, generator=torch.Generator().manual_seed(33))
    nz = lambda t: noise((B, 32, C), t)
    taus = R.timesteps(T, K)
    g, sig = _sig_table((B, 32, C), taus, 1.0, 52)
    with torch.no_grad():
        rx, rc = A.walk(O.make_model(p, ocfg), BETAS, taus, 1.0, sig, init.double(), nz, T, collect=R.slots(K))
    x, coll, _ = N.strided_dynamics(N.PRNGKey(0), model, BETAS, init, K, 1.0, noises=nz, analytic=("element", g))
    e = max([rel(x, rx)] + [rel(coll[k], v) for k, v in rc.items()])
    print(f"[element walk bf16 K={K}] worst rel-L2 of state + snapshots against float64: {e:.3e} (asserted at 1.5 x {WALK_BF16_MEASURED:.2e})")
    assert e <= 1.5 * WALK_BF16_MEASURED


def test_scalar_mode_is_the_strided_walk_on_a_hand_built_table():
    import smd_amd.ncsn as N
    import smd_amd.schedule as S
    _, _, model = make(42, 2, 8, 1)
    init = torch.randn(4, 32, 42, generator=torch.Generator().manual_seed(5))
    taus = S.stride_timesteps(T, K)
    gs = np.random.default_rng(53).uniform(0.2, 0.95, K)
    a = N.strided_dynamics(N.PRNGKey(9), model, BETAS, init, K, 0.5, analytic=("scalar", gs))
    assert model.sampler_arrangement["walk"] == "strided" and model.sampler_arrangement["graphed"]
    coef, plan = S.strided_coefficient_table(BETAS, taus, 0.5)
    coef[taus, 4] = np.sqrt(A.variance(BETAS, taus, 0.5, gs, clip=1.0)).astype(np.float32)
    model.drop_sampler_cache()
    x, coll, mp = N._strided_walk("strided", N.PRNGKey(9), model, BETAS, init, [int(t) for t in taus], coef, plan, ("hand", K), collect=True)
    assert torch.equal(a[0], x) and torch.equal(a[1], coll)
    # a per-element g that is constant over the elements: the element walk draws the same noise and scales it alike
    ge = np.broadcast_to(gs[:, None, None], (K, 32, 42))
    b = N.strided_dynamics(N.PRNGKey(9), model, BETAS, init, K, 0.5, analytic=("element", ge))
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    # the plain walk differs, and a second key draws other noise
    c = N.strided_dynamics(N.PRNGKey(9), model, BETAS, init, K, 0.5)
    assert not torch.equal(a[0], c[0])
    with pytest.raises(ValueError, match="no noise term"):
        N.strided_dynamics(N.PRNGKey(9), model, BETAS, init, K, 0.0, order=2, spacing="logsnr", analytic=("scalar", gs))
    with pytest.raises(ValueError, match="rows for a walk"):
        N.strided_dynamics(N.PRNGKey(9), model, BETAS, init, K, 0.5, analytic=("scalar", gs[:-1]))


def test_element_walk_arrangements_and_repeatability(monkeypatch):
    """graph replay == eager bitwise on one chain, the same rng twice gives the same bits, and B = 136 as 72 + 64 pipelined
    chains against one chain with the comparison and tolerance of tests/test_gpu_strided.py's two-chain test"""
    import smd_amd.ncsn as N
    _, _, model = make(C=512, L=2, H=8, K=1)
    B = 136
    g = torch.Generator().manual_seed(77)
    init = torch.randn(B, 32, 512, generator=g)
    ge = np.random.default_rng(54).uniform(0.2, 0.95, (K, 32, 512))

    def walk(chains, graph):
        monkeypatch.setenv("SMD_SAMPLER_CHAINS", str(chains))
        out = N.strided_dynamics(N.PRNGKey(5), model, BETAS, init, K, 1.0, use_graph=graph, analytic=("element", ge))
        return out, dict(model.sampler_arrangement)

    (x2, c2, m2), arr = walk(2, True)
    assert arr["chain_sizes"] == [72, 64] and arr["pipelined_unroll"] == 8 and arr["walk"] == "analytic"
    (x2b, c2b, m2b), _ = walk(2, True)                                  # the cached graphs, the same rng: the same bits
    assert torch.equal(x2, x2b) and torch.equal(c2, c2b) and torch.equal(m2, m2b)
    (x1, c1, m1), arr1 = walk(1, True)
    (xe, ce, me), _ = walk(1, False)
    assert arr1["chains"] == 1
    assert torch.equal(x1, xe) and torch.equal(c1, ce) and torch.equal(m1, me)
    slots = [s for s in R.slots(K) if s >= 0]
    assert torch.equal(c2[0], c1[0]) and all(float(c2[s].abs().max()) > 0 for s in slots)
    assert rel(x2, x1) < 5e-3, rel(x2, x1)
    assert all(rel(c2[s], c1[s]) < 5e-3 for s in slots)
    assert rel(m2[0], m1[0]) < 5e-3 and rel(m2[1], m1[1]) < 5e-3 and rel(m2[3], m1[3]) < 5e-3


def test_bound_with_the_scalar_variance_has_a_total_for_a_sub_sequence():
    import smd_amd.ncsn as N
    _, _, model = make(42, 2, 8, 1)
    x0 = _examples((4, 32, 42), 47)
    ts = np.unique(R.timesteps(T, 8))
    g, _ = N.estimate_score_moments(model, BETAS, x0, ts, rng=N.PRNGKey(3))
    plain = N.variational_bound(N.PRNGKey(4), model, BETAS, x0, 8)
    out = N.variational_bound(N.PRNGKey(4), model, BETAS, x0, 8, analytic=g)
    assert plain["total"] is None and out["total"] is None and np.array_equal(plain["terms"], out["terms"])
    assert out["analytic_total"].shape == (4,) and np.isfinite(out["analytic_total"]).all() and np.isfinite(out["analytic_bits_per_dim"])
    assert out["sigma2_ratio"].shape == (8,) and (out["sigma2_ratio"] >= 1 - 1e-12).all()
