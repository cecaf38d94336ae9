"""The variational bound on the GPU: the two kernels of csrc/bound.hip, teacher-forced on explicit arrays,
against the float64 restatement of tests/_bound_ref.py on the same float32 inputs and tables; then ncsn.variational_bound's walk
against the float64 network of oracle/ddpm_oracle.py, and its determinism, sharding and cache properties."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import _bound_ref as R
from _footprint import guarded, guarded_like

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
DEV = "cuda:0"
T = 1000
BETAS = np.linspace(np.float32(1e-6), np.float32(1e-2), T, dtype=np.float32)
SHAPES = [(3, 32, 42), (2, 32, 512), (4, 1, 512), (5, 1, 42)]
TS = (0, 1, 500, 999)


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def L():
    import smd_amd.lib as lib
    return lib


@pytest.fixture(scope="module")
def tab():
    import smd_amd.schedule as S
    return S.bound_tables(BETAS, np.arange(T))


def inputs(shape):
    rng = np.random.default_rng(0)
    x0 = np.clip(0.25 * rng.standard_normal(shape), -1, 1).astype(np.float32)
    eps = rng.standard_normal(shape).astype(np.float32)
    eh = (eps + 0.5 * rng.standard_normal(shape)).astype(np.float32)
    return x0, eps, eh


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def noise(L, table_d, x0, eps, t, *, draw=0, seed=(0, 0), off=0, x_t=None, bf=None, Cp=0, key=None):
    """smd_bound_noise on device tensors; returns (x_t, t_ptr)"""
    B, S, Cn = x0.shape
    tp = torch.tensor([t], dtype=torch.int32, device=DEV)
    x_t = torch.zeros_like(x0) if x_t is None else x_t
    L.check(L.get_lib().smd_bound_noise(x0.data_ptr(), B, S, Cn, Cp, table_d.data_ptr(), T, tp.data_ptr(), eps.data_ptr(), draw,
                                        seed[0], seed[1], None if key is None else key.data_ptr(), off, x_t.data_ptr(),
                                        None if bf is None else bf.data_ptr(), _stream()), "bound_noise")
    return x_t, tp


def terms(L, table_d, x0, eps, eh, t, *, clip=1.0, next_t=None, partial=None, arrive=None):
    """smd_bound_terms; returns (partial [T][B][3], t_ptr)"""
    B, S, Cn = x0.shape
    tp = torch.tensor([t], dtype=torch.int32, device=DEV)
    partial = torch.zeros((T, B, 3), dtype=torch.float32, device=DEV) if partial is None else partial
    L.check(L.get_lib().smd_bound_terms(x0.data_ptr(), eps.data_ptr(), eh.data_ptr(), B, S, Cn, table_d.data_ptr(), T, clip,
                                        tp.data_ptr(), None if next_t is None else next_t.data_ptr(),
                                        None if arrive is None else arrive.data_ptr(), partial.data_ptr(), _stream()), "bound_terms")
    return partial, tp


# ------------------------------------------------------------------ kernels, teacher-forced
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_against_float64(L, tab, shape):
    """x_t, its bf16 copy and the three sums at t in {0, 1, 500, 999}.  The sums stay within 1e-5 relative of float64 on the same
    float32 inputs and table rows: at most 16384 non-negative terms, tree summation of about 14 levels at 6e-8, and a
    per-element error of at most 3e-5 of random sign.  Both branches of the difference are exercised: the reference alone shows
    a clipped share of x0_hat within [5 %, 95 %] at t = 500 and 999 and none at t <= 1 (asserted first).  At t <= 1 the only
    elements that can clip are those the input recipe itself saturated, x0 = clip(0.25 N(0,1)) = +-1 exactly (6e-5 of them: none
    among the 4032 of (3, 32, 42), one among the 32768 of (2, 32, 512)): none is asserted wherever no x0 is saturated, and
    elsewhere that every clipped element is a saturated one."""
    x0, eps, eh = inputs(shape)
    table = tab["table"]
    table_d = dev(table)
    x0_d, eps_d, eh_d = dev(x0), dev(eps), dev(eh)
    B, S, Cn = shape
    Cp = (Cn + 63) // 64 * 64
    for t in TS:
        rec, share = R.x0_hat(x0, eps, eh, table[t])
        if t <= 1:
            saturated = np.abs(x0) == 1.0
            assert not (np.abs(rec) == 1.0)[~saturated].any() and share <= saturated.mean(), (t, share)
            assert share == 0.0 or saturated.any()
        else:
            assert 0.05 <= share <= 0.95, (t, share)
        bf = torch.zeros((B * S, Cp), dtype=torch.bfloat16, device=DEV)
        xt, _ = noise(L, table_d, x0_d, eps_d, t, bf=bf, Cp=Cp)
        want = R.x_t(x0, eps, table[t])
        scale = np.abs(float(table[t, 0]) * x0.astype(np.float64)) + np.abs(float(table[t, 1]) * eps.astype(np.float64))
        err = np.abs(xt.cpu().numpy().astype(np.float64) - want)
        print(f"{shape} t={t}: x_t max err / scale {float((err / scale).max()):.2e}, clipped share {share:.3f}")
        assert np.all(err <= 2e-7 * scale)
        assert torch.equal(bf[:, :Cn].reshape(B, S, Cn), xt.to(torch.bfloat16)) and not bf[:, Cn:].any()
        part, tp = terms(L, table_d, x0_d, eps_d, eh_d, t)
        got = part[t].double().cpu().numpy()
        ref = R.three_sums(x0, eps, eh, table[t])
        e = np.abs(got - ref) / ref
        print(f"{shape} t={t}: sums max rel err q {e[:, 0].max():.2e} e {e[:, 1].max():.2e} n {e[:, 2].max():.2e}")
        assert e.max() < 1e-5, (t, e.max(axis=0))
        assert int(tp) == t and not part[np.arange(T) != t].any()
        # clip = inf: no clamp, the sum is sqrt_m1^2 e_t up to the table's rounding
        part, _ = terms(L, table_d, x0_d, eps_d, eh_d, t, clip=float("inf"))
        ref = R.three_sums(x0, eps, eh, table[t], clip=np.inf)
        assert (np.abs(part[t].double().cpu().numpy() - ref) / ref).max() < 1e-5, t


@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_are_deterministic_and_batch_independent(L, tab, shape):
    """two calls give equal bits; row b computed with B = 1 equals row b of the batch, bitwise; the walk's advance"""
    x0, eps, eh = (dev(v) for v in inputs(shape))
    table_d = dev(tab["table"])
    next_t = dev(tab["next_t"])
    arrive = torch.zeros(1, dtype=torch.int32, device=DEV)
    for t in TS:
        p1, tp = terms(L, table_d, x0, eps, eh, t, next_t=next_t, arrive=arrive)
        p2, _ = terms(L, table_d, x0, eps, eh, t)
        assert torch.equal(p1, p2)
        assert int(tp) == int(tab["next_t"][t]) and int(arrive) == 0
        x1, _ = noise(L, table_d, x0, eps, t)
        x2, _ = noise(L, table_d, x0, eps, t)
        assert torch.equal(x1, x2)
        for b in range(shape[0]):
            pb, _ = terms(L, table_d, x0[b:b + 1].contiguous(), eps[b:b + 1].contiguous(), eh[b:b + 1].contiguous(), t)
            assert torch.equal(pb[t, 0], p1[t, b]), (t, b)
            xb, _ = noise(L, table_d, x0[b:b + 1].contiguous(), eps[b:b + 1].contiguous(), t)
            assert torch.equal(xb[0], x1[b])


@pytest.mark.parametrize("shape", [(4, 32, 42), (4, 1, 512)])
def test_philox_draw_is_keyed_by_the_global_sample(L, tab, shape):
    """the eps of global sample g depends on neither sample_offset nor B, is a stream of its own (id 5: the t = 0 draw is
    smd_rng_normal's stream 5 and none of 0..4), changes with t and with the key, and x_t is made from the eps written"""
    B, S, Cn = shape
    x0 = dev(inputs(shape)[0])
    table_d = dev(tab["table"])
    seed = (0x1234, 0x9)
    eps = torch.zeros_like(x0)
    xt, _ = noise(L, table_d, x0, eps, 500, draw=1, seed=seed)
    want = R.x_t(x0.cpu().numpy(), eps.cpu().numpy(), tab["table"][500])
    assert np.abs(xt.cpu().numpy() - want).max() < 1e-6 and abs(float(eps.std()) - 1.0) < 0.1
    for g in range(B):
        e1 = torch.zeros_like(x0[:1])
        noise(L, table_d, x0[g:g + 1].contiguous(), e1, 500, draw=1, seed=seed, off=g)
        assert torch.equal(e1[0], eps[g]), g
    e2 = torch.zeros_like(x0[:2])
    noise(L, table_d, x0[2:4].contiguous(), e2, 500, draw=1, seed=seed, off=2)
    assert torch.equal(e2, eps[2:4])
    key = torch.tensor([seed[0], seed[1]], dtype=torch.int32, device=DEV)          # the device-resident key wins
    ek = torch.zeros_like(x0)
    noise(L, table_d, x0, ek, 500, draw=1, seed=(1, 1), key=key)
    assert torch.equal(ek, eps)
    e0 = torch.zeros_like(x0)
    noise(L, table_d, x0, e0, 0, draw=1, seed=seed)
    assert not torch.equal(e0, eps)
    for sid in range(6):
        r = torch.zeros_like(x0)
        L.check(L.get_lib().smd_rng_normal(r.data_ptr(), B, S * Cn, seed[0], seed[1], sid, 0, _stream()), "rng_normal")
        assert torch.equal(r, e0) == (sid == 5), sid


@pytest.mark.parametrize("shape", [(3, 32, 42), (2, 32, 512), (5, 1, 42)])
def test_footprint(L, tab, shape):
    """only row t of partial, only the columns < C of the bf16 input, nothing past any array; t = -1 and t = T write nothing
    and leave *t_ptr alone"""
    B, S, Cn = shape
    Cp = (Cn + 63) // 64 * 64
    x0, eps, eh = (torch.from_numpy(v) for v in inputs(shape))
    table_d = dev(tab["table"])
    next_t = dev(tab["next_t"])
    arrive = torch.zeros(1, dtype=torch.int32, device=DEV)
    x0_v, x0_h = guarded_like(x0, DEV)
    eps_v, eps_h = guarded_like(eps, DEV)
    eh_v, eh_h = guarded_like(eh, DEV)
    for t in (500, -1, T):
        xt_v, xt_h = guarded(shape, torch.float32, DEV)
        bf_v, bf_h = guarded((B * S, Cn), torch.bfloat16, DEV, ld=Cp)
        pa_v, pa_h = guarded((T, B, 3), torch.float32, DEV)
        ed_v, ed_h = guarded(shape, torch.float32, DEV)
        for v in (xt_v, pa_v, ed_v):
            v.fill_(-7.0)
        bf_v.fill_(-7.0)
        snaps = [h.snapshot() for h in (x0_h, eps_h, eh_h)]
        _, tp = noise(L, table_d, x0_v, eps_v, t, x_t=xt_v, bf=bf_v, Cp=Cp)
        _, tp2 = noise(L, table_d, x0_v, ed_v, t, draw=1, seed=(3, 4), x_t=torch.zeros(shape, device=DEV))
        _, tp3 = terms(L, table_d, x0_v, eps_v, eh_v, t, next_t=next_t, partial=pa_v, arrive=arrive)
        torch.cuda.synchronize()
        for h, name in ((xt_h, "x_t"), (bf_h, "bf16 input"), (pa_h, "partial"), (ed_h, "drawn eps")):
            h.assert_untouched(name)
        for h, s, name in zip((x0_h, eps_h, eh_h), snaps, ("x0", "eps", "eps_hat")):
            h.assert_same(s, name)
        live = 0 <= t < T
        assert int(tp) == t and int(tp2) == t and int(tp3) == (int(tab["next_t"][t]) if live else t) and int(arrive) == 0
        rows = torch.arange(T, device=DEV) != t
        assert bool((pa_v[rows] == -7.0).all())
        if live:
            assert not bool((xt_v == -7.0).any()) and not bool((bf_v == -7.0).any()) and not bool((ed_v == -7.0).any())
            assert bool(torch.isfinite(pa_v[t]).all()) and not bool((pa_v[t] == -7.0).any())
        else:
            assert bool((xt_v == -7.0).all()) and bool((bf_v == -7.0).all()) and bool((ed_v == -7.0).all())


def test_argument_checks(L, tab):
    x0, eps, eh = (dev(v) for v in inputs((2, 32, 42)))
    table_d = dev(tab["table"])
    with pytest.raises(ValueError, match="clip"):
        terms(L, table_d, x0, eps, eh, 3, clip=0.0)
    with pytest.raises(ValueError, match="arrival counter"):
        terms(L, table_d, x0, eps, eh, 3, next_t=dev(tab["next_t"]))
    with pytest.raises(ValueError, match="bad shape"):
        noise(L, table_d, x0, eps, 3, bf=torch.zeros((64, 64), dtype=torch.bfloat16, device=DEV), Cp=40)


def test_torch_ops(tab):
    import smd_amd.ops  # noqa: F401
    x0, eps, eh = inputs((3, 32, 42))
    table_d = dev(tab["table"])
    t = torch.tensor([500], dtype=torch.int32, device=DEV)
    xt = torch.ops.smd_amd.bound_noise(dev(x0), dev(eps), table_d, t)
    assert np.abs(xt.cpu().numpy() - R.x_t(x0, eps, tab["table"][500])).max() < 1e-6
    sums = torch.ops.smd_amd.bound_terms(dev(x0), dev(eps), dev(eh), table_d, t, 1.0)
    ref = R.three_sums(x0, eps, eh, tab["table"][500])
    assert (np.abs(sums.double().cpu().numpy() - ref) / ref).max() < 1e-5 and int(t) == 500


# ------------------------------------------------------------------ the walk
T40 = 40
BETAS40 = np.linspace(np.float32(1e-6), np.float32(1e-2), T40, dtype=np.float32)

# Worst relative error against the float64 walk measured on the MI355X (per-timestep mean over the examples, total), times 1.5;
# tabulated in DESIGN.md section 17.  {(architecture, dtype): (terms, total)}
# At B = 4 (128 token rows) and B = 5 (5 rows) the engine's e4m3 GEMMs do not engage (they take multiples of 256 rows) and fp8
# runs the bf16 kernels: equal figures.  "transformer8" is the same network at B = 8, 256 rows, where they do.
MEASURED = {
    ("transformer", "bf16"): (1.558e-3, 1.405e-3),
    ("transformer", "fp8"): (1.558e-3, 1.405e-3),
    ("transformer", "fp32"): (5.166e-6, 3.656e-6),
    ("dense", "bf16"): (1.585e-3, 1.483e-4),
    ("dense", "fp8"): (1.585e-3, 1.483e-4),
    ("dense", "fp32"): (2.951e-5, 2.289e-5),
    ("transformer8", "fp8"): (2.932e-3, 2.660e-3),
}
LIMITS = {k: (None if v[0] is None else 1.5 * v[0], None if v[1] is None else 1.5 * v[1]) for k, v in MEASURED.items()}


def make_model(arch, dtype, nT):
    import ddpm_oracle as O
    import smd_amd.ncsn as N
    from smd_amd.engine import NetConfig
    if arch.startswith("transformer"):
        ocfg = O.NetConfig(data_channels=42, num_layers=2, num_heads=8, num_mlp_layers=1)
        cfg = NetConfig(data_channels=42, num_layers=2, num_heads=8, num_mlp_layers=1, num_timesteps=nT, dtype=dtype)
        B = 8 if arch == "transformer8" else 4
    else:
        ocfg = O.NetConfig(architecture="DenseDDPM", data_channels=42, num_layers=2)
        cfg = NetConfig(architecture="DenseDDPM", data_channels=42, num_layers=2, num_timesteps=nT, dtype=dtype)
        B = 5
    p = O.init_params(ocfg, 0, torch.float64)
    model = N.Model(cfg, DEV, seed=None)
    model.engine.load_named(p)
    shape = (B, *cfg.sample_shape)
    rng = np.random.default_rng(5)
    x0 = np.clip(0.25 * rng.standard_normal(shape), -1, 1).astype(np.float32)
    return model, O.make_model(p, ocfg), x0


_REF = {}


def reference_walk(arch, model64, betas, x0, eps, timesteps):
    """computed once per (architecture, schedule) and shared, unchanged, among the precisions"""
    key = (arch, len(betas), len(timesteps))
    if key not in _REF:
        lookup = {int(t): k for k, t in enumerate(timesteps)}
        _REF[key] = R.walk(model64, betas, x0, lambda t: eps[lookup[t]], [int(t) for t in timesteps])
    return _REF[key]


def walk_errors(out, ref):
    gm, rm = out["terms"].mean(axis=1), ref["terms"].mean(axis=1)
    e_terms = float(np.max(np.abs(gm - rm) / np.abs(rm)))
    e_total = None
    if ref["total"] is not None:
        e_total = float(abs(out["total"].mean() - ref["total"].mean()) / abs(ref["total"].mean()))
    return e_terms, e_total


@pytest.mark.parametrize("arch,dtype", [(a, d) for a in ("transformer", "dense") for d in ("bf16", "fp8", "fp32")] + [("transformer8", "fp8")])
def test_walk_against_the_float64_network(arch, dtype):
    """every timestep of a 40-step schedule with explicit eps: terms, prior and total against the float64 walk"""
    import smd_amd.ncsn as N
    model, model64, x0 = make_model(arch, dtype, T40)
    eps = np.random.default_rng(6).standard_normal((T40, *x0.shape)).astype(np.float32)
    out = N.variational_bound(N.PRNGKey(0), model, BETAS40, x0, 0, eps_in=eps)
    ref = reference_walk(arch, model64, BETAS40, x0, eps, np.arange(T40))
    assert np.array_equal(out["timesteps"], np.arange(T40)) and out["terms"].shape == (T40, x0.shape[0])
    e_terms, e_total = walk_errors(out, ref)
    e_prior = float(np.max(np.abs(out["prior"] - ref["prior"]) / np.abs(ref["prior"])))
    e_mse = float(np.max(np.abs(out["eps_mse"].mean(1) - ref["eps_mse"].mean(1)) / ref["eps_mse"].mean(1)))
    print(f"MEASURE walk {arch} {dtype}: terms {e_terms:.3e} total {e_total:.3e} prior {e_prior:.3e} eps_mse {e_mse:.3e} "
          f"bits/dim {out['bits_per_dim']:.5f} (float64 {ref['total'].mean() / (x0[0].size * np.log(2)):.5f})")
    assert e_prior < 1e-5                       # no network involved: the fp32 sum of x0^2
    D = x0[0].size
    assert abs(out["bits_per_dim"] - out["total"].mean() / (D * np.log(2))) < 1e-12 * abs(out["bits_per_dim"])
    lim_terms, lim_total = LIMITS[(arch, dtype)]
    assert lim_terms is not None, "the measured constants are not filled in"
    assert e_terms <= lim_terms and e_total <= lim_total
    if dtype == "bf16":
        assert lim_terms < 5e-2 and lim_total < 5e-2


def test_stride_on_the_base_schedule():
    """24 of the 1000 timesteps: the curve only, the same constants as the every-timestep bf16 walk"""
    import smd_amd.ncsn as N
    import smd_amd.schedule as S
    model, model64, x0 = make_model("transformer", "bf16", T)
    ts = np.sort(S.stride_timesteps(T, 24))
    eps = np.random.default_rng(7).standard_normal((len(ts), *x0.shape)).astype(np.float32)
    out = N.variational_bound(N.PRNGKey(0), model, BETAS, x0, 24, eps_in=eps)
    assert np.array_equal(out["timesteps"], ts) and out["timesteps"][0] == 0 and out["timesteps"][-1] == T - 1
    assert out["total"] is None and out["bits_per_dim"] is None and out["nats_per_dim"] is None
    ref = reference_walk("transformer", model64, BETAS, x0, eps, ts)
    e_terms, _ = walk_errors(out, ref)
    print(f"MEASURE stride transformer bf16: terms {e_terms:.3e}")
    lim_terms, _ = LIMITS[("transformer", "bf16")]
    assert lim_terms is not None, "the measured constants are not filled in"
    assert e_terms <= lim_terms


@pytest.fixture(scope="module")
def small():
    return make_model("transformer", "bf16", T40)


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("timesteps", "terms", "eps_mse", "prior", "total"))


def test_graph_and_eager_agree_and_repeat(small):
    import smd_amd.ncsn as N
    model, _, x0 = small
    g1 = N.variational_bound(N.PRNGKey(11), model, BETAS40, x0)
    g2 = N.variational_bound(N.PRNGKey(11), model, BETAS40, x0)                     # the cached graphs
    e1 = N.variational_bound(N.PRNGKey(11), model, BETAS40, x0, use_graph=False)
    assert same(g1, g2) and same(g1, e1)
    other = N.variational_bound(N.PRNGKey(12), model, BETAS40, x0)
    assert not np.array_equal(other["terms"], g1["terms"]) and np.array_equal(other["prior"], g1["prior"])
    assert np.isfinite(g1["terms"]).all() and g1["total"].shape == (x0.shape[0],)


@pytest.mark.parametrize("impl", ["philox", "threefry"])
def test_two_shards_are_the_unsharded_result(small, impl):
    import smd_amd.jax_random as J
    import smd_amd.ncsn as N
    model, _, x0 = small
    rng = N.make_key(21, impl)
    whole = N.variational_bound(rng, model, BETAS40, x0, global_num_samples=4)
    a = N.variational_bound(rng, model, BETAS40, x0[:2], sample_offset=0, global_num_samples=4)
    b = N.variational_bound(rng, model, BETAS40, x0[2:], sample_offset=2, global_num_samples=4)
    for k in ("terms", "eps_mse"):
        assert np.array_equal(np.concatenate([a[k], b[k]], axis=1), whole[k]), k
    for k in ("prior", "total"):
        assert np.array_equal(np.concatenate([a[k], b[k]]), whole[k]), k
    if impl == "threefry":
        # the draw of the last timestep is still in the walk's buffer: normal(split(rng, T)[T-1], (N_global, S, C)), this rank's window
        eps = model._sampler_graphs["bound"]["eps"]
        per = x0[0].size
        want = J.normal(J.split(rng, T40)[T40 - 1], x0[2:].shape, DEV, n_total=4 * per, offset=2 * per)
        assert torch.equal(eps, want)


def test_cache_slot(small):
    import smd_amd.ncsn as N
    model, _, x0 = small
    model.drop_sampler_cache()
    N.strided_dynamics(N.PRNGKey(1), model, BETAS40, torch.randn(x0.shape), 4)
    N.variational_bound(N.PRNGKey(1), model, BETAS40, x0)
    cache = model._sampler_graphs
    strided, first = cache["strided"], cache["bound"]
    assert set(cache) == {"strided", "bound"}
    N.variational_bound(N.PRNGKey(1), model, BETAS40, x0)
    assert cache["bound"] is first                                                  # same timestep set: reused
    N.variational_bound(N.PRNGKey(1), model, BETAS40, x0, 8)
    assert cache["bound"] is not first and cache["strided"] is strided and set(cache) == {"strided", "bound"}
    assert len(cache["bound"]["key"][0]) == 8
    model.drop_sampler_cache()
    assert "_sampler_graphs" not in model.__dict__
