"""The fp32 engine (NetConfig.dtype = "fp32": reference precision, inference only) against the float64 oracle.

Bounds.  SURVEY 8(c) gives 1e-5 per fp32 KERNEL (tests/test_gpu_fp32_kernels.py); for the whole network and for a walk no number
is known in advance, so each bound is MEASURED ON THE REFERENCE SIDE: oracle/ddpm_oracle.py once in float32 and once in float64
on the CPU with identical weights, inputs and noise; their rel-L2 is `g32`, what float32 arithmetic costs the reference's own
computation in another summation order.  The GPU bound is 4 x g32 for that quantity and shape (tiled MFMA reduction order over
K = 2048, hardware exp / tanh / sin against libm), far below the bf16 engine's 6e-3.  Every g32, GPU value and ratio is printed.

Measured on an MI355X: forward, 54 cases: g32 1.5e-6 .. 5.1e-5, GPU / g32 between 0.96 and 1.40, the bf16 engine
230 .. 3250 times further from float64; DenseDDPM ratio 1.06 .. 1.25; forward_level ratio 0.99 .. 1.43; T = 1000 walks: g32_walk
1.56e-6 (small) / 2.05e-6 (base), GPU 1.62e-6 / 2.12e-6 (ratio 1.04 / 1.03), metric rows ratio 1.10 / 1.11; B = 256 bf16 against fp32
after 50 steps: 1.7e-4.
"""
import time

import numpy as np
import pytest
import torch

import ddpm_oracle as O
from test_gpu_full_walk import BETAS, make, rel, step_noise

pytestmark = pytest.mark.gpu
MSG = "fp32 is an inference precision in this engine"
SQRT_AP_T = float(np.sqrt(np.cumprod(1.0 - np.asarray(BETAS, dtype=np.float64))[-1]))        # 0.0814: the noise level of t = T - 1
LEVELS = (0.9999995, 0.6, SQRT_AP_T)
CONFIGS = {"small": (2, 8, 1), "base": (6, 8, 2), "large": (8, 16, 3)}


def oracle_pair(p, ocfg, x, s):
    """eps_hat of the float64 and of the float32 CPU oracle on the same weights and inputs."""
    with torch.no_grad():
        r64 = O.make_model(p, ocfg)(x.double(), s.double())
        r32 = O.make_model({k: v.float() for k, v in p.items()}, ocfg)(x.float(), s.float())
    return r64, r32


def inputs(B, shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.clamp(0.25 * torch.randn(B, *shape, generator=g), -1, 1)


@pytest.mark.parametrize("C", [42, 146, 512])
@pytest.mark.parametrize("name", ["small", "base", "large"])
def test_forward_against_the_fp64_oracle(name, C):
    Lr, H, K = CONFIGS[name]
    ocfg, p, m32 = make(C, Lr, H, K, dtype="fp32")
    _, _, m16 = make(C, Lr, H, K, dtype="bf16")
    lines = []
    for B in (4, 5):
        x = inputs(B, (32, C), 7 + B)
        for lv in LEVELS:
            s = torch.full((B, 1, 1), lv)
            r64, r32 = oracle_pair(p, ocfg, x, s)
            g32 = rel(r32, r64)
            e32, e16 = rel(m32(x, s), r64), rel(m16(x, s), r64)
            lines.append(f"[{name} C={C} B={B} level={lv:.7g}] g32 {g32:.3e}  fp32 engine {e32:.3e} (ratio {e32 / g32:.2f})  bf16 engine {e16:.3e} ({e16 / e32:.0f}x)")
            print(lines[-1])
            assert e32 <= 4 * g32, lines[-1]
            assert e16 >= 10 * e32, lines[-1]


def test_forward_dense_ddpm_and_mixed_levels():
    import smd_amd.ncsn as N
    from smd_amd.engine import NetConfig
    ocfg = O.NetConfig(architecture="DenseDDPM", data_channels=512, num_layers=3, num_heads=8, num_mlp_layers=2)
    p = O.init_params(ocfg, 0, torch.float64)
    models = {}
    for dt in ("fp32", "bf16"):
        models[dt] = N.Model(NetConfig(architecture="DenseDDPM", data_channels=512, num_layers=3, num_heads=8, num_mlp_layers=2, dtype=dt),
                             "cuda:0", seed=None)
        models[dt].engine.load_named(p)
    for B in (4, 5, 64):
        x = inputs(B, (512,), B)
        for lv in LEVELS + (None,):
            s = torch.full((B, 1), lv) if lv is not None else (0.05 + 0.95 * torch.rand(B, 1, generator=torch.Generator().manual_seed(B)))
            r64, r32 = oracle_pair(p, ocfg, x, s)
            g32, e32, e16 = rel(r32, r64), rel(models["fp32"](x, s), r64), rel(models["bf16"](x, s), r64)
            print(f"[DenseDDPM B={B} level={lv}] g32 {g32:.3e}  fp32 engine {e32:.3e} (ratio {e32 / g32:.2f})  bf16 engine {e16:.3e}")
            assert e32 <= 4 * g32 and e16 >= 10 * e32


@pytest.mark.parametrize("name,C", [("small", 42), ("base", 512)])
def test_forward_level_through_the_film_tables(name, C):
    """forward_level reads row r of the T-row FiLM tables prepare_sampler built on the fp32 GEMM: noise level sqrt_ap[r]."""
    import ctypes
    import smd_amd.lib as lib
    Lr, H, K = CONFIGS[name]
    ocfg, p, model = make(C, Lr, H, K, dtype="fp32")
    eng = model.engine
    eng.set_schedule(BETAS, with_sampler=True)
    B = 5
    eng.bind(B, training=False)
    eng.prepare_sampler()
    x = inputs(B, (32, C), 3)
    sqrt_ap = eng._sched_tensors["sqrt_ap"].cpu()
    for r in (0, 500, 999):
        lvl = torch.tensor([r], dtype=torch.int32, device=eng.device)
        out = torch.empty(B, 32, C, device=eng.device)
        lib.check(eng.L.smd_engine_forward_level(eng.h, x.to(eng.device).data_ptr(), lvl.data_ptr(), out.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream), "forward_level")
        s = torch.full((B, 1, 1), float(sqrt_ap[r]))
        r64, r32 = oracle_pair(p, ocfg, x, s)
        g32, e = rel(r32, r64), rel(out, r64)
        same = torch.equal(out, model(x, s))          # the table row and the per-sample generator are the same three GEMMs
        print(f"[{name} C={C} table row {r}: level {float(sqrt_ap[r]):.7g}] g32 {g32:.3e}  forward_level {e:.3e} (ratio {e / g32:.2f}); == forward bitwise: {same}")
        assert e <= 4 * g32
        assert same


def test_batch_invariance_bitwise():
    """eps_hat of a sequence does not depend on the batch it is evaluated in: B = 4, 64 (2048 rows) and 256 (8192 rows)."""
    _, _, model = make(512, 6, 8, 2, dtype="fp32")
    x = inputs(256, (32, 512), 1)
    s = (0.05 + 0.95 * torch.rand(256, generator=torch.Generator().manual_seed(2))).view(256, 1, 1)
    big = model(x, s)
    for B in (4, 5, 64):
        assert torch.equal(model(x[:B], s[:B]), big[:B]), B
    assert torch.equal(model(x[100:104], s[100:104]), big[100:104])
    assert torch.equal(model(x, s), big)


@pytest.mark.parametrize("name,C", [("small", 42), ("base", 512)])
def test_full_T_walk_against_the_fp64_oracle(name, C):
    import smd_amd.ncsn as N
    Lr, H, K = CONFIGS[name]
    B = 2
    ocfg, p, model = make(C, Lr, H, K, dtype="fp32")
    init = torch.randn(B, 32, C, generator=torch.Generator().manual_seed(2718))
    nthreads = torch.get_num_threads()
    torch.set_num_threads(min(8, nthreads))
    t0 = time.perf_counter()
    try:
        with torch.no_grad():
            ref = {}
            for dt in (torch.float64, torch.float32):
                po = {k: v.to(dt) for k, v in p.items()}
                ref[dt] = O.diffusion_dynamics(O.make_model(po, ocfg), BETAS, init.to(dt), lambda t: step_noise(B, C, t).to(dt))
    finally:
        torch.set_num_threads(nthreads)
    t_or = time.perf_counter() - t0
    (rx, rc, rm), (fx, fc, fm) = ref[torch.float64], ref[torch.float32]
    g_state = max([rel(fx, rx)] + [rel(fc[k], rc[k]) for k in range(2, 41)])
    g_met = max(rel(fm[i].double(), rm[i].double()) for i in range(4))
    x, coll, met = N.diffusion_dynamics(N.PRNGKey(0), model, BETAS, init, noises=lambda t: step_noise(B, C, t))
    torch.cuda.synchronize()
    assert tuple(coll.shape) == (41, B, 32, C) and tuple(met.shape) == (4, 1000, 1)
    assert torch.equal(coll[0].cpu(), init) and float(coll[1].abs().max()) == 0.0
    e_state = max([rel(x, rx)] + [rel(coll[k], rc[k]) for k in range(2, 41)])
    e_rows = [rel(met.cpu().double()[i], rm.double()[i]) for i in range(4)]
    print(f"[{name} fp32 walk, T = 1000, B = {B}] g32_walk: state {g_state:.3e} metrics {g_met:.3e} | GPU: final state {rel(x, rx):.3e}, worst of "
          f"final + 39 snapshots {e_state:.3e} (ratio {e_state / g_state:.2f}); metric rows slope {e_rows[0]:.2e} step {e_rows[1]:.2e} "
          f"alpha {e_rows[2]:.2e} noise {e_rows[3]:.2e} (ratio {max(e_rows) / g_met:.2f}); oracle walks {t_or:.0f} s")
    assert e_state <= 4 * g_state
    assert max(e_rows) <= 4 * g_met
    assert float(x.abs().max()) <= 1.0 + 1e-6


def test_graph_replayed_walk_equals_eager_bitwise():
    import smd_amd.ncsn as N
    _, _, model = make(42, 2, 8, 1, dtype="fp32")
    init = torch.randn(4, 32, 42, generator=torch.Generator().manual_seed(5))
    a = N.diffusion_dynamics(N.PRNGKey(9), model, BETAS, init, use_graph=True)
    b = N.diffusion_dynamics(N.PRNGKey(9), model, BETAS, init, use_graph=False)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert model.sampler_arrangement["chains"] == 1
    assert float(a[1][1].abs().max()) == 0 and all(float(a[1][k].abs().max()) > 0 for k in range(2, 41))


def test_bf16_walk_against_the_fp32_engine_at_the_bench_batch():
    """The GPU as the yardstick at B = 256 (no CPU oracle): 50 reverse steps from t = 999 on the fused step's own Philox draws,
    one seed, bf16 engine against fp32 engine.  Bound: tests/test_gpu_bench_config.py asserts state rel-L2 < 1e-2 for its
    reverse-step comparison against the oracle and does not scale it with the number of steps (the full-length walk tests keep
    the same order, 1.5e-2): 1e-2 here."""
    import smd_amd.ncsn as N
    t0 = time.perf_counter()
    out = {}
    for dt in ("fp32", "bf16"):
        _, _, model = make(512, 6, 8, 2, dtype=dt)
        init = torch.randn(256, 32, 512, generator=torch.Generator().manual_seed(77))
        x, coll, met = N.diffusion_dynamics(N.PRNGKey(5), model, BETAS, init, t_stop=950)
        torch.cuda.synchronize()
        out[dt] = (x.cpu(), met.cpu(), dict(model.sampler_arrangement))
    e = rel(out["bf16"][0], out["fp32"][0])
    e_slope = rel(out["bf16"][1][0, :50], out["fp32"][1][0, :50])
    print(f"[B = 256 base, 50 reverse steps, Philox] bf16 state against the fp32 engine's: rel-L2 {e:.3e}; slope metric {e_slope:.3e}; "
          f"arrangement fp32 {out['fp32'][2]['chain_sizes']} bf16 {out['bf16'][2]['chain_sizes']}; wall {time.perf_counter() - t0:.1f} s")
    assert out["fp32"][2]["chains"] == 1
    assert 0 < e < 1e-2


def test_refusals_are_value_errors_with_the_sentence():
    import smd_amd.lib as lib
    import smd_amd.ncsn as N
    from smd_amd import ops
    from smd_amd.trainer import create_optimizer
    _, _, model = make(42, 2, 8, 1, dtype="fp32")
    eng = model.engine
    with pytest.raises(ValueError, match=MSG):
        eng.bind(4, training=True)
    with pytest.raises(ValueError, match=MSG):
        create_optimizer(model, 1e-3)
    with pytest.raises(ValueError, match=MSG):
        model.differentiable()
    x, s = torch.zeros(4, 32, 42, device="cuda"), torch.ones(4, 1, 1, device="cuda")
    with pytest.raises(ValueError, match=MSG):
        ops.eps_forward_train(x, s, eng.params, model._op_id)
    with pytest.raises(ValueError, match=MSG):
        eng.loss_backward(x, stage=3)
    with pytest.raises(ValueError, match=MSG):
        eng.optimizer_step(1e-3)
    with pytest.raises(ValueError, match="mutually exclusive"):
        eng.set_option("fp8", 1)
    _, _, m8 = make(42, 2, 8, 1, dtype="fp8")
    with pytest.raises(ValueError, match="mutually exclusive"):
        m8.engine.set_option("fp32", 1)
    # the split passes of the two-chain pipeline
    eng.set_schedule(BETAS, with_sampler=True)
    eng.bind(4, training=False)
    eng.prepare_sampler()
    t_ptr = torch.tensor([999], dtype=torch.int32, device="cuda")
    io = lib.SampleIO()
    io.x, io.t_ptr = x.data_ptr(), t_ptr.data_ptr()
    for part in (1, 2):
        with pytest.raises(ValueError, match="part"):
            eng.sample_step(io, part)
    torch.cuda.synchronize()
    assert int(t_ptr.item()) == 999 and float(x.abs().max()) == 0.0       # nothing was launched
    # workspace: grows under fp32, and a bf16 handle's is what it was
    _, _, m16 = make(42, 2, 8, 1, dtype="bf16")
    w32 = int(eng.L.smd_engine_workspace_bytes(eng.h, 8, 0))
    w16 = int(m16.engine.L.smd_engine_workspace_bytes(m16.engine.h, 8, 0))
    assert w32 > w16 > 0
