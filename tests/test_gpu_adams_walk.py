"""The third-order exponential Adams sampler as a walk on the GPU: fp32 and bf16 walks of both solvers against
the float64 table walk of tests/_adams_ref.py on the shipped tables, graph replay against eager launches, the two-chain pipeline,
the "adams" cache slot and its key, the other slots left alone, and one run of the command line.

Bounds.  fp32 walks: 4 x g32, the float32 CPU walk of _adams_ref against its float64 walk (DESIGN.md section 13's rule, as
tests/test_gpu_multistep.py).  bf16 walks: measured on an MI355X x 1.5 (BF16_MEASURED below, section 29), which must stay under
the 5e-2 SURVEY 8(c) allows bf16 samplers.
"""
import functools
import os
import sys

import pytest
import torch

import _adams_ref as A
import ddpm_oracle as O
from test_gpu_full_walk import BETAS, make, rel
from test_gpu_strided import worst_rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 1000
K = 20                                                                 # the logsnr grid snaps it to 18 iterations
SOLVERS = ("adams3", "adams3_pc")
NETS = {"small": (42, 2, 8, 1, 4), "base": (512, 6, 8, 2, 2)}          # C, L, H, mlp layers, B
# bf16 walks (logsnr, K = 20) against float64, rel-L2, worst of final state and snapshots, measured on an MI355X
BF16_MEASURED = {("small", "adams3"): 8.58e-3, ("small", "adams3_pc"): 8.17e-3, ("base", "adams3"): 8.02e-3, ("base", "adams3_pc"): 7.85e-3}


def logsnr_taus():
    return A.logsnr_timesteps(T, K, BETAS)


@functools.lru_cache(maxsize=None)
def reference(name, solver):
    """the float64 and the float32 walk of _adams_ref on the CPU oracle's network, driven by the shipped tables, computed once"""
    import smd_amd.schedule as S
    C, L, H, Km, B = NETS[name]
    ocfg, p, _ = make(C, L, H, Km, dtype="fp32")
    init = torch.randn(B, 32, C, generator=torch.Generator().manual_seed(34))
    taus = logsnr_taus()
    coef, plan = S.adams_coefficient_table(BETAS, taus, solver == "adams3_pc")
    rows = A.table_rows(coef, plan, taus, BETAS)
    out = []
    with torch.no_grad():
        for dt in (torch.float64, torch.float32):
            m = O.make_model({k: v.to(dt) for k, v in p.items()}, ocfg)
            out.append(A.table_walk(m, rows, init.to(dt), T, collect=A.slots(len(taus))))
    (rx, rc, rm), (fx, fc, fm) = out
    return init, taus, (rx, rc, rm), worst_rel(fx, fc, rx, rc), max(rel(fm[i], rm[i]) for i in (0, 1))


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", ["small", "base"])
def test_fp32_walk_against_the_float64_walk(name, solver):
    import smd_amd.ncsn as N
    C, L, H, Km, B = NETS[name]
    init, taus, (rx, rc, rm), g_state, g_met = reference(name, solver)
    _, _, model = make(C, L, H, Km, dtype="fp32")
    n = len(taus)
    x, coll, met = N.strided_dynamics(N.PRNGKey(0), model, BETAS, init, K, 0.0, spacing="logsnr", solver=solver)
    assert model.sampler_arrangement["walk"] == "adams" and model.sampler_arrangement["iterations"] == n == 18
    assert tuple(coll.shape) == (41, B, 32, C) and tuple(met.shape) == (4, n, 1)
    written = sorted(k for k in range(1, 41) if float(coll[k].abs().max()) > 0)
    assert written == sorted(rc) and torch.equal(coll[0].cpu(), init)
    e_state = worst_rel(x, coll, rx, rc)
    m = met[:, :, 0].cpu().double()
    e_met = max(rel(m[i], rm[i]) for i in (0, 1))
    print(f"[fp32 {solver} walk {name} K={K} ({n} iterations)] g32: state {g_state:.3e} metrics {g_met:.3e} | GPU: state + snapshots "
          f"{e_state:.3e} (ratio {e_state / g_state:.2f}), metric rows {e_met:.3e} (ratio {e_met / g_met:.2f})")
    assert e_state <= 4 * g_state
    assert e_met <= 4 * g_met
    assert float(x.abs().max()) <= 1.0                                 # the last iteration returns the clamped x0


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", ["small", "base"])
def test_bf16_walk_against_the_float64_walk(name, solver):
    import smd_amd.ncsn as N
    C, L, H, Km, B = NETS[name]
    init, taus, (rx, rc, _), _, _ = reference(name, solver)
    _, _, model = make(C, L, H, Km)
    x, coll, _ = N.strided_dynamics(N.PRNGKey(0), model, BETAS, init, K, 0.0, spacing="logsnr", solver=solver, use_graph=False)
    e = worst_rel(x, coll, rx, rc)
    print(f"[bf16 {solver} walk {name} K={K} B={B}] worst rel-L2 of state + snapshots against float64: {e:.3e}")
    tol = 1.5 * BF16_MEASURED[name, solver]
    assert tol < 5e-2
    assert e < tol


@pytest.mark.parametrize("solver", SOLVERS)
def test_graph_replay_equals_eager_and_the_extra_terms_are_live(solver):
    import smd_amd.ncsn as N
    _, _, model = make(42, 2, 8, 1)
    init = torch.randn(4, 32, 42, generator=torch.Generator().manual_seed(5))
    a = N.strided_dynamics(N.PRNGKey(9), model, BETAS, init, K, spacing="logsnr", solver=solver, use_graph=True)
    assert model.sampler_arrangement["graphed"] and model.sampler_arrangement["chains"] == 1
    b = N.strided_dynamics(N.PRNGKey(9), model, BETAS, init, K, spacing="logsnr", solver=solver, use_graph=False)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    c = N.strided_dynamics(N.PRNGKey(9), model, BETAS, init, K, order=2, spacing="logsnr")
    assert rel(c[0], a[0]) > 1e-3                                      # not the second-order walk: the extra terms are there
    with pytest.raises(ValueError, match="order=3"):
        N.strided_dynamics(N.PRNGKey(9), model, BETAS, init, K, order=3)


@pytest.mark.parametrize("infill", [False, True])
def test_two_chain_walk_equals_one_chain_and_eager(infill, monkeypatch):
    """B = 136 walks as 72 + 64 pipelined chains, each with its own ring.  The comparison and tolerance of
    tests/test_gpu_multistep.py's two-chain test."""
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
        out = N.strided_dynamics(N.PRNGKey(5), model, BETAS, init, K, 0.0, use_graph=graph, spacing="logsnr", solver="adams3_pc", **kw)
        return out, dict(model.sampler_arrangement)

    (x2, c2, m2), arr = walk(2, True)
    assert arr["chain_sizes"] == [72, 64] and arr["pipelined_unroll"] == 8 and arr["padded"] == 0 and arr["walk"] == "adams"
    (x1, c1, m1), arr1 = walk(1, True)
    (xe, ce, me), _ = walk(1, False)
    assert arr1["chains"] == 1
    assert torch.equal(x1, xe) and torch.equal(c1, ce) and torch.equal(m1, me)      # one chain: replay == eager, bitwise
    slots = [s for s in A.slots(len(logsnr_taus())) if s >= 0]
    assert torch.equal(c2[0], c1[0]) and all(float(c2[s].abs().max()) > 0 for s in slots)
    assert rel(x2, x1) < 5e-3, rel(x2, x1)
    assert all(rel(c2[s], c1[s]) < 5e-3 for s in slots)
    assert rel(m2[0], m1[0]) < 5e-3 and rel(m2[1], m1[1]) < 5e-3
    assert torch.equal(m2[2], m1[2])
    assert float((x2[72:] - init[72:].cuda()).abs().max()) > 0
    if infill:
        m = kw["infill_masks"].cuda().bool()
        assert torch.equal(x2[m], kw["infill_samples"].cuda()[m])                    # the last iteration returns the template


def test_steps_that_snap_to_the_same_number_of_iterations_do_not_share_graphs():
    """K = 19 and K = 20 are both 18 iterations on the lambda grid, on different timesteps: the key carries the walk"""
    import smd_amd.ncsn as N
    import smd_amd.schedule as S
    t19, t20 = (list(S.logsnr_timesteps(T, k, BETAS)) for k in (19, 20))
    assert len(t19) == len(t20) == 18 and t19 != t20
    init = torch.randn(4, 32, 42, generator=torch.Generator().manual_seed(10))
    walk = lambda m, k, solver="adams3_pc": N.strided_dynamics(N.PRNGKey(1), m, BETAS, init, k, spacing="logsnr", solver=solver)
    _, _, model = make(42, 2, 8, 1)
    a19 = walk(model, 19)
    entry = model._sampler_graphs["adams"]
    a20 = walk(model, 20)
    assert model._sampler_graphs["adams"] is not entry
    _, _, fresh = make(42, 2, 8, 1)
    want = walk(fresh, 20)
    assert all(torch.equal(u, v) for u, v in zip(a20, want))
    assert not torch.equal(a19[0], a20[0])
    entry = model._sampler_graphs["adams"]
    assert all(torch.equal(u, v) for u, v in zip(walk(model, 20), want)) and model._sampler_graphs["adams"] is entry
    # the other solver on the same timesteps is another entry too, and another result
    p = walk(model, 20, "adams3")
    assert model._sampler_graphs["adams"] is not entry and not torch.equal(p[0], want[0])
    assert all(torch.equal(u, v) for u, v in zip(p, walk(fresh, 20, "adams3")))


def test_the_other_walks_keep_their_slots_and_results():
    """a default-solver walk (order 1, order 2, the every-timestep entry) after an adams walk on the same model equals a fresh
    model's, bitwise, and the adams walk evicted none of their cache entries"""
    import smd_amd.ncsn as N
    init = torch.randn(4, 32, 42, generator=torch.Generator().manual_seed(6))
    _, _, model = make(42, 2, 8, 1)
    _, _, fresh = make(42, 2, 8, 1)
    others = (dict(order=1), dict(order=2, spacing="logsnr"), dict(order=1, spacing="logsnr", eta=0.5))
    run = lambda m, kw: N.strided_dynamics(N.PRNGKey(1), m, BETAS, init, K, **kw)
    first = [run(model, kw) for kw in others[:2]]
    kept = {k: model._sampler_graphs[k] for k in ("strided", "multistep")}
    run(model, dict(spacing="logsnr", solver="adams3_pc"))
    assert set(model._sampler_graphs) == {"strided", "multistep", "adams"}
    assert all(model._sampler_graphs[k] is v for k, v in kept.items())
    for kw, got in zip(others[:2], first):
        again, want = run(model, kw), run(fresh, kw)
        assert all(torch.equal(u, v) for u, v in zip(again, want)) and all(torch.equal(u, v) for u, v in zip(got, want))
    assert all(torch.equal(u, v) for u, v in zip(run(model, others[2]), run(fresh, others[2])))
    assert "adams" in model._sampler_graphs
    model.drop_sampler_cache()
    assert "_sampler_graphs" not in model.__dict__


def test_sample_passes_the_solver_on():
    import smd_amd.ncsn as N
    _, _, model = make(42, 2, 8, 1)
    g, c, _ = N.sample(model, BETAS, N.PRNGKey(2), (32, 42), num_samples=4, sampling="ddpm", ddim_steps=K, ddim_spacing="logsnr",
                       ddim_solver="adams3")
    assert model.sampler_arrangement["walk"] == "adams" and tuple(g.shape) == (4, 32, 42) and bool(torch.isfinite(g).all())
    with pytest.raises(ValueError, match="ddim_solver"):
        N.sample(model, BETAS, N.PRNGKey(2), (32, 42), num_samples=4, sampling="ddpm", ddim_solver="adams3")


def test_cli_generates_with_the_corrector(tmp_path):
    """sample_ncsn.py --synthetic --ddim_steps=20 --ddim_spacing=logsnr --ddim_solver=adams3_pc at the sizes of
    tests/test_gpu_multistep_cli.py (2 layers, T = 50, 8 samples), in this process: the reference's files, repeatably, and not the
    files of the default solver"""
    import importlib
    import numpy as np
    import smd_amd.data as D
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    sm = importlib.import_module("sample_ncsn")
    flags = [f"--flagfile={ROOT}/configs/ddpm-mel-32seq-512.cfg", "--synthetic", "--slice_ckpt=", f"--model_dir={tmp_path / 'no_model'}",
             "--num_layers=2", "--mlp_dims=256", "--num_mlp_layers=1", "--num_sigmas=50", "--sample_size=8", "--sampling=ddpm",
             "--ddim_steps=20", "--ddim_spacing=logsnr"]
    gens = {}
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        for name, extra in (("pc", ["--ddim_solver=adams3_pc"]), ("pc2", ["--ddim_solver=adams3_pc"]), ("default", [])):
            sm.main(["sample_ncsn.py", *flags, f"--sampling_dir={tmp_path / name}", *extra])
            gens[name] = D.load(str(tmp_path / name / "ncsn" / "generated.pkl"))
    finally:
        os.chdir(cwd)
    gen = gens["pc"]
    assert gen.shape == (8, 32, 512) and np.isfinite(gen).all() and np.abs(gen).max() <= 1.0
    assert np.array_equal(gen, gens["pc2"]) and not np.allclose(gen, gens["default"])
    coll = D.load(str(tmp_path / "pc" / "ncsn" / "collection.pkl"))
    assert coll.shape == (41, 8, 32, 512) and np.isfinite(coll).all()
