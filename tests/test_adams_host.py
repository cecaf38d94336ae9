"""Host side of the third-order exponential Adams sampler: the closed-form weights against quadrature, the
folded coefficient table against the two-stage float64 reference of tests/_adams_ref.py, the table's structure, the solver's
error on the analytic model of tests/test_multistep_host.py, the flag gates of sample_ncsn.py and the exports.  No GPU."""
import importlib
import logging
import os
import sys

import numpy as np
import pytest
import torch

import _adams_ref as A
import _multistep_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 1000


@pytest.fixture(scope="module")
def S():
    import smd_amd.schedule as S
    return S


@pytest.fixture(scope="module")
def betas(S):
    return S.create_noise_schedule(1e-6, 0.01, T, "linear")


# ------------------------------------------------------------------ the weights
@pytest.mark.parametrize("H", [1e-3, 3e-3, 1e-2, 0.1, 0.3, 0.499, 0.5, 0.7, 1.0, 2.0, 3.0])
def test_weights_against_quadrature(S, H):
    """predictor nodes (the interval's start and up to two behind it) and corrector nodes (the interval's end, its start and one
    behind), with neighbouring steps from half to twice H, on both sides of the series threshold: 1e-12 relative"""
    worst = 0.0
    for r1 in (0.5, 1.0, 2.0):
        for r2 in (0.5, 1.0, 2.0):
            lam_a = -1.25
            lam_b = lam_a + H
            back = [lam_a, lam_a - r1 * H, lam_a - r1 * H - r2 * H]
            for nodes in (back[:1], back[:2], back, [lam_b], [lam_b, lam_a], [lam_b, lam_a, lam_a - r1 * H]):
                got = S.exp_lagrange_weights(lam_a, lam_b, nodes)
                want = A.quad_weights(lam_a, lam_b, nodes)
                err = float(np.max(np.abs(got - want) / np.abs(want)))
                worst = max(worst, err)
                assert err <= 1e-12, (H, nodes, got, want)
                # the interpolant of a constant is the constant: the weights add up to Int e^(l - lam_b) dl = 1 - e^-H
                assert abs(got.sum() / -np.expm1(-H) - 1) <= 1e-12
    print(f"[H={H}] worst relative difference to 48-point Gauss-Legendre: {worst:.2e}")


def test_weights_refuse_an_empty_interval(S):
    for a, b in ((0.0, 0.0), (1.0, 0.5), (0.0, np.inf)):
        with pytest.raises(ValueError):
            S.exp_lagrange_weights(a, b, [a])


# ------------------------------------------------------------------ folded against unfolded
S2 = np.array([0.01, 0.0625, 0.25, 1.0])


def analytic_setup(betas):
    """the analytic Gaussian model of tests/test_multistep_host.py: data, seed and metric are section 18's"""
    ap = R.alphas_prod(betas)
    s2 = torch.from_numpy(S2)
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((64, 4)))

    def model(x, cond):
        a = cond ** 2
        return torch.sqrt(1 - a) * x / (a * s2 + 1 - a)

    exact = x * torch.sqrt(s2 / (ap[-1] * s2 + 1 - ap[-1]))
    return model, x, exact


def folded_walk(model, co, betas, taus, x):
    """x' = b x + A0 x0 + A1 h1 + A2 h2 + A3 h3 on the float64 coefficients of schedule.adams_coefficients, no clamp"""
    ap = R.alphas_prod(betas)[np.asarray(taus)]
    hist = [None, None, None]
    for j in range(len(taus)):
        eh = model(x, torch.full((x.shape[0], 1), float(np.sqrt(ap[j])), dtype=torch.float64))
        x0 = (x - np.sqrt(1 - ap[j]) * eh) / np.sqrt(ap[j])
        nx = co["b"][j] * x + co["A0"][j] * x0
        for i in (1, 2, 3):
            if co[f"A{i}"][j] != 0:
                nx = nx + co[f"A{i}"][j] * hist[i - 1]
        hist = [x0, hist[0], hist[1]]
        x = nx
    return x


@pytest.mark.parametrize("grid,K", [("logsnr", 10), ("logsnr", 20), ("logsnr", 80), ("uniform", 20), ("logsnr", 3), ("uniform", 2)])
@pytest.mark.parametrize("corrector", [False, True])
def test_folded_table_equals_the_unfolded_reference(S, betas, grid, K, corrector):
    taus = S.logsnr_timesteps(T, K, betas) if grid == "logsnr" else S.stride_timesteps(T, K)
    n = len(taus)
    co = S.adams_coefficients(betas, taus, corrector)
    ref = A.coefficients(betas, list(taus), np.inf)
    # the unfolded weights, and the fold written out again from the reference's own weights
    assert np.allclose(co["wp"], ref["wp"], rtol=1e-11, atol=0)
    if corrector:
        assert np.allclose(co["wc"], ref["wc"], rtol=1e-11, atol=0)
    else:
        assert not co["wc"].any()
    want = np.zeros((n, 4))
    for j in range(n):
        want[j, :3] = ref["alpha_s"][j] * ref["wp"][j]
        if corrector and 1 <= j < n - 1:
            g = ref["ratio"][j] * ref["alpha_t"][j]
            prev = ref["wp"][j - 1]
            want[j] += g * np.array([ref["wc"][j, 0], ref["wc"][j, 1] - prev[0], ref["wc"][j, 2] - prev[1], -prev[2]])
    got64 = np.stack([co[f"A{i}"] for i in range(4)], axis=1)
    assert np.allclose(got64, want, rtol=1e-10, atol=1e-15)
    coef, _ = S.adams_coefficient_table(betas, taus, corrector)
    got32 = coef[taus][:, [2, 8, 9, 10]].astype(np.float64)
    assert np.all(np.abs(got32 - want) <= 2.0 ** -23 * np.abs(want)), np.max(np.abs(got32 - want) / np.maximum(np.abs(want), 1e-300))
    assert np.all(np.abs(coef[taus, 3] - ref["ratio"]) <= 2.0 ** -23 * ref["ratio"])
    # the final states of the analytic-model walk: folded float64 coefficients against corrector-then-predictor
    model, x, _ = analytic_setup(betas)
    a = folded_walk(model, co, betas, taus, x)
    b, _, _ = A.walk(model, ref, x, T, corrector)
    err = float((a - b).norm() / b.norm())
    print(f"[{grid} K={K} corrector={corrector}] folded against two-stage, rel-L2 of the final state: {err:.2e}")
    assert err <= 1e-12


# ------------------------------------------------------------------ the table's structure
@pytest.mark.parametrize("grid,K", [("logsnr", 10), ("logsnr", 20), ("uniform", 20), ("logsnr", 3), ("uniform", 2), ("logsnr", 4)])
@pytest.mark.parametrize("corrector", [False, True])
@pytest.mark.parametrize("prediction", ["eps", "v"])
def test_table_structure(S, betas, grid, K, corrector, prediction):
    taus = S.logsnr_timesteps(T, K, betas) if grid == "logsnr" else S.stride_timesteps(T, K)
    n = len(taus)
    coef, plan = S.adams_coefficient_table(betas, taus, corrector, prediction=prediction)
    assert coef.dtype == np.float32 and coef.shape == (T, 12) and plan.dtype == np.int32 and plan.shape == (T, 4)
    base, base_plan = S.strided_coefficient_table(betas, taus, 0.0, prediction=prediction)
    assert np.array_equal(plan, base_plan)
    for c in (0, 1, 3, 4, 5, 6, 7):
        assert np.array_equal(coef[:, c].view(np.uint32), base[:, c].view(np.uint32)), c
    bits = coef.view(np.uint32)
    off = np.setdiff1d(np.arange(T), taus)
    assert not bits[off].any() and not bits[:, 11].any()              # exact +0: not even a sign bit
    for j, t in enumerate(taus):
        live = [True, j >= 1, j >= 2, corrector and j >= 3]
        if j == n - 1:
            live = [True, False, False, False]
            assert coef[t, 2] == 1.0 and coef[t, 3] == 0.0            # the last iteration returns x0
        for i, c in enumerate((2, 8, 9, 10)):
            assert (bits[t, c] != 0) == live[i], (j, i, coef[t, c])
    # consistency: a constant x0 history is integrated exactly, so the A add up to the strided a -- to the float32 rounding of
    # the (on the uniform grid large, alternating) A themselves: 2^-24 each and 2^-24 for a
    Acols = coef[taus][:, [2, 8, 9, 10]].astype(np.float64)
    assert np.all(np.abs(Acols.sum(axis=1) - base[taus, 2]) <= 2.0 ** -23 * np.abs(Acols).sum(axis=1))


def test_kept_coefficients_give_the_same_table_and_are_not_the_callers_to_change(S, betas):
    """a warm sampler builds its table on every call: the A columns are kept per (schedule, walk, solver), a second build has the
    first one's bits whatever clip / prediction it asks for, and writing into a returned table does not reach the next one"""
    taus = S.logsnr_timesteps(T, 20, betas)
    S._ADAMS_A_CACHE.clear()
    first, plan = S.adams_coefficient_table(betas, taus, True)
    assert len(S._ADAMS_A_CACHE) == 1
    first[:, 8:11] = 7.0
    again, plan2 = S.adams_coefficient_table(betas, taus, True)
    assert len(S._ADAMS_A_CACHE) == 1 and np.array_equal(plan, plan2)
    S._ADAMS_A_CACHE.clear()
    fresh, _ = S.adams_coefficient_table(betas, taus, True)
    assert np.array_equal(again.view(np.uint32), fresh.view(np.uint32)) and not (again[:, 8:11] == 7.0).any()
    other, _ = S.adams_coefficient_table(betas, taus, True, clip=np.inf, prediction="v")
    assert np.array_equal(other[:, [2, 8, 9, 10]].view(np.uint32), fresh[:, [2, 8, 9, 10]].view(np.uint32)) and len(S._ADAMS_A_CACHE) == 1
    pred, _ = S.adams_coefficient_table(betas, taus, False)                          # the other solver, another walk: other entries
    assert len(S._ADAMS_A_CACHE) == 2 and not pred[:, 10].any() and fresh[taus[4], 10] != 0
    for K in range(30, 60):
        S.adams_coefficient_table(betas, S.logsnr_timesteps(T, K, betas), False)
    assert len(S._ADAMS_A_CACHE) <= 16


def test_shipped_second_order_tables_are_untouched(S, betas):
    """multistep_coefficient_table is not routed through the new code: its documented numbers still stand"""
    taus = S.logsnr_timesteps(T, 20, betas)
    coef, _ = S.multistep_coefficient_table(betas, taus, 2)
    assert not coef[:, 9:].any() and coef[taus[1], 8] != 0
    assert S.MULTISTEP_COLUMNS == 12 and S.ADAMS_SOLVERS == ("adams3", "adams3_pc")


# ------------------------------------------------------------------ the solver's error on the analytic model
def analytic_error(S, betas, grid, K, solver):
    """the float64 table walk of the reference ON the shipped float32 tables (no clamp) from section 18's 64 draws at t = T - 1;
    rel-L2 of the final state against the closed solution of the probability-flow ODE"""
    model, x, exact = analytic_setup(betas)
    taus = S.stride_timesteps(T, K) if grid == "uniform" else S.logsnr_timesteps(T, K, betas)
    if solver in (1, 2):
        coef, plan = S.multistep_coefficient_table(betas, taus, solver, clip=np.inf)
        out, _, _ = R.walk(model, R.table_rows(coef, plan, taus, betas), x, T)
    else:
        coef, plan = S.adams_coefficient_table(betas, taus, solver == "adams3_pc", clip=np.inf)
        out, _, _ = A.table_walk(model, A.table_rows(coef, plan, taus, betas), x, T)
    return float((out - exact).norm() / exact.norm()), len(taus)


SOLVERS = (1, 2, "adams3", "adams3_pc")


@pytest.fixture(scope="module")
def errors(S, betas):
    out = {(g, K, s): analytic_error(S, betas, g, K, s) for g in ("uniform", "logsnr") for K in (10, 20, 40, 80) for s in SOLVERS}
    for g in ("uniform", "logsnr"):
        print(f"[{g}] K (iterations): order 1 / 2M / adams3 / adams3_pc")
        for K in (10, 20, 40, 80):
            print(f"    {K} ({out[g, K, 1][1]}): " + " / ".join(f"{out[g, K, s][0]:.2e}" for s in SOLVERS))
    return {k: v[0] for k, v in out.items()}


def test_adams3_is_no_worse_than_second_order_on_the_logsnr_grid(errors):
    for K in (10, 20, 40):
        assert errors["logsnr", K, "adams3"] <= errors["logsnr", K, 2], K


def test_adams3_beats_second_order_by_five_at_twenty_steps(errors):
    assert errors["logsnr", 20, "adams3"] <= errors["logsnr", 20, 2] / 5


def test_the_corrector_helps_at_twenty_steps(errors):
    assert errors["logsnr", 20, "adams3_pc"] <= errors["logsnr", 20, "adams3"]


def test_both_reach_the_grid_floor_at_eighty_steps(errors):
    """the last steps 3 -> 1 -> 0 of the integer grid have a fixed h whatever K is: a floor of about 2e-4"""
    for s in ("adams3", "adams3_pc"):
        assert errors["logsnr", 80, s] < 5e-4, s


def test_adams3_on_the_uniform_grid_is_worse_than_order_one(errors):
    assert errors["uniform", 10, "adams3"] > errors["uniform", 10, 1]


def test_the_documented_table(errors):
    """DESIGN.md section 29 prints these numbers, rounded to three digits: half a unit of the third digit is at most 0.5 %.  The
    corrector is WORSE than the predictor alone at K = 10 and at K = 40; the table says so."""
    doc = {("logsnr", "adams3"): (2.47e-2, 1.55e-3, 1.99e-4, 2.05e-4), ("logsnr", "adams3_pc"): (4.40e-2, 7.21e-4, 2.47e-4, 1.74e-4),
           ("uniform", "adams3"): (2.22e0, 1.06e0, 3.41e-1, 9.67e-2), ("uniform", "adams3_pc"): (2.29e0, 1.05e0, 3.35e-1, 9.47e-2)}
    for (grid, solver), row in doc.items():
        for K, want in zip((10, 20, 40, 80), row):
            assert errors[grid, K, solver] == pytest.approx(want, rel=5e-3), (grid, solver, K)
    assert errors["logsnr", 10, "adams3_pc"] > errors["logsnr", 10, "adams3"]
    assert errors["logsnr", 40, "adams3_pc"] > errors["logsnr", 40, "adams3"]


# ------------------------------------------------------------------ flags and exports
BASE = ["sample_ncsn.py", "--sampling=ddpm", "--num_sigmas=1000", "--synthetic"]


def flags_for(*argv):
    import smd_amd.flags as F
    fl = F.make_flags(include_sample=True)
    fl.parse(["--sampling=ddpm", "--num_sigmas=1000", *argv])
    return fl


def test_flag_defaults_and_refusals():
    import smd_amd.flags as F
    fl = F.make_flags(include_sample=True)
    assert fl.ddim_solver == "default" and fl.ddim_order == 1
    fl.parse(["--ddim_steps=20", "--ddim_solver=adams3_pc", "--ddim_spacing=logsnr"])
    assert fl.ddim_solver == "adams3_pc"
    sys.path.insert(0, ROOT)
    sm = importlib.import_module("sample_ncsn")
    with pytest.raises(SystemExit, match="give --ddim_steps"):
        sm.main(BASE + ["--ddim_solver=adams3"])
    with pytest.raises(SystemExit, match="needs --sampling=ddpm"):
        sm.main(["sample_ncsn.py", "--ddim_steps=8", "--ddim_solver=adams3", "--sampling=ald", "--synthetic"])
    with pytest.raises(SystemExit, match="--ddim_solver=adams3 with --ddim_order=2"):
        sm.main(BASE + ["--ddim_steps=8", "--ddim_solver=adams3", "--ddim_order=2"])
    with pytest.raises(SystemExit, match="--ddim_solver=adams3_pc is a deterministic solver: it needs --ddim_eta=0"):
        sm.main(BASE + ["--ddim_steps=8", "--ddim_solver=adams3_pc", "--ddim_eta=0.5"])
    with pytest.raises(SystemExit, match="--ddim_solver=adams3 with --ddim_encode"):
        sm.main(BASE + ["--ddim_steps=8", "--ddim_solver=adams3", "--interpolate", "--ddim_encode"])
    with pytest.raises(SystemExit, match="--ddim_solver=adams3 with --analytic_variance=scalar"):
        sm.main(BASE + ["--ddim_steps=8", "--ddim_solver=adams3", "--analytic_variance=scalar"])
    with pytest.raises((SystemExit, ValueError)):
        sm.main(BASE + ["--ddim_steps=8", "--ddim_solver=adams4"])
    # what was refused before is refused as before
    with pytest.raises(SystemExit, match="--ddim_order=3: 1 .* or 2"):
        sm.main(BASE + ["--ddim_steps=8", "--ddim_order=3"])
    with pytest.raises(SystemExit, match="--ddim_order=3: 1 .* or 2"):
        sm.main(BASE + ["--ddim_steps=8", "--ddim_order=3", "--ddim_solver=adams3"])


def test_accepted_combinations_and_the_uniform_grid_warning(caplog):
    sys.path.insert(0, ROOT)
    sm = importlib.import_module("sample_ncsn")
    for argv in (["--ddim_solver=default"], ["--ddim_steps=20", "--ddim_solver=default", "--ddim_eta=1.0"],
                 ["--ddim_steps=20", "--ddim_solver=adams3", "--ddim_spacing=logsnr"],
                 ["--ddim_steps=20", "--ddim_solver=adams3_pc", "--ddim_spacing=logsnr", "--ddim_order=1"],
                 ["--ddim_steps=20", "--ddim_solver=adams3_pc", "--ddim_spacing=logsnr", "--infill"],
                 ["--ddim_steps=20", "--ddim_solver=adams3", "--ddim_spacing=logsnr", "--interpolate"]):
        with caplog.at_level(logging.WARNING, logger="smd_amd"):
            caplog.clear()
            sm.check_ddim_flags(flags_for(*argv))
            assert not caplog.records, argv
    with caplog.at_level(logging.WARNING, logger="smd_amd"):
        caplog.clear()
        sm.check_ddim_flags(flags_for("--ddim_steps=20", "--ddim_solver=adams3"))         # allowed, with a warning
        assert len(caplog.records) == 1
        msg = caplog.records[0].getMessage()
        assert "ddim_spacing=logsnr" in msg and "section 29" in msg
    # a recorded walk stands in for --ddim_steps and for the grid
    with caplog.at_level(logging.WARNING, logger="smd_amd"):
        caplog.clear()
        fl = flags_for("--ddim_solver=adams3_pc")
        fl.ddim_steps = 4
        sm.check_ddim_flags(fl, walk=[999, 600, 200, 0])
        assert not caplog.records


def test_host_walk_refusals_need_no_gpu(betas):
    import smd_amd.ncsn as N
    init = torch.zeros(1, 32, 42)
    for kw, match in ((dict(solver="adams4"), "solver="), (dict(solver="adams3", order=2), "leave order at 1"),
                      (dict(solver="adams3", eta=0.5), "eta must be 0"),
                      (dict(solver="adams3_pc", analytic=("scalar", np.ones(20))), "analytic"), (dict(order=3), "order=3")):
        with pytest.raises(ValueError, match=match):
            N.strided_dynamics(N.PRNGKey(0), None, betas, init, 20, **kw)


def test_the_exports_are_declared_and_bound():
    import smd_amd.lib as lib
    stable = lib.declared_symbols(lab=False)
    assert "smd_engine_adams_step" in stable and "smd_adams_step" in stable
    res, args = lib._SIGS["smd_engine_adams_step"]
    assert len(args) == 6 and args[2] == lib._SIGS["smd_engine_multistep_step"][1][2]     # it reuses smd_multistep_plan
    assert [n for n, _ in lib.AdamsStepArgs._fields_][:3] == ["x", "hist", "eps_hat"]
    assert len(lib.SampleIO._fields_) == 17 and lib.ABI_VERSION == 8                      # added symbols only
    text = open(os.path.join(ROOT, "symbolic-music-diffusion_amd", "csrc", "smd_kernels.h")).read()
    assert "#define SMD_MULTISTEP_COLUMNS 12 " in text
