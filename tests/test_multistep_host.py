"""Host side of the second-order multistep sampler (DPM-Solver++(2M)) and of the lambda-uniform grid: timestep selection and
coefficient tables against the float64 formulas of tests/_multistep_ref.py, the solver's order of convergence on an analytic
model driven by the shipped tables, the flag gates of sample_ncsn.py and the new export.  No GPU."""
import importlib
import logging
import os
import sys

import numpy as np
import pytest
import torch

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


# ------------------------------------------------------------------ the grid
@pytest.mark.parametrize("K", [2, 3, 10, 20, 40, 80, 250, 1000])
def test_logsnr_timesteps(S, betas, K):
    taus = S.logsnr_timesteps(T, K, betas)
    assert list(taus) == R.logsnr_timesteps(T, K, betas)
    assert taus[0] == T - 1 and taus[-1] == 0 and 2 <= len(taus) <= K
    assert np.all(np.diff(taus) < 0)                                   # strictly descending
    if K == 10:
        assert list(taus) == [999, 769, 487, 223, 82, 29, 10, 3, 1, 0]
    if K in (20, 40, 80):                                              # near t = 0 the snapping merges points
        assert len(taus) == {20: 18, 40: 34, 80: 63}[K]


def test_logsnr_timesteps_on_a_short_schedule(S):
    b = S.create_noise_schedule(1e-4, 0.02, 50, "linear")
    for K in (2, 8, 50):
        taus = S.logsnr_timesteps(50, K, b)
        assert list(taus) == R.logsnr_timesteps(50, K, b) and taus[0] == 49 and taus[-1] == 0 and len(taus) <= K


@pytest.mark.parametrize("K", [1, 0, T + 1])
def test_logsnr_timesteps_refuses(S, betas, K):
    with pytest.raises(ValueError):
        S.logsnr_timesteps(T, K, betas)


def test_stride_timesteps_is_untouched(S):
    assert list(S.stride_timesteps(T, 10)) == [999, 888, 777, 666, 555, 444, 333, 222, 111, 0]


# ------------------------------------------------------------------ the tables
@pytest.mark.parametrize("grid,K", [("logsnr", 10), ("logsnr", 20), ("logsnr", 80), ("uniform", 20), ("uniform", 2), ("logsnr", 3)])
@pytest.mark.parametrize("order", [1, 2])
def test_tables_equal_the_reference_formulas(S, betas, grid, K, order):
    taus = S.logsnr_timesteps(T, K, betas) if grid == "logsnr" else S.stride_timesteps(T, K)
    n = len(taus)
    coef, plan = S.multistep_coefficient_table(betas, taus, order)
    assert coef.dtype == np.float32 and coef.shape == (T, 12) and plan.dtype == np.int32 and plan.shape == (T, 4)
    assert coef.strides[0] % 16 == 0
    ref = R.coefficients(betas, list(taus), order)
    # the paper's (ratio, gain, 1/(2r)) in the engine's columns: b = ratio, a0 = gain (1 + 1/(2r)), a1 = -gain / (2r)
    want = np.stack([ref["sqrt_recip"], ref["sqrt_m1"], ref["gain"] * (1 + ref["inv2r"]), ref["ratio"], np.zeros(n), ref["clip"],
                     ref["sqrt_as"], ref["sqrt_1m_as"], -ref["gain"] * ref["inv2r"]], axis=1)
    got = coef[taus, :9].astype(np.float64)
    # one float32 rounding of a float64 value (columns 0 / 1 are float32 expressions: two roundings); a and gain are the same
    # number computed as a difference and through expm1, so they agree to float64 cancellation, far inside 1e-6
    assert np.all(np.abs(got - want) <= 1e-6 * np.abs(want)), np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300))
    assert not coef[:, 9:].any() and not coef[:, 4].any()
    # the plan is the strided walk's, unchanged; rows off the walk are zero / -1
    base, base_plan = S.strided_coefficient_table(betas, taus, 0.0)
    assert np.array_equal(plan, base_plan)
    off = np.setdiff1d(np.arange(T), taus)
    assert not coef[off].any() and np.all(plan[off, :3] == -1)
    # no history on the first iteration, a first-order step that returns x0 on the last
    a1 = coef[taus, 8]
    assert a1[0] == 0 and a1[-1] == 0 and not np.signbit(a1[[0, -1]]).any()
    assert tuple(coef[0, [2, 3, 8]]) == (1.0, 0.0, 0.0)
    if order == 1:
        assert np.array_equal(coef[:, :8].view(np.uint32), base.view(np.uint32))        # the strided table, to the bit
        assert not coef[:, 8].any()
    elif n > 2:
        assert np.all(a1[1:-1] < 0) and np.all(coef[taus[1:-1], 2] > base[taus[1:-1], 2])
    co = S.multistep_coefficients(betas, taus, order)
    sc = S.strided_coefficients(betas, taus, 0.0)
    assert np.array_equal(co["b"], sc["b"]) and np.allclose(co["a0"] + co["a1"], sc["a"], rtol=1e-14, atol=0)
    if order == 1:
        assert np.array_equal(co["a0"], sc["a"]) and not co["a1"].any() and not co["w"].any()


def test_refuses_other_orders(S, betas):
    for order in (0, 3):
        with pytest.raises(ValueError, match="order"):
            S.multistep_coefficient_table(betas, S.stride_timesteps(T, 10), order)


def test_history_weight_on_an_exactly_uniform_lambda_schedule_is_one_half(S):
    """a toy schedule whose lambdas are exactly evenly spaced: ap_t = sigmoid(2 lambda_t), lambda linear in t -> every h equal"""
    n = 64
    lam = np.linspace(3.0, -3.0, n)
    ap = 1 / (1 + np.exp(-2 * lam))
    betas = 1 - ap / np.concatenate([[1.0], ap[:-1]])
    taus = S.logsnr_timesteps(n, 8, betas)
    assert list(taus) == list(S.stride_timesteps(n, 8))                # uniform in lambda IS uniform in t here
    co = S.multistep_coefficients(betas, taus, 2)
    assert co["w"][0] == 0 and co["w"][-1] == 0
    # the tables start from the FLOAT32 cumulative product: n roundings of 2^-24 in ap move lambda = (log ap - log(1 - ap)) / 2
    # by at most n 2^-24 / (2 (1 - ap_0)), an h (two lambdas) by twice that, w (two h) by twice that again, relatively
    h = 6.0 / 7
    tol = n * 2.0 ** -24 / (1 - ap[0]) / h
    assert tol < 2e-3
    assert np.isinf(co["h"][-1]) and np.all(np.abs(co["h"][:-1] / h - 1) <= tol)
    assert np.all(np.abs(co["w"][1:-1] / 0.5 - 1) <= 2 * tol)
    # ... and on the project's schedule a uniform-in-t grid weighs the history up to 3.7 (the documented finding)
    pb = S.create_noise_schedule(1e-6, 0.01, T, "linear")
    w = S.multistep_coefficients(pb, S.stride_timesteps(T, 10), 2)["w"]
    assert 3.6 < w.max() < 3.8


# ------------------------------------------------------------------ the solver's order, on an analytic model
S2 = np.array([0.01, 0.0625, 0.25, 1.0])


def analytic_error(S, betas, grid, K, order):
    """independent Gaussian data with variances S2: the exact eps_hat is sqrt(1 - ap_t) x / (ap_t s^2 + 1 - ap_t) and the
    probability-flow ODE has the closed solution x_s = x_t sqrt((ap_s s^2 + 1 - ap_s) / (ap_t s^2 + 1 - ap_t)).  The float64
    walk of the reference runs ON the shipped float32 tables (no clamp) from 64 draws at t = T - 1; rel-L2 of the final state."""
    ap = R.alphas_prod(betas)
    s2 = torch.from_numpy(S2)
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((64, 4)))

    def model(x, cond):
        a = cond ** 2
        return torch.sqrt(1 - a) * x / (a * s2 + 1 - a)

    exact = x * torch.sqrt(s2 / (ap[-1] * s2 + 1 - ap[-1]))             # ap_s = 1 at the end of the walk
    taus = S.stride_timesteps(T, K) if grid == "uniform" else S.logsnr_timesteps(T, K, betas)
    coef, plan = S.multistep_coefficient_table(betas, taus, order, clip=np.inf)
    out, _, _ = R.walk(model, R.table_rows(coef, plan, taus, betas), x, T)
    return float((out - exact).norm() / exact.norm()), len(taus)


@pytest.fixture(scope="module")
def errors(S, betas):
    out = {(g, K, o): analytic_error(S, betas, g, K, o) for g in ("uniform", "logsnr") for K in (10, 20, 40, 80) for o in (1, 2)}
    for g in ("uniform", "logsnr"):
        print(f"[{g}] K (iterations): order 1 / order 2 = " +
              ", ".join(f"{K} ({out[g, K, 1][1]}): {out[g, K, 1][0]:.2e} / {out[g, K, 2][0]:.2e}" for K in (10, 20, 40, 80)))
    return {k: v[0] for k, v in out.items()}


def test_order_two_on_the_logsnr_grid_beats_order_one_by_four(errors):
    for K in (10, 20, 40, 80):
        assert errors["logsnr", K, 2] <= errors["logsnr", K, 1] / 4, K


def test_order_two_converges_quadratically(errors):
    for K in (20, 40):
        assert errors["logsnr", K, 2] / errors["logsnr", 2 * K, 2] >= 3.0, K


def test_order_one_converges_linearly(errors):
    for grid in ("uniform", "logsnr"):
        for K in (10, 20, 40):
            assert 1.8 <= errors[grid, K, 1] / errors[grid, 2 * K, 1] <= 2.2, (grid, K)


def test_order_two_on_the_uniform_grid_is_worse_than_order_one(errors):
    assert errors["uniform", 10, 2] > errors["uniform", 10, 1]


def test_the_documented_table(errors):
    """DESIGN.md section 18 prints these numbers, rounded to three digits: half a unit of the third digit is at most 0.5 %"""
    doc = {("uniform", 1): (1.64e-1, 8.29e-2, 4.16e-2, 2.09e-2), ("uniform", 2): (4.48e-1, 1.82e-1, 6.79e-2, 2.36e-2),
           ("logsnr", 1): (2.29e-1, 1.16e-1, 5.82e-2, 2.92e-2), ("logsnr", 2): (3.66e-2, 1.35e-2, 3.52e-3, 9.10e-4)}
    for (grid, order), row in doc.items():
        for K, want in zip((10, 20, 40, 80), row):
            assert errors[grid, K, order] == pytest.approx(want, rel=5e-3), (grid, order, K)


# ------------------------------------------------------------------ flags and export
def test_flag_defaults_and_gates(caplog):
    import smd_amd.flags as F
    fl = F.make_flags(include_sample=True)
    assert fl.ddim_order == 1 and fl.ddim_spacing == "uniform"
    fl.parse(["--ddim_steps=50", "--ddim_order=2", "--ddim_spacing=logsnr"])
    assert fl.ddim_order == 2 and fl.ddim_spacing == "logsnr"
    sys.path.insert(0, ROOT)
    sm = importlib.import_module("sample_ncsn")
    base = ["sample_ncsn.py", "--sampling=ddpm", "--num_sigmas=1000", "--synthetic"]
    with pytest.raises(SystemExit, match="give --ddim_steps"):
        sm.main(base + ["--ddim_order=2"])
    with pytest.raises(SystemExit, match="give --ddim_steps"):
        sm.main(base + ["--ddim_spacing=logsnr"])
    with pytest.raises(SystemExit, match="--ddim_order=3: 1 .* or 2"):
        sm.main(base + ["--ddim_steps=8", "--ddim_order=3"])
    with pytest.raises(SystemExit, match="--ddim_order=0"):
        sm.main(base + ["--ddim_steps=8", "--ddim_order=0"])
    with pytest.raises(SystemExit, match="needs --ddim_eta=0"):
        sm.main(base + ["--ddim_steps=8", "--ddim_order=2", "--ddim_eta=0.5"])
    with pytest.raises(SystemExit, match="--ddim_order=2 with --ddim_encode"):
        sm.main(base + ["--ddim_steps=8", "--ddim_order=2", "--interpolate", "--ddim_encode"])
    with pytest.raises(SystemExit, match="needs --sampling=ddpm"):
        sm.main(["sample_ncsn.py", "--ddim_steps=8", "--ddim_order=2", "--sampling=ald", "--synthetic"])
    with pytest.raises((SystemExit, ValueError)):
        sm.main(base + ["--ddim_steps=8", "--ddim_spacing=cosine"])


def flags_for(*argv):
    import smd_amd.flags as F
    fl = F.make_flags(include_sample=True)
    fl.parse(["--sampling=ddpm", "--num_sigmas=1000", *argv])
    return fl


def test_check_ddim_flags_accepts_what_it_accepted_and_the_new_combinations(caplog):
    sys.path.insert(0, ROOT)
    sm = importlib.import_module("sample_ncsn")
    for argv in ([], ["--ddim_steps=50"], ["--ddim_steps=50", "--ddim_eta=1.0"], ["--ddim_steps=50", "--interpolate", "--ddim_encode"],
                 ["--ddim_order=1", "--ddim_spacing=uniform"],                           # the defaults, spelled out, without a walk
                 ["--ddim_steps=8", "--ddim_order=1", "--ddim_spacing=uniform"], ["--ddim_steps=8", "--ddim_order=2", "--ddim_spacing=logsnr"],
                 ["--ddim_steps=8", "--ddim_order=1", "--ddim_spacing=logsnr", "--ddim_eta=0.5"],
                 ["--ddim_steps=8", "--ddim_order=2", "--ddim_spacing=logsnr", "--infill"],
                 ["--ddim_steps=8", "--ddim_order=2", "--ddim_spacing=logsnr", "--interpolate"]):
        with caplog.at_level(logging.WARNING, logger="smd_amd"):
            caplog.clear()
            sm.check_ddim_flags(flags_for(*argv))
            assert not caplog.records, argv
    with caplog.at_level(logging.WARNING, logger="smd_amd"):
        caplog.clear()
        sm.check_ddim_flags(flags_for("--ddim_steps=8", "--ddim_order=2"))               # allowed, with a warning
        assert len(caplog.records) == 1 and "ddim_spacing=logsnr" in caplog.records[0].getMessage()


def test_the_export_is_declared_and_bound():
    import smd_amd.lib as lib
    assert "smd_engine_multistep_step" in lib.declared_symbols(lab=False)
    res, args = lib._SIGS["smd_engine_multistep_step"]
    assert len(args) == 6 and [n for n, _ in lib.MultistepPlan._fields_] == ["coef", "plan", "T"]
    assert [n for n, _ in lib.SampleIO._fields_][-1] == "key_ptr" and len(lib.SampleIO._fields_) == 17   # no field was added
    assert lib.ABI_VERSION == 8                                        # an added symbol only
