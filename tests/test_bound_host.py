"""Host side of the variational bound: the float64 tables of schedule.bound_tables against the second
form of the weights and the closed forms of tests/_bound_ref.py, the assembly of the bound from the kernels' sums, the flag
gates of sample_ncsn.py and the new exports.  No GPU."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

import _bound_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 1000
BETAS = np.linspace(np.float32(1e-6), np.float32(1e-2), T, dtype=np.float32)


@pytest.fixture(scope="module")
def S():
    import smd_amd.schedule as S
    return S


@pytest.fixture(scope="module")
def tab(S):
    return S.bound_tables(BETAS, np.arange(T))


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))))


def test_two_forms_of_the_weight_agree(tab):
    """mu1^2 / (2 bt) (bound_tables) against beta ap_prev / (2 (1-ap)(1-ap_prev)) (the reference), t >= 1, and the other scalars"""
    ref = R.tables(BETAS)
    assert rel(tab["w"][1:], ref["w"][1:]) < 1e-12
    assert rel(tab["w"][:1], ref["w"][:1]) < 1e-12
    for k in ("var_0", "decoder_const", "prior_a", "prior_c"):
        assert abs(tab[k] - ref[k]) <= 1e-12 * abs(ref[k]), k
    assert tab["table"].dtype == np.float32 and tab["table"].shape == (T, 4)
    assert np.array_equal(tab["table"], ref["table"].astype(np.float32))           # built in float64, rounded once


def test_var_0_is_the_posterior_variance_of_t_1(tab):
    beta, ap, app = R.alphas(BETAS)
    bt1 = beta[1] * (1 - app[1]) / (1 - ap[1])
    assert tab["var_0"] == bt1
    assert abs(tab["var_0"] - 9.27e-7) < 1e-9                                      # the base schedule's value
    assert abs(tab["decoder_const"] - (-6.03)) < 5e-3                              # nats per dimension: a density, negative


def test_perfect_prediction_leaves_only_the_decoder_constant(tab):
    rng = np.random.default_rng(0)
    x0 = np.clip(0.25 * rng.standard_normal((3, 32, 42)), -1, 1)
    eps = rng.standard_normal(x0.shape)
    ref = R.tables(BETAS)
    D = 32 * 42
    for t in (0, 1, 500, 999):
        q = R.three_sums(x0, eps, eps, ref["table"][t])[:, 0]
        L = R.term(ref, t, q, D)
        want = D * ref["decoder_const"] if t == 0 else 0.0
        assert np.all(np.abs(L - want) < 1e-12 * max(1.0, abs(want))), (t, L)


def test_without_clamp_the_term_is_eq_12(tab):
    """w_t q_t = beta_t / (2 alpha_t (1 - ap_{t-1})) e_t with clip = inf.  alpha_t is ap_t / ap_{t-1} of the table's own ap
    (the float32 cumulative product, promoted): that is where the identity holds to rounding.  Written with 1 - beta_t instead
    it holds to the 6e-8 by which one float32 cumprod step differs from its factor -- asserted too, at 1e-6."""
    rng = np.random.default_rng(1)
    x0 = np.clip(0.25 * rng.standard_normal((4, 32, 42)), -1, 1)
    eps = rng.standard_normal(x0.shape)
    eh = eps + 0.5 * rng.standard_normal(x0.shape)
    beta, ap, app = R.alphas(BETAS)
    ref = R.tables(BETAS)
    for t in (1, 2, 10, 500, 999):
        sums = R.three_sums(x0, eps, eh, ref["table"][t], clip=np.inf)
        mine = tab["w"][t] * sums[:, 0]
        eq12 = beta[t] / (2 * (ap[t] / app[t]) * (1 - app[t])) * sums[:, 1]
        assert rel(mine, eq12) < 1e-10, t
        assert rel(mine, beta[t] / (2 * (1 - beta[t]) * (1 - app[t])) * sums[:, 1]) < 1e-6, t


def test_prior_is_the_kl_of_two_normals(tab):
    rng = np.random.default_rng(2)
    x0 = np.clip(0.25 * rng.standard_normal((5, 32, 42)), -1, 1)
    _, ap, _ = R.alphas(BETAS)
    q = torch.distributions.Normal(torch.from_numpy(np.sqrt(ap[-1]) * x0), torch.tensor(np.sqrt(1 - ap[-1]), dtype=torch.float64))
    p = torch.distributions.Normal(torch.zeros((), dtype=torch.float64), torch.ones((), dtype=torch.float64))
    kl = torch.distributions.kl_divergence(q, p).sum(dim=(1, 2)).numpy()
    D = 32 * 42
    n = (x0 ** 2).sum(axis=(1, 2))
    assert rel(0.5 * (tab["prior_a"] * n + D * tab["prior_c"]), kl) < 1e-10
    assert rel(R.prior(R.tables(BETAS), n, D), kl) < 1e-10
    assert abs(tab["prior_a"] - 0.0066) < 1e-4                                     # the schedule does not end at 0


def test_next_t_tables(S):
    full = S.bound_tables(BETAS, np.arange(T))
    assert np.array_equal(full["next_t"], np.concatenate([np.arange(1, T), [-1]]).astype(np.int32))
    assert full["timesteps"][0] == 0 and full["timesteps"][-1] == T - 1
    for K in (2, 8, 24, 999):
        taus = S.stride_timesteps(T, K)
        tb = S.bound_tables(BETAS, taus)
        ts = tb["timesteps"]
        assert np.array_equal(ts, np.sort(taus)) and ts[0] == 0 and ts[-1] == T - 1
        assert tb["next_t"].dtype == np.int32 and tb["next_t"][T - 1] == -1
        walk, t = [], 0
        while t >= 0:
            walk.append(t)
            t = int(tb["next_t"][t])
        assert walk == [int(v) for v in ts]
        off = np.setdiff1d(np.arange(T), ts)
        assert np.all(tb["next_t"][off] == -1)
    with pytest.raises(ValueError):
        S.bound_tables(BETAS, [0, T])
    with pytest.raises(ValueError):
        S.bound_tables(BETAS, np.arange(T), clip=0.0)


def test_a_sub_sequence_has_no_total(S):
    rng = np.random.default_rng(3)
    D = 32 * 42
    full = S.bound_tables(BETAS, np.arange(T))
    sums = rng.random((T, 3, 3))
    out = S.bound_from_sums(full, sums, D)
    ref = R.tables(BETAS)
    want = np.stack([R.term(ref, t, sums[t, :, 0], D) for t in range(T)])
    assert rel(out["terms"], want) < 1e-12
    assert rel(out["total"], R.prior(ref, sums[0, :, 2], D) + want.sum(0)) < 1e-12
    assert abs(out["bits_per_dim"] - out["total"].mean() / (D * np.log(2))) < 1e-12 * abs(out["bits_per_dim"])
    assert abs(out["nats_per_dim"] - out["total"].mean() / D) < 1e-12 * abs(out["nats_per_dim"])
    assert np.array_equal(out["eps_mse"], sums[:, :, 1] / D)
    sub = S.bound_tables(BETAS, S.stride_timesteps(T, 24))
    out = S.bound_from_sums(sub, sums[:24], D)
    assert out["total"] is None and out["nats_per_dim"] is None and out["bits_per_dim"] is None
    assert out["terms"].shape == (24, 3) and out["prior"].shape == (3,) and len(out["timesteps"]) == 24
    with pytest.raises(ValueError):
        S.bound_from_sums(sub, sums[:23], D)


def test_flag_defaults_and_gates():
    import smd_amd.flags as F
    fl = F.make_flags(include_sample=True)
    assert fl.compute_bound is False and fl.bound_steps == 0 and fl.bound_only is False
    fl.parse(["--compute_bound", "--bound_steps=24", "--bound_only"])
    assert fl.compute_bound is True and fl.bound_steps == 24 and fl.bound_only is True
    sys.path.insert(0, ROOT)
    sm = importlib.import_module("sample_ncsn")
    base = ["sample_ncsn.py", "--num_sigmas=1000", "--synthetic"]
    with pytest.raises(SystemExit, match="--bound_steps: options of the variational bound, give --compute_bound"):
        sm.main(base + ["--bound_steps=24", "--sampling=ddpm", "--loss=ddpm"])
    with pytest.raises(SystemExit, match="--bound_only: options of the variational bound, give --compute_bound"):
        sm.main(base + ["--bound_only", "--sampling=ddpm", "--loss=ddpm"])
    with pytest.raises(SystemExit, match="--compute_bound: .* needs --sampling=ddpm .got --sampling=ald"):
        sm.main(base + ["--compute_bound", "--sampling=ald", "--loss=ddpm"])
    with pytest.raises(SystemExit, match="--compute_bound: .* --loss=ddpm .got --loss=dsm"):
        sm.main(base + ["--compute_bound", "--sampling=ddpm", "--loss=dsm"])
    with pytest.raises(SystemExit, match="--bound_steps=1: 0 .every timestep. or from 2 to --num_sigmas=1000"):
        sm.main(base + ["--compute_bound", "--bound_steps=1", "--sampling=ddpm", "--loss=ddpm"])
    with pytest.raises(SystemExit, match="--bound_steps=1001"):
        sm.main(base + ["--compute_bound", "--bound_steps=1001", "--sampling=ddpm", "--loss=ddpm"])


def test_the_exports_are_declared_and_bound():
    import smd_amd.lib as lib
    for name in ("smd_engine_bound_step", "smd_bound_noise", "smd_bound_terms"):
        assert name in lib.declared_symbols(lab=False) and name in lib._SIGS
    assert [n for n, _ in lib.BoundIO._fields_] == ["x0", "x_t", "eps", "t_ptr", "table", "next_t", "T", "clip", "eps_source", "seed_lo",
                                                    "seed_hi", "sample_offset", "key_ptr", "tf_keys", "tf_n_total", "partial"]
    assert lib.ABI_VERSION == 8
