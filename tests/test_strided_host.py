"""Host side of the strided (DDIM) sampler: timestep selection, coefficient tables and plans against the float64 formulas of
tests/_strided_ref.py, the flag gates of sample_ncsn.py and the new export.  No GPU."""
import importlib
import os
import sys

import numpy as np
import pytest

import _strided_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 1000


@pytest.fixture(scope="module")
def S():
    import smd_amd.schedule as S
    return S


@pytest.fixture(scope="module")
def betas(S):
    return S.create_noise_schedule(1e-6, 0.01, T, "linear")


@pytest.mark.parametrize("K", [2, 3, 8, 20, 50, 250, 999, 1000])
def test_stride_timesteps(S, K):
    taus = S.stride_timesteps(T, K)
    assert list(taus) == R.timesteps(T, K)
    assert len(taus) == K and taus[0] == T - 1 and taus[-1] == 0
    assert np.all(np.diff(taus) < 0)                                   # descending and unique
    if K == T:
        assert list(taus) == list(range(T - 1, -1, -1))


@pytest.mark.parametrize("K", [1, 0, T + 1])
def test_stride_timesteps_refuses(S, K):
    with pytest.raises(ValueError):
        S.stride_timesteps(T, K)


@pytest.mark.parametrize("K,eta", [(20, 0.0), (20, 0.7), (20, 1.0), (7, 1.0), (1000, 1.0), (2, 0.3)])
def test_strided_tables_equal_the_reference_formulas(S, betas, K, eta):
    taus = S.stride_timesteps(T, K)
    coef, plan = S.strided_coefficient_table(betas, taus, eta)
    assert coef.dtype == np.float32 and coef.shape == (T, 8) and plan.dtype == np.int32 and plan.shape == (T, 4)
    ref = R.descending(betas, list(taus), eta)
    cols = ("sqrt_recip", "sqrt_m1", "a", "b", "sigma", "clip", "sqrt_as", "sqrt_1m_as")
    want = np.stack([ref[c] for c in cols], axis=1)
    got = coef[taus].astype(np.float64)
    # one float32 rounding of a float64 value (columns 0 / 1 are float32 expressions: two roundings)
    assert np.all(np.abs(got - want) <= 1e-6 * np.abs(want)), np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300))
    assert np.array_equal(coef[taus, :2], S.reverse_coefficient_table(betas)[taus, :2])
    off = np.setdiff1d(np.arange(T), taus)
    assert not coef[off].any() and np.all(plan[off, 0] == -1) and np.all(plan[off, 1] == -1)
    assert list(plan[taus, 0]) == list(taus[1:]) + [-1]
    assert list(plan[taus, 1]) == list(range(K)) and not plan[:, 3].any()
    # the last iteration returns x0; eta = 0 draws nothing
    assert tuple(coef[0, 2:5]) == (1.0, 0.0, 0.0)
    if eta == 0.0:
        assert not coef[:, 4].any()
    else:
        assert np.all(coef[taus[:-1], 4] > 0)


def test_full_length_eta_one_is_the_ddpm_posterior(S, betas):
    """K = T, eta = 1: (sigma^2, a, b) are the posterior's (beta~, mu1, mu2) -- the algebraic identity, in float64 from the same
    alphas with beta_t := 1 - ap_t / ap_{t-1}."""
    taus = S.stride_timesteps(T, T)
    co = S.strided_coefficients(betas, taus, 1.0)
    ap = R.alphas_prod(betas)[taus]
    ap_prev = np.append(ap[1:], 1.0)
    beta = 1 - ap / ap_prev
    var = beta * (1 - ap_prev) / (1 - ap)
    mu1 = beta * np.sqrt(ap_prev) / (1 - ap)
    mu2 = (1 - ap_prev) * np.sqrt(1 - beta) / (1 - ap)
    for got, want in ((co["sigma"] ** 2, var), (co["a"], mu1), (co["b"], mu2)):
        assert np.all(np.abs(got - want) <= 1e-9 * np.abs(want) + 1e-300)


@pytest.mark.parametrize("K", [2, 8, 20, 39, 40, 41, 100, 1000])
def test_plan_slots_are_the_reference_bookkeeping_reversed(S, betas, K):
    taus = S.stride_timesteps(T, K)
    _, plan = S.strided_coefficient_table(betas, taus, 0.0)
    assert list(plan[taus, 2]) == list(S.collection_slot_table(K)[::-1]) == R.slots(K)
    assert np.all(plan[:, 2] <= 40)


@pytest.mark.parametrize("K", [2, 20, 1000])
def test_inversion_table(S, betas, K):
    taus = S.stride_timesteps(T, K)
    coef, plan = S.inversion_coefficient_table(betas, taus)
    ref = R.ascending(betas, list(taus))
    asc = np.asarray(sorted(taus))[:-1]
    want = np.stack([ref[c] for c in ("sqrt_recip", "sqrt_m1", "a", "b", "sigma", "clip", "sqrt_as", "sqrt_1m_as")], axis=1)
    got = coef[asc].astype(np.float64)
    assert np.all(np.isposinf(got[:, 5])) and np.all(np.isposinf(want[:, 5]))
    got, want = np.delete(got, 5, axis=1), np.delete(want, 5, axis=1)
    assert np.all(np.abs(got - want) <= 1e-6 * np.abs(want))
    assert list(plan[asc, 0]) == list(np.asarray(sorted(taus))[1:-1]) + [T]          # ends out of range: the walk stops by itself
    assert list(plan[asc, 1]) == list(range(K - 1)) and np.all(plan[:, 2] == -1)
    assert not coef[T - 1].any() and plan[T - 1, 1] == -1                          # no step is executed at T - 1
    assert not coef[:, 4].any()


def test_flag_defaults_and_gates():
    import smd_amd.flags as F
    fl = F.make_flags(include_sample=True)
    assert fl.ddim_steps == 0 and fl.ddim_eta == 0.0 and fl.ddim_encode is False
    fl.parse(["--ddim_steps=50", "--ddim_eta=0.5", "--ddim_encode"])
    assert fl.ddim_steps == 50 and fl.ddim_eta == 0.5 and fl.ddim_encode is True
    sys.path.insert(0, ROOT)
    sm = importlib.import_module("sample_ncsn")
    with pytest.raises(SystemExit, match="needs --sampling=ddpm"):
        sm.main(["sample_ncsn.py", "--ddim_steps=50", "--sampling=ald", "--synthetic"])
    with pytest.raises(SystemExit, match="--ddim_steps=1: 0 .every timestep. or from 2 to --num_sigmas=1000"):
        sm.main(["sample_ncsn.py", "--ddim_steps=1", "--sampling=ddpm", "--num_sigmas=1000", "--synthetic"])
    with pytest.raises(SystemExit, match="--ddim_steps=1001"):
        sm.main(["sample_ncsn.py", "--ddim_steps=1001", "--sampling=ddpm", "--num_sigmas=1000", "--synthetic"])
    with pytest.raises(SystemExit, match="give --ddim_steps"):
        sm.main(["sample_ncsn.py", "--ddim_eta=0.5", "--sampling=ddpm", "--num_sigmas=1000", "--synthetic"])
    with pytest.raises(SystemExit, match="needs --interpolate"):
        sm.main(["sample_ncsn.py", "--ddim_steps=8", "--ddim_encode", "--sampling=ddpm", "--num_sigmas=1000", "--synthetic"])


def test_the_export_is_declared_and_bound():
    import smd_amd.lib as lib
    assert "smd_engine_strided_step" in lib.declared_symbols(lab=False)
    res, args = lib._SIGS["smd_engine_strided_step"]
    assert len(args) == 5 and [n for n, _ in lib.StridePlan._fields_] == ["coef", "plan", "T"]
    assert lib.ABI_VERSION == 8                                        # an added symbol only
