"""Weighted training on the host: known answers of schedule.min_snr_weight and of the loss-history
tables, the identities the sampler rests on, the order of the ring, and planted faults -- each must be caught by the very
comparison tests/test_gpu_timestep.py applies to the kernels (tests/_timestep_ref.py check_*)."""
import re

import numpy as np
import pytest

import _timestep_ref as R


def _lib():
    from smd_amd import lib
    return lib


# ---------------------------------------------------------------------------------------------------- known answers
def test_min_snr_weight_known_answers():
    from smd_amd import schedule
    gamma = 5.0
    snr = np.array([0.01, 1.0, 4.999, 5.0, 5.001, 20.0, 500.0])
    ap = snr / (1.0 + snr)
    w = schedule.min_snr_weight(ap, gamma)
    assert w.dtype == np.float64
    np.testing.assert_allclose(w[snr <= gamma], 1.0, rtol=0, atol=1e-15)             # 1 where SNR <= gamma
    np.testing.assert_allclose(w[snr > gamma], gamma / snr[snr > gamma], rtol=1e-12)   # gamma / SNR above it
    np.testing.assert_allclose(w * snr, np.minimum(snr, gamma), rtol=1e-12)            # the paper's min(SNR, gamma) / SNR
    # the edges: ap = 1 is finite (0), ap = 0 is 1; gamma <= 0 and inf switch the weighting off
    assert schedule.min_snr_weight(np.array([1.0, 0.0]), gamma).tolist() == [0.0, 1.0]
    for g in (0.0, -1.0, float("inf")):
        assert schedule.min_snr_weight(ap, g).tolist() == [1.0] * len(ap)
    # the reference of the GPU tests is the same function of the noise level s = sqrt(ap)
    s = np.sqrt(ap).astype(np.float32)
    np.testing.assert_allclose(R.weight(s, None, gamma), schedule.min_snr_weight(s.astype(np.float64) ** 2, gamma), rtol=1e-15)


def test_constant_history_gives_uniform_p():
    n = 15
    h = np.full((n, R.DEPTH), 0.37, np.float32)
    p, p32, cdf, warmed = R.tables(h, np.full(n, R.DEPTH, np.int32))
    assert warmed
    np.testing.assert_allclose(p, 1.0 / n, rtol=1e-12)
    assert R.check_tables(p32, cdf, h, np.full(n, R.DEPTH)) == []


def test_twice_the_loss_twice_the_premix_probability():
    n, m = 15, float(R.MIX)
    h = np.full((n, R.DEPTH), 0.25, np.float32)
    h[4] *= 2
    p, _, _, _ = R.tables(h, np.full(n, R.DEPTH, np.int32))
    pre = (p - m / n) / (1.0 - m)                                     # undo the uniform mix
    np.testing.assert_allclose(pre[4] / pre[3], 2.0, rtol=1e-12)
    np.testing.assert_allclose(pre.sum(), 1.0, rtol=1e-12)


def test_warm_up_is_uniform():
    n = 15
    rng = np.random.default_rng(0)
    h = rng.random((n, R.DEPTH)).astype(np.float32)
    c = np.full(n, R.DEPTH, np.int32)
    c[7] = 9
    p, _, _, warmed = R.tables(h, c)
    assert not warmed and np.array_equal(p, np.full(n, 1.0 / n))


# ---------------------------------------------------------------------------------------------------- identities
@pytest.mark.parametrize("n", [15, 1000])
def test_identities(n):
    rng = np.random.default_rng(n)
    h = (rng.random((n, R.DEPTH)) * rng.random((n, 1)) * 3).astype(np.float32)
    p, p32, cdf, _ = R.tables(h, np.full(n, R.DEPTH, np.int32))
    assert abs(p.sum() - 1.0) < 1e-12                                                  # sum p = 1
    _labels, iw = R.draw(cdf, p32, np.zeros(1, np.float32), 1)
    iw_all = 1.0 / (n * p32.astype(np.float64))
    assert abs((p32.astype(np.float64) * iw_all).sum() - 1.0) < 1e-12                  # E_p[iw] = sum p / (n p) = 1
    assert (p >= float(R.MIX) / n * (1 - 1e-12)).all()                                 # the mix keeps every timestep reachable
    assert R.check_tables(p32, cdf, h, np.full(n, R.DEPTH)) == []


def test_draw_edges():
    p32 = np.array([0.25, 0.5, 0.25], np.float32)
    cdf = np.array([0.25, 0.75, 1.0], np.float32)
    below, above = np.nextafter(np.float32(0.25), np.float32(0)), np.nextafter(np.float32(0.25), np.float32(1))
    u = np.array([0.0, below, 0.25, above, np.nextafter(np.float32(1), np.float32(0))], np.float32)
    labels, iw = R.draw(cdf, p32, u, 1)
    assert labels.tolist() == [1, 1, 2, 2, 3]                          # first i with cdf[i] > u: u ON an entry takes the next one
    np.testing.assert_allclose(iw, [4 / 3, 4 / 3, 2 / 3, 2 / 3, 4 / 3], rtol=1e-12)
    short = np.array([0.25, 0.75, 1 - 2.0 ** -24], np.float32)         # a cdf that ends below 1: clamped to the last index
    assert R.draw(short, p32, u[-1:], 0)[0].tolist() == [2]


# ---------------------------------------------------------------------------------------------------- ring order
def test_ring_order_23_copies():
    n, base = 15, 1
    labels = np.full(23, 6 + base, np.int32)
    loss = np.arange(1, 24, dtype=np.float32)
    h, c = R.ring_update(np.zeros((n, R.DEPTH), np.float32), np.zeros(n, np.int32), labels, loss, base)
    assert c[6] == R.DEPTH and c.sum() == R.DEPTH
    assert h[6].tolist() == list(range(14, 24))                        # the last ten, oldest first
    assert not h[np.arange(n) != 6].any()
    # labels outside the table are dropped
    h2, c2 = R.ring_update(h, c, np.array([0, n + base], np.int32), np.ones(2, np.float32), base)
    assert np.array_equal(h2, h) and np.array_equal(c2, c)


# ---------------------------------------------------------------------------------------------------- planted faults
def _grad_case():
    rng = np.random.default_rng(1)
    B, S, C = 4, 8, 12
    pred, eps = rng.standard_normal((B, S, C)).astype(np.float32), rng.standard_normal((B, S, C)).astype(np.float32)
    snr = np.array([0.05, 5.0, 50.0, 2000.0])
    s = np.sqrt(snr / (1 + snr)).astype(np.float32)
    return pred, eps, s, np.float32(1.0 / (B * S * C))


def test_grad_check_accepts_the_reference_and_catches_inverted_snr():
    pred, eps, s, inv = _grad_case()
    g, loss, w = R.weighted_grad(pred, eps, s, None, 5.0, inv)
    assert R.check_grad(R.to_bf16(g), g)[0] == 0                       # the float64 value rounded to bf16 is inside the bound
    assert w[0] == 1.0 and w[3] < 0.01
    bad, _, _ = R.weighted_grad(pred, eps, s, None, 5.0, inv, fault="snr_inverted")
    assert R.check_grad(R.to_bf16(bad), g)[0] > 0                      # SNR / gamma instead of gamma / SNR
    # one bf16 ulp off on a single element is caught too: the bound is per element
    one = R.to_bf16(g)
    one[2, 3, 5] *= 1.0 + 2.0 ** -7
    assert R.check_grad(one, g)[0] == 1


def test_ring_overwrite_is_caught():
    n, base = 15, 0
    rng = np.random.default_rng(2)
    h0 = rng.random((n, R.DEPTH)).astype(np.float32)
    c0 = np.full(n, R.DEPTH, np.int32)
    labels, loss = np.array([3, 3], np.int32), np.array([7.0, 8.0], np.float32)
    good, _ = R.ring_update(h0, c0, labels, loss, base)
    bad, _ = R.ring_update(h0, c0, labels, loss, base, fault="ring_overwrite")
    assert good[3].tolist() == h0[3, 2:].tolist() + [7.0, 8.0]
    assert good.tobytes() != bad.tobytes()                             # the GPU test compares history byte for byte


def test_iw_without_n_and_exclusive_cdf_are_caught():
    n = 15
    rng = np.random.default_rng(3)
    h = rng.random((n, R.DEPTH)).astype(np.float32)
    c = np.full(n, R.DEPTH, np.int32)
    _, p32, cdf, _ = R.tables(h, c)
    u = rng.random(64).astype(np.float32)
    labels, iw = R.draw(cdf, p32, u, 1)
    assert R.check_draw(labels, iw.astype(np.float32), cdf, p32, u, 1) == (0, 0)
    _, iw_bad = R.draw(cdf, p32, u, 1, fault="iw_no_n")
    assert R.check_draw(labels, iw_bad.astype(np.float32), cdf, p32, u, 1)[1] == 64       # iw = 1 / p without n
    _, _, cdf_bad, _ = R.tables(h, c, fault="cdf_exclusive")
    assert "cdf end" in R.check_tables(p32, cdf_bad, h, c)                                 # an exclusive cdf ends at 1 - p[n-1]
    labels_bad, iw2 = R.draw(cdf_bad, p32, u, 1)
    assert R.check_draw(labels_bad, iw2.astype(np.float32), cdf, p32, u, 1)[0] > 0         # and shifts the labels


def test_chi2_threshold_passes_honest_draws():
    rng = np.random.default_rng(4)
    for n in (15, 1000):
        p = rng.random(n) + 0.05
        p /= p.sum()
        labels = rng.choice(n, size=65536, p=p) + 1
        q = R.chi2_quantile(n - 1)
        assert n - 1 < q < n - 1 + 12 * np.sqrt(2.0 * (n - 1)) + 40
        assert R.chi2_stat(labels, p, 1, 65536) < q
        assert R.chi2_stat(rng.integers(0, n, 65536) + 1, p, 1, 65536) > q     # uniform draws against a non-uniform p fail it


# ---------------------------------------------------------------------------------------------------- surface
def test_validate_training_options():
    from smd_amd.trainer import validate_training_options as V
    V("ddpm", "min_snr", "loss_second_moment", 1)
    V("ddpm", "min_snr", "uniform", 8)                                  # min-SNR needs no communication
    V("dsm", "none", "uniform", 8)
    with pytest.raises(ValueError, match="--loss=ddpm only"):
        V("dsm", "min_snr", "uniform", 1)
    with pytest.raises(ValueError, match="--loss=ddpm only"):
        V("dsm", "none", "loss_second_moment", 1)
    with pytest.raises(ValueError, match="single-process only"):
        V("ddpm", "none", "loss_second_moment", 2)
    with pytest.raises(ValueError, match="loss_weighting"):
        V("ddpm", "snr", "uniform", 1)


def test_flags_and_abi_surface():
    from smd_amd import flags as F
    lib = _lib()
    fl = F.make_flags(include_sample=False)
    fl.parse([])
    assert (fl.loss_weighting, fl.min_snr_gamma, fl.timestep_sampler, fl.resume) == ("none", 5.0, "uniform", False)
    fl.parse(["--loss_weighting=min_snr", "--min_snr_gamma=3", "--timestep_sampler=loss_second_moment"])
    assert (fl.loss_weighting, fl.min_snr_gamma, fl.timestep_sampler) == ("min_snr", 3.0, "loss_second_moment")
    text = open(lib.HEADER_PATH).read()
    for name in ("smd_timestep_draw", "smd_timestep_update", "smd_weighted_mse_fwd_bwd", "smd_engine_set_loss_weights",
                 "smd_engine_weight_per_sample"):
        assert name in lib._SIGS and re.search(r"\b%s\s*\(" % name, text), name
    assert lib.ABI_VERSION == 8                                        # added symbols only
