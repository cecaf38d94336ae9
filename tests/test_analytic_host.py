"""Host side of --analytic_variance: the optimal reverse variance of Bao et al. 2022 in closed form,
the bound with it, the moment tables, the flags and the sidecar.  No GPU.

The references are tests/_analytic_ref.py (written from the paper, independently of smd_amd/schedule.py) and, for the Gaussian
case, the exact law: for x0 ~ N(0, diag(v)) the true reverse process is Gaussian with a state-independent variance, so the
optimal variance reproduces every marginal exactly.
"""
import importlib
import os
import sys
import types

import numpy as np
import pytest

import _analytic_ref as A
import _strided_ref as R
import ddpm_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 1000
BETAS = O.create_noise_schedule(1e-6, 0.01, T, "linear")
V = np.array([1e-3, 0.04, 0.3, 1.0, 4.0])        # per-element data variances: far from exchangeable, on both sides of 1


def test_ddpm_identity_on_adjacent_timesteps():
    """lam^2 = bt_t on adjacent timesteps: sig2 = (beta_t / alpha_t) (1 - beta_t g_t / bb_t), relative 1e-12.  alpha_t is
    ap_t / ap_(t-1) of the float32 cumulative product every table starts from (and beta_t = 1 - alpha_t): the float32 betas
    themselves are not the ratios of that product to better than 1e-7 / beta."""
    import smd_amd.schedule as S
    ap = R.alphas_prod(BETAS)
    taus = np.arange(T)[::-1]
    g = np.random.default_rng(0).uniform(0, 1, T)                    # row j: timestep taus[j]
    s2 = S.analytic_variance(BETAS, taus, 1.0, g, clip=np.inf)
    t = taus[:-1]
    alpha = ap[t] / ap[t - 1]
    beta = 1 - alpha
    want = (beta / alpha) * (1 - beta * g[:-1] / (1 - ap[t]))
    assert np.max(np.abs(s2[:-1] - want) / want) <= 1e-12
    assert s2[-1] == 0.0
    np.testing.assert_allclose(s2, A.variance(BETAS, taus, 1.0, g), rtol=1e-12, atol=0)


@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_bounds_and_clip_cap(eta):
    import smd_amd.schedule as S
    taus = S.stride_timesteps(T, 10)
    K = len(taus)
    co = S.strided_coefficients(BETAS, taus, eta)
    lam2 = co["sigma"] ** 2
    ap = R.alphas_prod(BETAS)
    at, as_ = ap[taus], np.append(ap[taus[1:]], 1.0)
    h = np.sqrt((1 - at) * as_ / at) - np.sqrt(np.maximum(1 - as_ - lam2, 0))
    one = S.analytic_variance(BETAS, taus, eta, np.ones(K), clip=np.inf)
    np.testing.assert_allclose(one[:-1], lam2[:-1], rtol=1e-15, atol=0)                      # g = 1: lam^2
    zero = S.analytic_variance(BETAS, taus, eta, np.zeros(K), clip=np.inf)
    np.testing.assert_allclose(zero[:-1], (lam2 + h ** 2)[:-1], rtol=1e-15, atol=0)          # g = 0: the Theorem 2 upper bound
    # g outside [0, 1] is clipped to it
    np.testing.assert_array_equal(S.analytic_variance(BETAS, taus, eta, np.full(K, 1.7), clip=np.inf), one)
    np.testing.assert_array_equal(S.analytic_variance(BETAS, taus, eta, np.full(K, -0.2), clip=np.inf), zero)
    # the cap lam^2 + a^2 clip^2: it binds exactly where h^2 (1 - g) > a^2 clip^2
    for clip in (1.0, 0.05):
        capped = S.analytic_variance(BETAS, taus, eta, np.zeros(K), clip=clip)
        cap = lam2 + (co["a"] * clip) ** 2
        binds = (h ** 2 > (co["a"] * clip) ** 2)[:-1]
        np.testing.assert_allclose(capped[:-1], np.minimum(zero, cap)[:-1], rtol=1e-15, atol=0)
        assert np.array_equal(capped[:-1] < zero[:-1], binds)
        if clip == 0.05:
            assert binds.any()                   # the cap engages on this walk (the high-noise end) ...
    assert not (zero[:-1] > lam2[:-1] + co["a"][:-1] ** 2 * 1e12).any()                       # ... and a huge clip never does
    assert all(v[-1] == 0 for v in (one, zero, capped))
    # element mode broadcasts per element, shapes kept
    ge = np.random.default_rng(1).uniform(0, 1, (K, 3, 5))
    se = S.analytic_variance(BETAS, taus, eta, ge, clip=1.0)
    assert se.shape == (K, 3, 5)
    np.testing.assert_allclose(se, A.variance(BETAS, taus, eta, ge, clip=1.0), rtol=1e-12, atol=0)
    tab = S.analytic_sigma_table(BETAS, taus, eta, ge)
    assert tab.dtype == np.float32 and tab.shape == (K, 3, 5)
    np.testing.assert_array_equal(tab, np.sqrt(se).astype(np.float32))
    with pytest.raises(ValueError, match="walk of"):
        S.analytic_variance(BETAS, taus, eta, np.ones(K + 1))


@pytest.mark.parametrize("K", [5, 10, 50])
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_gaussian_data_in_closed_form(K, eta):
    """x0 ~ N(0, diag(v)) with the exact score: the element-mode variance reproduces Var(x_s) = ap_s v + bb_s after every iteration
    that produces a noisy level (the last iteration has sigma = 0 by the walks' convention and returns the posterior mean, whose
    variance is below v), to 1e-10 relative; the plain sigma_eta misses it."""
    import smd_amd.schedule as S
    taus = S.stride_timesteps(T, K)
    ap = R.alphas_prod(BETAS)
    g = A.gaussian_g(ap[taus][:, None], V[None, :])
    s2 = S.analytic_variance(BETAS, taus, eta, g, clip=np.inf)
    got, want = A.gaussian_walk_variances(BETAS, taus, eta, V, s2)
    assert np.max(np.abs(got[:-1] - want[:-1]) / want[:-1]) <= 1e-10
    plain = np.broadcast_to((S.strided_coefficients(BETAS, taus, eta)["sigma"] ** 2)[:, None], g.shape)
    pg, pw = A.gaussian_walk_variances(BETAS, taus, eta, V, plain)
    miss = np.max(np.abs(pg[:-1] - pw[:-1]) / pw[:-1])
    if K == 10:
        assert miss > 1e-3, miss
    assert (pg[:-1] <= pw[:-1] * (1 + 1e-12)).all()                  # and always from below: under-dispersed samples
    # scalar mode is exact when v is constant
    vc = np.full(4, 0.3)
    gs = A.gaussian_g(ap[taus], 0.3)
    sc = S.analytic_variance(BETAS, taus, eta, gs, clip=np.inf)
    got, want = A.gaussian_walk_variances(BETAS, taus, eta, vc, sc[:, None] * np.ones((1, 4)))
    assert np.max(np.abs(got[:-1] - want[:-1]) / want[:-1]) <= 1e-10
    np.testing.assert_allclose(S.analytic_scalar_g(np.broadcast_to(gs[:, None, None], (len(taus), 2, 3))), gs, rtol=1e-15)


def _gaussian_sums(taus_asc, v, D_rep, N=3):
    """sums [K][N][3] whose q_t is D E[(x0 - x0_hat)^2] of the Gaussian case: x0 - x0_hat = sqrt(bb / ap) (eps_hat - eps), and
    E[(eps - eps_hat)^2] = 1 - g for the exact score"""
    ap = R.alphas_prod(BETAS)[taus_asc]
    g = A.gaussian_g(ap, v)
    q = D_rep * (1 - ap) / ap * (1 - g)
    sums = np.zeros((len(taus_asc), N, 3))
    sums[:, :, 0] = q[:, None] * np.array([0.7, 1.0, 1.3])[None, :N]
    sums[:, :, 1] = D_rep * (1 - g)[:, None]
    sums[:, :, 2] = D_rep * v
    return sums, g


@pytest.mark.parametrize("K", [0, 24])
def test_bound_with_the_optimal_variance(K):
    import smd_amd.schedule as S
    D = 64
    ts = np.arange(T) if K == 0 else S.stride_timesteps(T, K)
    tab = S.bound_tables(BETAS, ts)
    asc = tab["timesteps"]
    taus = asc[::-1]
    sums, g_asc = _gaussian_sums(asc, 0.3, D)
    plain = S.bound_from_sums(tab, sums, D)
    # g = 1: the model's variance is the posterior's, the terms are bound_from_sums' (a^2 / (2 lam^2) = mu1^2 / (2 bt) on adjacent
    # timesteps; a strided walk has its own a and lam, so only K = T is compared)
    at1 = S.analytic_bound_from_sums(tab, sums, D, np.ones(len(asc)), taus, BETAS)
    assert np.isfinite(at1["total"]).all() and at1["total"].shape == (3,)
    np.testing.assert_array_equal(at1["sigma2_ratio"], np.ones(len(asc)))
    if K == 0:
        np.testing.assert_allclose(at1["terms"], plain["terms"], rtol=1e-9, atol=0)
        np.testing.assert_allclose(at1["total"], plain["total"], rtol=1e-9, atol=0)
    else:
        assert plain["total"] is None                               # the fixed variance gives no total for a sub-sequence ...
        assert isinstance(at1["bits_per_dim"], float)               # ... the K-step chain has one
    # sig2 optimal for the supplied q: with g' = 1 - q a^2 / (D h^2) the KL's minimiser lam^2 + a^2 q / D is the analytic form
    p = S._analytic_parts(BETAS, taus, 1.0)
    q_desc = sums[::-1, 1, 0]                                          # example 1 carries the exact Gaussian q
    g_opt = 1 - q_desc * p["a"] ** 2 / (D * p["h"] ** 2)
    g_opt[-1] = 1.0
    one_example = sums[:, 1:2, :]
    opt = S.analytic_bound_from_sums(tab, one_example, D, g_opt, taus, BETAS)
    base = S.analytic_bound_from_sums(tab, one_example, D, np.ones(len(asc)), taus, BETAS)
    assert (opt["terms"][1:] <= base["terms"][1:] * (1 + 1e-12) + 1e-12).all()
    assert (opt["terms"][1:] < base["terms"][1:]).any()
    np.testing.assert_array_equal(opt["terms"][0], base["terms"][0])  # the decoder term keeps var_0
    if K == 0:
        assert (opt["terms"][1:] <= plain["terms"][1:, 1:2] * (1 + 1e-9) + 1e-12).all()
    # any other variance is worse than the optimum for that q
    for other in (np.clip(g_opt * 0.5, 0, 1), np.clip(0.5 + 0.5 * g_opt, 0, 1)):
        o = S.analytic_bound_from_sums(tab, one_example, D, other, taus, BETAS)
        assert (o["terms"][1:] >= opt["terms"][1:] - 1e-9 * np.abs(opt["terms"][1:]) - 1e-12).all()
    with pytest.raises(ValueError, match="descending"):
        S.analytic_bound_from_sums(tab, sums, D, np.ones(len(asc)), asc, BETAS)
    with pytest.raises(ValueError, match="scalar mode"):
        S.analytic_bound_from_sums(tab, sums, D, np.ones((len(asc), 2)), taus, BETAS)
    # the existing functions return what they returned: the keys of both dicts, spelled out
    assert set(tab) == {"w", "var_0", "decoder_const", "prior_a", "prior_c", "table", "next_t", "timesteps", "clip"}
    assert set(plain) == {"timesteps", "terms", "eps_mse", "prior", "total", "nats_per_dim", "bits_per_dim", "var_0"}
    with pytest.raises(ValueError, match="betas for tables"):
        S.analytic_bound_from_sums(tab, sums, D, np.ones(len(asc)), taus, BETAS[:-1])


def test_the_two_forms_of_the_variance_agree_at_every_timestep():
    """At K = T ``analytic_bound_from_sums`` takes a = mu1, lam^2 = bt and h^2 = beta^2 / (alpha bb) from the float32 betas, as
    ``bound_tables`` does, and ``analytic_variance`` takes them from ratios of the float32 cumulative product.  The two are the
    same quantity up to how well those betas are the product's ratios: 1 - ap_t / ap_(t-1) carries the product's 2^-24 relative
    rounding, i.e. a relative error of up to ~2^-23 / beta_t in beta, and sig2 / lam^2 inherits it.  Checked as that bound, and
    exactly where it is tight: at g = 1 the ratio is 1 in both forms."""
    import smd_amd.schedule as S
    D = 8
    tab = S.bound_tables(BETAS, np.arange(T))
    taus = np.arange(T)[::-1]
    g = np.random.default_rng(7).uniform(0, 1, T)
    sums = np.ones((T, 1, 3))
    ratio = S.analytic_bound_from_sums(tab, sums, D, g, taus, BETAS)["sigma2_ratio"][::-1]       # by iteration
    lam2 = S.strided_coefficients(BETAS, taus, 1.0)["sigma"] ** 2
    other = S.analytic_variance(BETAS, taus, 1.0, g, clip=np.inf)[:-1] / lam2[:-1]
    b64 = BETAS.astype(np.float64)[taus[:-1]]
    # a few roundings of the cumulative product reach beta: the product at t and t - 1, and alpha_t = 1 - beta_t itself in float32
    bound = 8 * 2.0 ** -23 / b64
    rel_err = np.abs(ratio[:-1] - other) / other
    assert (rel_err <= bound).all(), float((rel_err / bound).max())
    assert float(np.median(rel_err)) < 1e-4                          # and at most timesteps it is far inside it
    one = S.analytic_bound_from_sums(tab, sums, D, np.ones(T), taus, BETAS)["sigma2_ratio"]
    np.testing.assert_array_equal(one, np.ones(T))


@pytest.mark.parametrize("kind", ["eps", "x0", "v"])
def test_moment_tables_recover_eps(kind):
    import smd_amd.schedule as S
    ts = S.stride_timesteps(T, 20)
    table, next_t = S.analytic_moment_tables(BETAS, ts, kind)
    assert table.dtype == np.float32 and table.shape == (T, 4) and not table[:, 2:].any()
    asc = np.unique(ts)
    assert next_t.dtype == np.int32 and list(next_t[asc]) == list(asc[1:]) + [-1]
    assert (np.delete(next_t, asc) == -1).all()
    if kind == "eps":
        assert (table[:, 0] == 0).all() and (table[:, 1] == 1).all()
    # float64 closed forms (what the table rounds once): A x_t + B out is eps to 1e-12 on synthetic (x0, eps)
    ap = R.alphas_prod(BETAS)
    rng = np.random.default_rng(3)
    x0, eps = np.clip(0.25 * rng.standard_normal(64), -1, 1), rng.standard_normal(64)
    worst = 0.0
    for t in (0, 1, 500, 999):
        sa, s1 = np.sqrt(ap[t]), np.sqrt(1 - ap[t])
        xt = sa * x0 + s1 * eps
        out = {"eps": eps, "x0": x0, "v": sa * eps - s1 * x0}[kind]
        Ab = {"eps": (0.0, 1.0), "x0": (1 / s1, -sa / s1), "v": (s1, sa)}[kind]
        np.testing.assert_array_equal(table[t, :2], np.asarray(Ab, dtype=np.float32))
        # the x0 form divides the cancelling x_t - sqrt(ap) x0 by sqrt(bb): its conditioning, not the table's, sets the error
        scale = np.abs(Ab[0] * xt) + np.abs(Ab[1] * out)
        worst = max(worst, float(np.max(np.abs(Ab[0] * xt + Ab[1] * out - eps) / scale)))
        np.testing.assert_allclose(A.eps_units(kind, ap[t], xt, out), Ab[0] * xt + Ab[1] * out, rtol=0, atol=1e-12 * scale.max())
    assert worst <= 1e-12, worst
    with pytest.raises(ValueError, match="timesteps must lie"):
        S.analytic_moment_tables(BETAS, [0, T], kind)


# ------------------------------------------------------------------ flags and sidecar
def test_flags_and_refusals():
    import smd_amd.flags as F
    fl = F.make_flags(include_sample=True)
    assert fl.analytic_variance == "none" and fl.analytic_draws == 1 and fl.analytic_moments == ""
    fl.parse(["--ddim_steps=8", "--analytic_variance=element", "--analytic_examples=64", "--analytic_draws=2"])
    assert fl.analytic_variance == "element" and fl.analytic_examples == 64 and fl.analytic_draws == 2
    sys.path.insert(0, ROOT)
    sm = importlib.import_module("sample_ncsn")
    base = ["sample_ncsn.py", "--sampling=ddpm", "--num_sigmas=1000", "--synthetic"]
    with pytest.raises(SystemExit, match="--analytic_variance=scalar belongs to the strided sampler: give --ddim_steps"):
        sm.main(base + ["--analytic_variance=scalar"])
    with pytest.raises(SystemExit, match="--analytic_variance=element with --ddim_order=2"):
        sm.main(base + ["--ddim_steps=8", "--ddim_order=2", "--ddim_spacing=logsnr", "--analytic_variance=element"])
    with pytest.raises(SystemExit, match="--analytic_variance=scalar.*needs --sampling=ddpm"):
        sm.main(["sample_ncsn.py", "--sampling=ald", "--synthetic", "--analytic_variance=scalar"])
    with pytest.raises(SystemExit, match="--analytic_variance=element with --compute_bound"):
        sm.main(base + ["--ddim_steps=8", "--loss=ddpm", "--compute_bound", "--analytic_variance=element"])
    with pytest.raises(SystemExit, match="--analytic_draws: options of the analytic variance"):
        sm.main(base + ["--ddim_steps=8", "--analytic_draws=2"])
    with pytest.raises(SystemExit, match="--analytic_examples=0"):
        sm.main(base + ["--ddim_steps=8", "--analytic_variance=scalar", "--analytic_examples=0"])
    with pytest.raises(SystemExit, match="--analytic_moments=/nonexistent/file: no such file"):
        sm.main(base + ["--ddim_steps=8", "--analytic_variance=scalar", "--analytic_moments=/nonexistent/file"])
    flags = F.make_flags(include_sample=True)
    flags.parse(["--sampling=ddpm", "--ddim_steps=8", "--analytic_variance=scalar"])
    with pytest.raises(SystemExit, match="--analytic_variance=scalar runs in a single process.*WORLD_SIZE=2"):
        sm.check_analytic_flags(flags, world=2)
    sm.check_analytic_flags(flags, world=1)
    for eta in ("0", "0.5", "1"):                                     # any --ddim_eta, with --infill / --interpolate
        for mode in ([], ["--infill"], ["--interpolate"]):
            f2 = F.make_flags(include_sample=True)
            f2.parse(["--sampling=ddpm", "--ddim_steps=8", f"--ddim_eta={eta}", "--analytic_variance=element", *mode])
            sm.check_analytic_flags(f2)


def test_sidecar_round_trip_and_refusals(tmp_path):
    import smd_amd.analytic as AN
    FLAGS = types.SimpleNamespace(model_dir=str(tmp_path / "none"), num_sigmas=1000, sigma_begin=1e-6, sigma_end=0.01,
                                  schedule_type="linear", dtype="bf16", data_shape=[32, 42])
    engine = types.SimpleNamespace(params=__import__("torch").arange(6, dtype=__import__("torch").float32))
    meta = AN.run_metadata(FLAGS, "eps", engine)
    assert set(meta) == set(AN.META_KEYS) and meta["checkpoint"] == "" and meta["prediction"] == "eps" and len(meta["weights"]) == 64
    engine.params[3] = 7.0                                           # other weights: another digest
    assert AN.run_metadata(FLAGS, "eps", engine)["weights"] != meta["weights"]
    ts = np.array([0, 142, 285, 999])
    g = np.random.default_rng(5).uniform(0, 1, (4, 32, 42))
    path = str(tmp_path / "ncsn" / AN.MOMENTS_FILE)
    AN.save_moments(path, g, ts, 512, meta)
    g2, ts2, count, meta2 = AN.load_moments(path)
    np.testing.assert_array_equal(g2, g)
    assert g2.dtype == np.float64 and list(ts2) == list(ts) and count == 512 and meta2 == meta
    rows = AN.check_moments(path, g2, ts2, meta2, meta, [999, 285, 0], (32, 42))
    np.testing.assert_array_equal(rows, g[[3, 2, 0]])
    with pytest.raises(ValueError, match="--analytic_moments=.*do not cover the walk: \\[500\\]"):
        AN.check_moments(path, g2, ts2, meta2, meta, [999, 500, 0], (32, 42))
    for key, other in (("prediction", "v"), ("num_sigmas", "100"), ("dtype", "fp32"), ("sigma_end", "0.02"), ("checkpoint", "ckpt_3"), ("weights", "0" * 64)):
        with pytest.raises(ValueError, match=f"--analytic_moments=.*{key}="):
            AN.check_moments(path, g2, ts2, meta2, dict(meta, **{key: other}), [999, 0], (32, 42))
    with pytest.raises(ValueError, match="g of shape"):
        AN.check_moments(path, g2, ts2, meta2, meta, [999, 0], (32, 512))
    with pytest.raises(ValueError, match="does not record"):
        AN.check_moments(path, g2, ts2, {k: v for k, v in meta2.items() if k != "dtype"}, meta, [999, 0], (32, 42))


def test_header_declares_and_binding_knows_the_new_entries():
    import smd_amd.build as B
    import smd_amd.lib as L
    names = L.declared_symbols(lab=False)
    for n in ("smd_score_moments", "smd_engine_moment_step", "smd_engine_analytic_step"):
        assert n in names and n in L._SIGS
    assert "analytic.hip" in B.SOURCES and "-fno-slp-vectorize" in B.EXTRA_FLAGS["analytic.hip"]
    text = open(L.HEADER_PATH).read()
    assert f"#define SMD_MOMENT_CHUNK {L.MOMENT_CHUNK}\n" in text
    assert [f[0] for f in L.MomentIO._fields_] == ["x0", "x_t", "eps", "t_ptr", "noise_table", "moment_table", "next_t", "T", "eps_source",
                                                   "seed_lo", "seed_hi", "sample_offset", "key_ptr", "tf_keys", "tf_n_total", "partial", "sums"]
