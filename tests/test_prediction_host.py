"""--prediction={eps,x0,v} on the host: the sampler tables, the min-SNR weight of each kind, the flags,
the start-up refusals and the checkpoint record.  No GPU.

The table identity.  For any x_t and eps_hat, the x0 a table recovers from the output a network of that kind would emit,
c0 x_t - c1 out, is the same for the three kinds.  It is asserted to 1e-12 relative in float64 on the float64 coefficients
(schedule.x0_coefficients) at every t of the base schedule; each table builder is then required to carry exactly those
coefficients rounded ONCE to float32 in its first two columns (x0, v: array_equal) -- the float32 columns themselves cannot
agree better than their own 2^-24 rounding, whatever the kind.  The eps columns are the reference's float32 expressions, which
every builder must return bit for bit when called without the argument; they lie within 4 float32 ulps of the float64 ones.
"""
import json
import os

import numpy as np
import pytest
import torch

import _prediction_ref as R
import _timestep_ref as TR
import smd_amd.schedule as S

BETAS = S.create_noise_schedule(1e-6, 0.01, 1000, "linear")          # the base schedule (configs/ddpm-base.cfg)
T = len(BETAS)
AP = S.alphas_cumprod(BETAS).astype(np.float64)
KINDS = ("eps", "x0", "v")


def test_prediction_kind_names():
    assert S.PREDICTIONS == KINDS
    assert [S.prediction_kind(k) for k in KINDS] == [0, 1, 2] and [S.prediction_kind(i) for i in range(3)] == [0, 1, 2]
    for bad in ("", "score", 3, -1, None, True):
        with pytest.raises(ValueError):
            S.prediction_kind(bad)


def test_recovered_x0_agrees_across_kinds_at_every_timestep():
    rng = np.random.default_rng(26)
    x_t, eps_hat = rng.standard_normal((T, 64)), rng.standard_normal((T, 64))
    ap = AP[:, None]
    x0 = {}
    for k, name in enumerate(KINDS):
        c0, c1 = S.x0_coefficients(AP, name)
        r0, r1 = R.x0_coefficients(k, AP)
        np.testing.assert_allclose(c0, r0, rtol=1e-15, atol=0)
        np.testing.assert_allclose(c1, r1, rtol=1e-13, atol=0)                  # sqrt(1/ap - 1) against sqrt(1 - ap) / sqrt(ap)
        out = R.output_of(k, x_t, eps_hat, ap)
        x0[name] = c0[:, None] * x_t - c1[:, None] * out
        np.testing.assert_allclose(R.eps_of(k, x_t, out, ap), eps_hat, rtol=0, atol=1e-9 * np.sqrt(1 / AP[-1]))
    scale = np.maximum(np.abs(x0["eps"]), np.abs(np.sqrt(1 / ap) * x_t) + np.abs(np.sqrt(1 / ap - 1) * eps_hat))
    for name in ("x0", "v"):
        assert (np.abs(x0[name] - x0["eps"]) <= 1e-12 * scale).all(), name


def _builders():
    taus = S.stride_timesteps(T, 50)
    ltaus = S.logsnr_timesteps(T, 18, BETAS)
    return {
        "reverse": (lambda **kw: S.reverse_coefficient_table(BETAS, **kw), 0, np.arange(T)),
        "strided": (lambda **kw: S.strided_coefficient_table(BETAS, taus, 0.3, **kw)[0], 0, taus),
        "inversion": (lambda **kw: S.inversion_coefficient_table(BETAS, taus, **kw)[0], 0, np.sort(taus)[:-1]),
        "multistep": (lambda **kw: S.multistep_coefficient_table(BETAS, ltaus, 2, **kw)[0], 0, ltaus),
        "bound": (lambda **kw: S.bound_tables(BETAS, np.arange(T), **kw)["table"], 2, np.arange(T)),
    }


@pytest.mark.parametrize("name", ["reverse", "strided", "inversion", "multistep", "bound"])
def test_table_builders_carry_the_coefficients(name):
    build, col, rows = _builders()[name]
    rows = np.asarray(rows)
    default = build()
    eps = build(prediction="eps")
    assert eps.dtype == np.float32 and np.array_equal(default, eps), "the default is the eps table, bit for bit"
    c0, c1 = S.x0_coefficients(AP, "eps")
    ulp = 4 * 2.0 ** -24
    assert (np.abs(eps[rows, col] - c0[rows]) <= ulp * c0[rows]).all() and (np.abs(eps[rows, col + 1] - c1[rows]) <= ulp * c1[rows]).all()
    for kind in ("x0", "v"):
        tab = build(prediction=kind)
        c0, c1 = S.x0_coefficients(AP, kind)
        assert tab.dtype == np.float32 and tab.shape == default.shape
        assert np.array_equal(tab[rows, col], c0[rows].astype(np.float32)), (name, kind)
        assert np.array_equal(tab[rows, col + 1], c1[rows].astype(np.float32)), (name, kind)
        other = np.ones(default.shape[1], bool)
        other[[col, col + 1]] = False
        assert np.array_equal(tab[:, other], default[:, other]), "nothing but the two columns changes"
        off = np.setdiff1d(np.arange(T), rows)
        assert np.array_equal(tab[off], default[off]), "rows off the walk stay as they were"
    # the plans and the other entries of the builders' results do not depend on the kind
    if name in ("strided", "inversion", "multistep"):
        taus = S.stride_timesteps(T, 50)
        f = {"strided": lambda **kw: S.strided_coefficient_table(BETAS, taus, 0.3, **kw),
             "inversion": lambda **kw: S.inversion_coefficient_table(BETAS, taus, **kw),
             "multistep": lambda **kw: S.multistep_coefficient_table(BETAS, taus, 2, **kw)}[name]
        assert np.array_equal(f()[1], f(prediction="v")[1])
    if name == "bound":
        a, b = S.bound_tables(BETAS, np.arange(T)), S.bound_tables(BETAS, np.arange(T), prediction="x0")
        assert np.array_equal(a["w"], b["w"]) and np.array_equal(a["next_t"], b["next_t"]) and a["var_0"] == b["var_0"]


TINY = 2.0 ** -40
AP_EDGE = np.array([0.0, TINY, 0.5, 1.0 - 2.0 ** -24, 1.0])


@pytest.mark.parametrize("gamma", [0.0, 5.0, float("inf")])
def test_min_snr_weight_closed_forms(gamma):
    w = {k: S.min_snr_weight(AP_EDGE, gamma, k) for k in KINDS}
    assert np.array_equal(S.min_snr_weight(AP_EDGE, gamma), w["eps"]), "the default is the eps weight"
    for k in KINDS:
        assert w[k].dtype == np.float64 and np.isfinite(w[k]).all(), (k, w[k])
    if gamma == 0.0 or np.isinf(gamma):                        # no SNR factor: all ones, for every kind
        for k in KINDS:
            assert (w[k] == 1.0).all()
        return
    snr = np.array([0.0, TINY / (1 - TINY), 1.0, (1.0 - 2.0 ** -24) / 2.0 ** -24, np.inf])
    assert w["eps"].tolist() == [1.0, 1.0, 1.0, gamma / snr[3], 0.0]
    np.testing.assert_allclose(w["x0"], [0.0, snr[1], 1.0, gamma, gamma], rtol=1e-15)
    np.testing.assert_allclose(w["v"], [0.0, snr[1] * (1 - TINY), 0.5, gamma * 2.0 ** -24, 0.0], rtol=1e-15)
    assert w["x0"][-1] == gamma and w["v"][-1] == 0.0 and w["x0"][0] == 0.0 and w["v"][0] == 0.0
    fin = np.isfinite(snr) & (snr > 0)                          # the identity w_v (SNR + 1) = w_x0 = w_eps SNR, where finite
    np.testing.assert_allclose(w["v"][fin] * (snr[fin] + 1), w["x0"][fin], rtol=1e-14)
    np.testing.assert_allclose(w["eps"][fin] * snr[fin], w["x0"][fin], rtol=1e-14)
    # the reference the GPU tests use evaluates the same forms from the stored noise level
    s = np.sqrt(AP_EDGE).astype(np.float32)
    for k, name in enumerate(KINDS):
        ap32 = s.astype(np.float64) ** 2
        got = R.weight(k, s, None, gamma)
        want = S.min_snr_weight(ap32, gamma, name)
        exact = (s == 1.0) | (s == 0.0)
        assert np.array_equal(got[exact], want[exact])
        np.testing.assert_allclose(got[~exact], want[~exact], rtol=1e-9)        # (1 - s)(1 + s) against 1 - s^2 at 1 - 2^-25


def test_reference_agrees_with_the_weighted_reference_at_kind_0():
    rng = np.random.default_rng(7)
    pred, eps, x0 = (rng.standard_normal((4, 3, 10)).astype(np.float32) for _ in range(3))
    s = np.array([1.0, 0.08, 0.7, 0.9999], np.float32)
    iw = np.array([0.5, 2.0, 1.0, 3.0], np.float32)
    inv = np.float32(1.0 / 120)
    for w_in in (None, iw):
        for gamma in (0.0, 5.0, float("inf")):
            a = R.param_grad(0, pred, eps, x0, s, w_in, gamma, inv)
            b = TR.weighted_grad(pred, eps, s, w_in, gamma, inv)
            for x, y in zip(a, b):
                np.testing.assert_allclose(x, y, rtol=1e-9, atol=0)     # (1 - s)(1 + s) here, 1 - s^2 there
    # and the targets: x0 is x0, v is s eps - sb x0, on which out = target gives zero loss and gradient
    for kind in (1, 2):
        t = R.target(kind, eps, x0, s)
        g, loss, w = R.param_grad(kind, t.astype(np.float32), eps, x0, s, None, 5.0, inv)
        assert np.abs(g).max() < 1e-6 and loss.max() < 1e-12
    np.testing.assert_allclose(R.target(2, eps, x0, s)[2], 0.7 * eps[2].astype(np.float64)
                               - np.sqrt(1 - np.float64(np.float32(0.7)) ** 2) * x0[2], rtol=1e-6, atol=1e-7)   # f32(0.7) for s
    assert np.array_equal(R.target(2, eps, x0, s)[0], eps[0].astype(np.float64))       # s = 1: v = eps


def test_loss_in_eps_units():
    from smd_amd.trainer import loss_in_eps_units
    loss = torch.tensor([0.5, 2.0, 1.0, 4.0])
    s = torch.tensor([1.0, 0.08, 0.7, 0.9])
    for k, name in enumerate(KINDS):
        got = float(loss_in_eps_units(loss, s, name))
        assert got == pytest.approx(R.loss_in_eps_units(k, loss.numpy(), s.numpy()), rel=1e-6), name
    assert float(loss_in_eps_units(loss, s, "eps")) == pytest.approx(1.875)
    # ap = 1 is left out of the x0 mean (three samples remain); a batch of nothing but ap = 1 gives 0, not a NaN
    ap = s.double().numpy()[1:] ** 2
    assert float(loss_in_eps_units(loss, s, "x0")) == pytest.approx(float((ap / (1 - ap) * loss.numpy()[1:]).mean()), rel=1e-6)
    assert float(loss_in_eps_units(loss[:1], s[:1], "x0")) == 0.0
    with pytest.raises(ValueError):
        loss_in_eps_units(loss, s, "score")


# ---------------------------------------------------------------------------------------------------- flags and refusals
def test_flag_defaults_and_choices():
    from smd_amd import flags as F
    tr, sa = F.make_flags(include_sample=False), F.make_flags(include_sample=True)
    assert tr.prediction == "eps" and sa.prediction == ""
    for k in KINDS:
        tr.parse([f"--prediction={k}"])
        sa.parse([f"--prediction={k}"])
        assert tr.prediction == k and sa.prediction == k and tr.is_present("prediction")
    with pytest.raises(F.FlagError):
        tr.parse(["--prediction=score"])
    with pytest.raises(F.FlagError):
        tr.parse(["--prediction="])                              # training always names its kind
    sa.parse(["--prediction="])                                  # sampling: empty = what the checkpoint says
    assert sa.prediction == ""
    assert "flax" in F.prediction_flag(True).help and "REQUIRED" in F.prediction_flag(True).help


def test_validate_training_options_refusals():
    from smd_amd.trainer import validate_training_options as V
    for k in KINDS:
        V("ddpm", "none", "uniform", 1, prediction=k, sampling="ddpm")
        V("ddpm", "min_snr", "loss_second_moment", 1, prediction=k)
    V("dsm", prediction="eps", sampling="ald")                   # what worked before still does
    V("ddpm", "min_snr", "uniform", 8)
    for k in ("x0", "v"):
        for loss in ("dsm", "ssm"):
            with pytest.raises(ValueError, match=r"--prediction.*--loss"):
                V(loss, prediction=k)
        for sampling in ("ald", "cas"):
            with pytest.raises(ValueError, match=r"--prediction.*--sampling"):
                V("ddpm", prediction=k, sampling=sampling)
    with pytest.raises(ValueError, match="--prediction must be one of"):
        V("ddpm", prediction="score")


def test_train_step_refuses_before_touching_the_engine():
    from smd_amd import ncsn
    from smd_amd.trainer import train_step
    with pytest.raises(ValueError, match="prediction must be one of"):
        train_step(ncsn.diffusion_loss, None, None, None, None, 1e-3, prediction="score")
    with pytest.raises(ValueError, match="diffusion_loss"):
        train_step(ncsn.denoising_score_matching_loss, None, None, None, None, 1e-3, prediction="v")
    with pytest.raises(ValueError, match="diffusion_loss"):
        train_step(lambda *a: None, None, None, None, None, 1e-3, prediction="x0")


# ---------------------------------------------------------------------------------------------------- checkpoint record
def _write(path, meta):
    from safetensors.torch import save_file
    save_file({"state/step": torch.zeros(1, dtype=torch.int32)}, path, metadata=meta)


def test_checkpoint_metadata_round_trip_and_refusals(tmp_path):
    from smd_amd import checkpoint as CK
    d = str(tmp_path)
    assert CK.checkpoint_prediction(d) is None and CK.checkpoint_train_options(d) == {}
    CK.check_resume_prediction(d, "v")                           # no checkpoint: nothing to contradict
    _write(os.path.join(d, "checkpoint_0"), {"format": "smd_amd-1"})          # written before the field existed: an eps model
    assert CK.checkpoint_prediction(d) is None
    CK.check_resume_prediction(d, "eps")
    with pytest.raises(ValueError, match=r"--resume.*--prediction=eps.*--prediction=v"):
        CK.check_resume_prediction(d, "v")
    # what save_checkpoint does with train_options: every value becomes a string of the metadata
    opts = {"loss_weighting": "min_snr", "min_snr_gamma": 5.0, "timestep_sampler": "uniform", "prediction": "v"}
    _write(os.path.join(d, "checkpoint_1"), {str(k): str(v) for k, v in opts.items()})
    assert CK.checkpoint_prediction(d) == "v" and CK.checkpoint_prediction(os.path.join(d, "checkpoint_1")) == "v"
    assert CK.checkpoint_train_options(d)["min_snr_gamma"] == "5.0"
    CK.check_resume_prediction(d, "v")
    for other in ("eps", "x0"):
        with pytest.raises(ValueError, match=r"--resume.*--prediction=v"):
            CK.check_resume_prediction(d, other)
    # sampling: empty flag = the record; a contradiction is refused; no record = eps unless the flag says otherwise
    assert CK.resolve_prediction("", "v") == "v" and CK.resolve_prediction("v", "v") == "v"
    assert CK.resolve_prediction("", None) == "eps" and CK.resolve_prediction("x0", None) == "x0"
    with pytest.raises(ValueError, match=r"--prediction=eps contradicts .* --prediction=v"):
        CK.resolve_prediction("eps", "v")
    with pytest.raises(ValueError):
        CK.resolve_prediction("", "score")


class _StubEngine:
    """what checkpoint.save_checkpoint reads of an engine: flat fp32 buffers with named views, the step counter, the dtype"""

    class cfg:
        dtype = "bf16"

    def __init__(self):
        self.params, self.m, self.v = torch.arange(6.0), torch.zeros(6), torch.ones(6)
        self.step_counter = torch.tensor([3], dtype=torch.int32)

    def named_views(self, flat):
        return {"Dense_0/kernel": flat[:4].view(2, 2), "Dense_0/bias": flat[4:]}


def test_save_checkpoint_records_the_kind_and_resume_reads_it(tmp_path):
    """through checkpoint.save_checkpoint itself, on the CPU: train_options reach the safetensors metadata, the reader functions
    find the kind there, and the tensors are untouched by it"""
    from types import SimpleNamespace
    from safetensors.torch import load_file
    from smd_amd import checkpoint as CK
    from smd_amd.train_utils import EarlyStopping
    d = str(tmp_path)
    eng = _StubEngine()
    target = (SimpleNamespace(engine=eng), SimpleNamespace(params=eng.params.clone(), mu=0.999), EarlyStopping(patience=1))
    for step, kind in ((0, "v"), (1, "x0")):
        opts = {"loss_weighting": "min_snr", "min_snr_gamma": 5.0, "timestep_sampler": "uniform", "prediction": kind}
        path = CK.save_checkpoint(d, target, step, train_options=opts)
        assert CK.checkpoint_prediction(path) == kind and CK.checkpoint_prediction(d) == kind          # the newest file
        assert CK.checkpoint_train_options(path)["loss_weighting"] == "min_snr"
        CK.check_resume_prediction(d, kind)
        with pytest.raises(ValueError, match=f"--prediction={kind}"):
            CK.check_resume_prediction(d, "eps")
        assert CK.resolve_prediction("", CK.checkpoint_prediction(d)) == kind
        assert torch.equal(load_file(path)["target/params/Dense_0/kernel"], eng.params[:4].view(2, 2))
    path = CK.save_checkpoint(d, target, 2)                       # a caller that passes no options: an eps model, as before
    assert CK.checkpoint_prediction(path) is None
    CK.check_resume_prediction(d, "eps")


def test_sample_cli_resolves_against_the_checkpoint(tmp_path):
    import sample_ncsn
    from smd_amd import flags as F
    d = str(tmp_path)
    _write(os.path.join(d, "checkpoint_3"), {"prediction": "x0"})
    FL = F.make_flags(include_sample=True)
    FL.parse([f"--model_dir={d}", "--sampling=ddpm"])
    assert sample_ncsn.resolve_prediction_flag(FL) == "x0"
    FL.parse(["--prediction=x0"])
    assert sample_ncsn.resolve_prediction_flag(FL) == "x0"
    FL.parse(["--prediction=eps"])
    with pytest.raises(ValueError, match="contradicts"):
        sample_ncsn.resolve_prediction_flag(FL)
    FL.parse(["--prediction=", "--sampling=ald"])
    with pytest.raises(ValueError, match=r"--sampling=ddpm"):
        sample_ncsn.resolve_prediction_flag(FL)
    FL.parse([f"--model_dir={os.path.join(d, 'nothing_here')}", "--sampling=ddpm"])
    assert sample_ncsn.resolve_prediction_flag(FL) == "eps"
    json.dumps(dict(prediction="v", eps_mse=None))             # what bound.json holds for a v model: plain JSON
