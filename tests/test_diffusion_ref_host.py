"""Host check of tests/_diffusion_ref.py: the fp32 emulation of every kernel of csrc/diffusion.hip stays inside its derived bound on
every regime and shape the GPU test uses (the bound is attainable), and each planted fault leaves it at one element at least by a
factor >= 2 (the bound is sharp enough to see a subtly wrong kernel).  For each fault the old whole-array criterion (rel-L2 of the
output the old tests looked at: 1e-5 state, 3e-3 xt / gradient, 1e-2 walks) is evaluated at the same shape.  CPU only."""
import numpy as np
import pytest

import _diffusion_ref as R

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def tab():
    return R.tables()


def _reverse_inputs(shape, t, regime, mask, cf):
    B, S, C, Cp = shape
    rng = R.case_rng(shape, t, regime, mask)
    x, eh = R.reverse_regime(regime, (B, S, C), cf[t], rng)
    z = rng.standard_normal((B, S, C)).astype(F32)
    m = R.make_mask(mask, (B, S, C), rng)
    s = rng.uniform(-1, 1, (B, S, C)).astype(F32) if m is not None else None
    zi = rng.standard_normal((B, S, C)).astype(F32) if m is not None else None
    return x, eh, z, m, s, zi


def test_reverse_step_emulation_stays_inside_the_bound(tab):
    _, cf, slot, _ = tab
    worst = {}
    for form, shape, t, regime, mask in R.reverse_cases(slot):
        vec, rg = R.step_form(shape[1], shape[2], shape[3], True)
        assert (vec, rg) == form, (shape, form)
        x, eh, z, m, s, zi = _reverse_inputs(shape, t, regime, mask, cf)
        nx, e_x, sz, e_sz = R.reverse_step_ref(x, eh, z, cf[t], t, m, s, zi)
        met, e_met = R.reverse_metrics_ref(x, eh, nx, e_x, sz, e_sz, vec, rg)
        for fma in (False, True):
            got, gmet = R.reverse_step_emu(x, eh, z, cf[t], t, vec, rg, m, s, zi, fma=fma)
            q = max(R.worst_ratio(got, nx, e_x), R.worst_ratio(gmet, met, e_met))
            assert q < 1, (shape, t, regime, mask, fma, q)
            worst[form] = max(worst.get(form, 0.0), q)
        if t == 0 and mask == "ones":
            assert np.array_equal(got, s)                          # the known region is the samples, bit for bit
    for form, q in sorted(worst.items()):
        print(f"reverse_step<{form[0]},{form[1]}> emulation: worst |err| / bound = {q:.3f}")


def _q_inputs(shape, ap_ext, which):
    B, S, C, Cp = shape
    rng = R.case_rng(shape, which)
    pos = (np.arange(S * C, dtype=F64) % 65521) / 65521.0 + 1.0          # distinct per position where S C < 65521, never 0
    x0 = (pos[None, :] * (1 + np.arange(B)[:, None] / 4096.0)).astype(F32).reshape(B, S, C)
    eps = rng.standard_normal((B, S, C)).astype(F32)
    if which == "labels":
        lab = rng.integers(1, R.T + 1, B)
        lab[:3] = (1, R.T, R.T + 7)[:min(3, B)]
        alpha = R.q_alpha_from_labels(lab, ap_ext, R.T)
    elif which == "alphas":
        alpha = np.resize(np.array([0.0, 1.0, 1.0 - 2.0 ** -24, 1e-30, 0.5], F32), B)
    else:
        alpha = rng.uniform(0.01, 50.0, B).astype(F32)                    # dsm: sigmas
    return x0, eps, alpha


def test_q_sample_emulation_stays_inside_the_bound(tab):
    _, _, _, ap_ext = tab
    worst = {}
    for form, shapes in R.Q_SHAPES.items():
        for shape in map(R.padded, shapes):
            assert R.q_form(*shape) == form, (shape, form)
            for which in ("labels", "alphas", "dsm"):
                x0, eps, alpha = _q_inputs(shape, ap_ext, which)
                xt, e_pre, s, e_s = R.q_sample_ref(x0, eps, alpha, which == "dsm")
                for fma in (True, False) if form >= 2 else (True,):
                    got, gs = R.q_sample_emu(x0, eps, alpha, which == "dsm", fma)
                    q = max(R.worst_ratio(R.bf16_value(R.bf16_bits(got)), xt, R.stored_bf16_bound(xt, e_pre)),
                            R.worst_ratio(gs, s, e_s + 1e-300))
                    assert q < 1, (shape, which, fma, q)
                    worst[form] = max(worst.get(form, 0.0), q)
                if which == "labels":                                   # label 1: alpha = 1, xt = bf16(x0) exactly
                    assert np.array_equal(R.bf16_bits(got[0]), R.bf16_bits(x0[0]))
    for form, q in sorted(worst.items()):
        print(f"q_sample {R.Q_FORMS[form]} emulation: worst |err| / bound = {q:.3f}")


def _loss_inputs(shape, regime, dsm):
    rng = R.case_rng(shape, regime, dsm)
    pred, eps = R.loss_regime(regime, shape, rng)
    sigma = rng.uniform(0.01, 1.0 if regime == "huge" else 50.0, shape[0]).astype(F32) if dsm else None
    return pred, eps, F32(1.0 / (3 * shape[0])), sigma                   # a global batch three times this shard


def test_loss_grad_emulation_stays_inside_the_bound():
    worst = {}
    for shape in R.LOSS_SHAPES:
        vec = R.loss_vec(shape[2], R.padded(shape)[3])
        for regime in R.LOSS_REGIMES:
            for dsm in (False, True):
                pred, eps, inv, sigma = _loss_inputs(shape, regime, dsm)
                g, e_g, loss, e_loss = R.loss_grad_ref(pred, eps, inv, sigma, vec)
                gg, gl = R.loss_grad_emu(pred, eps, inv, sigma, vec)
                q = max(R.worst_ratio(R.bf16_value(R.bf16_bits(gg)), g, R.stored_bf16_bound(g, e_g)), R.worst_ratio(gl, loss, e_loss))
                assert q < 1, (shape, regime, dsm, q)
                worst[(vec, dsm)] = max(worst.get((vec, dsm), 0.0), q)
    assert set(worst) == {(4, False), (4, True), (1, False), (1, True)}
    for (vec, dsm), q in sorted(worst.items()):
        print(f"mse_loss_grad<{vec}> {'dsm' if dsm else 'ddpm'} emulation: worst |err| / bound = {q:.3f}")


def _langevin_inputs(shape, mask):
    rng = R.case_rng(shape, mask, "langevin")
    x, g, z = (rng.standard_normal(shape).astype(F32) for _ in range(3))
    m = R.make_mask(mask, shape, rng)
    s = rng.uniform(-1, 1, shape).astype(F32) if m is not None else None
    zi = rng.standard_normal(shape).astype(F32) if m is not None else None
    return x, g, z, m, s, zi


def test_langevin_emulation_stays_inside_the_bound():
    worst = 0.0
    for shape in R.LANGEVIN_SHAPES:
        for mask in R.MASKS:
            x, g, z, m, s, zi = _langevin_inputs(shape, mask)
            alpha, coef, isg = F32(3.1e-4), F32(np.sqrt(2 * 3.1e-4)), F32(0.37)
            nx, e_x, stp, nz = R.langevin_step_ref(x, g, z, alpha, coef, m, s, zi, isg)
            met, e_met = R.langevin_metrics_ref(g, stp, nz)
            got, gmet = R.langevin_step_emu(x, g, z, alpha, coef, m, s, zi, isg)
            q = max(R.worst_ratio(got, nx, e_x), R.worst_ratio(gmet, met, e_met))
            assert q < 1, (shape, mask, q)
            worst = max(worst, q)
    print(f"langevin_step emulation: worst |err| / bound = {worst:.3f}")


def test_noise_embed_emulation_stays_inside_the_bound(tab):
    _, cf, _, _ = tab
    levels = np.array([0.0, 1e-4, 0.01, 0.3, 0.999, 1.0, cf[0, 6], cf[R.T // 2, 6], cf[R.T - 1, 6]], F32)
    worst = 0.0
    for ch in (128, 43):
        v, bound = R.noise_embed_ref(levels, ch)
        q = R.worst_ratio(R.noise_embed_emu(levels, ch), v, bound)
        assert q < 1, (ch, q)
        worst = max(worst, q)
    print(f"noise_embed emulation: worst |err| / bound = {worst:.3f}")


def test_float64_box_muller_is_the_oracle_of_the_philox_bits():
    """the reference of the normals test: shapes, the prefix property and the sample offset of philox_normals"""
    a = R.philox_normals(2, 44, (7, 9), R.STREAM_INIT)
    b = R.philox_normals(2, 42, (7, 9), R.STREAM_INIT)
    c = R.philox_normals(1, 44, (7, 9), R.STREAM_INIT, sample_offset=1)
    assert np.array_equal(a[:, :42], b) and np.array_equal(a[1:], c)
    assert abs(a.mean()) < 0.5 and 0.5 < a.std() < 1.5


# ------------------------------------------------------------------------------------------------ planted faults
def _factor(got, ref, bound):
    return R.worst_ratio(got, ref, bound)


def _reverse_fault(tab, fault, shape, t, mask="none", regime="normal", metric=False):
    """-> (factor by which the fault leaves the bound, rel-L2 of what the old test compared)"""
    _, cf, _, _ = tab
    shape = R.padded(shape)
    vec, rg = R.step_form(shape[1], shape[2], shape[3], True)
    x, eh, z, m, s, zi = _reverse_inputs(shape, t, regime, mask, cf)
    nx, e_x, sz, e_sz = R.reverse_step_ref(x, eh, z, cf[t], t, m, s, zi)
    met, e_met = R.reverse_metrics_ref(x, eh, nx, e_x, sz, e_sz, vec, rg)
    got, gmet = R.reverse_step_emu(x, eh, z, cf[t], t, vec, rg, m, s, zi, fault=fault, cf_row=cf[max(t - 1, 0)])
    if metric:
        return _factor(gmet, met, e_met), R.rel_l2(gmet.astype(F64).sum(0), met.sum(0))
    return _factor(got, nx, e_x), R.rel_l2(got, nx)


def _q_fault(tab, fault):
    _, _, _, ap_ext = tab
    shape = R.padded((9, 32, 512))
    x0, eps, alpha = _q_inputs(shape, ap_ext, "labels")
    xt, e_pre, _, _ = R.q_sample_ref(x0, eps, alpha)
    ref_img = np.zeros((shape[0] * shape[1], shape[3]), F64)
    ref_img[:, :shape[2]] = xt.reshape(-1, shape[2])
    bound = np.full(ref_img.shape, 0.0)
    bound[:, :shape[2]] = R.stored_bf16_bound(xt, e_pre).reshape(-1, shape[2])
    if fault == "label_not_clamped":                                    # label T + 7 reads past the table: modelled as the product going on
        alpha = alpha.copy()
        alpha[2] = F32(ap_ext[R.T] * (1 - 0.01) ** 7)
    got, _ = R.q_sample_emu(x0, eps, alpha, fault=fault)
    img = R.bf16_value(R.q_layout(got, shape[3], 0, fault="row_index" if fault == "row_index" else None))
    bound = np.where(bound == 0, 1e-300, bound)                         # padding: untouched means equal to the fill
    return _factor(img, ref_img, bound), R.rel_l2(img[:, :shape[2]], xt.reshape(-1, shape[2]))


def _loss_fault(fault):
    shape, vec = ((5, 3, 42), 1) if fault == "grad_factor_2" else ((5, 32, 512), 4)       # a shape at which the last wave has terms
    pred, eps, inv, _ = _loss_inputs(shape, "normal", False)
    g, e_g, loss, e_loss = R.loss_grad_ref(pred, eps, inv, None, vec)
    gg, gl = R.loss_grad_emu(pred, eps, inv, None, vec, fault=fault)
    if fault == "grad_factor_2":
        return _factor(R.bf16_value(R.bf16_bits(gg)), g, R.stored_bf16_bound(g, e_g)), R.rel_l2(gg, g)
    return _factor(gl, loss, e_loss), R.rel_l2(gl, loss)


def _bits_fault(which):
    """criteria that are bit equality: any difference is a failure (factor inf)"""
    rng = R.case_rng(which)
    x = rng.standard_normal((3, 32, 42)).astype(F32)
    if which == "bf16_truncated":
        a, b = R.bf16_bits(x, truncate=True), R.bf16_bits(x)
        return (np.inf if (a != b).any() else 0.0), R.rel_l2(R.bf16_value(a), R.bf16_value(b))
    coll = np.zeros((41,) + x.shape, F32)                               # snapshot_slot_plus_1
    want = coll.copy()
    want[7], coll[8] = x, x
    return (np.inf if not np.array_equal(coll, want) else 0.0), R.rel_l2(coll[7], want[7])


FAULTS = {
    # name: (how to run it, the old criterion that watched this output)
    "clamp applied after the mu1 product": (lambda tab: _reverse_fault(tab, "clamp_after_mu1", (3, 32, 42), 999, regime="clamped"), R.OLD_STATE_REL),
    "clamp missing on the negative side": (lambda tab: _reverse_fault(tab, "no_negative_clamp", (3, 32, 42), 1, regime="edge"), R.OLD_STATE_REL),
    "z not scaled by sigma": (lambda tab: _reverse_fault(tab, "z_unscaled", (3, 32, 42), 1), R.OLD_STATE_REL),
    "z added at t = 0": (lambda tab: _reverse_fault(tab, "z_at_t0", (3, 32, 42), 0, regime="tiny"), R.OLD_STATE_REL),
    "infill coefficients swapped": (lambda tab: _reverse_fault(tab, "infill_coef_swapped", (3, 32, 42), 500, "binary"), R.OLD_WALK_REL),
    "mask inverted": (lambda tab: _reverse_fault(tab, "mask_inverted", (3, 32, 42), 500, "quarter"), R.OLD_WALK_REL),
    "blend at another row's level": (lambda tab: _reverse_fault(tab, "blend_at_level_t", (3, 32, 42), 999, "ones"), R.OLD_WALK_REL),
    "one row group dropped at a ragged S": (lambda tab: _reverse_fault(tab, "drops_a_row_group", (2, 5, 516), 999, metric=True), R.OLD_STATE_REL),
    "sqrt per column at S = 1": (lambda tab: _reverse_fault(tab, "sqrt_per_column", (5, 1, 42), 999, metric=True), R.OLD_WALK_REL),
    "last column of C = 42 stale": (lambda tab: _reverse_fault(tab, "stale_last_column", (3, 32, 42), 1, regime="cancel"), R.OLD_STATE_REL),
    "snapshot written to slot + 1": (lambda tab: _bits_fault("snapshot_slot_plus_1"), R.OLD_STATE_REL),
    "q_sample row index off by one at a row boundary": (lambda tab: _q_fault(tab, "row_index"), R.OLD_XT_REL),
    "sb = 1 - alpha": (lambda tab: _q_fault(tab, "sb_is_one_minus_alpha"), R.OLD_XT_REL),
    "label not clamped": (lambda tab: _q_fault(tab, "label_not_clamped"), R.OLD_XT_REL),
    "gradient missing its factor 2": (lambda tab: _loss_fault("grad_factor_2"), R.OLD_XT_REL),
    "loss missing one wave's partial": (lambda tab: _loss_fault("loss_drops_a_wave"), 1e-5),
    "bf16 truncated instead of rounded": (lambda tab: _bits_fault("bf16_truncated"), R.OLD_XT_REL),
    "Langevin noise_coef applied to the gradient": (None, R.OLD_WALK_REL),
}


def _langevin_fault():
    shape = (3, 32, 42)
    x, g, z, m, s, zi = _langevin_inputs(shape, "none")
    alpha, coef = F32(3.1e-4), F32(np.sqrt(2 * 3.1e-4))
    nx, e_x, _, _ = R.langevin_step_ref(x, g, z, alpha, coef)
    got, _ = R.langevin_step_emu(x, g, z, alpha, coef, fault="noise_coef_on_gradient")
    return _factor(got, nx, e_x), R.rel_l2(got, nx)


@pytest.mark.parametrize("name", list(FAULTS))
def test_planted_fault_leaves_the_bound(tab, name):
    run, old = FAULTS[name]
    factor, rel = run(tab) if run else _langevin_fault()
    seen = "seen" if rel >= old else "NOT seen"
    print(f"fault '{name}': leaves the bound by {factor:.3g}x; whole-array rel-L2 {rel:.2e} against the old {old:g}: {seen}")
    assert factor >= 2, (name, factor)
