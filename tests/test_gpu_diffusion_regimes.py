"""The objective and sampler kernels of csrc/diffusion.hip, per element, against the float64 restatements and derived bounds of
tests/_diffusion_ref.py: reverse_step_kernel<VEC,RG>, q_sample_kernel / q_sample_quads_kernel,
mse_loss_grad_kernel<VEC>, langevin_step_kernel, the Philox normals and noise_embed_kernel.  No engine and no model: schedule tables
from smd_amd.schedule (T = 1000, linear), arrays from seeded generators, the kernels through the lab entries of
include/smd_hip_lab.h, which also report the instantiation the launcher chose.  Every output and all padding is pre-filled with NaN
or a sentinel; nothing outside the documented footprint may change.  Every test prints its worst |err| / bound."""
import ctypes

import numpy as np
import pytest
import torch

import _diffusion_ref as R
import ddpm_oracle as O

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
SENT = 0x5A5B                      # bf16 sentinel bits of untouched padding
T = R.T


@pytest.fixture(scope="module")
def L():
    import smd_amd.lib as lib
    return lib.get_lib()


@pytest.fixture(scope="module")
def tab(dev):
    betas, cf, slot, ap_ext = R.tables()
    return dict(cf=cf, slot=slot, ap=ap_ext, cfd=torch.from_numpy(cf).to(dev), slotd=torch.from_numpy(slot).to(dev),
                apd=torch.from_numpy(ap_ext).to(dev))


def P(t):
    return None if t is None else t.data_ptr()


def st():
    return torch.cuda.current_stream().cuda_stream


def ck(rc):
    import smd_amd.lib as lib
    lib.check(rc)


def dv(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ------------------------------------------------------------------------------------------------ reverse step
def launch_reverse(L, dev, tab, shape, t, x, eh, z=None, mask=None, samples=None, zi=None, key=(0, 0), key_ptr=None, offset=0,
                   tf=None, launches=1, x_off=0):
    """one (or `launches` consecutive) lab launches with every output pre-filled -> dict of what the kernel left"""
    import smd_amd.lib as lib
    B, S, C, Cp = shape
    xd = dv(x, dev)
    xb = torch.full((B * S, Cp), SENT, dtype=torch.int16, device=dev)
    coll = torch.full((41, B, S, C), float("nan"), device=dev)
    met = torch.full((T, B, 3), float("nan"), device=dev)
    tp = torch.tensor([t], dtype=torch.int32, device=dev)
    arrive = torch.zeros(1, dtype=torch.int32, device=dev)
    keep = [dv(eh, dev), dv(z, dev), dv(mask, dev), dv(samples, dev), dv(zi, dev), key_ptr]
    a = lib.ReverseStepLabArgs()
    a.x, a.eps_hat, a.B, a.S, a.C, a.Cp, a.T = xd.data_ptr() + x_off, P(keep[0]), B, S, C, Cp, T
    a.coef, a.t_ptr, a.t_advance, a.arrive, a.z_in = P(tab["cfd"]), P(tp), P(tp), P(arrive), P(keep[1])
    a.seed_lo, a.seed_hi, a.key_ptr, a.sample_offset = key[0], key[1], P(key_ptr), offset
    a.infill_masks, a.infill_samples, a.infill_z_in = P(keep[2]), P(keep[3]), P(keep[4])
    if tf is not None:
        keep.append(tf["keys"])
        a.tf_noise_keys, a.tf_n_total, a.tf_t0 = P(tf["keys"]), tf["n_total"], tf["t0"]
    a.x_bf16, a.metrics_partial, a.collection, a.slot_table = P(xb), P(met), P(coll), P(tab["slotd"])
    form = (ctypes.c_int32 * 2)(-1, -1)
    arrived = []
    for _ in range(launches):
        rc = L.smd_reverse_step_lab(ctypes.byref(a), form, st())
        if rc != 0:
            torch.cuda.synchronize()
            return dict(rc=rc, err=L.smd_last_error().decode(), x=xd.cpu().numpy(), t=int(tp.item()), arrive=int(arrive.item()),
                        form=tuple(form))
        torch.cuda.synchronize()
        arrived.append(int(arrive.item()))
    return dict(rc=0, x=xd.cpu().numpy(), xb=bits16(xb), coll=coll, met=met.cpu().numpy(), t=int(tp.item()), arrive=arrived,
                form=tuple(form))


def check_reverse(out, tab, shape, t, x, nx, e_x, met, e_met):
    """every output of one launch against the reference; -> worst |err| / bound"""
    B, S, C, Cp = shape
    q = R.worst_ratio(out["x"], nx, e_x)
    assert q < 1, ("state", shape, t, q)
    assert np.array_equal(out["xb"][:, :C], R.bf16_bits(out["x"]).reshape(B * S, C)), "bf16 copy is not the RNE of the written state"
    assert (out["xb"][:, C:] == SENT).all(), "bf16 padding touched"
    slot = int(tab["slot"][t])
    slot = slot if 0 <= slot <= 40 else -1
    others = torch.ones(41, dtype=torch.bool)
    if slot >= 0:
        assert same_bits(out["coll"][slot].cpu().numpy(), out["x"]), "collection slot differs from the state"
        others[slot] = False
    assert bool(torch.isnan(out["coll"][others.to(out["coll"].device)]).all()), "a collection slot outside the plan was written"
    rows = np.ones(T, bool)
    rows[t] = False
    assert np.isnan(out["met"][rows]).all(), "a metrics row of another timestep was written"
    qm = R.worst_ratio(out["met"][t], met, e_met)
    assert qm < 1, ("metrics", shape, t, qm, out["met"][t], met)
    assert out["t"] == t - 1 and out["arrive"] == [0], "hand-off"
    return max(q, qm)


def reverse_inputs(shape, t, regime, mask, cf):
    B, S, C, Cp = shape
    rng = R.case_rng(shape, t, regime, mask)
    x, eh = R.reverse_regime(regime, (B, S, C), cf[t], rng)
    z = rng.standard_normal((B, S, C)).astype(F32)
    m = R.make_mask(mask, (B, S, C), rng)
    s = rng.uniform(-1, 1, (B, S, C)).astype(F32) if m is not None else None
    zi = rng.standard_normal((B, S, C)).astype(F32) if m is not None else None
    return x, eh, z, m, s, zi


@pytest.mark.parametrize("form", list(R.REVERSE_SHAPES))
def test_reverse_step_every_regime_mask_and_timestep(L, dev, tab, form):
    worst, n = 0.0, 0
    for f, shape, t, regime, mask in R.reverse_cases(tab["slot"]):
        if f != form:
            continue
        x, eh, z, m, s, zi = reverse_inputs(shape, t, regime, mask, tab["cf"])
        out = launch_reverse(L, dev, tab, shape, t, x, eh, z, m, s, zi)
        assert out["rc"] == 0 and out["form"] == form, (shape, out)
        nx, e_x, sz, e_sz = R.reverse_step_ref(x, eh, z, tab["cf"][t], t, m, s, zi)
        met, e_met = R.reverse_metrics_ref(x, eh, nx, e_x, sz, e_sz, *form)
        worst = max(worst, check_reverse(out, tab, shape, t, x, nx, e_x, met, e_met))
        if t == 0 and mask == "ones":
            assert same_bits(out["x"], s)                         # the known region is the samples, bit for bit
        n += 1
    print(f"reverse_step<{form[0]},{form[1]}>: {n} cases, worst |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("t", [-1, T])
def test_reverse_step_outside_the_walk_is_a_no_op(L, dev, tab, t):
    for shape in ((3, 32, 512, 520), (5, 1, 42, 48)):
        x, eh, z, m, s, zi = reverse_inputs(shape, 5, "normal", "binary", tab["cf"])
        out = launch_reverse(L, dev, tab, shape, t, x, eh, z, m, s, zi)
        assert out["rc"] == 0 and same_bits(out["x"], x) and (out["xb"] == SENT).all()
        assert bool(torch.isnan(out["coll"]).all()) and np.isnan(out["met"]).all()
        assert out["t"] == t and out["arrive"] == [0]                    # t is not advanced, nobody arrived


def test_reverse_step_draws_in_the_kernel(L, dev, tab):
    """Philox against the host restatement (bound widened by |sigma| NORMAL_ABS), the key from device memory, a sample offset; one
    threefry case against the oracle's jax_normal"""
    worst = 0.0
    key = (0x1234567, 0x89ABCDE)
    for form, shape, off in (((4, 4), (3, 32, 512, 520), 0), ((1, 4), (3, 32, 42, 48), 5), ((4, 1), (2, 3, 64, 72), 2), ((1, 1), (5, 1, 42, 48), 1)):
        B, S, C, Cp = shape
        for t in (T - 1, 1):
            x, eh, _, m, s, _ = reverse_inputs(shape, t, "normal", "binary", tab["cf"])
            z = R.philox_normals(B, S * C, key, R.STREAM_Z, t, off).reshape(B, S, C)
            zi = R.philox_normals(B, S * C, key, R.STREAM_INFILL, t, off).reshape(B, S, C)
            out = launch_reverse(L, dev, tab, shape, t, x, eh, None, m, s, None, key=key, offset=off)
            assert out["rc"] == 0 and out["form"] == form
            nx, e_x, sz, e_sz = R.reverse_step_ref(x, eh, z, tab["cf"][t], t, m, s, zi, R.NORMAL_ABS, R.NORMAL_ABS)
            met, e_met = R.reverse_metrics_ref(x, eh, nx, e_x, sz, e_sz, *form)
            worst = max(worst, check_reverse(out, tab, shape, t, x, nx, e_x, met, e_met))
            kp = torch.tensor(list(key), dtype=torch.int64, device=dev).to(torch.int32)    # the same key read from device memory
            out2 = launch_reverse(L, dev, tab, shape, t, x, eh, None, m, s, None, key=(1, 2), key_ptr=kp, offset=off)
            assert same_bits(out2["x"], out["x"]) and same_bits(out2["met"][t], out["met"][t])
    # threefry: row (tf_t0 - t) of the key table, the window [offset S C, ...) of a global array of n_total elements
    shape, off, t0, t = (2, 6, 130, 136), 3, T - 1, T - 3
    B, S, C, Cp = shape
    n_total = (off + B + 1) * S * C
    keys = np.array([[11 + i, 1000 + 7 * i] for i in range(4)], np.uint32)
    x, eh, _, _, _, _ = reverse_inputs(shape, t, "normal", "none", tab["cf"])
    z = O.jax_normal((keys[t0 - t, 0], keys[t0 - t, 1]), n_total)[off * S * C:(off + B) * S * C].reshape(B, S, C).astype(F64)
    tf = dict(keys=torch.from_numpy(keys.view(np.int32)).to(dev), n_total=n_total, t0=t0)
    out = launch_reverse(L, dev, tab, shape, t, x, eh, None, offset=off, tf=tf)
    assert out["rc"] == 0 and out["form"] == (1, 4)
    nx, e_x, sz, e_sz = R.reverse_step_ref(x, eh, z, tab["cf"][t], t, z_abs=4e-7 * (1 + np.abs(z)))     # tests/test_gpu_jax_random.py close_normal
    met, e_met = R.reverse_metrics_ref(x, eh, nx, e_x, sz, e_sz, 1, 4)
    worst = max(worst, check_reverse(out, tab, shape, t, x, nx, e_x, met, e_met))
    print(f"reverse_step with in-kernel draws: worst |err| / bound = {worst:.3f}")


def test_reverse_step_hand_off_over_two_launches(L, dev, tab):
    shape, t = (3, 32, 42, 48), 7
    x, eh, z, _, _, _ = reverse_inputs(shape, t, "normal", "none", tab["cf"])
    out = launch_reverse(L, dev, tab, shape, t, x, eh, z, launches=2)
    assert out["rc"] == 0 and out["arrive"] == [0, 0] and out["t"] == t - 2
    assert not np.isnan(out["met"][t]).any() and not np.isnan(out["met"][t - 1]).any()
    assert np.isnan(np.delete(out["met"], [t, t - 1], axis=0)).all()


def test_vector_forms_refuse_a_pointer_four_bytes_off(L, dev, tab):
    """the refusal happens before any launch: the outputs and *t_ptr are untouched"""
    import smd_amd.lib as lib
    shape, t = (3, 32, 512, 520), 9
    B, S, C, Cp = shape
    x, eh, z, _, _, _ = reverse_inputs(shape, t, "normal", "none", tab["cf"])
    xpad = np.concatenate([x.reshape(-1), np.zeros(4, F32)])
    out = launch_reverse(L, dev, tab, (B, S, C, Cp), t, xpad, eh, z, x_off=4)
    assert out["rc"] < 0 and "16-byte aligned" in out["err"] and out["form"] == (-1, -1)
    assert same_bits(out["x"], xpad) and out["t"] == t and out["arrive"] == 0
    # q_sample (quads form and q_sample_kernel<true>) and mse_loss_grad (VEC 4)
    for qshape in ((9, 32, 512, 520), (9, 2, 42, 48)):
        Bq, Sq, Cq, Cpq = qshape
        x0 = torch.randn(Bq * Sq * Cq + 4, device=dev)
        eps = torch.randn(Bq, Sq, Cq, device=dev)
        xt = torch.full((Bq * Sq, Cpq), SENT, dtype=torch.int16, device=dev)
        eo = torch.full((Bq, Sq, Cq), float("nan"), device=dev)
        so = torch.full((Bq,), float("nan"), device=dev)
        lab = torch.full((Bq,), 5, dtype=torch.int32, device=dev)
        a = lib.QSampleLabArgs()
        a.x0, a.B, a.S, a.C, a.Cp, a.T, a.alphas_prod_ext, a.labels, a.label_min = x0.data_ptr() + 4, Bq, Sq, Cq, Cpq, T, P(tab["apd"]), P(lab), 1
        a.eps_in, a.xt_bf16, a.eps_out, a.s_out = P(eps), P(xt), P(eo), P(so)
        form = ctypes.c_int32(-1)
        rc = L.smd_q_sample_lab(ctypes.byref(a), ctypes.byref(form), st())
        torch.cuda.synchronize()
        assert rc < 0 and "16-byte aligned" in L.smd_last_error().decode() and form.value == -1
        assert bool((xt == SENT).all()) and bool(torch.isnan(eo).all()) and bool(torch.isnan(so).all())
    pred = torch.randn(5 * 32 * 512 + 4, device=dev)
    eps = torch.randn(5, 32, 512, device=dev)
    loss = torch.full((5,), float("nan"), device=dev)
    dp = torch.full((5 * 32, 520), SENT, dtype=torch.int16, device=dev)
    form = ctypes.c_int32(-1)
    rc = L.smd_loss_grad_lab(pred.data_ptr() + 4, P(eps), 5, 32, 512, 520, 0.1, P(loss), P(dp), None, ctypes.byref(form), st())
    torch.cuda.synchronize()
    assert rc < 0 and "16-byte aligned" in L.smd_last_error().decode() and form.value == -1
    assert bool((dp == SENT).all()) and bool(torch.isnan(loss).all())


# ------------------------------------------------------------------------------------------------ q_sample
def launch_q(L, dev, tab, shape, x0, eps, labels=None, alpha=None, dsm=False, key=(0, 0), offset=0):
    import smd_amd.lib as lib
    B, S, C, Cp = shape
    keep = [dv(x0, dev), dv(eps, dev), dv(None if labels is None else np.asarray(labels, np.int32), dev), dv(alpha, dev)]
    xt = torch.full((B * S, Cp), SENT, dtype=torch.int16, device=dev)
    eo = torch.full((B, S, C), float("nan"), device=dev)
    so = torch.full((B,), float("nan"), device=dev)
    a = lib.QSampleLabArgs()
    a.x0, a.B, a.S, a.C, a.Cp, a.T, a.alphas_prod_ext = P(keep[0]), B, S, C, Cp, T, P(tab["apd"])
    a.labels, a.label_min, a.alpha_in, a.dsm, a.eps_in = P(keep[2]), 1, P(keep[3]), int(dsm), P(keep[1])
    a.seed_lo, a.seed_hi, a.sample_offset, a.xt_bf16, a.eps_out, a.s_out = key[0], key[1], offset, P(xt), P(eo), P(so)
    form = ctypes.c_int32(-1)
    ck(L.smd_q_sample_lab(ctypes.byref(a), ctypes.byref(form), st()))
    torch.cuda.synchronize()
    return dict(xt=bits16(xt), eps=eo.cpu().numpy(), s=so.cpu().numpy(), form=form.value)


def q_inputs(shape, which):
    B, S, C, Cp = shape
    rng = R.case_rng(shape, which)
    pos = (np.arange(S * C, dtype=F64) % 65521) / 65521.0 + 1.0          # a distinct value per position (S C < 65521), never 0
    x0 = (pos[None, :] * (1 + np.arange(B)[:, None] / 4096.0)).astype(F32).reshape(B, S, C)
    return x0, rng.standard_normal((B, S, C)).astype(F32), rng


def check_q(out, shape, x0, eps, alpha, dsm=False):
    B, S, C, Cp = shape
    xt, e_pre, s, e_s = R.q_sample_ref(x0, eps, alpha, dsm)
    q = R.worst_ratio(R.bf16_value(out["xt"][:, :C]).reshape(B, S, C), xt, R.stored_bf16_bound(xt, e_pre))
    assert q < 1, ("xt", shape, q)
    assert (out["xt"][:, C:] == SENT).all(), "xt padding touched"
    assert same_bits(out["eps"], eps), "eps_out is not eps_in"
    qs = R.worst_ratio(out["s"], s, e_s + 1e-300)
    assert qs < 1, ("s_out", shape, qs)
    return max(q, qs)


@pytest.mark.parametrize("form", list(R.Q_SHAPES))
def test_q_sample_every_form_labels_alphas_and_dsm(L, dev, tab, form):
    worst = 0.0
    for shape in map(R.padded, R.Q_SHAPES[form]):
        B, S, C, Cp = shape
        x0, eps, rng = q_inputs(shape, "gpu")
        lab = rng.integers(1, T + 1, B)
        lab[:4] = (1, T, T + 7, 2 ** 30)[:min(4, B)]                      # alpha = 1; the last level; out of range: clamped to T
        out = launch_q(L, dev, tab, shape, x0, eps, labels=lab)
        assert out["form"] == form, (shape, R.Q_FORMS[out["form"]])
        worst = max(worst, check_q(out, shape, x0, eps, R.q_alpha_from_labels(lab, tab["ap"], T)))
        assert np.array_equal(out["xt"][:S, :C], R.bf16_bits(x0[0]).reshape(S, C))       # label 1: xt = bf16(x0) exactly
        alpha = np.resize(np.array([0.0, 1.0, 1.0 - 2.0 ** -24, 1e-30, 0.5], F32), B)
        out = launch_q(L, dev, tab, shape, x0, eps, labels=lab, alpha=alpha)
        assert out["form"] == form
        worst = max(worst, check_q(out, shape, x0, eps, alpha))
        sig = rng.uniform(0.01, 50.0, B).astype(F32)
        out = launch_q(L, dev, tab, shape, x0, eps, labels=lab, alpha=sig, dsm=True)
        assert out["form"] == form
        worst = max(worst, check_q(out, shape, x0, eps, sig, dsm=True))
    print(f"q_sample {R.Q_FORMS[form]}: worst |err| / bound = {worst:.3f}")


def test_q_sample_label_below_the_range_clamps_to_zero_and_draws_its_alpha(L, dev, tab):
    shape, key, off = (9, 32, 512, 520), (77, 99), 3
    x0, eps, _ = q_inputs(shape, "neg")
    lab = np.array([-5, 0, -2 ** 31, 3, 4, 5, 6, 7, 8])
    out = launch_q(L, dev, tab, shape, x0, eps, labels=lab, key=key, offset=off)
    alpha = tab["ap"][np.clip(lab, 1, T) - 1].copy()
    for b in range(3):                                                   # alpha is one of the two fp32 values of the documented expression
        cand = R.label_draw_alpha_candidates(tab["ap"], T, b + off, key)
        hit = [a for a in cand if F32(np.sqrt(a)) == out["s"][b]]
        assert hit, (b, cand, out["s"][b])
        alpha[b] = hit[0]
    print(f"q_sample label 0: worst |err| / bound = {check_q(out, shape, x0, eps, alpha):.3f}")


def test_q_sample_forms_agree_bitwise(L, dev, tab):
    """the promise of the explicit fma: the first 8 samples of a QPT = 4 launch are those of a QPT = 1 launch of the same 8"""
    shape = (512, 32, 132, 140)
    x0, eps, rng = q_inputs(shape, "agree")
    lab = rng.integers(1, T + 1, 512)
    big = launch_q(L, dev, tab, shape, x0, eps, labels=lab)
    small = launch_q(L, dev, tab, (8, 32, 132, 140), x0[:8], eps[:8], labels=lab[:8])
    assert (big["form"], small["form"]) == (0, 1)
    assert np.array_equal(big["xt"][:8 * 32], small["xt"]) and same_bits(big["eps"][:8], small["eps"]) and same_bits(big["s"][:8], small["s"])
    # Philox eps: the same draws in both forms, within the promise of csrc/rng.h of the float64 Box-Muller
    outs = [launch_q(L, dev, tab, s_, x0[:s_[0]], None, labels=lab[:s_[0]], key=(5, 6), offset=2) for s_ in (shape, (8, 32, 132, 140))]
    assert same_bits(outs[0]["eps"][:8], outs[1]["eps"]) and np.array_equal(outs[0]["xt"][:8 * 32], outs[1]["xt"])
    ref = R.philox_normals(8, 32 * 132, (5, 6), R.STREAM_EPS, 0, 2).reshape(8, 32, 132)
    q = R.worst_ratio(outs[1]["eps"], ref, R.NORMAL_ABS)
    print(f"q_sample Philox eps: worst |err| / 2e-6 = {q:.3f}")
    assert q < 1


# ------------------------------------------------------------------------------------------------ loss and gradient
def test_mse_loss_grad_both_forms_ddpm_and_dsm(L, dev):
    worst, reached = {}, set()
    for shape in R.LOSS_SHAPES:
        B, S, C, Cp = R.padded(shape)
        for regime in R.LOSS_REGIMES:
            for dsm in (False, True):
                rng = R.case_rng(shape, regime, dsm)
                pred, eps = R.loss_regime(regime, shape, rng)
                sigma = rng.uniform(0.01, 1.0 if regime == "huge" else 50.0, B).astype(F32) if dsm else None
                inv = F32(1.0 / (3 * B))                                 # a global batch three times this shard
                pd, ed, sd = dv(pred, dev), dv(eps, dev), dv(sigma, dev)
                loss = torch.full((B,), float("nan"), device=dev)
                dp = torch.full((B * S, Cp), SENT, dtype=torch.int16, device=dev)
                form = ctypes.c_int32(-1)
                ck(L.smd_loss_grad_lab(P(pd), P(ed), B, S, C, Cp, float(inv), P(loss), P(dp), P(sd), ctypes.byref(form), st()))
                torch.cuda.synchronize()
                vec = form.value
                assert vec == R.loss_vec(C, Cp)
                g, e_g, lref, e_l = R.loss_grad_ref(pred, eps, inv, sigma, vec)
                got = bits16(dp)
                assert (got[:, C:] == SENT).all(), "dpred padding touched"
                q = max(R.worst_ratio(R.bf16_value(got[:, :C]).reshape(B, S, C), g, R.stored_bf16_bound(g, e_g)),
                        R.worst_ratio(loss.cpu().numpy(), lref, e_l))
                assert q < 1, (shape, regime, dsm, q)
                reached.add((vec, dsm))
                worst[(vec, dsm)] = max(worst.get((vec, dsm), 0.0), q)
    assert reached == {(4, False), (4, True), (1, False), (1, True)}
    for (vec, dsm), q in sorted(worst.items()):
        print(f"mse_loss_grad<{vec}> {'dsm' if dsm else 'ddpm'}: worst |err| / bound = {q:.3f}")


# ------------------------------------------------------------------------------------------------ reach
def test_the_cases_reach_every_path(L, dev, tab):
    """what the lab entries report for the cases of this file: every reverse_step (VEC, RG), every q_sample form, both loss forms"""
    seen_r, seen_q = set(), set()
    for form, shapes in R.REVERSE_SHAPES.items():
        for shape in map(R.padded, shapes):
            x, eh, z, _, _, _ = reverse_inputs(shape, 3, "normal", "none", tab["cf"])
            out = launch_reverse(L, dev, tab, shape, 3, x, eh, z)
            assert out["form"] == form, (shape, out["form"])
            seen_r.add(out["form"])
    for form, shapes in R.Q_SHAPES.items():
        for shape in map(R.padded, shapes):
            x0, eps, _ = q_inputs(shape, "reach")
            out = launch_q(L, dev, tab, shape, x0, eps, labels=np.full(shape[0], 17))
            assert out["form"] == form, (shape, R.Q_FORMS[out["form"]])
            seen_q.add(R.Q_FORMS[out["form"]])
    assert seen_r == {(4, 4), (1, 4), (4, 1), (1, 1)} and seen_q == set(R.Q_FORMS)
    print("reverse_step forms:", sorted(seen_r), "q_sample forms:", sorted(seen_q))


# ------------------------------------------------------------------------------------------------ Langevin
def langevin_io(dev, x, g, z=None, mask=None, samples=None, zi=None, alpha=0.0, coef=0.0, isg=0.0):
    import smd_amd.lib as lib
    B = x.shape[0]
    keep = dict(x=dv(x, dev), g=dv(g, dev), z=dv(z, dev), m=dv(mask, dev), s=dv(samples, dev), zi=dv(zi, dev),
                met=torch.full((B, 3), float("nan"), device=dev), coll=torch.full(x.shape, float("nan"), device=dev))
    io = lib.LangevinIO()
    io.x, io.grad, io.alpha, io.noise_coef, io.z_in = P(keep["x"]), P(keep["g"]), float(alpha), float(coef), P(keep["z"])
    io.infill_samples, io.infill_masks, io.infill_z_in, io.infill_sigma = P(keep["s"]), P(keep["m"]), P(keep["zi"]), float(isg)
    io.metrics_partial, io.collect_out = P(keep["met"]), P(keep["coll"])
    return io, keep


def test_langevin_step_shapes_masks_and_draws(L, dev):
    worst = 0.0
    alpha, coef, isg = F32(3.1e-4), F32(np.sqrt(2 * 3.1e-4)), F32(0.37)
    for shape in R.LANGEVIN_SHAPES:
        B, S, C = shape
        for mask in R.MASKS:
            rng = R.case_rng(shape, mask, "langevin")
            x, g, z = (rng.standard_normal(shape).astype(F32) for _ in range(3))
            m = R.make_mask(mask, shape, rng)
            s = rng.uniform(-1, 1, shape).astype(F32) if m is not None else None
            zi = rng.standard_normal(shape).astype(F32) if m is not None else None
            for draws in ("explicit", "philox"):
                io, keep = langevin_io(dev, x, g, z if draws == "explicit" else None, m, s, zi if draws == "explicit" else None, alpha, coef, isg)
                zr, zir, za = z, zi, 0.0
                if draws == "philox":
                    io.seed_lo, io.seed_hi, io.step, io.sample_offset = 21, 43, 6, 2
                    zr = R.philox_normals(B, S * C, (21, 43), R.STREAM_Z, 6, 2).reshape(shape)
                    zir = R.philox_normals(B, S * C, (21, 43), R.STREAM_INFILL, 6, 2).reshape(shape) if m is not None else None
                    za = R.NORMAL_ABS
                ck(L.smd_langevin_step(ctypes.byref(io), B, S, C, st()))
                torch.cuda.synchronize()
                nx, e_x, stp, nz = R.langevin_step_ref(x, g, zr, alpha, coef, m, s, zir, isg, za, za)
                met, e_met = R.langevin_metrics_ref(g, stp, nz)
                got = keep["x"].cpu().numpy()
                q = max(R.worst_ratio(got, nx, e_x), R.worst_ratio(keep["met"].cpu().numpy(), met, e_met))
                assert q < 1, (shape, mask, draws, q)
                assert same_bits(keep["coll"].cpu().numpy(), got)
                worst = max(worst, q)
    print(f"langevin_step: worst |err| / bound = {worst:.3f}")


def test_langevin_table_mode_walks_three_rows_and_stops(L, dev):
    shape = (3, 32, 42)
    B, S, C = shape
    n = 3
    rng = R.case_rng("table")
    x = rng.standard_normal(shape).astype(F32)
    grads = [rng.standard_normal(shape).astype(F32) for _ in range(n)]
    table = np.array([[3e-4, 0.0245, 0.5, 0.9], [2e-4, 0.02, 0.4, 0.8], [1e-4, 0.0141, 0.3, 0.7]], F32)
    slots = np.array([-1, 2, 0], np.int32)
    keys = np.array([[3, 5, 7, 9], [11, 13, 17, 19], [23, 29, 31, 37]], np.uint32)
    n_total = 2 * B * S * C
    io, keep = langevin_io(dev, x, grads[0])
    keep.update(table=dv(table, dev), slots=dv(slots, dev), keys=dv(keys.view(np.int32), dev), k=torch.zeros(1, dtype=torch.int32, device=dev),
                arrive=torch.zeros(1, dtype=torch.int32, device=dev), coll=torch.full((3, B, S, C), float("nan"), device=dev),
                sig=torch.full((B,), float("nan"), device=dev), lvl=torch.full((1,), -7, dtype=torch.int32, device=dev),
                met=torch.full((n, B, 3), float("nan"), device=dev))
    io.collect_out, io.use_threefry, io.tf_n_total, io.sample_offset = None, 1, n_total, 1
    io.step_table, io.slot_table, io.key_table, io.k_ptr, io.arrive = P(keep["table"]), P(keep["slots"]), P(keep["keys"]), P(keep["k"]), P(keep["arrive"])
    io.collection, io.sigma_out, io.n_steps, io.level_out, io.steps_per_level, io.n_levels = P(keep["coll"]), P(keep["sig"]), n, P(keep["lvl"]), 2, 2
    io.metrics_partial = P(keep["met"])
    cur, worst, written = x, 0.0, set()
    for k in range(n + 1):
        keep["g"].copy_(torch.from_numpy(grads[min(k, n - 1)]))
        before = keep["x"].cpu().numpy()
        ck(L.smd_langevin_step(ctypes.byref(io), B, S, C, st()))
        torch.cuda.synchronize()
        got, met = keep["x"].cpu().numpy(), keep["met"].cpu().numpy()
        assert int(keep["arrive"].item()) == 0
        if k == n:                                                        # past the table: a no-op
            assert same_bits(got, before) and int(keep["k"].item()) == n
            break
        z = O.jax_normal((keys[k, 0], keys[k, 1]), n_total)[S * C:(1 + B) * S * C].reshape(shape).astype(F64)     # sample_offset 1
        nx, e_x, stp, nz = R.langevin_step_ref(cur, grads[k], z, table[k, 0], table[k, 1], z_abs=4e-7 * (1 + np.abs(z)))
        mref, e_met = R.langevin_metrics_ref(grads[k], stp, nz)
        q = max(R.worst_ratio(got, nx, e_x), R.worst_ratio(met[k], mref, e_met))
        assert q < 1, (k, q)
        worst = max(worst, q)
        assert np.isnan(met[k + 1:]).all() and int(keep["k"].item()) == k + 1
        assert np.array_equal(keep["sig"].cpu().numpy(), np.full(B, table[k, 3], F32)) and int(keep["lvl"].item()) == min((k + 1) // 2, 1)
        if slots[k] >= 0:
            written.add(int(slots[k]))
            assert same_bits(keep["coll"][slots[k]].cpu().numpy(), got)
        for s_ in set(range(3)) - written:
            assert bool(torch.isnan(keep["coll"][s_]).all())
        # the same update with the key of row k passed per launch: the same bits
        io2, keep2 = langevin_io(dev, cur, grads[k], alpha=table[k, 0], coef=table[k, 1], isg=table[k, 2])
        io2.use_threefry, io2.tf_n_total, io2.sample_offset = 1, n_total, 1
        io2.tf_noise_key[0], io2.tf_noise_key[1], io2.tf_infill_key[0], io2.tf_infill_key[1] = (int(v) for v in keys[k])
        ck(L.smd_langevin_step(ctypes.byref(io2), B, S, C, st()))
        torch.cuda.synchronize()
        assert same_bits(keep2["x"].cpu().numpy(), got) and same_bits(keep2["met"].cpu().numpy(), met[k])
        cur = got
    print(f"langevin_step table mode: worst |err| / bound = {worst:.3f}")


# ------------------------------------------------------------------------------------------------ normals, noise embedding
def test_philox_normals_keep_the_promise_of_rng_h(L, dev):
    """2^20 Philox blocks in both forms of fill_normal_kernel against the float64 Box-Muller of the same bits: |dz| <= 2e-6 per element"""
    key, stream, off = (0xDEADBEE, 0x1234567), R.STREAM_INIT, 3
    B, per = 4, 4 * 2 ** 18                                                # 2^20 blocks
    z = torch.full((B, per), float("nan"), device=dev)
    ck(L.smd_rng_normal(P(z), B, per, key[0], key[1], stream, off, st()))
    cut = torch.full((B, per - 2 + 8), float("nan"), device=dev)            # per_sample % 4 != 0: cut at the sample's end
    ck(L.smd_rng_normal(P(cut), B, per - 2, key[0], key[1], stream, off, st()))
    torch.cuda.synchronize()
    got, ref = z.cpu().numpy(), R.philox_normals(B, per, key, stream, 0, off)
    flat = cut.cpu().numpy().reshape(-1)
    assert same_bits(flat[:B * (per - 2)].reshape(B, per - 2), got[:, :per - 2]) and np.isnan(flat[B * (per - 2):]).all()
    q = R.worst_ratio(got, ref, R.NORMAL_ABS)
    i = np.unravel_index(np.argmax(np.abs(ref)), ref.shape)
    print(f"Philox normals, {B * per // 4} blocks: worst |dz| / 2e-6 = {q:.3f}; largest |z| = {abs(ref[i]):.4f}, there |dz| = {abs(got[i] - ref[i]):.2e}")
    assert abs(got[i] - ref[i]) <= R.NORMAL_ABS
    assert q < 1


def test_noise_embed_levels_and_an_odd_channel_count(L, dev, tab):
    cf = tab["cf"]
    levels = np.array([1.0, 0.9999995, 0.5, 0.08137959, 1e-3, cf[0, 6], cf[T // 2, 6], cf[T - 1, 6]], F32)
    worst = 0.0
    for ch, ld in ((128, 128), (43, 48)):
        out = torch.full((levels.size, ld), SENT, dtype=torch.int16, device=dev)
        sd = dv(levels, dev)
        ck(L.smd_noise_embed(P(sd), levels.size, ch, P(out), ld, st()))
        torch.cuda.synchronize()
        got = bits16(out)
        v, bound = R.noise_embed_ref(levels, ch)
        q = R.worst_ratio(R.bf16_value(got[:, :ch]), v, bound)
        assert q < 1, (ch, q)
        assert (got[:, ch:] == SENT).all()
        worst = max(worst, q)
    print(f"noise_embed: worst |err| / bound = {worst:.3f}")
