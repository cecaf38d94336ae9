"""smd_distill_noise / smd_distill_mid / smd_distill_loss (include/smd_hip.h) element by element against
tests/_distill_ref.py, the float64 reference evaluated on the kernels' fp32 inputs and fp32 table.  Every output lies in a
guarded arena (tests/_footprint.py) whose logical elements start as a NaN canary: a no-op sample must leave its rows as they
were, and the bytes around every output must come back untouched.

Shapes (B, S, C), one per instantiation of the (VEC, RG) launch: (3, 32, 42) VEC 1 RG 4, (2, 32, 8) VEC 4 RG 4, (5, 1, 6) VEC 1
RG 1, (2, 1, 8) VEC 4 RG 1.  Walk: T = 16, N = 4 (teacher walk 15 13 11 9 6 4 2 0).  Steps cycle through 0, N - 1 (the clean
step), 1, 1, 2; a second run replaces one sample's step by N or -1.

Inputs are what a distillation step sees: x0 in [-0.8, 0.8], z_t the noised x0, teacher outputs the exact outputs for x0 plus a
0.1-sigma perturbation, x1 / z_m the float64 reference of the previous kernel rounded to fp32.

Bounds, U = 2^-24 (one fp32 rounding, relative).
  z_t      U (|sigma_t eps| + |z_t|): the product and the FMA, one rounding each.
  x1       2 U (|c0 z_t| + |c1 out1|): the FMA and the subtraction of the product's carried rounding error.
  z_m      4 * 2^-23 (|a x1| + |b z_t|) + 1e-12, the bound tests/test_gpu_strided.py applies to the same formula; with equal steps,
           bitwise what smd_engine_strided_step writes at sigma = 0 from the same table entries.
  target   x0: 4 U (|w1 x1| + |w2 x2|); eps, v: that times alpha_t / sigma_t plus 4 U (|z_t| + alpha_t |x~|) / sigma_t.
  weight   2 U |w|.   loss: rtol 1e-5 (tests/test_gpu_prediction_kernel.py).   dpred: 4 U * 2 w inv (|pred| + |target|).
Every comparison prints its worst |err| / bound before it asserts.

Measured on an MI355X, worst |err| / bound over all runs of this file: z_t 0.969, x1 0.783, z_m 0.264, target 0.273, dpred 0.247,
weight 0.404; loss 1.46e-7 relative.  A first version of the loss kernel formed the target in fp32 (x~ = fmaf(w2, x2, w1 x1),
eps: fmaf(-alpha_t, x~, z_t) / sigma_t): its target stayed inside its bound (0.48) but dpred reached 9.21 x its bound for eps
and v students at the S = 32 shapes, because the cancelling difference over sigma_t puts the target's error at the size of
z_t / sigma_t while the dpred bound is written in |pred| + |target|.  The kernel now forms the target in float64 registers and
rounds once; the bounds were not touched.
"""
import numpy as np
import pytest
import torch

import _distill_ref as R
import _footprint as F

pytestmark = pytest.mark.gpu

from _distill_cases import BETAS, KINDS, N, SHAPES, T, U, P, bits, case, ck, st, steps_for, tables  # noqa: F401


@pytest.fixture(scope="module")
def L():
    import smd_amd.lib as lib
    return lib.get_lib()


def arena(shape, dev):
    return F.guarded(shape, torch.float32, dev)


def run_noise(L, dev, c, table_d, k_d, draw=False, seed=(0, 0), step=0, eps_out=None):
    B, S, C = c["x0"].shape
    zt, hz = arena((B, S, C), dev)
    lv, hl = arena((B,), dev)
    x0 = c["x0"].to(dev)
    if draw:
        ep, he = arena((B, S, C), dev)
    else:
        ep, he = c["eps"].to(dev), None
    with F.unchanged(*([x0, table_d, k_d] + ([] if draw else [ep]))):
        ck(L.smd_distill_noise(P(x0), B, S, C, P(table_d), N, P(k_d), P(ep), int(draw), seed[0], seed[1], 0, step, None, P(zt),
                               P(lv), st()), "distill_noise")
        torch.cuda.synchronize()
    for h, name in ((hz, "z_t"), (hl, "level")) + (((he, "eps"),) if draw else ()):
        h.assert_untouched(name)
    return zt.clone(), lv.clone(), ep.clone()


def run_mid(L, dev, c, table_d, k_d):
    B, S, C = c["z_t"].shape
    x1, h1 = arena((B, S, C), dev)
    zm, h2 = arena((B, S, C), dev)
    lv, h3 = arena((B,), dev)
    ins = [c["z_t"].to(dev), c["out1"].to(dev), table_d, k_d]
    with F.unchanged(*ins):
        ck(L.smd_distill_mid(P(ins[0]), P(ins[1]), B, S, C, P(table_d), N, P(k_d), P(x1), P(zm), P(lv), st()), "distill_mid")
        torch.cuda.synchronize()
    for h, name in ((h1, "x1"), (h2, "z_m"), (h3, "level")):
        h.assert_untouched(name)
    return x1.clone(), zm.clone(), lv.clone()


def run_loss(L, dev, c, table_d, k_d, kind, iw, inv, want_target=True):
    B, S, C = c["x1"].shape
    ls, h1 = arena((B,), dev)
    w, h2 = arena((B,), dev)
    dp, h3 = arena((B, S, C), dev)
    tg, h4 = arena((B, S, C), dev) if want_target else (None, None)
    ins = [c[n].to(dev) for n in ("x1", "z_m", "out2", "z_t", "pred")] + [table_d, k_d] + ([] if iw is None else [iw])
    with F.unchanged(*ins):
        ck(L.smd_distill_loss(P(ins[0]), P(ins[1]), P(ins[2]), P(ins[3]), P(ins[4]), kind, B, S, C, P(table_d), N, P(k_d), P(iw), inv,
                              P(ls), P(w), P(dp), P(tg), st()), "distill_loss")
        torch.cuda.synchronize()
    for h, name in ((h1, "loss"), (h2, "weight"), (h3, "dpred")) + (((h4, "target"),) if want_target else ()):
        h.assert_untouched(name)
    return ls.clone(), w.clone(), dp.clone(), None if tg is None else tg.clone()


def canary_rows(t, rows):
    """True when the rows ``rows`` of t still hold the arena's NaN canary, bit for bit"""
    want = torch.tensor([F.PATTERNS[0] & 0xFF, F.PATTERNS[0] >> 8], dtype=torch.uint8).repeat(2)
    got = bits(t[rows]).reshape(-1, 4)
    return bool((got == want).all())


def ratio(got, want, bound):
    live = ~np.isnan(want)
    assert np.isfinite(got[live]).all()
    return float(np.max(np.abs(got[live] - want[live]) / bound[live]))


def f64(t):
    return t.cpu().numpy().astype(np.float64)


def bcol(table, k, name, ndim=3):
    """column ``name`` of the fp32 table for the steps k, float64, broadcastable; out-of-range steps give NaN"""
    r, live = R.rows(table, k)
    v = r[:, R.COLS[name]].copy()
    v[~live] = np.nan
    return v.reshape((-1,) + (1,) * (ndim - 1))


# ------------------------------------------------------------------ smd_distill_noise
@pytest.mark.parametrize("B,S,C", SHAPES)
def test_noise(L, dev, B, S, C):
    table, _ = tables("v", "x0")
    table_d = torch.from_numpy(table).to(dev)
    c = case(B, S, C, "v")
    for bad in (None, N, -1):
        k = steps_for(B, bad)
        k_d = torch.from_numpy(k).to(dev)
        zt, lv, _ = run_noise(L, dev, c, table_d, k_d)
        zt2, lv2, _ = run_noise(L, dev, c, table_d, k_d)
        assert torch.equal(bits(zt), bits(zt2)) and torch.equal(bits(lv), bits(lv2)), "explicit eps: two calls agree bitwise"
        want, level = R.noise(c["x0"].numpy(), c["eps"].numpy(), table, k)
        bound = U * (np.abs(bcol(table, k, "sigma_t") * f64(c["eps"])) + np.abs(want)) + 1e-300
        r = ratio(f64(zt), want, bound)
        print(f"noise {B, S, C} bad={bad}: z_t worst |err| / bound = {r:.3f}")
        assert r <= 1.0
        live = ~np.isnan(level)
        assert f64(lv)[live].tolist() == level[live].tolist()
        if bad is not None:
            dead = np.nonzero(~live)[0].tolist()
            assert dead and canary_rows(zt, dead) and canary_rows(lv, dead), "a no-op sample writes nothing"
        # Philox: reproducible, a function of (seed, sample, step), and the same z_t recipe on the drawn eps
        d1 = run_noise(L, dev, c, table_d, k_d, draw=True, seed=(7, 1), step=5)
        d2 = run_noise(L, dev, c, table_d, k_d, draw=True, seed=(7, 1), step=5)
        d3 = run_noise(L, dev, c, table_d, k_d, draw=True, seed=(7, 1), step=6)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(d1, d2)), "Philox eps: two calls agree bitwise"
        lv_rows = np.nonzero(live)[0].tolist()
        assert not torch.equal(bits(d1[2][lv_rows]), bits(d3[2][lv_rows])), "another step, another draw"
        e = f64(d1[2])[live]
        assert np.isfinite(e).all() and abs(e.mean()) < 6 / np.sqrt(e.size) and abs(e.std() - 1) < 6 / np.sqrt(e.size) + 0.05
        wantd, _ = R.noise(c["x0"].numpy()[live], d1[2].cpu().numpy()[live], table, k[live])
        boundd = U * (np.abs(bcol(table, k[live], "sigma_t") * e) + np.abs(wantd)) + 1e-300
        assert ratio(f64(d1[0])[live], wantd, boundd) <= 1.0
        if bad is not None:
            assert canary_rows(d1[2], dead) and canary_rows(d1[0], dead)


# ------------------------------------------------------------------ smd_distill_mid
@pytest.mark.parametrize("teacher", ["eps", "v"])
@pytest.mark.parametrize("B,S,C", SHAPES)
def test_mid_mixed_steps(L, dev, B, S, C, teacher):
    table, _ = tables(teacher, "x0")
    table_d = torch.from_numpy(table).to(dev)
    c = case(B, S, C, teacher)
    for bad in (None, N):
        k = steps_for(B, bad)
        k_d = torch.from_numpy(k).to(dev)
        x1, zm, lv = run_mid(L, dev, c, table_d, k_d)
        again = run_mid(L, dev, c, table_d, k_d)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip((x1, zm, lv), again))
        wx1, wzm, wlv, _ = R.mid(c["z_t"].numpy(), c["out1"].numpy(), table, k)
        zt64, o64 = f64(c["z_t"]), f64(c["out1"])
        b_x1 = 2 * U * (np.abs(bcol(table, k, "c0_t") * zt64) + np.abs(bcol(table, k, "c1_t") * o64)) * (1 + 1e-6) + 1e-30
        b_zm = 4 * 2.0 ** -23 * (np.abs(bcol(table, k, "a") * wx1) + np.abs(bcol(table, k, "b") * zt64)) + 1e-12
        r1, r2 = ratio(f64(x1), wx1, b_x1), ratio(f64(zm), wzm, b_zm)
        print(f"mid {B, S, C} teacher={teacher} bad={bad}: x1 worst |err| / bound = {r1:.3f}, z_m {r2:.3f}")
        assert r1 <= 1.0 and r2 <= 1.0
        live = ~np.isnan(wlv)
        assert f64(lv)[live].tolist() == wlv[live].tolist()
        assert float(np.nanmax(np.abs(f64(x1)[live]))) <= 1.0                      # the clamp
        if bad is not None:
            dead = np.nonzero(~live)[0].tolist()
            assert canary_rows(x1, dead) and canary_rows(zm, dead) and canary_rows(lv, dead)


@pytest.mark.parametrize("arch,C", [("dense", 42), ("dense", 512), ("transformer", 42), ("transformer", 512)])
def test_mid_equal_steps_is_the_strided_step_bitwise(L, dev, arch, C):
    """One smd_engine_strided_step at sigma = 0 on a random state; the network's own output is read back (smd_engine_pred) and
    smd_distill_mid runs on the same state and output with every sample at the step whose row carries the same table entries:
    z_m has the strided state's bits.  (No engine-free strided entry exists.)  All four (VEC, RG) forms."""
    import smd_amd.lib as lib
    import smd_amd.ncsn as Nn
    import smd_amd.schedule as Sch
    from smd_amd.engine import NetConfig
    B = 3
    cfg = (NetConfig(architecture="DenseDDPM", data_channels=C, num_layers=2, num_heads=8, num_mlp_layers=2, num_timesteps=T)
           if arch == "dense" else NetConfig(data_channels=C, num_layers=2, num_heads=8, num_mlp_layers=1, num_timesteps=T))
    model = Nn.Model(cfg, "cuda:0", seed=0)
    eng = model.engine
    shape = (B, eng.S, C) if eng.S > 1 else (B, C)
    tw, _ = Sch.distill_walk(T, N)
    table, _ = Sch.distill_tables(BETAS, tw, "v", "x0", "none")
    coef, plan = Sch.strided_coefficient_table(BETAS, tw, 0.0, 1.0, prediction="v")
    eng.set_prediction("v")
    eng.set_schedule(BETAS, with_sampler=True)
    eng.bind(B, training=False)
    eng.prepare_sampler()
    table_d = torch.from_numpy(table).to(dev)
    g = torch.Generator().manual_seed(3)
    for k in range(N):
        t = int(tw[2 * k])
        assert coef[t, :4].tolist() == table[k, :4].tolist() and coef[t, 4] == 0.0 and coef[t, 5] == table[k, 4], \
            "the strided table of the teacher walk holds the distillation row's entries"
        coef_d, plan_d = torch.from_numpy(coef).to(dev), torch.from_numpy(plan).to(dev)
        sp = lib.StridePlan()
        sp.coef, sp.plan, sp.T = coef_d.data_ptr(), plan_d.data_ptr(), T
        x = torch.randn(*shape, generator=g).to(dev)
        x_in = x.clone()
        t_ptr = torch.tensor([t], dtype=torch.int32, device=dev)
        io = lib.SampleIO()
        io.x, io.t_ptr = x.data_ptr(), t_ptr.data_ptr()
        mp = torch.zeros((T, B, 3), device=dev)
        coll = torch.zeros((41, *shape), device=dev)
        io.metrics_partial, io.collection = mp.data_ptr(), coll.data_ptr()
        eng.load_state(x)
        eng.strided_step(io, sp)
        torch.cuda.synchronize()
        out = eng.last_pred().clone().reshape(x_in.shape)
        k_d = torch.full((B,), k, dtype=torch.int32, device=dev)
        S_ = eng.S
        x1 = torch.empty_like(x_in)
        zm = torch.empty_like(x_in)
        lv = torch.empty(B, device=dev)
        ck(L.smd_distill_mid(P(x_in), P(out), B, S_, C, P(table_d), N, P(k_d), P(x1), P(zm), P(lv), st()), "distill_mid")
        torch.cuda.synchronize()
        assert torch.equal(bits(zm), bits(x)), (arch, C, k)
        assert int(t_ptr.item()) == int(plan[t, 0]) == int(tw[2 * k + 1])


# ------------------------------------------------------------------ smd_distill_loss
_LOSS_RUNS = {}


def loss_runs(L, dev, B, S, C, teacher, student):
    """worst |err| / bound of every output of smd_distill_loss over (in-range / one no-op sample) x (iw null / given), measured
    once per case; everything that is no bound -- bitwise repeatability, the footprint, the no-op rows -- is asserted here"""
    key = (B, S, C, teacher, student)
    if key in _LOSS_RUNS:
        return _LOSS_RUNS[key]
    table, _ = tables(teacher, KINDS[student])
    table_d = torch.from_numpy(table).to(dev)
    c = case(B, S, C, teacher)
    inv = float(np.float32(1.0 / (4 * B * S * C)))                     # a global batch of four shards
    iw_given = (0.25 + np.arange(B, dtype=np.float32) * 1.5).astype(np.float32)
    worst = {}
    for bad in (None, -1):
        k = steps_for(B, bad)
        k_d = torch.from_numpy(k).to(dev)
        for iw in (None, iw_given):
            iw_d = None if iw is None else torch.from_numpy(iw).to(dev)
            ls, w, dp, tg = run_loss(L, dev, c, table_d, k_d, student, iw_d, inv)
            again = run_loss(L, dev, c, table_d, k_d, student, iw_d, inv)
            assert all(torch.equal(bits(a), bits(b)) for a, b in zip((ls, w, dp, tg), again)), "two calls agree bitwise"
            nt = run_loss(L, dev, c, table_d, k_d, student, iw_d, inv, want_target=False)
            assert all(torch.equal(bits(a), bits(b)) for a, b in zip((ls, w, dp), nt[:3])), "target_out changes no other output"
            ref = R.loss(c["x1"].numpy(), c["z_m"].numpy(), c["out2"].numpy(), c["z_t"].numpy(), c["pred"].numpy(), student, table, k,
                         iw, inv)
            live = ~np.isnan(ref["loss"])
            col = lambda name: bcol(table, k, name)
            b_t = 4 * U * (np.abs(col("w1") * f64(c["x1"])) + np.abs(col("w2") * ref["x2"]))
            if student != 1:
                b_t = (b_t * col("alpha_t") * col("inv_sigma_t")
                       + 4 * U * (np.abs(f64(c["z_t"])) + col("alpha_t") * np.abs(ref["xs"])) * col("inv_sigma_t"))
            b_d = 4 * U * 2 * ref["weight"].reshape(-1, 1, 1) * float(np.float32(inv)) * (np.abs(f64(c["pred"])) + np.abs(ref["target"]))
            r_t = ratio(f64(tg), ref["target"], b_t + 1e-300)
            r_d = ratio(f64(dp), ref["dpred"], b_d + 1e-300)
            wg, lg = f64(w)[live], f64(ls)[live]
            r_w = float(np.max(np.abs(wg - ref["weight"][live]) / (2 * U * ref["weight"][live])))
            r_l = float(np.max(np.abs(lg - ref["loss"][live]) / ref["loss"][live]))
            print(f"loss {B, S, C} teacher={teacher} student={KINDS[student]} bad={bad} iw={'null' if iw is None else 'given'}: "
                  f"target worst |err| / bound = {r_t:.3f}, dpred {r_d:.3f}, weight {r_w:.3f}, loss rel err {r_l:.2e}")
            for name, v in (("target", r_t), ("dpred", r_d), ("weight", r_w), ("loss", r_l)):
                worst[name] = max(worst.get(name, 0.0), v)
            if bad is not None:
                dead = np.nonzero(~live)[0].tolist()
                assert all(canary_rows(v, dead) for v in (ls, w, dp, tg)), "a no-op sample writes nothing"
    _LOSS_RUNS[key] = worst
    return worst


@pytest.mark.parametrize("student", [0, 1, 2], ids=KINDS)
@pytest.mark.parametrize("teacher", ["eps", "v"])
@pytest.mark.parametrize("B,S,C", SHAPES)
def test_loss_target_weight_and_sum(L, dev, B, S, C, teacher, student):
    worst = loss_runs(L, dev, B, S, C, teacher, student)
    assert worst["weight"] <= 1.0 and worst["loss"] <= 1e-5, worst
    assert worst["target"] <= 1.0, worst


@pytest.mark.parametrize("student", [0, 1, 2], ids=KINDS)
@pytest.mark.parametrize("teacher", ["eps", "v"])
@pytest.mark.parametrize("B,S,C", SHAPES)
def test_loss_dpred(L, dev, B, S, C, teacher, student):
    worst = loss_runs(L, dev, B, S, C, teacher, student)
    assert worst["dpred"] <= 1.0, worst


# ------------------------------------------------------------------ refusals
def test_misaligned_vector_pointers_are_refused_unlaunched(L, dev):
    B, S, C = 2, 32, 8
    table, _ = tables("v", "x0")
    table_d = torch.from_numpy(table).to(dev)
    c = case(B, S, C, "v")
    k_d = torch.from_numpy(steps_for(B)).to(dev)
    d = {n: v.to(dev) for n, v in c.items()}
    out, h = F.guarded((B * S * C + 4,), torch.float32, dev)
    lv, hl = F.guarded((B,), torch.float32, dev)
    off = out.data_ptr() + 4                                            # 4-byte aligned only
    with pytest.raises(ValueError, match="16-byte aligned"):
        ck(L.smd_distill_noise(P(d["x0"]), B, S, C, P(table_d), N, P(k_d), P(d["eps"]), 0, 0, 0, 0, 0, None, off, P(lv), st()))
    with pytest.raises(ValueError, match="16-byte aligned"):
        ck(L.smd_distill_mid(P(d["z_t"]), P(d["out1"]), B, S, C, P(table_d), N, P(k_d), P(d["x1"]), off, P(lv), st()))
    with pytest.raises(ValueError, match="16-byte aligned"):
        ck(L.smd_distill_loss(P(d["x1"]), P(d["z_m"]), P(d["out2"]), P(d["z_t"]), P(d["pred"]), 1, B, S, C, P(table_d), N, P(k_d), None,
                              1.0, P(lv), P(lv), off, None, st()))
    with pytest.raises(ValueError, match="kind=3"):
        ck(L.smd_distill_loss(P(d["x1"]), P(d["z_m"]), P(d["out2"]), P(d["z_t"]), P(d["pred"]), 3, B, S, C, P(table_d), N, P(k_d), None,
                              1.0, P(lv), P(lv), P(d["x1"]), None, st()))
    torch.cuda.synchronize()
    h.assert_untouched("refused output")
    hl.assert_untouched("refused level")
    assert canary_rows(out, slice(None)) and canary_rows(lv, slice(None)), "refused before the launch: nothing was written"
