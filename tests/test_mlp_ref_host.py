"""The element-wise criterion of the encoder MLP kernels (tests/_mlp_ref.py) is right, has room and is sharp: CPU only.

  * the closed forms of gelu and gelu' equal the oracle's gelu and its float64 autograd derivative; max |gelu''| is below the G2
    the bound uses; the largest value of the |xd| |1 - 2 s| ds term and the z at which it falls are printed;
  * the selector weights select, the regimes put z where they say, exactly (z is representable in fp32);
  * an fp32 emulation of the kernels' arithmetic (bf16 exactly at their rounding points, every fp32 sum in ascending and in
    descending order, exp2 and the reciprocal evaluated in fp32) stays inside the bound at every element of every regime, with
    selector W2 (every phase) and with dense W2; the saturated regimes give exactly -0 / 0 and bf16(z) / 1;
  * every planted fault leaves the bound where CAUGHT says (observable, regime, dense or selector W2);
  * the example the whole-matrix thresholds miss: b1 of ONE hidden unit off by 0.1 at M = 2048 (dense N(0, 1) inputs as in
    tests/test_gpu_kernels.py).  It moves one column of z by 0.1, i.e. z by 0.1 / (sqrt(2048) sigma_z) ~ 2.2e-3 in norm: the old
    criterion (3e-3 on h_out - h, 4e-3 on u, 6e-3 on dz) passes, the element-wise one fails on u and on dz.
"""
import pytest
import torch

import _mlp_ref as R
import ddpm_oracle as O

ROWS, M = 128, 1536          # one group of four samples; three phases, an odd number of chunks per quarter


def test_gelu_closed_forms_agree_with_the_oracle_and_its_autograd():
    z = torch.cat([torch.linspace(-12, 12, 48001, dtype=R.F64), torch.tensor([-200.0, -30.0, 30.0, 200.0], dtype=R.F64)]).requires_grad_(True)
    want = O.gelu(z)
    (g1,) = torch.autograd.grad(want.sum(), z, create_graph=True)
    (g2,) = torch.autograd.grad(g1.sum(), z)
    zd = z.detach()
    assert float((R.gelu(zd) - want.detach()).abs().max()) <= 1e-14 * 200
    assert float((R.gelu_grad(zd) - g1.detach()).abs().max()) <= 1e-13
    print(f"max |gelu''| = {float(g2.abs().max()):.4f} at z = {float(zd[g2.abs().argmax()]):.3f} (G2 = {R.G2})")
    assert float(g2.abs().max()) < R.G2
    near = zd[(zd > -2) & (zd < 0)]
    zc = near[R.gelu_grad(near).abs().argmin()]
    print(f"zero of gelu' at z = {float(zc):.4f}")
    assert abs(float(zc) - R.DCROSS) < 1e-3
    fine = torch.linspace(3.0, 8.0, 500001, dtype=R.F64)
    term = R.one_minus_s_term(fine)
    i = int(term.argmax())
    print(f"largest |xd| |1 - 2 s| ds = {float(term[i]):.3e} at z = {float(fine[i]):.4f} (xd = {float(R.xd_of(fine[i])):.1f}, "
          f"gelu' - 1 = {float(R.gelu_grad(fine[i]) - 1):.2e})")
    assert 4.9 < float(fine[i]) < 5.3 and 5e-6 < float(term[i]) < 8e-6


def test_the_selector_weights_select_and_the_regimes_are_exact():
    for Mx in (512, 1536, 2048):
        seen = torch.zeros(Mx)
        for p in range(R.n_phases(Mx)):
            S = R.selector_w2(Mx, p).double()
            for q in range(4):
                blk = S[R.quarter(Mx, q)]
                assert bool(((blk != 0).sum(0) == 1).all())                      # one live unit per (quarter, column)
            assert bool(((S != 0).sum(1) <= 1).all())
            seen += (S != 0).sum(1)
        assert bool((seen == 1).all())                                           # every unit live in exactly one phase
        W1, _ = R.selector_w1(Mx, torch.zeros(Mx, dtype=torch.int64), torch.zeros(Mx))
        assert bool(((W1 != 0).sum(0) == 1).all()) and bool(((W1 != 0).sum(1) == Mx // 128).all())
    for name in R.Z_REGIMES:
        pr = R.problem(name, ROWS, M)
        z = R.model(pr)["z"]
        lo, hi = float(z.min()), float(z.max())
        print(f"{name}: z in [{lo:.6g}, {hi:.6g}], {int(torch.unique(z).numel())} distinct values")
        want = dict(core=(-4.01, 4.01), zero=(-1e-6, 1e-6), dcross=(-0.77, -0.73), neg=(-12.02, -3.98), neg_sat=(-R.ZMAX, -20.0),
                    pos=(3.98, 8.02), pos_sat=(30.0, 200.0), mixed=(-R.ZMAX, 200.0))[name]
        assert want[0] <= lo and hi <= want[1]
        if name == "zero":
            assert bool((pr["a2"][0::4] == 0).all()) and bool((z[0::4] == 0).all()) and float(z.abs().max()) == 2.0 ** -20
        if name == "dcross":
            gz = R.gelu_grad(z)
            assert float(gz.min()) < 0 < float(gz.max())
        if name == "mixed":                                                     # neighbours in one packed pair, in tokens, in samples
            assert float((z[:, 0::2] != z[:, 1::2]).double().mean()) > 0.9 and float((z[:-1] != z[1:]).double().mean()) > 0.9
            assert float((z[:32] != z[32:64]).double().mean()) > 0.9


HOST_WORST = {}


def _judge(tag, name, got, ref, bound):
    r = R.worst_ratio(got, ref, bound)
    HOST_WORST[(tag, name)] = max(HOST_WORST.get((tag, name), 0.0), r)
    return r


@pytest.mark.parametrize("name", R.REGIMES)
def test_the_fp32_emulation_stays_inside_the_bound(name):
    base = R.problem(name, ROWS, M)
    for pr in [base] + [R.with_selector_w2(base, p) for p in range(R.n_phases(M))]:
        ref = R.model(pr)
        b = R.bounds(pr, ref)
        for desc in (False, True):
            em = R.emulate(pr, desc)
            assert bool(torch.isfinite(em["u"].float()).all()) and bool(torch.isfinite(em["dz"].float()).all())
            w = "dense" if pr["phase"] is None else "selector"
            rs = [_judge("u", name, em["u"], ref["u"], b["u"]), _judge("dz", name, em["dz"], ref["dz"], b["dz"])]
            for q in range(4):
                rs.append(_judge(f"fwd tile ({w} W2)", name, em["tiles"][q], ref["tiles"][q], b["tiles"][q]))
            val, bnd = R.da2_tiles_from_dz(em["dz"], pr["W1d"], M)
            rs.append(_judge("da2 tiles from dz", name, em["da2_tiles"], val, bnd))
            assert max(rs) <= 1.0, (name, pr["phase"], desc, rs)
            if pr["phase"] is not None and name != "random":                     # selector W1 and W2: z exact, a tile element is ONE unit
                z = ref["z"]
                assert torch.equal(em["z"].double(), z)
                if name == "neg_sat":
                    assert bool((em["u"].float() == 0).all()) and bool(torch.signbit(em["u"].float()).all()) and bool((em["dz"].float() == 0).all())
                if name == "pos_sat":
                    assert torch.equal(em["u"], R.bf(z)) and torch.equal(em["dz"], R.bf(ref["du"]))
    print(f"{name}: worst |err| / bound of the emulation: " + ", ".join(f"{k[0]} {v:.3f}" for k, v in sorted(HOST_WORST.items()) if k[1] == name))


# fault -> the (observable, regime, W2) combinations where it must leave the bound.  Observables: u, dz (bf16 [rows][M], the recompute
# backward's outputs and the fused kernel's save) and tiles (the four fp32 forward tiles, each judged on its own).
CAUGHT = {
    "b1-one-unit":               [("u", "random", "dense"), ("u", "core", "dense"), ("tiles", "core", "selector")],
    "units-swapped":             [("tiles", "core", "selector"), ("tiles", "mixed", "selector")],
    "b2-in-every-quarter":       [("tiles", "random", "dense"), ("tiles", "core", "selector")],
    "residual-missing":          [("tiles", "random", "dense"), ("tiles", "zero", "selector")],
    "last-chunk-into-next-tile": [("tiles", "random", "dense"), ("tiles", "pos", "selector")],
    "sample3-reads-sample0":     [("u", "random", "dense"), ("tiles", "mixed", "selector"), ("dz", "core", "dense")],
    "no-cubic-term":             [("u", "core", "dense"), ("u", "neg", "dense"), ("tiles", "core", "selector")],
    "grad-without-xd-term":      [("dz", "random", "dense"), ("dz", "dcross", "selector"), ("dz", "core", "dense")],
    "du-of-neighbour-token":     [("dz", "random", "dense"), ("dz", "pos_sat", "selector")],
}


@pytest.mark.parametrize("fault", R.FAULTS)
def test_every_planted_fault_leaves_the_bound(fault):
    assert set(CAUGHT) == set(R.FAULTS)
    seen = []
    for name in R.REGIMES:
        base = R.problem(name, ROWS, M)
        for w, pr in [("dense", base)] + [("selector", R.with_selector_w2(base, p)) for p in range(R.n_phases(M))]:
            ref = R.model(pr)
            b = R.bounds(pr, ref)
            ok, bad = R.model(pr, rounded=True), R.model(pr, fault, rounded=True)
            for obs in ("u", "dz", "tiles"):
                assert R.worst_ratio(ok[obs], ref[obs], b[obs]) <= 1.0                # the unplanted result passes
                r = R.worst_ratio(bad[obs], ref[obs], b[obs])
                if r > 1.0 and (obs, name, w) not in seen:
                    seen.append((obs, name, w))
    print(f"{fault}: leaves the bound in " + ", ".join(f"{o}/{n}/{w}" for o, n, w in seen))
    for want in CAUGHT[fault]:
        assert want in seen, (fault, want)
    if fault == "last-chunk-into-next-tile":                                     # the sum of the tiles cannot see it
        pr = R.problem("random", ROWS, M)
        assert R.rel(R.model(pr, fault)["h_out"], R.model(pr)["h_out"]) < 1e-12


def test_one_wrong_bias_passes_the_whole_matrix_thresholds_and_fails_the_bound():
    pr = dict(R.problem("random", ROWS, 2048))
    pr["b1_step"] = 0.1
    ref, bad = R.model(pr), R.model(pr, "b1-one-unit", rounded=True)
    b = R.bounds(pr, ref)
    h = pr["h"].double()
    old = dict(u=R.rel(bad["u"], ref["u"]), dz=R.rel(bad["dz"], ref["dz"]), h_out=R.rel(bad["h_out"] - h, ref["h_out"] - h))
    new = dict(u=R.worst_ratio(bad["u"], ref["u"], b["u"]), dz=R.worst_ratio(bad["dz"], ref["dz"], b["dz"]))
    print(f"b1[{R.FAULT_UNIT}] + 0.1 at M = 2048: whole-matrix rel {old}, worst |err| / bound {new}")
    assert old["u"] < R.OLD_U_REL and old["dz"] < R.OLD_DZ_REL and old["h_out"] < R.OLD_HOUT_REL
    assert new["u"] > 1.0 and new["dz"] > 1.0


@pytest.mark.parametrize("name", R.LN_REGIMES)
def test_layernorm_regimes_stay_inside_ln_fwd_bound(name):
    x = R.ln_rows(name, 96)
    g = torch.Generator().manual_seed(3)
    gamma, beta = 1 + 0.2 * torch.randn(128, generator=g), 0.1 * torch.randn(128, generator=g)
    want, e = R.ln_fwd_bound(x, gamma, beta)
    for flip in (False, True):                                                   # the statistics summed in two orders, in fp32
        xs = x.flip(-1) if flip else x
        s, s2 = torch.zeros(96), torch.zeros(96)
        for c in range(128):
            s, s2 = s + xs[:, c], s2 + xs[:, c] * xs[:, c]
        mean = (s * (1.0 / 128))[:, None]
        rstd = torch.rsqrt((s2 * (1.0 / 128))[:, None] - mean * mean + 1e-6)
        got = R.bf((x - mean) * rstd * gamma + beta)
        r = R.worst_ratio(got, want, e)
        print(f"LayerNorm regime {name}: worst |err| / bound {r:.3f}")
        assert r <= 1.0
    if name == "const":
        assert float(x[0::4].var(-1, unbiased=False).max()) == 0.0
    if name == "offset":
        assert float((x.mean(-1).abs() / x.std(-1)).min()) > 100
